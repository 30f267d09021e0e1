// Reverberation on the device: image-method room responses of a shoebox (Allen & Berkley 1979, RESTATED: not compared with a
// pyroomacoustics or rir-generator run), a batched FIR in which every row has its own filter of up to 8192 taps, and the fp64 energy
// of a row.  The contracts are the text in include/voicesplit_hip.h; tests/reverb_ref.py restates them in fp64.
//
//   rir_kernel        grid (tiles of 256 taps, R): a workgroup owns 256 taps of one response and walks ALL images of the response in
//                     the enumeration order (q, j, k, n, l, p), 256 at a time: thread e of a chunk forms image e's distance and delay
//                     (one sqrt per image and workgroup, not per tap), the images whose window (tau - 40, tau + 40) reaches the tile
//                     are compacted IN ORDER into LDS (wave ballots + the four wave counts), and every thread then adds the survivors
//                     to its own tap in that order.  An image that is skipped would have added exactly 0.0, so the bits of a tap are
//                     those of the full ordered sum: a function of the descriptor alone.  No atomics.  One sinpi per image: with
//                     ti = rint(tau), sin(pi (t - tau)) = -(-1)^(t - ti) sinpi(tau - ti).
//   fir_prep_kernel   grid B: the row's validity, max |x| over the samples the row reads and max |h| over its taps (maxima: order
//                     free), the two power-of-two scales of the split-f16 arm.
//   fir_fp32_kernel   VS_MATH_FP32: grid (tiles of 1024 outputs, B), 4 outputs per thread, h and x staged through LDS in segments of
//                     1024 taps; ONE fmaf chain per output in ascending k, acc = fmaf(h[k], x(at + i - k), acc) from acc = 0, which
//                     ends at k = nh - 1 (h = {1.0f} returns x bit for bit).
//   fir_f16x3_kernel  VS_MATH_F16X3: grid (tiles of 4096 outputs, B), four waves, a wave owns 32 x 32 outputs (rows a = blocks of
//                     P = 32 outputs, columns i = position in the block) and two fp32 accumulator tiles.  With X[e][j] = x(at + 32 e + j)
//                     and G_c[j][i] = h[32 c + i - j] (0 outside [0, nh)):  Out[a][i] = sum_c sum_j X[a - c][j] G_c[j][i]: a GEMM with
//                     no structural zeros, K = nh + 32.  Both operands are scaled by a power of two and split into f16 hi + lo planes
//                     in LDS, in segments of 32 tap blocks (1024 taps):
//                       x planes  samples in front of max(lo, at - nh + 1) are staged as zeros: the scale sx is taken over the samples
//                                 the sum reads, and the zero taps behind nh of the last tap block must not meet anything else;
//                                 [160 rows][32 halves], row stride 40 halves (80 B: sixteen consecutive rows start in sixteen different
//                                 groups of four banks), staged relative to `at`, so the A fragment of lane (r, hh) at k step s -- row
//                                 a - c, halves 16 s + 8 hh .. + 7 -- is ONE aligned ds_read_b128 whatever the alignment of `at`;
//                       h planes  the segment's taps REVERSED (rev[m] = h[1024 g + 1056 - m]), so that the B fragment of column i --
//                                 G_c[16 s + 8 hh + jj][i], jj = 0 .. 7 = rev[1056 - 32 c - i + 16 s + 8 hh + jj] -- is 8 consecutive
//                                 halves; its start is congruent to -i mod 8, so EIGHT copies are kept, copy v shifted by v elements
//                                 (copy_v[e] = rev[e + v]), and lane i reads copy (-i) mod 8 at a multiple of 8: again one aligned
//                                 ds_read_b128, never a ds_read_u16.  8 x 1096 halves x 2 planes = 35 KB; with the x planes 60.7 KB.
//                     Products per k step, in this order: accL += xh hl, accL += xl hh, accH += xh hh (v_mfma_f32_32x32x16_f16, fp32
//                     accumulation; the lo x lo product is dropped).  The small products have an accumulator of their own, so the long
//                     chain of accH carries nh + 32 additions, not three times as many.  y = (accH + accL) / (sx sh).
//                     K is walked c = 0, 1, .. (s = 0, 1 inside) from zero accumulators for every output: the order depends on neither B,
//                     the row index nor the tile; tap blocks behind the filter's end are left out (they would add zeros).  A row's
//                     bits depend on its own samples and its own filter alone (not even on at mod 8: the planes are staged from `at`).
//   row_energy_kernel one workgroup per row: thread t adds y[t], y[t + 256], .. squared in fp64 in ascending order, then a fixed
//                     binary fold of the 256 partial sums in LDS.  No atomics.
// KNOWN, NOT TUNED: the global loads of the staging are 4 bytes per lane (a row starts at any sample); every element of a segment of
// h is written to its eight copies with 2-byte LDS stores; a wave whose 1024 outputs lie behind L idles through the barriers; the
// B-fragment reads of a half wave touch 128 banks' worth of data, so they take two passes at the least.
#include <math.h>
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

namespace {

constexpr int kMaxTaps = 8192;
constexpr int kHalfWin = 40;                             // w(u) = 0 for |u| >= 40
constexpr int kRirTile = 256;
constexpr long long kMaxImages = 1LL << 24;

// |n| <= N[0], |l| <= N[1], |p| <= N[2]: |R_x| >= 2 L_x (|n| - 1) for source and receiver inside the room, and an image further than
// (nh + 40) c / fs adds nothing; an order limit m keeps |2 n - q| <= m, so |n| <= (m + 1) / 2
__host__ __device__ inline void image_bounds(const vs_room& r, int* N) {
  const double dmax = ((double)r.nh + kHalfWin) * r.c / r.fs;
  for (int d = 0; d < 3; ++d) {
    double n = floor(dmax / (2.0 * r.size[d])) + 1.0;
    if (!(n < 1e6)) n = 1e6;
    if (r.max_order >= 0 && n > (double)((r.max_order + 1) / 2)) n = (double)((r.max_order + 1) / 2);
    N[d] = (int)n;
  }
}

struct Hit { double tau, s0, amp; };

__global__ void __launch_bounds__(kRirTile) rir_kernel(const vs_room* __restrict__ rooms, int H, float* __restrict__ h) {
  __shared__ Hit hits[kRirTile];
  __shared__ int wcnt[kRirTile / 64];
  const vs_room rm = rooms[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * kRirTile, t = t0 + tid;
  if (t0 >= rm.nh || rm.nh > H) return;                                              // (uniform) the row behind nh was cleared by the host's memset
  int N[3];
  image_bounds(rm, N);
  const int ny = 2 * N[1] + 1, nz = 2 * N[2] + 1;
  const long long per = (long long)(2 * N[0] + 1) * ny * nz, total = 8 * per;
  // the host checked rooms_host; a device table that is not its copy must not turn into an endless walk: its row stays zero
  if (!(per > 0 && total <= kMaxImages)) return;                                     // (uniform)
  const double tlo = (double)(t0 - kHalfWin), thi = (double)(t0 + kRirTile - 1 + kHalfWin);
  double acc = 0.0;
  for (long long e0 = 0; e0 < total; e0 += kRirTile) {
    const long long e = e0 + tid;
    bool hit = false;
    Hit me = {0.0, 0.0, 0.0};
    if (e < total) {
      const int par = (int)(e / per);
      long long rem = e - par * per;
      const int p = (int)(rem % nz) - N[2];
      rem /= nz;
      const int l = (int)(rem % ny) - N[1];
      const int n = (int)(rem / ny) - N[0];
      const int q = (par >> 2) & 1, jj = (par >> 1) & 1, k = par & 1;
      const bool in_order = rm.max_order < 0 || abs(2 * n - q) + abs(2 * l - jj) + abs(2 * p - k) <= rm.max_order;
      const double Rx = (double)(1 - 2 * q) * rm.src[0] - rm.mic[0] + 2.0 * n * rm.size[0];
      const double Ry = (double)(1 - 2 * jj) * rm.src[1] - rm.mic[1] + 2.0 * l * rm.size[1];
      const double Rz = (double)(1 - 2 * k) * rm.src[2] - rm.mic[2] + 2.0 * p * rm.size[2];
      const double d = sqrt((Rx * Rx + Ry * Ry) + Rz * Rz);
      const double tau = d * rm.fs / rm.c;
      if (in_order && tau > tlo && tau < thi) {
        hit = true;
        double a = pow(rm.beta[0], (double)abs(n - q)) * pow(rm.beta[1], (double)abs(n));
        a = a * pow(rm.beta[2], (double)abs(l - jj));
        a = a * pow(rm.beta[3], (double)abs(l));
        a = a * pow(rm.beta[4], (double)abs(p - k));
        a = a * pow(rm.beta[5], (double)abs(p));
        me.amp = a / (4.0 * M_PI * d);
        me.tau = tau;
        me.s0 = sinpi(tau - rint(tau));
      }
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, cnt = 0;
#pragma unroll
    for (int w = 0; w < kRirTile / 64; ++w) {
      if (w < wave) base += wcnt[w];
      cnt += wcnt[w];
    }
    if (hit) hits[base + __popcll(mask & ((1ULL << lane) - 1ULL))] = me;
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const Hit x = hits[i];
      const double ti = rint(x.tau);
      const double dt = (double)t - ti;                                              // an integer
      const double u = dt - (x.tau - ti);
      if (fabs(u) < (double)kHalfWin) {
        const double sn = ((long long)dt & 1) ? x.s0 : -x.s0;                          // sin(pi u) = -(-1)^dt sinpi(tau - ti)
        const double sinc = u == 0.0 ? 1.0 : sn / (M_PI * u);
        const double win = 0.5 * (1.0 + cos(M_PI * u / (double)kHalfWin));
        acc += x.amp * (sinc * win);
      }
    }
  }
  if (t < rm.nh) h[(long long)blockIdx.y * H + t] = (float)acc;
}

// ---- the FIR ---------------------------------------------------------------------------------------------------------------------------
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

constexpr int kP = 32;                                   // outputs per GEMM row
constexpr int kSegBlocks = 32, kSegTaps = kSegBlocks * kP;
constexpr int kTileRows = 128, kTileOut = kTileRows * kP; // 4 waves x 32 rows x 32 outputs
constexpr int kXRows = kTileRows + kSegBlocks, kXStride = 40;
constexpr int kCopyLen = kSegTaps + 72;                  // 1096 halves: 16-byte multiples, and 548 dwords = 36 mod 64 banks from copy to copy
constexpr int kRevTop = kSegTaps + kP;                   // rev[m] = h[1024 g + 1056 - m]
constexpr int kF32Tile = 1024, kF32Seg = 1024;

struct FirJob {
  const float* samples;
  const long long* at;
  const long long* lo;
  const int* nh;
  const int* hrow;
  const float* h;
  float* y;
  const int* valid;
  const float* scale;                                    // [B][4] = sx, 1 / sx, sh, 1 / sh
  int L, H;
};

// 2^e with 2^14 <= m 2^e < 2^15 (f16 holds up to 65504), e clamped to +-100; 1 for m = 0
__device__ __forceinline__ void pow2_scale(float m, float* s) {
  int E = 0;
  if (m > 0.f) frexpf(m, &E);
  int e = m > 0.f ? 15 - E : 0;
  e = e > 100 ? 100 : (e < -100 ? -100 : e);
  s[0] = ldexpf(1.f, e);
  s[1] = ldexpf(1.f, -e);
}

__global__ void __launch_bounds__(256) fir_prep_kernel(const float* __restrict__ samples, long long total, const long long* __restrict__ at,
                                                       const long long* __restrict__ lo, const int* __restrict__ nh,
                                                       const int* __restrict__ hrow, const float* __restrict__ h, int R, int H, int L,
                                                       int* __restrict__ valid, float* __restrict__ scale) {
  __shared__ float red[2][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long a = at[b], l = lo[b];
  const int n = nh[b], r = hrow[b];
  const bool ok = l >= 0 && l <= a && a <= total - L && r >= 0 && r < R && n >= 1 && n <= H;
  if (!ok) {                                                                         // (uniform) nothing of the row is read
    if (tid == 0) {
      valid[b] = -1;
      scale[4 * b] = scale[4 * b + 1] = scale[4 * b + 2] = scale[4 * b + 3] = 1.f;
    }
    return;
  }
  const long long first = a - (n - 1) > l ? a - (n - 1) : l;
  float mx = 0.f, mh = 0.f;
  for (long long p = first + tid; p < a + L; p += 256) mx = fmaxf(mx, fabsf(samples[p]));
  const float* __restrict__ hp = h + (long long)r * H;
  for (int k = tid; k < n; k += 256) mh = fmaxf(mh, fabsf(hp[k]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    mh = fmaxf(mh, __shfl_xor(mh, d, 64));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = mx;
    red[1][tid >> 6] = mh;
  }
  __syncthreads();
  if (tid == 0) {
    mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    mh = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    valid[b] = 1;
    pow2_scale(mx, scale + 4 * b);
    pow2_scale(mh, scale + 4 * b + 2);
  }
}

__device__ __forceinline__ void zero_tile(float* __restrict__ y, int n0, int count, int L) {
  for (int i = threadIdx.x; i < count && n0 + i < L; i += blockDim.x) y[n0 + i] = 0.f;
}

__global__ void __launch_bounds__(256) fir_fp32_kernel(const FirJob j) {
  __shared__ float hs[kF32Seg];
  __shared__ float xs[kF32Seg + kF32Tile];
  const int b = blockIdx.y, tid = threadIdx.x, L = j.L;
  const int n0 = blockIdx.x * kF32Tile;
  float* __restrict__ y = j.y + (long long)b * L;
  if (j.valid[b] != 1) {                                                             // (uniform)
    zero_tile(y, n0, kF32Tile, L);
    return;
  }
  const long long at = j.at[b], lo = j.lo[b];
  const int nh = j.nh[b];
  const float* __restrict__ hp = j.h + (long long)j.hrow[b] * j.H;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < nh; k0 += kF32Seg) {
    if (k0) __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + tid + 256 * u;
      hs[tid + 256 * u] = k < nh ? hp[k] : 0.f;
    }
    // xs[q] = x(at + n0 - k0 - 1023 + q): output n0 + il and tap k0 + kk meet at q = il - kk + 1023
    for (int q = tid; q < kF32Seg + kF32Tile - 1; q += 256) {
      const long long rel = (long long)n0 - k0 - (kF32Seg - 1) + q;
      const long long p = at + rel;
      xs[q] = (p >= lo && rel < L) ? j.samples[p] : 0.f;
    }
    __syncthreads();
    const int kn = nh - k0 < kF32Seg ? nh - k0 : kF32Seg;
    const float* __restrict__ xr = xs + tid + (kF32Seg - 1);
    for (int kk = 0; kk < kn; ++kk) {
      const float hk = hs[kk];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(hk, xr[256 * u - kk], acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = n0 + tid + 256 * u;
    if (n < L) y[n] = acc[u];
  }
}

__device__ __forceinline__ void split_f16(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}

__global__ void __launch_bounds__(256) fir_f16x3_kernel(const FirJob j) {
  __shared__ __attribute__((aligned(16))) _Float16 xs[2][kXRows * kXStride];
  __shared__ __attribute__((aligned(16))) _Float16 hs[2][8][kCopyLen];
  const int b = blockIdx.y, tid = threadIdx.x, L = j.L;
  const int lane = tid & 63, wave = tid >> 6, i = lane & 31, hh = lane >> 5;
  const int A0 = blockIdx.x * kTileRows;
  float* __restrict__ y = j.y + (long long)b * L;
  if (j.valid[b] != 1) {                                                             // (uniform)
    zero_tile(y, A0 * kP, kTileOut, L);
    return;
  }
  const int nh = j.nh[b];
  const long long at = j.at[b];
  // the first sample the row's sum reads: the last tap block runs past nh with zero taps, and a sample in front of the window, which
  // the scale sx does not cover, must not meet them as an f16 infinity
  const long long lo = j.lo[b] > at - (nh - 1) ? j.lo[b] : at - (nh - 1);
  const float* __restrict__ hp = j.h + (long long)j.hrow[b] * j.H;
  const float sx = j.scale[4 * b], isx = j.scale[4 * b + 1], sh = j.scale[4 * b + 2], ish = j.scale[4 * b + 3];
  const int nblk = (nh + kP - 2) / kP + 1;                                           // tap blocks c = 0 .. (nh - 1 + 31) / 32
  const int nseg = (nblk + kSegBlocks - 1) / kSegBlocks;
  const bool active = (A0 + 32 * wave) * kP < L;                                     // (wave-uniform)
  const int v = (8 - (i & 7)) & 7;                                                   // this lane's copy of the reversed taps
  f32x16 accH, accL;
#pragma unroll
  for (int r = 0; r < 16; ++r) accH[r] = accL[r] = 0.f;

  for (int g = 0; g < nseg; ++g) {
    if (g) __syncthreads();                                                          // the previous segment's fragments have been read
    for (int m = tid; m < kCopyLen + 8; m += 256) {                                  // rev[m] -> copy_c[m - c], c = 0 .. 7
      const int hidx = g * kSegTaps + kRevTop - m;
      const float val = (hidx >= 0 && hidx < nh) ? hp[hidx] * sh : 0.f;
      _Float16 vh, vl;
      split_f16(val, vh, vl);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int e = m - c;
        if (e >= 0 && e < kCopyLen) {
          hs[0][c][e] = vh;
          hs[1][c][e] = vl;
        }
      }
    }
    const int E0 = A0 - g * kSegBlocks - (kSegBlocks - 1);                            // row of X in LDS row 0
    for (int qd = tid; qd < kXRows * (kP / 4); qd += 256) {
      const int row = qd >> 3, j4 = (qd & 7) * 4;
      const long long rel = (long long)(E0 + row) * kP + j4;                         // from `at`; negative in the history
      h4 ph, pl;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long p = at + rel + u;
        const float val = (p >= lo && rel + u < L) ? j.samples[p] * sx : 0.f;
        _Float16 vh, vl;
        split_f16(val, vh, vl);
        ph[u] = vh;
        pl[u] = vl;
      }
      *reinterpret_cast<h4*>(&xs[0][row * kXStride + j4]) = ph;
      *reinterpret_cast<h4*>(&xs[1][row * kXStride + j4]) = pl;
    }
    __syncthreads();
    if (active) {
      const int cmax = nblk - g * kSegBlocks < kSegBlocks ? nblk - g * kSegBlocks : kSegBlocks;
      for (int cl = 0; cl < cmax; ++cl) {
        const int arow = 32 * wave + i - cl + (kSegBlocks - 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int ao = arow * kXStride + 16 * s + 8 * hh;
          const int e0 = kRevTop - kP * cl - i + 16 * s + 8 * hh - v;                 // a multiple of 8 in [32, 1080]
          const h8 ah = *reinterpret_cast<const h8*>(&xs[0][ao]);
          const h8 al = *reinterpret_cast<const h8*>(&xs[1][ao]);
          const h8 bh = *reinterpret_cast<const h8*>(&hs[0][v][e0]);
          const h8 bl = *reinterpret_cast<const h8*>(&hs[1][v][e0]);
          accL = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, accL, 0, 0, 0);
          accL = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, accL, 0, 0, 0);
          accH = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, accH, 0, 0, 0);
        }
      }
    }
  }
  if (active) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
      const long long n = (long long)(A0 + 32 * wave + row) * kP + i;
      if (n < L) y[n] = ((accH[r] + accL[r]) * isx) * ish;
    }
  }
}

__global__ void __launch_bounds__(256) row_energy_kernel(const float* __restrict__ y, int L, double* __restrict__ energy) {
  __shared__ double part[256];
  const int tid = threadIdx.x;
  const float* __restrict__ row = y + (long long)blockIdx.x * L;
  double acc = 0.0;
  for (int i = tid; i < L; i += 256) {
    const double v = (double)row[i];
    acc += v * v;                                                                    // an fp32 square is exact in fp64
  }
  part[tid] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) part[tid] += part[tid + st];
    __syncthreads();
  }
  if (tid == 0) energy[blockIdx.x] = part[0];
}

int check_room(const vs_room& r, int k, int H) {
  for (int d = 0; d < 3; ++d) {
    VS_REQUIRE(isfinite(r.size[d]) && r.size[d] > 0.0, "rir_shoebox: room %d has size[%d] = %g (must be positive)", k, d, r.size[d]);
    VS_REQUIRE(r.src[d] > 0.0 && r.src[d] < r.size[d], "rir_shoebox: room %d: the source is outside the room (axis %d: %g of %g)", k, d,
               r.src[d], r.size[d]);
    VS_REQUIRE(r.mic[d] > 0.0 && r.mic[d] < r.size[d], "rir_shoebox: room %d: the receiver is outside the room (axis %d: %g of %g)", k, d,
               r.mic[d], r.size[d]);
  }
  for (int w = 0; w < 6; ++w)
    VS_REQUIRE(r.beta[w] >= -1.0 && r.beta[w] <= 1.0, "rir_shoebox: room %d: beta[%d] = %g is outside -1 .. 1", k, w, r.beta[w]);
  VS_REQUIRE(r.src[0] != r.mic[0] || r.src[1] != r.mic[1] || r.src[2] != r.mic[2],
             "rir_shoebox: room %d: source and receiver coincide (d = 0)", k);
  VS_REQUIRE(isfinite(r.c) && r.c > 0.0 && isfinite(r.fs) && r.fs > 0.0, "rir_shoebox: room %d: c = %g, fs = %g (must be positive)", k, r.c, r.fs);
  VS_REQUIRE(r.nh >= 1 && r.nh <= kMaxTaps && r.nh <= H, "rir_shoebox: room %d: nh = %d (1 .. min(%d, H = %d))", k, r.nh, kMaxTaps, H);
  VS_REQUIRE(r.max_order >= -1, "rir_shoebox: room %d: max_order = %d (-1 = no limit, or >= 0)", k, r.max_order);
  int N[3];
  image_bounds(r, N);
  const double images = 8.0 * (2.0 * N[0] + 1.0) * (2.0 * N[1] + 1.0) * (2.0 * N[2] + 1.0);
  VS_REQUIRE(images <= (double)kMaxImages, "rir_shoebox: room %d is too small for %d taps: %.0f images (at most %lld)", k, r.nh, images,
             kMaxImages);
  return 0;
}

}  // namespace

int vs_rir_shoebox(const vs_room* rooms_host, const vs_room* rooms, int R, int H, float* h, void* stream_) {
  VS_REQUIRE(R > 0 && R <= 65535, "rir_shoebox: R=%d responses (1 .. 65535)", R);
  VS_REQUIRE(H >= 1 && H <= kMaxTaps, "rir_shoebox: H=%d taps per row (1 .. %d)", H, kMaxTaps);
  VS_REQUIRE(rooms_host && rooms && h, "rir_shoebox: NULL argument");
  for (int k = 0; k < R; ++k)
    if (int rc = check_room(rooms_host[k], k, H)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  VS_CHECK_HIP(hipMemsetAsync(h, 0, (size_t)R * H * sizeof(float), stream));
  hipLaunchKernelGGL(rir_kernel, dim3((unsigned)((H + kRirTile - 1) / kRirTile), (unsigned)R), dim3(kRirTile), 0, stream, rooms, H, h);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_fir_rows(const float* samples, long long total, const long long* at, const long long* lo, const int* nh, const int* hrow, int B,
                int L, const float* h, int R, int H, int math, float* y, int* valid, float* scale, void* stream_) {
  VS_REQUIRE(math == VS_MATH_F16X3 || math == VS_MATH_FP32, "fir_rows: math=%d (VS_MATH_F16X3 or VS_MATH_FP32; no other arm is built)", math);
  VS_REQUIRE(B > 0 && B <= 65535, "fir_rows: B=%d rows (1 .. 65535)", B);
  VS_REQUIRE(L > 0 && L <= (1 << 24), "fir_rows: L=%d outputs per row (1 .. 2^24)", L);
  VS_REQUIRE(R > 0 && H >= 1 && H <= kMaxTaps, "fir_rows: h is [R=%d][H=%d] (R > 0, 1 <= H <= %d)", R, H, kMaxTaps);
  VS_REQUIRE(total >= L, "fir_rows: L=%d outputs from a buffer of %lld samples", L, total);
  VS_REQUIRE(samples && at && lo && nh && hrow && h && y && valid && scale, "fir_rows: NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(fir_prep_kernel, dim3((unsigned)B), dim3(256), 0, stream, samples, total, at, lo, nh, hrow, h, R, H, L, valid, scale);
  FirJob j = {samples, at, lo, nh, hrow, h, y, valid, scale, L, H};
  if (math == VS_MATH_FP32)
    hipLaunchKernelGGL(fir_fp32_kernel, dim3((unsigned)((L + kF32Tile - 1) / kF32Tile), (unsigned)B), dim3(256), 0, stream, j);
  else
    hipLaunchKernelGGL(fir_f16x3_kernel, dim3((unsigned)((L + kTileOut - 1) / kTileOut), (unsigned)B), dim3(256), 0, stream, j);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_row_energy(const float* y, int B, int L, double* energy, void* stream_) {
  VS_REQUIRE(B > 0 && B <= (1 << 24), "row_energy: B=%d rows (1 .. 2^24)", B);
  VS_REQUIRE(L > 0 && L <= (1 << 30), "row_energy: L=%d samples per row (1 .. 2^30)", L);
  VS_REQUIRE(y && energy, "row_energy: NULL argument");
  hipLaunchKernelGGL(row_energy_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream_, y, L, energy);
  VS_LAUNCH_CHECK();
  return 0;
}
