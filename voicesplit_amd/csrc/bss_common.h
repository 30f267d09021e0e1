// Device code shared by sdr.hip (vs_sdr: one source) and bss_eval.hip (vs_bss_eval: K sources): the sliding-window
// correlation tile, the chunk fold, the symmetric Toeplitz Levinson recursion, the projection tile and the fixed-order
// block sum.  All fp64; the inputs are fp32, so every product is exact, and every sum runs in an order fixed by the
// signal length alone.
#pragma once
#include "vs_common.h"

namespace {

constexpr int kFlen = 512;
// correlation pass
constexpr int kCorrTile = 2048;                       // samples of n per tile
constexpr int kCorrStage = kCorrTile + kFlen + 16;    // + lags up to 511 + the window's read-ahead
constexpr int kCorrLds = kCorrStage + (kCorrStage >> 3) + 1;
constexpr int kSlot = 1032;                           // r[512], D[512], sum e^2, pad: doubles per partial
// projection pass
constexpr int kProjTile = 4096;                       // outputs of P per tile, 16 per lane
constexpr int kProjStage = kProjTile + kFlen;         // s[m0 - 512 .. m0 + 4096)
constexpr int kProjLds = kProjStage + (kProjStage >> 4) + 1;
constexpr int kMaxChunks = 1024;                      // chunks per row at most (longer rows: several tiles per workgroup)

constexpr int kMaxRows = 1 << 20;
constexpr long long kMaxLen = 1LL << 40;

// LDS index with one pad double every 8 (correlation: lanes 8 doubles apart -> 9) / every 16 (projection: 16 -> 17), so
// that the 32 lanes of a ds_read_b64 group hit 32 distinct bank pairs
__device__ __forceinline__ int pos8(int m) { return m + (m >> 3); }
__device__ __forceinline__ int pos16(int m) { return m + (m >> 4); }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// how a row of N samples is cut into tiles and chunks (a chunk = the tiles of one workgroup)
struct BssTiling {
  long long corr_tiles, corr_tpw, corr_chunks;
  long long proj_tiles, proj_tpw, proj_chunks;
};

inline BssTiling bss_tiling(long long N) {
  BssTiling L;
  L.corr_tiles = (N + kCorrTile - 1) / kCorrTile;
  L.corr_tpw = (L.corr_tiles + kMaxChunks - 1) / kMaxChunks;
  L.corr_chunks = (L.corr_tiles + L.corr_tpw - 1) / L.corr_tpw;
  const long long M = N + kFlen - 1;
  L.proj_tiles = (M + kProjTile - 1) / kProjTile;
  L.proj_tpw = (L.proj_tiles + kMaxChunks - 1) / kMaxChunks;
  L.proj_chunks = (L.proj_tiles + L.proj_tpw - 1) / L.proj_tpw;
  return L;
}

// fixed-order tree sum of v over the 256 threads of a workgroup; red: 256 doubles of LDS; result valid in thread 0
__device__ __forceinline__ double block_sum256(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);          // commutative pairs: every lane ends with the same bits
  return v;
}

// ---- correlation tile: a "left" signal slid against two "right" signals --------------------------------------------
// x[n0 .. n0 + kCorrStage) of one fp32 row as fp64 into X (zero past N); ee += the squares of the tile's own samples
__device__ __forceinline__ void corr_stage(const float* __restrict__ x, long long N, long long n0, double* X, double* ee) {
  for (int i = threadIdx.x; i < kCorrStage; i += 256) {
    const long long g = n0 + i;
    const double v = g < N ? (double)x[g] : 0.0;
    X[pos8(i)] = v;
    if (ee && i < kCorrTile) *ee += v * v;
  }
}

// One staged tile: ar[j] += sum_n L[n] A[n + k0 + j], ad[j] += sum_n L[n] Bv[n + k0 + j] over this wave's quarter of the tile,
// k0 = 8 * lane: each lane owns 8 consecutive lags in registers and slides an 8-sample window of A and Bv along n.
__device__ __forceinline__ void corr_slide(const double* L, const double* A, const double* Bv, int wave, int lane, double (&ar)[8],
                                           double (&ad)[8]) {
  const int nb0 = wave * (kCorrTile / 4);                               // this wave's quarter of the tile
  const int k0 = lane * 8;                                              // this lane's lags k0 .. k0 + 7
  double ws[8], we[8];                                                  // slot (m - nb0 - k0) & 7 holds A[m], Bv[m]
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ws[i] = A[pos8(nb0 + k0 + i)];
    we[i] = Bv[pos8(nb0 + k0 + i)];
  }
  for (int nb = 0; nb < kCorrTile / 4; nb += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int n = nb0 + nb + u;
      const double a = L[pos8(n)];                                      // broadcast
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ar[j] = fma(a, ws[(u + j) & 7], ar[j]);                         // l[n] a[n + k0 + j]
        ad[j] = fma(a, we[(u + j) & 7], ad[j]);                         // l[n] b[n + k0 + j]
      }
      ws[u] = A[pos8(n + k0 + 8)];                                      // slot u: a[n + k0] is done, a[n + k0 + 8] next
      we[u] = Bv[pos8(n + k0 + 8)];
    }
  }
}

// The 4 waves' partials summed in wave order into one slot: out[0..512) = ar, out[512..1024) = ad, out[1024] = sum of ee.
// red, red2: two staging arrays of at least 2048 doubles each, free again (the caller has passed a barrier after the last slide).
__device__ __forceinline__ void corr_store(const double (&ar)[8], const double (&ad)[8], double ee, double* red, double* red2,
                                           double* __restrict__ out) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = lane * 8 + j;
    if (wave < 2) {
      red[wave * 1024 + k] = ar[j];
      red[wave * 1024 + 512 + k] = ad[j];
    } else {
      red2[(wave - 2) * 1024 + k] = ar[j];
      red2[(wave - 2) * 1024 + 512 + k] = ad[j];
    }
  }
  __syncthreads();
  for (int o = tid; o < 1024; o += 256)
    out[o] = ((red[o] + red[1024 + o]) + red2[o]) + red2[1024 + o];
  const double tot = block_sum256(ee, red);
  if (tid == 0) out[1024] = tot;
}

// one workgroup: the chunk slots of one row summed in chunk order
__device__ __forceinline__ void corr_fold(const double* __restrict__ p, int chunks, double* __restrict__ rd) {
  for (int o = threadIdx.x; o < 1025; o += 256) {
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += p[(long long)c * kSlot + o];
    rd[o] = v;
  }
}

// ---- Levinson recursion, one wavefront ------------------------------------------------------------------------------
// G C = D, G symmetric Toeplitz with first row rsrc[0..512), D = dsrc[0..512): the forward predictor a (a[0] = 1,
// G_i a = E e_0) and the solution x grow one order per step; a reversed is the backward predictor, which extends x to the
// next order.  r, d, a, x: 512 doubles of LDS each.  Returns 0 with C in x, or 1 when a prediction error is <= 0 or not
// finite (uniform across the wave).  rsrc[0] must be > 0.
__device__ __forceinline__ int levinson512(const double* __restrict__ rsrc, const double* __restrict__ dsrc, double* r, double* d,
                                           double* a, double* x, int lane) {
  for (int j = lane; j < kFlen; j += 64) {
    r[j] = rsrc[j];
    d[j] = dsrc[j];
    a[j] = 0.0;
    x[j] = 0.0;
  }
  const double r0 = rsrc[0];
  __syncthreads();
  if (lane == 0) {
    a[0] = 1.0;
    x[0] = d[0] / r0;
  }
  __syncthreads();
  double Err = r0;
  for (int i = 1; i < kFlen; ++i) {
    double pa = 0.0, px = 0.0;
    for (int j = lane; j < i; j += 64) {
      const double rr = r[i - j];
      pa = fma(a[j], rr, pa);
      px = fma(x[j], rr, px);
    }
    pa = wave_sum(pa);
    px = wave_sum(px);
    const double k = -pa / Err;
    double t[kFlen / 64];
#pragma unroll
    for (int m = 0; m < kFlen / 64; ++m) {
      const int j = lane + 64 * m;
      if (j <= i) t[m] = fma(k, a[i - j], a[j]);
    }
    __builtin_amdgcn_wave_barrier();                                    // every lane has read a before any lane writes it
#pragma unroll
    for (int m = 0; m < kFlen / 64; ++m) {
      const int j = lane + 64 * m;
      if (j <= i) a[j] = t[m];
    }
    __builtin_amdgcn_wave_barrier();
    Err = Err * (1.0 - k * k);
    if (!(Err > 0.0) || !isfinite(Err)) return 1;                       // uniform across the wave
    const double mu = (d[i] - px) / Err;
#pragma unroll
    for (int m = 0; m < kFlen / 64; ++m) {
      const int j = lane + 64 * m;
      if (j <= i) x[j] = fma(mu, a[i - j], x[j]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  return 0;
}

// ---- projection tile: 4096 outputs of a 512-tap filter, 16 per lane ------------------------------------------------
// local q <-> s[m0 - 512 + q] of one fp32 row as fp64 (zero outside [0, N))
__device__ __forceinline__ void proj_stage(const float* __restrict__ s, long long N, long long m0, double* S) {
  for (int i = threadIdx.x; i < kProjStage; i += 256) {
    const long long g = m0 - kFlen + i;
    S[pos16(i)] = (g >= 0 && g < N) ? (double)s[g] : 0.0;
  }
}

// acc[i] += sum_k Cl[k] s[m - k] for this lane's outputs m = m0 + 16 tid + i, against a sliding 16-sample window of S
__device__ __forceinline__ void proj_filter(const double* S, const double* Cl, double (&acc)[16]) {
  const int q0 = kFlen + threadIdx.x * 16;                              // this lane's outputs: local q0 + i
  double w[16];                                                         // slot (q - q0) & 15 holds s at local q
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = S[pos16(q0 + i)];
  for (int kb = 0; kb < kFlen; kb += 16) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int k = kb + u;
      const double c = Cl[k];                                           // broadcast
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fma(c, w[(i - u) & 15], acc[i]);      // C[k] s[m - k]
      w[(15 - u) & 15] = S[pos16(q0 - k - 1)];                          // s[q0 + 15 - k] is done, s[q0 - k - 1] next
    }
  }
}

}  // namespace
