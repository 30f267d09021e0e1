// The FFT form of the per-row FIR: uniformly partitioned overlap-save convolution in fp32 with kept filter spectra.  The contract is the
// text in include/voicesplit_hip.h (vs_fir_spectra / vs_fir_rows_fft); tests/fir_fft_ref.py restates it.  Bk = VS_FIR_FFT_BLOCK = 2048,
// N = 2 Bk; a real transform of N samples runs as ONE 2048-point complex FFT in LDS (fir_fft_core.h: three radix-8 passes and a radix-4
// pass, 17 KB with its padding) and a split step; a spectrum is kept packed, 2048 complex values (bin 0 carries bins 0 and Bk).
//
//   twiddle_kernel   T[i] = exp(-2 pi i / 4096): cospi / sinpi in fp64 on the exact argument i / 2048, rounded once to fp32.
//   spectra_kernel   grid (Pmax, R): block (p, r) transforms taps [p Bk, (p + 1) Bk) of response r (taps at or behind nh read as zero
//                    whatever the row holds); blocks with p >= P[r] = ceil(nh / Bk) leave their slot unwritten: it is never read.
//   window_kernel    grid (J + Pmax - 1, B): block (w, b) transforms window q = w - (Pmax - 1) of row b, x(at + (q - 1) Bk .. at + (q + 1) Bk).
//                    Windows no output block of the row needs (q < -(P - 1)) and windows wholly below lo (all zero: their products
//                    would add exact zeros to sums that start at +0, which changes no bit) are neither made nor read.
//   block_kernel     grid (J, B): block (j, b) forms Y[k] = sum_p H_p[k] X_{j-p}[k], p ascending from zero, thread per bin (8 bins a
//                    thread, fmaf chains in one fixed order), unpacks, transforms back and writes the last Bk samples times 2^-14.
// The sum over p is formed inside the inverse launch: a block reads P window spectra and P filter spectra of 16 KB each.  Sliding over j
// with the P filter values of a bin in registers would read each once per row; NOT BUILT: the filter spectra of a response are shared
// by every block of every row that uses it and stay in L2, and at P = 16 the reads are 12 MB per row of 48000 samples.
// Validity is every block's own test of (at, lo, hrow): no launch of its own; block (0, b) of window_kernel writes valid[b].
// Registers, LDS, spills (-Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md 6.8m.
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "fir_fft_core.h"
#include "vs_internal.h"

namespace {

using vs_fft::cf;
constexpr int kBk = VS_FIR_FFT_BLOCK;
constexpr int kMaxTapsFft = 32768;
constexpr int kThreads = vs_fft::kThreads;
constexpr size_t kSpecBytes = (size_t)kBk * sizeof(cf);  // one packed spectrum
static_assert(kBk == vs_fft::kM && kBk == 8 * kThreads, "a thread owns eight bins");

// the blob: T [4096] | P [R] int32 | spectra [R][Pmax][2048] cf
struct Blob { size_t cnt, spec, total; int Pmax; };
inline Blob blob_layout(int R, int H) {
  Blob L;
  L.Pmax = (H + kBk - 1) / kBk;
  L.cnt = align_up(vs_fft::kTable * sizeof(cf));
  L.spec = L.cnt + align_up((size_t)R * sizeof(int));
  L.total = L.spec + (size_t)R * L.Pmax * kSpecBytes;
  return L;
}

__global__ void __launch_bounds__(kThreads) twiddle_kernel(cf* __restrict__ T) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const double a = (double)i / 2048.0;                                               // exact
  T[i] = {(float)cospi(a), (float)-sinpi(a)};
}

// the 2048-point transform of buf (natural order in and out); every thread of the workgroup calls it; the caller's stores are behind a
// barrier on entry, and the result is behind one on return
__device__ __forceinline__ void fft2048(cf* buf, const cf* __restrict__ T, int tid) {
  cf v[8];
#pragma unroll
  for (int Ns = 1; Ns < 512; Ns *= 8) {
    __syncthreads();
    vs_fft::pass8_load(buf, T, tid, Ns, v);
    __syncthreads();
    vs_fft::pass8_store(buf, tid, Ns, v);
  }
  __syncthreads();
  vs_fft::pass4(buf, T, tid);
  vs_fft::pass4(buf, T, tid + kThreads);
  __syncthreads();
}

// packed spectrum of what buf holds (z[m] = (x[2 m], x[2 m + 1])) -> out[2048]
__device__ __forceinline__ void forward_to(cf* buf, const cf* __restrict__ T, int tid, cf* __restrict__ out) {
  fft2048(buf, T, tid);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = tid + kThreads * r;
    out[k] = vs_fft::pack_bin(buf[vs_fft::phys(k)], buf[vs_fft::phys((kBk - k) & (kBk - 1))], T[k], k);
  }
}

__global__ void __launch_bounds__(kThreads) spectra_kernel(const float* __restrict__ h, const int* __restrict__ nh, int H, int Pmax,
                                                           const cf* __restrict__ T, int* __restrict__ cnt, cf* __restrict__ spec) {
  __shared__ cf buf[vs_fft::kBuf];
  const int p = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  int n = nh[r];
  n = n < 1 ? 1 : (n > H ? H : n);                                                   // the host checked nh_host; a table that is not its copy stays inside the row
  const int P = (n + kBk - 1) / kBk;
  if (p == 0 && tid == 0) cnt[r] = P;
  if (p >= P) return;                                                                // (uniform)
  const float* __restrict__ hp = h + (size_t)r * H;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int m = tid + kThreads * u, k = p * kBk + 2 * m;
    buf[vs_fft::phys(m)] = {m < kBk / 2 && k < n ? hp[k] : 0.f, m < kBk / 2 && k + 1 < n ? hp[k + 1] : 0.f};
  }
  forward_to(buf, T, tid, spec + ((size_t)r * Pmax + p) * kBk);
}

struct RowsJob {
  const float* samples;
  long long total;
  const long long* at;
  const long long* lo;
  const int* hrow;
  const cf* T;
  const int* cnt;
  const cf* spec;
  cf* win;                                                 // [B][W][2048]
  float* y;
  int* valid;
  int L, R, Pmax, W;
};

struct Row { bool ok; long long at, lo; int r, P, qlow; };

// the row's own numbers, the same in every block of both launches
__device__ __forceinline__ Row row_of(const RowsJob& j, int b) {
  Row w;
  w.at = j.at[b];
  w.lo = j.lo[b];
  w.r = j.hrow[b];
  w.ok = w.lo >= 0 && w.lo <= w.at && w.at <= j.total - j.L && w.r >= 0 && w.r < j.R;
  w.P = 0;
  w.qlow = 0;
  if (w.ok) {
    const int P = j.cnt[w.r];
    w.P = P < 1 ? 1 : (P > j.Pmax ? j.Pmax : P);                                     // a blob that vs_fir_spectra did not fill stays inside the workspace
    // the first window that holds a sample: window q ends at at + (q + 1) Bk > lo  <=>  q >= -ceil((at - lo) / Bk)
    const long long back = (w.at - w.lo + kBk - 1) / kBk;
    w.qlow = back >= w.P - 1 ? -(w.P - 1) : -(int)back;
  }
  return w;
}

__global__ void __launch_bounds__(kThreads) window_kernel(const RowsJob j) {
  __shared__ cf buf[vs_fft::kBuf];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Row w = row_of(j, b);
  if (blockIdx.x == 0 && tid == 0) j.valid[b] = w.ok ? 1 : -1;
  const int q = (int)blockIdx.x - (j.Pmax - 1);
  if (!w.ok || q < w.qlow) return;                                                   // (uniform)
  const long long rel0 = (long long)(q - 1) * kBk;                                   // from `at`
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int m = tid + kThreads * u;
    const long long rel = rel0 + 2 * m, p = w.at + rel;
    buf[vs_fft::phys(m)] = {(p >= w.lo && rel < j.L) ? j.samples[p] : 0.f, (p + 1 >= w.lo && rel + 1 < j.L) ? j.samples[p + 1] : 0.f};
  }
  forward_to(buf, j.T, tid, j.win + ((size_t)b * j.W + blockIdx.x) * kBk);
}

__global__ void __launch_bounds__(kThreads) block_kernel(const RowsJob j) {
  __shared__ cf buf[vs_fft::kBuf];
  const int jb = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, L = j.L;
  float* __restrict__ y = j.y + (size_t)b * L + (size_t)jb * kBk;
  const int left = L - jb * kBk;                                                     // outputs of this block: min(left, Bk)
  const Row w = row_of(j, b);
  if (!w.ok) {                                                                       // (uniform)
    for (int i = tid; i < kBk && i < left; i += kThreads) y[i] = 0.f;
    return;
  }
  const int pe = jb - w.qlow + 1 < w.P ? jb - w.qlow + 1 : w.P;                      // partitions whose window exists: p <= jb - qlow
  const cf* __restrict__ H = j.spec + (size_t)w.r * j.Pmax * kBk;
  const cf* __restrict__ X = j.win + ((size_t)b * j.W + jb + j.Pmax - 1) * kBk;       // window jb; window jb - p lies p slots in front
  cf acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = {0.f, 0.f};
  for (int p = 0; p < pe; ++p) {
    const cf* __restrict__ hp = H + (size_t)p * kBk;
    const cf* __restrict__ xp = X - (size_t)p * kBk;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int k = tid + kThreads * r;
      const cf hv = hp[k], xv = xp[k];
      if (k == 0) {                                                                  // two real bins
        acc[r].x = fmaf(hv.x, xv.x, acc[r].x);
        acc[r].y = fmaf(hv.y, xv.y, acc[r].y);
      } else {
        acc[r].x = fmaf(-hv.y, xv.y, fmaf(hv.x, xv.x, acc[r].x));
        acc[r].y = fmaf(hv.y, xv.x, fmaf(hv.x, xv.y, acc[r].y));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[vs_fft::phys(tid + kThreads * r)] = acc[r];
  __syncthreads();
  cf z[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = tid + kThreads * r;
    z[r] = vs_fft::unpack_bin(acc[r], buf[vs_fft::phys((kBk - k) & (kBk - 1))], j.T[k], k);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[vs_fft::phys(tid + kThreads * r)] = z[r];
  fft2048(buf, j.T, tid);
  const float s = 1.f / 16384.f;                                                     // 2^-14: exact
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int m = tid + kThreads * u, i = 2 * m;
    const cf v = buf[vs_fft::phys(kBk / 2 + m)];
    if (i < left) y[i] = v.x * s;
    if (i + 1 < left) y[i + 1] = -v.y * s;
  }
}

inline int blocks_of(int L) { return (L + kBk - 1) / kBk; }

}  // namespace

size_t vs_fir_spectra_bytes(int R, int H) {
  if (R < 1 || H < 1 || H > kMaxTapsFft) {
    vs_set_error("fir_spectra_bytes: h is [R=%d][H=%d] (R >= 1, 1 <= H <= %d)", R, H, kMaxTapsFft);
    return 0;
  }
  return blob_layout(R, H).total;
}

int vs_fir_spectra(const float* h, const int* nh_host, const int* nh, int R, int H, void* spectra, size_t spectra_bytes, void* stream_) {
  VS_REQUIRE(R >= 1 && R <= 65535, "fir_spectra: R=%d responses (1 .. 65535)", R);
  VS_REQUIRE(H >= 1 && H <= kMaxTapsFft, "fir_spectra: H=%d taps per row (1 .. %d)", H, kMaxTapsFft);
  VS_REQUIRE(h && nh_host && nh && spectra, "fir_spectra: NULL argument");
  const Blob bl = blob_layout(R, H);
  VS_REQUIRE(spectra_bytes >= bl.total, "fir_spectra: the blob holds %zu bytes, [R=%d][H=%d] needs %zu (vs_fir_spectra_bytes)", spectra_bytes,
             R, H, bl.total);
  for (int r = 0; r < R; ++r)
    VS_REQUIRE(nh_host[r] >= 1 && nh_host[r] <= H, "fir_spectra: response %d has nh = %d (1 .. H = %d)", r, nh_host[r], H);
  hipStream_t stream = (hipStream_t)stream_;
  cf* T = at<cf>(spectra, 0);
  hipLaunchKernelGGL(twiddle_kernel, dim3(vs_fft::kTable / kThreads), dim3(kThreads), 0, stream, T);
  hipLaunchKernelGGL(spectra_kernel, dim3((unsigned)bl.Pmax, (unsigned)R), dim3(kThreads), 0, stream, h, nh, H, bl.Pmax, T,
                     at<int>(spectra, bl.cnt), at<cf>(spectra, bl.spec));
  VS_LAUNCH_CHECK();
  return 0;
}

size_t vs_fir_fft_workspace_bytes(int B, int L, int H) {
  if (B < 1 || B > 65535 || L < 1 || L > (1 << 24) || H < 1 || H > kMaxTapsFft) {
    vs_set_error("fir_fft_workspace_bytes: B=%d rows (1 .. 65535), L=%d outputs (1 .. 2^24), H=%d taps (1 .. %d)", B, L, H, kMaxTapsFft);
    return 0;
  }
  return (size_t)B * (blocks_of(L) + (H + kBk - 1) / kBk - 1) * kSpecBytes;
}

int vs_fir_rows_fft(const float* samples, long long total, const long long* at_, const long long* lo, const int* hrow, int B, int L,
                    const void* spectra, size_t spectra_bytes, int R, int H, void* workspace, size_t workspace_bytes, float* y, int* valid,
                    void* stream_) {
  VS_REQUIRE(B > 0 && B <= 65535, "fir_rows_fft: B=%d rows (1 .. 65535)", B);
  VS_REQUIRE(L > 0 && L <= (1 << 24), "fir_rows_fft: L=%d outputs per row (1 .. 2^24)", L);
  VS_REQUIRE(R >= 1 && H >= 1 && H <= kMaxTapsFft, "fir_rows_fft: the spectra are of h [R=%d][H=%d] (R >= 1, 1 <= H <= %d)", R, H, kMaxTapsFft);
  VS_REQUIRE(total >= L, "fir_rows_fft: L=%d outputs from a buffer of %lld samples", L, total);
  VS_REQUIRE(samples && at_ && lo && hrow && spectra && workspace && y && valid, "fir_rows_fft: NULL argument");
  const Blob bl = blob_layout(R, H);
  VS_REQUIRE(spectra_bytes >= bl.total, "fir_rows_fft: the blob holds %zu bytes, [R=%d][H=%d] needs %zu (vs_fir_spectra_bytes)", spectra_bytes,
             R, H, bl.total);
  const size_t need = vs_fir_fft_workspace_bytes(B, L, H);
  VS_REQUIRE(workspace_bytes >= need, "fir_rows_fft: the workspace holds %zu bytes, B=%d L=%d H=%d needs %zu (vs_fir_fft_workspace_bytes)",
             workspace_bytes, B, L, H, need);
  hipStream_t stream = (hipStream_t)stream_;
  const int J = blocks_of(L), W = J + bl.Pmax - 1;
  RowsJob j = {samples, total, at_, lo, hrow, at<cf>(spectra, 0), at<int>(spectra, bl.cnt), at<cf>(spectra, bl.spec),
               static_cast<cf*>(workspace), y, valid, L, R, bl.Pmax, W};
  hipLaunchKernelGGL(window_kernel, dim3((unsigned)W, (unsigned)B), dim3(kThreads), 0, stream, j);
  hipLaunchKernelGGL(block_kernel, dim3((unsigned)J, (unsigned)B), dim3(kThreads), 0, stream, j);
  VS_LAUNCH_CHECK();
  return 0;
}
