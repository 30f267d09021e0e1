// Single-source BSS-eval SDR (the number the reference's validation reports: utils/generic_utils.py:476-530,
// mir_eval.separation.bss_eval_sources(clean_wav, est_wav, False)[0][0]), batched over rows, all in fp64.
//
// For a reference s and an estimate e of N samples and the fixed distortion filter length L = 512:
//   r[k] = sum_n s[n] s[n+k],  D[k] = sum_n s[n] e[n+k],  k = 0..L-1      (G = Toeplitz(r): Gram matrix of s delayed 0..L-1)
//   C    = G^-1 D                                                          (symmetric Toeplitz Levinson recursion)
//   P    = s * C  (full convolution, N + L - 1 samples),  res = [e, 0] - P
//   SDR  = 10 log10(sum P^2 / sum res^2)   (+inf when sum res^2 == 0; with one source SIR is undefined and SDR = SAR)
// Inputs are fp32, so every product is exact in fp64; every sum runs in fp64 in an order fixed by N alone (no atomics):
// two calls give the same bits, and a row gives the same bits whether it is scored alone or inside a batch.
//
// Five launches on the caller's stream, no host synchronisation:
//   sdr_corr_kernel   grid (B, chunks): a workgroup stages 2048 samples (+ the 528-sample tail) of s and e in LDS as fp64;
//                     each lane owns 8 consecutive lags in registers and slides an 8-sample window of s and e along n;
//                     4 waves split the tile's n range and are summed in a fixed order; partial (r, D, sum e^2) -> slot
//   sdr_fold_kernel   one workgroup per row: the chunk slots summed in chunk order
//   sdr_levinson      one wavefront per row: 511 serial steps, both dot products of a step reduced with __shfl_xor
//   sdr_proj_kernel   grid (B, chunks): 4096 outputs of P per tile, 16 per lane against a sliding 16-sample window of s;
//                     partial (sum P^2, sum res^2) -> slot
//   sdr_final_kernel  per row: slots in chunk order -> SDR; status 1 (silent row) / 2 (solve failure) give NaN
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"
#include "bss_common.h"

namespace {

struct SdrLayout {
  long long corr_tiles, corr_tpw, corr_chunks;
  long long proj_tiles, proj_tpw, proj_chunks;
  size_t corr, rd, coef, proj, status, total;        // byte offsets into the workspace
};

SdrLayout sdr_layout(int B, long long N) {
  SdrLayout L;
  const BssTiling T = bss_tiling(N);
  L.corr_tiles = T.corr_tiles;  L.corr_tpw = T.corr_tpw;  L.corr_chunks = T.corr_chunks;
  L.proj_tiles = T.proj_tiles;  L.proj_tpw = T.proj_tpw;  L.proj_chunks = T.proj_chunks;
  size_t off = 0;
  L.corr = off;   off = align256(off + (size_t)B * L.corr_chunks * kSlot * sizeof(double));
  L.rd = off;     off = align256(off + (size_t)B * kSlot * sizeof(double));
  L.coef = off;   off = align256(off + (size_t)B * kFlen * sizeof(double));
  L.proj = off;   off = align256(off + (size_t)B * L.proj_chunks * 2 * sizeof(double));
  L.status = off; off = align256(off + (size_t)B * sizeof(int));
  L.total = off;
  return L;
}

__global__ void __launch_bounds__(256) sdr_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est, long long N,
                                                       long long tiles, long long tpw, double* __restrict__ part) {
  __shared__ double S[kCorrLds];
  __shared__ double E[kCorrLds];
  const int row = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const float* s = ref + (long long)row * N;
  const float* e = est + (long long)row * N;
  double ar[8], ad[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ar[j] = ad[j] = 0.0;
  double ee = 0.0;
  const long long t_end = min((long long)(chunk + 1) * tpw, tiles);
  for (long long t = (long long)chunk * tpw; t < t_end; ++t) {
    const long long n0 = t * kCorrTile;
    __syncthreads();                                                    // the previous tile's readers are done
    corr_stage(s, N, n0, S, nullptr);
    corr_stage(e, N, n0, E, &ee);
    __syncthreads();
    corr_slide(S, S, E, wave, lane, ar, ad);
  }
  // the 4 waves' partials, summed in wave order (the staging area is free again)
  __syncthreads();
  corr_store(ar, ad, ee, S, E, part + ((long long)row * gridDim.y + chunk) * kSlot);    // [4][1024] fits in S + E (2 x 2898 doubles)
}

__global__ void __launch_bounds__(256) sdr_fold_kernel(const double* __restrict__ part, int chunks, double* __restrict__ rd) {
  const int row = blockIdx.x;
  corr_fold(part + (long long)row * chunks * kSlot, chunks, rd + (long long)row * kSlot);
}

__global__ void __launch_bounds__(64) sdr_levinson(const double* __restrict__ rd, double* __restrict__ coef, int* __restrict__ status) {
  __shared__ double r[kFlen], d[kFlen], a[kFlen], x[kFlen];
  const int row = blockIdx.x, lane = threadIdx.x;
  const double* src = rd + (long long)row * kSlot;
  const double r0 = src[0], ee = src[1024];
  if (!(r0 > 0.0) || !(ee > 0.0)) {                                     // all-zero reference or estimate row
    if (lane == 0) status[row] = 1;
    return;
  }
  if (levinson512(src, src + kFlen, r, d, a, x, lane)) {
    if (lane == 0) status[row] = 2;
    return;
  }
  for (int j = lane; j < kFlen; j += 64) coef[(long long)row * kFlen + j] = x[j];
  if (lane == 0) status[row] = 0;
}

__global__ void __launch_bounds__(256) sdr_proj_kernel(const float* __restrict__ ref, const float* __restrict__ est, long long N,
                                                       long long tiles, long long tpw, const double* __restrict__ coef,
                                                       const int* __restrict__ status, double* __restrict__ part) {
  __shared__ double S[kProjLds];
  __shared__ double Cl[kFlen];
  const int row = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  double* out = part + ((long long)row * gridDim.y + chunk) * 2;
  if (status[row] != 0) {                                               // uniform: nothing to project
    if (tid == 0) out[0] = out[1] = 0.0;
    return;
  }
  const float* s = ref + (long long)row * N;
  const float* e = est + (long long)row * N;
  const long long M = N + kFlen - 1;
  for (int k = tid; k < kFlen; k += 256) Cl[k] = coef[(long long)row * kFlen + k];
  double pp = 0.0, rr = 0.0;
  const long long t_end = min((long long)(chunk + 1) * tpw, tiles);
  for (long long t = (long long)chunk * tpw; t < t_end; ++t) {
    const long long m0 = t * kProjTile;
    __syncthreads();
    proj_stage(s, N, m0, S);
    __syncthreads();
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    proj_filter(S, Cl, acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long m = m0 + tid * 16 + i;
      if (m < M) {
        const double ev = m < N ? (double)e[m] : 0.0;
        const double res = ev - acc[i];
        pp = fma(acc[i], acc[i], pp);
        rr = fma(res, res, rr);
      }
    }
  }
  const double tp = block_sum256(pp, S);
  const double tr = block_sum256(rr, S);
  if (tid == 0) {
    out[0] = tp;
    out[1] = tr;
  }
}

__global__ void __launch_bounds__(64) sdr_final_kernel(const double* __restrict__ part, int chunks, const int* __restrict__ st,
                                                       int B, double* __restrict__ sdr, int* __restrict__ status) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= B) return;
  const int s = st[row];
  status[row] = s;
  if (s != 0) {
    sdr[row] = __builtin_nan("");
    return;
  }
  double pp = 0.0, rr = 0.0;
  const double* p = part + (long long)row * chunks * 2;
  for (int c = 0; c < chunks; ++c) {
    pp += p[2 * c];
    rr += p[2 * c + 1];
  }
  sdr[row] = rr == 0.0 ? __builtin_inf() : 10.0 * log10(pp / rr);
}

}  // namespace

size_t vs_sdr_workspace_bytes(int B, long long N) {
  if (B <= 0 || B > kMaxRows || N <= 0 || N > kMaxLen) return 0;
  return sdr_layout(B, N).total;
}

int vs_sdr(const float* ref, const float* est, int B, long long N, double* sdr, int* status, void* ws, size_t ws_bytes,
           void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(B > 0 && B <= kMaxRows, "sdr: B=%d (1 .. %d)", B, kMaxRows);
  VS_REQUIRE(N > 0 && N <= kMaxLen, "sdr: N=%lld (1 .. %lld)", N, kMaxLen);
  VS_REQUIRE(ref && est && sdr && status && ws, "sdr: NULL argument");
  const SdrLayout L = sdr_layout(B, N);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total,
             "sdr: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  char* w = static_cast<char*>(ws);
  double* corr = reinterpret_cast<double*>(w + L.corr);
  double* rd = reinterpret_cast<double*>(w + L.rd);
  double* coef = reinterpret_cast<double*>(w + L.coef);
  double* proj = reinterpret_cast<double*>(w + L.proj);
  int* st = reinterpret_cast<int*>(w + L.status);
  hipLaunchKernelGGL(sdr_corr_kernel, dim3(B, (unsigned)L.corr_chunks), dim3(256), 0, stream, ref, est, N, L.corr_tiles,
                     L.corr_tpw, corr);
  hipLaunchKernelGGL(sdr_fold_kernel, dim3(B), dim3(256), 0, stream, corr, (int)L.corr_chunks, rd);
  hipLaunchKernelGGL(sdr_levinson, dim3(B), dim3(64), 0, stream, rd, coef, st);
  hipLaunchKernelGGL(sdr_proj_kernel, dim3(B, (unsigned)L.proj_chunks), dim3(256), 0, stream, ref, est, N, L.proj_tiles,
                     L.proj_tpw, coef, st, proj);
  hipLaunchKernelGGL(sdr_final_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, proj, (int)L.proj_chunks, st, B, sdr, status);
  VS_LAUNCH_CHECK();
  return 0;
}
