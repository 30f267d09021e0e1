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

// LDS index with one pad double every 8 (correlation: lanes 8 doubles apart -> 9) / every 16 (projection: 16 -> 17), so
// that the 32 lanes of a ds_read_b64 group hit 32 distinct bank pairs
__device__ __forceinline__ int pos8(int m) { return m + (m >> 3); }
__device__ __forceinline__ int pos16(int m) { return m + (m >> 4); }

struct SdrLayout {
  long long corr_tiles, corr_tpw, corr_chunks;
  long long proj_tiles, proj_tpw, proj_chunks;
  size_t corr, rd, coef, proj, status, total;        // byte offsets into the workspace
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

SdrLayout sdr_layout(int B, long long N) {
  SdrLayout L;
  L.corr_tiles = (N + kCorrTile - 1) / kCorrTile;
  L.corr_tpw = (L.corr_tiles + kMaxChunks - 1) / kMaxChunks;
  L.corr_chunks = (L.corr_tiles + L.corr_tpw - 1) / L.corr_tpw;
  const long long M = N + kFlen - 1;
  L.proj_tiles = (M + kProjTile - 1) / kProjTile;
  L.proj_tpw = (L.proj_tiles + kMaxChunks - 1) / kMaxChunks;
  L.proj_chunks = (L.proj_tiles + L.proj_tpw - 1) / L.proj_tpw;
  size_t off = 0;
  L.corr = off;   off = align256(off + (size_t)B * L.corr_chunks * kSlot * sizeof(double));
  L.rd = off;     off = align256(off + (size_t)B * kSlot * sizeof(double));
  L.coef = off;   off = align256(off + (size_t)B * kFlen * sizeof(double));
  L.proj = off;   off = align256(off + (size_t)B * L.proj_chunks * 2 * sizeof(double));
  L.status = off; off = align256(off + (size_t)B * sizeof(int));
  L.total = off;
  return L;
}

// fixed-order tree sum of v over the 256 threads of a workgroup; red: 256 doubles of LDS; result valid in thread 0
__device__ double block_sum256(double v, double* red) {
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
    for (int i = tid; i < kCorrStage; i += 256) {
      const long long g = n0 + i;
      const double sv = g < N ? (double)s[g] : 0.0;
      const double ev = g < N ? (double)e[g] : 0.0;
      S[pos8(i)] = sv;
      E[pos8(i)] = ev;
      if (i < kCorrTile) ee += ev * ev;
    }
    __syncthreads();
    const int nb0 = wave * (kCorrTile / 4);                             // this wave's quarter of the tile
    const int k0 = lane * 8;                                            // this lane's lags k0 .. k0 + 7
    double ws[8], we[8];                                                // slot (m - nb0 - k0) & 7 holds s[m], e[m]
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ws[i] = S[pos8(nb0 + k0 + i)];
      we[i] = E[pos8(nb0 + k0 + i)];
    }
    for (int nb = 0; nb < kCorrTile / 4; nb += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int n = nb0 + nb + u;
        const double a = S[pos8(n)];                                    // broadcast
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          ar[j] = fma(a, ws[(u + j) & 7], ar[j]);                       // s[n] s[n + k0 + j]
          ad[j] = fma(a, we[(u + j) & 7], ad[j]);                       // s[n] e[n + k0 + j]
        }
        ws[u] = S[pos8(n + k0 + 8)];                                    // slot u: s[n + k0] is done, s[n + k0 + 8] next
        we[u] = E[pos8(n + k0 + 8)];
      }
    }
  }
  // the 4 waves' partials, summed in wave order (the staging area is free again)
  __syncthreads();
  double* red = S;                                                      // [4][1024] fits in S + E (2 x 2898 doubles)
  double* red2 = E;
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
  double* out = part + ((long long)row * gridDim.y + chunk) * kSlot;
  for (int o = tid; o < 1024; o += 256)
    out[o] = ((red[o] + red[1024 + o]) + red2[o]) + red2[1024 + o];
  const double tot = block_sum256(ee, red);
  if (tid == 0) out[1024] = tot;
}

__global__ void __launch_bounds__(256) sdr_fold_kernel(const double* __restrict__ part, int chunks, double* __restrict__ rd) {
  const int row = blockIdx.x;
  const double* p = part + (long long)row * chunks * kSlot;
  for (int o = threadIdx.x; o < 1025; o += 256) {
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += p[(long long)c * kSlot + o];
    rd[(long long)row * kSlot + o] = v;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);          // commutative pairs: every lane ends with the same bits
  return v;
}

// Levinson recursion for G C = D, G symmetric Toeplitz with first row r: the forward predictor a (a[0] = 1, G_i a = E e_0)
// and the solution x grow one order per step; a reversed is the backward predictor, which extends x to the next order.
__global__ void __launch_bounds__(64) sdr_levinson(const double* __restrict__ rd, double* __restrict__ coef, int* __restrict__ status) {
  __shared__ double r[kFlen], d[kFlen], a[kFlen], x[kFlen];
  const int row = blockIdx.x, lane = threadIdx.x;
  const double* src = rd + (long long)row * kSlot;
  for (int j = lane; j < kFlen; j += 64) {
    r[j] = src[j];
    d[j] = src[kFlen + j];
    a[j] = 0.0;
    x[j] = 0.0;
  }
  const double r0 = src[0], ee = src[1024];
  if (!(r0 > 0.0) || !(ee > 0.0)) {                                     // all-zero reference or estimate row
    if (lane == 0) status[row] = 1;
    return;
  }
  __syncthreads();
  if (lane == 0) {
    a[0] = 1.0;
    x[0] = d[0] / r0;
  }
  __syncthreads();
  double Err = r0;
  int fail = 0;
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
    if (!(Err > 0.0) || !isfinite(Err)) {                               // uniform across the wave
      fail = 1;
      break;
    }
    const double mu = (d[i] - px) / Err;
#pragma unroll
    for (int m = 0; m < kFlen / 64; ++m) {
      const int j = lane + 64 * m;
      if (j <= i) x[j] = fma(mu, a[i - j], x[j]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (fail) {
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
    for (int i = tid; i < kProjStage; i += 256) {                       // local q <-> s[m0 - 512 + q]
      const long long g = m0 - kFlen + i;
      S[pos16(i)] = (g >= 0 && g < N) ? (double)s[g] : 0.0;
    }
    __syncthreads();
    const int q0 = kFlen + tid * 16;                                    // this lane's outputs m0 + 16 tid + i, local q0 + i
    double acc[16], w[16];                                              // slot (q - q0) & 15 holds s at local q
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc[i] = 0.0;
      w[i] = S[pos16(q0 + i)];
    }
    for (int kb = 0; kb < kFlen; kb += 16) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = kb + u;
        const double c = Cl[k];                                         // broadcast
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fma(c, w[(i - u) & 15], acc[i]);    // C[k] s[m - k]
        w[(15 - u) & 15] = S[pos16(q0 - k - 1)];                        // s[q0 + 15 - k] is done, s[q0 - k - 1] next
      }
    }
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

constexpr int kMaxRows = 1 << 20;
constexpr long long kMaxLen = 1LL << 40;

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
