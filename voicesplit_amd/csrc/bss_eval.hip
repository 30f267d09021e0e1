// Multi-source BSS-eval (mir_eval.separation.bss_eval_sources): SDR, SIR, SAR of K estimates against K references and
// the best permutation, batched over items, all in fp64.  sdr.hip is the K = 1 corner; the tiles, the Levinson recursion
// and the sums are shared (bss_common.h), and at K = 1 this file runs exactly vs_sdr's arithmetic.
//
// Per item, with the fixed filter length L = 512 and M = N + L - 1:
//   c_ij[m] = sum_n s_i[n] s_j[n+m],  d_iq[m] = sum_n s_i[n] e_q[n+m],  m = 0..L-1     (c_ij[-m] = c_ji[m])
//   G = block Toeplitz of the K x K blocks R[a-b], R[m][i,j] = c_ij[m];  C_q = G^-1 D_q, D_q[(a,i)] = d_iq[a]
//   P_all,q = sum_i C_q[:,i] * s_i;   P_jq = (Toeplitz(c_jj)^-1 d_jq) * s_j          (both M samples)
//   SDR[q,j] = |P_jq|^2 / |e_q - P_jq|^2,  SIR[q,j] = |P_jq|^2 / |P_all,q - P_jq|^2,  SAR[q] = |P_all,q|^2 / |e_q - P_all,q|^2   (dB)
// Launches on the caller's stream, no host synchronisation:
//   bss_corr_kernel    grid (B*K, chunks, K): left signal s_i staged once, slid against the pair (s_j, e_j); partial -> slot
//   bss_fold_kernel    one workgroup per (item, i, j): the chunk slots summed in chunk order
//   bss_block_kernel   K > 1, one workgroup per item: the block Levinson (Whittle-Wiggins-Robinson) recursion for G C = D
//   bss_single_kernel  one wavefront per needed (estimate q, reference j): the scalar recursion for Toeplitz(c_jj) x = d_jq
//   bss_proj_kernel    grid (B*K, chunks): per estimate q, P_all,q and every needed P_jq at the same samples; partial norms -> slot
//   bss_final_kernel   per item: slots in chunk order -> the criteria, the permutation search, NaN / -1 for status != 0
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"
#include "bss_common.h"

namespace {

constexpr int kMaxSrc = 6;
constexpr int kProjSlot = 3 * kMaxSrc + 2;            // per reference j: |P_j|^2, |e - P_j|^2, |P_all - P_j|^2; then |P_all|^2, |e - P_all|^2

struct BssLayout {
  BssTiling T;
  size_t corr, rd, bwd, sol, coef, proj, st_pair, st_block, total;       // byte offsets into the workspace
};

BssLayout bss_layout(int B, int K, long long N) {
  BssLayout L;
  L.T = bss_tiling(N);
  const size_t pairs = (size_t)B * K * K;
  const size_t blk = K > 1 ? pairs * kFlen * sizeof(double) : 0;
  size_t off = 0;
  L.corr = off;     off = align256(off + pairs * L.T.corr_chunks * kSlot * sizeof(double));
  L.rd = off;       off = align256(off + pairs * kSlot * sizeof(double));
  L.bwd = off;      off = align256(off + (K > 4 ? blk : 0));    // the reversed backward predictor, where LDS cannot hold it
  L.sol = off;      off = align256(off + blk);
  L.coef = off;     off = align256(off + pairs * kFlen * sizeof(double));
  L.proj = off;     off = align256(off + (size_t)B * K * L.T.proj_chunks * kProjSlot * sizeof(double));
  L.st_pair = off;  off = align256(off + pairs * sizeof(int));
  L.st_block = off; off = align256(off + (size_t)B * sizeof(int));
  L.total = off;
  return L;
}

// slot of (item, left i, right pair j): [0, 512) c_ij, [512, 1024) d_ij, [1024] sum e_j^2
__device__ __forceinline__ long long pair_index(int item, int i, int j, int K) { return ((long long)item * K + i) * K + j; }

__global__ void __launch_bounds__(256) bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est, int K, long long N,
                                                       long long tiles, long long tpw, double* __restrict__ part) {
  __shared__ double Lf[kCorrLds];                                       // the left signal s_i
  __shared__ double S[kCorrLds];                                        // the right pair: s_j, e_j
  __shared__ double E[kCorrLds];
  const int row = blockIdx.x, chunk = blockIdx.y, j = blockIdx.z, tid = threadIdx.x;      // row = item * K + i
  const int wave = tid >> 6, lane = tid & 63;
  const int item = row / K;
  const float* l = ref + (long long)row * N;
  const float* s = ref + ((long long)item * K + j) * N;
  const float* e = est + ((long long)item * K + j) * N;
  double ar[8], ad[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) ar[u] = ad[u] = 0.0;
  double ee = 0.0;
  const long long t_end = min((long long)(chunk + 1) * tpw, tiles);
  for (long long t = (long long)chunk * tpw; t < t_end; ++t) {
    const long long n0 = t * kCorrTile;
    __syncthreads();                                                    // the previous tile's readers are done
    corr_stage(l, N, n0, Lf, nullptr);
    corr_stage(s, N, n0, S, nullptr);
    corr_stage(e, N, n0, E, &ee);
    __syncthreads();
    corr_slide(Lf, S, E, wave, lane, ar, ad);
  }
  __syncthreads();
  corr_store(ar, ad, ee, S, E, part + (((long long)row * K + j) * gridDim.y + chunk) * kSlot);
}

__global__ void __launch_bounds__(256) bss_fold_kernel(const double* __restrict__ part, int chunks, double* __restrict__ rd) {
  const long long p = blockIdx.x;
  corr_fold(part + p * chunks * kSlot, chunks, rd + p * kSlot);
}

// ---- K x K helpers, everything in registers (K is a template parameter: all indices are static) ----------------------
template <int K>
__device__ __forceinline__ void mat_mul(const double* A, const double* Bm, double* C) {       // C = A B
#pragma unroll
  for (int r = 0; r < K; ++r)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) v = fma(A[r * K + k], Bm[k * K + c], v);
      C[r * K + c] = v;
    }
}

// inv = A^-1 by Gauss-Jordan elimination with partial pivoting; false when a pivot is 0 or anything is not finite.
// Rows are eliminated against the UNSCALED pivot row with the factor a[r][k] / p (a true division) and scaled only at the
// end: two rows with the same bits get the same operations until one of them is the pivot, the factor is then exactly 1 and
// the other row becomes exactly 0 and stays 0, so its pivot is exactly 0 -- a matrix with two identical rows is always caught.
template <int K>
__device__ __forceinline__ bool mat_inv(const double* A, double* inv) {
  double a[K * K], b[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    a[i] = A[i];
    b[i] = (i / K == i % K) ? 1.0 : 0.0;
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int r = k + 1; r < K; ++r) {
      const bool sw = fabs(a[r * K + k]) > fabs(a[k * K + k]);
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const double ta = a[k * K + c], tb = b[k * K + c];
        a[k * K + c] = sw ? a[r * K + c] : ta;
        a[r * K + c] = sw ? ta : a[r * K + c];
        b[k * K + c] = sw ? b[r * K + c] : tb;
        b[r * K + c] = sw ? tb : b[r * K + c];
      }
    }
    const double p = a[k * K + k];
    ok = ok && p != 0.0 && isfinite(p);
#pragma unroll
    for (int r = 0; r < K; ++r) {
      if (r == k) continue;
      const double f = a[r * K + k] / p;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        a[r * K + c] = fma(-f, a[k * K + c], a[r * K + c]);
        b[r * K + c] = fma(-f, b[k * K + c], b[r * K + c]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    const double v = b[i] / a[(i / K) * K + i / K];
    ok = ok && isfinite(v);
    inv[i] = v;
  }
  return ok;
}

// Block Levinson recursion for G C = D, one workgroup per item.  Blocks are stored element-major ("SoA"): element e = r * K + c
// of block j at [e * stride + j], so that the 256 threads, one block index each, read consecutive doubles.  R[m] and D come from
// where the fold left them (element (i, j) of R[m] at slot (i, j) + m, of D[a] at slot (i, q) + 512 + a).
//   F^(n): T_n F = [I, 0 .. 0]^T (forward predictor), B^(n): T_n B = [0 .. 0, I]^T (backward predictor), X^(n): T_n X = D[0..n)
//   e_F = sum_j R[n-j] F_j,  e_B = sum_j R[-(j+1)] B_j,  e_X = sum_j R[n-j] X_j
//   alpha = (I - e_B e_F)^-1, beta = -e_F alpha, delta = (I - e_F e_B)^-1, gamma = -e_B delta
//   F' = [F; 0] alpha + [0; B] beta,  B' = [F; 0] gamma + [0; B] delta,  X' = [X; 0] + B' (D[n] - e_X)
// B is kept reversed (Bt_j = B_{n-1-j}): then e_B = sum_j R[n-j]^T Bt_j, and step n reads and writes F_j and Bt_{n-j} together, in
// place.  A step: every thread sums its block indices' share of e_F, e_B, e_X; waves fold with shuffles, the 4 waves through LDS;
// wave 0 forms alpha .. delta and mu = D[n] - e_X and leaves them in LDS; every thread updates its block indices.
// LDS holds, of F, Bt, X and a copy of R (512 K^2 doubles each), the first kLds that fit: all four for K <= 3, F and Bt at K = 4,
// F alone at K = 5, 6; the others live in the workspace, which L2 holds.
template <int K>
struct BlockLds {
  static constexpr int kArrays = K <= 3 ? 4 : (K == 4 ? 2 : 1);
};

template <int K>
__global__ void __launch_bounds__(256) bss_block_kernel(const double* __restrict__ rd, double* __restrict__ bwd, double* __restrict__ sol,
                                                        int* __restrict__ st_block) {
  constexpr int KK = K * K;
  constexpr int kLds = BlockLds<K>::kArrays;
  constexpr bool kBtLds = kLds >= 2, kXLds = kLds >= 3, kRLds = kLds >= 4;
  constexpr int kRs = kRLds ? kFlen : kSlot;                            // element stride of R
  __shared__ double lds[kLds * kFlen * KK];
  __shared__ double red[4][3 * KK];
  __shared__ double coef[5 * KK];                                       // alpha, beta, gamma, delta, mu
  __shared__ int failed;
  const int item = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double* Rg = rd + (long long)item * KK * kSlot;
  double* Xg = sol + (long long)item * KK * kFlen;
  double* F = lds;
  double* Bt = kBtLds ? lds + kFlen * KK : bwd + (long long)item * KK * kFlen;
  double* X = kXLds ? lds + 2 * kFlen * KK : Xg;
  const double* R = kRLds ? lds + 3 * kFlen * KK : Rg;
  for (int i = tid; i < KK * kFlen; i += 256) {
    F[i] = 0.0;
    Bt[i] = 0.0;
    X[i] = 0.0;
    if (kRLds) lds[3 * kFlen * KK + i] = Rg[(i / kFlen) * kSlot + (i % kFlen)];
  }
  if (tid == 0) failed = 0;
  __syncthreads();
  if (tid == 0) {
    double r0[KK], inv[KK], d0[KK], x0[KK];
#pragma unroll
    for (int e = 0; e < KK; ++e) {
      r0[e] = Rg[e * kSlot];
      d0[e] = Rg[e * kSlot + kFlen];                                    // D[0]
    }
    if (!mat_inv<K>(r0, inv)) failed = 1;
    mat_mul<K>(inv, d0, x0);
#pragma unroll
    for (int e = 0; e < KK; ++e) {
      F[e * kFlen] = inv[e];
      Bt[e * kFlen] = inv[e];
      X[e * kFlen] = x0[e];
    }
  }
  __syncthreads();
  if (failed) {                                                         // uniform
    if (tid == 0) st_block[item] = 2;
    return;
  }
  for (int n = 1; n < kFlen; ++n) {
    double dn = 0.0;                                                    // D[n], one element per lane of wave 0: in flight during the sums
    if (wave == 0 && lane < KK) dn = Rg[lane * kSlot + kFlen + n];
    {
      double eF[KK], eB[KK], eX[KK];
#pragma unroll
      for (int e = 0; e < KK; ++e) eF[e] = eB[e] = eX[e] = 0.0;
#pragma unroll 1
      for (int j = tid; j < n; j += 256) {
        double Rm[KK];
#pragma unroll
        for (int e = 0; e < KK; ++e) Rm[e] = R[e * kRs + (n - j)];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int c = 0; c < K; ++c) {
            const double f = F[(k * K + c) * kFlen + j], b = Bt[(k * K + c) * kFlen + j], x = X[(k * K + c) * kFlen + j];
#pragma unroll
            for (int r = 0; r < K; ++r) {
              eF[r * K + c] = fma(Rm[r * K + k], f, eF[r * K + c]);
              eB[r * K + c] = fma(Rm[k * K + r], b, eB[r * K + c]);     // R[n-j]^T
              eX[r * K + c] = fma(Rm[r * K + k], x, eX[r * K + c]);
            }
          }
      }
#pragma unroll
      for (int e = 0; e < KK; ++e) {
        const double a = wave_sum(eF[e]), b = wave_sum(eB[e]), c = wave_sum(eX[e]);
        if (lane == 0) {
          red[wave][e] = a;
          red[wave][KK + e] = b;
          red[wave][2 * KK + e] = c;
        }
      }
    }
    __syncthreads();
    if (wave == 0) {                                                    // every lane the same bits; lane 0 writes
      double eF[KK], eB[KK], t0[KK], t1[KK];
#pragma unroll
      for (int e = 0; e < KK; ++e) {                                    // the 4 waves in wave order
        eF[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        eB[e] = ((red[0][KK + e] + red[1][KK + e]) + red[2][KK + e]) + red[3][KK + e];
      }
      mat_mul<K>(eB, eF, t0);
#pragma unroll
      for (int e = 0; e < KK; ++e) t0[e] = ((e / K == e % K) ? 1.0 : 0.0) - t0[e];
      bool ok = mat_inv<K>(t0, t1);                                     // alpha
      mat_mul<K>(eF, t1, t0);                                           // -beta
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < KK; ++e) {
          coef[e] = t1[e];
          coef[KK + e] = -t0[e];
        }
      }
      mat_mul<K>(eF, eB, t0);
#pragma unroll
      for (int e = 0; e < KK; ++e) t0[e] = ((e / K == e % K) ? 1.0 : 0.0) - t0[e];
      ok = mat_inv<K>(t0, t1) && ok;                                    // delta
      mat_mul<K>(eB, t1, t0);                                           // -gamma
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < KK; ++e) {
          coef[2 * KK + e] = -t0[e];
          coef[3 * KK + e] = t1[e];
        }
        if (!ok) failed = 1;
      }
      if (lane < KK)                                                    // mu = D[n] - e_X
        coef[4 * KK + lane] = dn - (((red[0][2 * KK + lane] + red[1][2 * KK + lane]) + red[2][2 * KK + lane]) + red[3][2 * KK + lane]);
    }
    __syncthreads();
    if (failed) {                                                       // uniform
      if (tid == 0) st_block[item] = 2;
      return;
    }
    const double* al = coef;
    const double* be = coef + KK;
    const double* ga = coef + 2 * KK;
    const double* de = coef + 3 * KK;
    const double* mu = coef + 4 * KK;
#pragma unroll 1
    for (int j = tid; j <= n; j += 256) {
#pragma unroll
      for (int r = 0; r < K; ++r) {                                     // row r of the new blocks needs row r of the old ones only
        asm volatile("" ::: "memory");                                  // coefficients are re-read from LDS row by row, not held in registers
        double Fj[K], Bi[K], Bn[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          Fj[k] = F[(r * K + k) * kFlen + j];
          Bi[k] = Bt[(r * K + k) * kFlen + (n - j)];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
          double vf = 0.0, vb = 0.0;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            vf = fma(Fj[k], al[k * K + c], vf);
            vb = fma(Fj[k], ga[k * K + c], vb);
          }
#pragma unroll
          for (int k = 0; k < K; ++k) {
            vf = fma(Bi[k], be[k * K + c], vf);
            vb = fma(Bi[k], de[k * K + c], vb);
          }
          F[(r * K + c) * kFlen + j] = vf;
          Bn[c] = vb;
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
          double v = X[(r * K + c) * kFlen + j];
#pragma unroll
          for (int k = 0; k < K; ++k) v = fma(Bn[k], mu[k * K + c], v);
          X[(r * K + c) * kFlen + j] = v;
          Bt[(r * K + c) * kFlen + (n - j)] = Bn[c];
        }
      }
    }
    __syncthreads();
  }
  if (kXLds)
    for (int i = tid; i < KK * kFlen; i += 256) Xg[i] = X[i];
  if (tid == 0) st_block[item] = 0;
}

// One wavefront per (item, estimate q, reference j): Toeplitz(c_jj) x = d_jq, as vs_sdr solves it for the pair (s_j, e_q).
// With diag_only, q = j.  coef and st_pair are indexed [item][q][j].
__global__ void __launch_bounds__(64) bss_single_kernel(const double* __restrict__ rd, int K, int diag_only, double* __restrict__ coef,
                                                        int* __restrict__ st_pair) {
  __shared__ double r[kFlen], d[kFlen], a[kFlen], x[kFlen];
  const int lane = threadIdx.x;
  int item, q, j;
  if (diag_only) {
    item = blockIdx.x / K;
    q = j = blockIdx.x % K;
  } else {
    item = blockIdx.x / (K * K);
    q = (blockIdx.x / K) % K;
    j = blockIdx.x % K;
  }
  const double* rsrc = rd + pair_index(item, j, j, K) * kSlot;          // c_jj
  const double* dsrc = rd + pair_index(item, j, q, K) * kSlot;          // d_jq in its second half, sum e_q^2 behind
  const long long out = pair_index(item, q, j, K);
  const double r0 = rsrc[0], ee = dsrc[1024];
  if (!(r0 > 0.0) || !(ee > 0.0)) {                                     // all-zero reference or estimate row
    if (lane == 0) st_pair[out] = 1;
    return;
  }
  if (levinson512(rsrc, dsrc + kFlen, r, d, a, x, lane)) {
    if (lane == 0) st_pair[out] = 2;
    return;
  }
  for (int k = lane; k < kFlen; k += 64) coef[out * kFlen + k] = x[k];
  if (lane == 0) st_pair[out] = 0;
}

// item status from the computed pairs' and the block solve's: 1 (a silent row) before 2 (a failed solve)
__device__ __forceinline__ int item_status(const int* __restrict__ st_pair, const int* __restrict__ st_block, int item, int K,
                                           int diag_only) {
  int s1 = 0, s2 = 0;
  for (int q = 0; q < K; ++q)
    for (int j = 0; j < K; ++j) {
      if (diag_only && j != q) continue;
      const int s = st_pair[pair_index(item, q, j, K)];
      s1 |= s == 1;
      s2 |= s == 2;
    }
  if (K > 1) s2 |= st_block[item] == 2;
  return s1 ? 1 : (s2 ? 2 : 0);
}

// Per (item, estimate q) and chunk of output samples: P_all,q (K > 1) and P_jq for every needed j at the same samples, and the
// partial norms.  At K = 1 P_all is P_0: nothing is filtered twice, and the two sums are vs_sdr's.
__global__ void __launch_bounds__(256) bss_proj_kernel(const float* __restrict__ ref, const float* __restrict__ est, int K, long long N,
                                                       long long tiles, long long tpw, int diag_only, const double* __restrict__ sol,
                                                       const double* __restrict__ coef, const int* __restrict__ st_pair,
                                                       const int* __restrict__ st_block, double* __restrict__ part) {
  __shared__ double S[kProjLds];
  __shared__ double Cl[kFlen];
  const int row = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;    // row = item * K + q
  const int item = row / K, q = row % K;
  double* out = part + ((long long)row * gridDim.y + chunk) * kProjSlot;
  if (item_status(st_pair, st_block, item, K, diag_only) != 0) {        // uniform: nothing to project
    if (tid < kProjSlot) out[tid] = 0.0;
    return;
  }
  const float* e = est + (long long)row * N;
  const long long M = N + kFlen - 1;
  double nrm[3 * kMaxSrc];
#pragma unroll
  for (int i = 0; i < 3 * kMaxSrc; ++i) nrm[i] = 0.0;
  double aa = 0.0, ra = 0.0;
  const long long t_end = min((long long)(chunk + 1) * tpw, tiles);
  for (long long t = (long long)chunk * tpw; t < t_end; ++t) {
    const long long m0 = t * kProjTile;
    double ev[16], all[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long m = m0 + tid * 16 + i;
      ev[i] = m < N ? (double)e[m] : 0.0;
      all[i] = 0.0;
    }
    if (K > 1) {
      for (int i = 0; i < K; ++i) {                                     // P_all,q += C_q[:, i] * s_i, sources in order
        __syncthreads();
        proj_stage(ref + ((long long)item * K + i) * N, N, m0, S);
        for (int k = tid; k < kFlen; k += 256) Cl[k] = sol[((long long)item * K * K + i * K + q) * kFlen + k];
        __syncthreads();
        proj_filter(S, Cl, all);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (m0 + tid * 16 + i < M) {
          const double res = ev[i] - all[i];
          aa = fma(all[i], all[i], aa);
          ra = fma(res, res, ra);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kMaxSrc; ++j) {
      if (j >= K || (diag_only && j != q)) continue;                    // uniform
      __syncthreads();
      proj_stage(ref + ((long long)item * K + j) * N, N, m0, S);
      for (int k = tid; k < kFlen; k += 256) Cl[k] = coef[pair_index(item, q, j, K) * kFlen + k];
      __syncthreads();
      double acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0;
      proj_filter(S, Cl, acc);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (m0 + tid * 16 + i < M) {
          const double res = ev[i] - acc[i];
          const double itf = K > 1 ? all[i] - acc[i] : 0.0;            // one source: no interference term
          nrm[3 * j] = fma(acc[i], acc[i], nrm[3 * j]);
          nrm[3 * j + 1] = fma(res, res, nrm[3 * j + 1]);
          nrm[3 * j + 2] = fma(itf, itf, nrm[3 * j + 2]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3 * kMaxSrc; ++i) {
    if (i / 3 >= K) continue;
    const double v = block_sum256(nrm[i], S);
    if (tid == 0) out[i] = v;
  }
  const double ta = block_sum256(aa, S);
  const double tr = block_sum256(ra, S);
  if (tid == 0) {
    out[3 * kMaxSrc] = ta;
    out[3 * kMaxSrc + 1] = tr;
  }
}

__device__ __forceinline__ double safe_db(double num, double den) { return den == 0.0 ? __builtin_inf() : 10.0 * log10(num / den); }

// One thread per item: the criteria of every computed pair, the permutation search and the outputs.
__global__ void __launch_bounds__(64) bss_final_kernel(const double* __restrict__ part, int chunks, const int* __restrict__ st_pair,
                                                       const int* __restrict__ st_block, int B, int K, int compute_permutation,
                                                       double* __restrict__ sdr, double* __restrict__ sir, double* __restrict__ sar,
                                                       int* __restrict__ perm, int* __restrict__ status, double* __restrict__ pairs) {
  const int item = blockIdx.x * 64 + threadIdx.x;
  if (item >= B) return;
  const double nan = __builtin_nan("");
  const int st = item_status(st_pair, st_block, item, K, !compute_permutation);
  status[item] = st;
  double* pr = pairs ? pairs + (long long)item * 3 * K * K : nullptr;
  if (st != 0) {
    for (int k = 0; k < K; ++k) {
      sdr[item * K + k] = sir[item * K + k] = sar[item * K + k] = nan;
      perm[item * K + k] = -1;
    }
    if (pr)
      for (int i = 0; i < 3 * K * K; ++i) pr[i] = nan;
    return;
  }
  double c_sdr[kMaxSrc * kMaxSrc], c_sir[kMaxSrc * kMaxSrc], c_sar[kMaxSrc * kMaxSrc];    // [estimate q][reference j]
  for (int q = 0; q < K; ++q) {
    const double* p = part + ((long long)item * K + q) * chunks * kProjSlot;
    double aa = 0.0, ra = 0.0;
    for (int c = 0; c < chunks; ++c) {
      aa += p[(long long)c * kProjSlot + 3 * kMaxSrc];
      ra += p[(long long)c * kProjSlot + 3 * kMaxSrc + 1];
    }
    for (int j = 0; j < K; ++j) {
      if (!compute_permutation && j != q) {
        c_sdr[q * K + j] = c_sir[q * K + j] = c_sar[q * K + j] = nan;
        continue;
      }
      double pp = 0.0, rr = 0.0, ii = 0.0;
      for (int c = 0; c < chunks; ++c) {
        pp += p[(long long)c * kProjSlot + 3 * j];
        rr += p[(long long)c * kProjSlot + 3 * j + 1];
        ii += p[(long long)c * kProjSlot + 3 * j + 2];
      }
      c_sdr[q * K + j] = safe_db(pp, rr);
      c_sir[q * K + j] = safe_db(pp, ii);
      c_sar[q * K + j] = K > 1 ? safe_db(aa, ra) : c_sdr[q * K + j];    // one source: P_all is P_0
    }
  }
  bool bad = false;                                                     // NaN from a solve that went wrong unnoticed: status 2
  for (int i = 0; i < K * K; ++i)
    if (compute_permutation || i / K == i % K) bad = bad || c_sdr[i] != c_sdr[i] || c_sir[i] != c_sir[i] || c_sar[i] != c_sar[i];
  if (bad) {
    status[item] = 2;
    for (int k = 0; k < K; ++k) {
      sdr[item * K + k] = sir[item * K + k] = sar[item * K + k] = nan;
      perm[item * K + k] = -1;
    }
    if (pr)
      for (int i = 0; i < 3 * K * K; ++i) pr[i] = nan;
    return;
  }
  if (pr)
    for (int i = 0; i < K * K; ++i) {
      pr[i] = c_sdr[i];
      pr[K * K + i] = c_sir[i];
      pr[2 * K * K + i] = c_sar[i];
    }
  int best[kMaxSrc], cur[kMaxSrc];
  for (int k = 0; k < K; ++k) best[k] = cur[k] = k;
  if (compute_permutation && K > 1) {
    double best_sum = 0.0;
    bool first = true;
    for (;;) {                                                          // lexicographic order = itertools.permutations(range(K))
      double sum = 0.0;
      for (int j = 0; j < K; ++j) sum += c_sir[cur[j] * K + j];
      if (first || sum > best_sum) {                                    // the first maximum wins
        best_sum = sum;
        first = false;
        for (int k = 0; k < K; ++k) best[k] = cur[k];
      }
      int i = K - 2;
      while (i >= 0 && cur[i] > cur[i + 1]) --i;
      if (i < 0) break;
      int l = K - 1;
      while (cur[l] < cur[i]) --l;
      int tmp = cur[i];
      cur[i] = cur[l];
      cur[l] = tmp;
      for (int lo = i + 1, hi = K - 1; lo < hi; ++lo, --hi) {
        tmp = cur[lo];
        cur[lo] = cur[hi];
        cur[hi] = tmp;
      }
    }
  }
  for (int j = 0; j < K; ++j) {
    sdr[item * K + j] = c_sdr[best[j] * K + j];
    sir[item * K + j] = c_sir[best[j] * K + j];
    sar[item * K + j] = c_sar[best[j] * K + j];
    perm[item * K + j] = best[j];
  }
}

template <int K>
void launch_block(int B, const double* rd, double* bwd, double* sol, int* st_block, hipStream_t stream) {
  hipLaunchKernelGGL(bss_block_kernel<K>, dim3(B), dim3(256), 0, stream, rd, bwd, sol, st_block);
}

bool bss_args_ok(int B, int K, long long N) {
  return B > 0 && B <= kMaxRows && K >= 1 && K <= kMaxSrc && N > 0 && N <= kMaxLen;
}

}  // namespace

size_t vs_bss_eval_workspace_bytes(int B, int K, long long N) {
  if (!bss_args_ok(B, K, N)) return 0;
  return bss_layout(B, K, N).total;
}

int vs_bss_eval(const float* ref, const float* est, int B, int K, long long N, int compute_permutation, double* sdr, double* sir,
                double* sar, int* perm, int* status, double* pairs, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(B > 0 && B <= kMaxRows, "bss_eval: B=%d (1 .. %d)", B, kMaxRows);
  VS_REQUIRE(K >= 1 && K <= kMaxSrc, "bss_eval: K=%d (1 .. %d)", K, kMaxSrc);
  VS_REQUIRE(N > 0 && N <= kMaxLen, "bss_eval: N=%lld (1 .. %lld)", N, kMaxLen);
  VS_REQUIRE(ref && est && sdr && sir && sar && perm && status && ws, "bss_eval: NULL argument");
  const BssLayout L = bss_layout(B, K, N);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total,
             "bss_eval: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  char* w = static_cast<char*>(ws);
  double* corr = reinterpret_cast<double*>(w + L.corr);
  double* rd = reinterpret_cast<double*>(w + L.rd);
  double* bwd = reinterpret_cast<double*>(w + L.bwd);
  double* sol = reinterpret_cast<double*>(w + L.sol);
  double* coef = reinterpret_cast<double*>(w + L.coef);
  double* proj = reinterpret_cast<double*>(w + L.proj);
  int* st_pair = reinterpret_cast<int*>(w + L.st_pair);
  int* st_block = reinterpret_cast<int*>(w + L.st_block);
  const int diag_only = compute_permutation ? 0 : 1;
  hipLaunchKernelGGL(bss_corr_kernel, dim3(B * K, (unsigned)L.T.corr_chunks, K), dim3(256), 0, stream, ref, est, K, N, L.T.corr_tiles,
                     L.T.corr_tpw, corr);
  hipLaunchKernelGGL(bss_fold_kernel, dim3(B * K * K), dim3(256), 0, stream, corr, (int)L.T.corr_chunks, rd);
  switch (K) {
    case 2: launch_block<2>(B, rd, bwd, sol, st_block, stream); break;
    case 3: launch_block<3>(B, rd, bwd, sol, st_block, stream); break;
    case 4: launch_block<4>(B, rd, bwd, sol, st_block, stream); break;
    case 5: launch_block<5>(B, rd, bwd, sol, st_block, stream); break;
    case 6: launch_block<6>(B, rd, bwd, sol, st_block, stream); break;
    default: break;                                                     // K = 1: the single-source solve is the whole solve
  }
  hipLaunchKernelGGL(bss_single_kernel, dim3(diag_only ? B * K : B * K * K), dim3(64), 0, stream, rd, K, diag_only, coef, st_pair);
  hipLaunchKernelGGL(bss_proj_kernel, dim3(B * K, (unsigned)L.T.proj_chunks), dim3(256), 0, stream, ref, est, K, N, L.T.proj_tiles,
                     L.T.proj_tpw, diag_only, sol, coef, st_pair, st_block, proj);
  hipLaunchKernelGGL(bss_final_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, proj, (int)L.T.proj_chunks, st_pair, st_block, B, K,
                     compute_permutation ? 1 : 0, sdr, sir, sar, perm, status, pairs);
  VS_LAUNCH_CHECK();
  return 0;
}
