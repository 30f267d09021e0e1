// cnn1 (models/voicesplit/model.py:17-19) of the channels-last paths: x [B][T][F] fp32 -> [B][T][F][64], 1x7 conv with BatchNorm +
// activation in the same pass (bf16 for VS_MATH_BF16, hi / lo f16 planes for the split-f16 forward), the statistics of its output
// from the input's moments, and its backward: in one pass over da1 by recomputation, and the older forms that read z1.
#include "nhwc_common.h"

namespace {

// The forward, the split forward and the one-pass backward share a setup and a walk that stay written out in each of them (as
// functions they move the kernels' registers: profiles/nhwc_edge_split.md):
//   setup  the lane's 8 channels as 4 pairs -- wr[q][k], sc[q], sh[q] hold channels c0 = 8 piece + 2 q and c0 + 1 -- because
//          v_pk_fma_f32 does two channels per issue slot
//   walk   a workgroup takes 32 pixels per sweep of the grid (8 lanes per pixel); the column f is carried along with sr = stride % F:
//          one 64-bit division per launch, not per pixel; the next pixel's load_x7 is issued before this one's exchange_x7

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// out[b][t][f][co] = act(scale[co] * sum_j w[co][j] x[b][t][f+j-3] + shift[co]); STATS: sum / sum of squares of out
template <int ACT, bool STATS>
__global__ __launch_bounds__(256)
void nhwc_conv_first_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                            const float* __restrict__ shift, unsigned short* __restrict__ out, long long npix, int F,
                            double* __restrict__ stats, const float* __restrict__ bias) {
  __shared__ float red[4 * 2 * 64];
  const int piece = threadIdx.x & 7;                      // channels 8*piece .. 8*piece+7
  // setup (with 64 channels x 7 taps + Mish per pixel this kernel is VALU-, not HBM-bound once the BatchNorm + activation ride in it)
  vs_f32x2 wr[4][7], sc[4], sh[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c0 = piece * 8 + 2 * q;
    sc[q] = vs_f32x2{scale[c0], scale[c0 + 1]};
    // bias != NULL: scale / shift are a BatchNorm's constants for z = conv + bias: act(scale (conv + bias) + shift)
    sh[q] = bias ? vs_f32x2{fmaf(bias[c0], sc[q].x, shift[c0]), fmaf(bias[c0 + 1], sc[q].y, shift[c0 + 1])} : vs_f32x2{shift[c0], shift[c0 + 1]};
#pragma unroll
    for (int k = 0; k < 7; ++k) wr[q][k] = vs_f32x2{w[c0 * 7 + k], w[(c0 + 1) * 7 + k]};
  }
  float acc[2][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { acc[0][j] = 0.f; acc[1][j] = 0.f; }
  const long long stride = (long long)gridDim.x * 32;     // pixels per sweep of the grid
  const int sr = (int)(stride % F);
  long long p = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  int f = (int)(p % F);
  // the next pixel's input sample is loaded before this one is computed: the loop is otherwise load -> ~150 VALU -> store with
  // nothing in flight (4 waves per SIMD do not cover a 2 us miss)
  float mine = p < npix ? load_x7(x + (p - f), f, F, piece) : 0.f;
  for (; p < npix; p += stride) {
    int fn = f + sr;
    if (fn >= F) fn -= F;
    const long long pn = p + stride;
    const float mine_next = pn < npix ? load_x7(x + (pn - fn), fn, F, piece) : 0.f;
    float xv[7];
    exchange_x7(mine, xv);
    mine = mine_next;
    f = fn;
    u4v pk;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      vs_f32x2 s2 = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 7; ++k) s2 = __builtin_elementwise_fma(wr[q][k], vs_f32x2{xv[k], xv[k]}, s2);
      const vs_f32x2 y = vs_act_fast2<ACT>(__builtin_elementwise_fma(s2, sc[q], sh[q]));
      if (STATS) {
        acc[0][2 * q] += y.x; acc[0][2 * q + 1] += y.y;
        acc[1][2 * q] = fmaf(y.x, y.x, acc[1][2 * q]); acc[1][2 * q + 1] = fmaf(y.y, y.y, acc[1][2 * q + 1]);
      }
      pk[q] = vs_pack_bf16(y.x, y.y);
    }
    __builtin_nontemporal_store(pk, reinterpret_cast<u4v*>(out + p * 64 + piece * 8));
  }
  if (STATS) fold_channel_sums<2>(acc, stats, red);
}

// ---- by recomputation (round 4) ------------------------------------------------------------------------------------------------------
// cnn1 is 7 MACs per output and its input is 1/64 of its output: nothing of it needs to be WRITTEN to be available again.
// Train-mode BatchNorm needs the batch statistics of z1 = conv(x) + bias before the activation can be applied -- but z1 is
// linear in seven shifted copies of x, so its per-channel sum and sum of squares follow from the 7 sums S[k] and the 28
// products R[k][k'] of the shifted inputs (ONE pass over the 46 MB input, independent of the 64 channels):
//   sum z_c   = sum_k w[c][k] S[k] + N b_c          sum z_c^2 = sum_kk' w[c][k] w[c][k'] R[k][k'] + 2 b_c sum_k w[c][k] S[k] + N b_c^2
// The forward then writes a1 = act(BN(z1)) in one pass (no z1 tensor, no apply pass); the backward recomputes z1 from x
// beside the derivative and needs ONE pass over da1: the BatchNorm backward dz = cA dy + cB z + cC is linear in dy and z,
// so dw[c][k] = sum dz x_k = cA sum(dy x_k) + cB sum(z x_k) + cC S[k], with sum(z x_k) = sum_k' w[c][k'] R[k'][k] + b_c S[k].
// x_k = x[b][t][f + k - 3], zero outside the row (ZeroPad2d((3, 3, 0, 0)), models/voicesplit/model.py:17).
constexpr int kMomN = 7 + 28;                            // S[0..6], then R[k][k'] for k <= k' row by row

__global__ __launch_bounds__(256)
void nhwc_first_moments_kernel(const float* __restrict__ x, long long npix, int F, double* __restrict__ mom, unsigned* turn) {
  __shared__ float red[4][kMomN];
  float acc[kMomN];
#pragma unroll
  for (int i = 0; i < kMomN; ++i) acc[i] = 0.f;
  const long long stride = (long long)gridDim.x * 256;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += stride) {
    const int f = (int)(p % F);
    const float* xr = x + (p - f);
    float xv[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int ff = f + k - 3;
      xv[k] = (ff >= 0 && ff < F) ? xr[ff] : 0.f;
    }
    int i = 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      acc[k] += xv[k];
#pragma unroll
      for (int k2 = k; k2 < 7; ++k2) { acc[i] = fmaf(xv[k], xv[k2], acc[i]); ++i; }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kMomN; ++i) {
    float v = acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  // deterministic mode: mom is [VS_BN_STAT_SLOTS][64] then (the workgroups of a slot add in index order, a fold kernel sums the slots);
  // mirrors slot_turn / slot_turn_begin / slot_turn_end
  const unsigned slot = blockIdx.x % VS_BN_STAT_SLOTS, rank_in_slot = blockIdx.x / VS_BN_STAT_SLOTS;
  unsigned* my_turn = turn ? turn + VS_TURN_SLOT + slot : nullptr;
  if (turn) mom += (size_t)slot * 64;
  vs_turn_begin(my_turn, rank_in_slot);
  if (threadIdx.x < kMomN) atomicAdd(mom + threadIdx.x, (double)red[0][threadIdx.x] + (double)red[1][threadIdx.x] + (double)red[2][threadIdx.x] + (double)red[3][threadIdx.x]);
  vs_turn_end(my_turn, rank_in_slot, (gridDim.x - slot + VS_BN_STAT_SLOTS - 1) / VS_BN_STAT_SLOTS);
}

__global__ void fold_moment_slots_kernel(const double* __restrict__ slots, double* __restrict__ mom) {      // 64 threads
  if (threadIdx.x >= kMomN) return;
  double v = 0.0;
  for (int k = 0; k < VS_BN_STAT_SLOTS; ++k) v += slots[(size_t)k * 64 + threadIdx.x];
  mom[threadIdx.x] = v;
}

__device__ __forceinline__ double mom_R(const double* mom, int k, int k2) {          // R[k][k2], symmetric
  if (k > k2) { const int t = k; k = k2; k2 = t; }
  return mom[7 + k * 7 - k * (k - 1) / 2 + (k2 - k)];
}

// stats[c] = {sum z_c, sum z_c^2} over the `count` pixels, from the moments (one thread per channel, fp64)
__global__ void nhwc_first_stats_kernel(const double* __restrict__ mom, const float* __restrict__ w, const float* __restrict__ bias,
                                        double count, double* __restrict__ stats) {
  const int c = threadIdx.x;
  if (c >= 64) return;
  const double b = bias[c];
  double ws = 0.0, q = 0.0;
  for (int k = 0; k < 7; ++k) {
    ws += (double)w[c * 7 + k] * mom[k];
    for (int k2 = 0; k2 < 7; ++k2) q += (double)w[c * 7 + k] * (double)w[c * 7 + k2] * mom_R(mom, k, k2);
  }
  stats[2 * c] = ws + count * b;
  stats[2 * c + 1] = q + 2.0 * b * ws + count * b * b;
}

// one pass over da1: per channel sum dy, sum dy xhat, sum dy x_k (k = 0..6) with z1 recomputed from x
template <int ACT>
__global__ __launch_bounds__(256)
void nhwc_first_bwd_kernel(const u4v* __restrict__ da, const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                           long long npix, int F, const float* __restrict__ scale, const float* __restrict__ shift,
                           const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ acc_out /* [64][9] */,
                           unsigned* turn) {
  __shared__ float red[4 * 9 * 64];
  const int piece = threadIdx.x & 7;
  // channel pairs throughout (v_pk_*_f32): per pixel and pair 7 FMAs for z, the derivative, 9 FMAs into the sums
  vs_f32x2 wr[4][7], bs[4], sc[4], sh[4], mu[4], is[4], acc[9][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c0 = piece * 8 + 2 * q;
    bs[q] = vs_f32x2{bias[c0], bias[c0 + 1]};
    sc[q] = vs_f32x2{scale[c0], scale[c0 + 1]};
    sh[q] = vs_f32x2{shift[c0], shift[c0 + 1]};
    mu[q] = vs_f32x2{mean[c0], mean[c0 + 1]};
    is[q] = vs_f32x2{invstd[c0], invstd[c0 + 1]};
#pragma unroll
    for (int k = 0; k < 7; ++k) wr[q][k] = vs_f32x2{w[c0 * 7 + k], w[(c0 + 1) * 7 + k]};
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k][q] = vs_f32x2{0.f, 0.f};
  }
  const long long stride = (long long)gridDim.x * 32;     // pixels per sweep of the grid
  const int sr = (int)(stride % F);
  long long p = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  int f = (int)(p % F);
  // The next pixel's gradient piece and input sample are loaded before this one is computed.  (Measured, tools/edge_micro.py at
  // B = 64: 1.07-1.10 ms = 1.4 TB/s with or without this, with a ring three deep, with branch-free loads, and with a two-deep ring
  // of untracked inline-assembly loads + explicit vmcnt at one wave per SIMD -- and the scalar form of the arithmetic ran the
  // same 1.1-1.2 ms as this packed one.  The loop is bound by its VALU work: ~160 instructions + 16 transcendentals per 8-channel
  // piece, and v_pk_fma_f32 buys nothing over two v_fma_f32 here.  Halving it means the matrix pipe: z as a K = 7 contraction and
  // the sums of dy x_k as a contraction over pixels -- not built.)
  auto process = [&](float mine, const u4v& g) {
    float xv[7];
    exchange_x7(mine, xv);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      vs_f32x2 zv = bs[q];
#pragma unroll
      for (int k = 0; k < 7; ++k) zv = __builtin_elementwise_fma(wr[q][k], vs_f32x2{xv[k], xv[k]}, zv);
      const vs_f32x2 dy = bf_pair(g[q]) * nhwc_act_grad2<ACT>(__builtin_elementwise_fma(zv, sc[q], sh[q]));
      acc[0][q] += dy;
      acc[1][q] = __builtin_elementwise_fma(dy, (zv - mu[q]) * is[q], acc[1][q]);
#pragma unroll
      for (int k = 0; k < 7; ++k) acc[2 + k][q] = __builtin_elementwise_fma(dy, vs_f32x2{xv[k], xv[k]}, acc[2 + k][q]);
    }
  };
  float mine = 0.f;
  u4v g = {0u, 0u, 0u, 0u};
  if (p < npix) {
    mine = load_x7(x + (p - f), f, F, piece);
    g = __builtin_nontemporal_load(da + p * 8 + piece);
  }
  for (; p < npix; p += stride) {
    int fn = f + sr;
    if (fn >= F) fn -= F;
    const long long pn = p + stride;
    float mine_next = 0.f;
    u4v g_next = {0u, 0u, 0u, 0u};
    if (pn < npix) {
      mine_next = load_x7(x + (pn - fn), fn, F, piece);
      g_next = __builtin_nontemporal_load(da + pn * 8 + piece);
    }
    process(mine, g);
    mine = mine_next;
    g = g_next;
    f = fn;
  }
  // the 9 x 8 form of fold_channel_sums' fold
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = (j & 1) ? acc[k][j >> 1].y : acc[k][j >> 1].x;
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 8) red[(wave * 9 + k) * 64 + lane * 8 + j] = s;
    }
  __syncthreads();
  // deterministic mode: acc_out is [VS_BN_STAT_SLOTS][64][9] then, the workgroups of a slot add in index order, a fold kernel sums the
  // slots in order (vs_common.h); mirrors slot_turn / slot_turn_begin / slot_turn_end
  const unsigned slot = blockIdx.x % VS_BN_STAT_SLOTS, rank_in_slot = blockIdx.x / VS_BN_STAT_SLOTS;
  unsigned* my_turn = turn ? turn + VS_TURN_SLOT + slot : nullptr;
  double* dst = turn ? acc_out + (size_t)slot * 576 : acc_out;
  vs_turn_begin(my_turn, rank_in_slot);
  for (int i = threadIdx.x; i < 9 * 64; i += 256) {
    const int k = i / 64, c = i - k * 64;
    atomicAdd(dst + c * 9 + k, (double)(red[(0 * 9 + k) * 64 + c] + red[(1 * 9 + k) * 64 + c] + red[(2 * 9 + k) * 64 + c] + red[(3 * 9 + k) * 64 + c]));
  }
  vs_turn_end(my_turn, rank_in_slot, (gridDim.x - slot + VS_BN_STAT_SLOTS - 1) / VS_BN_STAT_SLOTS);
}

__global__ void fold_slots_f64_kernel(const double* __restrict__ slots, int nslots, int n, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = 0.0;
  for (int k = 0; k < nslots; ++k) v += slots[(size_t)k * n + i];
  out[i] = v;
}

// parameter gradients of cnn1 + its BatchNorm from the sums above and the input moments (one thread per channel, fp64)
__global__ void nhwc_first_bwd_finalize_kernel(const double* __restrict__ acc /* [64][9] */, const double* __restrict__ mom,
                                               const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ scale,
                                               const float* __restrict__ mean, const float* __restrict__ invstd, double count, int train,
                                               float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dbias, float* __restrict__ dw) {
  const int c = threadIdx.x;
  if (c >= 64) return;
  const double sdy = acc[c * 9], sdyx = acc[c * 9 + 1];
  dgamma[c] = (float)sdyx;
  dbeta[c] = (float)sdy;
  const double cA = scale[c];                              // gamma * invstd
  double cB = 0.0, cC = 0.0;
  if (train) {
    cB = -cA * (double)invstd[c] * sdyx / count;
    cC = -cA * sdy / count - cB * (double)mean[c];
  }
  dbias[c] = train ? 0.f : (float)(cA * sdy);              // batch statistics: the gradient of a bias in front of them is exactly zero
  const double b = bias[c];
  for (int k = 0; k < 7; ++k) {
    double zx = b * mom[k];                                // sum z x_k
    for (int k2 = 0; k2 < 7; ++k2) zx += (double)w[c * 7 + k2] * mom_R(mom, k2, k);
    dw[c * 7 + k] = (float)(cA * acc[c * 9 + 2 + k] + cB * zx + cC * mom[k]);
  }
}

// ---- the older backward, from z1 ------------------------------------------------------------------------------------------------------
// BatchNorm backward pass 2 (dz1 = cA dy + cB z + cC, dy = da * act'(z * scale + shift): nhwc_bn.hip) fused with the 1x7 weight
// gradient: dz1 is contracted with the 7 shifted inputs on the spot and never written: acc[c][k] += dz1[b][t][f][c] * x[b][t][f + k - 3]
template <int ACT>
__global__ __launch_bounds__(256)
void nhwc_bn_bwd_first_kernel(const u4v* __restrict__ da, const u4v* __restrict__ z, const float* __restrict__ x,
                              long long npix, int F, const float* __restrict__ scale, const float* __restrict__ shift,
                              const float* __restrict__ coef, double* __restrict__ acc_out /* [64][7] */) {
  __shared__ float red[4 * 7 * 64];
  const int piece = threadIdx.x & 7;
  float sc[8], sh[8], cA[8], cB[8], cC[8], acc[7][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = piece * 8 + j;
    sc[j] = scale[c]; sh[j] = shift[c]; cA[j] = coef[c]; cB[j] = coef[64 + c]; cC[j] = coef[128 + c];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k][j] = 0.f;
  }
  const long long stride = (long long)gridDim.x * 32;     // pixels per sweep of the grid
  const int sr = (int)(stride % F);
  long long p = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  int f = (int)(p % F);
  for (; p < npix; p += stride, f += sr) {
    if (f >= F) f -= F;
    float xv[7];
    gather_x7(x + (p - f), f, F, piece, xv);
    const u4v g = __builtin_nontemporal_load(da + p * 8 + piece), v = __builtin_nontemporal_load(z + p * 8 + piece);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int j = 2 * q + e;
        const float zv = e ? bf_hi(v[q]) : bf_lo(v[q]);
        const float dy = (e ? bf_hi(g[q]) : bf_lo(g[q])) * nhwc_act_grad<ACT>(fmaf(zv, sc[j], sh[j]));
        const float dzv = fmaf(cA[j], dy, fmaf(cB[j], zv, cC[j]));
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[k][j] = fmaf(dzv, xv[k], acc[k][j]);
      }
    }
  }
  // the 7 x 8 form of fold_channel_sums' fold; one fp64 atomic per (channel, tap) and workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = acc[k][j];
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 8) red[(wave * 7 + k) * 64 + lane * 8 + j] = s;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 7 * 64; i += 256) {
    const int k = i / 64, c = i - k * 64;
    atomicAdd(acc_out + c * 7 + k, (double)(red[(0 * 7 + k) * 64 + c] + red[(1 * 7 + k) * 64 + c] + red[(2 * 7 + k) * 64 + c] + red[(3 * 7 + k) * 64 + c]));
  }
}

// ---- the split-f16 forward (conv_nhwc_f16x3.hip: VS_MATH_F16X3, eval BatchNorm) -------------------------------------------------------
// cnn1 computes in fp32 (7 FMAs per output) and writes y * s_y as hi / lo f16 planes; s_y comes from vs_nhwc_first_plan_impl's bound.
typedef _Float16 h2v __attribute__((ext_vector_type(2)));

// out_scale2 <- {s, 1 / s}, s = the power of two that maps max_c (|scale_c| sum_j |w_cj| max|x| + |shift_c|) (>= max |y|) into [2^14, 2^15);
// w = [nco][taps] (cnn1: 64 x 7, cnn8: 8 x 64)
__global__ void nhwc_first_plan_kernel(const unsigned* __restrict__ amax_in, int n_amax, const float* __restrict__ w, const float* __restrict__ scale,
                                       const float* __restrict__ shift, float* __restrict__ out_scale2, int nco, int taps) {
  const int c = threadIdx.x;                                  // 64 threads
  unsigned mb = 0;
  for (int i = c; i < n_amax; i += 64) mb = amax_in[i] > mb ? amax_in[i] : mb;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned other = __shfl_xor(mb, o, 64); mb = other > mb ? other : mb; }
  float bound = 0.3125f;
  if (c < nco) {
    float l1 = 0.f;
    for (int k = 0; k < taps; ++k) l1 += fabsf(w[c * taps + k]);
    bound = fmaxf(fabsf(scale[c]) * l1 * __uint_as_float(mb) + fabsf(shift[c]), 0.3125f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bound = fmaxf(bound, __shfl_xor(bound, o, 64));
  if (c == 0) {      // the power of two that takes the bound's exponent to 15, clamped (nhwc_conv_last_split_kernel has the same for its weights)
    float s = 1.f, si = 1.f;
    if (bound > 0.f && bound < 3.0e38f) {
      int e = 0;
      (void)frexpf(bound, &e);
      int k = 15 - e;
      k = k > 100 ? 100 : (k < -100 ? -100 : k);
      s = ldexpf(1.f, k);
      si = ldexpf(1.f, -k);
    }
    out_scale2[0] = s;
    out_scale2[1] = si;
  }
}

// max |x| of the path's input (any 4-byte alignment: the mixture may be a slice of a batch), folded into *amax (bits of a float >= 0);
// one atomic per workgroup (one per wave made 8192 of them queue up on the one address: 0.1 ms for 46 MB)
__global__ __launch_bounds__(256)
void absmax_any_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ amax) {
  __shared__ float red[4];
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.f) atomicMax(amax, __float_as_uint(m));
  }
}

// nhwc_conv_first_kernel with another store: hi / lo planes of y * s_y, and |max| of y for the next layer's plan
template <int ACT>
__global__ __launch_bounds__(256)
void nhwc_conv_first_split_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                  const float* __restrict__ shift, const float* __restrict__ out_scale2, unsigned short* __restrict__ out_hi,
                                  unsigned short* __restrict__ out_lo, unsigned* __restrict__ amax_out, long long npix, int F) {
  const int piece = threadIdx.x & 7;
  vs_f32x2 wr[4][7], sc[4], sh[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c0 = piece * 8 + 2 * q;
    sc[q] = vs_f32x2{scale[c0], scale[c0 + 1]};
    sh[q] = vs_f32x2{shift[c0], shift[c0 + 1]};
#pragma unroll
    for (int k = 0; k < 7; ++k) wr[q][k] = vs_f32x2{w[c0 * 7 + k], w[(c0 + 1) * 7 + k]};
  }
  const float sy = out_scale2[0];
  float am = 0.f;
  const long long stride = (long long)gridDim.x * 32;     // pixels per sweep of the grid
  const int sr = (int)(stride % F);
  long long p = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  int f = (int)(p % F);
  float mine = p < npix ? load_x7(x + (p - f), f, F, piece) : 0.f;
  for (; p < npix; p += stride) {
    int fn = f + sr;
    if (fn >= F) fn -= F;
    const long long pn = p + stride;
    const float mine_next = pn < npix ? load_x7(x + (pn - fn), fn, F, piece) : 0.f;
    float xv[7];
    exchange_x7(mine, xv);
    mine = mine_next;
    f = fn;
    u4v ph, pl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      vs_f32x2 s2 = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 7; ++k) s2 = __builtin_elementwise_fma(wr[q][k], vs_f32x2{xv[k], xv[k]}, s2);
      vs_f32x2 y = vs_act_fast2<ACT>(__builtin_elementwise_fma(s2, sc[q], sh[q]));
      am = fmaxf(am, fmaxf(fabsf(y.x), fabsf(y.y)));
      y = y * sy;
      const unsigned hb = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(y.x, y.y));
      const h2v h = __builtin_bit_cast(h2v, hb);
      ph[q] = hb;
      pl[q] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(y.x - (float)h[0], y.y - (float)h[1]));
    }
    __builtin_nontemporal_store(ph, reinterpret_cast<u4v*>(out_hi + p * 64 + piece * 8));
    __builtin_nontemporal_store(pl, reinterpret_cast<u4v*>(out_lo + p * 64 + piece * 8));
  }
  vs_absmax_commit(am, amax_out);
}

}  // namespace

int vs_nhwc_conv_first_impl(const float* x, const float* w, const float* scale, const float* shift, void* out,
                            int B, int T, int F, int act, double* bn_stats, hipStream_t stream, const float* bias) {
  VS_REQUIRE(x && w && scale && shift && out, "nhwc conv_first: NULL argument");
  VS_REQUIRE(B > 0 && T > 0 && F > 0, "nhwc conv_first: bad shape");
  const long long npix = (long long)B * T * F;
  // [r6, call 31] 2048 workgroups: 437 us, 4096: 412, 16384: 408, 65536: 508 (per-lane weights), one sweep: 1885
  const dim3 grid(stream_blocks(32, npix, (bn_stats && g_vs_turn) ? 2048 : 8192)), block(256);
  unsigned short* o = reinterpret_cast<unsigned short*>(out);
  if (bn_stats) {
    VS_REQUIRE(act == VS_ACT_NONE, "nhwc conv_first: fused statistics go with no activation");
    hipLaunchKernelGGL((nhwc_conv_first_kernel<VS_ACT_NONE, true>), grid, block, 0, stream, x, w, scale, shift, o, npix, F, bn_stats, bias);
  } else if (int rc = nhwc_dispatch_act(act, "nhwc conv_first", [&](auto A) {
               hipLaunchKernelGGL((nhwc_conv_first_kernel<decltype(A)::value, false>), grid, block, 0, stream, x, w, scale, shift, o, npix, F, nullptr, bias);
             })) return rc;
  VS_LAUNCH_CHECK();
  return 0;
}

// cnn1 by recomputation: the input moments (35 doubles: S[7], R[k <= k'] row by row), the batch statistics of z1 they imply
int vs_nhwc_first_moments_impl(const float* x, int B, int T, int F, double* mom, hipStream_t stream, double* det_slots, int mom_is_zero) {
  VS_REQUIRE(x && mom && B > 0 && T > 0 && F > 0, "nhwc first_moments: bad argument");
  const long long npix = (long long)B * T * F;
  if (!mom_is_zero) VS_CHECK_HIP(hipMemsetAsync(mom, 0, sizeof(double) * kMomN, stream));
  // at most two workgroups per CU: every workgroup ends in 35 fp64 atomics on the SAME 35 addresses, which the L2 serialises (2048
  // workgroups: 90 us for a pass over 46 MB)
  long long nb = (npix + 256 * 16 - 1) / (256 * 16);
  if (nb > 512) nb = 512;
  unsigned* turn = det_slots ? g_vs_turn : nullptr;           // deterministic mode needs the caller's slot scratch ([VS_BN_STAT_SLOTS][64] doubles)
  if (turn) {      // (the full grid: a workgroup waits for the one 64 below it, which was dispatched before it -- see vs_turn_begin)
    VS_CHECK_HIP(hipMemsetAsync(det_slots, 0, sizeof(double) * VS_BN_STAT_SLOTS * 64, stream));
  }
  hipLaunchKernelGGL(nhwc_first_moments_kernel, dim3((unsigned)(nb < 1 ? 1 : nb)), dim3(256), 0, stream, x, npix, F, turn ? det_slots : mom, turn);
  if (turn) hipLaunchKernelGGL(fold_moment_slots_kernel, dim3(1), dim3(64), 0, stream, det_slots, mom);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_nhwc_first_stats_impl(const double* mom, const float* w, const float* bias, double count, double* stats, hipStream_t stream) {
  VS_REQUIRE(mom && w && bias && stats && count > 0, "nhwc first_stats: bad argument");
  hipLaunchKernelGGL(nhwc_first_stats_kernel, dim3(1), dim3(64), 0, stream, mom, w, bias, count, stats);
  VS_LAUNCH_CHECK();
  return 0;
}

// cnn1 + its BatchNorm + activation backward in ONE pass over da1 (z1 recomputed from x): dgamma, dbeta, dbias, dw [64][7].
// scratch: 64 * 9 + 35 doubles
int vs_nhwc_first_bwd_impl(const void* da, const float* x, const float* w, const float* bias, int B, int T, int F, int act, int train,
                           const float* scale, const float* shift, const float* mean, const float* invstd,
                           float* dgamma, float* dbeta, float* dbias, float* dw, double* scratch, hipStream_t stream, const double* moments, double* det_slots) {
  VS_REQUIRE(da && x && w && bias && scale && shift && mean && invstd && dgamma && dbeta && dbias && dw && scratch, "nhwc first_bwd: NULL argument");
  VS_REQUIRE(B > 0 && T > 0 && F > 0, "nhwc first_bwd: bad shape");
  const long long npix = (long long)B * T * F;
  double* acc = scratch;
  VS_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 64 * 9, stream));
  const double* mom = moments;                             // the forward's (vs_forward_train keeps them in the tape), or recomputed here
  if (!mom) {
    if (int rc = vs_nhwc_first_moments_impl(x, B, T, F, scratch + 64 * 9, stream)) return rc;
    mom = scratch + 64 * 9;
  }
  const u4v* g = reinterpret_cast<const u4v*>(da);
  unsigned* turn = det_slots ? g_vs_turn : nullptr;          // deterministic mode needs the caller's slot scratch ([VS_BN_STAT_SLOTS][576] doubles)
  const dim3 grid(stream_blocks(32, npix)), block(256);
  double* sums = turn ? det_slots : acc;
  if (turn) VS_CHECK_HIP(hipMemsetAsync(det_slots, 0, sizeof(double) * VS_BN_STAT_SLOTS * 576, stream));
  if (int rc = nhwc_dispatch_act(act, "nhwc first_bwd", [&](auto A) {
        hipLaunchKernelGGL(nhwc_first_bwd_kernel<decltype(A)::value>, grid, block, 0, stream, g, x, w, bias, npix, F, scale, shift, mean, invstd, sums, turn);
      })) return rc;
  if (turn) hipLaunchKernelGGL(fold_slots_f64_kernel, dim3(3), dim3(192), 0, stream, det_slots, VS_BN_STAT_SLOTS, 576, acc);
  hipLaunchKernelGGL(nhwc_first_bwd_finalize_kernel, dim3(1), dim3(64), 0, stream, acc, mom, w, bias, scale, mean, invstd, (double)npix, train,
                     dgamma, dbeta, dbias, dw);
  VS_LAUNCH_CHECK();
  return 0;
}

// the older backward, second half: the pass that contracts dz1 with the input, dw [64][7] (acc: 448 doubles)
template <int ACT>
static int bn_bwd_first_contract(const void* dy, const void* z, const float* x, long long npix, int F, const float* scale, const float* shift,
                                 const float* coef, double* acc, float* dw, hipStream_t stream) {
  VS_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 448, stream));
  const dim3 grid(stream_blocks(32, npix)), block(256);
  hipLaunchKernelGGL(nhwc_bn_bwd_first_kernel<ACT>, grid, block, 0, stream, reinterpret_cast<const u4v*>(dy), reinterpret_cast<const u4v*>(z),
                     x, npix, F, scale, shift, coef, acc);
  return vs_cvt_f64_f32_impl(acc, dw, 448, stream);
}

// cnn1, from dy (the first pass was done by the kernel that produced dy): finalize + the contraction
int vs_nhwc_bn_bwd_first_from_dy_impl(const void* dy, const void* z, const float* x, int B, int T, int F, int train,
                                      const float* scale, const float* mean, const float* invstd,
                                      float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc /* 448 */,
                                      hipStream_t stream) {
  VS_REQUIRE(dy && z && x && dw && stats && coef && acc, "nhwc bn_bwd_first_from_dy: NULL argument");
  const long long npix = (long long)B * T * F;
  if (int rc = vs_bn_bwd_finalize_impl(stats, VS_BN_STAT_SLOTS, (double)npix, train, 64, scale, mean, invstd, dgamma, dbeta, dbias, coef, stream)) return rc;
  return bn_bwd_first_contract<VS_ACT_NONE>(dy, z, x, npix, F, scale, scale, coef, acc, dw, stream);
}

// cnn1, from da and z1: the statistics pass of nhwc_bn.hip, then the contraction (dz1 is not written)
int vs_nhwc_bn_act_bwd_first_impl(const void* da, const void* z, const float* x, int B, int T, int F, int act, int train,
                                  const float* scale, const float* shift, const float* mean, const float* invstd,
                                  float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc /* 448 */,
                                  hipStream_t stream) {
  VS_REQUIRE(da && z && x && dw && stats && coef && acc, "nhwc bn_act_bwd_first: NULL argument");
  const long long npix = (long long)B * T * F;
  if (int rc = vs_nhwc_bn_bwd_stats_pass("nhwc bn_act_bwd_first", da, z, npix, stream_blocks(512, npix * 8), act, train, scale, shift, mean, invstd,
                                         dgamma, dbeta, dbias, stats, coef, stream)) return rc;
  if (act == VS_ACT_MISH) return bn_bwd_first_contract<VS_ACT_MISH>(da, z, x, npix, F, scale, shift, coef, acc, dw, stream);
  if (act == VS_ACT_RELU) return bn_bwd_first_contract<VS_ACT_RELU>(da, z, x, npix, F, scale, shift, coef, acc, dw, stream);
  return bn_bwd_first_contract<VS_ACT_NONE>(da, z, x, npix, F, scale, shift, coef, acc, dw, stream);
}

int vs_absmax_any_impl(const float* x, long long n, unsigned* amax, hipStream_t stream) {
  VS_REQUIRE(x && amax && n > 0, "absmax: bad argument");
  hipLaunchKernelGGL(absmax_any_kernel, dim3(stream_blocks(256 * 16, n, 1024)), dim3(256), 0, stream, x, n, amax);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_nhwc_first_plan_impl(const unsigned* amax_in, int n_amax, const float* w, const float* scale, const float* shift, float* out_scale2,
                            hipStream_t stream) {
  VS_REQUIRE(amax_in && n_amax > 0 && w && scale && shift && out_scale2, "nhwc first_plan: bad argument");
  hipLaunchKernelGGL(nhwc_first_plan_kernel, dim3(1), dim3(64), 0, stream, amax_in, n_amax, w, scale, shift, out_scale2, 64, 7);
  VS_LAUNCH_CHECK();
  return 0;
}

// the same for cnn8 (8 output channels x 64 taps) when its output is written as the LSTM input GEMM's split operand (nhwc_last.hip
// consumes it; the plan kernel is the one above)
int vs_nhwc_last_plan_impl(const unsigned* amax_in, int n_amax, const float* w, const float* scale, const float* shift, float* out_scale2,
                           hipStream_t stream) {
  VS_REQUIRE(amax_in && n_amax > 0 && w && scale && shift && out_scale2, "nhwc last_plan: bad argument");
  hipLaunchKernelGGL(nhwc_first_plan_kernel, dim3(1), dim3(64), 0, stream, amax_in, n_amax, w, scale, shift, out_scale2, 8, 64);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_nhwc_conv_first_split_impl(const float* x, const float* w, const float* scale, const float* shift, const float* out_scale2,
                                  void* out_hi, void* out_lo, unsigned* amax_out, int B, int T, int F, int act, hipStream_t stream) {
  VS_REQUIRE(x && w && scale && shift && out_scale2 && out_hi && out_lo, "nhwc conv_first_split: NULL argument");
  VS_REQUIRE(B > 0 && T > 0 && F > 0, "nhwc conv_first_split: bad shape");
  const long long npix = (long long)B * T * F;
  const dim3 grid(stream_blocks(32, npix, 8192)), block(256);
  unsigned short* oh = reinterpret_cast<unsigned short*>(out_hi);
  unsigned short* ol = reinterpret_cast<unsigned short*>(out_lo);
  if (int rc = nhwc_dispatch_act(act, "nhwc conv_first_split", [&](auto A) {
        hipLaunchKernelGGL((nhwc_conv_first_split_kernel<decltype(A)::value>), grid, block, 0, stream, x, w, scale, shift, out_scale2, oh, ol, amax_out, npix, F);
      })) return rc;
  VS_LAUNCH_CHECK();
  return 0;
}
