// cnn8 (models/voicesplit/model.py:51-52) + transpose/view (:72-74) of the channels-last paths:
// [B][T][F][64] -> [B][T][8][F] fp32 (the LSTM feature layout) or the LSTM input GEMM's operand rows, from bf16 (VS_MATH_BF16) or
// from hi / lo f16 planes (the split-f16 forward), and its backward in one pass over a7 / z7.
#include "nhwc_common.h"

namespace {

// ---- the block walk of both forwards ------------------------------------------------------------------------------------------------
// One wave = a block of 16 pixels of a row per step, four waves per workgroup.  (row, block column) are carried along: one division
// per launch.  Workgroups go round the 8 XCDs: the ones of an XCD take neighbouring blocks, so that the 32- and 64-byte pieces of an
// output line meet in ONE L2 instead of leaving eight of them as partial writes.  The ten lines of setup stay written out in both
// kernels (as a function that returns the walk they move both kernels' streams: profiles/nhwc_edge_split.md).

// ---- forward, bf16 ------------------------------------------------------------------------------------------------------------------
// out[b][t][co][f] = act(scale[co] * sum_ci w[co][ci] in[b][t][f][ci] + shift[co]), co < 8.  One wave = 16 pixels of a
// row per step: the B operand of v_mfma_f32_16x16x32_bf16 is the pixels as they lie in memory (lane = (pixel, 8
// channels) = one 16-byte load), A = the 8 x 64 weights zero-padded to 16 rows; C rows 0..7 -> 8 feature rows.
// STATS: the per-channel sum and sum of squares of what is stored (train-mode BatchNorm of cnn8: models/voicesplit/model.py:52)
// accumulate per lane over the launch and flush once: stats[slot = block % VS_BN_STAT_SLOTS][8 channels][2] doubles
// (vs_bn_finalize_impl folds the slots).  Replaces a pass over the 370 MB feature tensor.
// PRE >= 0: `in` is the UN-normalised output z7 of the layer below and the kernel applies that layer's BatchNorm +
// activation PRE on its way into the matrix pipe (a7 = act(z7 * pre_scale + pre_shift), rounded to bf16 exactly as
// nhwc_bn_apply_kernel would have stored it): cnn8 is an HBM-bound consumer with idle VALU, so the training step needs no
// BatchNorm-apply pass for cnn7 and no a7 tensor at all (the backward recomputes it the same way).
template <int ACT, bool STATS = false, int PRE = -1>
__global__ __launch_bounds__(256)
void nhwc_conv_last_kernel(const unsigned short* __restrict__ in, const float* __restrict__ w, const float* __restrict__ scale,
                           const float* __restrict__ shift, float* __restrict__ out, long long nrows /* B*T */, int F,
                           double* __restrict__ stats, const float* __restrict__ pre_scale = nullptr, const float* __restrict__ pre_shift = nullptr,
                           unsigned short* __restrict__ rows_bf16 = nullptr, int Kp = 0, unsigned* turn = nullptr) {
  // rows_bf16 != NULL (eval forward, whole path): the output goes out as the bf16 A operand of the LSTM input GEMM instead -- rows
  // [nrows][Kp] (element co * F + f of row (b, t), the K padding zeroed by the wave that owns a row's first block), `out` unused
  __shared__ float red[4 * 16];
  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  vs_f32x2 psc[2][4], psh[2][4];      // PRE: constants of this lane's 16 channels (k-chunk kc: 32 kc + 8 g + 2 q, + 1)
  if (PRE >= 0) {
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ch = kc * 32 + g * 8 + 2 * q;
        psc[kc][q] = ld_pair(pre_scale, ch);
        psh[kc][q] = ld_pair(pre_shift, ch);
      }
  }
  vs_bf16x8 wa[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc)
#pragma unroll
    for (int j = 0; j < 8; ++j) wa[kc][j] = (__bf16)(n < 8 ? w[n * 64 + kc * 32 + g * 8 + j] : 0.f);
  float sc[4], sh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = (g * 4 + r) & 7;
    sc[r] = scale[co];
    sh[r] = shift[co];
  }
  const int blocks_per_row = (F + 15) >> 4;
  const long long nblk = nrows * blocks_per_row;
  const long long wstride = (long long)gridDim.x * 4;
  const long long sq = wstride / blocks_per_row;
  const int sr = (int)(wstride - sq * blocks_per_row);
  const int per_xcd = gridDim.x >> 3;
  const int vblock = (gridDim.x & 7) == 0 ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  long long blk = (long long)vblock * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  long long row = blk / blocks_per_row;
  int bc = (int)(blk - row * blocks_per_row);
  for (; blk < nblk; blk += wstride, row += sq, bc += sr) {
    if (bc >= blocks_per_row) { bc -= blocks_per_row; ++row; }
    const int f = bc * 16 + n;
    const bool ok = f < F;
    const u4v* src = reinterpret_cast<const u4v*>(in + ((row * F + (ok ? f : 0)) << 6)) + g;
    u4v b0 = ok ? src[0] : u4v{0u, 0u, 0u, 0u}, b1 = ok ? src[4] : u4v{0u, 0u, 0u, 0u};
    if (PRE >= 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const vs_f32x2 y0 = vs_act_fast2<(PRE >= 0 ? PRE : VS_ACT_NONE)>(__builtin_elementwise_fma(bf_pair(b0[q]), psc[0][q], psh[0][q]));
        const vs_f32x2 y1 = vs_act_fast2<(PRE >= 0 ? PRE : VS_ACT_NONE)>(__builtin_elementwise_fma(bf_pair(b1[q]), psc[1][q], psh[1][q]));
        b0[q] = vs_pack_bf16(y0.x, y0.y);
        b1[q] = vs_pack_bf16(y1.x, y1.y);
      }
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[0], __builtin_bit_cast(vs_bf16x8, b0), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[1], __builtin_bit_cast(vs_bf16x8, b1), c, 0, 0, 0);
    if (!STATS && PRE < 0 && rows_bf16) {
      if (ok && g < 2) {
        unsigned short* o = rows_bf16 + (size_t)row * Kp + (size_t)(g * 4) * F + f;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(size_t)r * F] = (unsigned short)(vs_pack_bf16(vs_act_fast<ACT>(fmaf(c[r], sc[r], sh[r])), 0.f) & 0xffffu);
      }
      if (bc == 0)
        for (int k = 8 * F + lane; k < Kp; k += 64) rows_bf16[(size_t)row * Kp + k] = 0;
    } else if (ok && g < 2) {
      float* o = out + (row * 8 + g * 4) * F + f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = vs_act_fast<ACT>(fmaf(c[r], sc[r], sh[r]));
        o[(size_t)r * F] = v;
        if (STATS) { ssum[r] += v; ssq[r] = fmaf(v, v, ssq[r]); }
      }
    }
  }
  if (STATS) {
    // lanes (g, n): channel 4 g + r for g < 2; fold the 16 columns of a group, then the four waves
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float a = ssum[r], b = ssq[r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
      if (n == 0 && g < 2) { red[wave * 16 + (g * 4 + r) * 2] = a; red[wave * 16 + (g * 4 + r) * 2 + 1] = b; }
    }
    __syncthreads();
    const SlotTurn st = slot_turn(turn);
    slot_turn_begin(st);
    if (threadIdx.x < 16)
      atomicAdd(stats + (size_t)st.slot * 16 + threadIdx.x,
                (double)red[threadIdx.x] + (double)red[16 + threadIdx.x] + (double)red[32 + threadIdx.x] + (double)red[48 + threadIdx.x]);
    slot_turn_end(st);
  }
}

// ---- forward, split f16 (conv_nhwc_f16x3.hip: VS_MATH_F16X3, eval BatchNorm) -------------------------------------------------------
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));

// out[b][t][co][f] = act(scale[co] * sum_ci w[co][ci] x[b][t][f][ci] + shift[co]), co < 8, x = (in_hi + in_lo) / s_x: the planes of
// cnn7's output.  B operands = the two planes' pixels as they lie in memory, A = the weights (rows 8..15 repeat rows 0..7)
// split into hi / lo after a power-of-two scale found here (512 values: one wave reduction); three products, fp32 accumulate.
// ROWS: the output goes out as the LSTM input GEMM's A operand instead -- hi / lo f16 rows [nrows][Kp] of out * out_scale2[0] (element
// co * F + f of row (b, t): the feature order of the fp32 form), columns 8 F .. Kp zeroed by the workgroups that own a row's first block.
template <int ACT, bool ROWS>
__global__ __launch_bounds__(256)
void nhwc_conv_last_split_kernel(const unsigned short* __restrict__ in_hi, const unsigned short* __restrict__ in_lo, const float* __restrict__ in_scale2,
                                 const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                                 float* __restrict__ out, long long nrows, int F,
                                 unsigned short* __restrict__ row_hi, unsigned short* __restrict__ row_lo, int Kp, const float* __restrict__ out_scale2) {
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  float wv[2][8], wmax = 0.f;
#pragma unroll
  for (int kc = 0; kc < 2; ++kc)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wv[kc][j] = w[(n & 7) * 64 + kc * 32 + g * 8 + j];      // A rows 8..15 repeat 0..7: accumulator rows g >= 2 repeat g - 2
      wmax = fmaxf(wmax, fabsf(wv[kc][j]));
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o, 64));
  float sw = 1.f, swi = 1.f;                                 // the power of two that takes |w|max's exponent to 10 (cf. nhwc_first_plan_kernel)
  if (wmax > 0.f && wmax < 3.0e38f) {
    int e = 0;
    (void)frexpf(wmax, &e);
    sw = ldexpf(1.f, 10 - e);
    swi = ldexpf(1.f, e - 10);
  }
  h8v wh[2], wl[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = wv[kc][j] * sw;
      wh[kc][j] = (_Float16)v;
      wl[kc][j] = (_Float16)(v - (float)wh[kc][j]);
    }
  const float inv = in_scale2[1] * swi;
  float sc[4], sh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = (g * 4 + r) & 7;
    sc[r] = scale[co] * inv;
    sh[r] = shift[co];
  }
  const float so = ROWS ? out_scale2[0] : 1.f;
  const int blocks_per_row = (F + 15) >> 4;
  const long long nblk = nrows * blocks_per_row;
  const long long wstride = (long long)gridDim.x * 4;
  const long long sq = wstride / blocks_per_row;
  const int sr = (int)(wstride - sq * blocks_per_row);
  const int per_xcd = gridDim.x >> 3;
  const int vblock = (gridDim.x & 7) == 0 ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  long long blk = (long long)vblock * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  long long row = blk / blocks_per_row;
  int bc = (int)(blk - row * blocks_per_row);
  const u4v z4 = {0u, 0u, 0u, 0u};
  // the next block's pixels are loaded before this one is contracted (the loop is otherwise load -> wait -> 6 MFMAs -> store)
  u4v h0 = z4, h1 = z4, l0 = z4, l1 = z4;
  auto fetch = [&](long long r, int c, u4v& a0, u4v& a1, u4v& b0, u4v& b1) {
    const int f = c * 16 + n;
    if (f < F) {
      const size_t e0 = (size_t)((r * F + f) << 6);
      const u4v* sh_ = reinterpret_cast<const u4v*>(in_hi + e0) + g;
      const u4v* sl_ = reinterpret_cast<const u4v*>(in_lo + e0) + g;
      a0 = __builtin_nontemporal_load(sh_); a1 = __builtin_nontemporal_load(sh_ + 4);
      b0 = __builtin_nontemporal_load(sl_); b1 = __builtin_nontemporal_load(sl_ + 4);
    } else {
      a0 = a1 = b0 = b1 = z4;
    }
  };
  if (blk < nblk) fetch(row, bc, h0, h1, l0, l1);
  for (; blk < nblk; blk += wstride) {
    long long rown = row + sq;
    int bcn = bc + sr;
    if (bcn >= blocks_per_row) { bcn -= blocks_per_row; ++rown; }
    u4v nh0 = z4, nh1 = z4, nl0 = z4, nl1 = z4;
    if (blk + wstride < nblk) fetch(rown, bcn, nh0, nh1, nl0, nl1);
    const int f = bc * 16 + n;
    const bool ok = f < F;
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[0], __builtin_bit_cast(h8v, h0), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[1], __builtin_bit_cast(h8v, h1), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[0], __builtin_bit_cast(h8v, l0), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[1], __builtin_bit_cast(h8v, l1), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[0], __builtin_bit_cast(h8v, h0), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[1], __builtin_bit_cast(h8v, h1), c, 0, 0, 0);
    if (ROWS) {
      if (ok) {                                                 // lanes g < 2 write the hi halves, their repeats (g >= 2) the lo halves
        unsigned short* dst = (g < 2 ? row_hi : row_lo) + (size_t)row * Kp + (size_t)((g & 1) * 4) * F + f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = vs_act_fast<ACT>(fmaf(c[r], sc[r], sh[r])) * so;
          const _Float16 vh = __builtin_bit_cast(h2v, __builtin_amdgcn_cvt_pkrtz(v, 0.f))[0];
          const _Float16 vl = __builtin_bit_cast(h2v, __builtin_amdgcn_cvt_pkrtz(v - (float)vh, 0.f))[0];
          dst[(size_t)r * F] = __builtin_bit_cast(unsigned short, g < 2 ? vh : vl);
        }
      }
      if (bc == 0) {                                         // this wave owns the row's padding
        for (int k = 8 * F + lane; k < Kp; k += 64) {
          row_hi[(size_t)row * Kp + k] = 0;
          row_lo[(size_t)row * Kp + k] = 0;
        }
      }
    } else if (ok && g < 2) {
      float* o = out + (row * 8 + g * 4) * F + f;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(size_t)r * F] = vs_act_fast<ACT>(fmaf(c[r], sc[r], sh[r]));
    }
    h0 = nh0; h1 = nh1; l0 = nl0; l1 = nl1;
    row = rown; bc = bcn;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// One pass over a7: din[b][t][f][ci] = sum_co w[co][ci] dz8[b][t][co][f]  (data gradient, bf16) and
// dw[co][ci] = sum_pixels dz8[..][co][..] a7[..][ci]  (weight gradient: per-workgroup partial sums part[block][co][ci])
// DYACT >= 0: the data gradient is turned into dy = din * act'(z7 * scale + shift) before it is stored, and the
// per-channel sums of dy and dy * xhat go to bn_stats (the first pass of cnn7's BatchNorm backward, fused)
struct LastBwdBn {
  const u4v* z;
  const float *scale, *shift, *mean, *invstd;
  double* stats;
  unsigned* turn;          // deterministic mode: the statistics are flushed in workgroup order; else NULL
};

// RECOMP: a7 is not read but recomputed from z7 (a7 = bf16(act(z7 * scale + shift)), the forward's own values: see
// nhwc_conv_last_kernel's PRE form) -- one 1.48 GB operand stream less
// Round 4: channel PAIRS throughout (v_pk_fma_f32: the 64 + 64 FMAs of the data and weight gradient and the activation /
// derivative were ~310 VALU instructions per pixel piece -- the kernel ran at 3 TB/s, VALU-bound), and the next pixel's
// operands are in flight while this one is computed (2 waves per SIMD do not hide a load issued at the top of its own iteration).
template <int DYACT, bool RECOMP = false>
__global__ __launch_bounds__(256)
void nhwc_conv_last_bwd_kernel(const float* __restrict__ dz8, const float* __restrict__ w, const u4v* __restrict__ a7,
                               u4v* __restrict__ din, float* __restrict__ part, long long npix, int F, LastBwdBn bn) {
  __shared__ float red[4 * 8 * 64];
  const int piece = threadIdx.x & 7;
  vs_f32x2 wr[8][4], acc[8][4];            // [co][pair], ci = 8 piece + 2 pair + {0, 1}
  vs_f32x2 sc[4], sh[4], mu[4], is[4], bacc[2][4];
#pragma unroll
  for (int co = 0; co < 8; ++co)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      wr[co][q] = ld_pair(w, co * 64 + piece * 8 + 2 * q);
      acc[co][q] = vs_f32x2{0.f, 0.f};
    }
  if (DYACT >= 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = piece * 8 + 2 * q;
      sc[q] = ld_pair(bn.scale, c); sh[q] = ld_pair(bn.shift, c);
      mu[q] = ld_pair(bn.mean, c); is[q] = ld_pair(bn.invstd, c);
      bacc[0][q] = vs_f32x2{0.f, 0.f}; bacc[1][q] = vs_f32x2{0.f, 0.f};
    }
  }
  const long long stride = (long long)gridDim.x * 32;
  const int sr = (int)(stride % F);
  const long long sq = stride / F;
  long long p = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  long long row = p / F;
  int f = (int)(p - row * F);
  // operands of a pixel piece, fetched one iteration ahead
  struct In { float d[8]; u4v zv, av; };
  auto fetch = [&](long long pq, long long rq, int fq, In& in) {
    const float* dzr = dz8 + rq * 8 * F + fq;
#pragma unroll
    for (int co = 0; co < 8; ++co) in.d[co] = dzr[(size_t)co * F];
    if (DYACT >= 0) in.zv = __builtin_nontemporal_load(bn.z + pq * 8 + piece);
    if (!RECOMP) in.av = __builtin_nontemporal_load(a7 + pq * 8 + piece);
  };
  In cur, nxt;
  cur.zv = cur.av = nxt.zv = nxt.av = u4v{0u, 0u, 0u, 0u};
  if (p < npix) fetch(p, row, f, cur);
  for (; p < npix; p += stride) {
    int fn = f + sr;
    long long rown = row + sq;
    if (fn >= F) { fn -= F; ++rown; }
    const long long pn = p + stride;
    if (pn < npix) fetch(pn, rown, fn, nxt);
    vs_f32x2 zf[4], dact[4];
    u4v av = cur.av;
    if (DYACT >= 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        zf[q] = bf_pair(cur.zv[q]);
        vs_f32x2 aq;
        nhwc_act_both2<(DYACT >= 0 ? DYACT : VS_ACT_NONE)>(__builtin_elementwise_fma(zf[q], sc[q], sh[q]), aq, dact[q]);
        if (RECOMP) av[q] = vs_pack_bf16(aq.x, aq.y);
      }
    }
    vs_f32x2 g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = vs_f32x2{0.f, 0.f};
#pragma unroll
    for (int co = 0; co < 8; ++co) {
      const vs_f32x2 dd = {cur.d[co], cur.d[co]};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        g[q] = __builtin_elementwise_fma(wr[co][q], dd, g[q]);
        acc[co][q] = __builtin_elementwise_fma(dd, bf_pair(av[q]), acc[co][q]);
      }
    }
    if (DYACT >= 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        g[q] *= dact[q];
        bacc[0][q] += g[q];
        bacc[1][q] = __builtin_elementwise_fma(g[q], (zf[q] - mu[q]) * is[q], bacc[1][q]);
      }
    }
    __builtin_nontemporal_store(u4v{vs_pack_bf16(g[0].x, g[0].y), vs_pack_bf16(g[1].x, g[1].y), vs_pack_bf16(g[2].x, g[2].y), vs_pack_bf16(g[3].x, g[3].y)},
                                din + p * 8 + piece);
    cur = nxt;
    f = fn;
    row = rown;
  }
  if (DYACT >= 0) {
    float b8[2][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      b8[0][2 * q] = bacc[0][q].x; b8[0][2 * q + 1] = bacc[0][q].y;
      b8[1][2 * q] = bacc[1][q].x; b8[1][2 * q + 1] = bacc[1][q].y;
    }
    fold_channel_sums<2>(b8, bn.stats, red, bn.turn);
    __syncthreads();
  }
  // the 8 x 8 form of fold_channel_sums' fold, into the workgroup's partial sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int co = 0; co < 8; ++co)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = (j & 1) ? acc[co][j >> 1].y : acc[co][j >> 1].x;
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 8) red[(wave * 8 + co) * 64 + lane * 8 + j] = s;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += 256) part[(size_t)blockIdx.x * 512 + i] = red[i] + red[512 + i] + red[1024 + i] + red[1536 + i];
}

}  // namespace

int vs_nhwc_conv_last_impl(const void* in, const float* w, const float* scale, const float* shift, float* out,
                           int B, int T, int F, int act, hipStream_t stream, double* bn_stats,
                           const float* pre_scale, const float* pre_shift, int pre_act, void* rows_bf16, int Kp) {
  VS_REQUIRE(in && w && scale && shift && (out || rows_bf16), "nhwc conv_last: NULL argument");
  VS_REQUIRE(!rows_bf16 || (!bn_stats && !pre_scale && Kp >= 8 * F), "nhwc conv_last: the row form is the plain eval layer's (Kp = %d)", Kp);
  unsigned short* rb = reinterpret_cast<unsigned short*>(rows_bf16);
  VS_REQUIRE(!pre_scale == !pre_shift, "nhwc conv_last: pre_scale and pre_shift come together");
  VS_REQUIRE(B > 0 && T > 0 && F > 0, "nhwc conv_last: bad shape");
  const long long nrows = (long long)B * T;
  const long long nblk = nrows * ((F + 15) / 16);
  // [r6, call 31] 2048 workgroups: 427 us, 4096: 411, 8192: 403, 16384: 444 (the statistics flush), 32768: 548; deterministic mode keeps 2048 (its
  // workgroups take turns per statistics slot: 128 turns instead of 32 cost the step 1.4 ms)
  const dim3 grid(stream_blocks(4, nblk, (bn_stats && g_vs_turn) ? 2048 : 8192)), block(256);
  const unsigned short* i = reinterpret_cast<const unsigned short*>(in);
  const float* nof = nullptr;
  if (pre_scale) {     // `in` is z7: the layer below's BatchNorm + activation applied on the way in; output unactivated (+ statistics)
    VS_REQUIRE(act == VS_ACT_NONE, "nhwc conv_last: the pre-activation form writes the unactivated output");
    VS_REQUIRE(pre_act == VS_ACT_MISH || pre_act == VS_ACT_RELU, "nhwc conv_last: pre-activation %d", pre_act);
    auto pre = [&](auto ST, auto PRE) {
      hipLaunchKernelGGL((nhwc_conv_last_kernel<VS_ACT_NONE, decltype(ST)::value, decltype(PRE)::value>), grid, block, 0, stream, i, w, scale, shift, out, nrows, F,
                         bn_stats, pre_scale, pre_shift, (unsigned short*)nullptr, 0, decltype(ST)::value ? g_vs_turn : (unsigned*)nullptr);
    };
    auto with_stats = [&](auto ST) {
      if (pre_act == VS_ACT_MISH) pre(ST, std::integral_constant<int, VS_ACT_MISH>());
      else pre(ST, std::integral_constant<int, VS_ACT_RELU>());
    };
    if (bn_stats) with_stats(std::true_type());
    else with_stats(std::false_type());
  } else if (bn_stats) {      // train mode: z8 = conv + bias unactivated, statistics of it ([VS_BN_STAT_SLOTS][8][2] doubles, zeroed by the caller)
    VS_REQUIRE(act == VS_ACT_NONE, "nhwc conv_last: statistics are those of the unactivated output");
    hipLaunchKernelGGL((nhwc_conv_last_kernel<VS_ACT_NONE, true>), grid, block, 0, stream, i, w, scale, shift, out, nrows, F, bn_stats,
                       nof, nof, (unsigned short*)nullptr, 0, g_vs_turn);
  } else if (int rc = nhwc_dispatch_act(act, "nhwc conv_last", [&](auto A) {
               hipLaunchKernelGGL(nhwc_conv_last_kernel<decltype(A)::value>, grid, block, 0, stream, i, w, scale, shift, out, nrows, F, (double*)nullptr, nof, nof, rb, Kp);
             })) return rc;
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_nhwc_conv_last_split_impl(const void* in_hi, const void* in_lo, const float* in_scale2, const float* w, const float* scale,
                                 const float* shift, float* out, int B, int T, int F, int act, hipStream_t stream,
                                 void* row_hi, void* row_lo, int Kp, const float* out_scale2) {
  VS_REQUIRE(in_hi && in_lo && in_scale2 && w && scale && shift && (out || row_hi), "nhwc conv_last_split: NULL argument");
  VS_REQUIRE(B > 0 && T > 0 && F > 0, "nhwc conv_last_split: bad shape");
  VS_REQUIRE(!row_hi || (row_lo && out_scale2 && Kp >= 8 * F), "nhwc conv_last_split: bad row-form arguments (Kp = %d)", Kp);
  const long long nrows = (long long)B * T;
  const long long nblk = nrows * ((F + 15) / 16);
  const dim3 grid(stream_blocks(4, nblk, 8192)), block(256);
  const unsigned short* ih = reinterpret_cast<const unsigned short*>(in_hi);
  const unsigned short* il = reinterpret_cast<const unsigned short*>(in_lo);
  unsigned short* rh = reinterpret_cast<unsigned short*>(row_hi);
  unsigned short* rl = reinterpret_cast<unsigned short*>(row_lo);
  if (int rc = nhwc_dispatch_act(act, "nhwc conv_last_split", [&](auto A) {
        if (rh) hipLaunchKernelGGL((nhwc_conv_last_split_kernel<decltype(A)::value, true>), grid, block, 0, stream, ih, il, in_scale2, w, scale, shift, out, nrows, F, rh, rl, Kp, out_scale2);
        else hipLaunchKernelGGL((nhwc_conv_last_split_kernel<decltype(A)::value, false>), grid, block, 0, stream, ih, il, in_scale2, w, scale, shift, out, nrows, F, rh, rl, Kp, out_scale2);
      })) return rc;
  VS_LAUNCH_CHECK();
  return 0;
}

// cnn8 backward: dz8 [B][T][8][F] fp32, a7 [B][T][F][64] bf16 -> din (bf16, same layout as a7) and dw [8][64];
// part: VS_NHWC_LAST_BWD_BLOCKS x 512 floats of scratch
// z7 != NULL: din is dy7 = da7 * act'(z7 * bn_scale + bn_shift) and bn_stats ([VS_BN_STAT_SLOTS][64][2] doubles, zeroed
// by the caller) receives the sums the BatchNorm backward of cnn7 starts from (vs_nhwc_bn_bwd_from_dy_impl)
int vs_nhwc_conv_last_bwd_impl(const float* dz8, const float* w, const void* a7, void* din, float* part, float* dw,
                               int B, int T, int F, const void* z7, int act, const float* bn_scale, const float* bn_shift,
                               const float* bn_mean, const float* bn_invstd, double* bn_stats, hipStream_t stream) {
  VS_REQUIRE(dz8 && w && din && part && dw, "nhwc conv_last_bwd: NULL argument");
  VS_REQUIRE(a7 || z7, "nhwc conv_last_bwd: a7 may only be NULL in the dy form (it is then recomputed from z7)");
  VS_REQUIRE(!z7 || (bn_scale && bn_shift && bn_mean && bn_invstd && bn_stats), "nhwc conv_last_bwd: the dy form needs the BatchNorm constants and statistics slots");
  const long long npix = (long long)B * T * F;
  long long nb = (npix + 31) / 32;
  if (nb > VS_NHWC_LAST_BWD_BLOCKS) nb = VS_NHWC_LAST_BWD_BLOCKS;
  const LastBwdBn bn{reinterpret_cast<const u4v*>(z7), bn_scale, bn_shift, bn_mean, bn_invstd, bn_stats, z7 ? g_vs_turn : nullptr};
  const dim3 grid((unsigned)nb), block(256);
  const u4v* a = reinterpret_cast<const u4v*>(a7);
  u4v* o = reinterpret_cast<u4v*>(din);
  // (its own chain: the dy form exists for Mish and ReLU only, each with a7 read or recomputed, and refuses in its own words)
  if (!z7) hipLaunchKernelGGL(nhwc_conv_last_bwd_kernel<-1>, grid, block, 0, stream, dz8, w, a, o, part, npix, F, bn);
  else if (act == VS_ACT_MISH && !a7) hipLaunchKernelGGL((nhwc_conv_last_bwd_kernel<VS_ACT_MISH, true>), grid, block, 0, stream, dz8, w, a, o, part, npix, F, bn);
  else if (act == VS_ACT_RELU && !a7) hipLaunchKernelGGL((nhwc_conv_last_bwd_kernel<VS_ACT_RELU, true>), grid, block, 0, stream, dz8, w, a, o, part, npix, F, bn);
  else if (act == VS_ACT_MISH) hipLaunchKernelGGL(nhwc_conv_last_bwd_kernel<VS_ACT_MISH>, grid, block, 0, stream, dz8, w, a, o, part, npix, F, bn);
  else if (act == VS_ACT_RELU) hipLaunchKernelGGL(nhwc_conv_last_bwd_kernel<VS_ACT_RELU>, grid, block, 0, stream, dz8, w, a, o, part, npix, F, bn);
  else VS_REQUIRE(false, "nhwc conv_last_bwd: dy form for activation %d", act);
  VS_LAUNCH_CHECK();
  return vs_reduce_partials_impl(part, (int)nb, 512, dw, stream);
}
