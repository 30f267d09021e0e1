// What the HBM-bound files of the channels-last bf16 / split-f16 path share (nhwc_first.hip: cnn1, nhwc_bn.hip: BatchNorm apply and
// backward, nhwc_last.hip: cnn8).  A pixel is 128 contiguous bytes = eight 16-byte pieces of 8 channels; every streaming kernel gives
// a lane one piece, so a wave moves 1 KiB per instruction and a lane's channels are fixed for the whole launch (grid strides are
// multiples of 8 pieces): per-channel constants live in registers and per-channel sums are per-lane partials, folded once at the end.
// Rule of this header (profiles/nhwc_edge_split.md): a helper is called where the kernel instance keeps its registers, LDS,
// occupancy and instruction stream; where it does not, the site is written out with a comment that names what it mirrors.
#pragma once
#include <type_traits>

#include "vs_internal.h"

// nhwc_bn.hip: memset of the slots, the statistics pass over (da, z) on `nb` workgroups, vs_bn_bwd_finalize_impl.  `site` prefixes
// the refusal of an unsupported activation.
int vs_nhwc_bn_bwd_stats_pass(const char* site, const void* da, const void* z, long long npix, int nb, int act, int train,
                              const float* scale, const float* shift, const float* mean, const float* invstd,
                              float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, hipStream_t stream);

namespace {

typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ vs_f32x2 bf_pair(unsigned u) { return vs_f32x2{bf_lo(u), bf_hi(u)}; }       // the two channels of a 32-bit word
__device__ __forceinline__ vs_f32x2 ld_pair(const float* v, int c) { return vs_f32x2{v[c], v[c + 1]}; }  // per-channel constants c, c + 1 (not in cnn1's kernels: moves them)

// ---- folds ------------------------------------------------------------------------------------------------------------------------
// The workgroups of a launch add to partial-sum slot blockIdx % VS_BN_STAT_SLOTS.  Deterministic mode (turn != NULL): the ones that
// share a slot add in index order (vs_common.h); the atomics go between slot_turn_begin and slot_turn_end.  Called by fold_channel_sums
// and nhwc_conv_last_kernel; nhwc_first_moments_kernel and nhwc_first_bwd_kernel keep the same lines written out.
struct SlotTurn { unsigned slot, rank; unsigned* word; };
__device__ __forceinline__ SlotTurn slot_turn(unsigned* turn) {
  const unsigned slot = blockIdx.x % VS_BN_STAT_SLOTS, rank_in_slot = blockIdx.x / VS_BN_STAT_SLOTS;
  return SlotTurn{slot, rank_in_slot, turn ? turn + VS_TURN_SLOT + slot : nullptr};
}
__device__ __forceinline__ void slot_turn_begin(const SlotTurn& t) { vs_turn_begin(t.word, t.rank); }
__device__ __forceinline__ void slot_turn_end(const SlotTurn& t) {
  vs_turn_end(t.word, t.rank, (gridDim.x - t.slot + VS_BN_STAT_SLOTS - 1) / VS_BN_STAT_SLOTS);
}

// The lane-to-channel fold: per-lane partial sums of a lane's 8 channels (channel piece = lane & 7; v[q][j] for channel 8 * (lane & 7) + j)
// are folded over the eight lanes of a wave that share the piece, land in lds[wave][q][64 channels], and are summed over the four waves.
// This function is the 2 x 8 form and adds the result to stats[slot][channel][which] (doubles).  The 7 x 8, 8 x 8 and 9 x 8 sites
// (nhwc_bn_bwd_first_kernel, nhwc_conv_last_bwd_kernel, nhwc_first_bwd_kernel) are written out where they stand: behind any shared
// form they lose the parent's instruction stream (profiles/nhwc_edge_split.md).
template <int NV>
__device__ __forceinline__ void fold_channel_sums(const float (&v)[NV][8], double* __restrict__ stats, float* lds /* [4 waves][NV][64] */,
                                                  unsigned* turn = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = v[q][j];
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 8) lds[(wave * NV + q) * 64 + lane * 8 + j] = s;
    }
  __syncthreads();
  const SlotTurn st = slot_turn(turn);
  slot_turn_begin(st);
  for (int i = threadIdx.x; i < NV * 64; i += blockDim.x) {
    const int q = i / 64, c = i - q * 64;
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += lds[(w * NV + q) * 64 + c];
    atomicAdd(stats + (size_t)(blockIdx.x % VS_BN_STAT_SLOTS) * 128 + c * 2 + q, (double)s);
  }
  slot_turn_end(st);
}

// ---- the 7 input samples of a cnn1 pixel ------------------------------------------------------------------------------------------
// x[f-3 .. f+3] for all 8 lanes that share the pixel (one lane per 8 channels): lane `piece` loads sample `piece` (one load
// instruction per wave instead of seven mostly redundant ones) and the group exchanges them by lane permutes.
__device__ __forceinline__ float load_x7(const float* xr, int f, int F, int piece) {
  const int ff = f + piece - 3;
  return (piece < 7 && ff >= 0 && ff < F) ? xr[ff] : 0.f;
}
__device__ __forceinline__ void exchange_x7(float mine, float (&xv)[7]) {
  const int base = (int)(threadIdx.x & 56u);               // first lane of the pixel's group inside the wave
#pragma unroll
  for (int k = 0; k < 7; ++k) xv[k] = __shfl(mine, base + k, 64);
}
__device__ __forceinline__ void gather_x7(const float* xr, int f, int F, int piece, float (&xv)[7]) {
  exchange_x7(load_x7(xr, f, F, piece), xv);
}

// ---- activation derivatives -------------------------------------------------------------------------------------------------------
template <int ACT>
__device__ __forceinline__ float nhwc_act_grad(float y) {
  if (ACT == VS_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (ACT == VS_ACT_MISH) return vs_mish_grad_fast(y);
  return 1.f;
}

// Mish' for a pair of channels = r (n + 4 y u (u + 1) r), u = e^y, n = u (u + 2), r = 1 / (n + 2) (the identity derived at
// conv_nhwc.hip's dy epilogue): one exp2 and one rcp per channel, the rest packed; y clamped at 20, where n r = 1 and the second
// term vanishes in fp32 (no selects).  n and r are vs_mish_fast2's, so y * (n * r) is bitwise the activation that
// nhwc_bn_apply_kernel and the PRE form of nhwc_conv_last_kernel store.
struct MishParts2 { vs_f32x2 yc, u, n, r; };
__device__ __forceinline__ MishParts2 nhwc_mish_parts2(vs_f32x2 y) {
  MishParts2 m;
  m.yc = vs_f32x2{fminf(y.x, 20.0f), fminf(y.y, 20.0f)};
  const vs_f32x2 e = m.yc * 1.44269504088896340736f;
  m.u = vs_f32x2{__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
  m.n = m.u * (m.u + 2.0f);
  const vs_f32x2 d = m.n + 2.0f;
  m.r = vs_f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  return m;
}
__device__ __forceinline__ vs_f32x2 nhwc_mish_grad2(const MishParts2& m) {
  return m.r * __builtin_elementwise_fma((m.yc * 4.0f) * m.r, __builtin_elementwise_fma(m.u, m.u, m.u), m.n);
}
template <int ACT>
__device__ __forceinline__ vs_f32x2 nhwc_act_grad2(vs_f32x2 y) {
  if (ACT == VS_ACT_RELU) return vs_f32x2{y.x > 0.f ? 1.f : 0.f, y.y > 0.f ? 1.f : 0.f};
  if (ACT == VS_ACT_MISH) return nhwc_mish_grad2(nhwc_mish_parts2(y));
  return vs_f32x2{1.f, 1.f};
}
// activation and derivative together
template <int ACT>
__device__ __forceinline__ void nhwc_act_both2(vs_f32x2 y, vs_f32x2& a, vs_f32x2& d) {
  if (ACT == VS_ACT_MISH) {
    const MishParts2 m = nhwc_mish_parts2(y);
    a = y * (m.n * m.r);
    d = nhwc_mish_grad2(m);
  } else if (ACT == VS_ACT_RELU) {
    a = vs_f32x2{fmaxf(y.x, 0.0f), fmaxf(y.y, 0.0f)};
    d = vs_f32x2{y.x > 0.0f ? 1.0f : 0.0f, y.y > 0.0f ? 1.0f : 0.0f};
  } else {
    a = y;
    d = vs_f32x2{1.0f, 1.0f};
  }
}

// ---- host: grids and the activation dispatch ----------------------------------------------------------------------------------------
int stream_blocks(long long items_per_block_sweep, long long total, long long cap = 2048) {
  long long nb = (total + items_per_block_sweep - 1) / items_per_block_sweep;
  if (nb > cap) nb = cap;
  return nb < 1 ? 1 : (int)nb;
}
// The pure elementwise passes (no sums, no per-block flush): ONE sweep -- a workgroup per `items_per_block_sweep`, no grid-stride loop.
// [r6, calls 28-29] A 2048-block grid-stride loop over a 1.48 GB tensor (stride 8 MB) reads and writes at 4.7-5.3 TB/s; the same kernel
// launched with a workgroup per 512 pieces at 6.35 (BatchNorm apply 0.627 -> 0.467 ms, the backward pass from dy 0.918 -> 0.758), and the
// rate rises monotonically with the grid in between (tools/stream_probe.hip, profiles/r06_experiments.md section 15): workgroups dispatched in
// index order walk the tensor as one front, a strided loop keeps 2048 fronts 4 KB wide in flight.
int stream_blocks_wide(long long items_per_block_sweep, long long total) {
  long long nb = (total + items_per_block_sweep - 1) / items_per_block_sweep;
  if (nb > (1LL << 24)) nb = 1LL << 24;
  return nb < 1 ? 1 : (int)nb;
}

// launch(std::integral_constant<int, ACT>) for act = Mish / ReLU / none; anything else is refused as "<site>: unsupported activation"
template <class LAUNCH>
int nhwc_dispatch_act(int act, const char* site, LAUNCH&& launch) {
  if (act == VS_ACT_MISH) launch(std::integral_constant<int, VS_ACT_MISH>());
  else if (act == VS_ACT_RELU) launch(std::integral_constant<int, VS_ACT_RELU>());
  else if (act == VS_ACT_NONE) launch(std::integral_constant<int, VS_ACT_NONE>());
  else VS_REQUIRE(false, "%s: unsupported activation %d", site, act);
  return 0;
}

}  // namespace
