// What conv_f16x3.hip (weight packing, one-tile-per-workgroup kernels) and conv_f16x3_pk.hip (persistent 5x5 kernel) share: the
// packed-weight layout both sides must agree on, the hi / lo split, and the launchers' activation dispatch.  Rule of this header
// (profiles/conv_f16x3_trim.md): a helper is called where every kernel instance keeps its registers, LDS, occupancy and
// instruction stream.
#pragma once
#include <type_traits>

#include "vs_common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kCo = 64;
constexpr int kCi = 64;
constexpr int kChunk = 16;              // input channels per LDS stage = K of one MFMA
constexpr int kNChunk = kCi / kChunk;   // 4
constexpr unsigned kOob = 0x7FFFFFF0u;  // a byte offset no buffer descriptor of these kernels covers: the load returns 0, the store is dropped
constexpr int kTileF = 32;
// packed weight layout: [chunk][tap][cb(2)][part(2)][lane(64)][8 x f16]; element j of the lane vector:
//   part(W[co = cb*32 + (lane&31)][ci = chunk*16 + 8*(lane>>5) + j][kt][kf] * s_w),   part 0 = hi, 1 = lo
constexpr int kTapBytes = 2 * 2 * 64 * 16;   // one (chunk, tap): 2 co blocks x 2 parts x 64 lanes x 16 B
constexpr int kTapVec = kTapBytes / 16;      // 256 x 16 B per tap

__device__ __forceinline__ void split2(float x0, float x1, f16x2& hi, f16x2& lo) {
  hi = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(x0, x1));
  lo = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(x0 - (float)hi[0], x1 - (float)hi[1]));
}

// launch(std::integral_constant<int, ACT>()) for the activation code `act`; host code (the form of nhwc_dispatch_act)
template <typename LAUNCH>
int conv_f16x3_dispatch_act(int act, const char* site, LAUNCH&& launch) {
  if (act == VS_ACT_RELU) launch(std::integral_constant<int, VS_ACT_RELU>());
  else if (act == VS_ACT_MISH) launch(std::integral_constant<int, VS_ACT_MISH>());
  else if (act == VS_ACT_NONE) launch(std::integral_constant<int, VS_ACT_NONE>());
  else VS_REQUIRE(false, "%s: unknown activation %d", site, act);
  return 0;
}

}  // namespace
