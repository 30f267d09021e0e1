// Device code shared by mix.hip (vs_trim_bounds) and mix_seq.hip (vs_split_point): the frame energies of librosa's silence
// detection (frame_length 2048, hop_length 512, centred frames, reflect padding) as fp64 sums of 512-sample blocks.
#pragma once
#include "vs_common.h"

namespace {

constexpr int kFrame = 2048, kHop = 512, kPad = kFrame / 2;
constexpr int kMinClip = kPad + 1;                     // the reflection needs y[1024]
constexpr long long kMaxClip = 1LL << 30;              // bounds are int32
constexpr double kAmin = 1e-10;                        // power_to_db(amin=1e-10)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One wave: the sum of squares (fp64; fp32 squares are exact in fp64) of block b of the reflect-padded region y = samples[off : off + n],
// n >= 1025: padded samples [512 b, 512 b + 512) = region samples k0 .. k0 + 511, k0 = 512 b - 1024.  A block inside the region is read
// with 16-byte loads from the first 16-byte boundary on (the base of `samples` is 16-byte aligned, `off` is arbitrary), the up to three
// samples in front and behind by single lanes; a block that touches the padding indexes sample by sample and never leaves [0, n) of
// its own region.  Every lane returns the sum.
__device__ __forceinline__ double block_sumsq(const float* __restrict__ samples, long long off, int n, int b, int lane) {
  const float* __restrict__ y = samples + off;
  const int k0 = b * kHop - kPad;
  double acc = 0.0;
  if (k0 >= 0 && k0 + kHop <= n) {
    const long long g0 = off + k0;                                     // index in the flat buffer
    const int head = (int)((4 - (g0 & 3)) & 3);                        // samples in front of the first 16-byte boundary
    const int nvec = (kHop - head) >> 2, tail = (kHop - head) & 3;
    const float4* __restrict__ v = reinterpret_cast<const float4*>(samples + g0 + head);
    for (int q = lane; q < nvec; q += 64) {
      const float4 x = v[q];
      acc += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
    }
    if (lane < head) {
      const float x = y[k0 + lane];
      acc += (double)x * x;
    }
    if (lane < tail) {
      const float x = y[k0 + kHop - tail + lane];
      acc += (double)x * x;
    }
  } else {
    for (int j = lane; j < kHop; j += 64) {
      int k = k0 + j;
      if (k < 0) k = -k;                                               // yp[1024 - k] = y[k]
      if (k >= n) k = 2 * (n - 1) - k;                                 // yp[1024 + n - 1 + k] = y[n - 1 - k]
      const float x = y[k];                                            // 0 <= k < n for n >= 1025
      acc += (double)x * x;
    }
  }
  return wave_sum_f64(acc);
}

// mse of frame f from the block sums of its region
__device__ __forceinline__ double frame_mse(const double* __restrict__ s, int f) {
  return ((s[f] + s[f + 1]) + (s[f + 2] + s[f + 3])) * (1.0 / kFrame);
}

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // four floats at any sample index

__device__ __forceinline__ float mix_norm(float m) { return (float)(1.1 * (double)m); }

}  // namespace
