// BatchNorm + activation over channels-last bf16 tensors [npix][64]: the apply pass z -> a and the backward
//   dy = da * act'(z * scale + shift);  pass 1: per-channel sum dy, sum dy * xhat (xhat = (z - mean) * invstd);
//   pass 2: dz = cA * dy + cB * z + cC (coefficients from bn_bwd_finalize, conv_bwd.hip), bf16, may overwrite da.
// All three are streaming passes: a lane keeps its piece's 8 channels for the whole launch.
#include "nhwc_common.h"

namespace {

// The streaming loop of the three kernels, written out in each (as a function over load / consume closures it moved every instance's
// registers: profiles/nhwc_edge_split.md): two pieces in flight per lane (four: 0.628 vs 0.625 ms at B = 64 for the apply pass, round 4).

// dy and dz of one channel
template <int ACT>
__device__ __forceinline__ float bn_bwd_dy(float g, float z, float sc, float sh) { return g * nhwc_act_grad<ACT>(fmaf(z, sc, sh)); }
__device__ __forceinline__ float bn_bwd_dz(float cA, float cB, float cC, float dy, float z) { return fmaf(cA, dy, fmaf(cB, z, cC)); }

template <int ACT>
__global__ __launch_bounds__(256)
void nhwc_bn_apply_kernel(const u4v* __restrict__ z, u4v* __restrict__ a, const float* __restrict__ scale,
                          const float* __restrict__ shift, long long npieces) {
  const int piece = threadIdx.x & 7;
  vs_f32x2 sc[4], sh[4];                                   // the lane's 8 channels as the 4 pairs its 32-bit words hold
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    sc[q] = ld_pair(scale, piece * 8 + 2 * q);
    sh[q] = ld_pair(shift, piece * 8 + 2 * q);
  }
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  auto apply = [&](const u4v v) {
    u4v o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const vs_f32x2 y = vs_act_fast2<ACT>(__builtin_elementwise_fma(bf_pair(v[q]), sc[q], sh[q]));
      o[q] = vs_pack_bf16(y.x, y.y);
    }
    return o;
  };
  for (; i + stride < npieces; i += 2 * stride) {
    const u4v v0 = __builtin_nontemporal_load(z + i), v1 = __builtin_nontemporal_load(z + i + stride);
    __builtin_nontemporal_store(apply(v0), a + i);
    __builtin_nontemporal_store(apply(v1), a + i + stride);
  }
  if (i < npieces) __builtin_nontemporal_store(apply(__builtin_nontemporal_load(z + i)), a + i);
}

template <int ACT>
__global__ __launch_bounds__(256)
void nhwc_bn_bwd_stats_kernel(const u4v* __restrict__ da, const u4v* __restrict__ z, long long npieces,
                              const float* __restrict__ scale, const float* __restrict__ shift,
                              const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ stats) {
  __shared__ float red[4 * 2 * 64];
  const int piece = threadIdx.x & 7;
  float sc[8], sh[8], mu[8], is[8], acc[2][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = piece * 8 + j;
    sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; is[j] = invstd[c];
    acc[0][j] = 0.f; acc[1][j] = 0.f;
  }
  const long long stride = (long long)gridDim.x * 256;
  auto eat = [&](const u4v g, const u4v v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float z0 = bf_lo(v[q]), z1 = bf_hi(v[q]);
      const float d0 = bn_bwd_dy<ACT>(bf_lo(g[q]), z0, sc[2 * q], sh[2 * q]);
      const float d1 = bn_bwd_dy<ACT>(bf_hi(g[q]), z1, sc[2 * q + 1], sh[2 * q + 1]);
      acc[0][2 * q] += d0;
      acc[0][2 * q + 1] += d1;
      acc[1][2 * q] = fmaf(d0, (z0 - mu[2 * q]) * is[2 * q], acc[1][2 * q]);
      acc[1][2 * q + 1] = fmaf(d1, (z1 - mu[2 * q + 1]) * is[2 * q + 1], acc[1][2 * q + 1]);
    }
  };
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < npieces; i += 2 * stride) {
    const u4v g0 = __builtin_nontemporal_load(da + i), v0 = __builtin_nontemporal_load(z + i);
    const u4v g1 = __builtin_nontemporal_load(da + i + stride), v1 = __builtin_nontemporal_load(z + i + stride);
    eat(g0, v0);
    eat(g1, v1);
  }
  if (i < npieces) eat(__builtin_nontemporal_load(da + i), __builtin_nontemporal_load(z + i));
  fold_channel_sums<2>(acc, stats, red);
}

template <int ACT>
__global__ __launch_bounds__(256)
void nhwc_bn_bwd_apply_kernel(const u4v* da, const u4v* __restrict__ z, u4v* dz, long long npieces,
                              const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ coef) {
  const int piece = threadIdx.x & 7;
  float sc[8], sh[8], cA[8], cB[8], cC[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = piece * 8 + j;
    sc[j] = scale[c]; sh[j] = shift[c]; cA[j] = coef[c]; cB[j] = coef[64 + c]; cC[j] = coef[128 + c];
  }
  const long long stride = (long long)gridDim.x * 256;
  auto apply = [&](const u4v g, const u4v v) {
    u4v o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float z0 = bf_lo(v[q]), z1 = bf_hi(v[q]);
      const float d0 = bn_bwd_dy<ACT>(bf_lo(g[q]), z0, sc[2 * q], sh[2 * q]);
      const float d1 = bn_bwd_dy<ACT>(bf_hi(g[q]), z1, sc[2 * q + 1], sh[2 * q + 1]);
      o[q] = vs_pack_bf16(bn_bwd_dz(cA[2 * q], cB[2 * q], cC[2 * q], d0, z0), bn_bwd_dz(cA[2 * q + 1], cB[2 * q + 1], cC[2 * q + 1], d1, z1));
    }
    return o;
  };
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < npieces; i += 2 * stride) {
    const u4v g0 = __builtin_nontemporal_load(da + i), v0 = __builtin_nontemporal_load(z + i);
    const u4v g1 = __builtin_nontemporal_load(da + i + stride), v1 = __builtin_nontemporal_load(z + i + stride);
    __builtin_nontemporal_store(apply(g0, v0), dz + i);
    __builtin_nontemporal_store(apply(g1, v1), dz + i + stride);
  }
  if (i < npieces) __builtin_nontemporal_store(apply(__builtin_nontemporal_load(da + i), __builtin_nontemporal_load(z + i)), dz + i);
}

// pass 2 on `nb` workgroups
int bn_bwd_apply_pass(const void* da, const void* z, void* dz, long long npieces, int nb, int act, const float* scale, const float* shift,
                      const float* coef, hipStream_t stream) {
  const u4v* g = reinterpret_cast<const u4v*>(da);
  const u4v* zz = reinterpret_cast<const u4v*>(z);
  u4v* o = reinterpret_cast<u4v*>(dz);
  if (int rc = nhwc_dispatch_act(act, "nhwc bn_act_bwd", [&](auto A) {
        hipLaunchKernelGGL(nhwc_bn_bwd_apply_kernel<decltype(A)::value>, dim3(nb), dim3(256), 0, stream, g, zz, o, npieces, scale, shift, coef);
      })) return rc;
  VS_LAUNCH_CHECK();
  return 0;
}

// beside the weight gradient on the side stream (vs_backward): ONE block per CU.  The pass from dy then takes 1.8 ms instead of 1.2 -- still
// inside the weight gradient's 1.95 -- and takes less from it (2.06 -> 1.94 ms per layer, -0.4 ms per step: profiles/r05_bn_finalize_ab.md).
// (128: +2.2 ms per step, 512: +0.2 -- round 5, call 10; [r6, call 32] a contiguous part per workgroup instead of the strided loop: the
// pass 1.9 -> 1.7 ms, the weight gradient beside it and the step unchanged -- not kept.)  The two-pass form throttles both passes the same
// way (the round-6 re-run of the two-pass A/B: +4 ms per step, profiles/r06_experiments.md).
int throttle_beside_wgrad(int nb, int beside_wgrad) { return (beside_wgrad && nb > 256) ? 256 : nb; }

}  // namespace

// a = act(z * scale[c] + shift[c]) over [npix][64] bf16; a may alias z
int vs_nhwc_bn_apply_impl(const void* z, void* a, long long npix, int act, const float* scale, const float* shift, hipStream_t stream) {
  VS_REQUIRE(z && a && scale && shift && npix > 0, "nhwc bn_apply: bad argument");
  const long long npieces = npix * 8;
  const dim3 grid(stream_blocks_wide(512, npieces)), block(256);
  const u4v* zi = reinterpret_cast<const u4v*>(z);
  u4v* ao = reinterpret_cast<u4v*>(a);
  if (int rc = nhwc_dispatch_act(act, "nhwc bn_apply", [&](auto A) {
        hipLaunchKernelGGL(nhwc_bn_apply_kernel<decltype(A)::value>, grid, block, 0, stream, zi, ao, scale, shift, npieces);
      })) return rc;
  VS_LAUNCH_CHECK();
  return 0;
}

// pass 1 + finalize: clears the slots, sums on `nb` workgroups, parameter gradients and the coefficients of pass 2
int vs_nhwc_bn_bwd_stats_pass(const char* site, const void* da, const void* z, long long npix, int nb, int act, int train,
                              const float* scale, const float* shift, const float* mean, const float* invstd,
                              float* dgamma, float* dbeta, float* dbias, double* stats /* [VS_BN_STAT_SLOTS][64][2] */, float* coef, hipStream_t stream) {
  const long long npieces = npix * 8;
  const u4v* g = reinterpret_cast<const u4v*>(da);
  const u4v* zz = reinterpret_cast<const u4v*>(z);
  VS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(double) * VS_BN_STAT_SLOTS * 128, stream));
  if (int rc = nhwc_dispatch_act(act, site, [&](auto A) {
        hipLaunchKernelGGL(nhwc_bn_bwd_stats_kernel<decltype(A)::value>, dim3(nb), dim3(256), 0, stream, g, zz, npieces, scale, shift, mean, invstd, stats);
      })) return rc;
  return vs_bn_bwd_finalize_impl(stats, VS_BN_STAT_SLOTS, (double)npix, train, 64, scale, mean, invstd, dgamma, dbeta, dbias, coef, stream);
}

// BatchNorm + activation backward over [npix][64] bf16 (dz may alias da): parameter gradients + dz
int vs_nhwc_bn_act_bwd_impl(const void* da, const void* z, void* dz, long long npix, int act, int train,
                            const float* scale, const float* shift, const float* mean, const float* invstd,
                            float* dgamma, float* dbeta, float* dbias, double* stats /* [VS_BN_STAT_SLOTS][64][2] */, float* coef,
                            hipStream_t stream, int beside_wgrad) {
  VS_REQUIRE(da && z && dz && scale && shift && mean && invstd && stats && coef && npix > 0, "nhwc bn_act_bwd: bad argument");
  const int nb = throttle_beside_wgrad(stream_blocks(512, npix * 8), beside_wgrad);
  if (int rc = vs_nhwc_bn_bwd_stats_pass("nhwc bn_act_bwd", da, z, npix, nb, act, train, scale, shift, mean, invstd, dgamma, dbeta, dbias, stats, coef, stream))
    return rc;
  return bn_bwd_apply_pass(da, z, dz, npix * 8, nb, act, scale, shift, coef, stream);
}

// The same with the first pass already done by the kernel that produced dy = da * act'(.) (conv_nhwc.hip's dy
// epilogue, cnn8's backward in nhwc_last.hip): stats holds the per-channel sums; parameter gradients + dz = cA dy + cB z + cC
int vs_nhwc_bn_bwd_from_dy_impl(const void* dy, const void* z, void* dz, long long npix, int train,
                                const float* scale, const float* mean, const float* invstd,
                                float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, hipStream_t stream, int rezero_doubles,
                                int beside_wgrad) {
  VS_REQUIRE(dy && z && dz && scale && mean && invstd && stats && coef && npix > 0, "nhwc bn_bwd_from_dy: bad argument");
  const long long npieces = npix * 8;
  const int nb = throttle_beside_wgrad(beside_wgrad ? stream_blocks(512, npieces) : stream_blocks_wide(512, npieces), beside_wgrad);
  if (int rc = vs_bn_bwd_finalize_impl(stats, VS_BN_STAT_SLOTS, (double)npix, train, 64, scale, mean, invstd, dgamma, dbeta, dbias, coef, stream,
                                       rezero_doubles)) return rc;
  return bn_bwd_apply_pass(dy, z, dz, npieces, nb, VS_ACT_NONE, scale, scale, coef, stream);
}
