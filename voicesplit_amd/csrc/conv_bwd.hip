// Backward of the conv stack in the NCHW fp32 layout (the `.backward()` half of train.py:94-110 through
// models/voicesplit/model.py:15-52): the fp32 weight gradient of the 64->64 layers, the
// BatchNorm+activation backward, and the two bandwidth-bound edge layers cnn1 and cnn8.
// The weight gradient in split-f16 arithmetic (VS_MATH_F16X3) is in wgrad_f16x3.hip, the
// channels-last bf16 one in wgrad_nhwc.hip.
//
//   data gradient   dIn = conv(dZ, flip/transpose(W))  -> the FORWARD kernel (conv_mfma.hip) fed
//                   with weights packed by conv_pack_weights_kernel(..., transpose_flip = 1)
//   weight gradient dW[co][ci][kt][kf] = sum_{b,t,f} dZ[b][co][t][f] * In[b][ci][t+(kt-KT/2)*dil][f+kf-KF/2]
//                   -> conv64_wgrad_kernel below: an implicit GEMM with M = co, N = ci, K = pixels
//   BatchNorm+act   dZ = scale*(dY - mean(dY) - xhat*mean(dY*xhat)),  dY = dA * act'(Y)
//                   (train: batch statistics; eval: dZ = scale*dY) -> two streaming passes
//
// conv64_wgrad_kernel.  Workgroup = 4 waves, fixed time tap kt, all KF frequency taps; it walks a
// contiguous range of (utterance, frame, 64-bin segment) tiles and keeps its 64x64xKF partial
// sums in accumulator registers the whole time (wave w owns the 32x32 block (co block w>>1,
// ci block w&1) for every kf: 16*KF registers).  Per tile the dZ row segment [64 co][64 f] and
// the input row segment [64 ci][64+KF-1 f] of frame t+(kt-KT/2)*dil are staged global -> VGPR ->
// LDS (raw buffer loads, out-of-range offsets return 0 = ZeroPad2d; the loads of the next tile
// are in flight during the MFMAs).  K runs over pixels: lane (row = lane&31, half = lane>>5)
// reads the four pixels 8*kg+4*half+0..3 of its channel row with ONE ds_read_b128 (row pitch 68
// floats: conflict-free for the b128 lane groups), and the KF shifted input windows are just
// different registers of two such reads -- no data movement per tap.  Frames whose shifted input
// row lies outside the image contribute nothing and are skipped (10 % of the rows at dil = 16).
// The partial sums of the G workgroups of each kt go to a workspace and are summed in a fixed
// order by conv64_wgrad_reduce_kernel (deterministic, no atomics; shared with wgrad_f16x3.hip).
#include "vs_internal.h"

namespace {

constexpr unsigned kOob = 0x7FFFFFF0u;
constexpr int kNF = 64;    // output pixels (frequency bins) per tile
constexpr int kPD = 68;    // LDS row pitch in floats: >= 64+4, == 4 (mod 64)

struct WgradArgs {
  const float* dz;   // [B][64][T][F]
  const float* in;   // [B][64][T][F]
  float* part;       // [G][KT][KF][64 co][64 ci]
  int B, T, F, dil, KT, nseg, G;
};

template <int KF>
__global__ __launch_bounds__(256, KF == 1 ? 4 : 3)
void conv64_wgrad_kernel(WgradArgs g) {
  constexpr int PADF = KF / 2;
  __shared__ __attribute__((aligned(16))) float sD[64 * kPD];
  __shared__ __attribute__((aligned(16))) float sA[64 * kPD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;

  // block -> (kt, group): the KT workgroups of one group walk the same tiles at about the same
  // time; bid % 8 is the XCD (observed placement, speed only), so keep them on one L2.
  const int bid = blockIdx.x;
  const int xcd = bid & 7;
  const int kt = (bid >> 3) % g.KT;
  const int grp = ((bid >> 3) / g.KT) * 8 + xcd;

  const int off_t = (kt - g.KT / 2) * g.dil;
  const int t_lo = off_t < 0 ? -off_t : 0;
  const int t_hi = off_t > 0 ? g.T - off_t : g.T;
  const int nvt = t_hi > t_lo ? t_hi - t_lo : 0;
  const int ntiles = g.B * nvt * g.nseg;          // < 2^31, checked by the launcher
  const int per = (ntiles + g.G - 1) / g.G;
  int tile = grp * per;
  const int tile_end = tile + per < ntiles ? tile + per : ntiles;

  const size_t plane = (size_t)g.T * g.F;
  const unsigned plane_bytes = (unsigned)(plane * sizeof(float));

  f32x16 acc[KF];
#pragma unroll
  for (int k = 0; k < KF; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

  float sd[16], sa[16], sx = 0.f;
  int nv_next = 0;
  auto issue = [&](int tl) {
    const int bt = tl / g.nseg;
    const int seg = tl - bt * g.nseg;
    const int b = bt / nvt;
    const int t = t_lo + (bt - b * nvt);
    const int f0 = seg * kNF;
    nv_next = g.F - f0 < kNF ? g.F - f0 : kNF;
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.dz + (size_t)b * 64 * plane), 0, 64u * plane_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.in + (size_t)b * 64 * plane), 0, 64u * plane_bytes, 0x00020000);
    const int fd = f0 + lane;
    const unsigned vd = fd < g.F ? (unsigned)((t * g.F + fd) * 4) : kOob;
    const int fa = f0 - PADF + lane;
    const unsigned va = (fa >= 0 && fa < g.F) ? (unsigned)(((t + off_t) * g.F + fa) * 4) : kOob;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const unsigned so = (unsigned)(wave + 4 * i) * plane_bytes;     // channel plane, wave-uniform
      sd[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rd, vd, so, 0));
      sa[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, va, so, 0));
    }
    if (KF > 1) {   // the KF-1 halo columns 64..64+KF-2: one (channel, column) per thread
      const int ch = tid >> 2, col = kNF + (tid & 3);
      const int fx = f0 - PADF + col;
      const unsigned vx = (fx >= 0 && fx < g.F) ? (unsigned)(ch * plane_bytes + ((t + off_t) * g.F + fx) * 4) : kOob;
      sx = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, vx, 0, 0));
    }
  };

  const int cb = wave >> 1, nb = wave & 1;
  const float* pd = sD + (cb * 32 + l31) * kPD + 4 * half;
  const float* pa = sA + (nb * 32 + l31) * kPD + 4 * half;

  if (tile < tile_end) issue(tile);
  while (tile < tile_end) {
    __syncthreads();          // every wave is done reading the previous tile
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      sD[(wave + 4 * i) * kPD + lane] = sd[i];
      sA[(wave + 4 * i) * kPD + lane] = sa[i];
    }
    if (KF > 1) sA[(tid >> 2) * kPD + kNF + (tid & 3)] = sx;
    const int nkg = (nv_next + 7) >> 3;
    __syncthreads();
    ++tile;
    if (tile < tile_end) issue(tile);
#pragma unroll
    for (int kg = 0; kg < kNF / 8; ++kg) {
      if (kg < nkg) {         // block-uniform
        const float4 d4 = *reinterpret_cast<const float4*>(pd + 8 * kg);
        float w[8];
        {
          const float4 w0 = *reinterpret_cast<const float4*>(pa + 8 * kg);
          w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w;
        }
        if (KF > 1) {
          const float4 w1 = *reinterpret_cast<const float4*>(pa + 8 * kg + 4);
          w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float dv = j == 0 ? d4.x : j == 1 ? d4.y : j == 2 ? d4.z : d4.w;
#pragma unroll
          for (int kf = 0; kf < KF; ++kf)
            acc[kf] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv, w[j + kf], acc[kf], 0, 0, 0);
        }
      }
    }
  }

  // partial sums: D row = co (r&3)+8*(r>>2)+4*half, D col = ci = lane&31
  float* out = g.part + ((size_t)grp * g.KT + kt) * KF * 4096;
#pragma unroll
  for (int kf = 0; kf < KF; ++kf)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      out[(size_t)kf * 4096 + co * 64 + nb * 32 + l31] = acc[kf][r];
    }
}

// dW[co][ci][kt][kf] = sum_g part[g][kt][kf][co][ci]; SCALED (split-f16 partial sums): times 1/(s_dz*s_in)
template <bool SCALED>
__global__ void conv64_wgrad_reduce_kernel(const float* __restrict__ part, int G, int NT, float* __restrict__ dw,
                                           const float* __restrict__ dz_scale, const float* __restrict__ in_scale) {
  const int total = NT * 4096;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  float s = 0.f;
  for (int gq = 0; gq < G; ++gq) s += part[(size_t)gq * total + idx];
  const int tap = idx >> 12, co = (idx >> 6) & 63, ci = idx & 63;
  if (SCALED) s *= dz_scale[1] * in_scale[1];
  dw[((size_t)co * 64 + ci) * NT + tap] = s;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm + activation backward.  The tensor is seen as rows [R][L] with channel = r % C:
// NCHW activations R = B*C, L = T*F; the LSTM-feature layout of cnn8 R = B*T*8, L = F, C = 8.
// ---------------------------------------------------------------------------------------------
template <int ACT>
__device__ __forceinline__ float act_grad(float y) {
  if (ACT == VS_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (ACT == VS_ACT_MISH) return vs_mish_grad_fast(y);
  return 1.f;
}

// Both passes walk (row, chunk) items of one channel per block like the forward BatchNorm kernels
// (vs_walk_chunk, conv_edge.hip): grid (blocks per channel, C), float4 middles, two packs in flight.
template <int W> struct BnBwdPack { static constexpr int N = W; VsPack<W> g, z; };

// pass 1: stats[c] += { sum dY, sum dY*xhat },  dY = dA * act'(z*scale+shift), xhat = (z-mean)*invstd
template <int ACT>
__global__ __launch_bounds__(256)
void bn_act_bwd_stats_kernel(const float* __restrict__ da, const float* __restrict__ z, int C, long long rows_c, int L,
                             const float* __restrict__ scale, const float* __restrict__ shift,
                             const float* __restrict__ mean, const float* __restrict__ invstd,
                             double* __restrict__ stats, unsigned* turn = nullptr) {
  const int c = blockIdx.y;
  const float sc = scale[c], sh = shift[c], mu = mean[c], is = invstd[c];
  const int gx = vs_row_chunks(L);
  double d1 = 0.0, d2 = 0.0;
  for (long long it = blockIdx.x; it < rows_c * gx; it += gridDim.x) {
    const long long off = (c + (long long)C * (it / gx)) * L;
    const float* pz = z + off;
    const float* pg = da + off;
    float s1 = 0.f, s2 = 0.f;
    vs_walk_chunk(L, vs_row_phase(pz, pg), (int)(it % gx),
                  [&](int i, auto w) {
                    BnBwdPack<decltype(w)::value> r;
                    r.g = vs_ldv<decltype(w)::value>(pg + i);
                    r.z = vs_ldv<decltype(w)::value>(pz + i);
                    return r;
                  },
                  [&](int, auto v) {
#pragma unroll
                    for (int e = 0; e < decltype(v)::N; ++e) {
                      const float zv = v.z.v[e];
                      const float dy = v.g.v[e] * act_grad<ACT>(fmaf(zv, sc, sh));
                      s1 += dy;
                      s2 = fmaf(dy, (zv - mu) * is, s2);
                    }
                  });
    d1 += s1;
    d2 += s2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d1 += __shfl_down(d1, o, 64);
    d2 += __shfl_down(d2, o, 64);
  }
  __shared__ double sh2[8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sh2[2 * w] = d1; sh2[2 * w + 1] = d2; }
  __syncthreads();
  unsigned* my_turn = turn ? turn + VS_TURN_CHANNEL + c : nullptr;      // deterministic mode: the workgroups of a channel add in index order (a word per channel)
  vs_turn_begin(my_turn, blockIdx.x);
  if (threadIdx.x == 0) {
    atomicAdd(&stats[2 * c], sh2[0] + sh2[2] + sh2[4] + sh2[6]);
    atomicAdd(&stats[2 * c + 1], sh2[1] + sh2[3] + sh2[5] + sh2[7]);
  }
  vs_turn_end(my_turn, blockIdx.x, gridDim.x);
}

// per channel: parameter gradients and the coefficients of pass 2,  dZ = cA*dY + cB*z + cC
//   train: dZ = scale*(dY - s1/N - xhat*s2/N);   eval: dZ = scale*dY
//   dgamma = s2, dbeta = s1, dbias(conv) = sum dZ = 0 (train) / scale*s1 (eval)
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ stats, double count, int train, int C,
                                       const float* __restrict__ scale, const float* __restrict__ mean,
                                       const float* __restrict__ invstd,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dbias,
                                       float* __restrict__ coef /* [3][C] */) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double s1 = stats[2 * c], s2 = stats[2 * c + 1];
  if (dgamma) dgamma[c] = (float)s2;
  if (dbeta) dbeta[c] = (float)s1;
  const double sc = scale[c];
  if (train) {
    const double k1 = s1 / count, k2 = s2 / count, is = invstd[c], mu = mean[c];
    coef[c] = (float)sc;
    coef[C + c] = (float)(-sc * k2 * is);
    coef[2 * C + c] = (float)(-sc * k1 + sc * k2 * is * mu);
    if (dbias) dbias[c] = 0.f;
  } else {
    coef[c] = (float)sc;
    coef[C + c] = 0.f;
    coef[2 * C + c] = 0.f;
    if (dbias) dbias[c] = (float)(sc * s1);
  }
}

// pass 2: dz = cA*(dA*act'(z*scale+shift)) + cB*z + cC     (dz may alias da)
template <int ACT>
__global__ __launch_bounds__(256)
void bn_act_bwd_apply_kernel(const float* da, const float* __restrict__ z, int C, long long rows_c, int L,
                             const float* __restrict__ scale, const float* __restrict__ shift,
                             const float* __restrict__ coef, float* dz, unsigned* amax_out) {
  const int c = blockIdx.y;
  const float sc = scale[c], sh = shift[c], cA = coef[c], cB = coef[C + c], cC = coef[2 * C + c];
  const int gx = vs_row_chunks(L);
  float m = 0.f;
  for (long long it = blockIdx.x; it < rows_c * gx; it += gridDim.x) {
    const long long off = (c + (long long)C * (it / gx)) * L;
    const float* pz = z + off;
    const float* pg = da + off;
    float* po = dz + off;
    vs_walk_chunk(L, vs_row_phase(pz, pg, po), (int)(it % gx),
                  [&](int i, auto w) {
                    BnBwdPack<decltype(w)::value> r;
                    r.g = vs_ldv<decltype(w)::value>(pg + i);
                    r.z = vs_ldv<decltype(w)::value>(pz + i);
                    return r;
                  },
                  [&](int i, auto v) {
#pragma unroll
                    for (int e = 0; e < decltype(v)::N; ++e) {
                      const float zv = v.z.v[e];
                      const float dy = v.g.v[e] * act_grad<ACT>(fmaf(zv, sc, sh));
                      const float o = fmaf(cA, dy, fmaf(cB, zv, cC));
                      v.g.v[e] = o;
                      m = fmaxf(m, fabsf(o));
                    }
                    vs_stv(po + i, v.g);
                  });
  }
  vs_absmax_commit(m, amax_out);
}

// ---------------------------------------------------------------------------------------------
// cnn8 (1x1, 64->8, output in the LSTM feature layout [B][T][8][F])
// ---------------------------------------------------------------------------------------------
// dIn[b][ci][t][f] = sum_o W[o][ci] * dZ[b][t][o][f].  A thread owns 4 consecutive pixels of the
// plane and writes them as one 16-byte store per channel (1 KB per wave instruction instead of
// 256 B; planes are only 4-byte aligned -- T*F is odd -- and the stores are issued unaligned).
__global__ __launch_bounds__(256)
void conv_last_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ din, int T, int F) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int plane = T * F;
  const int pix0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int b = blockIdx.y;
  if (pix0 >= plane) return;
  const int np = plane - pix0 < 4 ? plane - pix0 : 4;
  float v[8][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int pix = pix0 + (e < np ? e : 0);
    const int t = pix / F, f = pix - t * F;
    const float* src = dz + ((size_t)b * T + t) * 8 * F + f;
#pragma unroll
    for (int o = 0; o < 8; ++o) v[o][e] = src[(size_t)o * F];
  }
  float* dst = din + (size_t)b * 64 * plane + pix0;
#pragma unroll 2
  for (int c = 0; c < 64; ++c) {
    f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const float wv = w[o * 64 + c];
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = fmaf(wv, v[o][e], a[e]);
    }
    float* q = dst + (size_t)c * plane;
    if (np == 4) {
      __builtin_memcpy(q, &a, 16);          // one global_store_dwordx4, any 4-byte alignment
    } else {
      for (int e = 0; e < np; ++e) q[e] = a[e];
    }
  }
}

// part[blk][o][ci] = sum over this block's (b, t, 256-bin segment) tiles of dZ[o][pix]*In[ci][pix].
// HBM-bound (2.96 GB of input per launch): a tile is 64 channel rows x 256 bins, each row segment one
// 16-byte-per-lane load (1 KB per wave instruction; rows are only 4-byte aligned: issued unaligned),
// the next tile travels to registers while this one is multiplied, and the multiply reads LDS as
// b128 (4 bins per read, row pitch 260 floats: lane = channel hits 16 different bank quads) --
// 3 LDS instructions per 8 FMAs.  (First version: 64-bin tiles, dword loads, 3 scalar LDS reads per
// 2 FMAs: 1.47 ms.)
constexpr int kLwSeg = 256;           // bins per tile
constexpr int kLwPitch = kLwSeg + 4;  // floats
__global__ __launch_bounds__(256)
void conv_last_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ in, float* __restrict__ part,
                            int B, int T, int F, int nseg) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) float lw_smem[];
  float* const sA = lw_smem;                       // [64][kLwPitch]
  float* const sD = lw_smem + 64 * kLwPitch;       // [8][kLwPitch]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ci = lane, og = w;
  f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const long long ntiles = (long long)B * T * nseg;
  const size_t plane = (size_t)T * F;

  f4 ra[16], rd[2];
  // 4 bins of one row starting at p (row has `left` bins from p on): full groups as one 16-byte load
  auto load4 = [&](const float* p, int left) -> f4 {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (left >= 4) {
      __builtin_memcpy(&v, p, 16);
    } else {
      for (int e = 0; e < left; ++e) v[e] = p[e];
    }
    return v;
  };
  auto issue = [&](long long tile) {
    const int seg = (int)(tile % nseg);
    const long long bt = tile / nseg;
    const long long b = bt / T, t = bt % T;
    const int f = seg * kLwSeg + 4 * lane;
    const int left = F - f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ch = w + 4 * i;
      ra[i] = load4(in + ((size_t)(b * 64 + ch)) * plane + (size_t)t * F + f, left);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = w + 4 * i;
      rd[i] = load4(dz + ((size_t)bt * 8 + o) * F + f, left);
    }
  };

  long long tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    const int seg = (int)(tile % nseg);
    const int nv = F - seg * kLwSeg < kLwSeg ? F - seg * kLwSeg : kLwSeg;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) *reinterpret_cast<f4*>(&sA[(w + 4 * i) * kLwPitch + 4 * lane]) = ra[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f4*>(&sD[(w + 4 * i) * kLwPitch + 4 * lane]) = rd[i];
    __syncthreads();
    if (tile + gridDim.x < ntiles) issue(tile + gridDim.x);
    const int n4 = (nv + 3) >> 2;                  // bins beyond nv were staged as zeros
    const float* pa = sA + ci * kLwPitch;
    const float* p0 = sD + (2 * og) * kLwPitch;
    const float* p1 = p0 + kLwPitch;
#pragma unroll 4
    for (int q = 0; q < n4; ++q) {
      const f4 a = *reinterpret_cast<const f4*>(pa + 4 * q);
      const f4 d0 = *reinterpret_cast<const f4*>(p0 + 4 * q);
      const f4 d1 = *reinterpret_cast<const f4*>(p1 + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0[e] = fmaf(a[e], d0[e], acc0[e]);
        acc1[e] = fmaf(a[e], d1[e], acc1[e]);
      }
    }
  }
  part[(size_t)blockIdx.x * 512 + (2 * og) * 64 + ci] = (acc0[0] + acc0[1]) + (acc0[2] + acc0[3]);
  part[(size_t)blockIdx.x * 512 + (2 * og + 1) * 64 + ci] = (acc1[0] + acc1[1]) + (acc1[2] + acc1[3]);
}

// out[i] = sum_g part[g][i].  A thread owns four consecutive outputs (16-byte loads) and keeps eight slabs in flight:
// the 128 slabs x 1.6 MB of a 5x5 weight gradient are a 210 MB stream, not a latency chain.
__global__ __launch_bounds__(256)
void reduce_partials_kernel(const float* __restrict__ part, int G, int n, float* __restrict__ out) {
  const int idx = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (idx >= n) return;
  if (idx + 4 <= n && (n & 3) == 0) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int gq = 0;
    for (; gq + 8 <= G; gq += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(part + (size_t)(gq + u) * n + idx);
#pragma unroll
      for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    for (; gq < G; ++gq) {
      const float4 v = *reinterpret_cast<const float4*>(part + (size_t)gq * n + idx);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(out + idx) = s;
    return;
  }
  for (int e = idx; e < n && e < idx + 4; ++e) {
    float s = 0.f;
    for (int gq = 0; gq < G; ++gq) s += part[(size_t)gq * n + e];
    out[e] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// cnn1 (1x7, 1->64): dW[c][k] = sum_{b,t,f} dZ[b][c][t][f] * x[b][t][f+k-3]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void conv_first_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x, double* __restrict__ acc,
                             int T, int F) {
  const int plane = T * F;
  const int c = blockIdx.y, b = blockIdx.z;
  const float* pz = dz + ((size_t)b * 64 + c) * plane;
  const float* px = x + (size_t)b * plane;
  float s[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) s[k] = 0.f;
  const int e0 = blockIdx.x * 4096;
  const int e1 = e0 + 4096 < plane ? e0 + 4096 : plane;
  for (int e = e0 + threadIdx.x; e < e1; e += 256) {
    const int f = e % F;
    const float v = pz[e];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int ff = f + k - 3;
      const float xv = (ff >= 0 && ff < F) ? px[e + k - 3] : 0.f;
      s[k] = fmaf(v, xv, s[k]);
    }
  }
  __shared__ double red[4][7];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    double d = s[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
    if (lane == 0) red[w][k] = d;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    atomicAdd(&acc[c * 7 + k], red[0][k] + red[1][k] + red[2][k] + red[3][k]);
  }
}

// xp[r][F+6] = {0,0,0, x[r][0..F-1], 0,0,0}: the 1x7 taps of cnn1 read it without edge tests
__global__ void pad_rows3_kernel(const float* __restrict__ x, float* __restrict__ xp, long long rows, int F) {
  const int P = F + 6;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows * P; i += (long long)gridDim.x * 256) {
    const long long r = i / P;
    const int j = (int)(i - r * P);
    xp[i] = (j >= 3 && j < F + 3) ? x[r * F + (j - 3)] : 0.f;
  }
}

// cnn1: pass 2 of the BatchNorm backward with the 1x7 weight gradient folded in.  dZ1 has no other
// consumer (the input needs no gradient), so it is formed in registers and contracted with the
// seven shifted inputs on the spot, dW[c][k] += dZ1[b][c][t][f] * x[b][t][f+k-3], instead of being
// written (2.96 GB at B=64) and read back by conv_first_wgrad_kernel.  Same (row, chunk) walk as
// bn_act_bwd_apply_kernel; xp = zero-padded input rows (pad_rows3_kernel).
template <int ACT>
__global__ __launch_bounds__(256)
void bn_act_bwd_first_kernel(const float* __restrict__ da, const float* __restrict__ z, const float* __restrict__ xp,
                             long long B, int T, int F, const float* __restrict__ scale, const float* __restrict__ shift,
                             const float* __restrict__ coef, double* __restrict__ acc /* [64][7] */) {
  constexpr int C = 64;
  const int c = blockIdx.y;
  const int L = T * F, P = F + 6;
  const float sc = scale[c], sh = shift[c], cA = coef[c], cB = coef[C + c], cC = coef[2 * C + c];
  const float invF = 1.0f / (float)F;
  const int gx = vs_row_chunks(L);
  double d[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) d[k] = 0.0;
  for (long long it = blockIdx.x; it < B * gx; it += gridDim.x) {
    const long long b = it / gx;
    const long long off = (c + (long long)C * b) * L;
    const float* pz = z + off;
    const float* pg = da + off;
    const float* xb = xp + b * T * P;
    float s[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] = 0.f;
    vs_walk_chunk(L, vs_row_phase(pz, pg), (int)(it % gx),
                  [&](int i, auto w) {
                    BnBwdPack<decltype(w)::value> r;
                    r.g = vs_ldv<decltype(w)::value>(pg + i);
                    r.z = vs_ldv<decltype(w)::value>(pz + i);
                    return r;
                  },
                  [&](int i, auto v) {
                    constexpr int W = decltype(v)::N;
                    // (t, f) of element i: float quotient (i < 2^24) with a one-step correction
                    int t = (int)((float)i * invF);
                    int f = i - t * F;
                    if (f < 0) { f += F; --t; } else if (f >= F) { f -= F; ++t; }
                    float dzv[W];
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                      const float zv = v.z.v[e];
                      const float dy = v.g.v[e] * act_grad<ACT>(fmaf(zv, sc, sh));
                      dzv[e] = fmaf(cA, dy, fmaf(cB, zv, cC));
                    }
                    const float* xr = xb + (size_t)t * P + f;      // tap k of element e of this row: xr[e + k]
                    if (f + W <= F) {
                      float xs[W + 6];
#pragma unroll
                      for (int j = 0; j < W + 6; ++j) xs[j] = xr[j];
#pragma unroll
                      for (int e = 0; e < W; ++e)
#pragma unroll
                        for (int k = 0; k < 7; ++k) s[k] = fmaf(dzv[e], xs[e + k], s[k]);
                    } else {                                        // the pack runs into the next frame
#pragma unroll
                      for (int e = 0; e < W; ++e) {
                        const float* q = (f + e < F) ? xr + e : xr + e + 6;
#pragma unroll
                        for (int k = 0; k < 7; ++k) s[k] = fmaf(dzv[e], q[k], s[k]);
                      }
                    }
                  });
#pragma unroll
    for (int k = 0; k < 7; ++k) d[k] += s[k];
  }
  __shared__ double red[4][7];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    double x = d[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) red[w][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    atomicAdd(&acc[c * 7 + k], red[0][k] + red[1][k] + red[2][k] + red[3][k]);
  }
}

}  // namespace

// ---- host side --------------------------------------------------------------------------------

// Persistent grid = one resident round: KT * groups <= 256 CUs x workgroups per CU (3 for the
// 5x5 kernel at <= 168 VGPRs, 4 for the 7x1 one), groups a multiple of 8 (XCD mapping).  A grid
// even slightly above the resident capacity would run a second, nearly empty round.
extern "C" int vs_conv64_wgrad_groups(int KT) { return KT == 7 ? 144 : 152; }

extern "C" size_t vs_conv64_wgrad_partial_floats(int KT, int KF) {
  // fp32 kernel: vs_conv64_wgrad_groups slabs; split-f16 ring kernel: 128 (5x5) / 256 (7x1) slabs
  const size_t g32 = (size_t)vs_conv64_wgrad_groups(KT), g16 = KF == 5 ? 128 : 256;
  return (g32 > g16 ? g32 : g16) * KT * KF * 4096;
}

int vs_conv64_wgrad_impl(const float* dz, const float* in, float* part, float* dw,
                         int B, int T, int F, int KT, int KF, int dil, hipStream_t stream) {
  VS_REQUIRE(B > 0 && T > 0 && F > 0 && dil > 0, "conv64_wgrad: bad shape B=%d T=%d F=%d dil=%d", B, T, F, dil);
  VS_REQUIRE((KT == 7 && KF == 1) || (KT == 5 && KF == 5), "conv64_wgrad: unsupported kernel %dx%d", KT, KF);
  VS_REQUIRE((long long)64 * T * F * 4 < (long long)kOob, "conv64_wgrad: T*F=%lld too large for 32-bit offsets", (long long)T * F);
  VS_REQUIRE((long long)B * T * ((F + kNF - 1) / kNF) < 2147483647LL, "conv64_wgrad: too many tiles");
  const int G = vs_conv64_wgrad_groups(KT);
  WgradArgs a{dz, in, part, B, T, F, dil, KT, (F + kNF - 1) / kNF, G};
  dim3 grid(G * KT), block(256);
  if (KF == 5) hipLaunchKernelGGL(conv64_wgrad_kernel<5>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(conv64_wgrad_kernel<1>, grid, block, 0, stream, a);
  return vs_conv64_wgrad_reduce_impl(part, G, KT * KF, dw, nullptr, nullptr, stream);
}

// the fixed-order sum over the G slabs of partial sums; dz_scale2 / in_scale2 {s, 1/s}: the split-f16 operand scales (NULL: fp32 partials)
int vs_conv64_wgrad_reduce_impl(const float* part, int G, int NT, float* dw, const float* dz_scale2, const float* in_scale2, hipStream_t stream) {
  const dim3 grid((NT * 4096 + 255) / 256), block(256);
  if (dz_scale2) hipLaunchKernelGGL(conv64_wgrad_reduce_kernel<true>, grid, block, 0, stream, part, G, NT, dw, dz_scale2, in_scale2);
  else hipLaunchKernelGGL(conv64_wgrad_reduce_kernel<false>, grid, block, 0, stream, part, G, NT, dw, dz_scale2, in_scale2);
  VS_LAUNCH_CHECK();
  return 0;
}

// BatchNorm+activation backward over rows [R][L], channel = r % C (see above).
//   stats [C][2] double scratch, coef [3][C] float scratch; dz may alias da.
int vs_bn_act_bwd_impl(const float* da, const float* z, float* dz, int C, long long R, int L, int act, int train,
                       const float* scale, const float* shift, const float* mean, const float* invstd,
                       float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, unsigned* amax_out,
                       hipStream_t stream) {
  VS_REQUIRE(C > 0 && R > 0 && L > 0 && R % C == 0, "bn_act_bwd: bad shape C=%d R=%lld L=%d", C, R, L);
  VS_REQUIRE(R <= 2147483647LL && C <= 65535, "bn_act_bwd: too many rows");
  VS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(double) * 2 * C, stream));
  const long long rows_per_c = R / C;
  unsigned* turn = C <= 64 ? g_vs_turn : nullptr;          // (the turn region holds a word for each of 64 channels: the features' BatchNorm, C = 8, is the user)
  const int bpc_full = vs_bn_blocks_per_channel(C, rows_per_c, L);
  // deterministic mode: chains of at most 64 turns per channel behind the pass (~0.2 ms), 64 * C workgroups all resident at once; the
  // apply pass below keeps the full grid (round 6: sixteen per channel on BOTH passes cost 4.2 ms at B = 64 -- 128 workgroups cannot
  // stream 1.9 GB)
  int bpc = (turn && bpc_full > 64) ? 64 : bpc_full;
  int bpc_apply = bpc_full;
  if (C <= 8) {      // [r6, calls 34-35] the features' BatchNorm (8 channels of 601-element rows): more, shorter-lived workgroups -- statistics pass
    // 256 -> 512 per channel (373 -> 330 us; 4096: 736, its flush), apply pass 256 -> 4096 (304 -> 216 us; all rows: 250); step -0.09 ms
    const long long items = rows_per_c * vs_row_chunks(L);
    if (!turn && bpc < 512) bpc = (int)(items < 512 ? items : 512);
    if (bpc_apply < 4096) bpc_apply = (int)(items < 4096 ? items : 4096);
  }
  dim3 grid(bpc, C), block(256);
  switch (act) {
    case VS_ACT_RELU: hipLaunchKernelGGL(bn_act_bwd_stats_kernel<VS_ACT_RELU>, grid, block, 0, stream, da, z, C, rows_per_c, L, scale, shift, mean, invstd, stats, turn); break;
    case VS_ACT_MISH: hipLaunchKernelGGL(bn_act_bwd_stats_kernel<VS_ACT_MISH>, grid, block, 0, stream, da, z, C, rows_per_c, L, scale, shift, mean, invstd, stats, turn); break;
    case VS_ACT_NONE: hipLaunchKernelGGL(bn_act_bwd_stats_kernel<VS_ACT_NONE>, grid, block, 0, stream, da, z, C, rows_per_c, L, scale, shift, mean, invstd, stats, turn); break;
    default: VS_REQUIRE(false, "bn_act_bwd: unknown activation %d", act);
  }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, stream, stats, (double)rows_per_c * L, train, C,
                     scale, mean, invstd, dgamma, dbeta, dbias, coef);
  const dim3 grid_apply(bpc_apply, C);
  switch (act) {
    case VS_ACT_RELU: hipLaunchKernelGGL(bn_act_bwd_apply_kernel<VS_ACT_RELU>, grid_apply, block, 0, stream, da, z, C, rows_per_c, L, scale, shift, coef, dz, amax_out); break;
    case VS_ACT_MISH: hipLaunchKernelGGL(bn_act_bwd_apply_kernel<VS_ACT_MISH>, grid_apply, block, 0, stream, da, z, C, rows_per_c, L, scale, shift, coef, dz, amax_out); break;
    default: hipLaunchKernelGGL(bn_act_bwd_apply_kernel<VS_ACT_NONE>, grid_apply, block, 0, stream, da, z, C, rows_per_c, L, scale, shift, coef, dz, amax_out); break;
  }
  VS_LAUNCH_CHECK();
  return 0;
}

namespace {
__global__ void bn_bwd_fold_slots_kernel(double* __restrict__ stats, int n, int slots) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = 0.0;
  for (int k = 0; k < slots; ++k) v += stats[(size_t)k * n + i];
  stats[i] = v;
}
}  // namespace

// stats: [slots][C][2] doubles {sum dy, sum dy*xhat} (slots > 1: folded into slot 0 first) -> parameter gradients and
// the three per-channel coefficients of the apply pass
namespace {
// one launch: fold the slots, the coefficients, clear the scratch (vs_fold_slots; the arithmetic of bn_bwd_finalize_kernel, to the letter)
__global__ __launch_bounds__(VS_FOLD_THREADS)
void bn_bwd_fold_finalize_kernel(double* __restrict__ stats, int slots, int rezero, double count, int train, int C,
                                 const float* __restrict__ scale, const float* __restrict__ mean, const float* __restrict__ invstd,
                                 float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dbias, float* __restrict__ coef) {
  __shared__ double part[8 * 128], tot[128];
  vs_fold_slots(stats, 2 * C, slots, rezero, part, tot);
  const int c = threadIdx.x;
  if (c >= C) return;
  const double s1 = tot[2 * c], s2 = tot[2 * c + 1];
  if (dgamma) dgamma[c] = (float)s2;
  if (dbeta) dbeta[c] = (float)s1;
  const double sc = scale[c];
  if (train) {
    const double k1 = s1 / count, k2 = s2 / count, is = invstd[c], mu = mean[c];
    coef[c] = (float)sc;
    coef[C + c] = (float)(-sc * k2 * is);
    coef[2 * C + c] = (float)(-sc * k1 + sc * k2 * is * mu);
    if (dbias) dbias[c] = 0.f;
  } else {
    coef[c] = (float)sc;
    coef[C + c] = 0.f;
    coef[2 * C + c] = 0.f;
    if (dbias) dbias[c] = (float)(sc * s1);
  }
}
}  // namespace

int vs_bn_bwd_finalize_impl(double* stats, int slots, double count, int train, int C, const float* scale, const float* mean,
                            const float* invstd, float* dgamma, float* dbeta, float* dbias, float* coef, hipStream_t stream, int rezero_doubles) {
  VS_REQUIRE(stats && coef && C > 0 && count > 0, "bn_bwd_finalize: bad argument");
  if (rezero_doubles > 0 && C <= 64) {
    hipLaunchKernelGGL(bn_bwd_fold_finalize_kernel, dim3(1), dim3(VS_FOLD_THREADS), 0, stream, stats, slots, rezero_doubles, count, train, C,
                       scale, mean, invstd, dgamma, dbeta, dbias, coef);
    VS_LAUNCH_CHECK();
    return 0;
  }
  if (slots > 1) hipLaunchKernelGGL(bn_bwd_fold_slots_kernel, dim3((2 * C + 127) / 128), dim3(128), 0, stream, stats, 2 * C, slots);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, stream, stats, count, train, C,
                     scale, mean, invstd, dgamma, dbeta, dbias, coef);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_conv_last_dgrad_impl(const float* dz, const float* w, float* din, int B, int T, int F, hipStream_t stream) {
  VS_REQUIRE(B > 0 && T > 0 && F > 0 && B <= 65535, "conv_last_dgrad: bad shape B=%d T=%d F=%d", B, T, F);
  hipLaunchKernelGGL(conv_last_dgrad_kernel, dim3((T * F + 1023) / 1024, B), dim3(256), 0, stream, dz, w, din, T, F);
  VS_LAUNCH_CHECK();
  return 0;
}

extern "C" int vs_conv_last_wgrad_blocks(void) { return 512; }   // two resident workgroups per CU: one round

int vs_conv_last_wgrad_impl(const float* dz, const float* in, float* part /* [blocks][512] */, float* dw,
                            int B, int T, int F, hipStream_t stream) {
  VS_REQUIRE(B > 0 && T > 0 && F > 0, "conv_last_wgrad: bad shape B=%d T=%d F=%d", B, T, F);
  const int nblk = vs_conv_last_wgrad_blocks();
  const size_t lds = (size_t)72 * kLwPitch * sizeof(float);        // 74.9 KB: two workgroups per CU
  VS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_last_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(conv_last_wgrad_kernel, dim3(nblk), dim3(256), lds, stream, dz, in, part, B, T, F, (F + kLwSeg - 1) / kLwSeg);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, part, nblk, 512, dw);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_reduce_partials_impl(const float* part, int G, int n, float* out, hipStream_t stream) {
  VS_REQUIRE(G > 0 && n > 0, "reduce_partials: bad shape G=%d n=%d", G, n);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((n + 1023) / 1024), dim3(256), 0, stream, part, G, n, out);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_conv_first_wgrad_impl(const float* dz, const float* x, double* acc /* [64][7] */, float* dw,
                             int B, int T, int F, hipStream_t stream) {
  VS_REQUIRE(B > 0 && T > 0 && F > 0 && B <= 65535, "conv_first_wgrad: bad shape B=%d T=%d F=%d", B, T, F);
  VS_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 448, stream));
  hipLaunchKernelGGL(conv_first_wgrad_kernel, dim3((T * F + 4095) / 4096, 64, B), dim3(256), 0, stream, dz, x, acc, T, F);
  return vs_cvt_f64_f32_impl(acc, dw, 448, stream);
}

// cnn1: BatchNorm+activation backward and the 1x7 weight gradient in one go (dZ1 is never stored).
//   da, z: [B][64][T][F]; x: [B][T][F]; xpad: B*T*(F+6) floats of scratch; acc: 448 doubles.
int vs_bn_act_bwd_first_impl(const float* da, const float* z, const float* x, float* xpad, int B, int T, int F, int act, int train,
                             const float* scale, const float* shift, const float* mean, const float* invstd,
                             float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc,
                             hipStream_t stream) {
  VS_REQUIRE(B > 0 && T > 0 && F >= 4 && (long long)T * F < (1 << 24), "bn_act_bwd_first: bad shape B=%d T=%d F=%d (needs F >= 4, T*F < 2^24)", B, T, F);
  constexpr int C = 64;
  const int L = T * F;
  VS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(double) * 2 * C, stream));
  VS_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 448, stream));
  dim3 grid(vs_bn_blocks_per_channel(C, B, L), C), block(256);
  const long long rows = (long long)B * T;
  hipLaunchKernelGGL(pad_rows3_kernel, dim3((unsigned)((rows * (F + 6) + 255) / 256 < 4096 ? (rows * (F + 6) + 255) / 256 : 4096)), block, 0, stream,
                     x, xpad, rows, F);
  switch (act) {
    case VS_ACT_RELU: hipLaunchKernelGGL(bn_act_bwd_stats_kernel<VS_ACT_RELU>, grid, block, 0, stream, da, z, C, (long long)B, L, scale, shift, mean, invstd, stats); break;
    case VS_ACT_MISH: hipLaunchKernelGGL(bn_act_bwd_stats_kernel<VS_ACT_MISH>, grid, block, 0, stream, da, z, C, (long long)B, L, scale, shift, mean, invstd, stats); break;
    case VS_ACT_NONE: hipLaunchKernelGGL(bn_act_bwd_stats_kernel<VS_ACT_NONE>, grid, block, 0, stream, da, z, C, (long long)B, L, scale, shift, mean, invstd, stats); break;
    default: VS_REQUIRE(false, "bn_act_bwd_first: unknown activation %d", act);
  }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(1), dim3(64), 0, stream, stats, (double)B * L, train, C,
                     scale, mean, invstd, dgamma, dbeta, dbias, coef);
  switch (act) {
    case VS_ACT_RELU: hipLaunchKernelGGL(bn_act_bwd_first_kernel<VS_ACT_RELU>, grid, block, 0, stream, da, z, xpad, (long long)B, T, F, scale, shift, coef, acc); break;
    case VS_ACT_MISH: hipLaunchKernelGGL(bn_act_bwd_first_kernel<VS_ACT_MISH>, grid, block, 0, stream, da, z, xpad, (long long)B, T, F, scale, shift, coef, acc); break;
    default: hipLaunchKernelGGL(bn_act_bwd_first_kernel<VS_ACT_NONE>, grid, block, 0, stream, da, z, xpad, (long long)B, T, F, scale, shift, coef, acc); break;
  }
  return vs_cvt_f64_f32_impl(acc, dw, 448, stream);
}
