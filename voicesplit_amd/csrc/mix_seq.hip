// The noisy training items without voice overlay: what mix_wavfiles_without_voice_overlay (utils/generic_utils.py:27-296) does on
// the CPU around librosa.effects.split and sklearn's minmax_scale, as stated in include/voicesplit_hip.h.
//
// vs_clip_range     clip_range_kernel, a workgroup per clip: min and max of the trimmed region.  Once per pool.
// vs_split_point    split_point_kernel, a workgroup per region, the block-sum scheme of trim_clip_kernel (mix_common.h):
//     1. a wave per 512-sample block of the reflect-padded region: its sum of squares in fp64 -> the region's workspace slice;
//     2. the region's maximum frame energy;
//     3. every thread owns a contiguous run of frames and counts the interval starts (a non-silent frame behind a silent one) and
//        ends in it; thread 0 turns the 256 counts into offsets; the threads walk their runs again and write the intervals, and the
//        one that meets end number count / 2 writes the split point.
// vs_mix_sequence   on the caller's stream, nothing allocated:
//   memset             aux := 0: the three slots of every item (bit patterns; the minimum's key is stored inverted so that all
//                      three are maxima over a zero)
//   seq_range_kernel   grid (chunks of 2048 samples of the range slice, B): min and max of n1 + n2 -> atomicMax on the key slots.
//                      The key of a float orders like the float, so the result does not depend on arrival order
//   seq_sweep_kernel<false>  grid (chunks of 2048 output samples, B): max |v| of the chunk -> atomicMax on the item's slot
//   seq_sweep_kernel<true>   the same grid: every workgroup forms the noise affines and the norm for itself from the slots and
//                      writes its 2048 samples of both rows, zeros behind the item's end
//   seq_final_kernel   slots -> aux, norm, valid
// The streaming kernels are ONE sweep of short-lived workgroups.  A workgroup resolves the item's segment ends once;
// a lane's four samples take the vector path (four-byte-aligned 16-byte loads of the voice and of both noises) when they lie in one
// segment, and sample by sample across a segment boundary or the item's end.  Rows are stored 16 bytes per lane when L % 4 == 0.
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"
#include "mix_common.h"

namespace {

constexpr int kMaxItems = 1 << 24;
constexpr int kSeqChunk = 2048;                        // samples of one row per workgroup: 256 lanes x 2 x 4
constexpr int kAux = 8;                                // floats of aux per item: slots 0 .. 2 during the call

// a key that orders like the float (finite values; -0 below +0)
__device__ __forceinline__ unsigned f32_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- vs_clip_range ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) clip_range_kernel(const float* __restrict__ samples, const long long* __restrict__ offsets,
                                                         const int* __restrict__ bounds, float* __restrict__ range) {
  __shared__ float red_lo[256], red_hi[256];
  const long long clip = blockIdx.x;
  const int tid = threadIdx.x;
  const long long off = offsets[clip];
  const int n = (int)(offsets[clip + 1] - off);
  int start = 0, end = n;
  if (bounds) {
    start = max(0, min(n, bounds[2 * clip]));
    end = max(start, min(n, bounds[2 * clip + 1]));
  }
  const float* __restrict__ y = samples + off;
  float lo = INFINITY, hi = -INFINITY;
  for (int k = start + tid; k < end; k += 256) {
    const float x = y[k];
    lo = fminf(lo, x);
    hi = fmaxf(hi, x);
  }
  red_lo[tid] = lo;
  red_hi[tid] = hi;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      red_lo[tid] = fminf(red_lo[tid], red_lo[tid + st]);
      red_hi[tid] = fmaxf(red_hi[tid], red_hi[tid + st]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    range[2 * clip] = end > start ? red_lo[0] : 0.f;
    range[2 * clip + 1] = end > start ? red_hi[0] : 0.f;
  }
}

// ---- vs_split_point ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline long long split_slice(long long n_max) { return n_max / kHop + 4; }     // doubles per region

__global__ void __launch_bounds__(256) split_point_kernel(const float* __restrict__ samples, const long long* __restrict__ regions,
                                                          const double* __restrict__ ratio, long long ws_stride,
                                                          double* __restrict__ ws, int* __restrict__ count, int* __restrict__ split,
                                                          int* __restrict__ intervals, int cap) {
  __shared__ double red_d[256];
  __shared__ int n_start[256], n_end[256];
  const long long item = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long off = regions[2 * item];
  const int n = (int)regions[2 * item + 1];
  double* __restrict__ s = ws + item * ws_stride;
  const int nblocks = n / kHop + 4, nframes = n / kHop + 1;

  // 1. block sums; the reflection stays inside [off, off + n)
  for (int b = wave; b < nblocks; b += 4) {
    const double acc = block_sumsq(samples, off, n, b, lane);
    if (lane == 0) s[b] = acc;
  }
  __syncthreads();

  // 2. the reference level
  double mx = 0.0;
  for (int f = tid; f < nframes; f += 256) mx = fmax(mx, frame_mse(s, f));
  red_d[tid] = mx;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red_d[tid] = fmax(red_d[tid], red_d[tid + st]);
    __syncthreads();
  }
  const double ref = fmax(kAmin, red_d[0]), rt = ratio[item];
  auto loud = [&](int f) { return f >= 0 && f < nframes && fmax(kAmin, frame_mse(s, f)) / ref > rt; };

  // 3. intervals: a start at f when f is loud and f - 1 is not, an end at f (exclusive) when f - 1 is loud and f is not; frame
  // nframes counts as silent, and the last thread owns that transition
  const int per = (nframes + 255) / 256;
  const int f_lo = min(nframes, tid * per), f_hi = min(nframes, f_lo + per);
  int ns = 0, ne = 0;
  {
    bool prev = loud(f_lo - 1);
    for (int f = f_lo; f < f_hi; ++f) {
      const bool cur = loud(f);
      ns += cur && !prev;
      ne += !cur && prev;
      prev = cur;
    }
    if (tid == 255 && loud(nframes - 1)) ++ne;
  }
  n_start[tid] = ns;
  n_end[tid] = ne;
  __syncthreads();
  if (tid == 0) {
    int as = 0, ae = 0;
    for (int k = 0; k < 256; ++k) {
      const int vs = n_start[k], ve = n_end[k];
      n_start[k] = as;
      n_end[k] = ae;
      as += vs;
      ae += ve;
    }
    red_d[0] = (double)as;                                             // starts and ends pair up: as == ae
  }
  __syncthreads();
  const int total = (int)red_d[0], mid = total / 2;
  int ks = n_start[tid], ke = n_end[tid];
  int* __restrict__ row = intervals ? intervals + item * cap * 2 : nullptr;
  auto put_end = [&](int f) {
    const int v = min(n, f * kHop);
    if (row && ke < cap) row[2 * ke + 1] = v;
    if (ke == mid) split[item] = v;
    ++ke;
  };
  bool prev = loud(f_lo - 1);
  for (int f = f_lo; f < f_hi; ++f) {
    const bool cur = loud(f);
    if (cur && !prev) {
      if (row && ks < cap) row[2 * ks] = f * kHop;
      ++ks;
    }
    if (!cur && prev) put_end(f);
    prev = cur;
  }
  if (tid == 255 && loud(nframes - 1)) put_end(nframes);
  if (tid == 0) {
    count[item] = total;
    if (total == 0) split[item] = n;                                   // ratio >= 1 (or NaN): no frame is loud; the header's fallback
  }
}

// ---- vs_mix_sequence --------------------------------------------------------------------------------------------------------
struct SeqItem {
  bool ok, noise;        // the item's indices are inside both buffers; a segment has a noise_sel >= 0
  int e0, e1, n;         // segment ends: segment 0 is [0, e0), 1 is [e0, e1), 2 is [e1, n)
};

// every workgroup checks its item for itself (uniform): an item that fails is not read
__device__ __forceinline__ SeqItem seq_resolve(const vs_seq_item& it, int L, int R, long long total, long long noise_total) {
  SeqItem r;
  bool ok = true, noise = false;
  long long n = 0;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int len = it.len[s];
    ok = ok && len >= 0 && len <= L;
    if (len > 0) {
      ok = ok && it.src_at[s] >= 0 && it.src_at[s] <= total - len && it.noise_sel[s] >= -1 && it.noise_sel[s] <= 1;
      noise = noise || it.noise_sel[s] >= 0;
    }
    n += len;
  }
  ok = ok && n <= L;
  if (ok && noise) {
    const int rl = it.range_len;
    ok = it.noise1_at >= 0 && it.noise1_at <= noise_total - n && it.noise2_at >= 0 && it.noise2_at <= noise_total - n &&
         rl >= 1 && rl <= R && it.range_at1 >= 0 && it.range_at1 <= noise_total - rl && it.range_at2 >= 0 &&
         it.range_at2 <= noise_total - rl;
  }
  r.ok = ok;
  r.noise = ok && noise;
  r.e0 = ok ? it.len[0] : 0;
  r.e1 = ok ? it.len[0] + it.len[1] : 0;
  r.n = ok ? (int)n : 0;
  return r;
}

struct SeqAffine { float g[2], b[2]; };

// minmax_scale's affine for both feature ranges from the slots of the range pass: fp64 without contraction, rounded once
__device__ __forceinline__ SeqAffine seq_affine(const unsigned* __restrict__ ax, const vs_seq_item& it, bool noise, float* nmin_out,
                                                float* nmax_out) {
  SeqAffine a = {{0.f, 0.f}, {0.f, 0.f}};
  float nmin = 0.f, nmax = 0.f;
  if (noise) {
    nmin = key_f32(~ax[0]);
    nmax = key_f32(ax[1]);
    double den = __dsub_rn((double)nmax, (double)nmin);
    if (den == 0.0) den = 1.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double sc = __ddiv_rn(__dsub_rn((double)it.hi[k], (double)it.lo[k]), den);
      a.g[k] = (float)sc;
      a.b[k] = (float)__dsub_rn((double)it.lo[k], __dmul_rn((double)nmin, sc));
    }
  }
  if (nmin_out) *nmin_out = nmin;
  if (nmax_out) *nmax_out = nmax;
  return a;
}

__global__ void __launch_bounds__(256) seq_range_kernel(const float* __restrict__ noise, long long total, long long noise_total,
                                                        const vs_seq_item* __restrict__ items, int L, int R,
                                                        unsigned* __restrict__ aux) {
  __shared__ float red_lo[4], red_hi[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const vs_seq_item& it = items[b];
  const SeqItem r = seq_resolve(it, L, R, total, noise_total);
  const int rl = it.range_len, j0 = blockIdx.x * kSeqChunk;
  if (!r.noise || j0 >= rl) return;                                    // uniform
  const float* __restrict__ a = noise + it.range_at1;
  const float* __restrict__ c = noise + it.range_at2;
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = j0 + (u * 256 + tid) * 4;
    if (j + 3 < rl) {
      const f32x4_a4 av = *reinterpret_cast<const f32x4_a4*>(a + j);
      const f32x4_a4 cv = *reinterpret_cast<const f32x4_a4*>(c + j);
      const float s0 = av.x + cv.x, s1 = av.y + cv.y, s2 = av.z + cv.z, s3 = av.w + cv.w;
      lo = fminf(fminf(lo, fminf(s0, s1)), fminf(s2, s3));
      hi = fmaxf(fmaxf(hi, fmaxf(s0, s1)), fmaxf(s2, s3));
    } else {
      for (int k = j; k < rl; ++k) {
        const float sk = a[k] + c[k];
        lo = fminf(lo, sk);
        hi = fmaxf(hi, sk);
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  if ((tid & 63) == 0) {
    red_lo[tid >> 6] = lo;
    red_hi[tid >> 6] = hi;
  }
  __syncthreads();
  if (tid == 0) {                                                      // j0 < rl: the workgroup saw at least one sample
    lo = fminf(fminf(red_lo[0], red_lo[1]), fminf(red_lo[2], red_lo[3]));
    hi = fmaxf(fmaxf(red_hi[0], red_hi[1]), fmaxf(red_hi[2], red_hi[3]));
    atomicMax(aux + (long long)b * kAux, ~f32_key(lo));
    atomicMax(aux + (long long)b * kAux + 1, f32_key(hi));
  }
}

// kWrite == false: max |v| of the chunk -> slot 2.  kWrite == true: both rows of the chunk.
template <bool kWrite>
__global__ void __launch_bounds__(256) seq_sweep_kernel(const float* __restrict__ samples, long long total,
                                                        const float* __restrict__ noise, long long noise_total,
                                                        const vs_seq_item* __restrict__ items, int L, int R,
                                                        const float* __restrict__ norm_in, unsigned* __restrict__ aux,
                                                        float* __restrict__ mixed, float* __restrict__ target) {
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const vs_seq_item& it = items[b];
  const SeqItem r = seq_resolve(it, L, R, total, noise_total);
  unsigned* __restrict__ ax = aux + (long long)b * kAux;
  const int j0 = blockIdx.x * kSeqChunk;
  if (!kWrite && j0 >= r.n) return;                                    // uniform: nothing of the item in this chunk
  const SeqAffine na = seq_affine(ax, it, r.noise, nullptr, nullptr);
  float norm = 1.f;
  bool zero = false;
  if (kWrite) {
    norm = norm_in ? norm_in[b] : mix_norm(__uint_as_float(ax[2]));
    zero = !r.ok || norm == 0.f;                                       // refused or silent: rows of zeros, nothing read
  }
  // per segment: the voice sample of output t is samples[base[s] + t]
  const long long base0 = it.src_at[0], base1 = it.src_at[1] - r.e0, base2 = it.src_at[2] - r.e1;
  const float* __restrict__ n1 = noise + (r.noise ? it.noise1_at : 0);
  const float* __restrict__ n2 = noise + (r.noise ? it.noise2_at : 0);
  auto seg_of = [&](int t) { return t < r.e0 ? 0 : (t < r.e1 ? 1 : 2); };
  auto value = [&](float x, float a, float c, float gain, float bias, int sel) {
    float v = fmaf(gain, x, bias);
    if (sel >= 0) v = v + fmaf(sel ? na.g[1] : na.g[0], a + c, sel ? na.b[1] : na.b[0]);
    return v;
  };
  float* __restrict__ mo = kWrite ? mixed + (long long)b * L : nullptr;
  float* __restrict__ to = kWrite ? target + (long long)b * L : nullptr;
  const bool rows_aligned = (L & 3) == 0;                              // and the output bases are 16-byte aligned (checked by the host)
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = j0 + (u * 256 + tid) * 4;
    if (j >= (kWrite ? L : r.n)) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
    if (!zero) {
      const int s = seg_of(j);
      if (j + 3 < r.n && seg_of(j + 3) == s) {
        const float gain = it.gain[s], bias = it.bias[s];
        const int sel = it.noise_sel[s];
        const bool tgt = it.in_target[s] != 0;
        const long long base = s == 0 ? base0 : (s == 1 ? base1 : base2);
        const f32x4_a4 xv = *reinterpret_cast<const f32x4_a4*>(samples + base + j);
        f32x4_a4 av = {0.f, 0.f, 0.f, 0.f}, cv = av;
        if (sel >= 0) {
          av = *reinterpret_cast<const f32x4_a4*>(n1 + j);
          cv = *reinterpret_cast<const f32x4_a4*>(n2 + j);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[k] = value(xv[k], av[k], cv[k], gain, bias, sel);
          w[k] = tgt ? v[k] : 0.f;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int t = j + k;
          if (t < r.n) {
            const int st = seg_of(t);
            const int sel = it.noise_sel[st];
            const long long base = st == 0 ? base0 : (st == 1 ? base1 : base2);
            v[k] = value(samples[base + t], sel >= 0 ? n1[t] : 0.f, sel >= 0 ? n2[t] : 0.f, it.gain[st], it.bias[st], sel);
            w[k] = it.in_target[st] != 0 ? v[k] : 0.f;
          }
        }
      }
    }
    if (kWrite) {
      if (!zero) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                  // 0 / norm = 0 behind the item's end and in silent target segments
          v[k] = v[k] / norm;
          w[k] = w[k] / norm;
        }
      }
      if (j + 3 < L && rows_aligned) {
        *reinterpret_cast<float4*>(mo + j) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(to + j) = make_float4(w[0], w[1], w[2], w[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (j + k < L) {
            mo[j + k] = v[k];
            to[j + k] = w[k];
          }
        }
      }
    } else {
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
  }
  if (!kWrite) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
      if (m > 0.f) atomicMax(ax + 2, __float_as_uint(m));              // m >= 0: the order of the bit patterns is the order of the values
    }
  }
}

__global__ void __launch_bounds__(64) seq_final_kernel(long long total, long long noise_total, const vs_seq_item* __restrict__ items,
                                                       int B, int L, int R, const float* __restrict__ norm_in, float* __restrict__ aux,
                                                       float* __restrict__ norm, int* __restrict__ valid,
                                                       int* __restrict__ invalid_count) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const vs_seq_item& it = items[b];
  const SeqItem r = seq_resolve(it, L, R, total, noise_total);
  float* __restrict__ ax = aux + (long long)b * kAux;
  float nmin, nmax;
  const SeqAffine na = seq_affine(reinterpret_cast<const unsigned*>(ax), it, r.noise, &nmin, &nmax);
  const float m = r.ok ? ax[2] : 0.f;
  const float nb = norm_in ? norm_in[b] : mix_norm(m);
  const int v = !r.ok ? -1 : (nb != 0.f ? 1 : 0);
  ax[0] = nmin;
  ax[1] = nmax;
  ax[2] = m;
  ax[3] = na.g[0];
  ax[4] = na.b[0];
  ax[5] = na.g[1];
  ax[6] = na.b[1];
  ax[7] = 0.f;
  norm[b] = nb;
  valid[b] = v;
  if (invalid_count && v != 1) atomicAdd(invalid_count, 1);
}

}  // namespace

int vs_clip_range(const float* samples, long long total, const long long* offsets_host, const long long* offsets, const int* bounds,
                  int N, float* range, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(N > 0 && N <= kMaxItems, "clip_range: N=%d clips (1 .. %d)", N, kMaxItems);
  VS_REQUIRE(total > 0 && offsets_host, "clip_range: total=%lld samples, host offsets %s", total, offsets_host ? "given" : "NULL");
  VS_REQUIRE(offsets_host[0] >= 0 && offsets_host[N] <= total, "clip_range: offsets [%lld, %lld] leave the buffer of %lld samples",
             offsets_host[0], offsets_host[N], total);
  for (int i = 0; i < N; ++i) {
    const long long n = offsets_host[i + 1] - offsets_host[i];
    VS_REQUIRE(n >= 0 && n <= kMaxClip, "clip_range: clip %d has %lld samples (0 .. %lld)", i, n, kMaxClip);
  }
  VS_REQUIRE(samples && offsets && range, "clip_range: NULL argument");
  hipLaunchKernelGGL(clip_range_kernel, dim3((unsigned)N), dim3(256), 0, stream, samples, offsets, bounds, range);
  VS_LAUNCH_CHECK();
  return 0;
}

size_t vs_split_workspace_bytes(long long n_max, int B) {
  if (n_max < kMinClip || n_max > kMaxClip || B <= 0 || B > kMaxItems) {
    vs_set_error("split_workspace_bytes: n_max=%lld samples (%d .. %lld), B=%d regions", n_max, kMinClip, kMaxClip, B);
    return 0;
  }
  return align_up((size_t)(split_slice(n_max) * B) * sizeof(double));
}

int vs_split_point(const float* samples, long long total, const long long* regions_host, const long long* regions,
                   const double* ratio, int B, int* count, int* split, int* intervals, int cap, void* ws, size_t ws_bytes,
                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(B > 0 && B <= kMaxItems, "split_point: B=%d regions (1 .. %d)", B, kMaxItems);
  VS_REQUIRE(total > 0 && regions_host, "split_point: total=%lld samples, host regions %s", total, regions_host ? "given" : "NULL");
  long long n_max = 0;
  for (int b = 0; b < B; ++b) {
    const long long at = regions_host[2 * b], n = regions_host[2 * b + 1];
    VS_REQUIRE(n >= kMinClip, "split_point: region %d has %lld samples, fewer than %d (the reflect padding of 1024 samples would wrap)",
               b, n, kMinClip);
    VS_REQUIRE(n <= kMaxClip, "split_point: region %d has %lld samples, more than %lld", b, n, kMaxClip);
    VS_REQUIRE(at >= 0 && at <= total - n, "split_point: region %d [%lld, +%lld) leaves the buffer of %lld samples", b, at, n, total);
    n_max = n > n_max ? n : n_max;
  }
  VS_REQUIRE(samples && regions && ratio && count && split && ws, "split_point: NULL argument");
  VS_REQUIRE(!intervals || cap > 0, "split_point: an interval buffer of cap=%d", cap);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(samples) & 15) == 0, "split_point: the sample buffer must be 16-byte aligned");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= vs_split_workspace_bytes(n_max, B),
             "split_point: workspace too small or misaligned (%zu < %zu)", ws_bytes, vs_split_workspace_bytes(n_max, B));
  hipLaunchKernelGGL(split_point_kernel, dim3((unsigned)B), dim3(256), 0, stream, samples, regions, ratio, split_slice(n_max),
                     static_cast<double*>(ws), count, split, intervals, cap);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_mix_sequence(const float* samples, long long total, const float* noise, long long noise_total, const vs_seq_item* items,
                    int B, int L, int R, const float* norm_in, float* mixed_wav, float* target_wav, float* norm, float* aux,
                    int* valid, int* invalid_count, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(B > 0 && B <= 65535, "mix_sequence: B=%d (1 .. 65535)", B);
  VS_REQUIRE(L > 0 && L <= (1 << 30) && R > 0 && R <= (1 << 30), "mix_sequence: L=%d, R=%d samples (1 .. 2^30)", L, R);
  VS_REQUIRE(total > 0 && noise_total > 0, "mix_sequence: buffers of %lld and %lld samples", total, noise_total);
  VS_REQUIRE(samples && noise && items && norm && aux && valid, "mix_sequence: NULL argument");
  VS_REQUIRE((mixed_wav == nullptr) == (target_wav == nullptr), "mix_sequence: mixed_wav and target_wav are given or left out together");
  VS_REQUIRE(mixed_wav || !norm_in, "mix_sequence: norm_in without output rows leaves nothing to compute");
  VS_REQUIRE(((reinterpret_cast<uintptr_t>(mixed_wav) | reinterpret_cast<uintptr_t>(target_wav)) & 15) == 0,
             "mix_sequence: the output rows must be 16-byte aligned");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(items) & 7) == 0 && (reinterpret_cast<uintptr_t>(aux) & 3) == 0,
             "mix_sequence: items must be 8-byte aligned");
  unsigned* slots = reinterpret_cast<unsigned*>(aux);
  const dim3 grid((unsigned)((L + kSeqChunk - 1) / kSeqChunk), (unsigned)B);
  const dim3 rgrid((unsigned)((R + kSeqChunk - 1) / kSeqChunk), (unsigned)B);
  VS_CHECK_HIP(hipMemsetAsync(slots, 0, (size_t)B * kAux * sizeof(unsigned), stream));
  hipLaunchKernelGGL(seq_range_kernel, rgrid, dim3(256), 0, stream, noise, total, noise_total, items, L, R, slots);
  if (!norm_in)
    hipLaunchKernelGGL(seq_sweep_kernel<false>, grid, dim3(256), 0, stream, samples, total, noise, noise_total, items, L, R, norm_in,
                       slots, mixed_wav, target_wav);
  if (mixed_wav)
    hipLaunchKernelGGL(seq_sweep_kernel<true>, grid, dim3(256), 0, stream, samples, total, noise, noise_total, items, L, R, norm_in,
                       slots, mixed_wav, target_wav);
  hipLaunchKernelGGL(seq_final_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, total, noise_total, items, B, L, R, norm_in, aux,
                     norm, valid, invalid_count);
  VS_LAUNCH_CHECK();
  return 0;
}
