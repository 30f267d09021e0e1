// Training mixtures from a pool of clean utterances resident on the device: what mix_wavfiles (utils/generic_utils.py:300-345)
// does on the CPU one triplet at a time around librosa.
//
// The pool is ONE flat fp32 buffer of `total` samples; clip i is samples[offsets[i] : offsets[i + 1]] (int64 offsets: a pool of a
// few hundred thousand utterances holds more than 2^31 samples).
//
// vs_trim_bounds: librosa.effects.trim(y, top_db=20) with its defaults (frame_length 2048, hop_length 512, ref=np.max), as
// stated in include/voicesplit_hip.h.  A frame is four consecutive 512-sample blocks of the reflect-padded clip, so
//   trim_clip_kernel  one workgroup per clip, three phases behind workgroup barriers:
//     1. a wave per 512-sample block (block_sumsq, mix_common.h): its sum of squares in fp64 (fp32 squares are exact in fp64) -> the clip's slice of the
//        workspace.  A block that lies inside the clip is read with 16-byte loads from the first 16-byte boundary on, the up to
//        three samples in front and behind by single lanes (clip offsets are arbitrary); the blocks that touch the reflect padding
//        (the first two and the last three or four of a clip) index sample by sample and never leave [0, n) of their own clip;
//     2. a thread per frame: mse = (s[f] + s[f+1] + s[f+2] + s[f+3]) / 2048, the clip's maximum, then the first and last frame
//        with max(1e-10, mse) / max(1e-10, max mse) > 1e-2;
//     3. optionally max |y| over the trimmed region (the planner drops clips whose trimmed region is all zero).
// It runs once per pool.
//
// vs_mix_clips: one batch, on the caller's stream, in four launches that allocate nothing:
//   memset            the B max slots (the `norm` array itself, read as bit patterns) := 0
//   mix_max_kernel    grid (chunks of 2048 samples, B): max |c + i| of the chunk -> atomicMax on the slot.  The maximum of
//                     non-negative floats is the maximum of their bit patterns and does not depend on arrival order: reruns are
//                     bit-identical
//   mix_scale_kernel  the same grid: norm = float(1.1 * double(m)) computed by every workgroup for itself from the slot,
//                     mixed = (c + i) / norm, target = c / norm (IEEE division); all-zero rows when m == 0
//   mix_final_kernel  slot -> norm[b] = float(1.1 * double(m)), valid[b]
// Both streaming kernels are ONE sweep of short-lived workgroups, 16 bytes per lane where the addresses allow it:
// the two source rows start at arbitrary samples, each with its own misalignment, so their loads are four-byte-aligned vector
// loads; the output rows are 16-byte aligned whenever L is a multiple of four.
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"
#include "mix_common.h"

namespace {

constexpr int kMaxClips = 1 << 24;
constexpr double kRatio = 1e-2;                        // top_db = 20

// clip i owns ws[floor(offsets[i] / 512) + 4 i, + n_i / 512 + 4): disjoint for consecutive clips, no prefix sum needed
__host__ __device__ inline long long trim_slice(long long off, long long i) { return off / kHop + 4 * i; }

__global__ void __launch_bounds__(256) trim_clip_kernel(const float* __restrict__ samples, const long long* __restrict__ offsets,
                                                        double* __restrict__ ws, int* __restrict__ bounds, float* __restrict__ peak) {
  __shared__ double red_d[256];
  __shared__ int red_lo[256], red_hi[256];
  const long long clip = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long off = offsets[clip];
  const int n = (int)(offsets[clip + 1] - off);
  const float* __restrict__ y = samples + off;
  double* __restrict__ s = ws + trim_slice(off, clip);
  const int nblocks = n / kHop + 4, nframes = n / kHop + 1;

  // 1. block b = padded samples [512 b, 512 b + 512) = clip samples k0 .. k0 + 511, k0 = 512 b - 1024
  for (int b = wave; b < nblocks; b += 4) {
    const double acc = block_sumsq(samples, off, n, b, lane);
    if (lane == 0) s[b] = acc;
  }
  __syncthreads();                                                     // the block sums of this clip, written by this workgroup

  // 2. frames
  double mx = 0.0;
  for (int f = tid; f < nframes; f += 256) mx = fmax(mx, ((s[f] + s[f + 1]) + (s[f + 2] + s[f + 3])) * (1.0 / kFrame));
  red_d[tid] = mx;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red_d[tid] = fmax(red_d[tid], red_d[tid + st]);
    __syncthreads();
  }
  const double ref = fmax(kAmin, red_d[0]);
  int lo = 0x7fffffff, hi = -1;
  for (int f = tid; f < nframes; f += 256) {
    const double mse = ((s[f] + s[f + 1]) + (s[f + 2] + s[f + 3])) * (1.0 / kFrame);
    if (fmax(kAmin, mse) / ref > kRatio) {
      lo = min(lo, f);
      hi = max(hi, f);
    }
  }
  red_lo[tid] = lo;
  red_hi[tid] = hi;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      red_lo[tid] = min(red_lo[tid], red_lo[tid + st]);
      red_hi[tid] = max(red_hi[tid], red_hi[tid + st]);
    }
    __syncthreads();
  }
  const int first = red_lo[0], last = red_hi[0];
  const int start = last >= 0 ? first * kHop : 0;
  const int end = last >= 0 ? min(n, (last + 1) * kHop) : 0;
  if (tid == 0) {
    bounds[2 * clip] = start;
    bounds[2 * clip + 1] = end;
  }
  if (!peak) return;

  // 3. max |y| over [start, end)
  float pk = 0.f;
  for (int k = start + tid; k < end; k += 256) pk = fmaxf(pk, fabsf(y[k]));
  __syncthreads();
  float* red_f = reinterpret_cast<float*>(red_d);
  red_f[tid] = pk;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red_f[tid] = fmaxf(red_f[tid], red_f[tid + st]);
    __syncthreads();
  }
  if (tid == 0) peak[clip] = red_f[0];
}

// ---- mixtures ---------------------------------------------------------------------------------------------------------------
constexpr int kMixChunk = 2048;                        // samples of one row per workgroup: 256 lanes x 2 x 4

__device__ __forceinline__ bool mix_in_range(long long at, int L, long long total) { return at >= 0 && at <= total - L; }

__global__ void __launch_bounds__(256) mix_max_kernel(const float* __restrict__ samples, long long total,
                                                      const long long* __restrict__ clean_at, const long long* __restrict__ interf_at,
                                                      int L, unsigned* __restrict__ slot) {
  __shared__ float red[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long ca = clean_at[b], ia = interf_at[b];
  if (!mix_in_range(ca, L, total) || !mix_in_range(ia, L, total)) return;      // uniform: the slot stays 0, valid = -1
  const float* __restrict__ c = samples + ca;
  const float* __restrict__ x = samples + ia;
  float m = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = blockIdx.x * kMixChunk + (u * 256 + tid) * 4;
    if (j + 3 < L) {
      const f32x4_a4 cv = *reinterpret_cast<const f32x4_a4*>(c + j);
      const f32x4_a4 xv = *reinterpret_cast<const f32x4_a4*>(x + j);
      m = fmaxf(fmaxf(m, fmaxf(fabsf(cv.x + xv.x), fabsf(cv.y + xv.y))), fmaxf(fabsf(cv.z + xv.z), fabsf(cv.w + xv.w)));
    } else {
      for (int k = j; k < L; ++k) m = fmaxf(m, fabsf(c[k] + x[k]));
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.f) atomicMax(slot + b, __float_as_uint(m));              // m >= 0: the order of the bit patterns is the order of the values
  }
}

__global__ void __launch_bounds__(256) mix_scale_kernel(const float* __restrict__ samples, long long total,
                                                        const long long* __restrict__ clean_at, const long long* __restrict__ interf_at,
                                                        int L, const unsigned* __restrict__ slot, float* __restrict__ mixed,
                                                        float* __restrict__ target) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const float m = __uint_as_float(slot[b]);
  const bool zero = m == 0.f;                                          // silent sum, or an index out of range: rows of zeros, nothing read
  const float norm = mix_norm(m);
  const float* __restrict__ c = samples + (zero ? 0 : clean_at[b]);
  const float* __restrict__ x = samples + (zero ? 0 : interf_at[b]);
  float* __restrict__ mo = mixed + (long long)b * L;
  float* __restrict__ to = target + (long long)b * L;
  const bool rows_aligned = (L & 3) == 0;                              // and the output bases are 16-byte aligned (checked by the host)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = blockIdx.x * kMixChunk + (u * 256 + tid) * 4;
    if (j + 3 < L) {
      float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), tv = mv;
      if (!zero) {
        const f32x4_a4 cv = *reinterpret_cast<const f32x4_a4*>(c + j);
        const f32x4_a4 xv = *reinterpret_cast<const f32x4_a4*>(x + j);
        mv = make_float4((cv.x + xv.x) / norm, (cv.y + xv.y) / norm, (cv.z + xv.z) / norm, (cv.w + xv.w) / norm);
        tv = make_float4(cv.x / norm, cv.y / norm, cv.z / norm, cv.w / norm);
      }
      if (rows_aligned) {
        *reinterpret_cast<float4*>(mo + j) = mv;
        *reinterpret_cast<float4*>(to + j) = tv;
      } else {
        mo[j] = mv.x; mo[j + 1] = mv.y; mo[j + 2] = mv.z; mo[j + 3] = mv.w;
        to[j] = tv.x; to[j + 1] = tv.y; to[j + 2] = tv.z; to[j + 3] = tv.w;
      }
    } else {
      for (int k = j; k < L; ++k) {
        mo[k] = zero ? 0.f : (c[k] + x[k]) / norm;
        to[k] = zero ? 0.f : c[k] / norm;
      }
    }
  }
}

__global__ void __launch_bounds__(64) mix_final_kernel(long long total, const long long* __restrict__ clean_at,
                                                       const long long* __restrict__ interf_at, int B, int L, float* __restrict__ norm,
                                                       int* __restrict__ valid, int* __restrict__ invalid_count) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float m = __uint_as_float(reinterpret_cast<const unsigned*>(norm)[b]);
  const bool in_range = mix_in_range(clean_at[b], L, total) && mix_in_range(interf_at[b], L, total);
  const int v = !in_range ? -1 : (m == 0.f ? 0 : 1);
  norm[b] = mix_norm(m);
  valid[b] = v;
  if (invalid_count && v != 1) atomicAdd(invalid_count, 1);
}

int trim_check(long long total, const long long* offsets_host, int N) {
  VS_REQUIRE(N > 0 && N <= kMaxClips, "trim_bounds: N=%d clips (1 .. %d)", N, kMaxClips);
  VS_REQUIRE(total > 0 && offsets_host, "trim_bounds: total=%lld samples, host offsets %s", total, offsets_host ? "given" : "NULL");
  VS_REQUIRE(offsets_host[0] >= 0 && offsets_host[N] <= total, "trim_bounds: offsets [%lld, %lld] leave the buffer of %lld samples",
             offsets_host[0], offsets_host[N], total);
  for (int i = 0; i < N; ++i) {
    const long long n = offsets_host[i + 1] - offsets_host[i];
    VS_REQUIRE(n >= kMinClip, "trim_bounds: clip %d has %lld samples, fewer than %d (the reflect padding of 1024 samples would wrap)",
               i, n, kMinClip);
    VS_REQUIRE(n <= kMaxClip, "trim_bounds: clip %d has %lld samples, more than %lld", i, n, kMaxClip);
  }
  return 0;
}

}  // namespace

size_t vs_trim_workspace_bytes(long long total, int N) {
  if (total <= 0 || N <= 0 || N > kMaxClips) {
    vs_set_error("trim_workspace_bytes: total=%lld samples, N=%d clips", total, N);
    return 0;
  }
  return align_up((size_t)(total / kHop + 4LL * N + 4) * sizeof(double));
}

int vs_trim_bounds(const float* samples, long long total, const long long* offsets_host, const long long* offsets, int N,
                   int* bounds, float* peak, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = trim_check(total, offsets_host, N)) return rc;
  VS_REQUIRE(samples && offsets && bounds && ws, "trim_bounds: NULL argument");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(samples) & 15) == 0, "trim_bounds: the sample buffer must be 16-byte aligned");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= vs_trim_workspace_bytes(total, N),
             "trim_bounds: workspace too small or misaligned (%zu < %zu)", ws_bytes, vs_trim_workspace_bytes(total, N));
  hipLaunchKernelGGL(trim_clip_kernel, dim3((unsigned)N), dim3(256), 0, stream, samples, offsets, static_cast<double*>(ws), bounds, peak);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_mix_clips(const float* samples, long long total, const long long* clean_at, const long long* interf_at, int B, int L,
                 float* mixed_wav, float* target_wav, float* norm, int* valid, int* invalid_count, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(B > 0 && B <= 65535, "mix_clips: B=%d (1 .. 65535)", B);
  VS_REQUIRE(L > 0 && L <= (1 << 30) && total >= L, "mix_clips: L=%d samples from a buffer of %lld", L, total);
  VS_REQUIRE(samples && clean_at && interf_at && mixed_wav && target_wav && norm && valid, "mix_clips: NULL argument");
  VS_REQUIRE(((reinterpret_cast<uintptr_t>(mixed_wav) | reinterpret_cast<uintptr_t>(target_wav)) & 15) == 0,
             "mix_clips: the output rows must be 16-byte aligned");
  unsigned* slot = reinterpret_cast<unsigned*>(norm);
  const dim3 grid((unsigned)((L + kMixChunk - 1) / kMixChunk), (unsigned)B);
  VS_CHECK_HIP(hipMemsetAsync(slot, 0, (size_t)B * sizeof(unsigned), stream));
  hipLaunchKernelGGL(mix_max_kernel, grid, dim3(256), 0, stream, samples, total, clean_at, interf_at, L, slot);
  hipLaunchKernelGGL(mix_scale_kernel, grid, dim3(256), 0, stream, samples, total, clean_at, interf_at, L, slot, mixed_wav, target_wav);
  hipLaunchKernelGGL(mix_final_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, total, clean_at, interf_at, B, L, norm, valid,
                     invalid_count);
  VS_LAUNCH_CHECK();
  return 0;
}
