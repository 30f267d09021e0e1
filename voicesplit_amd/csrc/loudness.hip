// Programme loudness on the device: ITU-R BS.1770-4 integrated loudness of N mono clips of unequal length in one flat buffer, and the
// linear gain that goes with it -- the `ffmpeg-normalize` half of the reference's scripts/normalise-resample.sh (the other half is
// resample.hip).  The definition (K-weighting from the bilinear transform, 100 ms sub-blocks, 400 ms blocks at 75 % overlap, the two
// gates) is the text in include/voicesplit_hip.h; its constants are those of libebur128 AS REMEMBERED and it was not compared with
// an ffmpeg or libebur128 run.
//
// The K-weighting filter is recursive, so serial in time.  It is made parallel inside a clip by cutting the clip at its sub-blocks of
// S samples: the filter is linear, so the state behind sub-block k is  s(k+1) = step s(k) + p(k)  with p(k) the state the sub-block
// leaves behind when it is entered with a zero state and `step` the zero-input map of S samples (4 x 4, built on the host).
//
//   slots_kernel     exclusive prefix sum of the clips' slot counts (m + 1 per clip): where each clip's sub-blocks live in the workspace
//   sweep_kernel<0>  zero-state sweep: one LANE per sub-block runs the recurrence over its S samples from s = 0 and stores p(k)
//   scan_kernel      one lane per clip: s(0) = 0, s(k+1) = step s(k) + p(k); p(k) is overwritten by the true start state s(k)
//   sweep_kernel<1>  energy sweep: every lane reruns its sub-block from s(k) and sums w^2 in one ascending chain into e(k); the fp32
//                    maximum of |x| of its samples too (one more lane takes the samples behind the last whole sub-block)
//   gate_kernel      one wave per clip: blocks, absolute gate, relative gate, lufs, counts, valid, the clip's peak, the copy of e
//
// sweep_kernel: a workgroup is ONE wave and owns 64 consecutive sub-blocks of one clip, grid (tiles, clips).  The lanes of a wave read
// rows S samples apart, so a [64 rows] x [32 samples] tile goes through LDS: it is loaded with the lanes ALONG the rows (each half
// wave one 128-byte run of a row, 32 loads per lane and tile), stored with a row stride of 33 floats (ds_write_b32 / ds_read_b32 have 32
// banks per half wave: rows 33 apart are conflict-free both ways), and read back with one lane per row.  The next tile's loads are
// issued before the fp64 chain of the current tile starts and land in LDS behind it (two buffers), so the chain, which is what bounds
// a lane (10 dependent fp64 operations per sample), does not wait on memory.  16.5 KiB of LDS per wave: nine waves per CU.
// KNOWN, NOT TUNED: the loads are 4 bytes per lane, not 16 (a clip may start at any sample and S may be odd, so a row has no fixed
// alignment); a clip with fewer than 64 sub-blocks leaves lanes of its one wave idle; grid.x is sized for the longest clip of a launch.
//
// Every result of a clip is a function of the clip's samples alone: a lane's chain reads its own row and its own start state, the scan
// and the gate walk one clip in an order that depends only on m, and the peak is a maximum.  Offsets, neighbours, N and the call do
// not show in a bit.
#include <math.h>
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

namespace {

constexpr int kMinRate = 8000, kMaxRate = 192000;
constexpr long long kMaxClip = 1LL << 30;
constexpr long long kMaxTotal = 1LL << 48;
constexpr int kCols = 32, kRowStride = kCols + 1, kRows = 64;
constexpr int kScaleThreads = 256, kScaleTile = kScaleThreads * 8;      // vs_scale_clips: 2048 samples per workgroup
constexpr int kSlotThreads = 1024;

// ---- the plan (host only) ----------------------------------------------------------------------------------------------------------
inline void filter_step(const vs_loudness_dims* d, double x, double* s) {
  const double u = d->b1[0] * x + s[0];
  s[0] = d->b1[1] * x - d->a1[0] * u + s[1];
  s[1] = d->b1[2] * x - d->a1[1] * u;
  const double w = u + s[2];
  s[2] = -2.0 * u - d->a2[0] * w + s[3];
  s[3] = u - d->a2[1] * w;
}

int plan(int fs, vs_loudness_dims* d) {
  VS_REQUIRE(d, "loudness_plan: NULL dims");
  VS_REQUIRE(fs >= kMinRate && fs <= kMaxRate, "loudness_plan: sample rate %d outside %d .. %d", fs, kMinRate, kMaxRate);
  memset(d, 0, sizeof(*d));
  d->sample_rate = fs;
  d->sub = (fs + 5) / 10;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(M_PI * f0 / (double)fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    d->b1[0] = (Vh + Vb * K / Q + K * K) / a0;
    d->b1[1] = 2.0 * (K * K - Vh) / a0;
    d->b1[2] = (Vh - Vb * K / Q + K * K) / a0;
    d->a1[0] = 2.0 * (K * K - 1.0) / a0;
    d->a1[1] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(M_PI * f0 / (double)fs);
    const double den = 1.0 + K / Q + K * K;
    d->b2[0] = 1.0; d->b2[1] = -2.0; d->b2[2] = 1.0;
    d->a2[0] = 2.0 * (K * K - 1.0) / den;
    d->a2[1] = (1.0 - K / Q + K * K) / den;
  }
  for (int c = 0; c < 4; ++c) {                          // the recurrence itself, S times from each unit state
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[c] = 1.0;
    for (int i = 0; i < d->sub; ++i) filter_step(d, 0.0, s);
    for (int r = 0; r < 4; ++r) d->step[r][c] = s[r];
  }
  return 0;
}

int checked(const vs_loudness_dims* dims, const char* what) {
  VS_REQUIRE(dims, "%s: NULL dims", what);
  vs_loudness_dims own;
  if (int rc = plan(dims->sample_rate, &own)) return rc;
  VS_REQUIRE(memcmp(&own, dims, sizeof(own)) == 0, "%s: dims are not what vs_loudness_plan(%d) returns", what, dims->sample_rate);
  return 0;
}

// workspace: slot_at [N + 1] int64 | state [slots][4] fp64 | energy [slots] fp64 | peak [slots] fp32, every piece 256-byte aligned
struct Layout { size_t slot_at, state, energy, peak, total; };
inline Layout layout(long long N, long long slots) {
  Layout l;
  l.slot_at = 0;
  l.state = align_up((size_t)(N + 1) * 8);
  l.energy = l.state + align_up((size_t)slots * 32);
  l.peak = l.energy + align_up((size_t)slots * 8);
  l.total = l.peak + align_up((size_t)slots * 4);
  return l;
}

struct Filter { double b10, b11, b12, a10, a11, a20, a21; };

struct Job {
  const float* samples;
  const long long* clips;                                // [N][2] = (at, n), device; already offset to the launch's first clip
  const long long* slot_at;                              // the same
  double* state;
  double* energy;
  float* peak;
  Filter f;
  int S;
};

// ---- where each clip's sub-blocks live ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSlotThreads) slots_kernel(const long long* __restrict__ clips, int N, int S, long long* __restrict__ slot_at) {
  __shared__ long long part[kSlotThreads];
  const int tid = threadIdx.x;
  const int per = (N + kSlotThreads - 1) / kSlotThreads;
  const int lo = tid * per < N ? tid * per : N, hi = lo + per < N ? lo + per : N;
  long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += clips[2LL * i + 1] / S + 1;
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kSlotThreads; d <<= 1) {            // inclusive scan
    const long long v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    slot_at[i] = run;
    run += clips[2LL * i + 1] / S + 1;
  }
  if (tid == kSlotThreads - 1) slot_at[N] = part[tid];
}

// ---- the two sweeps -------------------------------------------------------------------------------------------------------------------
template <bool ENERGY>
__global__ void __launch_bounds__(kRows) sweep_kernel(const Job j) {
  __shared__ float tile[2][kRows * kRowStride];
  const int clip = blockIdx.y, lane = threadIdx.x, S = j.S;
  const long long at = j.clips[2LL * clip], n = j.clips[2LL * clip + 1];
  const long long m = n / S;
  // rows of this clip: the zero-state sweep needs p(0 .. m - 2); the energy sweep every whole sub-block and, for the peak, the rest
  const long long rows = ENERGY ? m + (n > m * S ? 1 : 0) : m - 1;
  const long long k0 = (long long)blockIdx.x * kRows;
  if (k0 >= rows) return;                                                           // (uniform)
  const long long slot = j.slot_at[clip] + k0 + lane;
  const long long k = k0 + lane;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, e = 0.0;
  float pk = 0.f;
  if (ENERGY && k < m) {
    const double* st = j.state + 4 * slot;
    s1 = st[0]; s2 = st[1]; s3 = st[2]; s4 = st[3];
  }
  const Filter f = j.f;
  const float* __restrict__ x = j.samples + at + k0 * S;                             // sample 0 of the tile's row 0
  const long long left = n - k0 * S;                                                 // samples of the clip from there on
  const int col = lane & (kCols - 1), half = lane >> 5;
  const int nq = (S + kCols - 1) / kCols;
  float reg[kRows / 2];

  auto fetch = [&](int q) {                                                          // tile q -> reg, zero where the clip has no sample
    const int c = q * kCols + col;
#pragma unroll
    for (int i = 0; i < kRows / 2; ++i) {
      const long long idx = (long long)(2 * i + half) * S + c;
      reg[i] = (c < S && idx < left) ? x[idx] : 0.f;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kRows / 2; ++i) tile[buf][(2 * i + half) * kRowStride + col] = reg[i];
  };
  auto sample = [&](float xf) {
    if (ENERGY) pk = fmaxf(pk, fabsf(xf));
    const double xd = (double)xf;
    const double u = fma(f.b10, xd, s1);
    s1 = fma(f.b11, xd, fma(-f.a10, u, s2));
    s2 = fma(-f.a11, u, f.b12 * xd);
    const double w = u + s3;
    s3 = fma(-f.a20, w, fma(-2.0, u, s4));
    s4 = fma(-f.a21, w, u);
    if (ENERGY) e = fma(w, w, e);
  };

  fetch(0);
  stage(0);
  __syncthreads();
  for (int q = 0; q < nq; ++q) {
    const bool more = q + 1 < nq;
    if (more) fetch(q + 1);
    const float* __restrict__ row = tile[q & 1] + lane * kRowStride;
    const int cnt = S - q * kCols;                                                   // the sub-block ends inside the last tile
    if (cnt >= kCols) {
#pragma unroll
      for (int c = 0; c < kCols; ++c) sample(row[c]);
    } else {
      for (int c = 0; c < cnt; ++c) sample(row[c]);
    }
    if (more) stage((q + 1) & 1);
    __syncthreads();
  }
  if (ENERGY) {
    if (k < m) j.energy[slot] = e;
    if (k < rows) j.peak[slot] = pk;
  } else if (k < rows) {
    double* st = j.state + 4 * slot;
    st[0] = s1; st[1] = s2; st[2] = s3; st[3] = s4;
  }
}

struct Step { double m[4][4]; };

__global__ void __launch_bounds__(256) scan_kernel(const long long* __restrict__ clips, const long long* __restrict__ slot_at, int N, int S,
                                                   const Step step, double* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const long long m = clips[2LL * i + 1] / S;
  double* st = state + 4 * slot_at[i];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long k = 0; k < m; ++k) {
    double p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = k < m - 1 ? st[4 * k + r] : 0.0;
      st[4 * k + r] = s[r];
    }
    double t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      t[r] = fma(step.m[r][3], s[3], fma(step.m[r][2], s[2], fma(step.m[r][1], s[1], step.m[r][0] * s[0]))) + p[r];
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = t[r];
  }
}

// ---- blocks and gates ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct Gate {
  const long long* clips;
  const long long* slot_at;
  const double* e;
  const float* pk;
  double* lufs;
  float* peak;
  int* counts;
  int* valid;
  double* energy;
  const long long* energy_at;
  double abs_gate;
  int S;
};

__global__ void __launch_bounds__(64) gate_kernel(const Gate g) {
  const int clip = blockIdx.x, lane = threadIdx.x, S = g.S;
  const long long n = g.clips[2LL * clip + 1];
  const long long m = n / S, rows = m + (n > m * S ? 1 : 0);
  const long long slot0 = g.slot_at[clip];
  const double* __restrict__ e = g.e + slot0;
  float pk = 0.f;
  for (long long k = lane; k < rows; k += 64) pk = fmaxf(pk, g.pk[slot0 + k]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d, 64));
  if (g.energy) {
    double* out = g.energy + g.energy_at[clip];
    for (long long k = lane; k < m; k += 64) out[k] = e[k];
  }
  const long long nb = m >= 4 ? m - 3 : 0;
  const double div = 4.0 * (double)S;
  // lane l takes blocks l, l + 64, ... in ascending order, then one butterfly over the lanes: an order that depends only on m
  double sum = 0.0;
  int cnt = 0;
  for (long long b = lane; b < nb; b += 64) {
    const double z = (((e[b] + e[b + 1]) + e[b + 2]) + e[b + 3]) / div;
    if (z > g.abs_gate) { sum += z; ++cnt; }
  }
  const int n_abs = wave_sum(cnt);
  const double rel_gate = 0.1 * (wave_sum(sum) / (double)n_abs);                      // NaN without a block: every comparison fails
  sum = 0.0;
  cnt = 0;
  for (long long b = lane; b < nb; b += 64) {
    const double z = (((e[b] + e[b + 1]) + e[b + 2]) + e[b + 3]) / div;
    if (z > g.abs_gate && z > rel_gate) { sum += z; ++cnt; }
  }
  const int n_rel = wave_sum(cnt);
  const double mean = wave_sum(sum) / (double)n_rel;
  if (lane == 0) {
    const bool ok = n_abs > 0 && n_rel > 0;
    g.lufs[clip] = ok ? -0.691 + 10.0 * log10(mean) : -INFINITY;
    g.valid[clip] = ok ? 1 : 0;
    g.peak[clip] = pk;
    g.counts[3LL * clip] = (int)nb;
    g.counts[3LL * clip + 1] = n_abs;
    g.counts[3LL * clip + 2] = n_rel;
  }
}

// ---- the gain ---------------------------------------------------------------------------------------------------------------------------
// grid (tiles, clips): a workgroup scales kScaleTile samples of one clip and ends; 16-byte loads and stores from the first 16-byte
// boundary of the tile on, single floats in front of it and behind the last whole vector
__global__ void __launch_bounds__(kScaleThreads) scale_kernel(float* __restrict__ samples, const long long* __restrict__ clips,
                                                              const float* __restrict__ gain) {
  const int clip = blockIdx.y, tid = threadIdx.x;
  const long long n = clips[2LL * clip + 1];
  const long long t0 = (long long)blockIdx.x * kScaleTile;
  if (t0 >= n) return;
  const float g = gain[clip];
  float* __restrict__ x = samples + clips[2LL * clip] + t0;
  const int count = (int)(n - t0 < kScaleTile ? n - t0 : kScaleTile);
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2);
  if (head > count) head = count;
  const int nvec = (count - head) >> 2, tail0 = head + 4 * nvec;
  if (tid < head) x[tid] = x[tid] * g;
  for (int q = tid; q < nvec; q += kScaleThreads) {
    float4* p = reinterpret_cast<float4*>(x + head + 4 * q);
    float4 v = *p;
    v.x = v.x * g; v.y = v.y * g; v.z = v.z * g; v.w = v.w * g;
    *p = v;
  }
  if (tid < count - tail0) x[tail0 + tid] = x[tail0 + tid] * g;
}

// the clip table on the host: every clip inside [0, total], 0 <= n <= 2^30
int check_table(const char* what, const long long* clips_host, int N, long long total) {
  for (int i = 0; i < N; ++i) {
    const long long at = clips_host[2LL * i], n = clips_host[2LL * i + 1];
    VS_REQUIRE(n >= 0 && n <= kMaxClip, "%s: clip %d has %lld samples (0 .. 2^30)", what, i, n);
    VS_REQUIRE(at >= 0 && at <= total - n, "%s: clip %d = [%lld, + %lld) leaves the buffer of %lld samples", what, i, at, n, total);
  }
  return 0;
}

}  // namespace

int vs_loudness_plan(int sample_rate, vs_loudness_dims* dims) { return plan(sample_rate, dims); }

size_t vs_loudness_workspace_bytes(const vs_loudness_dims* dims, long long total, int N) {
  if (checked(dims, "loudness_workspace_bytes")) return 0;
  if (total < 0 || total > kMaxTotal || N <= 0) {
    vs_set_error("loudness_workspace_bytes: total=%lld (0 .. 2^48), N=%d (> 0)", total, N);
    return 0;
  }
  return layout(N, total / dims->sub + N).total;
}

int vs_loudness(const vs_loudness_dims* dims, const float* samples, long long total, const long long* clips_host, const long long* clips,
                int N, double* lufs, float* peak, int* counts, int* valid, double* energy, const long long* energy_at, void* workspace,
                size_t workspace_bytes, void* stream_) {
  if (int rc = checked(dims, "loudness")) return rc;
  VS_REQUIRE(N > 0, "loudness: N=%d clips", N);
  VS_REQUIRE(samples && clips_host && clips && lufs && peak && counts && valid && workspace, "loudness: NULL argument");
  VS_REQUIRE(!energy || energy_at, "loudness: energy without energy_at (NULL)");
  VS_REQUIRE(total >= 0 && total <= kMaxTotal, "loudness: a buffer of %lld samples (0 .. 2^48)", total);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "loudness: the workspace must be 256-byte aligned");
  if (int rc = check_table("loudness", clips_host, N, total)) return rc;
  const int S = dims->sub;
  long long slots = 0;
  for (int i = 0; i < N; ++i) slots += clips_host[2LL * i + 1] / S + 1;
  const Layout l = layout(N, slots);
  VS_REQUIRE(workspace_bytes >= l.total, "loudness: workspace too small: %zu bytes, these %d clips need %zu", workspace_bytes, N, l.total);
  hipStream_t stream = (hipStream_t)stream_;
  long long* slot_at = at<long long>(workspace, l.slot_at);
  Job j = {};
  j.samples = samples;
  j.state = at<double>(workspace, l.state);
  j.energy = at<double>(workspace, l.energy);
  j.peak = at<float>(workspace, l.peak);
  j.f = {dims->b1[0], dims->b1[1], dims->b1[2], dims->a1[0], dims->a1[1], dims->a2[0], dims->a2[1]};
  j.S = S;
  Step step;
  memcpy(step.m, dims->step, sizeof(step.m));

  hipLaunchKernelGGL(slots_kernel, dim3(1), dim3(kSlotThreads), 0, stream, clips, N, S, slot_at);
  VS_LAUNCH_CHECK();
  for (int pass = 0; pass < 2; ++pass) {
    for (int first = 0; first < N; first += 65535) {
      const int rows = N - first < 65535 ? N - first : 65535;
      long long longest = 0;                                                         // sub-block rows of the longest clip of this launch
      for (int i = first; i < first + rows; ++i) {
        const long long n = clips_host[2LL * i + 1], m = n / S;
        const long long r = pass ? m + (n > m * S ? 1 : 0) : m - 1;
        if (r > longest) longest = r;
      }
      if (longest <= 0) continue;
      j.clips = clips + 2LL * first;
      j.slot_at = slot_at + first;
      const dim3 grid((unsigned)((longest + kRows - 1) / kRows), (unsigned)rows);
      if (pass) hipLaunchKernelGGL(sweep_kernel<true>, grid, dim3(kRows), 0, stream, j);
      else hipLaunchKernelGGL(sweep_kernel<false>, grid, dim3(kRows), 0, stream, j);
      VS_LAUNCH_CHECK();
    }
    if (pass == 0) {
      hipLaunchKernelGGL(scan_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, clips, slot_at, N, S, step, j.state);
      VS_LAUNCH_CHECK();
    }
  }
  Gate g = {};
  g.clips = clips; g.slot_at = slot_at; g.e = j.energy; g.pk = j.peak;
  g.lufs = lufs; g.peak = peak; g.counts = counts; g.valid = valid;
  g.energy = energy; g.energy_at = energy_at;
  g.abs_gate = pow(10.0, (-70.0 + 0.691) / 10.0);
  g.S = S;
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)N), dim3(64), 0, stream, g);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_scale_clips(float* samples, long long total, const long long* clips_host, const long long* clips, const float* gain, int N,
                   void* stream_) {
  VS_REQUIRE(N > 0, "scale_clips: N=%d clips", N);
  VS_REQUIRE(samples && clips_host && clips && gain, "scale_clips: NULL argument");
  VS_REQUIRE(total >= 0 && total <= kMaxTotal, "scale_clips: a buffer of %lld samples (0 .. 2^48)", total);
  if (int rc = check_table("scale_clips", clips_host, N, total)) return rc;
  for (int first = 0; first < N; first += 65535) {
    const int rows = N - first < 65535 ? N - first : 65535;
    long long longest = 0;
    for (int i = first; i < first + rows; ++i)
      if (clips_host[2LL * i + 1] > longest) longest = clips_host[2LL * i + 1];
    if (longest == 0) continue;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((longest + kScaleTile - 1) / kScaleTile), (unsigned)rows), dim3(kScaleThreads), 0,
                       (hipStream_t)stream_, samples, clips + 2LL * first, gain + first);
    VS_LAUNCH_CHECK();
  }
  return 0;
}
