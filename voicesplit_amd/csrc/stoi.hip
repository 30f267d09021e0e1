// Speech intelligibility on the device: STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of R (reference, estimate) pairs of
// unequal length in two flat 10 kHz buffers that share one clip table.  The definition (window, silent-frame removal by the
// reference's frame energies, one-third-octave band envelopes, 30-frame segments, the two correlation forms) is the text in
// include/voicesplit_hip.h: pystoi's algorithm AS REMEMBERED, restated, not compared with a pystoi run.
//
//   slots_kernel    exclusive prefix sum of the clips' frame counts F: where each clip's frames live in the workspace
//   energy_kernel   one wave per frame of x: e_f = 20 log10(sqrt(sum (w x_f)^2) + EPS), lane l sums samples l, l + 64, l + 128, l + 192 in
//                   that order, then one butterfly over the lanes
//   gate_kernel     one workgroup per clip: max_f e (exact in any order), the keep mask, its exclusive scan (wave ballots, chunks of 256
//                   frames in ascending order) into the list src(q) of kept source frames; writes (F, Mk) and status
//   band_kernel     one workgroup per (clip, signal, 8 kept frames): the frames of the REBUILT signal are formed in LDS straight from the
//                   source (the rebuilt signal is never stored: sample 128 q + r is w[r + 128] s[128 src(q - 1) + 128 + r] +
//                   w[r] s[128 src(q) + r], one term in the first and the last half frame), windowed again, and thread k - 7 takes the
//                   512-point DFT bin k = 7 .. 218 of all 8 frames over the 256 non-zero samples in ascending order; then thread (g, j)
//                   sums |.|^2 over band j's bins in ascending order and stores the square root
//   corr_kernel     one wave per segment m = 30 .. Mk (four per workgroup): the 15 x 30 block is recomputed from the envelopes -- no
//                   running sums -- and the segment's sum goes to partial[m - 30]
//   fold_kernel     one wave per clip: lane l adds partial[l], partial[l + 64], .. in ascending order, one butterfly; d = sum / (J M) or
//                   sum / (N M), or 1e-5 exactly with status 1
//
// At most six launches on the stream for any R (a launch without work for the table is left out).  Arithmetic: plain fp64 FMAs on the vector pipe.  The DFT is 256 x 212 complex multiply-adds per
// frame, 3.2 G FMAs for 64 clips of 3 s: a tenth of a millisecond at the vector fp64 peak, which as published for this part equals the
// fp64 matrix peak -- the matrix instruction would save LDS reads, not arithmetic, and its 16 x 16 x 4 blocking would fix a summation
// order over groups of four samples for no gain in time that matters beside the launches.  The twiddles exp(-2 pi i t / 512) are one 512-entry
// table of (cos, sin) pairs in LDS built with sincospi; thread k reads entry (k i) mod 512 with one 16-byte read: stride k entries
// across the lanes, conflict-free for odd i and 2^a-way for i = 2^a * odd (2.9-way on average), while the 8 frame samples of a step
// are one broadcast of 64 contiguous bytes.  KNOWN, NOT TUNED: the last wave of band_kernel has 20 of 64 lanes busy; grids are sized by
// the longest clip's F, not by Mk.
//
// Every result of a clip is a function of the clip's samples alone: each chain above runs in an order fixed by F, Mk and m, and nothing
// outside [at, at + n) is read.  Offsets, neighbours, R and the call do not show in a bit.
#include <math.h>
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

namespace {

constexpr int kW = 256, kHop = 128, kNfft = 512, kBands = 15, kSeg = 30;
constexpr int kBin0 = 7, kBins = 212;                     // bins 7 .. 218
constexpr long long kMaxClip = 1LL << 24;
constexpr long long kMaxTotal = 1LL << 48;
constexpr int kSlotThreads = 1024;
constexpr int kEnergyFrames = 32;                         // frames of one energy workgroup (4 waves, 8 frames each)
constexpr int kG = 8;                                     // frames of one band workgroup
constexpr int kSegWaves = 4;                              // segments of one corr workgroup
#define VS_STOI_EPS 2.220446049250313e-16                 /* 2^-52 */

__host__ __device__ inline long long frames_of(long long n) { return n >= kW ? (n - kW) / kHop + 1 : 0; }

// ---- the plan (host only) ----------------------------------------------------------------------------------------------------------
int plan(vs_stoi_dims* d) {
  VS_REQUIRE(d, "stoi_plan: NULL dims");
  memset(d, 0, sizeof(*d));
  d->frame = kW; d->hop = kHop; d->nfft = kNfft; d->bands = kBands; d->seg = kSeg;
  d->clip = 1.0 + pow(10.0, 15.0 / 20.0);
  d->dyn_db = 40.0;
  auto nearest = [](double f) {                             // the first bin of the 10000 / 512 Hz grid nearest to f
    int best = 0;
    double bd = INFINITY;
    for (int k = 0; k <= kNfft / 2; ++k) {
      const double t = (double)k * 10000.0 / (double)kNfft - f, dd = t * t;
      if (dd < bd) { bd = dd; best = k; }
    }
    return best;
  };
  for (int j = 0; j < kBands; ++j) {
    d->lo[j] = nearest(150.0 * pow(2.0, (2.0 * j - 1.0) / 6.0));
    d->hi[j] = nearest(150.0 * pow(2.0, (2.0 * j + 1.0) / 6.0));
  }
  return 0;
}

int checked(const vs_stoi_dims* dims, const char* what) {
  VS_REQUIRE(dims, "%s: NULL dims", what);
  vs_stoi_dims own;
  if (int rc = plan(&own)) return rc;
  VS_REQUIRE(memcmp(&own, dims, sizeof(own)) == 0, "%s: dims are not what vs_stoi_plan returns", what);
  VS_REQUIRE(own.lo[0] == kBin0 && own.hi[kBands - 1] == kBin0 + kBins, "%s: the band edges left bins %d .. %d", what, kBin0, kBin0 + kBins - 1);
  return 0;
}

// workspace: frame_at [R + 1] int64 | e [slots] fp64 | src [slots] int32 | env [slots][2][15] fp64 (per clip [2][15][Mk]) | partial
// [slots] fp64, every piece 256-byte aligned; slots = the clips' frame counts summed
struct Layout { size_t frame_at, e, src, env, partial, total; };
inline Layout layout(long long R, long long slots) {
  Layout l;
  l.frame_at = 0;
  l.e = align_up((size_t)(R + 1) * 8);
  l.src = l.e + align_up((size_t)slots * 8);
  l.env = l.src + align_up((size_t)slots * 4);
  l.partial = l.env + align_up((size_t)slots * 2 * kBands * 8);
  l.total = l.partial + align_up((size_t)slots * 8);
  return l;
}

struct Bands { int lo[kBands], hi[kBands]; };

struct Job {
  const float* sig[2];                                    // reference, estimate
  const long long* clips;                                 // [R][2] = (at, n), device
  const long long* frame_at;
  double* e;
  int* src;
  double* env;
  double* partial;
  double* d;
  int* frames;                                            // [R][2] = (F, Mk)
  int* status;
  double* tob;
  const long long* tob_at;
  Bands bands;
  double clip;
};

__device__ __forceinline__ double window(int i) { return 0.5 - 0.5 * cospi(2.0 * (double)(i + 1) / 257.0); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ---- where each clip's frames live -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSlotThreads) slots_kernel(const long long* __restrict__ clips, int R, long long* __restrict__ frame_at) {
  __shared__ long long part[kSlotThreads];
  const int tid = threadIdx.x;
  const int per = (R + kSlotThreads - 1) / kSlotThreads;
  const int lo = (long long)tid * per < R ? tid * per : R, hi = lo + per < R ? lo + per : R;
  long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += frames_of(clips[2LL * i + 1]);
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
    frame_at[i] = run;
    run += frames_of(clips[2LL * i + 1]);
  }
  if (tid == kSlotThreads - 1) frame_at[R] = part[tid];
}

// ---- (a) gate and compaction ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) energy_kernel(const Job j) {
  const int clip = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long at = j.clips[2LL * clip], F = frames_of(j.clips[2LL * clip + 1]);
  const long long f0 = (long long)blockIdx.y * kEnergyFrames;
  if (f0 >= F) return;                                                               // (uniform)
  double w[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) w[c] = window(lane + 64 * c);
  const float* __restrict__ x = j.sig[0] + at;
  double* __restrict__ e = j.e + j.frame_at[clip];
  for (long long f = f0 + wave; f < F && f < f0 + kEnergyFrames; f += 4) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double v = w[c] * (double)x[f * kHop + lane + 64 * c];
      acc += v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) e[f] = 20.0 * log10(sqrt(acc) + VS_STOI_EPS);
  }
}

__global__ void __launch_bounds__(256) gate_kernel(const Job j, double dyn_db) {
  __shared__ double smax[4];
  __shared__ int scount[4];
  const int clip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long F = frames_of(j.clips[2LL * clip + 1]);
  const long long base = j.frame_at[clip];
  const double* __restrict__ e = j.e + base;
  double mx = -INFINITY;
  for (long long f = tid; f < F; f += 256) mx = fmax(mx, e[f]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
  if (lane == 0) smax[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
  const double thr = mx - dyn_db;
  long long run = 0;
  for (long long f0 = 0; f0 < F; f0 += 256) {
    const long long f = f0 + tid;
    const bool keep = f < F && thr - e[f] < 0.0;
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ULL << lane) - 1ULL));
    __syncthreads();                                                                 // the previous chunk's counts have been read
    if (lane == 0) scount[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, all = 0;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {
      if (wv < wave) off += scount[wv];
      all += scount[wv];
    }
    if (keep) j.src[base + run + off + before] = (int)f;
    run += all;
  }
  if (tid == 0) {
    j.frames[2LL * clip] = (int)F;
    j.frames[2LL * clip + 1] = (int)run;
    j.status[clip] = run < kSeg ? 1 : 0;
  }
}

// ---- (b) band envelopes ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) band_kernel(const Job j) {
  __shared__ double2 tw[kNfft];                                                      // (cos, sin)(2 pi t / 512)
  __shared__ double v[kW * kG];                                                      // [sample][frame]; afterwards the powers [frame][bin]
  const int clip = blockIdx.x, sig = blockIdx.z, tid = threadIdx.x;
  const int Mk = j.frames[2LL * clip + 1];
  const int q0 = blockIdx.y * kG;
  if (q0 >= Mk) return;                                                              // (uniform)
  for (int t = tid; t < kNfft; t += 256) {
    double s, c;
    sincospi((double)t / 256.0, &s, &c);
    tw[t] = make_double2(c, s);
  }
  const long long base = j.frame_at[clip];
  const int* __restrict__ src = j.src + base;
  const float* __restrict__ s = j.sig[sig] + j.clips[2LL * clip];
  {
    const int r = tid & (kHop - 1);
    const double w_lo = window(r), w_hi = window(r + kHop), w_own = tid < kHop ? w_lo : w_hi;
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int q = q0 + g;
      double val = 0.0;
      if (q < Mk) {
        if (tid < kHop) {                                                            // rebuilt sample 128 q + r: the tail of q - 1, then the head of q
          const double cur = w_lo * (double)s[(long long)kHop * src[q] + r];
          val = q > 0 ? w_hi * (double)s[(long long)kHop * src[q - 1] + kHop + r] + cur : cur;
        } else {                                                                     // rebuilt sample 128 (q + 1) + r: the tail of q, then the head of q + 1
          const double cur = w_hi * (double)s[(long long)kHop * src[q] + kHop + r];
          val = q + 1 < Mk ? cur + w_lo * (double)s[(long long)kHop * src[q + 1] + r] : cur;
        }
      }
      v[tid * kG + g] = w_own * val;
    }
  }
  __syncthreads();
  double re[kG], im[kG];
#pragma unroll
  for (int g = 0; g < kG; ++g) re[g] = im[g] = 0.0;
  if (tid < kBins) {
    const int k = kBin0 + tid;
    int idx = 0;
#pragma unroll 4
    for (int i = 0; i < kW; ++i) {
      const double2 t = tw[idx];
      const double* __restrict__ row = v + i * kG;
#pragma unroll
      for (int g = 0; g < kG; ++g) {
        re[g] = fma(row[g], t.x, re[g]);
        im[g] = fma(row[g], t.y, im[g]);
      }
      idx = (idx + k) & (kNfft - 1);
    }
  }
  __syncthreads();
  if (tid < kBins) {
#pragma unroll
    for (int g = 0; g < kG; ++g) v[g * kBins + tid] = re[g] * re[g] + im[g] * im[g];
  }
  __syncthreads();
  if (tid < kG * kBands) {
    const int g = tid / kBands, b = tid - g * kBands, q = q0 + g;
    if (q < Mk) {
      double sum = 0.0;
      for (int k = j.bands.lo[b]; k < j.bands.hi[b]; ++k) sum += v[g * kBins + k - kBin0];
      const double env = sqrt(sum);
      j.env[2LL * kBands * base + (long long)(sig * kBands + b) * Mk + q] = env;
      if (j.tob) j.tob[j.tob_at[clip] + (long long)(sig * kBands + b) * Mk + q] = env;
    }
  }
}

// ---- (c) correlation -------------------------------------------------------------------------------------------------------------------
template <bool EXT>
__global__ void __launch_bounds__(64 * kSegWaves) corr_kernel(const Job j) {
  __shared__ double xs[kSegWaves][kBands * kSeg], ys[kSegWaves][kBands * kSeg];
  __shared__ double dots[kSegWaves][32];
  const int clip = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Mk = j.frames[2LL * clip + 1];
  const int M = Mk - kSeg + 1;
  if ((int)blockIdx.y * kSegWaves >= M) return;                                      // (uniform)
  const int seg = blockIdx.y * kSegWaves + wave;                                     // the block X[:, seg : seg + 30]
  const bool live = seg < M;
  const long long base = j.frame_at[clip];
  const double* __restrict__ X = j.env + 2LL * kBands * base + seg;
  const double* __restrict__ Y = X + (long long)kBands * Mk;
  double* xw = xs[wave];
  double* yw = ys[wave];
  if (live && lane < kBands) {                                                       // one band row per lane, every sum in ascending n
    const double* __restrict__ x = X + (long long)lane * Mk;
    const double* __restrict__ y = Y + (long long)lane * Mk;
    double xr[kSeg], yr[kSeg];
#pragma unroll
    for (int n = 0; n < kSeg; ++n) { xr[n] = x[n]; yr[n] = y[n]; }
    if (!EXT) {
      double sx = 0.0, sy = 0.0;
#pragma unroll
      for (int n = 0; n < kSeg; ++n) { sx += xr[n] * xr[n]; sy += yr[n] * yr[n]; }
      const double c = sqrt(sx) / (sqrt(sy) + VS_STOI_EPS);
#pragma unroll
      for (int n = 0; n < kSeg; ++n) yr[n] = fmin(c * yr[n], xr[n] * j.clip);
    }
    double mx = 0.0, my = 0.0;
#pragma unroll
    for (int n = 0; n < kSeg; ++n) { mx += xr[n]; my += yr[n]; }
    mx /= (double)kSeg; my /= (double)kSeg;
    double nx = 0.0, ny = 0.0;
#pragma unroll
    for (int n = 0; n < kSeg; ++n) {
      xr[n] -= mx; yr[n] -= my;
      nx += xr[n] * xr[n]; ny += yr[n] * yr[n];
    }
    nx = sqrt(nx) + VS_STOI_EPS; ny = sqrt(ny) + VS_STOI_EPS;
    if (EXT) {
#pragma unroll
      for (int n = 0; n < kSeg; ++n) { xw[lane * kSeg + n] = xr[n] / nx; yw[lane * kSeg + n] = yr[n] / ny; }
    } else {
      double dot = 0.0;
#pragma unroll
      for (int n = 0; n < kSeg; ++n) dot += (xr[n] / nx) * (yr[n] / ny);
      dots[wave][lane] = dot;
    }
  }
  __syncthreads();
  if (EXT) {
    if (live && lane < kSeg) {                                                       // one column per lane, every sum in ascending band
      double xc[kBands], yc[kBands];
      double mx = 0.0, my = 0.0;
#pragma unroll
      for (int b = 0; b < kBands; ++b) { xc[b] = xw[b * kSeg + lane]; yc[b] = yw[b * kSeg + lane]; mx += xc[b]; my += yc[b]; }
      mx /= (double)kBands; my /= (double)kBands;
      double nx = 0.0, ny = 0.0;
#pragma unroll
      for (int b = 0; b < kBands; ++b) {
        xc[b] -= mx; yc[b] -= my;
        nx += xc[b] * xc[b]; ny += yc[b] * yc[b];
      }
      nx = sqrt(nx) + VS_STOI_EPS; ny = sqrt(ny) + VS_STOI_EPS;
      double dot = 0.0;
#pragma unroll
      for (int b = 0; b < kBands; ++b) dot += (xc[b] / nx) * (yc[b] / ny);
      dots[wave][lane] = dot;
    }
    __syncthreads();
  }
  if (live && lane == 0) {
    double sum = 0.0;
    for (int i = 0; i < (EXT ? kSeg : kBands); ++i) sum += dots[wave][i];
    j.partial[base + seg] = sum;
  }
}

__global__ void __launch_bounds__(64) fold_kernel(const Job j, int extended) {
  const int clip = blockIdx.x, lane = threadIdx.x;
  const int Mk = j.frames[2LL * clip + 1];
  const int M = Mk - kSeg + 1;
  if (M <= 0) {
    if (lane == 0) j.d[clip] = 1e-5;
    return;
  }
  const double* __restrict__ p = j.partial + j.frame_at[clip];
  double sum = 0.0;
  for (int m = lane; m < M; m += 64) sum += p[m];
  sum = wave_sum(sum);
  if (lane == 0) j.d[clip] = sum / ((double)(extended ? kSeg : kBands) * (double)M);
}

}  // namespace

int vs_stoi_plan(vs_stoi_dims* dims) { return plan(dims); }

size_t vs_stoi_workspace_bytes(const vs_stoi_dims* dims, long long total, int R) {
  if (checked(dims, "stoi_workspace_bytes")) return 0;
  if (total < 0 || total > kMaxTotal || R <= 0) {
    vs_set_error("stoi_workspace_bytes: total=%lld (0 .. 2^48), R=%d (> 0)", total, R);
    return 0;
  }
  return layout(R, total / kHop + 1).total;
}

int vs_stoi(const vs_stoi_dims* dims, const float* ref, const float* est, long long total, const long long* clips_host,
            const long long* clips, int R, int extended, double* d, int* frames, int* status, double* tob, const long long* tob_at,
            void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = checked(dims, "stoi")) return rc;
  VS_REQUIRE(R > 0, "stoi: R=%d clips", R);
  VS_REQUIRE(ref && est && clips_host && clips && d && frames && status && workspace, "stoi: NULL argument");
  VS_REQUIRE(!tob || tob_at, "stoi: tob without tob_at (NULL)");
  VS_REQUIRE(extended == 0 || extended == 1, "stoi: extended=%d (0 or 1)", extended);
  VS_REQUIRE(total >= 0 && total <= kMaxTotal, "stoi: buffers of %lld samples (0 .. 2^48)", total);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "stoi: the workspace must be 256-byte aligned");
  long long slots = 0, longest = 0;
  for (int i = 0; i < R; ++i) {
    const long long at = clips_host[2LL * i], n = clips_host[2LL * i + 1];
    VS_REQUIRE(n >= 0 && n <= kMaxClip, "stoi: clip %d has %lld samples (0 .. 2^24)", i, n);
    VS_REQUIRE(at >= 0 && at <= total - n, "stoi: clip %d = [%lld, + %lld) leaves the buffers of %lld samples", i, at, n, total);
    const long long F = frames_of(n);
    slots += F;
    if (F > longest) longest = F;
  }
  const Layout l = layout(R, slots);
  VS_REQUIRE(workspace_bytes >= l.total, "stoi: workspace too small: %zu bytes, these %d clips need %zu", workspace_bytes, R, l.total);
  hipStream_t stream = (hipStream_t)stream_;
  Job j = {};
  j.sig[0] = ref; j.sig[1] = est;
  j.clips = clips;
  j.frame_at = at<long long>(workspace, l.frame_at);
  j.e = at<double>(workspace, l.e);
  j.src = at<int>(workspace, l.src);
  j.env = at<double>(workspace, l.env);
  j.partial = at<double>(workspace, l.partial);
  j.d = d; j.frames = frames; j.status = status;
  j.tob = tob; j.tob_at = tob_at;
  memcpy(j.bands.lo, dims->lo, sizeof(j.bands.lo));
  memcpy(j.bands.hi, dims->hi, sizeof(j.bands.hi));
  j.clip = dims->clip;

  hipLaunchKernelGGL(slots_kernel, dim3(1), dim3(kSlotThreads), 0, stream, clips, R, at<long long>(workspace, l.frame_at));
  VS_LAUNCH_CHECK();
  if (longest > 0) {
    hipLaunchKernelGGL(energy_kernel, dim3((unsigned)R, (unsigned)((longest + kEnergyFrames - 1) / kEnergyFrames)), dim3(256), 0, stream, j);
    VS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)R), dim3(256), 0, stream, j, dims->dyn_db);
  VS_LAUNCH_CHECK();
  if (longest > 0) {
    hipLaunchKernelGGL(band_kernel, dim3((unsigned)R, (unsigned)((longest + kG - 1) / kG), 2), dim3(256), 0, stream, j);
    VS_LAUNCH_CHECK();
  }
  const long long segs = longest - kSeg + 1;
  if (segs > 0) {
    const dim3 grid((unsigned)R, (unsigned)((segs + kSegWaves - 1) / kSegWaves));
    if (extended) hipLaunchKernelGGL(corr_kernel<true>, grid, dim3(64 * kSegWaves), 0, stream, j);
    else hipLaunchKernelGGL(corr_kernel<false>, grid, dim3(64 * kSegWaves), 0, stream, j);
    VS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fold_kernel, dim3((unsigned)R), dim3(64), 0, stream, j, extended);
  VS_LAUNCH_CHECK();
  return 0;
}
