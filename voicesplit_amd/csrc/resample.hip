// Sample-rate conversion on the device: librosa.load(path, sr=...) of mix_wavfiles (utils/generic_utils.py:300-345) and of both audio
// processors' load_wav, as a polyphase Kaiser-windowed sinc.  The definition (rates -> L, M, H, T, the taps, n_out, y[n]) is the text
// in include/voicesplit_hip.h; it restates resampy's kaiser_best from memory and was not compared with a resampy or librosa run.
//
//   bank_kernel            one thread per tap, fp64 (sin, the I0 power series), one rounding to fp32.  Once per pair of rates.
//   resample_tile_kernel   ONE sweep of short-lived workgroups, grid (tiles, rows or clips).  A workgroup owns P whole
//                          periods of one row (a period = L consecutive outputs, which consume M inputs):
//     1. the input span of the tile, P M + T - 1 floats, goes to LDS once, zero where the stream has no sample (in front of sample 0,
//        behind stream_len, outside a clip) -- the only reads of x, all inside the caller's buffer;
//     2. lanes map to PERIODS and a wave takes one place q in the period at a time (units of 64 periods x 1 place, dealt round-robin
//        to the four waves).  The place fixes the phase r = (q M) mod L, so the T taps of bank row r are wave-uniform (scalar loads
//        of one contiguous row) and each lane runs the fmaf chain of its own output over LDS at lane stride M.  Lanes mapped to
//        consecutive n would gather from 64 different bank rows per tap;
//     3. the P L outputs are staged in LDS (index p L + q) and stored in order, 16 bytes per lane from the first 16-byte boundary of
//        the row on.
//     LDS at lane stride M: ds_read_b32 has 32 banks per half wave, so an odd M is conflict-free and M = 160 (48000 -> 44100) would
//     put a half wave on one bank.  For even M the staging index is skewed, i -> i + (i >> ctz(M)): the lane stride becomes
//     (M >> e)(2^e + 1), odd.  Two more integer instructions per tap, only in the instance for even M.
//     P is the largest number of periods (at most 1024, a multiple of 64 above 64) whose input span and outputs fit 72 KiB: two
//     workgroups per CU.  44100 -> 16000 (M = 441, L = 160) gets P = 30: less than half a wave works per unit; known, not tuned.
//   resample_direct_kernel a thread per output straight from global memory, for the pairs of rates whose tile would hold fewer than 8
//                          periods (M + L above about 2000).  The same chain, hence the same bits.
// Every output is fmaf(tap[T-1], x[b+H], ... fmaf(tap[0], x[b-H], +0)): multiplying by a staged zero and skipping a sample that does
// not exist give the same bits (+0 + -0 = +0 and a chain that starts at +0 never reaches -0), so neither the tile, the kernel, the
// window [y_first, y_first + y_count) nor the buffer [x_first, x_first + x_count) shows in a result.
#include <math.h>
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

namespace {

constexpr int kZ = 64;                                  // zero crossings on each side at the lower of the two rates
constexpr double kBeta = 14.769656459379492, kRho = 0.9475937167399596;
constexpr long long kMaxBankBytes = 4LL << 20;
constexpr int kThreads = 256;
constexpr int kLdsFloats = 18432;                       // 72 KiB: two workgroups per CU (160 KiB)
constexpr int kMaxTilePeriods = 1024, kMinTilePeriods = 8;
constexpr long long kMaxPos = 1LL << 48;                // stream positions: n M and n_in L stay inside 64 bits (L, M < 2^14)

__host__ __device__ inline int skewed(int i, int sh) { return i + (i >> sh); }
inline int skew_shift(int M) { return (M & 1) ? 0 : __builtin_ctz((unsigned)M); }       // 0: no skew
// floats of LDS for the input span of P periods, rounded to 16 bytes (the outputs are staged behind it)
inline long long span_floats(long long P, int M, int T, int sh) {
  const long long last = P * M + T - 2;
  return ((sh ? last + (last >> sh) : last) + 1 + 3) & ~3LL;
}

int plan(int sr_in, int sr_out, vs_resample_dims* d) {
  VS_REQUIRE(d, "resample_plan: NULL dims");
  VS_REQUIRE(sr_in > 0 && sr_out > 0, "resample_plan: rates %d -> %d must be positive", sr_in, sr_out);
  int a = sr_in, b = sr_out;
  while (b) { const int t = a % b; a = b; b = t; }
  const int L = sr_out / a, M = sr_in / a;
  long long H = 0;
  if (L != 1 || M != 1) H = L >= M ? kZ : ((long long)kZ * M + L - 1) / L;       // ceil(Z / s), s = min(1, L / M)
  const long long T = 2 * H + 1;
  VS_REQUIRE(T * 4 <= kMaxBankBytes && (long long)L * T * 4 <= kMaxBankBytes,
             "resample_plan: %d -> %d needs a bank of L = %d rows of T = %lld taps, more than %lld bytes: refused", sr_in, sr_out, L, T,
             kMaxBankBytes);
  const int sh = skew_shift(M);
  int P = kMaxTilePeriods;
  while (P > 0 && span_floats(P, M, (int)T, sh) + (long long)P * L > kLdsFloats) --P;
  if (P > 64) P &= ~63;
  if (P < kMinTilePeriods) P = 0;
  memset(d, 0, sizeof(*d));
  d->sr_in = sr_in; d->sr_out = sr_out;
  d->L = L; d->M = M; d->H = (int)H; d->T = (int)T;
  d->tile_periods = P;
  d->lds_bytes = P ? (int)((span_floats(P, M, (int)T, sh) + (long long)P * L) * 4) : 0;
  d->bank_bytes = (size_t)L * (size_t)T * 4;
  return 0;
}

// the caller's dims against a plan of our own: the launch geometry and the LDS carve never come from unchecked numbers
int checked(const vs_resample_dims* dims, const char* what) {
  VS_REQUIRE(dims, "%s: NULL dims", what);
  vs_resample_dims own;
  if (int rc = plan(dims->sr_in, dims->sr_out, &own)) return rc;
  VS_REQUIRE(memcmp(&own, dims, sizeof(own)) == 0, "%s: dims are not what vs_resample_plan(%d, %d) returns", what, dims->sr_in, dims->sr_out);
  return 0;
}

inline long long out_len(int L, int M, long long n_in) { return (n_in * L + M - 1) / M; }

// ---- the bank -----------------------------------------------------------------------------------------------------------------
__device__ double bessel_i0(double x) {                  // sum_k ((x / 2)^k / k!)^2; x <= beta: about 40 terms
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

__global__ void __launch_bounds__(kThreads) bank_kernel(float* __restrict__ bank, int L, int M, int H, int T) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (long long)L * T) return;
  if (H == 0) {                                          // equal rates: a copy
    bank[idx] = 1.f;
    return;
  }
  const int r = (int)(idx / T), j = (int)(idx - (long long)r * T) - H;
  const double s = L < M ? (double)L / (double)M : 1.0;
  const double t = s * ((double)r / (double)L - (double)j);
  double h = 0.0;
  if (fabs(t) < (double)kZ) {
    const double a = kRho * t, u = t / (double)kZ;
    const double sinc = a == 0.0 ? 1.0 : sin(M_PI * a) / (M_PI * a);
    h = kRho * sinc * bessel_i0(kBeta * sqrt(1.0 - u * u)) / bessel_i0(kBeta);
  }
  bank[idx] = (float)(s * h);
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------------
struct Job {
  const float* bank;
  const float* x;
  float* y;
  const long long* clips;                                // not NULL: clip form, [rows][3] = {first input, n_in, first output}
  long long x_first, x_count, x_stride, stream_len, y_first, y_count, y_stride;
  int L, M, H, T, P, sh, span_floats;
};

struct Row {
  const float* x;                                        // x[k - x_first] = stream sample k for lo <= k < hi; zero elsewhere
  float* y;                                              // y[n - y_first]
  long long x_first, lo, hi, y_first, y_count;
};

__device__ __forceinline__ Row resolve(const Job& j, int row) {
  Row r;
  if (j.clips) {
    const long long* c = j.clips + 3LL * row;
    r.x = j.x + c[0];
    r.x_first = 0; r.lo = 0; r.hi = c[1];
    r.y = j.y + c[2];
    r.y_first = 0; r.y_count = (c[1] * j.L + j.M - 1) / j.M;
  } else {
    r.x = j.x + (long long)row * j.x_stride;
    r.x_first = j.x_first;
    r.lo = j.x_first > 0 ? j.x_first : 0;
    r.hi = j.x_first + j.x_count;
    if (j.stream_len >= 0 && j.stream_len < r.hi) r.hi = j.stream_len;
    r.y = j.y + (long long)row * j.y_stride;
    r.y_first = j.y_first; r.y_count = j.y_count;
  }
  return r;
}

template <bool SKEW>
__global__ void __launch_bounds__(kThreads) resample_tile_kernel(const Job j) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* __restrict__ sx = smem;
  float* __restrict__ sy = smem + j.span_floats;
  const Row r = resolve(j, blockIdx.y);
  if (r.y_count <= 0) return;
  const int L = j.L, M = j.M, T = j.T, P = j.P, sh = j.sh, tid = threadIdx.x;
  const long long p0 = r.y_first / L + (long long)blockIdx.x * P;                  // the tile's first period
  const long long n0 = p0 * L;
  const long long n_begin = r.y_first > n0 ? r.y_first : n0;
  long long n_end = r.y_first + r.y_count;
  if (n_end > n0 + (long long)P * L) n_end = n0 + (long long)P * L;
  if (n_begin >= n_end) return;                                                    // (uniform) a shorter row or clip
  const int np = (int)((n_end - n0 + L - 1) / L);                                  // periods of this tile with an output, <= P

  // 1. stream samples [k0, k0 + span) -> sx
  const long long k0 = p0 * M - j.H;
  const int span = np * M + T - 1;
  for (int i = tid; i < span; i += kThreads) {
    const long long k = k0 + i;
    const float v = (k >= r.lo && k < r.hi) ? r.x[k - r.x_first] : 0.f;
    sx[SKEW ? skewed(i, sh) : i] = v;
  }
  __syncthreads();

  // 2. units of (64 periods, one phase)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int units = ((np + 63) >> 6) * L;
  for (int u = wave; u < units; u += kThreads / 64) {
    const int g = u / L, ph = u - g * L;
    const unsigned pm = (unsigned)ph * (unsigned)M;                                // < 2^27: n M of output n = p L + ph, less p L M
    const int off = (int)(pm / (unsigned)L);                                       // its b, less p M
    const float* __restrict__ taps = j.bank + (size_t)(pm - (unsigned)off * (unsigned)L) * T;     // bank row r = (n M) mod L
    const int p = g * 64 + lane;
    if (p < np) {
      const int base = p * M + off;                                                // sample b - H of this output, as an index of the span
      float acc = 0.f;
#pragma unroll 16
      for (int jj = 0; jj < T; ++jj) {
        const int i = base + jj;
        acc = fmaf(taps[jj], sx[SKEW ? skewed(i, sh) : i], acc);
      }
      sy[p * L + ph] = acc;
    }
  }
  __syncthreads();

  // 3. outputs [n_begin, n_end) in order
  const float* __restrict__ src = sy + (n_begin - n0);
  float* __restrict__ dst = r.y + (n_begin - r.y_first);
  const int count = (int)(n_end - n_begin);
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 2);     // floats in front of the first 16-byte boundary
  if (head > count) head = count;
  const int nvec = (count - head) >> 2, tail0 = head + 4 * nvec;
  if (tid < head) dst[tid] = src[tid];
  for (int q = tid; q < nvec; q += kThreads) {
    const float* s4 = src + head + 4 * q;
    *reinterpret_cast<float4*>(dst + head + 4 * q) = make_float4(s4[0], s4[1], s4[2], s4[3]);
  }
  if (tid < count - tail0) dst[tail0 + tid] = src[tail0 + tid];
}

__global__ void __launch_bounds__(kThreads) resample_direct_kernel(const Job j) {
  const Row r = resolve(j, blockIdx.y);
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= r.y_count) return;
  const long long nm = (r.y_first + idx) * j.M;
  const long long b = nm / j.L;
  const float* __restrict__ taps = j.bank + (size_t)(nm - b * j.L) * j.T;
  const long long k = b - j.H;
  float acc = 0.f;
  for (int jj = 0; jj < j.T; ++jj) {
    const long long kk = k + jj;
    const float v = (kk >= r.lo && kk < r.hi) ? r.x[kk - r.x_first] : 0.f;
    acc = fmaf(taps[jj], v, acc);
  }
  r.y[idx] = acc;
}

// rows: grid.y; max_outputs / first_output: of the longest row (rows of the clip form start at output 0)
int launch(const vs_resample_dims* d, Job j, long long first_output, long long max_outputs, int rows, hipStream_t stream) {
  if (max_outputs <= 0) return 0;
  j.L = d->L; j.M = d->M; j.H = d->H; j.T = d->T; j.P = d->tile_periods;
  j.sh = skew_shift(d->M);
  if (d->tile_periods == 0) {
    const long long nb = (max_outputs + kThreads - 1) / kThreads;
    VS_REQUIRE(nb < (1LL << 31), "resample: %lld outputs per row in one call", max_outputs);
    hipLaunchKernelGGL(resample_direct_kernel, dim3((unsigned)nb, (unsigned)rows), dim3(kThreads), 0, stream, j);
    VS_LAUNCH_CHECK();
    return 0;
  }
  j.span_floats = (int)span_floats(d->tile_periods, d->M, d->T, j.sh);
  const long long periods = (first_output + max_outputs + d->L - 1) / d->L - first_output / d->L;
  const long long tiles = (periods + d->tile_periods - 1) / d->tile_periods;
  VS_REQUIRE(tiles < (1LL << 31), "resample: %lld outputs per row in one call", max_outputs);
  auto kernel = j.sh ? resample_tile_kernel<true> : resample_tile_kernel<false>;
  VS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, d->lds_bytes));
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(kThreads), (size_t)d->lds_bytes, stream, j);
  VS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int vs_resample_plan(int sr_in, int sr_out, vs_resample_dims* dims) { return plan(sr_in, sr_out, dims); }

long long vs_resample_out_len(const vs_resample_dims* dims, long long n_in) {
  if (!dims || dims->L <= 0 || dims->M <= 0 || n_in < 0 || n_in > kMaxPos) {
    vs_set_error("resample_out_len: n_in=%lld (0 .. 2^48) with dims %s", n_in, dims ? "that are not a plan" : "NULL");
    return -1;
  }
  return out_len(dims->L, dims->M, n_in);
}

int vs_resample_bank(const vs_resample_dims* dims, float* bank, void* stream_) {
  if (int rc = checked(dims, "resample_bank")) return rc;
  VS_REQUIRE(bank && (reinterpret_cast<uintptr_t>(bank) & 15) == 0, "resample_bank: the bank must be a 16-byte aligned device buffer");
  const long long n = (long long)dims->L * dims->T;
  hipLaunchKernelGGL(bank_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream_, bank, dims->L,
                     dims->M, dims->H, dims->T);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_resample(const vs_resample_dims* dims, const float* bank, const float* x, long long x_first, long long x_count, long long x_stride,
                long long stream_len, float* y, long long y_first, long long y_count, long long y_stride, int B, void* stream_) {
  if (int rc = checked(dims, "resample")) return rc;
  const int L = dims->L, M = dims->M, H = dims->H;
  VS_REQUIRE(B > 0 && B <= 65535, "resample: B=%d rows (1 .. 65535)", B);
  VS_REQUIRE(y_first >= 0 && y_count >= 0 && y_first + y_count <= kMaxPos, "resample: outputs [%lld, + %lld) (inside 0 .. 2^48)", y_first, y_count);
  VS_REQUIRE(x_count >= 0 && x_first >= -kMaxPos && x_first + x_count <= kMaxPos, "resample: buffer [%lld, + %lld) (inside +- 2^48)", x_first, x_count);
  VS_REQUIRE(stream_len >= -1 && stream_len <= kMaxPos, "resample: stream_len=%lld (-1: unknown, or 0 .. 2^48)", stream_len);
  VS_REQUIRE(stream_len < 0 || y_first + y_count <= out_len(L, M, stream_len),
             "resample: outputs [%lld, %lld) of a stream of %lld samples, which has %lld", y_first, y_first + y_count, stream_len,
             stream_len < 0 ? 0 : out_len(L, M, stream_len));
  if (y_count == 0) return 0;
  VS_REQUIRE(bank && y && (x || x_count == 0), "resample: NULL argument");
  VS_REQUIRE(B == 1 || (y_stride >= y_count && x_stride >= x_count), "resample: row strides %lld / %lld shorter than the rows %lld / %lld",
             x_stride, y_stride, x_count, y_count);
  // samples the outputs read, inside the stream: they must be in the buffer
  long long k_lo = y_first * M / L - H, k_hi = (y_first + y_count - 1) * M / L + H;
  if (k_lo < 0) k_lo = 0;
  if (stream_len >= 0 && k_hi > stream_len - 1) k_hi = stream_len - 1;
  VS_REQUIRE(k_lo > k_hi || (x_first <= k_lo && k_hi < x_first + x_count),
             "resample: outputs [%lld, %lld) read stream samples [%lld, %lld], the buffer holds [%lld, %lld)", y_first, y_first + y_count,
             k_lo, k_hi, x_first, x_first + x_count);
  Job j = {};
  j.bank = bank; j.x = x; j.y = y;
  j.x_first = x_first; j.x_count = x_count; j.x_stride = x_stride; j.stream_len = stream_len;
  j.y_first = y_first; j.y_count = y_count; j.y_stride = y_stride;
  return launch(dims, j, y_first, y_count, B, (hipStream_t)stream_);
}

int vs_resample_clips(const vs_resample_dims* dims, const float* bank, const float* in, long long in_total, float* out, long long out_total,
                      const long long* clips_host, const long long* clips, int N, void* stream_) {
  if (int rc = checked(dims, "resample_clips")) return rc;
  VS_REQUIRE(N > 0, "resample_clips: N=%d clips", N);
  VS_REQUIRE(bank && in && out && clips_host && clips, "resample_clips: NULL argument");
  VS_REQUIRE(in_total >= 0 && in_total <= kMaxPos && out_total >= 0 && out_total <= kMaxPos, "resample_clips: buffers of %lld / %lld samples",
             in_total, out_total);
  for (int first = 0; first < N; first += 65535) {
    const int rows = N - first < 65535 ? N - first : 65535;
    long long longest = 0;
    for (int i = first; i < first + rows; ++i) {
      const long long* c = clips_host + 3LL * i;
      VS_REQUIRE(c[1] >= 0 && c[0] >= 0 && c[0] <= in_total - c[1], "resample_clips: clip %d = [%lld, + %lld) leaves the input buffer of %lld samples",
                 i, c[0], c[1], in_total);
      const long long n_out = out_len(dims->L, dims->M, c[1]);
      VS_REQUIRE(c[2] >= 0 && c[2] <= out_total - n_out, "resample_clips: the %lld outputs of clip %d at %lld leave the output buffer of %lld samples",
                 n_out, i, c[2], out_total);
      if (n_out > longest) longest = n_out;
    }
    Job j = {};
    j.bank = bank; j.x = in; j.y = out;
    j.clips = clips + 3LL * first;
    if (int rc = launch(dims, j, 0, longest, rows, (hipStream_t)stream_)) return rc;
  }
  return 0;
}
