// The wavernn and waveglow audio back ends of WrapperAudioProcessor (utils/audio_processor.py:61-438, utils/audio.py:49-135,
// utils/stft.py:36-99) around stft.hip's transform.  Both foreign processors run the transform the voicefilter one runs (periodic
// Hann centred in the frame, reflect padding, |D| = sqrt(re^2 + im^2)); what differs is the CODEC between a linear magnitude and the
// stored value, a pre-emphasis in front of the transform, a mel projection behind it, and the padding of Griffin-Lim's inner
// transform (griffin_lim.hip).  Here:
//   front end      frames of the pre-emphasised clip (the difference formed inside the framing gather) -> the split-f16 contraction
//                  of vs_wav_to_spec -> |D| [-> mel basis] -> encode
//   codec          decode / encode of a whole array, evaluated in fp64 and rounded once (as gl_target_kernel does)
//   projection     out = max(floor, in @ W^T) in fixed-order fp32 FMAs: mel basis, its pseudo-inverse, mag_to_mel
//   inverse        the iSTFT of a linear magnitude with a given phase
//   de-emphasis    y[n] = x[n] + a y[n-1] as a two-sweep scan in fp64 (the scheme of loudness.hip's K-weighting filter)
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "stft_common.h"

namespace {

constexpr int kDeBlock = 128;      // samples per block of the de-emphasis scan (vs_deemphasis_block)
constexpr int kDeTile = 64;        // blocks per workgroup: one wave, a thread per block, the tile staged in LDS

// ---- codec ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// linear magnitude -> stored value
__device__ __forceinline__ float codec_encode(double m, const vs_audio_codec& c) {
  m = fmax(c.floor, m);
  if (c.kind == VS_CODEC_LOG) return (float)log(m);
  const double S = 20.0 * log10(m) - c.ref_level_db;
  if (c.kind == VS_CODEC_DB01) return (float)(clampd(S / -c.min_level_db, -1.0, 0.0) + 1.0);
  if (!c.signal_norm) return (float)S;                                       // _normalize :140-155
  double n = (S - c.min_level_db) / -c.min_level_db;
  if (c.symmetric_norm) {
    n = (2.0 * c.max_norm) * n - c.max_norm;
    if (c.clip_norm) n = clampd(n, -c.max_norm, c.max_norm);
  } else {
    n = c.max_norm * n;
    if (c.clip_norm) n = clampd(n, 0.0, c.max_norm);
  }
  return (float)n;
}

// stored value -> linear magnitude (fp64; the caller rounds)
__device__ __forceinline__ double codec_decode(double v, const vs_audio_codec& c) {
  if (c.kind == VS_CODEC_LOG) return exp(v);
  double S = v;
  if (c.kind == VS_CODEC_DB01) {
    S = (clampd(v, 0.0, 1.0) - 1.0) * -c.min_level_db;
  } else if (c.signal_norm) {                                                // _denormalize :157-173: clip first
    if (c.symmetric_norm) {
      if (c.clip_norm) S = clampd(S, -c.max_norm, c.max_norm);
      S = ((S + c.max_norm) * -c.min_level_db / (2.0 * c.max_norm)) + c.min_level_db;
    } else {
      if (c.clip_norm) S = clampd(S, 0.0, c.max_norm);
      S = (S * -c.min_level_db / c.max_norm) + c.min_level_db;
    }
  }
  return pow(10.0, (S + c.ref_level_db) * 0.05);
}

__global__ __launch_bounds__(256)
void codec_decode_kernel(const float* spec, const float* mask, float* mag, long long n, vs_audio_codec c) {      // mag may be spec
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    double v = spec[i];
    if (mask) v *= (double)mask[i];
    mag[i] = (float)codec_decode(v, c);
  }
}

__global__ __launch_bounds__(256)
void codec_encode_kernel(const float* mag, float* spec, long long n, vs_audio_codec c) {      // spec may be mag
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    spec[i] = codec_encode((double)mag[i], c);
}

// ---- front end --------------------------------------------------------------------------------------------------------------
// stft_frames_kernel on the pre-emphasised clip p[n] = x[n] - a x[n-1] (x[-1] = 0): the reflection picks the sample of p, the
// difference is formed in fp64 and rounded once, so the frame carries half an ulp of p, not of x.  S > n_fft / 2: one reflection.
__global__ __launch_bounds__(256)
void codec_frames_kernel(const float* __restrict__ wav, float* __restrict__ frames, VsStftShape s, double a, unsigned* __restrict__ amax) {
  const long long n = (long long)s.B * s.T * s.win;
  float mx = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.win;
    const int j = (int)(i - m * s.win);
    const int b = (int)(m / s.T), t = (int)(m - (long long)b * s.T);
    int idx = s.hop * t - s.lead + j;
    if (idx < 0) idx = -idx;
    if (idx >= s.S) idx = 2 * (s.S - 1) - idx;
    const float* x = wav + (size_t)b * s.S;
    const double prev = idx > 0 ? (double)x[idx - 1] : 0.0;
    const float p = (float)((double)x[idx] - a * prev);
    const float v = hann_w(j, s) * p;
    frames[i] = v;
    mx = fmaxf(mx, fabsf(v));
  }
  vs_absmax_commit(mx, amax);
}

// (re | im) rows -> out = |D| (linear: the mel projection follows) or encode(|D|), and phase = angle(D)
__global__ __launch_bounds__(256)
void codec_features_kernel(const float* __restrict__ reim, float* __restrict__ out, float* __restrict__ phase, VsStftShape s,
                           vs_audio_codec c, int linear) {
  const long long n = (long long)s.B * s.T * s.F;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.F;
    const int f = (int)(i - m * s.F);
    const float re = reim[m * s.ldk + f], im = reim[m * s.ldk + s.F + f];
    const float mag = sqrtf(re * re + im * im);
    out[i] = linear ? mag : codec_encode((double)mag, c);
    if (phase) phase[i] = atan2f(im, re);
  }
}

// ---- projection -------------------------------------------------------------------------------------------------------------
// out[m][n] = max(floor, sum_k in[m][k] w[n][k]), one fmaf chain per output in the order k = 0 .. K-1.  A workgroup owns a 16 x 16
// tile of outputs and walks K in slices of 32 staged in LDS (row stride 33: no bank conflicts on the column reads).
__global__ __launch_bounds__(256)
void project_floor_kernel(const float* __restrict__ in, const float* __restrict__ w, float* __restrict__ out, long long M, int N, int K,
                          float floor) {
  __shared__ float a_s[16][33], w_s[16][33];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const long long m0 = (long long)blockIdx.y * 16;
  const int n0 = blockIdx.x * 16;
  float acc = 0.f;
  for (int k0 = 0; k0 < K; k0 += 32) {
    for (int e = threadIdx.x; e < 16 * 32; e += 256) {
      const int r = e >> 5, k = k0 + (e & 31);
      a_s[r][e & 31] = (m0 + r < M && k < K) ? in[(size_t)(m0 + r) * K + k] : 0.f;
      w_s[r][e & 31] = (n0 + r < N && k < K) ? w[(size_t)(n0 + r) * K + k] : 0.f;
    }
    __syncthreads();
    const int kn = K - k0 < 32 ? K - k0 : 32;
    for (int k = 0; k < kn; ++k) acc = fmaf(a_s[ty][k], w_s[tx][k], acc);
    __syncthreads();
  }
  if (m0 + ty < M && n0 + tx < N) out[(size_t)(m0 + ty) * N + n0 + tx] = fmaxf(floor, acc);
}

// ---- inverse with a given phase ---------------------------------------------------------------------------------------------
// spec_to_reim_kernel behind the decoder: reim[m][k] = mag cos phi (k < F) | mag sin phi
__global__ __launch_bounds__(256)
void mag_to_reim_kernel(const float* __restrict__ mag, const float* __restrict__ phase, float* __restrict__ reim, VsStftShape s,
                        unsigned* __restrict__ amax) {
  const long long n = (long long)s.B * s.T * s.F;
  float mx = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.F;
    const int f = (int)(i - m * s.F);
    float sn, cs;
    sincosf(phase[i], &sn, &cs);
    const float re = mag[i] * cs, im = mag[i] * sn;
    reim[m * s.ldk + f] = re;
    reim[m * s.ldk + s.F + f] = im;
    if (f == 0) for (int c = s.K; c < s.ldk; ++c) reim[m * s.ldk + c] = 0.f;
    mx = fmaxf(mx, fmaxf(fabsf(re), fabsf(im)));
  }
  vs_absmax_commit(mx, amax);
}

// ---- pre-emphasis and its inverse -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void preemphasis_kernel(const float* __restrict__ x, float* __restrict__ y, long long N, double a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float* xr = x + (size_t)blockIdx.y * N;
  const double prev = i > 0 ? (double)xr[i - 1] : 0.0;
  y[(size_t)blockIdx.y * N + i] = (float)((double)xr[i] - a * prev);
}

// One sweep of the recurrence z[j] = x[j] + a z[j-1] over every block of kDeBlock samples from a zero state.  A workgroup is one
// wave; it stages kDeTile consecutive blocks of one row in LDS with coalesced loads (row stride kDeBlock + 1: thread t walks row t
// without bank conflicts), then thread t sweeps block t.
//   FINAL = false: last[row][k] = z[L-1] of every block that has a successor.
//   FINAL = true:  y[j] = fp32(z[j] + a^(j+1) carry[row][k]), a^(j+1) by repeated multiplication from a: a function of j alone.
// Grid (tiles, B).  nblk = ceil(N / kDeBlock).
template <bool FINAL>
__global__ __launch_bounds__(kDeTile)
void deemphasis_sweep_kernel(const float* __restrict__ x, float* __restrict__ y, long long N, int nblk, double a,
                             double* __restrict__ last, const double* __restrict__ carry) {
  __shared__ float tile[kDeTile * (kDeBlock + 1)];
  const int row = blockIdx.y;
  const long long base = (long long)blockIdx.x * kDeTile * kDeBlock;      // first sample of the tile
  const long long left = N - base;
  const int cnt = left < (long long)kDeTile * kDeBlock ? (int)left : kDeTile * kDeBlock;
  const float* xr = x + (size_t)row * N + base;
  for (int e = threadIdx.x; e < cnt; e += kDeTile) tile[(e / kDeBlock) * (kDeBlock + 1) + (e % kDeBlock)] = xr[e];
  __syncthreads();
  const int k = blockIdx.x * kDeTile + threadIdx.x;                       // this thread's block of the row
  const int len = cnt - (int)threadIdx.x * kDeBlock < kDeBlock ? cnt - (int)threadIdx.x * kDeBlock : kDeBlock;
  if (k < nblk && len > 0) {
    float* t = tile + threadIdx.x * (kDeBlock + 1);
    double z = 0.0;
    if constexpr (FINAL) {
      const double c = carry[(size_t)row * nblk + k];
      double ap = 1.0;
      for (int j = 0; j < len; ++j) {      // products and sums rounded one by one (no contraction): the bits of the plain recurrence
        z = __dadd_rn((double)t[j], __dmul_rn(a, z));
        ap = __dmul_rn(ap, a);
        t[j] = (float)__dadd_rn(z, __dmul_rn(ap, c));
      }
    } else {
      for (int j = 0; j < len; ++j) z = __dadd_rn((double)t[j], __dmul_rn(a, z));
      if (k + 1 < nblk) last[(size_t)row * nblk + k] = z;
    }
  }
  if constexpr (FINAL) {
    __syncthreads();
    float* yr = y + (size_t)row * N + base;
    for (int e = threadIdx.x; e < cnt; e += kDeTile) yr[e] = tile[(e / kDeBlock) * (kDeBlock + 1) + (e % kDeBlock)];
  }
}

// carry[row][0] = 0, carry[row][k+1] = a^L carry[row][k] + last[row][k]: one thread per row, a^L by the sweep's own multiplications
__global__ void deemphasis_carry_kernel(const double* __restrict__ last, double* __restrict__ carry, int B, int nblk, double a) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  double aL = 1.0;
  for (int j = 0; j < kDeBlock; ++j) aL = __dmul_rn(aL, a);
  double c = 0.0;
  for (int k = 0; k < nblk; ++k) {
    carry[(size_t)row * nblk + k] = c;
    if (k + 1 < nblk) c = __dadd_rn(__dmul_rn(aL, c), last[(size_t)row * nblk + k]);
  }
}

int check_codec(const vs_audio_codec* c, const char* what) {
  VS_REQUIRE(c != nullptr, "%s: codec is NULL", what);
  VS_REQUIRE(c->kind == VS_CODEC_DB01 || c->kind == VS_CODEC_DBNORM || c->kind == VS_CODEC_LOG, "%s: unknown codec kind %d", what, c->kind);
  VS_REQUIRE(c->floor > 0.0, "%s: codec floor %g must be positive", what, c->floor);
  if (c->kind != VS_CODEC_LOG) {
    VS_REQUIRE(c->min_level_db < 0.0, "%s: min_level_db %g must be negative", what, c->min_level_db);
    VS_REQUIRE(c->kind != VS_CODEC_DBNORM || !c->signal_norm || c->max_norm > 0.0, "%s: max_norm %g must be positive", what, c->max_norm);
  }
  return 0;
}

}  // namespace

extern "C" {

int vs_codec_wav_to_spec(const vs_loss_dims* d, const vs_audio_codec* codec, const float* wav, const float* mel_basis, int n_mels,
                         float* out, float* phase, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VsStftShape s;
  if (int rc = vs_stft_make_shape(d, &s)) return rc;
  if (int rc = check_codec(codec, "codec_wav_to_spec")) return rc;
  s.periodic = 1;
  const VsStftLayout L = vs_stft_layout(s);
  VS_REQUIRE(wav && out, "codec_wav_to_spec: NULL argument");
  VS_REQUIRE(mel_basis == nullptr || (n_mels > 0 && ((long long)s.B * s.T + 15) / 16 <= 65535), "codec_wav_to_spec: n_mels=%d, B*T=%lld with a mel basis", n_mels, (long long)s.B * s.T);
  VS_REQUIRE(s.S > s.n_fft / 2, "codec_wav_to_spec: clip shorter than the reflect padding");
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total, "codec_wav_to_spec: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  const int M = s.B * s.T;
  float* frames = at<float>(ws, L.frames_e);
  float* basis = at<float>(ws, L.fbasis);
  float* reim = at<float>(ws, L.reim_e);
  float* mag = at<float>(ws, L.reim_t);            // [M][F] of the [M][ldk] region: the linear magnitude in front of the mel basis
  const bool split = vs_stft_split(s);
  unsigned* amax = at<unsigned>(ws, L.amax);
  float* scales = at<float>(ws, L.scales);
  if (split) VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)VS_AMAX_SLOTS * 4, stream));
  hipLaunchKernelGGL(codec_frames_kernel, dim3(vs_grid_for((long long)M * s.win, split ? 2048 : 16384)), dim3(256), 0, stream, wav, frames, s,
                     codec->preemphasis, split ? amax : nullptr);
  vs_stft_basis_launch(basis, s, scales + 6, stream);
  if (split) if (int rc = vs_scale_from_absmax_impl(amax, VS_AMAX_SLOTS, scales, stream)) return rc;
  if (int rc = vs_stft_contract(split, 0, frames, s.win, basis, s.win, reim, s.ldk, M, s.K, s.win, scales, scales + 6, stream)) return rc;
  const unsigned gf = vs_grid_for((long long)M * s.F, 16384);
  if (mel_basis == nullptr) {
    hipLaunchKernelGGL(codec_features_kernel, dim3(gf), dim3(256), 0, stream, reim, out, phase, s, *codec, 0);
  } else {
    hipLaunchKernelGGL(codec_features_kernel, dim3(gf), dim3(256), 0, stream, reim, mag, phase, s, *codec, 1);
    hipLaunchKernelGGL(project_floor_kernel, dim3((n_mels + 15) / 16, (M + 15) / 16), dim3(256), 0, stream, mag, mel_basis, out, (long long)M,
                       n_mels, s.F, 0.f);
    hipLaunchKernelGGL(codec_encode_kernel, dim3(vs_grid_for((long long)M * n_mels, 16384)), dim3(256), 0, stream, out, out, (long long)M * n_mels, *codec);
  }
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_codec_decode(const vs_audio_codec* codec, const float* spec, const float* mask, long long n, float* mag, void* stream_) {
  if (int rc = check_codec(codec, "codec_decode")) return rc;
  VS_REQUIRE(spec && mag && n > 0, "codec_decode: NULL argument or n=%lld", n);
  hipLaunchKernelGGL(codec_decode_kernel, dim3(vs_grid_for(n, 16384)), dim3(256), 0, (hipStream_t)stream_, spec, mask, mag, n, *codec);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_codec_encode(const vs_audio_codec* codec, const float* mag, long long n, float* spec, void* stream_) {
  if (int rc = check_codec(codec, "codec_encode")) return rc;
  VS_REQUIRE(spec && mag && n > 0, "codec_encode: NULL argument or n=%lld", n);
  hipLaunchKernelGGL(codec_encode_kernel, dim3(vs_grid_for(n, 16384)), dim3(256), 0, (hipStream_t)stream_, mag, spec, n, *codec);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_project_floor(const float* in, const float* w, float* out, long long M, int N, int K, float floor, void* stream_) {
  VS_REQUIRE(in && w && out, "project_floor: NULL argument");
  VS_REQUIRE(M > 0 && N > 0 && K > 0, "project_floor: bad dims M=%lld N=%d K=%d", M, N, K);
  VS_REQUIRE((M + 15) / 16 <= 65535, "project_floor: M=%lld too large", M);
  hipLaunchKernelGGL(project_floor_kernel, dim3((N + 15) / 16, (unsigned)((M + 15) / 16)), dim3(256), 0, (hipStream_t)stream_, in, w, out, M, N, K, floor);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_mag_to_wav(const vs_loss_dims* d, const float* mag, const float* phase, float* wav, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VsStftShape s;
  if (int rc = vs_stft_make_shape(d, &s)) return rc;
  s.periodic = 1;
  s.true_phase = 1;
  const VsStftLayout L = vs_stft_layout(s);
  VS_REQUIRE(mag && phase && wav, "mag_to_wav: NULL argument");
  if (int rc = vs_stft_check_envelope(s)) return rc;
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total, "mag_to_wav: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  const int M = s.B * s.T;
  float* basis = at<float>(ws, L.basis);
  float* env = at<float>(ws, L.env);
  float* reim = at<float>(ws, L.reim_e);
  float* frames = at<float>(ws, L.frames_e);
  const bool split = vs_stft_split(s);
  unsigned* amax = at<unsigned>(ws, L.amax);
  float* scales = at<float>(ws, L.scales);
  vs_istft_basis_launch(basis, s, scales + 6, stream);
  vs_istft_envelope_launch(env, s, stream);
  if (split) VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)VS_AMAX_SLOTS * 4, stream));
  hipLaunchKernelGGL(mag_to_reim_kernel, dim3(vs_grid_for((long long)M * s.F, split ? 2048 : 16384)), dim3(256), 0, stream, mag, phase, reim, s,
                     split ? amax : nullptr);
  if (split) if (int rc = vs_scale_from_absmax_impl(amax, VS_AMAX_SLOTS, scales, stream)) return rc;
  if (int rc = vs_stft_contract(split, 0, reim, s.ldk, basis, s.ldk, frames, s.win, M, s.win, s.K, scales, scales + 6, stream)) return rc;
  vs_overlap_add_launch(frames, env, wav, s, stream);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_deemphasis_block(void) { return kDeBlock; }

size_t vs_deemphasis_workspace_bytes(int B, long long N) {
  if (B <= 0 || N <= 0) { vs_set_error("deemphasis: bad dims B=%d N=%lld", B, N); return 0; }
  const long long nblk = (N + kDeBlock - 1) / kDeBlock;
  return 2 * align_up((size_t)B * nblk * 8);
}

int vs_deemphasis(const float* x, float* y, int B, long long N, double coef, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(x && y && x != y, "deemphasis: NULL argument, or x == y");
  VS_REQUIRE(B > 0 && B <= 65535 && N > 0 && N < (1ll << 40), "deemphasis: bad dims B=%d N=%lld", B, N);
  VS_REQUIRE(coef > -1.0 && coef < 1.0, "deemphasis: coefficient %g must lie inside (-1, 1)", coef);
  const long long nblk_ll = (N + kDeBlock - 1) / kDeBlock;
  VS_REQUIRE(nblk_ll < (1ll << 31), "deemphasis: N=%lld too large", N);
  const int nblk = (int)nblk_ll;
  const size_t piece = align_up((size_t)B * nblk * 8);
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= 2 * piece, "deemphasis: workspace too small or misaligned (%zu < %zu)", ws_bytes, 2 * piece);
  double* last = at<double>(ws, 0);
  double* carry = at<double>(ws, piece);
  const unsigned tiles = (unsigned)((nblk + kDeTile - 1) / kDeTile);
  hipLaunchKernelGGL(deemphasis_sweep_kernel<false>, dim3(tiles, B), dim3(kDeTile), 0, stream, x, y, N, nblk, coef, last, (const double*)nullptr);
  hipLaunchKernelGGL(deemphasis_carry_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, last, carry, B, nblk, coef);
  hipLaunchKernelGGL(deemphasis_sweep_kernel<true>, dim3(tiles, B), dim3(kDeTile), 0, stream, x, y, N, nblk, coef, (double*)nullptr, carry);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_preemphasis(const float* x, float* y, int B, long long N, double coef, void* stream_) {
  VS_REQUIRE(x && y && x != y, "preemphasis: NULL argument, or x == y");
  VS_REQUIRE(B > 0 && B <= 65535 && N > 0 && (N + 255) / 256 < (1ll << 31), "preemphasis: bad dims B=%d N=%lld", B, N);
  hipLaunchKernelGGL(preemphasis_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, (hipStream_t)stream_, x, y, N, coef);
  VS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
