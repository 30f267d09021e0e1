// Griffin-Lim (vs_griffin_lim): the other branch of ap.inv_spectrogram: no phase given -> _griffin_lim(S**power),
// utils/audio_processor.py:492-496, 516-523
//   y = istft(S * angles);  n_iter times: angles = exp(1j * angle(stft(y))), y = istft(S * angles)
// as phase retrieval by alternating projections, resident on the device: bases, envelope, S and the iSTFT-side operand scale are built
// once.  Fixed for the whole call: the target magnitude S [M][F] and, per item, sum S^2 (den[b], fp64).  One iteration is
//   frames <- w * reflect(overlap_add(frames) / env)   (stft.hip's two kernels, or gl_reframe_kernel in one launch)
//   reim   <- frames @ fbasis^T                        (STFT)
//   reim   <- S * reim / |reim|                        (gl_project_kernel, in place)
//   frames <- reim @ basis^T                           (iSTFT)
// so the phase only ever exists as a direction: no atan2 / sincos / exp inside the loop.
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "stft_common.h"

namespace {

// sum of v over a workgroup of 256 (valid in every thread after the barrier), the four waves in a fixed order
__device__ __forceinline__ double gl_block_sum(double v) {
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// vmax[item] = bits of max clip(a*b, 0, 1) over the item (S is monotone in it): one integer atomicMax per wave
// LINEAR (vs_griffin_lim_mag): a is a linear magnitude, the maximum is that of |a|
template <bool LINEAR>
__global__ __launch_bounds__(256)
void gl_item_max_kernel(const float* __restrict__ a, const float* __restrict__ b, unsigned* __restrict__ vmax, VsStftShape s) {
  const int item = blockIdx.y;
  const int n = s.T * s.F;
  const size_t base = (size_t)item * n;
  float m = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    float v = a[base + i];
    if constexpr (LINEAR) {
      m = fmaxf(m, fabsf(v));
    } else {
      if (b) v *= b[base + i];
      m = fmaxf(m, fminf(fmaxf(v, 0.f), 1.f));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(&vmax[item], __float_as_uint(m));
}

// Every item runs at its own power-of-two level: S[item] is stored times 2^-e, e = the exponent of the item's largest S, and the
// last overlap-add multiplies by gain[item] = 2^e.  The loop is linear in the level, so this changes no value -- but the split-f16
// contractions take ONE operand scale for the whole batch, and a quiet item beside a loud one (1e-5 of its level: an all-zero mask)
// would keep its lo halves in f16 subnormals.
// S = (db_to_amp(denormalize(a*b) + ref))^power as an fp32 array, the first spectrum S * e^{i phase} as (re | im) rows (ld padding
// zeroed), |max| S (the iSTFT-side operand scale of every round: |re|, |im| <= S after a projection, up to an ulp of rounding in
// S * (re * rsqrt) -- covered by the scale rule of scale_from_absmax_kernel, which puts the bound in [2^9, 2^10), a factor 64 below
// f16's largest value) and den[b] += sum S^2.
// grid (gx, B): a workgroup stays inside one item.
// LINEAR (vs_griffin_lim_mag): S = |a|^power, a a linear magnitude (np.abs(S ** power) of _griffin_lim's callers)
template <bool LINEAR>
__global__ __launch_bounds__(256)
void gl_target_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ phase, float power,
                      float* __restrict__ S, float* __restrict__ reim, double* __restrict__ den, VsStftShape s,
                      unsigned* __restrict__ amax, const unsigned* __restrict__ vmax, float* __restrict__ gain) {
  const int item = blockIdx.y;
  const int n = s.T * s.F;
  const size_t base = (size_t)item * n;
  const double kpow = 0.11512925464970228 * (double)power;      // ln(10) / 20 * power
  int e = 0;
  if constexpr (LINEAR) (void)frexp(pow((double)__uint_as_float(vmax[item]), (double)power), &e);
  else (void)frexp(exp((((double)__uint_as_float(vmax[item]) - 1.0) * (-(double)s.min_level_db) + (double)s.ref_level_db) * kpow), &e);
  e = e > 120 ? 120 : (e < -120 ? -120 : e);
  const double level = ldexp(1.0, -e);
  if (blockIdx.x == 0 && threadIdx.x == 0) gain[item] = ldexpf(1.f, e);
  float mx = 0.f;
  double acc = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int t = i / s.F, f = i - t * s.F;
    const size_t row = ((size_t)item * s.T + t) * s.ldk;
    // in fp64, once per call: S is what every round is measured against (an fp32 dB value alone is only good to ~7e-7 of S)
    double v = a[base + i];
    float mag;
    if constexpr (LINEAR) {
      mag = (float)(pow(fabs(v), (double)power) * level);
    } else {
      if (b) v *= (double)b[base + i];
      const double db = (fmin(fmax(v, 0.0), 1.0) - 1.0) * (-(double)s.min_level_db) + (double)s.ref_level_db;
      mag = (float)(exp(db * kpow) * level);
    }
    float sn, cs;
    sincosf(phase[base + i], &sn, &cs);
    S[base + i] = mag;
    reim[row + f] = mag * cs;
    reim[row + s.F + f] = mag * sn;
    if (f == 0) for (int c = s.K; c < s.ldk; ++c) reim[row + c] = 0.f;
    mx = fmaxf(mx, mag);
    acc += (double)mag * (double)mag;
  }
  vs_absmax_commit(mx, amax);
  acc = gl_block_sum(acc);
  if (threadIdx.x == 0) atomicAdd(&den[item], acc);
}

// The projection onto the target magnitude, in place on the (re | im) rows: reim <- S * reim * rsqrt(re^2 + im^2).  A bin whose
// |D|^2 is below the smallest normal float takes phase 0 -- (S, 0), as np.angle(0) == 0 -- never NaN.  num (or NULL):
// num[b] += sum (|D| - S)^2 in fp64, one atomic per workgroup (the waveform path has none).  amax_reset (or NULL): the |max| array
// the NEXT re-framing launch commits into is cleared here, after this round's scale has been derived from it.
__global__ __launch_bounds__(256)
void gl_project_kernel(float* __restrict__ reim, const float* __restrict__ S, double* __restrict__ num, unsigned* __restrict__ amax_reset,
                       VsStftShape s) {
  const int item = blockIdx.y;
  const int n = s.T * s.F;
  const size_t base = (size_t)item * n;
  if (amax_reset && blockIdx.x == 0 && item == 0)
    for (int i = threadIdx.x; i < VS_AMAX_SLOTS; i += 256) amax_reset[i] = 0u;
  double acc = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int t = i / s.F, f = i - t * s.F;
    const size_t row = ((size_t)item * s.T + t) * s.ldk;
    const float re = reim[row + f], im = reim[row + s.F + f];
    const float tgt = S[base + i];
    const float n2 = re * re + im * im;
    float ore = tgt, oim = 0.f, mag = 0.f;
    if (n2 >= 1.17549435e-38f) {
      const float r = rsqrtf(n2);
      ore = tgt * (re * r);
      oim = tgt * (im * r);
      mag = n2 * r;
    }
    reim[row + f] = ore;
    reim[row + s.F + f] = oim;
    if (f == 0) for (int c = s.K; c < s.ldk; ++c) reim[row + c] = 0.f;
    const double d = (double)mag - (double)tgt;
    acc += d * d;
  }
  if (num) {
    acc = gl_block_sum(acc);
    if (threadIdx.x == 0) atomicAdd(&num[item], acc);
  }
}

// overlap_add_kernel and stft_frames_kernel in one launch: out[m][j] = w[j] * y[b][reflect(hop*t - lead + j)] with
// y[b][sp] = (sum_t' in[b*T+t'][sp - hop*t' + lead]) / env[sp] formed on the fly (the same sums in the same order: the same bits).
// ZERO: the clip is padded with zeros instead of its reflection (stft_frames_kernel<true>).
template <bool ZERO>
__global__ __launch_bounds__(256)
void gl_reframe_kernel(const float* __restrict__ in, const float* __restrict__ env, float* __restrict__ out, VsStftShape s,
                       unsigned* __restrict__ amax) {
  const long long n = (long long)s.B * s.T * s.win;
  float mx = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.win;
    const int j = (int)(i - m * s.win);
    const int b = (int)(m / s.T), t = (int)(m - (long long)b * s.T);
    int sp = s.hop * t - s.lead + j;
    float v;
    if constexpr (ZERO) {
      v = (sp < 0 || sp >= s.S) ? 0.f : hann_w(j, s) * (stft_gather(in, b, sp, s) / env[sp]);
    } else {
      if (sp < 0) sp = -sp;
      if (sp >= s.S) sp = 2 * (s.S - 1) - sp;
      v = hann_w(j, s) * (stft_gather(in, b, sp, s) / env[sp]);
    }
    out[i] = v;
    mx = fmaxf(mx, fabsf(v));
  }
  vs_absmax_commit(mx, amax);
}

// the last overlap-add of the call: overlap_add_kernel's sums in its order, times the item's level gain[b] = 2^e (gl_target_kernel)
__global__ __launch_bounds__(256)
void gl_overlap_add_gain_kernel(const float* __restrict__ frames, const float* __restrict__ env, const float* __restrict__ gain,
                                float* __restrict__ wav, VsStftShape s) {
  const int sp = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (sp >= s.S) return;
  wav[(size_t)b * s.S + sp] = (stft_gather(frames, b, sp, s) / env[sp]) * gain[b];
}

// res[i][b]: sum (|D_i| - S)^2  ->  || |D_i| - S || / || S ||
__global__ void gl_residual_kernel(double* __restrict__ res, const double* __restrict__ den, int n_iter, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_iter * B) return;
  const double d = den[i % B];
  res[i] = d > 0.0 ? sqrt(res[i] / d) : 0.0;
}

int g_gl_reframe = 0;      // vs_set_griffin_lim_reframe

// vs_griffin_lim (linear = false: spec, mask are stored dB01 values) and vs_griffin_lim_mag (linear = true: spec is a linear
// magnitude, mask NULL; zero_pad: the inner transform pads the clip with zeros)
int gl_run(const vs_loss_dims* d, const float* spec, const float* mask, bool linear, bool zero_pad, const float* init_phase, float power,
           int n_iter, float* wav, double* residual, void* ws, size_t ws_bytes, hipStream_t stream);

}  // namespace

extern "C" {

size_t vs_griffin_lim_workspace_bytes(const vs_loss_dims* d) { return vs_sisnr_workspace_bytes(d); }

int vs_set_griffin_lim_reframe(int mode) {
  VS_REQUIRE(mode >= 0 && mode <= 2, "vs_set_griffin_lim_reframe: mode %d (0 = default, 1 = overlap-add + framing, 2 = one gather launch)", mode);
  g_gl_reframe = mode;
  return 0;
}

int vs_griffin_lim(const vs_loss_dims* d, const float* spec, const float* mask, const float* init_phase, float power, int n_iter,
                   float* wav, double* residual, void* ws, size_t ws_bytes, void* stream_) {
  return gl_run(d, spec, mask, false, false, init_phase, power, n_iter, wav, residual, ws, ws_bytes, (hipStream_t)stream_);
}

int vs_griffin_lim_mag(const vs_loss_dims* d, const float* mag, const float* init_phase, float power, int n_iter, int pad,
                       float* wav, double* residual, void* ws, size_t ws_bytes, void* stream_) {
  VS_REQUIRE(pad == VS_PAD_REFLECT || pad == VS_PAD_ZERO, "griffin_lim_mag: pad=%d (0 = reflect, 1 = zeros)", pad);
  return gl_run(d, mag, nullptr, true, pad == VS_PAD_ZERO, init_phase, power, n_iter, wav, residual, ws, ws_bytes, (hipStream_t)stream_);
}

}  // extern "C"

namespace {

int gl_run(const vs_loss_dims* d, const float* spec, const float* mask, bool linear, bool zero_pad, const float* init_phase, float power,
           int n_iter, float* wav, double* residual, void* ws, size_t ws_bytes, hipStream_t stream) {
  VsStftShape s;
  if (int rc = vs_stft_make_shape(d, &s)) return rc;
  s.periodic = 1;
  s.true_phase = 1;
  const VsStftLayout L = vs_stft_layout(s);
  VS_REQUIRE(spec && init_phase && wav, "griffin_lim: NULL argument");
  VS_REQUIRE(n_iter >= 0, "griffin_lim: n_iter=%d", n_iter);
  VS_REQUIRE(power > 0.f && power < 3.0e38f, "griffin_lim: power=%g must be greater than 0", (double)power);
  VS_REQUIRE(s.S > s.n_fft / 2, "griffin_lim: clip shorter than the reflect padding");
  VS_REQUIRE((long long)s.T * s.F < (1ll << 31), "griffin_lim: T*F too large");
  if (int rc = vs_stft_check_envelope(s)) return rc;
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total, "griffin_lim: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  const int M = s.B * s.T;
  float* basis = at<float>(ws, L.basis);
  float* fbasis = at<float>(ws, L.fbasis);
  float* env = at<float>(ws, L.env);
  float* reim = at<float>(ws, L.reim_e);
  float* S = at<float>(ws, L.reim_t);              // [M][F] of the [M][ldk] region
  float* frames = at<float>(ws, L.frames_e);
  float* frames2 = at<float>(ws, L.frames_t);      // the gather form reads one array and writes the other
  double* den = at<double>(ws, L.mom);
  unsigned* vmax = at<unsigned>(ws, L.coef);       // [B] uint, then [B] float: every item's level (gl_target_kernel)
  float* gain = at<float>(ws, L.coef) + s.B;
  const bool split = vs_stft_split(s);
  unsigned* amax = at<unsigned>(ws, L.amax);       // [0]: the windowed frames of this round, [1]: S
  float* scales = at<float>(ws, L.scales);         // {s, 1/s}: frames, reim, iSTFT basis, STFT basis
  const bool gather = g_gl_reframe != 1;           // the default is the form with one launch fewer (not yet measured: tools/griffin_lim_time.py)
  vs_istft_basis_launch(basis, s, scales + 4, stream);
  vs_stft_basis_launch(fbasis, s, scales + 6, stream);
  vs_istft_envelope_launch(env, s, stream);
  if (split) VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)2 * VS_AMAX_SLOTS * 4, stream));
  VS_CHECK_HIP(hipMemsetAsync(den, 0, (size_t)s.B * 8, stream));
  VS_CHECK_HIP(hipMemsetAsync(vmax, 0, (size_t)s.B * 4, stream));
  const bool want_res = residual != nullptr && n_iter > 0;
  if (want_res) VS_CHECK_HIP(hipMemsetAsync(residual, 0, (size_t)n_iter * s.B * 8, stream));
  // one resident round of workgroups for the passes that end in a |max| commit or an fp64 atomic (vs_sisnr_loss, call 13)
  const int per_item = (s.T * s.F + 255) / 256;
  int gx = 2048 / s.B < 1 ? 1 : 2048 / s.B;
  if (gx > per_item) gx = per_item;
  const unsigned gfr = vs_grid_for((long long)M * s.win, split ? 2048 : 16384);
  auto istft = [&](float* out) {      // out[M][win] = reim[M][K] @ basis[win][K]^T
    return vs_stft_contract(split, 0, reim, s.ldk, basis, s.ldk, out, s.win, M, s.win, s.K, scales + 2, scales + 4, stream);
  };
  if (linear) {
    hipLaunchKernelGGL(gl_item_max_kernel<true>, dim3(gx, s.B), dim3(256), 0, stream, spec, mask, vmax, s);
    hipLaunchKernelGGL(gl_target_kernel<true>, dim3(gx, s.B), dim3(256), 0, stream, spec, mask, init_phase, power, S, reim, den, s,
                       split ? amax + VS_AMAX_SLOTS : nullptr, vmax, gain);
  } else {
    hipLaunchKernelGGL(gl_item_max_kernel<false>, dim3(gx, s.B), dim3(256), 0, stream, spec, mask, vmax, s);
    hipLaunchKernelGGL(gl_target_kernel<false>, dim3(gx, s.B), dim3(256), 0, stream, spec, mask, init_phase, power, S, reim, den, s,
                       split ? amax + VS_AMAX_SLOTS : nullptr, vmax, gain);
  }
  if (split) if (int rc = vs_scale_from_absmax_impl(amax + VS_AMAX_SLOTS, VS_AMAX_SLOTS, scales + 2, stream)) return rc;
  if (int rc = istft(frames)) return rc;
  for (int it = 0; it < n_iter; ++it) {
    float* cur = frames;
    if (gather) {
      if (zero_pad) hipLaunchKernelGGL(gl_reframe_kernel<true>, dim3(gfr), dim3(256), 0, stream, frames, env, frames2, s, split ? amax : nullptr);
      else hipLaunchKernelGGL(gl_reframe_kernel<false>, dim3(gfr), dim3(256), 0, stream, frames, env, frames2, s, split ? amax : nullptr);
      cur = frames2;
    } else {
      vs_overlap_add_launch(frames, env, wav, s, stream);
      vs_stft_frames_launch(wav, frames, s, split ? amax : nullptr, gfr, stream, zero_pad ? 1 : 0);
    }
    if (split) if (int rc = vs_scale_from_absmax_impl(amax, VS_AMAX_SLOTS, scales, stream)) return rc;
    if (int rc = vs_stft_contract(split, 0, cur, s.win, fbasis, s.win, reim, s.ldk, M, s.K, s.win, scales, scales + 6, stream)) return rc;
    hipLaunchKernelGGL(gl_project_kernel, dim3(gx, s.B), dim3(256), 0, stream, reim, S, want_res ? residual + (size_t)it * s.B : nullptr,
                       split ? amax : nullptr, s);
    if (int rc = istft(frames)) return rc;
  }
  hipLaunchKernelGGL(gl_overlap_add_gain_kernel, dim3((s.S + 255) / 256, s.B), dim3(256), 0, stream, frames, env, gain, wav, s);
  if (want_res) hipLaunchKernelGGL(gl_residual_kernel, dim3((n_iter * s.B + 255) / 256), dim3(256), 0, stream, residual, den, n_iter, s.B);
  VS_LAUNCH_CHECK();
  return 0;
}

}  // namespace
