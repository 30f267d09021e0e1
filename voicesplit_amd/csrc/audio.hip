// Audio front / back end of inference: test.py's loop around the model
//   mixed_spec, mixed_phase = ap.get_spec_from_audio(wav)        utils/audio_processor.py:469-476
//   est_wav = ap.inv_spectrogram(est_mask*mixed_spec, mixed_phase)    :478-491, generic_utils.py:496-504
// both as one GEMM against a windowed DFT basis plus a gather (frames in / overlap-add out): stft.hip's transform with librosa's
// periodic Hann window and, on the way back, the true phase (mag*cos, mag*sin).  Here: the dB / phase epilogue and the two entry points.
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "stft_common.h"

namespace {

// spec = clip((20 log10(max(1e-5, |D|)) - ref) / -min_db, -1, 0) + 1;  phase = angle(D)
// (wav2spec, utils/audio_processor.py:469-476 with amp_to_db :537-538 and normalize :543-544)
__global__ __launch_bounds__(256)
void reim_to_features_kernel(const float* __restrict__ reim, float* __restrict__ spec, float* __restrict__ phase, VsStftShape s) {
  const long long n = (long long)s.B * s.T * s.F;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.F;
    const int f = (int)(i - m * s.F);
    const float re = reim[m * s.ldk + f], im = reim[m * s.ldk + s.F + f];
    const float mag = sqrtf(re * re + im * im);
    const float db = 20.0f * log10f(fmaxf(1e-5f, mag)) - s.ref_level_db;
    spec[i] = fminf(fmaxf(db / (-s.min_level_db), -1.0f), 0.0f) + 1.0f;
    if (phase) phase[i] = atan2f(im, re);
  }
}

}  // namespace

extern "C" {

size_t vs_audio_workspace_bytes(const vs_loss_dims* d) { return vs_sisnr_workspace_bytes(d); }

int vs_wav_to_spec(const vs_loss_dims* d, const float* wav, float* spec, float* phase, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VsStftShape s;
  if (int rc = vs_stft_make_shape(d, &s)) return rc;
  s.periodic = 1;
  const VsStftLayout L = vs_stft_layout(s);
  VS_REQUIRE(wav && spec, "wav_to_spec: NULL argument");
  VS_REQUIRE(s.S > s.n_fft / 2, "wav_to_spec: clip shorter than the reflect padding");
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total, "wav_to_spec: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  const int M = s.B * s.T;
  float* frames = at<float>(ws, L.frames_e);
  float* basis = at<float>(ws, L.fbasis);
  float* reim = at<float>(ws, L.reim_e);
  // (the contraction as split-f16 products, as in vs_sisnr_loss [r6]; win % 4 != 0 falls to the kernel's scalar-load instance)
  const bool split = vs_stft_split(s);
  unsigned* amax = at<unsigned>(ws, L.amax);
  float* scales = at<float>(ws, L.scales);
  if (split) VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)VS_AMAX_SLOTS * 4, stream));
  vs_stft_frames_launch(wav, frames, s, split ? amax : nullptr, vs_grid_for((long long)M * s.win, split ? 2048 : 16384), stream);
  vs_stft_basis_launch(basis, s, scales + 6, stream);
  if (split) if (int rc = vs_scale_from_absmax_impl(amax, VS_AMAX_SLOTS, scales, stream)) return rc;
  if (int rc = vs_stft_contract(split, 0, frames, s.win, basis, s.win, reim, s.ldk, M, s.K, s.win, scales, scales + 6, stream)) return rc;
  hipLaunchKernelGGL(reim_to_features_kernel, dim3(vs_grid_for((long long)M * s.F, 16384)), dim3(256), 0, stream, reim, spec, phase, s);
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_spec_to_wav(const vs_loss_dims* d, const float* spec, const float* mask, const float* phase, float* wav,
                   void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VsStftShape s;
  if (int rc = vs_stft_make_shape(d, &s)) return rc;
  s.periodic = 1;
  s.true_phase = 1;
  const VsStftLayout L = vs_stft_layout(s);
  VS_REQUIRE(spec && phase && wav, "spec_to_wav: NULL argument");
  if (int rc = vs_stft_check_envelope(s)) return rc;
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total, "spec_to_wav: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  const int M = s.B * s.T;
  float* basis = at<float>(ws, L.basis);
  float* env = at<float>(ws, L.env);
  float* reim = at<float>(ws, L.reim_e);
  float* frames = at<float>(ws, L.frames_e);
  // (the contraction as split-f16 products, as in vs_sisnr_loss [r6])
  const bool split = vs_stft_split(s);
  unsigned* amax = at<unsigned>(ws, L.amax);
  float* scales = at<float>(ws, L.scales);
  vs_istft_basis_launch(basis, s, scales + 6, stream);
  vs_istft_envelope_launch(env, s, stream);
  if (split) VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)VS_AMAX_SLOTS * 4, stream));
  vs_spec_to_reim_launch(spec, mask, phase, reim, s, split ? amax : nullptr, vs_grid_for((long long)M * s.F, split ? 2048 : 16384), stream);
  if (split) if (int rc = vs_scale_from_absmax_impl(amax, VS_AMAX_SLOTS, scales, stream)) return rc;
  if (int rc = vs_stft_contract(split, 0, reim, s.ldk, basis, s.ldk, frames, s.win, M, s.win, s.K, scales, scales + 6, stream)) return rc;
  vs_overlap_add_launch(frames, env, wav, s, stream);
  VS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
