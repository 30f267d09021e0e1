// What loss.hip, audio.hip, griffin_lim.hip and speaker.hip's log-mel front end share: the short-time transform as ONE GEMM against a
// windowed DFT basis plus a gather (frames in / overlap-add out).  The window is `win` <= n_fft samples wide and centred in the frame,
// so only `win` of a frame's n_fft time samples matter: the (inverse) real FFT restricted to them, times the window, is a dense
// [2*(n_fft/2+1)] x [win] matrix.  The shape, the window and the workspace layout are here, the kernels more than one of those files
// launches are in stft.hip behind the launchers declared below.
#pragma once
#include "vs_internal.h"

constexpr float kLn10Over20 = 0.11512925464970229f;      // dB -> amplitude: 10^(dB/20) = exp(dB * ln10/20)

struct VsStftShape {
  int B, T, F, n_fft, hop, win, S;   // S samples per utterance: hop*(T-1) (vs_stft_make_shape), or the clip's own length (log-mel)
  int lead;                          // window sample j of frame t is output sample hop*t - lead + j: n_fft/2 - (n_fft-win)/2
                                     // (the window sits at (n_fft-win)/2 in the frame: win/2 only for even win)
  int K, ldk;                        // K = 2F (re | im), ldk = K rounded up to 4
  float min_level_db, ref_level_db;
  int periodic;      // 0: hann(win, periodic=False) (torch_spec2wav :509); 1: librosa/scipy 'hann' (fftbins=True)
  int true_phase;    // 0: mag*e^{cos}, mag*e^{sin} (torch_spec2wav :506-509); 1: mag*cos, mag*sin (spec2wav :478-481)
};

// one workspace for the loss head, the audio legs and Griffin-Lim (vs_*_workspace_bytes of the three return its total)
struct VsStftLayout { size_t basis, fbasis, env, reim_e, reim_t, frames_e, frames_t, wav_e, wav_t, dwav, mom, coef, amax, scales, total; };

// Hann window of the training loss (torch.hamming_window(win, periodic=False, 0.5, 0.5)) or of
// librosa's stft/istft (scipy get_window('hann', win, fftbins=True))
__device__ __forceinline__ float hann_w(int j, const VsStftShape& s) {
  const int den = s.periodic ? s.win : s.win - 1;
  return den > 0 ? 0.5f - 0.5f * cospif(2.0f * (float)j / (float)den) : 1.0f;
}

// gather form of the overlap-add: the sum over the <= ceil(win/hop) frames that cover sample sp of item b, latest frame first
__device__ __forceinline__ float stft_gather(const float* __restrict__ frames, int b, int sp, const VsStftShape& s) {
  int t_hi = (sp + s.lead) / s.hop;
  if (t_hi > s.T - 1) t_hi = s.T - 1;
  float acc = 0.f;
  for (int t = t_hi; t >= 0; --t) {
    const int j = sp - s.hop * t + s.lead;
    if (j >= s.win) break;
    acc += frames[((size_t)b * s.T + t) * s.win + j];
  }
  return acc;
}

// workgroups of 256 for n elements, at most `cap` (grid-stride kernels) and at least one
inline unsigned vs_grid_for(long long n, unsigned cap = 2048) {
  const long long nb = (n + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : (nb < (long long)cap ? nb : (long long)cap));
}

// ---- stft.hip ----
// the geometry of B items of T frames and S samples each (lead, K, ldk; symmetric window, the training loss's phase form)
void vs_stft_fill_shape(const vs_loss_dims* d, int B, int T, int S, VsStftShape* s);
int vs_stft_make_shape(const vs_loss_dims* d, VsStftShape* s);      // the checks of the loss / audio / Griffin-Lim entry points, S = hop*(T-1)
VsStftLayout vs_stft_layout(const VsStftShape& s);
int vs_stft_check_envelope(const VsStftShape& s);                   // refuses a window envelope that reaches zero
// whether the contractions over M = B*T rows run as split-f16 products: the operands must fit gemm_f16x3.hip's 32-bit offsets
inline bool vs_stft_split(const VsStftShape& s) { return (size_t)s.B * s.T * s.ldk * 4 < (1ull << 32) - 4096; }
// C[M][N] = A[M][K] @ W^T (layout_w 0: W [N][ldw]) or A @ W (layout_w 1: W [K][ldw]).  split: split-f16 products (gemm_f16x3.hip) under
// the operand scales {s, 1/s} a_scale2 / w_scale2, over the WHOLE rows of A (lda columns: the zeroed ld padding behind K included);
// otherwise the general fp32 GEMM over K columns.
int vs_stft_contract(bool split, int layout_w, const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                     const float* a_scale2, const float* w_scale2, hipStream_t);
// launchers of the shared kernels (scale2 / amax may be NULL; `grid`: workgroups of the grid-stride kernels)
void vs_istft_basis_launch(float* basis, const VsStftShape& s, float* scale2, hipStream_t);
void vs_istft_envelope_launch(float* env, const VsStftShape& s, hipStream_t);
void vs_stft_basis_launch(float* basis, const VsStftShape& s, float* scale2, hipStream_t);
void vs_stft_frames_launch(const float* wav, float* frames, const VsStftShape& s, unsigned* amax, unsigned grid, hipStream_t,
                           int zero_pad = 0 /* 1: pad the clip with zeros instead of its reflection */);
void vs_spec_to_reim_launch(const float* a, const float* b, const float* phase, float* reim, const VsStftShape& s, unsigned* amax, unsigned grid,
                            hipStream_t);
void vs_overlap_add_launch(const float* frames, const float* env, float* wav, const VsStftShape& s, hipStream_t);
