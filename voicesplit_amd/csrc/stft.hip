// The short-time transform shared by the training loss (loss.hip), the inference audio legs (audio.hip), Griffin-Lim (griffin_lim.hip)
// and the speaker encoder's log-mel front end (speaker.hip): the kernels more than one of them launches, the shape / workspace /
// envelope helpers and the one contraction call (stft_common.h).
//
// Synthesis: spectrum rows (re | im) @ basis^T -> windowed frames (istft_basis_kernel, ONE GEMM on the matrix cores: 19264 x 1202 x 400
// at B=64), then a gather-form overlap-add (every output sample sums its <= ceil(win/hop) frames and divides by the window envelope).
// Analysis: reflect-padded windowed frames (stft_frames_kernel) @ fbasis^T -> (re | im) rows (stft_basis_kernel).
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "stft_common.h"

namespace {

// basis[j][k]: contribution of spectrum entry k (k < F: Re_k, else Im_{k-F}) to windowed sample j
// of a frame (time index n = (n_fft-win)/2 + j): onesided irfft weights c_k/n_fft, c = 1 for DC and
// Nyquist, 2 otherwise.
// scale2 (or NULL): {s, 1/s} of the split-f16 contractions for this operand, from its analytic bound 2 / n_fft (the rule of
// scale_from_absmax_kernel, conv_f16x3.hip: the bound lands in [2^9, 2^10))
__global__ void istft_basis_kernel(float* __restrict__ basis, VsStftShape s, float* __restrict__ scale2 = nullptr) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && scale2) {
    int e = 0;
    (void)frexpf(2.0f / (float)s.n_fft, &e);
    scale2[0] = ldexpf(1.f, 10 - e);
    scale2[1] = ldexpf(1.f, e - 10);
  }
  if (idx >= s.win * s.ldk) return;
  const int j = idx / s.ldk, k = idx - j * s.ldk;
  float v = 0.f;
  if (k < s.K) {
    const int kk = k < s.F ? k : k - s.F;
    const int n = (s.n_fft - s.win) / 2 + j;
    const int r = (int)(((long long)kk * n) % s.n_fft);          // exact angle reduction
    float sn, cs;
    sincospif(2.0f * (float)r / (float)s.n_fft, &sn, &cs);
    const float c = (kk == 0 || 2 * kk == s.n_fft) ? 1.0f : 2.0f;
    v = (k < s.F ? cs : -sn) * c / (float)s.n_fft * hann_w(j, s);
  }
  basis[idx] = v;
}

// window envelope after centring: env[s'] = sum over frames of win^2 at that sample
__global__ void istft_envelope_kernel(float* __restrict__ env, VsStftShape s) {
  const int sp = blockIdx.x * blockDim.x + threadIdx.x;
  if (sp >= s.S) return;
  const int off = s.lead;                    // sample sp sits at frame-local j = sp - hop*t + off
  float e = 0.f;
  int t_hi = (sp + off) / s.hop;
  if (t_hi > s.T - 1) t_hi = s.T - 1;
  for (int t = t_hi; t >= 0; --t) {
    const int j = sp - s.hop * t + off;
    if (j >= s.win) break;
    const float w = hann_w(j, s);
    e = fmaf(w, w, e);
  }
  env[sp] = e;
}

// reim[m][k] = mag * exp(cos phi) (k < F) | mag * exp(sin phi) (k >= F);  v = a*b (mixed*mask) or a
__global__ __launch_bounds__(256)
void spec_to_reim_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ phase,
                         float* __restrict__ reim, VsStftShape s, unsigned* __restrict__ amax = nullptr) {
  const long long n = (long long)s.B * s.T * s.F;
  float mx = 0.f;      // max |re|, |im| of what this thread wrote: the operand scale of the split-f16 contraction (vs_absmax_commit)
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.F;
    const int f = (int)(i - m * s.F);
    float v = a[i];
    if (b) v *= b[i];
    const float db = (fminf(fmaxf(v, 0.f), 1.f) - 1.f) * (-s.min_level_db) + s.ref_level_db;
    const float mag = expf(db * kLn10Over20);
    float sn, cs;
    sincosf(phase[i], &sn, &cs);
    const float re = s.true_phase ? mag * cs : mag * expf(cs), im = s.true_phase ? mag * sn : mag * expf(sn);
    reim[m * s.ldk + f] = re;
    reim[m * s.ldk + s.F + f] = im;
    if (f == 0) for (int c = s.K; c < s.ldk; ++c) reim[m * s.ldk + c] = 0.f;      // the row's ld padding (a contraction over ldk columns reads it)
    mx = fmaxf(mx, fmaxf(fabsf(re), fabsf(im)));
  }
  vs_absmax_commit(mx, amax);
}

// frames[m][j] = w[j] * wav_reflect[b][hop*t - lead + j]     (librosa.stft: center=True, reflect padding;
// only the win samples under the centred window matter).  The clip ends where it ends: reflection about sample S - 1, and
// S > n_fft / 2 (every caller requires it) makes one reflection enough: the index never leaves [0, S).
// ZERO: librosa's pad_mode='constant' instead (the waveglow Griffin-Lim): a sample outside the clip is 0.
template <bool ZERO>
__global__ __launch_bounds__(256)
void stft_frames_kernel(const float* __restrict__ wav, float* __restrict__ frames, VsStftShape s, unsigned* __restrict__ amax = nullptr) {
  const long long n = (long long)s.B * s.T * s.win;
  float mx = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.win;
    const int j = (int)(i - m * s.win);
    const int b = (int)(m / s.T), t = (int)(m - (long long)b * s.T);
    int idx = s.hop * t - s.lead + j;
    float v;
    if constexpr (ZERO) {
      v = (idx < 0 || idx >= s.S) ? 0.f : hann_w(j, s) * wav[(size_t)b * s.S + idx];
    } else {
      if (idx < 0) idx = -idx;
      if (idx >= s.S) idx = 2 * (s.S - 1) - idx;
      v = hann_w(j, s) * wav[(size_t)b * s.S + idx];
    }
    frames[i] = v;
    mx = fmaxf(mx, fabsf(v));
  }
  vs_absmax_commit(mx, amax);
}

// fwd_basis[k][j]: Re_k = sum_j x_j cos(2 pi k n_j / N), Im_k = -sum_j x_j sin(...), n_j = (N-win)/2 + j
__global__ void stft_basis_kernel(float* __restrict__ basis, VsStftShape s, float* __restrict__ scale2 = nullptr) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && scale2) { scale2[0] = 512.f; scale2[1] = 1.f / 512.f; }      // |cos|, |sin| <= 1 = 0.5 * 2^1 -> 2^(10 - 1) (scale_from_absmax_kernel's rule)
  if (idx >= s.K * s.win) return;
  const int k = idx / s.win, j = idx - k * s.win;
  const int kk = k < s.F ? k : k - s.F;
  const int n = (s.n_fft - s.win) / 2 + j;
  const int r = (int)(((long long)kk * n) % s.n_fft);
  float sn, cs;
  sincospif(2.0f * (float)r / (float)s.n_fft, &sn, &cs);
  basis[idx] = k < s.F ? cs : -sn;
}

// wav[b][sp] = (sum_t frames[b*T+t][sp - hop*t + lead]) / env[sp]
__global__ __launch_bounds__(256)
void overlap_add_kernel(const float* __restrict__ frames, const float* __restrict__ env, float* __restrict__ wav, VsStftShape s) {
  const int sp = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (sp >= s.S) return;
  wav[(size_t)b * s.S + sp] = stft_gather(frames, b, sp, s) / env[sp];
}

}  // namespace

void vs_istft_basis_launch(float* basis, const VsStftShape& s, float* scale2, hipStream_t stream) {
  hipLaunchKernelGGL(istft_basis_kernel, dim3((s.win * s.ldk + 255) / 256), dim3(256), 0, stream, basis, s, scale2);
}
void vs_istft_envelope_launch(float* env, const VsStftShape& s, hipStream_t stream) {
  hipLaunchKernelGGL(istft_envelope_kernel, dim3((s.S + 255) / 256), dim3(256), 0, stream, env, s);
}
void vs_stft_basis_launch(float* basis, const VsStftShape& s, float* scale2, hipStream_t stream) {
  hipLaunchKernelGGL(stft_basis_kernel, dim3((s.K * s.win + 255) / 256), dim3(256), 0, stream, basis, s, scale2);
}
void vs_stft_frames_launch(const float* wav, float* frames, const VsStftShape& s, unsigned* amax, unsigned grid, hipStream_t stream, int zero_pad) {
  if (zero_pad) hipLaunchKernelGGL(stft_frames_kernel<true>, dim3(grid), dim3(256), 0, stream, wav, frames, s, amax);
  else hipLaunchKernelGGL(stft_frames_kernel<false>, dim3(grid), dim3(256), 0, stream, wav, frames, s, amax);
}
void vs_spec_to_reim_launch(const float* a, const float* b, const float* phase, float* reim, const VsStftShape& s, unsigned* amax, unsigned grid,
                            hipStream_t stream) {
  hipLaunchKernelGGL(spec_to_reim_kernel, dim3(grid), dim3(256), 0, stream, a, b, phase, reim, s, amax);
}
void vs_overlap_add_launch(const float* frames, const float* env, float* wav, const VsStftShape& s, hipStream_t stream) {
  hipLaunchKernelGGL(overlap_add_kernel, dim3((s.S + 255) / 256, s.B), dim3(256), 0, stream, frames, env, wav, s);
}

void vs_stft_fill_shape(const vs_loss_dims* d, int B, int T, int S, VsStftShape* s) {
  s->B = B; s->T = T; s->F = d->F; s->n_fft = d->n_fft; s->hop = d->hop; s->win = d->win;
  s->S = S;
  s->lead = d->n_fft / 2 - (d->n_fft - d->win) / 2;
  s->K = 2 * d->F;
  s->ldk = (s->K + 3) & ~3;
  s->min_level_db = d->min_level_db; s->ref_level_db = d->ref_level_db;
  s->periodic = 0; s->true_phase = 0;
}

int vs_stft_make_shape(const vs_loss_dims* d, VsStftShape* s) {
  VS_REQUIRE(d != nullptr, "loss dims is NULL");
  VS_REQUIRE(d->B > 0 && d->T > 1 && d->F > 1 && d->hop > 0 && d->win > 0, "loss: bad dims B=%d T=%d F=%d hop=%d win=%d", d->B, d->T, d->F, d->hop, d->win);
  VS_REQUIRE(d->n_fft == 2 * (d->F - 1), "loss: num_freq F=%d must be n_fft/2+1 (n_fft=%d)", d->F, d->n_fft);
  VS_REQUIRE(d->win <= d->n_fft && d->hop <= d->win, "loss: need hop <= win <= n_fft");
  VS_REQUIRE(d->B <= 65535, "loss: B too large");
  vs_stft_fill_shape(d, d->B, d->T, d->hop * (d->T - 1), s);
  return 0;
}

VsStftLayout vs_stft_layout(const VsStftShape& s) {
  VsStftLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  const size_t M = (size_t)s.B * s.T;
  L.basis = take((size_t)s.win * s.ldk * 4);
  L.fbasis = take((size_t)s.K * s.win * 4);     // analysis basis [K][win] (vs_wav_to_spec)
  L.env = take((size_t)s.S * 4);
  L.reim_e = take(M * s.ldk * 4);       // later reused for d(reim)
  L.reim_t = take(M * s.ldk * 4);
  L.frames_e = take(M * s.win * 4);     // later reused for d(frames)
  L.frames_t = take(M * s.win * 4);
  L.wav_e = take((size_t)s.B * s.S * 4);
  L.wav_t = take((size_t)s.B * s.S * 4);
  L.dwav = take((size_t)s.B * s.S * 4);
  L.mom = take((size_t)s.B * 8 * 8);
  L.coef = take((size_t)s.B * 8 * 4);
  L.amax = take((size_t)3 * VS_AMAX_SLOTS * 4);      // running |max| of the three fp32 operands of the split-f16 contractions (vs_sisnr_loss)
  L.scales = take(4 * 2 * 4);                        // {s, 1/s}: reim (estimate), reim (target), d(frames), basis
  L.total = off;
  return L;
}

// The overlap-add divides by the window envelope.  With little or no overlap (hop close to win) a Hann
// window leaves samples whose envelope is 0 (w[0] = 0, and w[win-1] = 0 for the non-periodic form):
// torchaudio.functional.istft asserts `window_envelop.abs().min() > 1e-11` there and librosa only
// divides where the envelope exceeds tiny -- refuse such configurations instead of emitting inf/nan.
// Same formula as istft_envelope_kernel, evaluated on the host (first / last window and one steady
// period are enough: the envelope is hop-periodic in between); cached for the last shape seen.
int vs_stft_check_envelope(const VsStftShape& s) {
  static thread_local int c_key[5] = {0, 0, 0, 0, 0};
  static thread_local double c_min = 0.0;
  const int key[5] = {s.hop, s.win, s.T, s.periodic, 1};
  bool hit = true;
  for (int i = 0; i < 5; ++i) hit = hit && key[i] == c_key[i];
  if (!hit) {
    const int off = s.lead, den = s.periodic ? s.win : s.win - 1;
    auto env_at = [&](int sp) {
      double e = 0.0;
      int t_hi = (sp + off) / s.hop;
      if (t_hi > s.T - 1) t_hi = s.T - 1;
      for (int t = t_hi; t >= 0; --t) {
        const int j = sp - s.hop * t + off;
        if (j >= s.win) break;
        const double w = den > 0 ? 0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * (double)j / (double)den) : 1.0;
        e += w * w;
      }
      return e;
    };
    double mn = 1e300;
    const int span = s.win + s.hop;
    for (int sp = 0; sp < s.S; ++sp) {
      if (sp >= span && sp < s.S - span) { sp = s.S - span - 1; continue; }
      const double e = env_at(sp);
      if (e < mn) mn = e;
    }
    c_min = mn;
    for (int i = 0; i < 5; ++i) c_key[i] = key[i];
  }
  VS_REQUIRE(c_min > 1e-11, "istft: window envelope reaches %.3g (hop=%d win=%d %s Hann): the overlap-add would divide by zero; "
             "use hop <= win/2", c_min, s.hop, s.win, s.periodic ? "periodic" : "symmetric");
  return 0;
}

int vs_stft_contract(bool split, int layout_w, const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                     const float* a_scale2, const float* w_scale2, hipStream_t stream) {
  VsGemm g{.A = A, .lda = lda, .W = W, .ldw = ldw, .w_kmajor = layout_w, .C = C, .ldc = ldc, .M = M, .N = N, .K = K};
  if (split) {
    g.arith = VS_GEMM_SPLIT_F16;
    g.K = lda;      // the split kernel contracts over the whole zero-padded rows
    g.a_scale2 = a_scale2;
    g.w_scale2 = w_scale2;
  }
  return vs_gemm_impl(g, stream);
}
