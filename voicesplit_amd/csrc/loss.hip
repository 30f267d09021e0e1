// The caller side of the mask during training (train.py:95-108):
//   output = mixed * mask                                            train.py:95
//   wav    = ap.torch_inv_spectrogram(output, spec_phase)            utils/audio_processor.py:498-509
//   loss   = SiSNR_With_Pit()(wav, target_wav, seq_len)              utils/generic_utils.py:417-474
// computed on the GPU together with d(loss)/d(mask), so that the training step needs no torchaudio
// (torchaudio.functional.istft, which the reference calls, no longer exists) and no autograd graph
// over ~1 GB of waveform-domain intermediates.
//
// The reference's inverse spectrogram, quirks included:
//   S   = (clamp(spec,0,1) - 1) * (-min_level_db) + ref_level_db;   mag = 10^(S/20)
//   re  = mag * exp(cos(phase)),  im = mag * exp(sin(phase))         (":507-509" multiplies by
//         torch.exp of the stacked [cos, sin] -- not mag*cos, mag*sin; reproduced as is)
//   wav = istft(re + i*im, n_fft, hop, win, hann(win, periodic=False), center=True)
// MI355X formulation: the iSTFT is stft.hip's (ONE GEMM against the windowed inverse-DFT basis, then the
// gather-form overlap-add); the backward pass is the transposed GEMM and the same gather, and the
// SI-SNR (one source: PIT is the identity) reduces to six per-utterance moments in fp64.
// Also here: the power-law loss of the voicefilter configuration (vs_powerlaw_loss).
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "stft_common.h"

namespace {

// dframes[m][j] = dwav[b][sp] / env[sp],  sp = hop*t - lead + j  (0 outside the kept samples)
__global__ __launch_bounds__(256)
void overlap_add_bwd_kernel(const float* __restrict__ dwav, const float* __restrict__ env, float* __restrict__ dframes, VsStftShape s,
                            unsigned* __restrict__ amax = nullptr) {
  const long long n = (long long)s.B * s.T * s.win;
  float mx = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.win;
    const int j = (int)(i - m * s.win);
    const int b = (int)(m / s.T), t = (int)(m - (long long)b * s.T);
    const int sp = s.hop * t - s.lead + j;
    const float v = (sp >= 0 && sp < s.S) ? dwav[(size_t)b * s.S + sp] / env[sp] : 0.f;
    dframes[i] = v;
    mx = fmaxf(mx, fabsf(v));
  }
  vs_absmax_commit(mx, amax);
}

// six fp64 moments per utterance: sum_all s, and over the unmasked samples: n, e, s, e*s, e^2, s^2
__global__ __launch_bounds__(256)
void sisnr_moments_kernel(const float* __restrict__ est, const float* __restrict__ src, const int* __restrict__ len,
                          double* __restrict__ mom /* [B][8] */, VsStftShape s) {
  const int b = blockIdx.y;
  const int L = len ? (len[b] < s.S ? (len[b] > 0 ? len[b] : 0) : s.S) : s.S;
  double a[6] = {0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < s.S; i += gridDim.x * 256) {
    const double e = est[(size_t)b * s.S + i], r = src[(size_t)b * s.S + i];
    a[0] += r;
    if (i < L) { a[1] += e; a[2] += r; a[3] += e * r; a[4] += e * e; a[5] += r * r; }
  }
  __shared__ double red[4][6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_down(a[q], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) red[threadIdx.x >> 6][q] = a[q];
  }
  __syncthreads();
  // one addition per workgroup and moment, its four waves in a fixed order (deterministic mode launches ONE workgroup per utterance:
  // then nothing about the sum depends on arrival order)
  if (threadIdx.x < 6) atomicAdd(&mom[b * 8 + threadIdx.x], (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]));
}

// per utterance: SI-SNR and the three coefficients of d(loss)/d(est[t]) = m_t*(cs*zs_t + ce*ze_t - c0);
// utils/generic_utils.py:437-473 with C = 1 (one source: the permutation search is the identity)
__global__ void sisnr_finalize_kernel(const double* __restrict__ mom, const int* __restrict__ len, float* __restrict__ coef /* [B][8] */,
                                      float* __restrict__ loss, VsStftShape s) {
  __shared__ double acc[64];
  const int tid = threadIdx.x;
  double part = 0.0;
  const double eps = 1e-16;
  for (int b = tid; b < s.B; b += 64) {
    const double nlen = len ? (double)len[b] : (double)s.S;          // num_samples = source_lengths (as given)
    const int Lm_i = len ? (len[b] < s.S ? (len[b] > 0 ? len[b] : 0) : s.S) : s.S;
    const double Lm = Lm_i;                                          // samples the mask keeps
    const double* m = mom + b * 8;
    const double mu_s = m[0] / nlen, mu_e = m[1] / nlen;             // means over ALL samples / num_samples
    const double Sze = m[1] - Lm * mu_e, Szs = m[2] - Lm * mu_s;
    const double dot = m[3] - mu_s * m[1] - mu_e * m[2] + Lm * mu_e * mu_s;
    const double Z = m[5] - 2 * mu_s * m[2] + Lm * mu_s * mu_s;      // sum zs^2
    const double E = m[4] - 2 * mu_e * m[1] + Lm * mu_e * mu_e;      // sum ze^2
    const double es = Z + eps;
    const double P = dot * dot * Z / (es * es);
    const double c = (es + eps) / (es * es);
    const double N = E - c * dot * dot + eps;
    const double snr = P / N;
    part += 10.0 * log10(snr + eps);
    // d l_b / d ze_t = k*( dP_t/N - P/N^2 * dN_t ),  dP_t = 2 dot Z/es^2 * zs_t,  dN_t = 2 ze_t - 2 c dot zs_t
    const double k = 10.0 / (log(10.0) * (snr + eps)) * (-1.0 / s.B);      // loss = 20 - mean_b l_b
    const double gs = k * (2 * dot * Z / (es * es) / N + P / (N * N) * 2 * c * dot);
    const double ge = k * (-P / (N * N) * 2);
    // ze_t = (e_t m_t - mu_e) m_t  ->  d/de_u = m_u ( g_u - sum_t m_t g_t / num_samples )
    const double gsum = gs * Szs + ge * Sze;
    float* o = coef + b * 8;
    o[0] = (float)gs; o[1] = (float)ge; o[2] = (float)(gsum / nlen); o[3] = (float)mu_s; o[4] = (float)mu_e;
    o[5] = (float)Lm_i;
  }
  acc[tid] = part;
  __syncthreads();
  if (tid == 0) {
    double t = 0;
    for (int i = 0; i < 64; ++i) t += acc[i];
    *loss = (float)(20.0 - t / s.B);
  }
}

__global__ __launch_bounds__(256)
void sisnr_grad_kernel(const float* __restrict__ est, const float* __restrict__ src, const float* __restrict__ coef,
                       float* __restrict__ dwav, VsStftShape s) {
  const int b = blockIdx.y;
  const float gs = coef[b * 8], ge = coef[b * 8 + 1], g0 = coef[b * 8 + 2], mu_s = coef[b * 8 + 3], mu_e = coef[b * 8 + 4];
  const int L = (int)coef[b * 8 + 5];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < s.S; i += gridDim.x * 256) {
    float g = 0.f;
    if (i < L) {
      const float zs = src[(size_t)b * s.S + i] - mu_s, ze = est[(size_t)b * s.S + i] - mu_e;
      g = fmaf(gs, zs, fmaf(ge, ze, -g0));
    }
    dwav[(size_t)b * s.S + i] = g;
  }
}

// dmask[i] = mixed[i] * [0 <= v <= 1] * (-min_db) * ln10/20 * mag * (dre*e^{cos} + dim*e^{sin}),  v = mixed*mask
__global__ __launch_bounds__(256)
void reim_to_dmask_kernel(const float* __restrict__ mixed, const float* __restrict__ mask, const float* __restrict__ phase,
                          const float* __restrict__ dreim, float* __restrict__ dmask, VsStftShape s) {
  const long long n = (long long)s.B * s.T * s.F;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long m = i / s.F;
    const int f = (int)(i - m * s.F);
    const float x = mixed[i], v = x * mask[i];
    float g = 0.f;
    if (v >= 0.f && v <= 1.f) {
      const float db = (v - 1.f) * (-s.min_level_db) + s.ref_level_db;
      const float mag = expf(db * kLn10Over20);
      float sn, cs;
      sincosf(phase[i], &sn, &cs);
      const float d = dreim[m * s.ldk + f] * expf(cs) + dreim[m * s.ldk + s.F + f] * expf(sn);
      g = x * (-s.min_level_db) * kLn10Over20 * mag * d;
    }
    dmask[i] = g;
  }
}

// ---- PowerLaw_Compressed_Loss (utils/generic_utils.py:353-373), the criterion train.py:74-75 picks
// for loss_name == 'power_law_compression' (the voicefilter configuration):
//   o = mixed*mask + 1e-16, t = target + 1e-16, po = o^p, pt = t^p
//   loss = mean((|pt| - |po|)^2) + ratio * mean((pt - po)^2)
// One streaming pass: both sums in fp64 (two atomics per workgroup) and, since the gradient needs
// nothing from the reduction but 1/n,
//   dmask = mixed * p*o^(p-1) * ( 2(|po| - |pt|) sign(po) + 2 ratio (po - pt) ) / n
// which is what autograd gives through mul / add / pow / abs / MSELoss.  A negative o makes po NaN,
// as torch.pow does.
__global__ __launch_bounds__(256)
void powerlaw_kernel(const float* __restrict__ mixed, const float* __restrict__ mask, const float* __restrict__ target,
                     long long n, float power, float ratio, double* __restrict__ sums, float* __restrict__ dmask) {
  constexpr float kEps = 1e-16f;
  const float inv_n = (float)(1.0 / (double)n);
  double a0 = 0.0, a1 = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float mx = mixed[i];
    const float o = mx * mask[i] + kEps;
    const float t = target[i] + kEps;
    const float po = powf(o, power), pt = powf(t, power);
    const float ds = fabsf(pt) - fabsf(po), dc = pt - po;
    a0 += (double)(ds * ds);
    a1 += (double)(dc * dc);
    if (dmask) {
      const float sgn = po > 0.f ? 1.f : (po < 0.f ? -1.f : 0.f);
      const float dpo = (-2.f * ds * sgn - 2.f * ratio * dc) * inv_n;
      dmask[i] = mx * (power * powf(o, power - 1.f)) * dpo;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_down(a0, off, 64);
    a1 += __shfl_down(a1, off, 64);
  }
  __shared__ double sh[8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sh[2 * w] = a0; sh[2 * w + 1] = a1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&sums[0], sh[0] + sh[2] + sh[4] + sh[6]);
    atomicAdd(&sums[1], sh[1] + sh[3] + sh[5] + sh[7]);
  }
}

__global__ void powerlaw_finalize_kernel(const double* __restrict__ sums, long long n, float ratio, float* __restrict__ loss) {
  *loss = (float)(sums[0] / (double)n + (double)ratio * (sums[1] / (double)n));
}

}  // namespace

extern "C" {

size_t vs_sisnr_workspace_bytes(const vs_loss_dims* d) {
  VsStftShape s;
  return vs_stft_make_shape(d, &s) ? 0 : vs_stft_layout(s).total;
}

int vs_sisnr_loss(const vs_loss_dims* d, const float* mixed, const float* mask, const float* target, const float* phase,
                  const int* seq_len, void* ws, size_t ws_bytes, float* loss, float* dmask, float* est_wav, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VsStftShape s;
  if (int rc = vs_stft_make_shape(d, &s)) return rc;
  const VsStftLayout L = vs_stft_layout(s);
  VS_REQUIRE(mixed && mask && target && phase && loss, "sisnr_loss: NULL argument");
  if (int rc = vs_stft_check_envelope(s)) return rc;
  VS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total, "sisnr_loss: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  const int M = s.B * s.T;
  const long long nspec = (long long)M * s.F;
  float* basis = at<float>(ws, L.basis);
  float* env = at<float>(ws, L.env);
  // [r6] The three contractions of this head (two iSTFTs, one backward) run as split-f16 products (gemm_f16x3.hip: fp32-class results from
  // the f16 matrix pipe -- 0.31 + 0.32 + 0.23 ms on the fp32 pipe at B = 64 before) whenever the operands fit its
  // 32-bit offsets; their power-of-two operand scales come from |max| values the producing kernels track themselves.
  const bool split = vs_stft_split(s);
  unsigned* amax = at<unsigned>(ws, L.amax);
  float* scales = at<float>(ws, L.scales);
  vs_istft_basis_launch(basis, s, scales + 6, stream);
  vs_istft_envelope_launch(env, s, stream);
  // both spectrograms -> (re | im) rows -> windowed frames (one GEMM each) -> waveforms
  float* reim[2] = {at<float>(ws, L.reim_e), at<float>(ws, L.reim_t)};
  float* frames[2] = {at<float>(ws, L.frames_e), at<float>(ws, L.frames_t)};
  float* wav[2] = {at<float>(ws, L.wav_e), at<float>(ws, L.wav_t)};
  // (the ld padding columns are zeroed by spec_to_reim_kernel itself [r6]: the memset that did it wrote both arrays, 186 MB, for two
  // floats per row)
  if (split) VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)3 * VS_AMAX_SLOTS * 4, stream));
  // with the |max| commit at the end of every wave (a load and maybe an atomic: ~3 us of latency) the grid is ONE resident round of
  // long-lived workgroups -- 16384 short ones paid that latency eight times over (56 -> 100 us per launch, call 13)
  const unsigned cap = split ? 2048 : 16384;
  vs_spec_to_reim_launch(mixed, mask, phase, reim[0], s, split ? amax : nullptr, vs_grid_for(nspec, cap), stream);
  vs_spec_to_reim_launch(target, nullptr, phase, reim[1], s, split ? amax + VS_AMAX_SLOTS : nullptr, vs_grid_for(nspec, cap), stream);
  for (int q = 0; q < 2; ++q) {
    if (split) if (int rc = vs_scale_from_absmax_impl(amax + q * VS_AMAX_SLOTS, VS_AMAX_SLOTS, scales + 2 * q, stream)) return rc;
    if (int rc = vs_stft_contract(split, 0, reim[q], s.ldk, basis, s.ldk, frames[q], s.win, M, s.win, s.K, scales + 2 * q, scales + 6, stream)) return rc;
    vs_overlap_add_launch(frames[q], env, wav[q], s, stream);
  }
  if (est_wav) VS_CHECK_HIP(hipMemcpyAsync(est_wav, wav[0], (size_t)s.B * s.S * 4, hipMemcpyDeviceToDevice, stream));
  // SI-SNR
  double* mom = at<double>(ws, L.mom);
  float* coef = at<float>(ws, L.coef);
  VS_CHECK_HIP(hipMemsetAsync(mom, 0, (size_t)s.B * 8 * 8, stream));
  const int gx = vs_opt(VS_OPT_DETERMINISTIC) ? 1 : (s.S + 256 * 16 - 1) / (256 * 16);
  hipLaunchKernelGGL(sisnr_moments_kernel, dim3(gx, s.B), dim3(256), 0, stream, wav[0], wav[1], seq_len, mom, s);
  hipLaunchKernelGGL(sisnr_finalize_kernel, dim3(1), dim3(64), 0, stream, mom, seq_len, coef, loss, s);
  if (dmask) {
    float* dwav = at<float>(ws, L.dwav);
    hipLaunchKernelGGL(sisnr_grad_kernel, dim3(gx, s.B), dim3(256), 0, stream, wav[0], wav[1], coef, dwav, s);
    float* dframes = frames[0];
    hipLaunchKernelGGL(overlap_add_bwd_kernel, dim3(vs_grid_for((long long)M * s.win, cap)), dim3(256), 0, stream, dwav, env, dframes, s,
                       split ? amax + 2 * VS_AMAX_SLOTS : nullptr);
    float* dreim = reim[0];
    // d(reim)[M][K] = d(frames)[M][win] @ basis[win][K]
    if (split) if (int rc = vs_scale_from_absmax_impl(amax + 2 * VS_AMAX_SLOTS, VS_AMAX_SLOTS, scales + 4, stream)) return rc;
    if (int rc = vs_stft_contract(split, 1, dframes, s.win, basis, s.ldk, dreim, s.ldk, M, s.K, s.win, scales + 4, scales + 6, stream)) return rc;
    hipLaunchKernelGGL(reim_to_dmask_kernel, dim3(vs_grid_for(nspec, 16384)), dim3(256), 0, stream, mixed, mask, phase, dreim, dmask, s);
  }
  VS_LAUNCH_CHECK();
  return 0;
}

int vs_powerlaw_loss(const float* mixed, const float* mask, const float* target, long long n, float power,
                     float complex_loss_ratio, double* scratch, float* loss, float* dmask, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(mixed && mask && target && scratch && loss, "powerlaw_loss: NULL argument");
  VS_REQUIRE(n > 0, "powerlaw_loss: n=%lld", n);
  VS_CHECK_HIP(hipMemsetAsync(scratch, 0, 2 * sizeof(double), stream));
  hipLaunchKernelGGL(powerlaw_kernel, dim3(vs_grid_for(n)), dim3(256), 0, stream, mixed, mask, target, n, power, complex_loss_ratio, scratch, dmask);
  hipLaunchKernelGGL(powerlaw_finalize_kernel, dim3(1), dim3(1), 0, stream, scratch, n, complex_loss_ratio, loss);
  VS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
