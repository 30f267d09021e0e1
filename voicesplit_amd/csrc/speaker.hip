// GE2E speaker encoder, inference only: reference audio -> 256-d d-vector (the `dvec` every other path of this library takes).
// What the reference runs in notebooks/GE2E-Seungwonpark-ExtractSpeakerEmbedding-...py with ap.get_mel
// (utils/audio_processor.py:460-467) in front:
//   mel  = log10(mel_basis @ |stft(wav, n_fft 1200, hop 160, win 400, hann, center, reflect)|^2 + 1e-6)        [n_mels][T]
//   x    = nn.LSTM(n_mels -> H, layers)(mel.unfold(1, window, stride))[:, -1, :]                               [N][H]
//   p    = Linear(H -> E)(x);  dvec = mean over the utterance's windows of p / |p|_2
//
// Front end: the STFT is stft.hip's, the kernels vs_wav_to_spec launches (frames, split-f16 GEMM against the windowed DFT basis), on a
// shape of one clip with reflection at the clip's TRUE end (any n > n_fft / 2); then a power epilogue, the F -> n_mels contraction and the log.
//
// Recurrence (the hot path): the batch is the number of windows N (6 for a 3 s clip, ~1000 for a preprocessing batch), H = 768,
// three stacked layers, 80 steps.  Schedule: a WAVEFRONT of window + layers - 1 ticks; at tick d layer l runs its step t = d - l
// (it needs layer l-1 at step t and itself at step t-1: both finished at tick d-1).  One launch per tick covers every active layer
// (grid.z), so there are window + layers - 1 = 82 launches where a layer-by-layer schedule has 240, and no device-wide barrier and
// no spin anywhere: the stream order between two ticks is the only synchronisation (nothing persistent, nothing to poison).
// A workgroup is four waves = four blocks of 32 windows; a wave owns 32 windows x 32 hidden units x the four gates (four 32x32
// accumulators fed by ONE A fragment), K = [h_{l-1,t} | h_{l,t-1}] walked in 16-wide chunks in an order that does not depend on N:
// a window's result is bitwise the same in every batch.  Operands go straight from L2 into the MFMA fragment registers (the weights
// are packed in fragment order: 16 contiguous bytes per lane), the four waves of a workgroup read the same weight lines.
// The layer-0 input projection W_ih0 @ mel is computed ONCE PER FRAME for the whole mel (overlapping windows share it).
// VS_MATH_F16X3: h (|h| < 1, exchanged as f16 hi + lo of h * 2^10) and the weights (scaled by the power of two that puts max|W| of the
// layer into [2^9, 2^10)) as split-f16, three products, fp32 accumulate; VS_MATH_FP32: a plain fp32 FMA step kernel (cross-check arm).
#include <math.h>

#include "../../include/voicesplit_hip.h"
#include "stft_common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int kMaxLayers = 4;
constexpr float kHScale = 1024.f;      // h is exchanged as f16(h * 2^10) + f16(remainder), as in lstm_fwd.hip

struct SpkShape {
  int M, H, L, E, W, S, math;
  int Hk;      // H rounded up to the 16-wide K chunk of the f16 MFMA
  int nub;     // blocks of 32 hidden units
};

int make_shape(const vs_speaker_dims* d, SpkShape* s) {
  VS_REQUIRE(d != nullptr, "speaker: dims is NULL");
  VS_REQUIRE(d->n_mels > 0 && d->hidden > 0 && d->emb > 0, "speaker: n_mels=%d hidden=%d emb=%d must be positive", d->n_mels, d->hidden, d->emb);
  VS_REQUIRE(d->n_mels <= 4096 && d->hidden <= 8192 && d->emb <= 8192, "speaker: n_mels=%d hidden=%d emb=%d too large", d->n_mels, d->hidden, d->emb);
  VS_REQUIRE(d->hidden % 8 == 0, "speaker: hidden H=%d must be a multiple of 8", d->hidden);
  VS_REQUIRE(d->layers >= 1 && d->layers <= kMaxLayers, "speaker: layers=%d (1 .. %d)", d->layers, kMaxLayers);
  VS_REQUIRE(d->window >= 1 && d->window <= 65536, "speaker: window=%d must be >= 1", d->window);
  VS_REQUIRE(d->stride >= 1, "speaker: stride=%d must be >= 1", d->stride);
  VS_REQUIRE(d->math == VS_MATH_FP32 || d->math == VS_MATH_F16X3 || d->math == VS_MATH_BF16, "speaker: unknown math %d", d->math);
  VS_REQUIRE(d->math != VS_MATH_BF16, "speaker: VS_MATH_BF16 (single-product f16) is not built for the speaker encoder; use VS_MATH_F16X3 or VS_MATH_FP32");
  s->M = d->n_mels; s->H = d->hidden; s->L = d->layers; s->E = d->emb; s->W = d->window; s->S = d->stride; s->math = d->math;
  s->Hk = (s->H + 15) / 16 * 16;
  s->nub = (s->H + 31) / 32;
  return 0;
}

// ---- prepared weights ------------------------------------------------------------------------------------------------------
// header (64 floats): [l] uint bit pattern of max|W| of layer l's [W_ih | W_hh] (layer 0: W_hh), [8 + 2l] = {s, 1/s} of that layer
// w_ih0 [4H][M], bias [L][4H] (b_ih + b_hh), proj_w [E][H], proj_b [E]: fp32 copies (the embed call takes no parameter pointers)
// per layer: VS_MATH_F16X3: hi and lo planes in fragment order [unit block][K chunk][gate][lane][8]; VS_MATH_FP32: [4H][Kl] fp32
struct PrepLayout { size_t header, wih0, bias, proj_w, proj_b, w[kMaxLayers], wlo[kMaxLayers], total; };

inline int layer_k(const SpkShape& s, int l) { return s.math == VS_MATH_F16X3 ? (l ? 2 * s.Hk : s.Hk) : (l ? 2 * s.H : s.H); }

void prep_layout(const SpkShape& s, PrepLayout* P) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  P->header = take(64 * 4);
  P->wih0 = take((size_t)4 * s.H * s.M * 4);
  P->bias = take((size_t)s.L * 4 * s.H * 4);
  P->proj_w = take((size_t)s.E * s.H * 4);
  P->proj_b = take((size_t)s.E * 4);
  for (int l = 0; l < kMaxLayers; ++l) {
    P->w[l] = P->wlo[l] = 0;
    if (l >= s.L) continue;
    if (s.math == VS_MATH_F16X3) {
      const size_t plane = (size_t)s.nub * (layer_k(s, l) / 16) * 4 * 64 * 8 * 2;
      P->w[l] = take(plane);
      P->wlo[l] = take(plane);
    } else {
      P->w[l] = take((size_t)4 * s.H * layer_k(s, l) * 4);
    }
  }
  P->total = off;
}

__global__ __launch_bounds__(256)
void spk_absmax_kernel(const float* __restrict__ a, long long na, const float* __restrict__ b, long long nb, unsigned* __restrict__ out) {
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256)
    m = fmaxf(m, fabsf(i < na ? a[i] : b[i - na]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
}

// {s, 1/s}: the power of two that maps max|W| into [2^9, 2^10) (the rule of the other split-f16 operands); all-zero weights: 1
__global__ void spk_scale_kernel(float* __restrict__ header, int L) {
  const int l = threadIdx.x;
  if (l >= L) return;
  const float m = __uint_as_float(reinterpret_cast<const unsigned*>(header)[l]);
  int e = 0;
  float sc = 1.f, inv = 1.f;
  if (m > 0.f && m < 3.0e38f) {
    (void)frexpf(m, &e);                 // m = f * 2^e, f in [0.5, 1)
    e = 10 - e;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    sc = ldexpf(1.f, e);
    inv = ldexpf(1.f, -e);
  }
  header[8 + 2 * l] = sc;
  header[9 + 2 * l] = inv;
}

__global__ __launch_bounds__(256)
void spk_copy_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = b ? a[i] + b[i] : a[i];
}

// element k of layer l's concatenated K axis for gate row `row`: [W_ih (layers > 0) | W_hh], each part padded to Hp columns
__device__ __forceinline__ float spk_w_at(const float* __restrict__ w_ih, const float* __restrict__ w_hh, int H, int Hp, int row, int k) {
  if (w_ih) {
    if (k < Hp) return k < H ? w_ih[(size_t)row * H + k] : 0.f;
    k -= Hp;
  }
  return k < H ? w_hh[(size_t)row * H + k] : 0.f;
}

// fragment order of the B operand of v_mfma_f32_32x32x16_f16: lane holds B[k = 16 kc + 8 (lane >> 5) + j][column = lane & 31], j = 0..7
__global__ __launch_bounds__(256)
void spk_pack_f16_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ scale2,
                         _Float16* __restrict__ hi, _Float16* __restrict__ lo, int H, int Hk, int nkc, long long total) {
  const float sc = scale2[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63), g = (int)((i >> 9) & 3);
    const long long rest = i >> 11;
    const int kc = (int)(rest % nkc), ub = (int)(rest / nkc);
    const int unit = ub * 32 + (lane & 31), k = kc * 16 + 8 * (lane >> 5) + j;
    float v = 0.f;
    if (unit < H) v = spk_w_at(w_ih, w_hh, H, Hk, g * H + unit, k) * sc;
    const _Float16 h = (_Float16)v;
    hi[i] = h;
    lo[i] = (_Float16)(v - (float)h);
  }
}

__global__ __launch_bounds__(256)
void spk_pack_f32_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, float* __restrict__ out, int H, int Kl, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int row = (int)(i / Kl), k = (int)(i - (long long)row * Kl);
    out[i] = spk_w_at(w_ih, w_hh, H, H, row, k);
  }
}

// ---- workspace of vs_speaker_embed --------------------------------------------------------------------------------------------
struct WsLayout { size_t xproj, win_frame, state, state_bytes, hA, hB, c, h_last, proj, total; };

void ws_layout(const SpkShape& s, long long N, long long frames, WsLayout* Wl) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  Wl->xproj = take((size_t)frames * 4 * s.H * 4);
  Wl->win_frame = take((size_t)N * 4);
  Wl->state = off;
  if (s.math == VS_MATH_F16X3) {
    Wl->hA = take((size_t)s.L * 2 * N * s.Hk * 2);      // hi planes [L][2 parities][N][Hk] f16
    Wl->hB = take((size_t)s.L * 2 * N * s.Hk * 2);      // lo planes
  } else {
    Wl->hA = take((size_t)s.L * 2 * N * s.H * 4);       // h [L][2][N][H] fp32
    Wl->hB = Wl->hA;
  }
  Wl->c = take((size_t)s.L * N * s.H * 4);
  Wl->state_bytes = off - Wl->state;
  Wl->h_last = take((size_t)N * s.H * 4);
  Wl->proj = take((size_t)N * s.E * 4);
  Wl->total = off;
}

// first frame of every window: window n of utterance u starts at utt_frames[u] + (n - utt_windows[u]) * stride
__global__ void spk_window_frames_kernel(const int* __restrict__ utt_frames, const int* __restrict__ utt_windows, int U, int N, int stride,
                                         int window, int frames, int* __restrict__ win_frame) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int lo = 0, hi = U - 1;                    // last u with utt_windows[u] <= n
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (utt_windows[mid] <= n) lo = mid; else hi = mid - 1;
  }
  long long f = (long long)utt_frames[lo] + (long long)(n - utt_windows[lo]) * stride;
  const long long fmax = (long long)frames - window;      // offsets are the caller's: keep every read inside the mel whatever they say
  f = f < 0 ? 0 : (f > fmax ? fmax : f);
  win_frame[n] = (int)f;
}

struct StepArgs {
  const _Float16* wh[kMaxLayers];
  const _Float16* wl[kMaxLayers];
  const float* wf[kMaxLayers];       // VS_MATH_FP32: [4H][Kl]
  const float* header;
  const float* bias;                 // [L][4H]
  const float* xproj;                // [frames][4H], bias of layer 0 included
  const int* win_frame;
  _Float16* hhi; _Float16* hlo;      // [L][2][N][Hk]
  float* hf;                         // VS_MATH_FP32: [L][2][N][H]
  float* c;                          // [L][N][H]
  float* h_last;                     // [N][H]
  int N, H, Hk, L, W;
};

__device__ __forceinline__ float spk_cell(float pi, float pf, float pg, float po, float* __restrict__ c) {
  const float ig = vs_sigmoid_fast(pi), fg = vs_sigmoid_fast(pf), gg = vs_tanh_fast(pg), og = vs_sigmoid_fast(po);
  const float cn = fmaf(fg, *c, ig * gg);
  *c = cn;
  return og * vs_tanh_fast(cn);
}

// One tick of the wavefront, split-f16: blockIdx = (block of 128 windows, block of 32 hidden units, active layer).
__global__ __launch_bounds__(256)
void spk_step_f16x3_kernel(StepArgs a, int tick, int lmin) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int layer = lmin + blockIdx.z;
  const int t = tick - layer;
  const int rb = blockIdx.x * 4 + wave;
  if (rb * 32 >= a.N) return;                          // no barrier below: a wave without rows just leaves
  const int ub = blockIdx.y;
  const int r = lane & 31, hh = lane >> 5;
  const int arow = min(rb * 32 + r, a.N - 1);          // rows past N read a valid row; their results are dropped
  const size_t plane = (size_t)a.N * a.Hk;
  const int nkc1 = a.Hk >> 4, nkc0 = layer ? nkc1 : 0, nkc = nkc0 + nkc1;
  // lower layer at this step (parity t & 1), this layer at the step before (the other parity)
  const size_t off0 = layer ? ((size_t)(layer - 1) * 2 + (t & 1)) * plane : 0;
  const size_t off1 = ((size_t)layer * 2 + ((t + 1) & 1)) * plane;
  const size_t aoff = (size_t)arow * a.Hk + hh * 8;
  const h8* __restrict__ wh = reinterpret_cast<const h8*>(a.wh[layer]) + (size_t)ub * nkc * 256 + lane;
  const h8* __restrict__ wl = reinterpret_cast<const h8*>(a.wl[layer]) + (size_t)ub * nkc * 256 + lane;
  f32x16 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[g][i] = 0.f;
  for (int kc = 0; kc < nkc; ++kc) {
    const size_t src = (kc < nkc0 ? off0 + (size_t)kc * 16 : off1 + (size_t)(kc - nkc0) * 16) + aoff;
    const h8 ah = *reinterpret_cast<const h8*>(a.hhi + src);
    const h8 al = *reinterpret_cast<const h8*>(a.hlo + src);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const h8 bh = wh[(size_t)(kc * 4 + g) * 64];
      const h8 bl = wl[(size_t)(kc * 4 + g) * 64];
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[g], 0, 0, 0);
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[g], 0, 0, 0);
      acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[g], 0, 0, 0);
    }
  }
  const int unit = ub * 32 + r;                        // C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (unit >= a.H) return;
  const float inv = a.header[9 + 2 * layer] * (1.0f / kHScale);
  const int H4 = 4 * a.H;
  const size_t own = ((size_t)layer * 2 + (t & 1)) * plane;
  const bool last = layer == a.L - 1 && t == a.W - 1;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int n = rb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hh;
    if (n >= a.N) continue;
    const float* __restrict__ add = layer ? a.bias + (size_t)layer * H4 : a.xproj + (size_t)(a.win_frame[n] + t) * H4;
    const float h = spk_cell(fmaf(acc[0][reg], inv, add[unit]), fmaf(acc[1][reg], inv, add[a.H + unit]),
                             fmaf(acc[2][reg], inv, add[2 * a.H + unit]), fmaf(acc[3][reg], inv, add[3 * a.H + unit]),
                             a.c + ((size_t)layer * a.N + n) * a.H + unit);
    const float hs = h * kHScale;
    const _Float16 hi = (_Float16)hs;
    a.hhi[own + (size_t)n * a.Hk + unit] = hi;
    a.hlo[own + (size_t)n * a.Hk + unit] = (_Float16)(hs - (float)hi);
    if (last) a.h_last[(size_t)n * a.H + unit] = h;
  }
}

// The same tick in plain fp32 (VS_MATH_FP32, the cross-check arm): one wave per (hidden unit, block of 8 windows, active layer),
// the lanes split K, fp32 FMA chains folded by a fixed shuffle tree.
__global__ __launch_bounds__(64)
void spk_step_fp32_kernel(StepArgs a, int tick, int lmin) {
  const int lane = threadIdx.x;
  const int layer = lmin + blockIdx.z;
  const int t = tick - layer;
  const int unit = blockIdx.x, n0 = blockIdx.y * 8;
  const int H = a.H, K0 = layer ? H : 0, Kl = K0 + H;
  const size_t plane = (size_t)a.N * H;
  const float* __restrict__ x0 = a.hf + (layer ? ((size_t)(layer - 1) * 2 + (t & 1)) * plane : 0);
  const float* __restrict__ x1 = a.hf + ((size_t)layer * 2 + ((t + 1) & 1)) * plane;
  const float* __restrict__ w = a.wf[layer];
  float acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[i][g] = 0.f;
  for (int k = lane; k < Kl; k += 64) {
    float wv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) wv[g] = w[(size_t)(g * H + unit) * Kl + k];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int n = min(n0 + i, a.N - 1);
      const float x = k < K0 ? x0[(size_t)n * H + k] : x1[(size_t)n * H + (k - K0)];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[i][g] = fmaf(wv[g], x, acc[i][g]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[i][g] += __shfl_xor(acc[i][g], o, 64);
  if (lane != 0) return;
  const int H4 = 4 * H;
  const bool last = layer == a.L - 1 && t == a.W - 1;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = n0 + i;
    if (n >= a.N) break;
    const float* __restrict__ add = layer ? a.bias + (size_t)layer * H4 : a.xproj + (size_t)(a.win_frame[n] + t) * H4;
    const float h = spk_cell(acc[i][0] + add[unit], acc[i][1] + add[H + unit], acc[i][2] + add[2 * H + unit], acc[i][3] + add[3 * H + unit],
                             a.c + ((size_t)layer * a.N + n) * H + unit);
    a.hf[((size_t)layer * 2 + (t & 1)) * plane + (size_t)n * H + unit] = h;
    if (last) a.h_last[(size_t)n * H + unit] = h;
  }
}

// dvec[u] = mean over the utterance's windows of proj[n] / |proj[n]|_2   (notebook :83-84; no windows: zeros)
__global__ __launch_bounds__(256)
void spk_pool_kernel(const float* __restrict__ proj, const int* __restrict__ utt_windows, int N, int E, float* __restrict__ dvec) {
  __shared__ float red[4];
  const int u = blockIdx.x;
  int w0 = utt_windows[u], w1 = utt_windows[u + 1];
  w0 = w0 < 0 ? 0 : w0;
  w1 = w1 > N ? N : w1;
  constexpr int PER = 32;                           // E <= 8192
  float acc[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) acc[q] = 0.f;
  for (int n = w0; n < w1; ++n) {
    const float* __restrict__ p = proj + (size_t)n * E;
    float ss = 0.f;
    for (int e = threadIdx.x; e < E; e += 256) ss = fmaf(p[e], p[e], ss);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = threadIdx.x + q * 256;
      if (e < E) acc[q] += p[e] / norm;
    }
  }
  const float cnt = (float)(w1 > w0 ? w1 - w0 : 1);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int e = threadIdx.x + q * 256;
    if (e < E) dvec[(size_t)u * E + e] = acc[q] / cnt;
  }
}

// ---- log-mel front end --------------------------------------------------------------------------------------------------------
struct MelLayout { size_t frames, basis, reim, amax, scales, total; };

// stft_common.h's shape for ONE clip of n samples: T = 1 + n / hop frames, reflection at the clip's true end (S = n), librosa's window
int mel_shape(const vs_loss_dims* d, long long n, int n_mels, VsStftShape* s) {
  VS_REQUIRE(d != nullptr, "wav_to_logmel: dims is NULL");
  VS_REQUIRE(d->F > 1 && d->hop > 0 && d->win > 0, "wav_to_logmel: bad dims F=%d hop=%d win=%d", d->F, d->hop, d->win);
  VS_REQUIRE(d->n_fft == 2 * (d->F - 1), "wav_to_logmel: num_freq F=%d must be n_fft/2+1 (n_fft=%d)", d->F, d->n_fft);
  VS_REQUIRE(d->win <= d->n_fft && d->hop <= d->win, "wav_to_logmel: need hop <= win <= n_fft");
  VS_REQUIRE(d->n_fft <= 65536, "wav_to_logmel: n_fft=%d too large", d->n_fft);
  VS_REQUIRE(n_mels >= 1 && n_mels <= 4096, "wav_to_logmel: n_mels=%d (1 .. 4096)", n_mels);
  VS_REQUIRE(n > d->n_fft / 2, "wav_to_logmel: clip of n=%lld samples is not longer than the reflect padding n_fft/2=%d", n, d->n_fft / 2);
  VS_REQUIRE(n <= (1LL << 28), "wav_to_logmel: n=%lld too large (one call per utterance)", n);
  vs_stft_fill_shape(d, 1, 1 + (int)(n / d->hop), (int)n, s);
  s->periodic = 1;
  return 0;
}

MelLayout mel_layout(const VsStftShape& s) {
  MelLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  L.frames = take((size_t)s.T * s.win * 4);
  L.basis = take((size_t)s.K * s.win * 4);
  L.reim = take((size_t)s.T * s.ldk * 4);
  L.amax = take((size_t)VS_AMAX_SLOTS * 4);
  L.scales = take(8 * 4);
  L.total = off;
  return L;
}

// mel[m][t] = log10(sum_f mel_basis[m][f] (re^2 + im^2) + 1e-6): one workgroup per frame, the power row in LDS, one wave per mel row
__global__ __launch_bounds__(256)
void mel_power_log_kernel(const float* __restrict__ reim, const float* __restrict__ mel_basis, float* __restrict__ mel, VsStftShape s, int n_mels) {
  extern __shared__ float pw[];
  const int t = blockIdx.x;
  const float* __restrict__ row = reim + (size_t)t * s.ldk;
  for (int f = threadIdx.x; f < s.F; f += 256) {
    const float re = row[f], im = row[s.F + f];
    pw[f] = fmaf(re, re, im * im);
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int m = wave; m < n_mels; m += 4) {
    const float* __restrict__ b = mel_basis + (size_t)m * s.F;
    float acc = 0.f;
    for (int f = lane; f < s.F; f += 64) acc = fmaf(b[f], pw[f], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) mel[(size_t)m * s.T + t] = log10f(acc + 1e-6f);
  }
}

}  // namespace

extern "C" {

size_t vs_speaker_prepared_bytes(const vs_speaker_dims* d) {
  SpkShape s;
  if (make_shape(d, &s)) return 0;
  PrepLayout P;
  prep_layout(s, &P);
  return P.total;
}

int vs_speaker_prepare(const vs_speaker_dims* d, const vs_speaker_params* p, void* prepared, size_t prepared_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SpkShape s;
  if (int rc = make_shape(d, &s)) return rc;
  VS_REQUIRE(p && prepared, "speaker_prepare: NULL argument");
  for (int l = 0; l < s.L; ++l)
    VS_REQUIRE(p->w_ih[l] && p->w_hh[l] && p->b_ih[l] && p->b_hh[l], "speaker_prepare: NULL parameter of layer %d", l);
  VS_REQUIRE(p->proj_w && p->proj_b, "speaker_prepare: NULL projection parameter");
  PrepLayout P;
  prep_layout(s, &P);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0 && prepared_bytes >= P.total,
             "speaker_prepare: prepared buffer too small or misaligned (%zu < %zu)", prepared_bytes, P.total);
  float* header = at<float>(prepared, P.header);
  VS_CHECK_HIP(hipMemsetAsync(header, 0, 64 * 4, stream));
  const long long H4 = 4LL * s.H;
  hipLaunchKernelGGL(spk_copy_kernel, dim3(vs_grid_for(H4 * s.M)), dim3(256), 0, stream, p->w_ih[0], (const float*)nullptr, at<float>(prepared, P.wih0), H4 * s.M);
  for (int l = 0; l < s.L; ++l)
    hipLaunchKernelGGL(spk_copy_kernel, dim3(vs_grid_for(H4)), dim3(256), 0, stream, p->b_ih[l], p->b_hh[l], at<float>(prepared, P.bias) + l * H4, H4);
  hipLaunchKernelGGL(spk_copy_kernel, dim3(vs_grid_for((long long)s.E * s.H)), dim3(256), 0, stream, p->proj_w, (const float*)nullptr,
                     at<float>(prepared, P.proj_w), (long long)s.E * s.H);
  hipLaunchKernelGGL(spk_copy_kernel, dim3(vs_grid_for(s.E)), dim3(256), 0, stream, p->proj_b, (const float*)nullptr, at<float>(prepared, P.proj_b), (long long)s.E);
  if (s.math == VS_MATH_F16X3) {
    for (int l = 0; l < s.L; ++l) {
      const long long nhh = H4 * s.H, nih = l ? nhh : 0;
      hipLaunchKernelGGL(spk_absmax_kernel, dim3(vs_grid_for(nhh + nih, 256)), dim3(256), 0, stream, p->w_hh[l], nhh, l ? p->w_ih[l] : p->w_hh[l], nih,
                         reinterpret_cast<unsigned*>(header) + l);
    }
    hipLaunchKernelGGL(spk_scale_kernel, dim3(1), dim3(64), 0, stream, header, s.L);
    for (int l = 0; l < s.L; ++l) {
      const int nkc = layer_k(s, l) / 16;
      const long long total = (long long)s.nub * nkc * 4 * 64 * 8;
      hipLaunchKernelGGL(spk_pack_f16_kernel, dim3(vs_grid_for(total)), dim3(256), 0, stream, l ? p->w_ih[l] : (const float*)nullptr, p->w_hh[l],
                         header + 8 + 2 * l, at<_Float16>(prepared, P.w[l]), at<_Float16>(prepared, P.wlo[l]), s.H, s.Hk, nkc, total);
    }
  } else {
    for (int l = 0; l < s.L; ++l) {
      const int Kl = layer_k(s, l);
      hipLaunchKernelGGL(spk_pack_f32_kernel, dim3(vs_grid_for(H4 * Kl)), dim3(256), 0, stream, l ? p->w_ih[l] : (const float*)nullptr, p->w_hh[l],
                         at<float>(prepared, P.w[l]), s.H, Kl, H4 * Kl);
    }
  }
  VS_LAUNCH_CHECK();
  return 0;
}

size_t vs_speaker_workspace_bytes(const vs_speaker_dims* d, int N, int total_frames) {
  SpkShape s;
  if (make_shape(d, &s)) return 0;
  if (N < 1 || total_frames < s.W || N > (1 << 22) || total_frames > (1 << 26)) {
    vs_set_error("speaker: N=%d windows (1 .. 2^22), total_frames=%d (window=%d .. 2^26)", N, total_frames, s.W);
    return 0;
  }
  WsLayout Wl;
  ws_layout(s, N, total_frames, &Wl);
  return Wl.total;
}

int vs_speaker_embed(const vs_speaker_dims* d, const void* prepared, size_t prepared_bytes, const float* mel, int total_frames,
                     const int* utt_frames, const int* utt_windows, int U, int N, float* h_last, float* proj, float* dvec,
                     void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SpkShape s;
  if (int rc = make_shape(d, &s)) return rc;
  VS_REQUIRE(prepared && mel && utt_frames && utt_windows && ws, "speaker_embed: NULL argument");
  VS_REQUIRE(U >= 1 && U <= (1 << 22), "speaker_embed: U=%d utterances (1 .. 2^22)", U);
  VS_REQUIRE(N >= 1 && N <= (1 << 22), "speaker_embed: N=%d windows (1 .. 2^22)", N);
  VS_REQUIRE(total_frames >= s.W && total_frames <= (1 << 26), "speaker_embed: total_frames=%d (window=%d .. 2^26)", total_frames, s.W);
  PrepLayout P;
  prep_layout(s, &P);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0 && prepared_bytes >= P.total,
             "speaker_embed: prepared buffer too small or misaligned (%zu < %zu)", prepared_bytes, P.total);
  WsLayout Wl;
  ws_layout(s, N, total_frames, &Wl);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= Wl.total,
             "speaker_embed: workspace too small or misaligned (%zu < %zu)", ws_bytes, Wl.total);
  const int H4 = 4 * s.H;
  const float* header = at<float>(prepared, P.header);
  const float* bias = at<float>(prepared, P.bias);
  float* xproj = at<float>(ws, Wl.xproj);
  int* win_frame = at<int>(ws, Wl.win_frame);
  float* hl = h_last ? h_last : at<float>(ws, Wl.h_last);
  float* pj = proj ? proj : at<float>(ws, Wl.proj);
  // zero state: h of step -1, c, and the K padding of the f16 planes (the epilogue never writes it)
  VS_CHECK_HIP(hipMemsetAsync(at<char>(ws, Wl.state), 0, Wl.state_bytes, stream));
  hipLaunchKernelGGL(spk_window_frames_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, utt_frames, utt_windows, U, N, s.S, s.W, total_frames, win_frame);
  // layer-0 input projection, once per frame: xproj[f][4H] = mel[:, f] @ W_ih0^T + b_ih0 + b_hh0 (fp32 matrix pipe; mel is K-major)
  if (int rc = vs_gemm_impl({.A = mel, .lda = total_frames, .a_kmajor = 1, .W = at<float>(prepared, P.wih0), .ldw = s.M, .C = xproj, .ldc = H4,
                             .M = total_frames, .N = H4, .K = s.M, .bias1 = bias}, stream)) return rc;
  StepArgs a;
  for (int l = 0; l < kMaxLayers; ++l) {
    a.wh[l] = l < s.L ? at<_Float16>(prepared, P.w[l]) : nullptr;
    a.wl[l] = l < s.L ? at<_Float16>(prepared, P.wlo[l]) : nullptr;
    a.wf[l] = l < s.L ? at<float>(prepared, P.w[l]) : nullptr;
  }
  a.header = header; a.bias = bias; a.xproj = xproj; a.win_frame = win_frame;
  a.hhi = at<_Float16>(ws, Wl.hA); a.hlo = at<_Float16>(ws, Wl.hB); a.hf = at<float>(ws, Wl.hA);
  a.c = at<float>(ws, Wl.c); a.h_last = hl;
  a.N = N; a.H = s.H; a.Hk = s.Hk; a.L = s.L; a.W = s.W;
  for (int tick = 0; tick < s.W + s.L - 1; ++tick) {
    const int lmin = tick - (s.W - 1) > 0 ? tick - (s.W - 1) : 0;
    const int lmax = tick < s.L - 1 ? tick : s.L - 1;
    if (s.math == VS_MATH_F16X3)
      hipLaunchKernelGGL(spk_step_f16x3_kernel, dim3((N + 127) / 128, s.nub, lmax - lmin + 1), dim3(256), 0, stream, a, tick, lmin);
    else
      hipLaunchKernelGGL(spk_step_fp32_kernel, dim3(s.H, (N + 7) / 8, lmax - lmin + 1), dim3(64), 0, stream, a, tick, lmin);
  }
  VS_LAUNCH_CHECK();
  if (proj || dvec) {
    if (int rc = vs_gemm_impl({.A = hl, .lda = s.H, .W = at<float>(prepared, P.proj_w), .ldw = s.H, .C = pj, .ldc = s.E,
                               .M = N, .N = s.E, .K = s.H, .bias1 = at<float>(prepared, P.proj_b)}, stream)) return rc;
  }
  if (dvec) {
    hipLaunchKernelGGL(spk_pool_kernel, dim3(U), dim3(256), 0, stream, pj, utt_windows, N, s.E, dvec);
    VS_LAUNCH_CHECK();
  }
  return 0;
}

size_t vs_logmel_workspace_bytes(const vs_loss_dims* d, long long n, int n_mels) {
  VsStftShape s;
  return mel_shape(d, n, n_mels, &s) ? 0 : mel_layout(s).total;
}

int vs_wav_to_logmel(const vs_loss_dims* d, const float* wav, long long n, const float* mel_basis, int n_mels, float* mel,
                     void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VsStftShape s;
  if (int rc = mel_shape(d, n, n_mels, &s)) return rc;
  VS_REQUIRE(wav && mel_basis && mel && ws, "wav_to_logmel: NULL argument");
  const MelLayout L = mel_layout(s);
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0 && ws_bytes >= L.total,
             "wav_to_logmel: workspace too small or misaligned (%zu < %zu)", ws_bytes, L.total);
  float* frames = at<float>(ws, L.frames);
  float* basis = at<float>(ws, L.basis);
  float* reim = at<float>(ws, L.reim);
  unsigned* amax = at<unsigned>(ws, L.amax);
  float* scales = at<float>(ws, L.scales);
  VS_CHECK_HIP(hipMemsetAsync(amax, 0, (size_t)VS_AMAX_SLOTS * 4, stream));
  vs_stft_frames_launch(wav, frames, s, amax, vs_grid_for((long long)s.T * s.win), stream);
  vs_stft_basis_launch(basis, s, scales + 2, stream);
  if (int rc = vs_scale_from_absmax_impl(amax, VS_AMAX_SLOTS, scales, stream)) return rc;
  if (int rc = vs_stft_contract(/*split=*/true, 0, frames, s.win, basis, s.win, reim, s.ldk, s.T, s.K, s.win, scales, scales + 2, stream)) return rc;
  hipLaunchKernelGGL(mel_power_log_kernel, dim3(s.T), dim3(256), (size_t)s.F * 4, stream, reim, mel_basis, mel, s, n_mels);
  VS_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
