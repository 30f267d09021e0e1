// Inference orchestration, the twin of train.hip: the workspace and prepared-weights layouts, and the tape-less forward as
// validation plus per-configuration stage functions over one context -- whole path (vs_forward*), stages (vs_conv_stack_fwd*,
// vs_bilstm_fwd*, vs_head_fwd).  Which kernel runs on which buffer, in which order -- no arithmetic lives here.
//
// Reference graph: models/voicesplit/model.py:66-89.
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

typedef VsProfScope ProfScope;

namespace {

constexpr int kConvOut[8] = {64, 64, 64, 64, 64, 64, 64, 8};      // output channels of cnn1 .. cnn8

int check_dims(const vs_dims* d) {
  VS_REQUIRE(d != nullptr, "dims is NULL");
  VS_REQUIRE(d->B > 0 && d->T > 0 && d->F > 0 && d->E > 0 && d->H > 0 && d->FC1 > 0 && d->FC2 > 0,
             "dims must be positive: B=%d T=%d F=%d E=%d H=%d FC1=%d FC2=%d", d->B, d->T, d->F, d->E, d->H, d->FC1, d->FC2);
  VS_REQUIRE(d->H % 8 == 0, "lstm_dim H=%d must be a multiple of 8", d->H);
  VS_REQUIRE(d->math == VS_MATH_FP32 || d->math == VS_MATH_F16X3 || d->math == VS_MATH_BF16, "dims.math=%d is not a VS_MATH_* code", d->math);
  VS_REQUIRE((long long)d->B * d->T < 2147483647LL / 8, "B*T too large");
  return 0;
}

int check_conv_params(const vs_params* p, const char* what) {
  for (int l = 0; l < 8; ++l) {
    const vs_conv_layer& c = p->conv[l];
    VS_REQUIRE(c.weight && c.bias && c.bn_weight && c.bn_bias && c.bn_running_mean && c.bn_running_var,
               "%s: layer %d has a NULL parameter", what, l + 1);
  }
  return 0;
}

// packed weights of mid layer i in whichever form the configuration uses (fp32 MFMA fragments are the largest of the NCHW
// forms; the channels-last split-f16 forward keeps its row norms / scale / per-call plan behind the packed planes)
size_t conv_packed_bytes(int i) {
  const size_t a = vs_conv64_packed_floats(kMid[i].kt, kMid[i].kf) * 4, b = vs_nhwc_f16x3_layer_scratch_bytes(kMid[i].kt, kMid[i].kf);
  return a > b ? a : b;
}

int layout(const vs_dims* d, vs_ws_layout* L) {
  if (int rc = check_dims(d)) return rc;
  const size_t B = d->B, T = d->T, F = d->F, H = d->H;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  L->act0 = take(B * 64 * T * F * 4);
  L->act1 = take(B * 64 * T * F * 4);
  L->feat = take(B * T * 8 * F * 4);
  L->dvbias = take(B * 8 * H * 4);
  L->xg = take(B * T * 8 * H * 4);
  L->lstm_out = take(B * T * 2 * H * 4);
  L->fc1_out = take(B * T * (size_t)d->FC1 * 4);
  for (int i = 0; i < 6; ++i) L->conv_packed[i] = take(conv_packed_bytes(i));
  L->bn_scale = take(8 * 64 * 4);
  L->bn_shift = take(8 * 64 * 4);
  L->bn_stats = take((size_t)VS_BN_STAT_SLOTS * 64 * 2 * 8);    // partial slots of one layer at a time (stream-ordered reuse)
  L->lstm_packed = take(vs_lstm_packed_floats(d->H) * 4);
  L->lstm_state = take(vs_lstm_state_floats(d->B, d->H) * 4);
  L->conv_scales = take(8 * VS_SCALE_SLOT_FLOATS * 4);
  L->gemm_scales = take(16 * 4);
  L->total_bytes = off;
  return 0;
}

int check_ws_pointer(const void* ws) {
  VS_REQUIRE(ws != nullptr, "workspace is NULL");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  return 0;
}

int check_ws(const vs_dims* d, void* ws, size_t ws_bytes, vs_ws_layout* L) {
  if (int rc = layout(d, L)) return rc;
  if (int rc = check_ws_pointer(ws)) return rc;
  VS_REQUIRE(ws_bytes >= L->total_bytes, "workspace too small: %zu < %zu bytes", ws_bytes, L->total_bytes);
  return 0;
}

// ---- several enrolled speakers per mixture: the workspace of vs_workspace_bytes(dims) -- conv buffers, features and the shared gate
// pre-activations G = its xg region, all for B -- followed by what grows with the B*K sequences
struct MultiLayout { vs_ws_layout base; size_t rb, lstm_state, lstm_out, fc1_out, total_bytes; };

int multi_layout(const vs_dims* d, int K, MultiLayout* M) {
  if (int rc = layout(d, &M->base)) return rc;
  VS_REQUIRE(K >= 1, "multi: K=%d speakers per mixture (K >= 1)", K);
  VS_REQUIRE((long long)d->B * K * d->T < 2147483647LL / 8 && (long long)d->B * K <= 65535, "multi: B*K*T too large (B=%d K=%d T=%d)", d->B, K, d->T);
  const size_t N = (size_t)d->B * K, T = d->T, H = d->H;
  size_t off = align_up(M->base.total_bytes);
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  M->rb = take(N * 8 * H * 4);
  M->lstm_state = take(vs_lstm_state_floats((int)N, d->H) * 4);
  M->lstm_out = take(N * T * 2 * H * 4);
  M->fc1_out = take(N * T * (size_t)d->FC1 * 4);
  M->total_bytes = off;
  return 0;
}

int check_multi_ws(const vs_dims* d, int K, void* ws, size_t ws_bytes, MultiLayout* M) {
  if (int rc = multi_layout(d, K, M)) return rc;
  if (int rc = check_ws_pointer(ws)) return rc;
  VS_REQUIRE(ws_bytes >= M->total_bytes, "workspace too small: %zu < %zu bytes (vs_multi_workspace_bytes)", ws_bytes, M->total_bytes);
  return 0;
}

// dvec is [B][K][E]; the row biases and the recurrence's state are sized for the B*K sequences, lstm_out is [B][K][T][2H]
struct MultiBufs { int K; float *rb, *lstm_state, *lstm_out, *fc1_out; };
MultiBufs multi_bufs(void* ws, const MultiLayout& M, int K) {
  return {K, at<float>(ws, M.rb), at<float>(ws, M.lstm_state), at<float>(ws, M.lstm_out), at<float>(ws, M.fc1_out)};
}

// ---- prepared weights (vs_prepare_weights / vs_forward_prepared): everything an eval-mode forward derives from
// the parameters alone -- BatchNorm folded into per-channel scale/shift, conv weights in MFMA fragment order with
// their power-of-two scale, W_ih split into f16 halves with its scale, W_hh in fragment order.  Independent of B, T.
struct PrepLayout {
  size_t bn_scale, bn_shift, conv_packed[6], gemm_wscale, wih_hi, wih_lo, lstm_packed, head_packed, total_bytes;
};
struct Prep {
  float *bn_scale, *bn_shift;
  void* conv_packed[6];
  float* gemm_wscale;     // [8]: scale2 of W_ih at [0..1], |max| scratch at [4]
  _Float16 *wih_hi, *wih_lo;      // VS_MATH_BF16: wih_hi holds W_ih as bf16 rows [8H][Kp] (the B operand of gemm_bf16.hip), wih_lo nothing
  float* lstm_packed;
  void* head_packed;      // VS_MATH_BF16: fc1 / fc2 in the fused head's fragment order (head_fused.hip), else NULL
};

bool head_images_prepared(const vs_dims* d) { return d->math == VS_MATH_BF16 && vs_head_fused_supported(2 * d->H, d->FC1, d->FC2); }

int prep_layout(const vs_dims* d, PrepLayout* L) {
  if (int rc = check_dims(d)) return rc;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  L->bn_scale = take(8 * 64 * 4);
  L->bn_shift = take(8 * 64 * 4);
  for (int i = 0; i < 6; ++i) L->conv_packed[i] = take(conv_packed_bytes(i));
  L->gemm_wscale = take(8 * 4);
  const VsLstmSplitLayout S = vs_lstm_split_layout(0, 8 * d->F, d->H);
  L->wih_hi = take(S.nw);
  L->wih_lo = take(S.nw);
  L->lstm_packed = take(vs_lstm_packed_floats(d->H) * 4);
  L->head_packed = take(head_images_prepared(d) ? vs_head_fused_packed_bytes(2 * d->H, d->FC1, d->FC2) : 0);
  L->total_bytes = off;
  return 0;
}

int prep_pointers(const vs_dims* d, const void* blob, size_t bytes, Prep* P) {
  PrepLayout L;
  if (int rc = prep_layout(d, &L)) return rc;
  VS_REQUIRE(blob != nullptr, "prepared weights: NULL buffer");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(blob) & 255) == 0, "prepared weights: buffer must be 256-byte aligned");
  VS_REQUIRE(bytes >= L.total_bytes, "prepared weights: buffer too small: %zu < %zu bytes", bytes, L.total_bytes);
  void* b = const_cast<void*>(blob);
  P->bn_scale = at<float>(b, L.bn_scale);
  P->bn_shift = at<float>(b, L.bn_shift);
  for (int i = 0; i < 6; ++i) P->conv_packed[i] = at<char>(b, L.conv_packed[i]);
  P->gemm_wscale = at<float>(b, L.gemm_wscale);
  P->wih_hi = at<_Float16>(b, L.wih_hi);
  P->wih_lo = at<_Float16>(b, L.wih_lo);
  P->lstm_packed = at<float>(b, L.lstm_packed);
  P->head_packed = head_images_prepared(d) ? at<void>(b, L.head_packed) : nullptr;
  return 0;
}

}  // namespace

int vs_check_dims_impl(const vs_dims* d) { return check_dims(d); }

// ---- pieces of the schedule that the training forward (train.hip) shares ----
int vs_conv64_layer_impl(int math, const float* in, const float* w, void* packed, float* scales8 /* one scale slot */, int in_amax_ready,
                         const float* scale, const float* shift, float* out, int B, int T, int F, int KT, int KF,
                         int dil, int act, int transpose_flip, unsigned* amax_out, hipStream_t stream, double* bn_stats) {
  VS_REQUIRE(math == VS_MATH_FP32 || math == VS_MATH_F16X3,
             "conv64 layer: math=%d has no NCHW kernels (the bf16 arithmetic is channels-last)", math);
  if (math == VS_MATH_F16X3) {     // power-of-two operand scales, packed hi / lo weight image
    if (in_amax_ready) {
      if (int rc = vs_scale_from_absmax_impl(vs_amax_slot(scales8), VS_AMAX_SLOTS, scales8, stream)) return rc;
    } else {
      if (int rc = vs_pow2_scale_impl(in, (long long)B * 64 * T * F, vs_amax_slot(scales8), scales8, stream)) return rc;
    }
    if (int rc = vs_conv64_pack_f16_impl(w, static_cast<_Float16*>(packed), KT, KF, transpose_flip,
                                         reinterpret_cast<unsigned*>(scales8 + 4), scales8 + 2, stream)) return rc;
    return vs_conv64_f16x3_fwd_impl(in, static_cast<const _Float16*>(packed), scale, shift, scales8, scales8 + 2, out,
                                    B, T, F, KT, KF, dil, act, amax_out, stream, bn_stats);
  }
  VS_REQUIRE(bn_stats == nullptr, "conv64 layer: fused BatchNorm statistics are not offered by the fp32 kernels");
  if (int rc = vs_conv64_pack_impl(w, static_cast<float*>(packed), KT, KF, transpose_flip, stream)) return rc;
  return vs_conv64_fwd_impl(in, static_cast<const float*>(packed), scale, shift, out, B, T, F, KT, KF, dil, act, stream);
}

// the split-f16 / bf16 image of W_ih[:, :K] of both directions: scale2 (2 floats), then hi and lo halves [8H][Kp]
int vs_lstm_split_wih_impl(int math, const float* w_ih0, const float* w_ih1, int H, int K, int KE, unsigned* amax1,
                           float* w_scale2, _Float16* Wh, _Float16* Wl, hipStream_t stream) {
  const size_t dir1 = (size_t)4 * H * vs_lstm_split_layout(0, K, H).Kp;
  VS_CHECK_HIP(hipMemsetAsync(amax1, 0, sizeof(unsigned), stream));
  if (int rc = vs_absmax_accum_impl(w_ih0, (long long)4 * H * KE, amax1, stream)) return rc;
  if (int rc = vs_absmax_accum_impl(w_ih1, (long long)4 * H * KE, amax1, stream)) return rc;
  if (int rc = vs_scale_from_absmax_impl(amax1, 1, w_scale2, stream)) return rc;
  if (!Wh) return 0;
  if (int rc = vs_split_rows_impl(w_ih0, 4 * H, K, KE, w_scale2, Wh, Wl, 0, stream, math)) return rc;
  return vs_split_rows_impl(w_ih1, 4 * H, K, KE, w_scale2, Wh + dir1, Wl + dir1, 0, stream, math);
}

bool vs_lstm_rows_fit(int M, int K, int H, const void* scratch, size_t scratch_bytes, bool prepared) {
  const VsLstmSplitLayout S = vs_lstm_split_layout(M, K, H);
  if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 255) != 0) return false;
  if (prepared) return S.Wh <= scratch_bytes;
  return scratch_bytes >= vs_gemm_presplit_bytes(M, 8 * H, K) && S.Wl + S.nw <= scratch_bytes;
}

// scratch: any idle device buffer (the conv activation ping-pong in inference, a gradient buffer in
// training).  When it can hold both operands split into f16 hi/lo arrays (vs_lstm_rows_fit),
// the split is a pass of its own and the GEMM streams halves; otherwise (tiny batches: the split
// weights alone are 62 MB) the GEMM converts fp32 tiles while it stages them.
int vs_lstm_input_gemm_impl(int math, const float* feat, int K, const float* w_ih0, const float* w_ih1, int H, int KE,
                            float* xg, int M, const float* rowbias, int T, float* gs, void* scratch, size_t scratch_bytes,
                            hipStream_t stream, const VsLstmGemmReady& ready) {
  char* base = static_cast<char*>(scratch);
  // the bf16 configuration's own GEMM (gemm_bf16.hip): feat and W_ih as bf16 arrays that the backward pass reuses.  It needs
  // room for the bf16 copy of feat, and for the bf16 W_ih unless that arrives prepared (vs_prepare_weights keeps it in the
  // prepared blob): a B = 1 clip of a second has room for the first but not for the 31 MB of the second.
  const VsLstmBf16Layout Lb = vs_lstm_bf16_layout(M, K, H);
  if (math == VS_MATH_BF16 && scratch && (reinterpret_cast<uintptr_t>(scratch) & 255) == 0 &&
      scratch_bytes >= (ready.wh ? Lb.wih : Lb.dxg)) {
    if (!ready.feat_bf16) {      // (the training forward's BatchNorm apply of cnn8 writes it itself)
      if (int rc = vs_cvt_rows_bf16_impl(feat, M, K, K, base + Lb.feat, Lb.Kp, stream)) return rc;
    }
    if (!ready.wh) {      // (prepared weights: the bf16 W_ih lives in the prepared blob)
      if (int rc = vs_cvt_rows_bf16_impl(w_ih0, 4 * H, K, KE, base + Lb.wih, Lb.Kp, stream)) return rc;
      if (int rc = vs_cvt_rows_bf16_impl(w_ih1, 4 * H, K, KE, base + Lb.wih + (size_t)4 * H * Lb.Kp * 2, Lb.Kp, stream)) return rc;
    }
    const void* wih = ready.wh ? static_cast<const void*>(ready.wh) : static_cast<const void*>(base + Lb.wih);
    return vs_gemm_bf16_impl({.A = base + Lb.feat, .lda = Lb.Kp, .B = wih, .ldb = Lb.Kp, .C = xg, .ldc = 8 * H, .M = M, .N = 8 * H, .K = K,
                              .rowbias = rowbias, .ldrb = 8 * H, .group = T}, stream);
  }
  // x @ [W_ih; W_ih_reverse]^T converted from the fp32 tensors while staged: the fp32 kernel, or the split kernel with the scales below
  VsGemm xw{.A = feat, .lda = K, .W = w_ih0, .ldw = KE, .W_hi = w_ih1, .n_split = 4 * H, .C = xg, .ldc = 8 * H, .M = M, .N = 8 * H, .K = K,
            .rowbias = rowbias, .ldrb = 8 * H, .group = T};
  if (math == VS_MATH_FP32) return vs_gemm_impl(xw, stream);
  // VS_MATH_BF16 without room for the bf16 operand copies: the split-operand GEMM re-derives its operands from the fp32 tensors.  A
  // prepared blob of this arithmetic holds W_ih as bf16 bits (no f16 halves, no scale) -- never to be read as the split form.
  const bool prepared = ready.wscale2 != nullptr && math != VS_MATH_BF16;
  const VsLstmSplitLayout S = vs_lstm_split_layout(M, K, H);
  const bool presplit = vs_lstm_rows_fit(M, K, H, scratch, scratch_bytes, prepared);
  VS_REQUIRE(!ready.feat_rows || (math == VS_MATH_F16X3 && presplit), "lstm input gemm: the split feature rows were announced but do not fit");
  unsigned* amax = reinterpret_cast<unsigned*>(gs + 4);
  if (!ready.feat_rows) { if (int rc = vs_pow2_scale_impl(feat, (long long)M * K, amax, gs, stream)) return rc; }
  // (addresses only: without a scratch that fits, !presplit, none of the four is handed to a kernel)
  _Float16 *Ah = reinterpret_cast<_Float16*>(base + S.Ah), *Al = reinterpret_cast<_Float16*>(base + S.Al);
  _Float16 *Wh = reinterpret_cast<_Float16*>(base + S.Wh), *Wl = reinterpret_cast<_Float16*>(base + S.Wl);
  const float* wscale2 = prepared ? ready.wscale2 : gs + 2;
  if (!prepared) {
    if (int rc = vs_lstm_split_wih_impl(math, w_ih0, w_ih1, H, K, KE, amax + 1, gs + 2, presplit ? Wh : nullptr, Wl, stream)) return rc;
  }
  if (!presplit) {
    xw.arith = math == VS_MATH_BF16 ? VS_GEMM_SPLIT_BF16 : VS_GEMM_SPLIT_F16;
    xw.a_scale2 = gs;
    xw.w_scale2 = wscale2;
    return vs_gemm_impl(xw, stream);
  }
  if (!ready.feat_rows) { if (int rc = vs_split_rows_impl(feat, M, K, K, gs, Ah, Al, 0, stream, math)) return rc; }
  return vs_gemm_presplit_impl(Ah, Al, prepared ? ready.wh : Wh, prepared ? ready.wl : Wl, S.Kp, xg, 8 * H, M, 8 * H, nullptr, nullptr,
                               rowbias, 8 * H, T, VS_ACT_NONE, 0, gs, wscale2, stream, math);
}

namespace {

// One forward call's context: what every stage reads off the dims, the parameters and the workspace.  Built once behind the
// validation of the entry point; the stage functions below take it by const reference.
struct BnPair { float *scale, *shift; };
struct Fwd {
  const vs_dims* d;
  const vs_params* p;
  void* ws;
  vs_ws_layout L;
  hipStream_t stream;
  int conv_act, bn_mode;
  bool train;                  // bn_mode == VS_BN_TRAIN: BatchNorm on batch statistics (running statistics updated), no tape
  const Prep* prep;            // prepared weights (eval), or NULL
  const int* lengths;          // device [B]: a ragged batch (eval, channels-last arithmetics), or NULL
  const MultiBufs* multi;      // several speakers per mixture, or NULL
  const VsLstmCarry* carry;    // the recurrence's forward direction from / to a caller-held state (a stream chunk), or NULL
  int B, T, F, H;
  size_t act_bytes;            // one buffer of the conv activation ping-pong
  template <typename U>
  U* at(size_t off) const { return ::at<U>(ws, off); }
  // scale / shift of layer l's epilogue: folded by vs_prepare_weights, or built per call in the workspace
  BnPair bn(int l) const {
    return {(prep ? prep->bn_scale : at<float>(L.bn_scale)) + 64 * l, (prep ? prep->bn_shift : at<float>(L.bn_shift)) + 64 * l};
  }
  double* stats() const { return at<double>(L.bn_stats); }
  // eval: BatchNorm folded from the running statistics, activation fused into the conv.  train: the conv writes conv + bias
  // (scale = 1, shift = bias, no activation); batch statistics, normalisation and activation follow as a second pass, which then
  // overwrites the layer's scale / shift with the batch's.
  int layer_act() const { return train ? VS_ACT_NONE : conv_act; }
  // ragged batch: rows behind each item's own end := 0 (one sweep over a channels-last tensor)
  int zero_tails(void* a, size_t row_bytes) const {
    return lengths ? vs_zero_tail_rows_impl(a, B, T, row_bytes, lengths, stream) : 0;
  }
};

Fwd make_fwd(const vs_dims* d, const vs_params* p, void* ws, const vs_ws_layout& L, int conv_act, int bn_mode, hipStream_t stream,
             const Prep* prep = nullptr, const int* lengths = nullptr, const MultiBufs* multi = nullptr, const VsLstmCarry* carry = nullptr) {
  Fwd f;
  f.d = d; f.p = p; f.ws = ws; f.L = L; f.stream = stream; f.conv_act = conv_act; f.bn_mode = bn_mode; f.train = bn_mode == VS_BN_TRAIN;
  f.prep = prep; f.lengths = lengths; f.multi = multi; f.carry = carry;
  f.B = d->B; f.T = d->T; f.F = d->F; f.H = d->H; f.act_bytes = (size_t)d->B * 64 * d->T * d->F * sizeof(float);
  return f;
}

// ---- stage 1: conv stack, models/voicesplit/model.py:68-74 ----
// The whole-path eval forward (nobody reads the fp32 features) lets cnn8 write the A operand of the LSTM input GEMM into the idle
// second ping-pong buffer itself -- bf16 rows (VS_MATH_BF16) or split-f16 hi / lo rows with a planned scale (VS_MATH_F16X3): no fp32
// features, no conversion / |max| / split passes.  Decided here, once per call: conv_stack() produces that form, bilstm() consumes it.
bool cnn8_writes_gemm_operand(const Fwd& f) {
  if (f.train || vs_opt(VS_OPT_FEAT_ROWS) == 0) return false;
  const int M = f.B * f.T, K = 8 * f.F;
  if (f.d->math == VS_MATH_BF16) {
    const VsLstmBf16Layout Lb = vs_lstm_bf16_layout(M, K, f.H);
    return f.act_bytes >= (f.prep ? Lb.wih : Lb.dxg);
  }
  return f.d->math == VS_MATH_F16X3 && vs_lstm_rows_fit(M, K, f.H, f.at<char>(f.L.act1), f.act_bytes, f.prep != nullptr);
}

// BASELINE configs[2]: channels-last bf16 activations [B][T][F][64] in the ping-pong buffers (half their size), conv_nhwc.hip /
// nhwc_first.hip / nhwc_bn.hip / nhwc_last.hip kernels.  eval: BatchNorm + activation in the conv epilogue; train: z = conv + bias with statistics from the
// epilogue, then one apply pass in place.
int convs_nhwc_bf16(const Fwd& f, const float* x, float* feat, bool rows) {
  const vs_params* p = f.p;
  const int B = f.B, T = f.T, F = f.F, act = f.layer_act();
  void* abuf[2] = {f.at<void>(f.L.act0), f.at<void>(f.L.act1)};
  double* stats = f.stats();
  const long long npix = (long long)B * T * F;
  const size_t row_bytes = (size_t)F * 64 * 2;
  int c = 0;
  {
    ProfScope ps(VS_PROF_CNN1, f.stream);
    const vs_conv_layer& cl = p->conv[0];
    const BnPair k = f.bn(0);
    if (f.train) {
      // cnn1 by recomputation (nhwc_first.hip): statistics of z1 from the input's moments, then one pass that writes act(BN(z1))
      double* mom = stats + 128;                          // behind slot 0 of the statistics scratch
      if (int rc = vs_nhwc_first_moments_impl(x, B, T, F, mom, f.stream)) return rc;
      if (int rc = vs_nhwc_first_stats_impl(mom, cl.weight, cl.bias, (double)npix, stats, f.stream)) return rc;
      if (int rc = vs_bn_finalize_impl(stats, 1, (double)npix, 64, cl.bn_weight, cl.bn_bias, cl.bn_running_mean, cl.bn_running_var, kBnEps,
                                       kBnMomentum, k.scale, k.shift, nullptr, nullptr, f.stream)) return rc;
      if (int rc = vs_nhwc_conv_first_impl(x, cl.weight, k.scale, k.shift, abuf[c], B, T, F, f.conv_act, nullptr, f.stream, cl.bias)) return rc;
    } else if (int rc = vs_nhwc_conv_first_impl(x, cl.weight, k.scale, k.shift, abuf[c], B, T, F, act, nullptr, f.stream)) return rc;
    if (int rc = f.zero_tails(abuf[c], row_bytes)) return rc;
  }
  for (int i = 0; i < 6; ++i) {
    const int l = i + 1;
    ProfScope ps(VS_PROF_CNN2 + i, f.stream);
    const vs_conv_layer& cl = p->conv[l];
    const BnPair k = f.bn(l);
    void* packed = f.prep ? f.prep->conv_packed[i] : f.at<void>(f.L.conv_packed[i]);
    if (!f.prep) { if (int rc = vs_nhwc_pack_impl(cl.weight, packed, kMid[i].kt, kMid[i].kf, 0, f.stream)) return rc; }
    if (f.train) VS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(double) * VS_BN_STAT_SLOTS * 128, f.stream));
    if (int rc = vs_nhwc_conv_impl(abuf[c], packed, k.scale, k.shift, abuf[c ^ 1], B, T, F, kMid[i].kt, kMid[i].kf,
                                   kMid[i].dil, act, f.train ? stats : nullptr, f.stream)) return rc;
    c ^= 1;
    if (f.train) {
      if (int rc = vs_bn_finalize_impl(stats, VS_BN_STAT_SLOTS, (double)npix, 64, cl.bn_weight, cl.bn_bias, cl.bn_running_mean,
                                       cl.bn_running_var, kBnEps, kBnMomentum, k.scale, k.shift, nullptr, nullptr, f.stream)) return rc;
      if (int rc = vs_nhwc_bn_apply_impl(abuf[c], abuf[c], npix, f.conv_act, k.scale, k.shift, f.stream)) return rc;
    }
    if (l < 6) { if (int rc = f.zero_tails(abuf[c], row_bytes)) return rc; }
  }
  ProfScope ps(VS_PROF_CNN8, f.stream);
  const vs_conv_layer& cl = p->conv[7];
  const BnPair k = f.bn(7);
  if (rows) {      // six layers: the input is act0 again and act1 is idle
    const VsLstmBf16Layout Lb = vs_lstm_bf16_layout((long long)B * T, 8 * F, f.H);
    return vs_nhwc_conv_last_impl(abuf[c], cl.weight, k.scale, k.shift, nullptr, B, T, F, act, f.stream, nullptr,
                                  nullptr, nullptr, VS_ACT_NONE, f.at<char>(f.L.act1) + Lb.feat, Lb.Kp);
  }
  if (int rc = vs_nhwc_conv_last_impl(abuf[c], cl.weight, k.scale, k.shift, feat, B, T, F, act, f.stream)) return rc;
  if (!f.train) return 0;
  return vs_bn_train_feat_impl(feat, feat, B, T, F, cl.bn_weight, cl.bn_bias, cl.bn_running_mean, cl.bn_running_var, kBnEps, kBnMomentum,
                               f.conv_act, stats, k.scale, k.shift, nullptr, nullptr, f.stream);
}

// BASELINE configs[1], eval: activations as channels-last hi / lo f16 planes in the ping-pong buffers; every layer writes its
// output at a scale derived on the device from the tracked |max| of its input (conv_nhwc_f16x3.hip), no host round trip.
int convs_nhwc_f16x3(const Fwd& f, const float* x, float* feat, bool rows) {
  const vs_params* p = f.p;
  const int B = f.B, T = f.T, F = f.F, act = f.layer_act();
  const size_t half = (size_t)B * T * F * 64 * 2, row_bytes = (size_t)F * 64 * 2;
  char* plane[2][2] = {{f.at<char>(f.L.act0), f.at<char>(f.L.act0) + half}, {f.at<char>(f.L.act1), f.at<char>(f.L.act1) + half}};
  float* cs = f.at<float>(f.L.conv_scales);
  VS_CHECK_HIP(hipMemsetAsync(cs, 0, 8 * VS_SCALE_SLOT_FLOATS * sizeof(float), f.stream));
  auto slot = [&](int l) { return cs + VS_SCALE_SLOT_FLOATS * l; };          // [0..1]: scale pair of layer l's input; + 8: its |max|
  {
    ProfScope ps(VS_PROF_CNN1, f.stream);
    const BnPair k = f.bn(0);
    if (int rc = vs_absmax_any_impl(x, (long long)B * T * F, vs_amax_slot(slot(0)), f.stream)) return rc;
    if (int rc = vs_nhwc_first_plan_impl(vs_amax_slot(slot(0)), 1, p->conv[0].weight, k.scale, k.shift, slot(1), f.stream)) return rc;
    if (int rc = vs_nhwc_conv_first_split_impl(x, p->conv[0].weight, k.scale, k.shift, slot(1), plane[0][0], plane[0][1], vs_amax_slot(slot(1)),
                                               B, T, F, act, f.stream)) return rc;
    if (int rc = f.zero_tails(plane[0][0], row_bytes)) return rc;
    if (int rc = f.zero_tails(plane[0][1], row_bytes)) return rc;
  }
  int c = 0;
  for (int i = 0; i < 6; ++i) {
    const int l = i + 1;
    ProfScope ps(VS_PROF_CNN2 + i, f.stream);
    const BnPair k = f.bn(l);
    char* mine = f.at<char>(f.L.conv_packed[i]);
    void* wpart = f.prep ? f.prep->conv_packed[i] : mine;
    float* plan = reinterpret_cast<float*>(mine + vs_nhwc_f16x3_wpart_bytes(kMid[i].kt, kMid[i].kf));
    // (cnn7's |max| is tracked only when cnn8 plans its output scale from it)
    if (int rc = vs_nhwc_f16x3_layer_impl(plane[c][0], plane[c][1], slot(l), vs_amax_slot(slot(l)), VS_AMAX_SLOTS, p->conv[l].weight,
                                          k.scale, k.shift, wpart, f.prep ? 1 : 0, plan, plane[c ^ 1][0], plane[c ^ 1][1],
                                          slot(l + 1), (l < 6 || rows) ? vs_amax_slot(slot(l + 1)) : nullptr, B, T, F, kMid[i].kt, kMid[i].kf,
                                          kMid[i].dil, act, f.stream)) return rc;
    c ^= 1;
    if (l < 6) {
      if (int rc = f.zero_tails(plane[c][0], row_bytes)) return rc;
      if (int rc = f.zero_tails(plane[c][1], row_bytes)) return rc;
    }
  }
  ProfScope ps(VS_PROF_CNN8, f.stream);
  const BnPair k = f.bn(7);
  if (!rows)
    return vs_nhwc_conv_last_split_impl(plane[c][0], plane[c][1], slot(7), p->conv[7].weight, k.scale, k.shift, feat, B, T, F, act, f.stream);
  // six layers: the input planes fill act0 again and act1 is idle; the rows go out at a scale planned from the tracked |max| of the input
  const VsLstmSplitLayout S = vs_lstm_split_layout((long long)B * T, 8 * F, f.H);
  float* gs = f.at<float>(f.L.gemm_scales);
  char* base = f.at<char>(f.L.act1);
  if (int rc = vs_nhwc_last_plan_impl(vs_amax_slot(slot(7)), VS_AMAX_SLOTS, p->conv[7].weight, k.scale, k.shift, gs, f.stream)) return rc;
  return vs_nhwc_conv_last_split_impl(plane[c][0], plane[c][1], slot(7), p->conv[7].weight, k.scale, k.shift, nullptr,
                                      B, T, F, act, f.stream, base + S.Ah, base + S.Al, S.Kp, gs);
}

// fp32 [B][64][T][F] activations: the strict fp32 arithmetic in either mode (prepared weights: packed once), and the split-f16
// arithmetic in train mode, where every producer of a conv operand folds its |max| into the consumer's scale slot
int convs_nchw(const Fwd& f, const float* x, float* feat) {
  const vs_params* p = f.p;
  const int B = f.B, T = f.T, F = f.F, act = f.layer_act();
  float* abuf[2] = {f.at<float>(f.L.act0), f.at<float>(f.L.act1)};
  double* stats = f.stats();
  float* cs = f.at<float>(f.L.conv_scales);
  const bool split = f.d->math == VS_MATH_F16X3;     // (train mode only: the eval forward of that arithmetic is channels-last)
  if (split) VS_CHECK_HIP(hipMemsetAsync(cs, 0, 8 * VS_SCALE_SLOT_FLOATS * sizeof(float), f.stream));
  auto amax_for = [&](int consumer_layer) -> unsigned* {    // consumer_layer = conv index 1..6 (cnn2..cnn7)
    return (split && consumer_layer >= 1 && consumer_layer <= 6) ? vs_amax_slot(cs + VS_SCALE_SLOT_FLOATS * consumer_layer) : nullptr;
  };
  auto bn_train = [&](int l, int stats_slots) -> int {
    const vs_conv_layer& cl = p->conv[l];
    const BnPair k = f.bn(l);
    return vs_bn_train_impl(abuf[l & 1], abuf[l & 1], B, 64, T * F, cl.bn_weight, cl.bn_bias, cl.bn_running_mean, cl.bn_running_var, kBnEps,
                            kBnMomentum, f.conv_act, stats, k.scale, k.shift, nullptr, nullptr, amax_for(l + 1), f.stream, stats_slots);
  };
  {
    ProfScope ps(VS_PROF_CNN1, f.stream);
    const BnPair k = f.bn(0);
    if (int rc = vs_conv_first_fwd_impl(x, p->conv[0].weight, k.scale, k.shift, abuf[0], B, T, F, act, nullptr, f.stream)) return rc;
    if (f.train) { if (int rc = bn_train(0, 0)) return rc; }
  }
  const bool fuse = f.train && split;        // statistics of a layer accumulated by its conv epilogue
  for (int i = 0; i < 6; ++i) {
    const int l = i + 1;      // layer l reads abuf[i & 1] and writes abuf[l & 1]
    ProfScope ps(VS_PROF_CNN2 + i, f.stream);
    const BnPair k = f.bn(l);
    if (fuse) VS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(double) * VS_BN_STAT_SLOTS * 128, f.stream));
    if (f.prep) {
      if (int rc = vs_conv64_fwd_impl(abuf[i & 1], static_cast<const float*>(f.prep->conv_packed[i]), k.scale, k.shift,
                                      abuf[l & 1], B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, act, f.stream)) return rc;
    } else if (int rc = vs_conv64_layer_impl(f.d->math, abuf[i & 1], p->conv[l].weight, f.at<float>(f.L.conv_packed[i]), cs + VS_SCALE_SLOT_FLOATS * l, 1,
                                             k.scale, k.shift, abuf[l & 1], B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, act, 0, nullptr,
                                             f.stream, fuse ? stats : nullptr)) return rc;
    if (f.train) { if (int rc = bn_train(l, fuse ? VS_BN_STAT_SLOTS : 0)) return rc; }
  }
  // cnn8, written straight into the LSTM feature layout
  ProfScope ps(VS_PROF_CNN8, f.stream);
  const vs_conv_layer& cl = p->conv[7];
  const BnPair k = f.bn(7);
  if (int rc = vs_conv_last_fwd_impl(abuf[0], cl.weight, k.scale, k.shift, feat, B, T, F, act, f.stream)) return rc;
  if (!f.train) return 0;
  return vs_bn_train_feat_impl(feat, feat, B, T, F, cl.bn_weight, cl.bn_bias, cl.bn_running_mean, cl.bn_running_var, kBnEps, kBnMomentum,
                               f.conv_act, stats, k.scale, k.shift, nullptr, nullptr, f.stream);
}

// rows: cnn8 writes the LSTM input GEMM's A operand instead of feat (cnn8_writes_gemm_operand; the stage entry points pass false)
int conv_stack(const Fwd& f, const float* x, float* feat, bool rows) {
  const vs_dims* d = f.d;
  const vs_params* p = f.p;
  VS_REQUIRE(p && x, "conv_stack: NULL argument");
  VS_REQUIRE(f.conv_act == VS_ACT_MISH || f.conv_act == VS_ACT_RELU, "conv_stack: conv_act must be MISH or RELU");
  VS_REQUIRE(f.bn_mode == VS_BN_EVAL || f.bn_mode == VS_BN_TRAIN, "conv_stack: unknown bn_mode %d", f.bn_mode);
  VS_REQUIRE(!(f.prep && f.train), "conv_stack: prepared weights are an eval-mode form (BatchNorm folded)");
  VS_REQUIRE(!f.lengths || (!f.train && d->math != VS_MATH_FP32),
             "conv_stack: per-item lengths are served in eval mode by the channels-last arithmetics (VS_MATH_F16X3, VS_MATH_BF16), not by %s",
             f.train ? "train mode" : "VS_MATH_FP32");
  if (int rc = check_conv_params(p, "conv_stack")) return rc;
  if (!feat) feat = f.at<float>(f.L.feat);
  // Ragged batch (lengths != NULL): every layer with extent in time (cnn2 7x1, cnn3..cnn7 5x5 dilated) must see ZEROS behind each item's
  // own end, as its ZeroPad2d gives the item alone.  So x is read from a copy with zeroed tails (in the feature region: cnn8 writes it only
  // when cnn1 is long done, or never), and the outputs of cnn1..cnn6 get their tail rows zeroed before the next layer reads them -- one
  // sweep per layer over the channels-last tensor(s).  The convs themselves run over all B*T rows (no row-group skipping: see DESIGN.md
  // 6.8b); the |max| that the split-f16 layers track therefore includes the finite tail rows they computed, which moves a power-of-two
  // operand scale at most, as a batch mate does.  cnn7's and cnn8's tails stay: nothing behind them looks across rows.
  if (f.lengths) {
    float* xz = f.at<float>(f.L.feat);
    VS_CHECK_HIP(hipMemcpyAsync(xz, x, sizeof(float) * (size_t)d->B * d->T * d->F, hipMemcpyDeviceToDevice, f.stream));
    if (int rc = vs_zero_tail_rows_impl(xz, d->B, d->T, sizeof(float) * (size_t)d->F, f.lengths, f.stream)) return rc;
    x = xz;
  }
  // per-layer epilogue constants (Fwd::layer_act): folded by vs_prepare_weights, folded here, or the identity in front of batch statistics
  if (!f.prep && !f.train) {
    for (int l = 0; l < 8; ++l) {
      const vs_conv_layer& c = p->conv[l];
      const BnPair k = f.bn(l);
      if (int rc = vs_bn_fold_impl(c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, c.bias, kBnEps, kConvOut[l], k.scale, k.shift, f.stream)) return rc;
    }
  } else if (!f.prep) {
    VS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(f.bn(0).scale), 0x3f800000 /* 1.0f */, 8 * 64, f.stream));
    for (int l = 0; l < 8; ++l)
      VS_CHECK_HIP(hipMemcpyAsync(f.bn(l).shift, p->conv[l].bias, sizeof(float) * kConvOut[l], hipMemcpyDeviceToDevice, f.stream));
  }
  if (d->math == VS_MATH_BF16) return convs_nhwc_bf16(f, x, feat, rows);
  if (d->math == VS_MATH_F16X3 && !f.train) return convs_nhwc_f16x3(f, x, feat, rows);
  return convs_nchw(f, x, feat);
}

// ---- stage 2: d-vector concat + BiLSTM, models/voicesplit/model.py:77-82 ----
// feat_rows: cnn8 left the input GEMM's A operand in the second ping-pong buffer (conv_stack).  multi: dvec is [B][K][E]
int bilstm(const Fwd& f, const float* feat, const float* dvec, float* lstm_out, bool feat_rows) {
  const vs_dims* d = f.d;
  const vs_params* p = f.p;
  const vs_ws_layout& L = f.L;
  const MultiBufs* multi = f.multi;
  VS_REQUIRE(p && dvec, "bilstm: NULL argument");
  VS_REQUIRE(!multi || lstm_out, "bilstm: the multi-speaker form writes the caller's lstm_out");
  if (!feat) feat = f.at<float>(L.feat);
  if (!lstm_out) lstm_out = f.at<float>(L.lstm_out);
  const int B = f.B, T = f.T, H = f.H, K = 8 * d->F, KE = K + d->E;
  const int NS = multi ? B * multi->K : B;          // sequences of the recurrence = rows of the d-vector GEMM
  float* dvbias = multi ? multi->rb : f.at<float>(L.dvbias);
  float* xg = f.at<float>(L.xg);
  {
    ProfScope ps(VS_PROF_LSTM_GEMM, f.stream);
    for (int dir = 0; dir < 2; ++dir) {
      VS_REQUIRE(p->w_ih[dir] && p->w_hh[dir] && p->b_ih[dir] && p->b_hh[dir], "bilstm: NULL LSTM parameter (dir %d)", dir);
      // cat((x, dvec.repeat(T))) @ W_ih^T == x @ W_ih[:, :8F]^T + (dvec @ W_ih[:, 8F:]^T): the
      // second term does not depend on t -> one [B][4H] row bias per utterance (+ b_ih + b_hh).
      if (int rc = vs_gemm_impl({.A = dvec, .lda = d->E, .W = p->w_ih[dir] + K, .ldw = KE, .C = dvbias + (size_t)dir * 4 * H, .ldc = 8 * H,
                                 .M = NS, .N = 4 * H, .K = d->E, .bias1 = p->b_ih[dir], .bias2 = p->b_hh[dir]}, f.stream)) return rc;
    }
    // both directions in one launch (N = 8H): twice the workgroups, half the tail quantisation.  multi: the K speakers of a mixture
    // share its gate pre-activations, so the big GEMM runs once per mixture WITHOUT the row bias; the shared-input recurrence adds each
    // sequence's own (lstm_fwd.hip).  The conv stack is done: its activation ping-pong is the GEMM's operand scratch (feat may be the
    // caller's own buffer) -- the second buffer where cnn8 left the A operand, else both.
    VsLstmGemmReady ready;
    if (f.prep) { ready.wscale2 = f.prep->gemm_wscale; ready.wh = f.prep->wih_hi; ready.wl = f.prep->wih_lo; }
    ready.feat_bf16 = feat_rows && d->math == VS_MATH_BF16;
    ready.feat_rows = feat_rows && d->math == VS_MATH_F16X3;
    const size_t both = L.act1 == L.act0 + f.act_bytes ? 2 * f.act_bytes : f.act_bytes;
    if (int rc = vs_lstm_input_gemm_impl(d->math, feat, K, p->w_ih[0], p->w_ih[1], H, KE, xg, B * T, multi ? nullptr : dvbias, T,
                                         f.at<float>(L.gemm_scales), f.at<char>(feat_rows ? L.act1 : L.act0), feat_rows ? f.act_bytes : both,
                                         f.stream, ready)) return rc;
  }
  float* packed = f.prep ? f.prep->lstm_packed : f.at<float>(L.lstm_packed);
  if (!f.prep) { if (int rc = vs_lstm_pack_impl(p->w_hh[0], p->w_hh[1], packed, H, f.stream, d->math)) return rc; }
  ProfScope ps(VS_PROF_LSTM_REC, f.stream);
  // (lengths: the input GEMM above ran over all B*T rows; the recurrence keeps the rows behind an item's end out of its state)
  if (multi)
    return vs_bilstm_recurrent_impl(xg, packed, multi->lstm_state, lstm_out, nullptr, nullptr, NS, T, H, f.stream, d->math, f.lengths, dvbias, multi->K,
                                    f.carry);
  return vs_bilstm_recurrent_impl(xg, packed, f.at<float>(L.lstm_state), lstm_out, nullptr, nullptr, B, T, H, f.stream, d->math, f.lengths,
                                  nullptr, 1, f.carry);
}

// ---- stage 3: head, models/voicesplit/model.py:83-87 ----
// over the B*T rows of lstm_out (NULL: the workspace's), or the B*K*T rows of the multi-speaker form
int head(const Fwd& f, const float* lstm_out, float* logits, float* mask) {
  const vs_dims* d = f.d;
  const vs_params* p = f.p;
  VS_REQUIRE(p && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "head: NULL parameter");
  VS_REQUIRE(mask || logits, "head: no output requested");
  if (!lstm_out) lstm_out = f.multi ? f.multi->lstm_out : f.at<float>(f.L.lstm_out);
  float* h1 = f.multi ? f.multi->fc1_out : f.at<float>(f.L.fc1_out);
  const int M = f.B * (f.multi ? f.multi->K : 1) * f.T;
  ProfScope ps(VS_PROF_HEAD, f.stream);
  if (d->math == VS_MATH_BF16 && vs_head_fused_supported(2 * d->H, d->FC1, d->FC2)) {
    // one launch, h1 in registers between the two contractions (head_fused.hip).  The weights' fragment images come prepared
    // (vs_prepare_weights) or are packed here into the conv stack's first activation buffer, idle by now (stream order) -- the
    // same images either way, so the two routes stay bit-identical.  A clip of a frame or two at full width cannot hold them:
    // the two-launch form below (same roundings, fp32 summation order differs)
    const void* img = f.prep ? f.prep->head_packed : nullptr;
    if (!img && f.L.act1 - f.L.act0 >= vs_head_fused_packed_bytes(2 * d->H, d->FC1, d->FC2)) {
      void* scratch = f.at<void>(f.L.act0);
      if (int rc = vs_head_fused_pack_impl(p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, 2 * d->H, d->FC1, d->FC2, scratch, f.stream)) return rc;
      img = scratch;
    }
    if (img) return vs_head_fused_impl(lstm_out, img, nullptr, logits, mask, M, 2 * d->H, d->FC1, d->FC2, f.stream);
  }
  // VS_MATH_BF16: bf16-rounded operands on the bf16 matrix instruction, fp32 accumulate and epilogue
  const VsGemmArith arith = d->math == VS_MATH_BF16 ? VS_GEMM_FP32_BF16 : VS_GEMM_FP32;
  // relu(lstm) -> fc1 -> relu
  if (int rc = vs_gemm_impl({.arith = arith, .A = lstm_out, .lda = 2 * d->H, .a_relu = 1, .W = p->fc1_w, .ldw = 2 * d->H, .C = h1, .ldc = d->FC1,
                             .M = M, .N = d->FC1, .K = 2 * d->H, .bias1 = p->fc1_b, .act = VS_ACT_RELU}, f.stream)) return rc;
  // fc2 -> sigmoid
  VsGemm fc2{.arith = arith, .A = h1, .lda = d->FC1, .W = p->fc2_w, .ldw = d->FC1, .C = logits, .ldc = d->FC2,
             .M = M, .N = d->FC2, .K = d->FC1, .bias1 = p->fc2_b};
  if (logits) { if (int rc = vs_gemm_impl(fc2, f.stream)) return rc; }
  if (!mask) return 0;
  fc2.C = mask;
  fc2.act = VS_ACT_SIGMOID;
  return vs_gemm_impl(fc2, f.stream);
}

// ---- the whole path: what every vs_forward* runs behind its own validation ----
int forward(const Fwd& f, const float* x, const float* dvec, float* mask) {
  const bool rows = cnn8_writes_gemm_operand(f);
  if (int rc = conv_stack(f, x, nullptr, rows)) return rc;
  if (int rc = bilstm(f, nullptr, dvec, f.multi ? f.multi->lstm_out : nullptr, rows)) return rc;
  if (int rc = head(f, nullptr, nullptr, mask)) return rc;
  if (!f.lengths) return 0;
  // the head ran over every row (a zero LSTM row still gives sigmoid(bias terms)): the mask's tail rows are stored as zeros here
  const int K = f.multi ? f.multi->K : 1;
  return vs_zero_tail_rows_impl(mask, f.B * K, f.T, sizeof(float) * (size_t)f.d->FC2, f.lengths, f.stream, K);
}

int check_ragged(const vs_dims* d, const int* lengths, const char* what) {
  if (int rc = check_dims(d)) return rc;
  VS_REQUIRE(lengths != nullptr, "%s: lengths is NULL", what);
  VS_REQUIRE(d->math == VS_MATH_F16X3 || d->math == VS_MATH_BF16,
             "%s: per-item lengths are served by VS_MATH_F16X3 and VS_MATH_BF16; VS_MATH_FP32 has no ragged route", what);
  return 0;
}

int check_multi(const vs_dims* d, const float* dvecs, int K, const char* what) {
  if (int rc = check_dims(d)) return rc;
  VS_REQUIRE(K >= 1, "%s: K=%d speakers per mixture (K >= 1)", what, K);
  VS_REQUIRE(dvecs != nullptr, "%s: dvecs is NULL", what);
  VS_REQUIRE(d->math == VS_MATH_F16X3 || d->math == VS_MATH_BF16,
             "%s: several speakers per mixture are served by VS_MATH_F16X3 and VS_MATH_BF16; VS_MATH_FP32 has no shared-input recurrence", what);
  return 0;
}

}  // namespace

extern "C" {

int vs_workspace_layout(const vs_dims* dims, vs_ws_layout* out) {
  VS_REQUIRE(out != nullptr, "layout out pointer is NULL");
  memset(out, 0, sizeof(*out));
  return layout(dims, out);
}

size_t vs_workspace_bytes(const vs_dims* dims) {
  vs_ws_layout L;
  memset(&L, 0, sizeof(L));
  if (layout(dims, &L)) return 0;
  return L.total_bytes;
}

size_t vs_multi_workspace_bytes(const vs_dims* dims, int K) {
  MultiLayout M;
  memset(&M, 0, sizeof(M));
  if (multi_layout(dims, K, &M)) return 0;
  return M.total_bytes;
}

// eval-mode forward with the weight-only work done once (validation / serving: weights do not change
// between calls; utils/generic_utils.py:476-558 runs the model sample by sample at B = 1)
size_t vs_prepared_bytes(const vs_dims* dims) {
  PrepLayout L;
  memset(&L, 0, sizeof(L));
  if (prep_layout(dims, &L)) return 0;
  return L.total_bytes;
}

int vs_prepare_weights(const vs_dims* d, const vs_params* p, void* prepared, size_t prepared_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  Prep P;
  if (int rc = prep_pointers(d, prepared, prepared_bytes, &P)) return rc;
  VS_REQUIRE(p != nullptr, "prepare_weights: params is NULL");
  if (int rc = check_conv_params(p, "prepare_weights")) return rc;
  for (int l = 0; l < 8; ++l) {
    const vs_conv_layer& c = p->conv[l];
    if (int rc = vs_bn_fold_impl(c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, c.bias, kBnEps, kConvOut[l],
                                 P.bn_scale + 64 * l, P.bn_shift + 64 * l, stream)) return rc;
  }
  for (int i = 0; i < 6; ++i) {
    const float* w = p->conv[i + 1].weight;
    if (d->math == VS_MATH_BF16) {
      if (int rc = vs_nhwc_pack_impl(w, P.conv_packed[i], kMid[i].kt, kMid[i].kf, 0, stream)) return rc;
    } else if (d->math == VS_MATH_F16X3) {
      if (int rc = vs_nhwc_f16x3_prepare_wpart_impl(w, P.conv_packed[i], kMid[i].kt, kMid[i].kf, stream)) return rc;
    } else {
      if (int rc = vs_conv64_pack_impl(w, static_cast<float*>(P.conv_packed[i]), kMid[i].kt, kMid[i].kf, 0, stream)) return rc;
    }
  }
  for (int dir = 0; dir < 2; ++dir)
    VS_REQUIRE(p->w_ih[dir] && p->w_hh[dir], "prepare_weights: NULL LSTM parameter (dir %d)", dir);
  const int K = 8 * d->F, KE = K + d->E;
  if (d->math == VS_MATH_BF16) {      // [8H][Kp] bf16, both directions stacked: the B operand of gemm_bf16.hip
    const int Kp = vs_lstm_bf16_layout(0, K, d->H).Kp;
    if (int rc = vs_cvt_rows_bf16_impl(p->w_ih[0], 4 * d->H, K, KE, P.wih_hi, Kp, stream)) return rc;
    if (int rc = vs_cvt_rows_bf16_impl(p->w_ih[1], 4 * d->H, K, KE, P.wih_hi + (size_t)4 * d->H * Kp, Kp, stream)) return rc;
  } else if (d->math != VS_MATH_FP32) {
    if (int rc = vs_lstm_split_wih_impl(d->math, p->w_ih[0], p->w_ih[1], d->H, K, KE,
                                        reinterpret_cast<unsigned*>(P.gemm_wscale + 4), P.gemm_wscale, P.wih_hi, P.wih_lo, stream)) return rc;
  }
  if (P.head_packed) {
    VS_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "prepare_weights: NULL head parameter");
    if (int rc = vs_head_fused_pack_impl(p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, 2 * d->H, d->FC1, d->FC2, P.head_packed, stream)) return rc;
  }
  return vs_lstm_pack_impl(p->w_hh[0], p->w_hh[1], P.lstm_packed, d->H, stream, d->math);
}

// ---- the whole path ----
int vs_forward(const vs_dims* d, const vs_params* p, const float* x, const float* dvec, int conv_act, int bn_mode,
               void* ws, size_t ws_bytes, float* mask, void* stream) {
  VS_REQUIRE(mask != nullptr, "forward: mask is NULL");
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return forward(make_fwd(d, p, ws, L, conv_act, bn_mode, (hipStream_t)stream), x, dvec, mask);
}

int vs_forward_prepared(const vs_dims* d, const vs_params* p, const void* prepared, size_t prepared_bytes,
                        const float* x, const float* dvec, int conv_act, void* ws, size_t ws_bytes, float* mask, void* stream) {
  VS_REQUIRE(mask != nullptr, "forward_prepared: mask is NULL");
  Prep P;
  if (int rc = prep_pointers(d, prepared, prepared_bytes, &P)) return rc;
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return forward(make_fwd(d, p, ws, L, conv_act, VS_BN_EVAL, (hipStream_t)stream, &P), x, dvec, mask);
}

// the same forward on a padded batch of clips of unequal length, each as if alone (see the header)
int vs_forward_prepared_ragged(const vs_dims* d, const vs_params* p, const void* prepared, size_t prepared_bytes,
                               const float* x, const float* dvec, const int* lengths, int conv_act,
                               void* ws, size_t ws_bytes, float* mask, void* stream) {
  VS_REQUIRE(mask != nullptr, "forward_prepared_ragged: mask is NULL");
  if (int rc = check_ragged(d, lengths, "forward_prepared_ragged")) return rc;
  Prep P;
  if (int rc = prep_pointers(d, prepared, prepared_bytes, &P)) return rc;
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return forward(make_fwd(d, p, ws, L, conv_act, VS_BN_EVAL, (hipStream_t)stream, &P, lengths), x, dvec, mask);
}

// several enrolled speakers per mixture: conv stack and LSTM input GEMM once, recurrence and head per speaker (see the header)
int vs_forward_prepared_multi(const vs_dims* d, const vs_params* p, const void* prepared, size_t prepared_bytes,
                              const float* x, const float* dvecs, int K, const int* lengths, int conv_act,
                              void* ws, size_t ws_bytes, float* mask, void* stream) {
  if (int rc = check_multi(d, dvecs, K, "forward_prepared_multi")) return rc;
  VS_REQUIRE(mask != nullptr, "forward_prepared_multi: mask is NULL");
  Prep P;
  if (int rc = prep_pointers(d, prepared, prepared_bytes, &P)) return rc;
  MultiLayout M;
  if (int rc = check_multi_ws(d, K, ws, ws_bytes, &M)) return rc;
  const MultiBufs mb = multi_bufs(ws, M, K);
  return forward(make_fwd(d, p, ws, M.base, conv_act, VS_BN_EVAL, (hipStream_t)stream, &P, lengths, &mb), x, dvecs, mask);
}

// ---- the stages on their own ----
int vs_conv_stack_fwd(const vs_dims* d, const vs_params* p, const float* x, int conv_act, int bn_mode,
                      void* ws, size_t ws_bytes, float* feat, void* stream) {
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return conv_stack(make_fwd(d, p, ws, L, conv_act, bn_mode, (hipStream_t)stream), x, feat, false);
}

int vs_conv_stack_fwd_ragged(const vs_dims* d, const vs_params* p, const float* x, const int* lengths, int conv_act,
                             void* ws, size_t ws_bytes, float* feat, void* stream) {
  if (int rc = check_ragged(d, lengths, "conv_stack_fwd_ragged")) return rc;
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return conv_stack(make_fwd(d, p, ws, L, conv_act, VS_BN_EVAL, (hipStream_t)stream, nullptr, lengths), x, feat, false);
}

int vs_bilstm_fwd(const vs_dims* d, const vs_params* p, const float* feat, const float* dvec,
                  void* ws, size_t ws_bytes, float* lstm_out, void* stream) {
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return bilstm(make_fwd(d, p, ws, L, VS_ACT_NONE, VS_BN_EVAL, (hipStream_t)stream), feat, dvec, lstm_out, false);
}

int vs_bilstm_fwd_ragged(const vs_dims* d, const vs_params* p, const float* feat, const float* dvec, const int* lengths,
                         void* ws, size_t ws_bytes, float* lstm_out, void* stream) {
  if (int rc = check_ragged(d, lengths, "bilstm_fwd_ragged")) return rc;
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return bilstm(make_fwd(d, p, ws, L, VS_ACT_NONE, VS_BN_EVAL, (hipStream_t)stream, nullptr, lengths), feat, dvec, lstm_out, false);
}

int vs_bilstm_fwd_multi(const vs_dims* d, const vs_params* p, const float* feat, const float* dvecs, int K, const int* lengths,
                        void* ws, size_t ws_bytes, float* lstm_out, void* stream) {
  if (int rc = check_multi(d, dvecs, K, "bilstm_fwd_multi")) return rc;
  VS_REQUIRE(feat && lstm_out, "bilstm_fwd_multi: NULL argument");
  MultiLayout M;
  if (int rc = check_multi_ws(d, K, ws, ws_bytes, &M)) return rc;
  const MultiBufs mb = multi_bufs(ws, M, K);
  return bilstm(make_fwd(d, p, ws, M.base, VS_ACT_NONE, VS_BN_EVAL, (hipStream_t)stream, nullptr, lengths, &mb), feat, dvecs, lstm_out, false);
}

int vs_bilstm_fwd_carry(const vs_dims* d, const vs_params* p, const float* feat, const float* dvec,
                        const float* state_in, float* state_out, int keep,
                        void* ws, size_t ws_bytes, float* lstm_out, void* stream) {
  if (int rc = check_dims(d)) return rc;
  if (int rc = vs_lstm_carry_check(d->math, d->H, d->T, keep, state_out, "bilstm_fwd_carry")) return rc;
  VS_REQUIRE(feat && lstm_out, "bilstm_fwd_carry: NULL argument");
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  const VsLstmCarry carry{state_in, state_out, keep};
  return bilstm(make_fwd(d, p, ws, L, VS_ACT_NONE, VS_BN_EVAL, (hipStream_t)stream, nullptr, nullptr, nullptr, &carry), feat, dvec, lstm_out, false);
}

// one chunk of a stream for K enrolled speakers per mixture: the input GEMM once without row bias, the carry x shared-input recurrence
// over the B*K sequences (see the header)
int vs_bilstm_fwd_carry_multi(const vs_dims* d, const vs_params* p, const float* feat, const float* dvecs, int K,
                              const float* state_in, float* state_out, int keep,
                              void* ws, size_t ws_bytes, float* lstm_out, void* stream) {
  if (int rc = check_multi(d, dvecs, K, "bilstm_fwd_carry_multi")) return rc;
  if (int rc = vs_lstm_carry_check(d->math, d->H, d->T, keep, state_out, "bilstm_fwd_carry_multi")) return rc;
  VS_REQUIRE(feat && lstm_out, "bilstm_fwd_carry_multi: NULL argument");
  MultiLayout M;
  if (int rc = check_multi_ws(d, K, ws, ws_bytes, &M)) return rc;
  const MultiBufs mb = multi_bufs(ws, M, K);
  const VsLstmCarry carry{state_in, state_out, keep};
  return bilstm(make_fwd(d, p, ws, M.base, VS_ACT_NONE, VS_BN_EVAL, (hipStream_t)stream, nullptr, nullptr, &mb, &carry), feat, dvecs, lstm_out, false);
}

int vs_head_fwd(const vs_dims* d, const vs_params* p, const float* lstm_out, void* ws, size_t ws_bytes,
                float* logits, float* mask, void* stream) {
  vs_ws_layout L;
  if (int rc = check_ws(d, ws, ws_bytes, &L)) return rc;
  return head(make_fwd(d, p, ws, L, VS_ACT_NONE, VS_BN_EVAL, (hipStream_t)stream), lstm_out, logits, mask);
}

}  // extern "C"
