// extern "C" surface of libvoicesplit_hip.so (declared in include/voicesplit_hip.h) below the model: the error string, the option
// table, the opt-in profiling scopes, and the pass-through wrappers of the kernel-level entry points that the unit tests drive.
// (The forward pass and its layouts: forward.hip; the training schedule: train.hip.)
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

// ---- error string --------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void vs_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- opt-in per-stage timing (bench.py roofline leg) -------------------------------------------
// vs_profile_begin(n) pre-creates HIP events for n forward calls; while enabled every stage of
// vs_conv_stack_fwd / vs_bilstm_fwd / vs_head_fwd is bracketed by two events recorded on the
// caller's stream (no synchronisation, ~1 us each).  vs_profile_end() synchronises the events,
// sums the elapsed time per slot and frees them.  Instrumentation only: process-global, not
// thread safe, off by default.
// defaults of vs_set_option (include/voicesplit_hip.h, enum vs_option)
int g_vs_options[VS_OPT_COUNT] = {/*FWD_PROLOGUE*/ 1, /*HEAD_LEAF_SIDE*/ 1, /*FEAT_ROWS*/ 1, /*HEAD_BWD_GEMM*/ 1, /*ABLATION*/ 0, /*DETERMINISTIC*/ 0};
thread_local unsigned* g_vs_turn = nullptr;

namespace {
struct Prof {
  bool on = false;
  int max_calls = 0;
  int calls[VS_PROF_SLOTS] = {0};
  hipEvent_t* ev = nullptr;   // [max_calls][VS_PROF_SLOTS][2]
} g_prof;

}  // namespace

// a slot may be entered several times per step (e.g. one BatchNorm scope per layer): every entry
// gets its own event pair, `calls` counts entries
VsProfScope::VsProfScope(int slot, hipStream_t s_) : s(s_), idx(-1) {
  if (!g_prof.on || g_prof.calls[slot] >= g_prof.max_calls) return;
  idx = (g_prof.calls[slot]++ * VS_PROF_SLOTS + slot) * 2;
  (void)hipEventRecord(g_prof.ev[idx], s);
}
VsProfScope::~VsProfScope() { if (idx >= 0) (void)hipEventRecord(g_prof.ev[idx + 1], s); }

extern "C" {

int vs_abi_version(void) { return VS_ABI_VERSION; }

int vs_set_option(int option, int value) {
  VS_REQUIRE(option >= 0 && option < VS_OPT_COUNT, "vs_set_option: unknown option %d", option);
  bool ok = true;
  switch (option) {
    case VS_OPT_FWD_PROLOGUE: case VS_OPT_HEAD_LEAF_SIDE: case VS_OPT_FEAT_ROWS: case VS_OPT_HEAD_BWD_GEMM: case VS_OPT_DETERMINISTIC:
      ok = value == 0 || value == 1; break;
    default: ok = value >= 0; break;
  }
  VS_REQUIRE(ok, "vs_set_option: value %d is outside the range of option %d", value, option);
  g_vs_options[option] = value;
  return 0;
}

int vs_get_option(int option) { return (option >= 0 && option < VS_OPT_COUNT) ? g_vs_options[option] : -1; }

int vs_profile_begin(int max_calls) {
  VS_REQUIRE(!g_prof.on, "profile: already enabled");
  VS_REQUIRE(max_calls > 0 && max_calls <= 4096, "profile: max_calls=%d out of range", max_calls);
  max_calls *= 8;   // slots entered once per layer (BatchNorm passes) use up to 8 entries per step
  const int n = max_calls * VS_PROF_SLOTS * 2;
  g_prof.ev = new hipEvent_t[n];
  for (int i = 0; i < n; ++i) VS_CHECK_HIP(hipEventCreate(&g_prof.ev[i]));
  for (int i = 0; i < VS_PROF_SLOTS; ++i) g_prof.calls[i] = 0;
  g_prof.max_calls = max_calls;
  g_prof.on = true;
  return 0;
}

int vs_profile_end(float* ms_total, int* calls) {
  VS_REQUIRE(g_prof.on, "profile: not enabled");
  g_prof.on = false;
  int rc = 0;
  for (int slot = 0; slot < VS_PROF_SLOTS; ++slot) {
    double tot = 0;
    for (int c = 0; c < g_prof.calls[slot]; ++c) {
      const int idx = (c * VS_PROF_SLOTS + slot) * 2;
      float ms = 0.f;
      hipError_t e = hipEventSynchronize(g_prof.ev[idx + 1]);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_prof.ev[idx], g_prof.ev[idx + 1]);
      if (e != hipSuccess) { vs_set_error("profile: %s", hipGetErrorString(e)); rc = -2; }
      tot += ms;
    }
    if (ms_total) ms_total[slot] = (float)tot;
    if (calls) calls[slot] = g_prof.calls[slot];
  }
  const int n = g_prof.max_calls * VS_PROF_SLOTS * 2;
  for (int i = 0; i < n; ++i) (void)hipEventDestroy(g_prof.ev[i]);
  delete[] g_prof.ev;
  g_prof.ev = nullptr;
  g_prof.max_calls = 0;
  return rc;
}
const char* vs_last_error(void) { return g_err; }

int vs_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* conv_bias,
               float eps, int C, float* scale, float* shift, void* stream) {
  return vs_bn_fold_impl(gamma, beta, mean, var, conv_bias, eps, C, scale, shift, (hipStream_t)stream);
}

int vs_conv_first_fwd(const float* x, const float* w, const float* scale, const float* shift, float* out,
                      int B, int T, int F, int act, void* stream) {
  return vs_conv_first_fwd_impl(x, w, scale, shift, out, B, T, F, act, nullptr, (hipStream_t)stream);
}

int vs_conv64_pack(const float* w, float* packed, int KT, int KF, void* stream) {
  return vs_conv64_pack_impl(w, packed, KT, KF, 0, (hipStream_t)stream);
}

int vs_conv64_fwd(const float* in, const float* packed, const float* scale, const float* shift, float* out,
                  int B, int T, int F, int KT, int KF, int dil, int act, void* stream) {
  VS_REQUIRE(in != out, "conv64: in-place is not supported");
  return vs_conv64_fwd_impl(in, packed, scale, shift, out, B, T, F, KT, KF, dil, act, (hipStream_t)stream);
}

int vs_pow2_scale(const float* x, long long n, void* amax_scratch, float* scale2, void* stream) {
  VS_REQUIRE(x && amax_scratch && scale2, "pow2_scale: NULL argument");
  return vs_pow2_scale_impl(x, n, static_cast<unsigned*>(amax_scratch), scale2, (hipStream_t)stream);
}

int vs_conv64_pack_f16(const float* w, void* packed, int KT, int KF, int transpose_flip, void* amax_scratch,
                       float* w_scale2, void* stream) {
  VS_REQUIRE(w && packed && amax_scratch && w_scale2, "conv64_pack_f16: NULL argument");
  return vs_conv64_pack_f16_impl(w, static_cast<_Float16*>(packed), KT, KF, transpose_flip,
                                 static_cast<unsigned*>(amax_scratch), w_scale2, (hipStream_t)stream);
}

int vs_conv64_f16x3_fwd(const float* in, const void* packed, const float* scale, const float* shift,
                        const float* in_scale2, const float* w_scale2, float* out,
                        int B, int T, int F, int KT, int KF, int dil, int act, void* stream) {
  VS_REQUIRE(in != out, "conv64_f16x3: in-place is not supported");
  return vs_conv64_f16x3_fwd_impl(in, static_cast<const _Float16*>(packed), scale, shift, in_scale2, w_scale2, out,
                                  B, T, F, KT, KF, dil, act, nullptr, (hipStream_t)stream);
}

// ---- channels-last bf16 kernels of the VS_MATH_BF16 path (csrc/conv_nhwc.hip) -----------------------------
size_t vs_nhwc_conv_packed_bytes(int KT, int KF) { return vs_nhwc_packed_bytes(KT, KF); }

int vs_nhwc_conv_pack(const float* w, void* packed, int KT, int KF, int transpose_flip, void* stream) {
  return vs_nhwc_pack_impl(w, packed, KT, KF, transpose_flip, (hipStream_t)stream);
}

int vs_nhwc_conv(const void* in, const void* packed, const float* scale, const float* shift, void* out,
                 int B, int T, int F, int KT, int KF, int dil, int act, double* bn_stats, void* stream) {
  VS_REQUIRE(in != out, "nhwc_conv: in-place is not supported");
  return vs_nhwc_conv_impl(in, packed, scale, shift, out, B, T, F, KT, KF, dil, act, bn_stats, (hipStream_t)stream);
}

size_t vs_nhwc_conv_f16x3_scratch_bytes(int KT, int KF) { return vs_nhwc_f16x3_layer_scratch_bytes(KT, KF); }

int vs_nhwc_conv_f16x3_layer(const void* in_hi, const void* in_lo, const float* in_scale2, const unsigned* amax_in, int n_amax,
                             const float* w, const float* bn_scale, const float* bn_shift, void* scratch, int packed_ready,
                             void* out_hi, void* out_lo, float* out_scale2, unsigned* amax_out,
                             int B, int T, int F, int KT, int KF, int dil, int act, void* stream) {
  VS_REQUIRE(in_hi && in_lo && out_hi && out_lo && in_scale2 && amax_in && n_amax > 0 && bn_scale && bn_shift && out_scale2,
             "nhwc_conv_f16x3: NULL argument");
  VS_REQUIRE(in_hi != out_hi && in_lo != out_lo && in_hi != out_lo && in_lo != out_hi, "nhwc_conv_f16x3: in-place is not supported");
  VS_REQUIRE((KT == 5 && KF == 5) || (KT == 7 && KF == 1), "nhwc_conv_f16x3: kernel %dx%d is not one of the stack's (7x1, 5x5)", KT, KF);
  VS_REQUIRE(scratch != nullptr, "nhwc_conv_f16x3: NULL scratch");
  float* plan = reinterpret_cast<float*>(static_cast<char*>(scratch) + vs_nhwc_f16x3_wpart_bytes(KT, KF));
  return vs_nhwc_f16x3_layer_impl(in_hi, in_lo, in_scale2, amax_in, n_amax, w, bn_scale, bn_shift, scratch, packed_ready, plan, out_hi, out_lo,
                                  out_scale2, amax_out, B, T, F, KT, KF, dil, act, (hipStream_t)stream);
}

int vs_f16x3_split(const float* x, const float* scale2, void* hi, void* lo, long long n, void* stream) {
  return vs_f16x3_split_impl(x, scale2, hi, lo, n, (hipStream_t)stream);
}

int vs_f16x3_merge(const void* hi, const void* lo, const float* scale2, float* x, long long n, void* stream) {
  return vs_f16x3_merge_impl(hi, lo, scale2, x, n, (hipStream_t)stream);
}

int vs_cvt_rows_bf16(const float* src, long long rows, int K, int ld, void* dst, int Kp, void* stream) {
  return vs_cvt_rows_bf16_impl(src, rows, K, ld, dst, Kp, (hipStream_t)stream);
}

int vs_gemm_bf16(int a_kmajor, int b_kmajor, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                 const float* rowbias, int ldrb, int group, int accumulate, void* stream) {
  return vs_gemm_bf16_impl({.A = A, .lda = lda, .a_kmajor = a_kmajor, .B = B, .ldb = ldb, .b_kmajor = b_kmajor, .C = C, .ldc = ldc,
                            .M = M, .N = N, .K = K, .rowbias = rowbias, .ldrb = ldrb, .group = group, .accumulate = accumulate},
                           (hipStream_t)stream);
}

int vs_gemm_bf16_split(int a_kmajor, int b_kmajor, const void* A, int lda, const void* B, int ldb, float* C, float* C2, int ldc, int split_m,
                       int M, int N, int K, int accumulate, void* stream) {
  VS_REQUIRE(C2 && split_m > 0 && split_m < M, "gemm_bf16_split: needs C2 and 0 < split_m < M (split_m %d, M %d)", split_m, M);
  return vs_gemm_bf16_impl({.A = A, .lda = lda, .a_kmajor = a_kmajor, .B = B, .ldb = ldb, .b_kmajor = b_kmajor, .C = C, .ldc = ldc,
                            .C2 = C2, .split_m = split_m, .M = M, .N = N, .K = K, .accumulate = accumulate}, (hipStream_t)stream);
}

int vs_gemm_bf16_gated(int a_kmajor, int b_kmajor, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                       const float* gate, int ldg, void* stream) {
  VS_REQUIRE(gate != nullptr, "gemm_bf16_gated: gate is NULL");
  return vs_gemm_bf16_impl({.A = A, .lda = lda, .a_kmajor = a_kmajor, .B = B, .ldb = ldb, .b_kmajor = b_kmajor, .C = C, .ldc = ldc,
                            .M = M, .N = N, .K = K, .gate = gate, .ldg = ldg}, (hipStream_t)stream);
}

int vs_nhwc_conv_first(const float* x, const float* w, const float* scale, const float* shift, void* out,
                       int B, int T, int F, int act, double* bn_stats, void* stream) {
  return vs_nhwc_conv_first_impl(x, w, scale, shift, out, B, T, F, act, bn_stats, (hipStream_t)stream);
}

int vs_nhwc_bn_apply(const void* z, void* a, long long npix, int act, const float* scale, const float* shift, void* stream) {
  return vs_nhwc_bn_apply_impl(z, a, npix, act, scale, shift, (hipStream_t)stream);
}

// cnn1 by recomputation (nhwc_first.hip)
int vs_nhwc_first_moments(const float* x, int B, int T, int F, double* moments, void* stream) {
  return vs_nhwc_first_moments_impl(x, B, T, F, moments, (hipStream_t)stream);
}
int vs_nhwc_first_stats(const double* moments, const float* w, const float* bias, double count, double* stats, void* stream) {
  return vs_nhwc_first_stats_impl(moments, w, bias, count, stats, (hipStream_t)stream);
}
int vs_nhwc_first_bwd_scratch_doubles(void) { return VS_FIRST_BWD_SCRATCH_DOUBLES; }
int vs_nhwc_first_bwd(const void* da, const float* x, const float* w, const float* bias, int B, int T, int F, int act, int bn_mode,
                      const float* scale, const float* shift, const float* mean, const float* invstd,
                      float* dgamma, float* dbeta, float* dbias, float* dw, double* scratch, void* stream) {
  VS_REQUIRE(bn_mode == VS_BN_EVAL || bn_mode == VS_BN_TRAIN, "nhwc_first_bwd: unknown bn_mode %d", bn_mode);
  return vs_nhwc_first_bwd_impl(da, x, w, bias, B, T, F, act, bn_mode == VS_BN_TRAIN, scale, shift, mean, invstd, dgamma, dbeta, dbias, dw,
                                scratch, (hipStream_t)stream);
}

// train-mode BatchNorm2d between a conv that accumulated statistics and the apply pass (the piecewise form of what
// vs_forward_train does per layer)
int vs_bn_finalize(double* stats, int slots, double count, int C, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float eps, float momentum,
                   float* scale, float* shift, float* mean_out, float* invstd_out, void* stream) {
  VS_REQUIRE(eps >= 0.f && momentum >= 0.f && momentum <= 1.f, "bn_finalize: eps %g / momentum %g out of range", (double)eps, (double)momentum);
  VS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize: give both running buffers or neither");
  return vs_bn_finalize_impl(stats, slots, count, C, gamma, beta, running_mean, running_var, eps, momentum, scale, shift, mean_out, invstd_out,
                             (hipStream_t)stream);
}

int vs_nhwc_conv_last(const void* in, const float* w, const float* scale, const float* shift, float* out,
                      int B, int T, int F, int act, void* stream) {
  return vs_nhwc_conv_last_impl(in, w, scale, shift, out, B, T, F, act, (hipStream_t)stream);
}

// cnn8 on the un-normalised output z7 of cnn7: BatchNorm + activation of cnn7 applied on the way into the matrix pipe
int vs_nhwc_conv_last_pre(const void* z7, const float* pre_scale, const float* pre_shift, int pre_act, const float* w,
                          const float* scale, const float* shift, float* out, double* bn_stats, int B, int T, int F, void* stream) {
  VS_REQUIRE(pre_scale && pre_shift, "nhwc_conv_last_pre: NULL BatchNorm constants");
  return vs_nhwc_conv_last_impl(z7, w, scale, shift, out, B, T, F, VS_ACT_NONE, (hipStream_t)stream, bn_stats, pre_scale, pre_shift, pre_act);
}

size_t vs_nhwc_conv_wgrad_partial_floats(int KT, int KF) { return vs_nhwc_wgrad_partial_floats(KT, KF); }

int vs_nhwc_conv_wgrad(const void* dz, const void* in, float* partials, float* dw, int B, int T, int F, int KT, int KF, int dil,
                       void* stream) {
  return vs_nhwc_wgrad_impl(dz, in, partials, dw, B, T, F, KT, KF, dil, (hipStream_t)stream);
}

int vs_nhwc_bn_act_bwd(const void* da, const void* z, void* dz, long long npix, int act, int bn_mode,
                       const float* scale, const float* shift, const float* mean, const float* invstd,
                       float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, void* stream) {
  return vs_nhwc_bn_act_bwd_impl(da, z, dz, npix, act, bn_mode == VS_BN_TRAIN, scale, shift, mean, invstd, dgamma, dbeta, dbias,
                                 stats, coef, (hipStream_t)stream);
}

int vs_nhwc_bn_act_bwd_first(const void* da, const void* z, const float* x, int B, int T, int F, int act, int bn_mode,
                             const float* scale, const float* shift, const float* mean, const float* invstd,
                             float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc, void* stream) {
  return vs_nhwc_bn_act_bwd_first_impl(da, z, x, B, T, F, act, bn_mode == VS_BN_TRAIN, scale, shift, mean, invstd, dgamma, dbeta, dbias,
                                       dw, stats, coef, acc, (hipStream_t)stream);
}

int vs_nhwc_conv_last_bwd_blocks(void) { return VS_NHWC_LAST_BWD_BLOCKS; }

int vs_nhwc_conv_last_bwd(const float* dz8, const float* w, const void* a7, void* din, float* partials, float* dw,
                          int B, int T, int F, void* stream) {
  return vs_nhwc_conv_last_bwd_impl(dz8, w, a7, din, partials, dw, B, T, F, nullptr, VS_ACT_NONE, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    (hipStream_t)stream);
}

// ---- the dy forms: the producer of a data gradient also does the first pass of the BatchNorm backward below it ----
int vs_nhwc_conv_dy(const void* dz, const void* packed, void* dy, const void* z, int act,
                    const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd, double* bn_stats,
                    int B, int T, int F, int KT, int KF, int dil, void* stream) {
  VS_REQUIRE(dz != dy, "nhwc_conv_dy: in-place is not supported");
  return vs_nhwc_conv_dy_impl(dz, packed, dy, z, act, bn_scale, bn_shift, bn_mean, bn_invstd, bn_stats, B, T, F, KT, KF, dil, (hipStream_t)stream);
}

int vs_nhwc_conv_last_bwd_dy(const float* dz8, const float* w, const void* a7, void* dy, float* partials, float* dw,
                             const void* z7, int act, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                             const float* bn_invstd, double* bn_stats, int B, int T, int F, void* stream) {
  VS_REQUIRE(z7, "nhwc_conv_last_bwd_dy: NULL z7");
  return vs_nhwc_conv_last_bwd_impl(dz8, w, a7, dy, partials, dw, B, T, F, z7, act, bn_scale, bn_shift, bn_mean, bn_invstd, bn_stats,
                                    (hipStream_t)stream);
}

int vs_nhwc_bn_bwd_from_dy(const void* dy, const void* z, void* dz, long long npix, int bn_mode,
                           const float* scale, const float* mean, const float* invstd,
                           float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, void* stream) {
  return vs_nhwc_bn_bwd_from_dy_impl(dy, z, dz, npix, bn_mode == VS_BN_TRAIN, scale, mean, invstd, dgamma, dbeta, dbias, stats, coef,
                                     (hipStream_t)stream);
}

int vs_nhwc_bn_bwd_first_from_dy(const void* dy, const void* z, const float* x, int B, int T, int F, int bn_mode,
                                 const float* scale, const float* mean, const float* invstd,
                                 float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc, void* stream) {
  return vs_nhwc_bn_bwd_first_from_dy_impl(dy, z, x, B, T, F, bn_mode == VS_BN_TRAIN, scale, mean, invstd, dgamma, dbeta, dbias, dw,
                                           stats, coef, acc, (hipStream_t)stream);
}

int vs_conv_last_fwd(const float* in, const float* w, const float* scale, const float* shift, float* out,
                     int B, int T, int F, int act, void* stream) {
  return vs_conv_last_fwd_impl(in, w, scale, shift, out, B, T, F, act, (hipStream_t)stream);
}

int vs_gemm_nt(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
               const float* bias1, const float* bias2, const float* rowbias, int ldrb, int group,
               int a_relu, int act, void* stream) {
  return vs_gemm_impl({.A = A, .lda = lda, .a_relu = a_relu, .W = W, .ldw = ldw, .C = C, .ldc = ldc, .M = M, .N = N, .K = K,
                       .bias1 = bias1, .bias2 = bias2, .rowbias = rowbias, .ldrb = ldrb, .group = group, .act = act}, (hipStream_t)stream);
}

int vs_lstm_pack(const float* w_hh_fwd, const float* w_hh_bwd, float* packed, int H, void* stream) {
  return vs_lstm_pack_impl(w_hh_fwd, w_hh_bwd, packed, H, (hipStream_t)stream);
}

int vs_bilstm_recurrent(const float* xg, const float* packed_whh, float* state, float* out,
                        int B, int T, int H, void* stream) {
  return vs_bilstm_recurrent_impl(xg, packed_whh, state, out, nullptr, nullptr, B, T, H, (hipStream_t)stream);
}

// the same four calls with the arithmetic of the recurrent products chosen by the caller (what vs_forward* / vs_backward
// pass from dims.math): pack and recurrence must be given the same value
static int check_lstm_math(int math) {
  VS_REQUIRE(math == VS_MATH_FP32 || math == VS_MATH_F16X3 || math == VS_MATH_BF16, "lstm: unknown math %d", math);
  return 0;
}
int vs_lstm_pack_math(const float* w_hh_fwd, const float* w_hh_bwd, float* packed, int H, int math, void* stream) {
  if (int rc = check_lstm_math(math)) return rc;
  VS_REQUIRE(w_hh_fwd && w_hh_bwd && packed, "lstm_pack_math: NULL argument");
  return vs_lstm_pack_impl(w_hh_fwd, w_hh_bwd, packed, H, (hipStream_t)stream, math);
}
int vs_bilstm_recurrent_math(const float* xg, const float* packed_whh, float* state, float* out, float* gates_save, float* c_save,
                             int B, int T, int H, int math, void* stream) {
  if (int rc = check_lstm_math(math)) return rc;
  VS_REQUIRE(xg && packed_whh && state && out, "bilstm_recurrent_math: NULL argument");
  return vs_bilstm_recurrent_impl(xg, packed_whh, state, out, gates_save, c_save, B, T, H, (hipStream_t)stream, math);
}
int vs_lstm_pack_t_math(const float* w_hh_fwd, const float* w_hh_bwd, float* packed_t, int H, int math, void* stream) {
  if (int rc = check_lstm_math(math)) return rc;
  VS_REQUIRE(w_hh_fwd && w_hh_bwd && packed_t, "lstm_pack_t_math: NULL argument");
  return vs_lstm_pack_t_impl(w_hh_fwd, w_hh_bwd, packed_t, H, (hipStream_t)stream, math);
}
int vs_bilstm_recurrent_bwd_math(const float* packed_t, float* state, float* gates, const float* c_all, const float* dout,
                                 int B, int T, int H, int math, void* stream) {
  if (int rc = check_lstm_math(math)) return rc;
  VS_REQUIRE(packed_t && state && gates && c_all && dout, "bilstm_recurrent_bwd_math: NULL argument");
  return vs_bilstm_bwd_recurrent_impl(packed_t, state, gates, c_all, dout, B, T, H, (hipStream_t)stream, math);
}

int vs_zero_tail_rows(void* ptr, int B, int T, size_t row_bytes, const int* lengths, void* stream) {
  return vs_zero_tail_rows_impl(ptr, B, T, row_bytes, lengths, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// unit-test surface of the backward kernels (pass-through wrappers; the training schedule itself is train.hip)
// ---------------------------------------------------------------------------------------------
int vs_conv64_pack_dgrad(const float* w, float* packed, int KT, int KF, void* stream) {
  return vs_conv64_pack_impl(w, packed, KT, KF, 1, (hipStream_t)stream);
}

int vs_conv64_wgrad(const float* dz, const float* in, float* partials, float* dw, int B, int T, int F, int KT, int KF,
                    int dil, void* stream) {
  VS_REQUIRE(dz && in && partials && dw, "conv64_wgrad: NULL argument");
  return vs_conv64_wgrad_impl(dz, in, partials, dw, B, T, F, KT, KF, dil, (hipStream_t)stream);
}

int vs_conv64_wgrad_f16x3(const float* dz, const float* in, float* partials, float* dw, float* scratch8,
                          int B, int T, int F, int KT, int KF, int dil, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(dz && in && partials && dw && scratch8, "conv64_wgrad_f16x3: NULL argument");
  unsigned* amax = reinterpret_cast<unsigned*>(scratch8 + 4);
  if (int rc = vs_pow2_scale_impl(dz, (long long)B * 64 * T * F, amax, scratch8, stream)) return rc;
  if (int rc = vs_pow2_scale_impl(in, (long long)B * 64 * T * F, amax + 1, scratch8 + 2, stream)) return rc;
  return vs_conv64_wgrad_f16x3_impl(dz, in, scratch8, scratch8 + 2, partials, dw, B, T, F, KT, KF, dil, stream);
}

int vs_bn_act_bwd(const float* da, const float* z, float* dz, int C, long long R, int L, int act, int bn_mode,
                  const float* scale, const float* shift, const float* mean, const float* invstd,
                  float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, void* stream) {
  VS_REQUIRE(da && z && dz && scale && shift && mean && invstd && stats && coef, "bn_act_bwd: NULL argument");
  return vs_bn_act_bwd_impl(da, z, dz, C, R, L, act, bn_mode == VS_BN_TRAIN, scale, shift, mean, invstd, dgamma, dbeta, dbias,
                            stats, coef, nullptr, (hipStream_t)stream);
}

int vs_bn_act_bwd_first(const float* da, const float* z, const float* x, float* xpad, int B, int T, int F, int act, int bn_mode,
                        const float* scale, const float* shift, const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc, void* stream) {
  VS_REQUIRE(da && z && x && xpad && scale && shift && mean && invstd && dw && stats && coef && acc, "bn_act_bwd_first: NULL argument");
  return vs_bn_act_bwd_first_impl(da, z, x, xpad, B, T, F, act, bn_mode == VS_BN_TRAIN, scale, shift, mean, invstd, dgamma, dbeta, dbias,
                                  dw, stats, coef, acc, (hipStream_t)stream);
}

int vs_conv_last_dgrad(const float* dz, const float* w, float* din, int B, int T, int F, void* stream) {
  return vs_conv_last_dgrad_impl(dz, w, din, B, T, F, (hipStream_t)stream);
}

int vs_conv_last_wgrad(const float* dz, const float* in, float* partials, float* dw, int B, int T, int F, void* stream) {
  return vs_conv_last_wgrad_impl(dz, in, partials, dw, B, T, F, (hipStream_t)stream);
}

int vs_conv_first_wgrad(const float* dz, const float* x, double* acc, float* dw, int B, int T, int F, void* stream) {
  return vs_conv_first_wgrad_impl(dz, x, acc, dw, B, T, F, (hipStream_t)stream);
}

int vs_gemm(int layout_a, int layout_w, const float* A, int lda, const float* W, int ldw, float* C, int ldc,
            int M, int N, int K, const float* bias, const float* gate, int ldg, int a_relu, int w_relu, int act,
            int accumulate, int w_shift, int w_group, int splits, float* partials, void* stream) {
  VS_REQUIRE(A && W && C, "gemm: NULL argument");
  return vs_gemm_impl({.A = A, .lda = lda, .a_kmajor = layout_a, .a_relu = a_relu, .W = W, .ldw = ldw, .w_kmajor = layout_w, .w_relu = w_relu,
                       .C = C, .ldc = ldc, .accumulate = accumulate, .M = M, .N = N, .K = K, .bias1 = bias, .gate = gate, .ldg = ldg,
                       .act = act, .w_shift = w_shift, .w_group = w_group, .splits = splits, .partials = partials}, (hipStream_t)stream);
}

int vs_gemm_f16x3(int layout_a, int layout_w, const float* A, int lda, const float* W, int ldw, float* C, int ldc,
                  int M, int N, int K, const float* bias, const float* gate, int ldg, int a_relu, int w_relu, int act,
                  int accumulate, float* scratch8, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(A && W && C && scratch8, "gemm_f16x3: NULL argument");
  const VsGemm g{.arith = VS_GEMM_SPLIT_F16, .A = A, .lda = lda, .a_kmajor = layout_a, .a_relu = a_relu, .W = W, .ldw = ldw,
                 .w_kmajor = layout_w, .w_relu = w_relu, .C = C, .ldc = ldc, .accumulate = accumulate, .M = M, .N = N, .K = K, .bias1 = bias,
                 .gate = gate, .ldg = ldg, .act = act, .a_scale2 = scratch8, .w_scale2 = scratch8 + 2};
  if (int rc = vs_gemm_check(g)) return rc;      // a bad descriptor is refused before anything is enqueued
  unsigned* amax = reinterpret_cast<unsigned*>(scratch8 + 4);
  // the operands are dense [rows][ld] buffers here: scale over the whole buffers
  if (int rc = vs_pow2_scale_impl(A, (long long)(layout_a ? K : M) * lda, amax, scratch8, stream)) return rc;
  if (int rc = vs_pow2_scale_impl(W, (long long)(layout_w ? K : N) * ldw, amax + 1, scratch8 + 2, stream)) return rc;
  return vs_gemm_impl(g, stream);
}

int vs_bilstm_recurrent_train(const float* xg, const float* packed_whh, float* state, float* out, float* gates_save,
                              float* c_save, int B, int T, int H, void* stream) {
  return vs_bilstm_recurrent_impl(xg, packed_whh, state, out, gates_save, c_save, B, T, H, (hipStream_t)stream);
}

int vs_lstm_pack_t(const float* w_hh_fwd, const float* w_hh_bwd, float* packed_t, int H, void* stream) {
  return vs_lstm_pack_t_impl(w_hh_fwd, w_hh_bwd, packed_t, H, (hipStream_t)stream);
}

int vs_bilstm_recurrent_bwd(const float* packed_t, float* state, float* gates, const float* c_all, const float* dout,
                            int B, int T, int H, void* stream) {
  return vs_bilstm_bwd_recurrent_impl(packed_t, state, gates, c_all, dout, B, T, H, (hipStream_t)stream);
}

int vs_sigmoid_bwd(const float* dmask, const float* mask, float* dlogits, long long n, void* stream) {
  return vs_sigmoid_bwd_impl(dmask, mask, dlogits, n, (hipStream_t)stream);
}

int vs_colsum(const float* x, int ld, int groups, int rows, int N, float* out, int ldo, void* stream) {
  return vs_colsum_impl(x, ld, groups, rows, N, out, ldo, (hipStream_t)stream);
}

}  // extern "C"
