// Training orchestration: vs_forward_train (forward that keeps the tape) and vs_backward: two short
// drivers over per-stage functions.  Which kernel runs on which buffer, in which order -- no
// arithmetic lives here.  (The extern "C" unit-test surface of the backward kernels: capi.hip.)
//
// Reference graph being differentiated: models/voicesplit/model.py:66-89 (forward) as driven by
// train.py:94-110 (mask -> loss -> loss.backward()).
#include <mutex>
#include <stdlib.h>
#include <string.h>

#include "../../include/voicesplit_hip.h"
#include "vs_internal.h"

namespace {

constexpr int kSplitK = 16;    // split-K factor of the small weight-gradient GEMMs (fc1, fc2, W_hh)

inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

int tape_layout(const vs_dims* d, vs_tape_layout* L) {
  if (int rc = vs_check_dims_impl(d)) return rc;
  memset(L, 0, sizeof(*L));
  const size_t B = d->B, T = d->T, F = d->F, H = d->H, M = B * T;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  // conv activations: fp32 [B][64][T][F], or channels-last bf16 [B][T][F][64] in the bf16 configuration (half the bytes)
  const size_t act = B * 64 * T * F * (d->math == VS_MATH_BF16 ? 2 : 4);
  // (bf16 configuration: cnn1 is recomputed from x in the backward pass -- no z[0] tensor, round 4)
  for (int l = 0; l < 7; ++l) { L->z[l] = take(d->math == VS_MATH_BF16 && l == 0 ? 256 : act); L->a[l] = take(act); }
  L->z8 = take(M * 8 * F * 4);
  L->feat = take(M * 8 * F * 4);
  L->bn_scale = take(8 * 64 * 4);
  L->bn_shift = take(8 * 64 * 4);
  L->bn_mean = take(8 * 64 * 4);
  L->bn_invstd = take(8 * 64 * 4);
  L->gates = take(M * 8 * H * 4);
  L->cstate = take(M * 2 * H * 4);
  L->lstm_out = take(M * 2 * H * 4);
  L->fc1_out = take(M * (size_t)d->FC1 * 4);
  L->dlogits = take(M * (size_t)d->FC2 * 4);
  L->dfc1 = take(M * (size_t)d->FC1 * 4);
  L->dlstm_out = take(M * 2 * H * 4);
  L->dsum = take(B * 8 * H * 4);
  L->dfeat = take(M * 8 * F * 4);
  L->grad0 = take(act);
  L->grad1 = take(act);
  L->dvbias = take(B * 8 * H * 4);
  for (int i = 0; i < 6; ++i) L->conv_packed[i] = take(vs_conv64_packed_floats(kMid[i].kt, kMid[i].kf) * 4);
  L->pack_tmp = take(vs_conv64_packed_floats(5, 5) * 4);
  L->lstm_packed = take(vs_lstm_packed_floats(d->H) * 4);
  L->lstm_packed_t = take(vs_lstm_packed_t_floats(d->H) * 4);
  L->lstm_state = take(vs_lstm_state_floats(d->B, d->H) * 4);
  L->lstm_bwd_state = take(vs_lstm_bwd_state_floats(d->B, d->H) * 4);
  L->consts = take(128 * 4);
  L->bn_stats = take((size_t)VS_BN_STAT_SLOTS * 64 * 2 * 8);
  L->bn_coef = take(3 * 64 * 4);
  L->first_acc = take((64 + VS_FIRST_BWD_SCRATCH_DOUBLES) * 8);      // [cnn1's input moments (forward -> backward)][backward scratch]
  L->colsum_tmp = take(2 * B * max3(8 * H, d->FC1, d->FC2) * 4);      // two halves: the caller's stream, the side stream's leaves
  // one scratch region, reused by the stream-ordered consumers: conv wgrad partial sums,
  // cnn8 wgrad partials, split-K partials of the fc / W_hh weight gradients
  size_t part = vs_conv64_wgrad_partial_floats(5, 5);
  part = max3(part, vs_conv64_wgrad_partial_floats(7, 1), (size_t)vs_conv_last_wgrad_blocks() * 512);
  part = max3(part, (size_t)kSplitK * d->FC2 * d->FC1, (size_t)kSplitK * d->FC1 * 2 * H);
  part = max3(part, (size_t)kSplitK * 4 * H * H, (size_t)0);
  L->partials = take(part * 4);
  L->conv_scales = take(16 * VS_SCALE_SLOT_FLOATS * 4);
  L->gemm_scales = take(32 * 4);
  // bf16 configuration: feat / W_ih / dxg as bf16 arrays shared by the forward GEMM and the two backward contractions
  L->lstm_bf16 = take(d->math == VS_MATH_BF16 ? vs_lstm_bf16_layout((long long)M, 8 * (int)F, (int)H).total : 256);
  // (behind the turn words: the per-slot sums of cnn1's backward in deterministic mode, [VS_BN_STAT_SLOTS][576] doubles)
  L->det_turn = take(VS_TURN_WORDS * 4 + (size_t)VS_BN_STAT_SLOTS * 576 * 8);
  for (int i = 0; i < 6; ++i) L->conv_packed_t[i] = take(vs_conv64_packed_floats(kMid[i].kt, kMid[i].kf) * 4);
  L->total_bytes = off;
  return 0;
}

int check_tape(const vs_dims* d, void* tape, size_t bytes, vs_tape_layout* L) {
  if (int rc = tape_layout(d, L)) return rc;
  VS_REQUIRE(tape != nullptr, "tape is NULL");
  VS_REQUIRE((reinterpret_cast<uintptr_t>(tape) & 255) == 0, "tape must be 256-byte aligned");
  VS_REQUIRE(bytes >= L->total_bytes, "tape too small: %zu < %zu bytes", bytes, L->total_bytes);
  return 0;
}

int check_params(const vs_params* p) {
  VS_REQUIRE(p != nullptr, "params is NULL");
  for (int l = 0; l < 8; ++l) {
    const vs_conv_layer& c = p->conv[l];
    VS_REQUIRE(c.weight && c.bias && c.bn_weight && c.bn_bias && c.bn_running_mean && c.bn_running_var,
               "conv layer %d has a NULL parameter", l + 1);
  }
  for (int dir = 0; dir < 2; ++dir)
    VS_REQUIRE(p->w_ih[dir] && p->w_hh[dir] && p->b_ih[dir] && p->b_hh[dir], "NULL LSTM parameter (dir %d)", dir);
  VS_REQUIRE(p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "NULL head parameter");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Weight gradients on a side stream.  Layer l's weight gradient needs dz_l and the tape's a_{l-1}; nothing on the
// data-gradient chain (BatchNorm backward of layer l-1 -> data gradient of layer l-1 -> ...) needs ITS result.  It
// is a matrix-pipe kernel with one workgroup per CU and an idle memory system; the two BatchNorm backward passes
// of the next layer are pure HBM streams with idle matrix pipes (2.65 ms per layer, 16 ms per step).  So the weight
// gradient of layer l is launched on a second stream right after the data gradient of layer l and runs beside the
// BatchNorm backward of layer l-1; the data gradient of layer l-1 -- which overwrites dz_l -- waits for it.
// Same kernels, same order of every sum: results are bit-identical to the one-stream schedule.
// One side stream + event pair per device, created on first use; the caller's stream is joined before vs_backward
// returns, so the fork is invisible outside (and legal under stream capture).
// ---------------------------------------------------------------------------------------------
int g_bwd_overlap = 1;

struct SideStream { hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr, leaves = nullptr; };
SideStream g_side[16];
// One call's use of the side stream.  Every exit path after a fork -- the error returns included -- orders the caller's stream after
// what the side stream has been given (it writes gradients and the shared partial-sum scratch), and leaves no unjoined fork behind in
// a stream capture: fork() arms the guard, the wait that ends a join disarms it.  side == NULL is the one-stream schedule: every
// member is a no-op and to() is the caller's stream.
struct SideJoin {
  SideStream* side = nullptr;
  hipStream_t stream = nullptr;
  bool forked = false;
  hipStream_t to() const { return side ? side->s : stream; }
  // the side stream continues behind everything the caller's stream holds so far
  int fork() {
    if (!side) return 0;
    VS_CHECK_HIP(hipEventRecord(side->fork, stream));
    VS_CHECK_HIP(hipStreamWaitEvent(side->s, side->fork, 0));
    forked = true;
    return 0;
  }
  // the two halves of a join, for callers that have work for the caller's stream in between: mark() on the side stream ...
  int mark() {
    if (!side) return 0;
    VS_CHECK_HIP(hipEventRecord(side->join, side->s));
    return 0;
  }
  // ... and the caller's stream behind the last mark
  int wait() {
    if (!side) return 0;
    VS_CHECK_HIP(hipStreamWaitEvent(stream, side->join, 0));
    forked = false;
    return 0;
  }
  int join() {
    if (int rc = mark()) return rc;
    return wait();
  }
  ~SideJoin() {
    if (!side || !forked) return;
    if (hipEventRecord(side->join, side->s) == hipSuccess) (void)hipStreamWaitEvent(stream, side->join, 0);
  }
};
// the side stream and its events are shared by every caller on the device: one call enqueues at a time
// (host threads driving different caller streams would otherwise re-record an event another call is about to wait on)
std::mutex g_side_mutex;
// (not std::unique_lock: its lock() / unlock() are out-of-line template members that libstdc++ marks default-visible, i.e. they would
// become exports of the library -- tests/test_abi_cpu.py compares the dynamic symbol table with the header)
struct SideLock {
  bool held = false;
  void lock() { g_side_mutex.lock(); held = true; }
  void unlock() { if (held) { g_side_mutex.unlock(); held = false; } }
  ~SideLock() { unlock(); }
};
int side_stream(SideStream** out) {
  int dev = 0;
  VS_CHECK_HIP(hipGetDevice(&dev));
  VS_REQUIRE(dev >= 0 && dev < 16, "side stream: device index out of range");
  SideStream& ss = g_side[dev];
  if (!ss.s) {
    // [r6] LOW priority -- not for the priority but for the hardware queue.  HIP maps the streams of one priority onto a pool of (by
    // default four) hardware queues; a process that has initialised RCCL holds more normal-priority streams than that, and this
    // stream, created later, then SHARES a queue with the caller's stream: the two no longer run concurrently and every kernel of the
    // backward pass runs alone (46.2 -> 49.4-49.7 ms per step with the process group merely initialised: bench.py --force-collectives,
    // profiles/r06_experiments.md section 5).  A stream of another priority draws from another pool.  At N = 1 without RCCL the three
    // priorities measure the same within 0.1 ms (46.3 / 46.4 / 46.4 ms normal / high / low, two rounds in one call); what runs here --
    // weight gradients, leaves, weight packs -- is off the critical path by construction.
    int lo = 0, hi = 0;                                  // (numerically: hi <= lo, lo = the least priority)
    VS_CHECK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    VS_CHECK_HIP(hipStreamCreateWithPriority(&ss.s, hipStreamNonBlocking, lo));
    VS_CHECK_HIP(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
    VS_CHECK_HIP(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming));
    VS_CHECK_HIP(hipEventCreateWithFlags(&ss.leaves, hipEventDisableTiming));
  }
  *out = &ss;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// One training call's context: what both passes read off the dims, the parameters and the tape.  Built once behind the
// validation; the stage functions below take it by const reference.
// ---------------------------------------------------------------------------------------------
struct BnConsts { float *scale, *shift, *mean, *invstd; };
struct Step {
  const vs_dims* d;
  const vs_params* p;
  void* tape;
  vs_tape_layout L;
  hipStream_t stream;      // the caller's
  int conv_act;
  bool train;              // BatchNorm on batch statistics
  bool nhwc;               // BASELINE configs[2]: the channels-last bf16 configuration (VS_MATH_BF16); else the NCHW route (fp32, split-f16)
  bool det;                // deterministic mode (bf16 configuration): the turn words of this tape
  // the mask head as ONE launch (head_fused.hip): the weights' fragment images go into the backward pass's partial-sum scratch, idle
  // during the forward pass.  Decided here, once: weight_images() packs the image, head() consumes it.
  bool head_fused;
  int B, T, F, H, M, K8, KE;
  VsLstmBf16Layout lb;     // bf16 configuration: feat / W_ih / dxg as bf16 arrays inside L.lstm_bf16
  float *ones, *zeros;     // [64] each
  double* stats;
  float *coef, *part;
  float* cs;               // split-f16 convs: the conv scale slots (slot l: input of conv index l; slot 8 + l: dz of conv index l)
  template <typename T>
  T* at(size_t off) const { return ::at<T>(tape, off); }
  BnConsts bn(int l) const {
    return {at<float>(L.bn_scale) + 64 * l, at<float>(L.bn_shift) + 64 * l, at<float>(L.bn_mean) + 64 * l, at<float>(L.bn_invstd) + 64 * l};
  }
  unsigned* turn() const { return det ? at<unsigned>(L.det_turn) : nullptr; }
};

Step make_step(const vs_dims* d, const vs_params* p, void* tape, const vs_tape_layout& L, int conv_act, int bn_mode, hipStream_t stream) {
  Step st;
  st.d = d; st.p = p; st.tape = tape; st.L = L; st.stream = stream; st.conv_act = conv_act;
  st.train = bn_mode == VS_BN_TRAIN;
  st.nhwc = d->math == VS_MATH_BF16;
  st.det = st.nhwc && vs_opt(VS_OPT_DETERMINISTIC) != 0;
  st.head_fused = st.nhwc && vs_head_fused_supported(2 * d->H, d->FC1, d->FC2) &&
                  L.conv_scales - L.partials >= vs_head_fused_packed_bytes(2 * d->H, d->FC1, d->FC2);
  st.B = d->B; st.T = d->T; st.F = d->F; st.H = d->H;
  st.M = d->B * d->T; st.K8 = 8 * d->F; st.KE = st.K8 + d->E;
  st.lb = vs_lstm_bf16_layout((long long)st.M, st.K8, st.H);
  st.ones = st.at<float>(L.consts);
  st.zeros = st.ones + 64;
  st.stats = st.at<double>(L.bn_stats);
  st.coef = st.at<float>(L.bn_coef);
  st.part = st.at<float>(L.partials);
  st.cs = st.at<float>(L.conv_scales);
  return st;
}

// ---------------------------------------------------------------------------------------------
// forward stages
// ---------------------------------------------------------------------------------------------
// The forward's statistics scratch is cleared ONCE (by arm); every finalize folds the slots and clears this much of the scratch behind
// itself in the same launch (vs_fold_slots): no memset kernel in front of the conv launches.
constexpr int kFwdStatsDoubles = VS_BN_STAT_SLOTS * 128;

// One launch in front of the bf16 forward pass: ones[64] = 1, zeros[64] = 0, up to three scratch arrays cleared (16-byte granules).
struct ArmArgs { float* ones; void* z[3]; unsigned n16[3]; };
__global__ __launch_bounds__(256)
void forward_arm_kernel(ArmArgs a) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i < 64) { a.ones[i] = 1.f; a.ones[64 + i] = 0.f; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    if (i < a.n16[r]) reinterpret_cast<uint4*>(a.z[r])[i] = make_uint4(0u, 0u, 0u, 0u);
}

int arm(const Step& st) {
  if (st.nhwc) {
    // [r6] the constants and every scratch array the pass wants cleared, in ONE launch (they were six runtime fill dispatches, 54 us in
    // front of the first kernel of the step: tools/dispatch_census.py).  Deterministic mode: the turn words of this tape are armed
    // here; every launch that takes turns re-arms its own.
    ArmArgs a{st.ones, {st.stats, st.at<void>(st.L.first_acc), st.turn()},
              {VS_BN_STAT_SLOTS * 128 * 8 / 16, 64 * 8 / 16, (unsigned)(st.det ? VS_TURN_WORDS * 4 / 16 : 0)}};
    unsigned most = 8;
    for (unsigned n : a.n16) most = n > most ? n : most;
    hipLaunchKernelGGL(forward_arm_kernel, dim3((most + 255) / 256), dim3(256), 0, st.stream, a);
    return 0;
  }
  VS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st.ones), 0x3f800000 /* 1.0f */, 64, st.stream));
  VS_CHECK_HIP(hipMemsetAsync(st.zeros, 0, 64 * sizeof(float), st.stream));
  // split-f16 convs: the BatchNorm+activation pass that produces a layer's input also folds its |max| into that layer's scale slot
  if (st.d->math == VS_MATH_F16X3) VS_CHECK_HIP(hipMemsetAsync(st.cs, 0, 16 * VS_SCALE_SLOT_FLOATS * sizeof(float), st.stream));
  return 0;
}

// the d-vector folded into a per-utterance row bias of the LSTM input projection (one direction)
int dvec_bias(const Step& st, const float* dvec, int dir, hipStream_t s) {
  const vs_params* p = st.p;
  return vs_gemm_impl({.A = dvec, .lda = st.d->E, .W = p->w_ih[dir] + st.K8, .ldw = st.KE,
                       .C = st.at<float>(st.L.dvbias) + (size_t)dir * 4 * st.H, .ldc = 8 * st.H, .M = st.B, .N = 4 * st.H, .K = st.d->E,
                       .bias1 = p->b_ih[dir], .bias2 = p->b_hh[dir]}, s);
}

// ---- the weight-only work of a bf16 step ------------------------------------------------------------------------------------------
// Packing the six conv weights, the bf16 copy of W_ih, the d-vector fold, the recurrent and head weight images depend on nothing the
// conv stack produces: 14 launches of 5-45 us that used to sit, with their launch gaps, in front of their consumers on the one
// stream (~0.25 ms of a step).  With the prologue on they run on the side stream beside cnn1 and the caller's stream joins in front
// of cnn2; with it off they are the first launches on the caller's stream.
int weight_images(const Step& st, const float* dvec, hipStream_t s) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  for (int i = 0; i < 6; ++i)
    if (int rc = vs_nhwc_pack_impl(p->conv[i + 1].weight, st.at<void>(L.conv_packed[i]), kMid[i].kt, kMid[i].kf, 0, s)) return rc;
  // [r6] the backward pass's weight images too (same weights, idle side stream): they were 0.1 ms on the backward's critical path
  for (int i = 0; i < 6; ++i)
    if (int rc = vs_nhwc_pack_impl(p->conv[i + 1].weight, st.at<void>(L.conv_packed_t[i]), kMid[i].kt, kMid[i].kf, 1, s)) return rc;
  if (int rc = vs_lstm_pack_t_impl(p->w_hh[0], p->w_hh[1], st.at<float>(L.lstm_packed_t), st.H, s, st.d->math)) return rc;
  for (int dir = 0; dir < 2; ++dir) {
    if (int rc = dvec_bias(st, dvec, dir, s)) return rc;
    if (int rc = vs_cvt_rows_bf16_impl(p->w_ih[dir], 4 * st.H, st.K8, st.KE, st.at<char>(L.lstm_bf16) + st.lb.wih + (size_t)dir * 4 * st.H * st.lb.Kp * 2,
                                       st.lb.Kp, s)) return rc;
  }
  if (int rc = vs_lstm_pack_impl(p->w_hh[0], p->w_hh[1], st.at<float>(L.lstm_packed), st.H, s, st.d->math)) return rc;
  if (st.head_fused) {
    if (int rc = vs_head_fused_pack_impl(p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, 2 * st.H, st.d->FC1, st.d->FC2, st.part, s)) return rc;
  }
  return 0;
}

// cnn1 of the bf16 configuration, by recomputation: the batch statistics of z1 = conv(x) + bias from the 35 moments of the input's
// seven shifts (one pass over the 46 MB input), then ONE pass that writes a1 = act(BN(z1)): no z1 tensor, no apply pass (nhwc_first.hip)
int cnn1_nhwc(const Step& st, const float* x) {
  VsProfScope ps(VS_PROF_CNN1, st.stream);
  const vs_conv_layer& c = st.p->conv[0];
  const BnConsts k = st.bn(0);
  const double npix = (double)((long long)st.B * st.T * st.F);
  // (the moments stay in the tape for the backward pass: first_acc = [35 moments, padded to 64][backward scratch])
  double* mom = st.at<double>(st.L.first_acc);
  // (deterministic mode: per-slot sums in the backward pass's dfeat buffer, which nothing uses before the loss)
  if (int rc = vs_nhwc_first_moments_impl(x, st.B, st.T, st.F, mom, st.stream, st.det ? st.at<double>(st.L.dfeat) : nullptr, /*mom_is_zero=*/1)) return rc;
  if (st.train) {
    if (int rc = vs_nhwc_first_stats_impl(mom, c.weight, c.bias, npix, st.stats, st.stream)) return rc;
    if (int rc = vs_bn_finalize_impl(st.stats, 1, npix, 64, c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, kBnEps,
                                     kBnMomentum, k.scale, k.shift, k.mean, k.invstd, st.stream, kFwdStatsDoubles)) return rc;
  } else {
    if (int rc = vs_bn_eval_consts_impl(c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, kBnEps, 64, k.scale, k.shift, k.mean, k.invstd, st.stream)) return rc;
  }
  return vs_nhwc_conv_first_impl(x, c.weight, k.scale, k.shift, st.at<void>(st.L.a[0]), st.B, st.T, st.F, st.conv_act, nullptr, st.stream, c.bias);
}

// cnn2 .. cnn8 on channels-last bf16 z / a (conv_nhwc.hip, nhwc_bn.hip, nhwc_last.hip); statistics from the conv epilogues
int convs_nhwc(const Step& st) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  const int B = st.B, T = st.T, F = st.F;
  const long long npix = (long long)B * T * F;
  for (int i = 0; i < 6; ++i) {
    const int l = i + 1;
    const vs_conv_layer& c = p->conv[l];
    const BnConsts k = st.bn(l);
    {
      VsProfScope ps(VS_PROF_CNN2 + i, st.stream);
      if (int rc = vs_nhwc_conv_impl(st.at<void>(L.a[l - 1]), st.at<void>(L.conv_packed[i]), st.ones, c.bias, st.at<void>(L.z[l]), B, T, F,
                                     kMid[i].kt, kMid[i].kf, kMid[i].dil, VS_ACT_NONE, st.train ? st.stats : nullptr, st.stream)) return rc;
    }
    VsProfScope ps(VS_PROF_FWD_BN, st.stream);
    if (st.train) {
      if (int rc = vs_bn_finalize_impl(st.stats, VS_BN_STAT_SLOTS, (double)npix, 64, c.bn_weight, c.bn_bias, c.bn_running_mean,
                                       c.bn_running_var, kBnEps, kBnMomentum, k.scale, k.shift, k.mean, k.invstd, st.stream, kFwdStatsDoubles)) return rc;
      // cnn7's BatchNorm + activation is applied by its consumer: cnn8 is an HBM-bound kernel with idle VALU (forward: on the
      // way into its matrix pipe; backward: recomputed beside the derivative), so train mode has no apply pass over z7
      // and no a7 tensor.  Everything else -- finalize, running statistics, the constants -- stays.
      if (l == 6) continue;
    } else {
      if (int rc = vs_bn_eval_consts_impl(c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, kBnEps, 64, k.scale, k.shift, k.mean, k.invstd, st.stream)) return rc;
    }
    if (int rc = vs_nhwc_bn_apply_impl(st.at<void>(L.z[l]), st.at<void>(L.a[l]), npix, st.conv_act, k.scale, k.shift, st.stream)) return rc;
  }
  VsProfScope ps(VS_PROF_CNN8, st.stream);
  const vs_conv_layer& c = p->conv[7];
  if (!st.train) return vs_nhwc_conv_last_impl(st.at<void>(L.a[6]), c.weight, st.ones, c.bias, st.at<float>(L.z8), B, T, F, VS_ACT_NONE, st.stream);
  const BnConsts k7 = st.bn(6);
  return vs_nhwc_conv_last_impl(st.at<void>(L.z[6]), c.weight, st.ones, c.bias, st.at<float>(L.z8), B, T, F, VS_ACT_NONE, st.stream,
                                st.stats, k7.scale, k7.shift, st.conv_act);
}

// BatchNorm + activation over an fp32 tensor, z -> a (both kept): the NCHW route's layers, and the features of a bf16 eval-mode forward
int bn_fp32(const Step& st, int l, const float* z, float* a, int C, bool feat_layout, int stats_slots = 0) {
  VsProfScope ps(VS_PROF_FWD_BN, st.stream);
  const vs_conv_layer& c = st.p->conv[l];
  const BnConsts k = st.bn(l);
  const int B = st.B, T = st.T, F = st.F;
  unsigned* amax = (st.d->math == VS_MATH_F16X3 && l + 1 <= 6) ? vs_amax_slot(st.cs + VS_SCALE_SLOT_FLOATS * (l + 1)) : nullptr;
  if (st.train) {
    return feat_layout
               ? vs_bn_train_feat_impl(z, a, B, T, F, c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, kBnEps,
                                       kBnMomentum, st.conv_act, st.stats, k.scale, k.shift, k.mean, k.invstd, st.stream)
               : vs_bn_train_impl(z, a, B, C, T * F, c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, kBnEps,
                                  kBnMomentum, st.conv_act, st.stats, k.scale, k.shift, k.mean, k.invstd, amax, st.stream, stats_slots);
  }
  if (int rc = vs_bn_eval_consts_impl(c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var, kBnEps, C, k.scale, k.shift, k.mean, k.invstd, st.stream)) return rc;
  return feat_layout ? vs_bn_apply_feat_impl(z, a, B, T, F, st.conv_act, k.scale, k.shift, st.stream)
                     : vs_bn_apply_impl(z, a, B, C, T * F, st.conv_act, k.scale, k.shift, amax, st.stream);
}

// cnn1 .. cnn8 of the NCHW route (fp32, split-f16): conv + bias -> z (kept), then BatchNorm + activation -> a (kept)
int convs_nchw(const Step& st, const float* x) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  const int B = st.B, T = st.T, F = st.F;
  {
    VsProfScope ps(VS_PROF_CNN1, st.stream);
    if (int rc = vs_conv_first_fwd_impl(x, p->conv[0].weight, st.ones, p->conv[0].bias, st.at<float>(L.z[0]), B, T, F, VS_ACT_NONE, nullptr, st.stream)) return rc;
  }
  if (int rc = bn_fp32(st, 0, st.at<float>(L.z[0]), st.at<float>(L.a[0]), 64, false)) return rc;
  // batch statistics of z accumulated by the conv epilogue itself (split-f16 kernels): one pass less over z
  const bool fuse = st.train && st.d->math == VS_MATH_F16X3;
  for (int i = 0; i < 6; ++i) {
    const int l = i + 1;
    {
      VsProfScope ps(VS_PROF_CNN2 + i, st.stream);
      if (fuse) VS_CHECK_HIP(hipMemsetAsync(st.stats, 0, sizeof(double) * VS_BN_STAT_SLOTS * 128, st.stream));
      if (int rc = vs_conv64_layer_impl(st.d->math, st.at<float>(L.a[l - 1]), p->conv[l].weight, st.at<float>(L.conv_packed[i]),
                                        st.cs + VS_SCALE_SLOT_FLOATS * l, 1, st.ones, p->conv[l].bias, st.at<float>(L.z[l]),
                                        B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, VS_ACT_NONE, 0, nullptr, st.stream,
                                        fuse ? st.stats : nullptr)) return rc;
    }
    if (int rc = bn_fp32(st, l, st.at<float>(L.z[l]), st.at<float>(L.a[l]), 64, false, fuse ? VS_BN_STAT_SLOTS : 0)) return rc;
  }
  VsProfScope ps(VS_PROF_CNN8, st.stream);
  return vs_conv_last_fwd_impl(st.at<float>(L.a[6]), p->conv[7].weight, st.ones, p->conv[7].bias, st.at<float>(L.z8), B, T, F, VS_ACT_NONE, st.stream);
}

// cnn8's BatchNorm + activation: z8 -> feat.  Returns (through feat_bf16_ready) whether the bf16 rows of feat were written as well.
int features_bn(const Step& st, bool* feat_bf16_ready) {
  const vs_tape_layout& L = st.L;
  *feat_bf16_ready = st.nhwc && st.train;
  if (!*feat_bf16_ready) return bn_fp32(st, 7, st.at<float>(L.z8), st.at<float>(L.feat), 8, true);
  // cnn8's batch statistics came out of its own epilogue: finalize + the apply pass
  VsProfScope ps(VS_PROF_FWD_BN, st.stream);
  const vs_conv_layer& c = st.p->conv[7];
  const BnConsts k = st.bn(7);
  if (int rc = vs_bn_finalize_impl(st.stats, VS_BN_STAT_SLOTS, (double)st.B * st.T * st.F, 8, c.bn_weight, c.bn_bias, c.bn_running_mean, c.bn_running_var,
                                   kBnEps, kBnMomentum, k.scale, k.shift, k.mean, k.invstd, st.stream, kFwdStatsDoubles)) return rc;
  // ... which also writes the bf16 row-form copy of the features the LSTM GEMMs read
  return vs_bn_apply_feat_bf16_impl(st.at<float>(L.z8), st.at<float>(L.feat), st.at<char>(L.lstm_bf16) + st.lb.feat, st.lb.Kp, st.B, st.T, st.F, st.conv_act,
                                    k.scale, k.shift, st.stream);
}

// BiLSTM (d-vector folded into a per-utterance row bias), gates and cell states kept
int lstm(const Step& st, const float* dvec, bool feat_bf16_ready) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  float* xg = st.at<float>(L.gates);
  float* packed = st.at<float>(L.lstm_packed);
  {
    VsProfScope ps(VS_PROF_LSTM_GEMM, st.stream);
    // The NCHW route has no weight_images(): its d-vector fold and its recurrent weight image are issued here, around the contraction.
    // The backward pass's gradient buffers are idle during the forward pass: the contraction's operand scratch.  bf16 configuration:
    // the bf16 W_ih is already in its place in the tape (weight_images) -- handed over as "prepared" so that it is not converted again.
    if (!st.nhwc) {
      for (int dir = 0; dir < 2; ++dir)
        if (int rc = dvec_bias(st, dvec, dir, st.stream)) return rc;
    }
    VsLstmGemmReady ready;
    ready.wh = st.nhwc ? reinterpret_cast<const _Float16*>(st.at<char>(L.lstm_bf16) + st.lb.wih) : nullptr;
    ready.feat_bf16 = feat_bf16_ready;
    if (int rc = vs_lstm_input_gemm_impl(st.d->math, st.at<float>(L.feat), st.K8, p->w_ih[0], p->w_ih[1], st.H, st.KE, xg, st.M, st.at<float>(L.dvbias), st.T,
                                         st.at<float>(L.gemm_scales), st.nhwc ? st.at<char>(L.lstm_bf16) : st.at<char>(L.grad0),
                                         st.nhwc ? L.total_bytes - L.lstm_bf16 : 2 * (L.grad1 - L.grad0), st.stream, ready)) return rc;
  }
  if (!st.nhwc) {
    if (int rc = vs_lstm_pack_impl(p->w_hh[0], p->w_hh[1], packed, st.H, st.stream, st.d->math)) return rc;
  }
  VsProfScope ps(VS_PROF_LSTM_REC, st.stream);
  return vs_bilstm_recurrent_impl(xg, packed, st.at<float>(L.lstm_state), st.at<float>(L.lstm_out), xg, st.at<float>(L.cstate), st.B, st.T, st.H,
                                  st.stream, st.d->math);
}

// relu -> fc1 -> relu -> fc2 -> sigmoid (models/voicesplit/model.py:83-87)
int head(const Step& st, float* mask) {
  VsProfScope ps(VS_PROF_HEAD, st.stream);
  const vs_params* p = st.p;
  const int H = st.H, FC1 = st.d->FC1, FC2 = st.d->FC2;
  float* lstm_out = st.at<float>(st.L.lstm_out);
  float* h1 = st.at<float>(st.L.fc1_out);
  // one launch, h1 in registers between the two contractions and stored once for the backward pass (head_fused.hip)
  if (st.head_fused) return vs_head_fused_impl(lstm_out, st.part, h1, nullptr, mask, st.M, 2 * H, FC1, FC2, st.stream);
  const VsGemmArith arith = st.nhwc ? VS_GEMM_FP32_BF16 : VS_GEMM_FP32;
  if (int rc = vs_gemm_impl({.arith = arith, .A = lstm_out, .lda = 2 * H, .a_relu = 1, .W = p->fc1_w, .ldw = 2 * H, .C = h1, .ldc = FC1,
                             .M = st.M, .N = FC1, .K = 2 * H, .bias1 = p->fc1_b, .act = VS_ACT_RELU}, st.stream)) return rc;
  return vs_gemm_impl({.arith = arith, .A = h1, .lda = FC1, .W = p->fc2_w, .ldw = FC1, .C = mask, .ldc = FC2,
                       .M = st.M, .N = FC2, .K = FC1, .bias1 = p->fc2_b, .act = VS_ACT_SIGMOID}, st.stream);
}

// ---------------------------------------------------------------------------------------------
// backward stages
// ---------------------------------------------------------------------------------------------
// The bf16 backward keeps the two-kernel BatchNorm-backward finalize and a memset of the statistics scratch in front of every dy
// launch (0 = nothing is cleared behind a finalize): the fused form (one launch that folds, finalizes and clears) measured +1.6 ms
// per step beside a 2048-block BatchNorm pass and neutral beside the one-block-per-CU pass (round 5: profiles/r05_experiments.md
// section 2 and its last paragraph; re-measured in round 6, call 12: 46.85 ms either way, three alternating runs).
constexpr int kBwdFinalizeClearsDoubles = 0;

// sigmoid, fc2, relu, fc1, relu (models/voicesplit/model.py:83-87 backwards)
int head_bwd(const Step& st, SideJoin& sj, const float* mask, const float* dmask, const vs_grads* g) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  hipStream_t stream = st.stream;
  const int B = st.B, T = st.T, H = st.H, M = st.M, FC1 = st.d->FC1, FC2 = st.d->FC2;
  float* dlogits = st.at<float>(L.dlogits);
  float* h1 = st.at<float>(L.fc1_out);
  float* dfc1 = st.at<float>(L.dfc1);
  float* lstm_out = st.at<float>(L.lstm_out);
  float* dlstm = st.at<float>(L.dlstm_out);
  float* tmp = st.at<float>(L.colsum_tmp);
  VsProfScope ps(VS_PROF_BWD_HEAD, stream);
  // VS_MATH_BF16: the four head contractions on bf16-rounded operands (fp32 accumulate, fp32 split-K partials)
  const VsGemmArith arith = st.nhwc ? VS_GEMM_FP32_BF16 : VS_GEMM_FP32;
  // [r5] The two weight gradients of the head are leaves: with VS_OPT_HEAD_LEAF_SIDE they go to the side stream, where they run beside
  // the BPTT -- a latency-bound launch that leaves the CUs' arithmetic idle -- instead of in front of it (same kernels, same sums).
  const bool leaf_side = sj.side != nullptr && vs_opt(VS_OPT_HEAD_LEAF_SIDE) != 0;
  hipStream_t hs = leaf_side ? sj.side->s : stream;
  // [r5] The two data-gradient contractions of the head (the serial ones) on gemm_bf16.hip's kernel: bf16 row copies of dlogits / dfc1
  // and bf16 copies of the two weights in the idle gradient buffer of the conv stack (its backward has not begun), the relu mask in
  // the epilogue.  Same operand roundings as the generic kernel's in-flight conversion.
  const int K2p = (FC2 + 63) / 64 * 64, K1p = (FC1 + 63) / 64 * 64, N1p = (FC1 + 7) / 8 * 8, N2p = (2 * H + 7) / 8 * 8;
  const size_t o_df = align_up((size_t)M * K2p * 2), o_w2 = o_df + align_up((size_t)M * K1p * 2), o_w1 = o_w2 + align_up((size_t)FC2 * N1p * 2);
  const size_t head_need = o_w1 + align_up((size_t)FC1 * N2p * 2);
  const bool head_bf16 = st.nhwc && vs_opt(VS_OPT_HEAD_BWD_GEMM) != 0 && FC1 % 4 == 0 && (2 * H) % 4 == 0 && head_need <= L.grad1 - L.grad0;
  char* hb = st.at<char>(L.grad0);
  // the bias gradients (column sums) are leaves as well: on the side stream they use the second half of the column-sum scratch
  float* tmp_leaf = leaf_side ? tmp + (size_t)B * max3(8 * H, FC1, FC2) : tmp;
  // dfc1 = (dlogits @ W2) * (h1 > 0)
  if (head_bf16) {
    if (int rc = vs_cvt_rows_bf16_impl(p->fc2_w, FC2, FC1, FC1, hb + o_w2, N1p, stream)) return rc;
    if (int rc = vs_cvt_rows_bf16_impl(p->fc1_w, FC1, 2 * H, 2 * H, hb + o_w1, N2p, stream)) return rc;
    if (int rc = vs_sigmoid_bwd_rows_impl(dmask, mask, dlogits, M, FC2, hb, K2p, stream)) return rc;
    if (int rc = vs_gemm_bf16_impl({.A = hb, .lda = K2p, .B = hb + o_w2, .ldb = N1p, .b_kmajor = 1, .C = dfc1, .ldc = FC1,
                                    .M = M, .N = FC1, .K = FC2, .gate = h1, .ldg = FC1}, stream)) return rc;
  } else {
    if (int rc = vs_sigmoid_bwd_impl(dmask, mask, dlogits, (long long)M * FC2, stream)) return rc;
    if (int rc = vs_gemm_impl({.arith = arith, .A = dlogits, .lda = FC2, .W = p->fc2_w, .ldw = FC1, .w_kmajor = 1, .C = dfc1, .ldc = FC1,
                               .M = M, .N = FC1, .K = FC2, .gate = h1, .ldg = FC1}, stream)) return rc;
  }
  if (leaf_side) { if (int rc = sj.fork()) return rc; }
  if (int rc = vs_colsum_impl(dlogits, FC2, B, T, FC2, tmp_leaf, FC2, hs)) return rc;
  if (int rc = vs_colsum_impl(tmp_leaf, FC2, 1, B, FC2, g->fc2_b, FC2, hs)) return rc;
  // dW2 = dlogits^T @ h1
  if (int rc = vs_gemm_impl({.arith = arith, .A = dlogits, .lda = FC2, .a_kmajor = 1, .W = h1, .ldw = FC1, .w_kmajor = 1,
                             .C = g->fc2_w, .ldc = FC1, .M = FC2, .N = FC1, .K = M, .splits = kSplitK, .partials = st.part}, hs)) return rc;
  if (int rc = vs_colsum_impl(dfc1, FC1, B, T, FC1, tmp_leaf, FC1, hs)) return rc;
  if (int rc = vs_colsum_impl(tmp_leaf, FC1, 1, B, FC1, g->fc1_b, FC1, hs)) return rc;
  // dW1 = dfc1^T @ relu(lstm_out)
  if (int rc = vs_gemm_impl({.arith = arith, .A = dfc1, .lda = FC1, .a_kmajor = 1, .W = lstm_out, .ldw = 2 * H, .w_kmajor = 1, .w_relu = 1,
                             .C = g->fc1_w, .ldc = 2 * H, .M = FC1, .N = 2 * H, .K = M, .splits = kSplitK, .partials = st.part}, hs)) return rc;
  // dlstm_out = (dfc1 @ W1) * (lstm_out > 0)
  if (head_bf16) {
    if (int rc = vs_cvt_rows_bf16_impl(dfc1, M, FC1, FC1, hb + o_df, K1p, stream)) return rc;
    return vs_gemm_bf16_impl({.A = hb + o_df, .lda = K1p, .B = hb + o_w1, .ldb = N2p, .b_kmajor = 1, .C = dlstm, .ldc = 2 * H,
                              .M = M, .N = 2 * H, .K = FC1, .gate = lstm_out, .ldg = 2 * H}, stream);
  }
  return vs_gemm_impl({.arith = arith, .A = dfc1, .lda = FC1, .W = p->fc1_w, .ldw = 2 * H, .w_kmajor = 1, .C = dlstm, .ldc = 2 * H,
                       .M = M, .N = 2 * H, .K = FC1, .gate = lstm_out, .ldg = 2 * H}, stream);
}

// BiLSTM: back-propagation through time; the gate gradients replace the gates in the tape
int bptt(const Step& st) {
  const vs_tape_layout& L = st.L;
  float* wpt = st.at<float>(L.lstm_packed_t);
  // (bf16 configuration: vs_forward_train left the image in the tape [r6])
  if (!st.nhwc) { if (int rc = vs_lstm_pack_t_impl(st.p->w_hh[0], st.p->w_hh[1], wpt, st.H, st.stream, st.d->math)) return rc; }
  VsProfScope ps(VS_PROF_BWD_LSTM_REC, st.stream);
  return vs_bilstm_bwd_recurrent_impl(wpt, st.at<float>(L.lstm_bwd_state), st.at<float>(L.gates), st.at<float>(L.cstate), st.at<float>(L.dlstm_out),
                                      st.B, st.T, st.H, st.stream, st.d->math);
}

// The LSTM's parameter gradients (dW_ih, dW_hh, biases, d-vector), on the side stream when there is one: leaves, nothing down the
// conv stack needs them.
int lstm_leaves(const Step& st, const SideJoin& sj, const float* dvec, const vs_grads* g) {
  hipStream_t ls = sj.to();
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  const int B = st.B, T = st.T, H = st.H, M = st.M, K8 = st.K8, KE = st.KE, E = st.d->E;
  const bool f16x3 = st.d->math == VS_MATH_F16X3;
  float* dxg = st.at<float>(L.gates);
  float* dsum = st.at<float>(L.dsum);
  float* feat = st.at<float>(L.feat);
  float* lstm_out = st.at<float>(L.lstm_out);
  float* tmp = st.at<float>(L.colsum_tmp);
  float* gsc = st.at<float>(L.gemm_scales);
  char* bfb = st.at<char>(L.lstm_bf16);
  // bf16 configuration: dW_ih[:, :8F] of both directions in one col x col contraction over K = B*T: rows < 4H -> dW_ih, the rest -> dW_ih_reverse
  auto dwih_bf16 = [&]() -> int {
    return vs_gemm_bf16_impl({.A = bfb + st.lb.dxg, .lda = 8 * H, .a_kmajor = 1, .B = bfb + st.lb.feat, .ldb = st.lb.Kp, .b_kmajor = 1,
                              .C = g->w_ih[0], .ldc = KE, .C2 = g->w_ih[1], .split_m = 4 * H, .M = 8 * H, .N = K8, .K = M}, ls);
  };
  // [r5] on a side stream it goes LAST: one persistent workgroup per CU, which slows the HBM-bound pass beside it down 3x
  const bool wih_last = sj.side != nullptr;
  VsProfScope ps(VS_PROF_BWD_LSTM_GEMM, ls);
  // sum_t of the gate gradients per utterance, then over the batch: bias / d-vector-column gradients, all leaves [r6: here, on the
  // leaves' stream, instead of in front of the dfeat contraction on the caller's]
  if (int rc = vs_colsum_impl(dxg, 8 * H, B, T, 8 * H, dsum, 8 * H, ls)) return rc;
  if (int rc = vs_colsum_impl(dsum, 8 * H, 1, B, 8 * H, tmp, 8 * H, ls)) return rc;
  for (int dir = 0; dir < 2; ++dir) {
    VS_CHECK_HIP(hipMemcpyAsync(g->b_ih[dir], tmp + (size_t)dir * 4 * H, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, ls));
    VS_CHECK_HIP(hipMemcpyAsync(g->b_hh[dir], tmp + (size_t)dir * 4 * H, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, ls));
    const float* dxg_d = dxg + (size_t)dir * 4 * H;
    // dW_ih[:, :8F] = dxg_d^T @ feat
    if (st.nhwc) {
      if (dir == 0 && !wih_last) { if (int rc = dwih_bf16()) return rc; }
    } else {
      VsGemm dwih{.A = dxg_d, .lda = 8 * H, .a_kmajor = 1, .W = feat, .ldw = K8, .w_kmajor = 1, .C = g->w_ih[dir], .ldc = KE,
                  .M = 4 * H, .N = K8, .K = M};
      if (f16x3) { dwih.arith = VS_GEMM_SPLIT_F16; dwih.a_scale2 = gsc + 8; dwih.w_scale2 = gsc; }
      if (int rc = vs_gemm_impl(dwih, ls)) return rc;
    }
    // dW_ih[:, 8F:] = (sum_t dxg_d)^T @ dvec    (the repeated d-vector columns, model.py:77-81)
    if (int rc = vs_gemm_impl({.A = dsum + (size_t)dir * 4 * H, .lda = 8 * H, .a_kmajor = 1, .W = dvec, .ldw = E, .w_kmajor = 1,
                               .C = g->w_ih[dir] + K8, .ldc = KE, .M = 4 * H, .N = E, .K = B}, ls)) return rc;
    // dW_hh = sum_t dgates_t^T h_{t-1}: the lstm_out rows shifted by one frame inside each utterance
    // (VS_MATH_BF16: on bf16-rounded operands like the other contractions of this configuration)
    if (int rc = vs_gemm_impl({.arith = st.nhwc ? VS_GEMM_FP32_BF16 : VS_GEMM_FP32, .A = dxg_d, .lda = 8 * H, .a_kmajor = 1,
                               .W = lstm_out + (size_t)dir * H, .ldw = 2 * H, .w_kmajor = 1, .C = g->w_hh[dir], .ldc = H,
                               .M = 4 * H, .N = H, .K = M, .w_shift = dir ? 1 : -1, .w_group = T, .splits = kSplitK, .partials = st.part},
                              ls)) return rc;
    if (g->dvec) {
      if (int rc = vs_gemm_impl({.A = dsum + (size_t)dir * 4 * H, .lda = 8 * H, .W = p->w_ih[dir] + K8, .ldw = KE, .w_kmajor = 1,
                                 .C = g->dvec, .ldc = E, .accumulate = dir, .M = B, .N = E, .K = 4 * H}, ls)) return rc;
    }
  }
  if (st.nhwc && wih_last) { if (int rc = dwih_bf16()) return rc; }
  return 0;
}

// dfeat = d(gates) @ W_ih[:, :8F] on the caller's stream -- only dfeat continues down the conv stack -- and the LSTM's leaves.
// [r5] The leaf contractions start on the side stream right here, beside the dfeat contraction and the HBM-bound BatchNorm backward of the
// features that follow on the caller's stream, with dW_ih LAST among them (started behind the features' BatchNorm backward or behind
// cnn8's backward they collide with cnn7's data gradient: measured slower in round 5, profiles/r05_experiments.md section 3; those
// orders are not offered any more).
int dfeat_and_leaves(const Step& st, SideJoin& sj, const float* dvec, const vs_grads* g) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  hipStream_t stream = st.stream;
  const int H = st.H, M = st.M, K8 = st.K8, KE = st.KE;
  const bool f16x3 = st.d->math == VS_MATH_F16X3;
  float* dxg = st.at<float>(L.gates);
  float* dfeat = st.at<float>(L.dfeat);
  float* gsc = st.at<float>(L.gemm_scales);
  char* bfb = st.at<char>(L.lstm_bf16);
  {
    VsProfScope ps(VS_PROF_BWD_LSTM_GEMM, stream);
    if (f16x3) {
      // split-f16 mode: the two large contractions (dW_ih feat part, dfeat) reuse the forward's scales
      // of feat / W_ih (gemm_scales[0..3]) and one new scale for the gate gradients
      if (int rc = vs_pow2_scale_impl(dxg, (long long)M * 8 * H, reinterpret_cast<unsigned*>(gsc + 12), gsc + 8, stream)) return rc;
    } else if (st.nhwc) {
      // the gate gradients as bf16 [M][8H]: row-form A of dfeat, col-form A of dW_ih (gemm_bf16.hip)
      // (round 6: the BPTT kernel storing this form itself beside the fp32 one saved the 0.13 ms pass and cost the recurrence 0.2 ms --
      // 32 more scattered lines per store instruction in a loop bound by exactly those: profiles/r06_experiments.md section 9)
      if (int rc = vs_cvt_rows_bf16_impl(dxg, M, 8 * H, 8 * H, bfb + st.lb.dxg, 8 * H, stream)) return rc;
    }
  }
  if (int rc = sj.fork()) return rc;
  {
    VsProfScope ps(VS_PROF_BWD_LSTM_GEMM, stream);
    if (st.nhwc) {
      // dfeat = dxg @ [W_ih; W_ih_reverse][:, :8F]: both directions in one contraction over K = 8H
      if (int rc = vs_gemm_bf16_impl({.A = bfb + st.lb.dxg, .lda = 8 * H, .B = bfb + st.lb.wih, .ldb = st.lb.Kp, .b_kmajor = 1,
                                      .C = dfeat, .ldc = K8, .M = M, .N = K8, .K = 8 * H}, stream)) return rc;
    } else {
      for (int dir = 0; dir < 2; ++dir) {
        const float* dxg_d = dxg + (size_t)dir * 4 * H;
        // dfeat (+)= dxg_d @ W_ih[:, :8F]
        VsGemm df{.A = dxg_d, .lda = 8 * H, .W = p->w_ih[dir], .ldw = KE, .w_kmajor = 1, .C = dfeat, .ldc = K8, .accumulate = dir,
                  .M = M, .N = K8, .K = 4 * H};
        if (f16x3) { df.arith = VS_GEMM_SPLIT_F16; df.a_scale2 = gsc + 8; df.w_scale2 = gsc + 2; }
        if (int rc = vs_gemm_impl(df, stream)) return rc;
      }
    }
  }
  if (int rc = lstm_leaves(st, sj, dvec, g)) return rc;
  // ABI 9: the caller's event for "head + BiLSTM gradients are final" (vs_grads.leaves_event): recorded behind the last leaf launch,
  // on the stream the leaves ran on (the head's leaves were enqueued earlier on the same stream, or on `stream` ahead of the fork)
  if (g->leaves_event) VS_CHECK_HIP(hipEventRecord((hipEvent_t)g->leaves_event, sj.to()));
  if (sj.side) VS_CHECK_HIP(hipEventRecord(sj.side->leaves, sj.side->s));      // (the shared partial-sum scratch `part` is free behind this)
  return 0;
}

// cnn8's BatchNorm + activation backward on the fp32 features: dfeat -> dz8, in place
int features_bn_bwd(const Step& st, const vs_grads* g) {
  // split-f16 convs: dz of layer l is the operand of its data- and weight-gradient launches; the
  // BatchNorm backward pass that produces it folds its |max| into slot 8+l  (this function serves the bf16 route too)
  if (st.d->math != VS_MATH_FP32) VS_CHECK_HIP(hipMemsetAsync(st.cs + 8 * VS_SCALE_SLOT_FLOATS, 0, 8 * VS_SCALE_SLOT_FLOATS * sizeof(float), st.stream));
  VsProfScope ps(VS_PROF_BWD_BN, st.stream);
  const BnConsts k = st.bn(7);
  float* dfeat = st.at<float>(st.L.dfeat);
  return vs_bn_act_bwd_impl(dfeat, st.at<float>(st.L.z8), dfeat, 8, (long long)st.M * 8, st.F, st.conv_act, st.train, k.scale, k.shift, k.mean, k.invstd,
                            g->conv[7].bn_weight, g->conv[7].bn_bias, g->conv[7].bias, st.stats, st.coef, nullptr, st.stream);
}

// BASELINE configs[2]: cnn8 .. cnn1 backward on channels-last bf16 tensors (nhwc_last.hip, nhwc_bn.hip, nhwc_first.hip, conv_nhwc.hip, wgrad_nhwc.hip).
// Every kernel that produces a layer's input gradient (cnn8's backward, the data-gradient convs) applies the activation derivative of
// the layer below on the spot and accumulates the BatchNorm backward sums (the dy forms): the BatchNorm backward proper is then
// finalize + one pass (see kBwdFinalizeClearsDoubles for the memsets).
// [r6] Roles of the two streams: the MATRIX kernels (data gradient, weight gradient) stay on the caller's stream, back to back; the
// HBM-bound pass that consumes the gradient a data gradient just produced -- layer l-1's BatchNorm backward, cnn1's one-pass backward
// behind cnn2's -- forks to the side stream and runs beside layer l's weight gradient.  Rounds 3-5 had it the other way round (weight
// gradients on the side stream): the weight gradient, the longer of each pair, then started a cross-stream wait (~25 us) late and the
// next data gradient waited for it across streams again; now the wait at the end of a pair is for a pass that ends ~0.1 ms before the
// weight gradient does, and cnn1's backward (0.95 ms alone, VALU-bound) runs beside cnn2's weight gradient (0.8 ms) instead of behind it
// (1.55 ms for the pair instead of 1.77).  45.46 -> 45.17 ms per step, three alternating runs (profiles/r06_experiments.md section 10).
int convs_bwd_nhwc(const Step& st, SideJoin& sj, const float* x, const vs_grads* g) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  hipStream_t stream = st.stream;
  const int B = st.B, T = st.T, F = st.F;
  const long long npix = (long long)B * T * F;
  void* gb[2] = {st.at<void>(L.grad0), st.at<void>(L.grad1)};
  int c = 0;
  // layer l's BatchNorm backward from the sums its dy launch left: gbuf -> dz_l, in place
  auto from_dy = [&](int l, void* gbuf, hipStream_t s, int beside) -> int {
    VsProfScope ps(VS_PROF_BWD_BN, s);
    const BnConsts k = st.bn(l);
    return vs_nhwc_bn_bwd_from_dy_impl(gbuf, st.at<void>(L.z[l]), gbuf, npix, st.train, k.scale, k.mean, k.invstd,
                                       g->conv[l].bn_weight, g->conv[l].bn_bias, g->conv[l].bias, st.stats, st.coef, s, kBwdFinalizeClearsDoubles, beside);
  };
  {
    // cnn8: dz8 -> dW8, and dA7 with cnn7's activation derivative and BatchNorm backward sums
    VsProfScope ps(VS_PROF_BWD_EDGE, stream);
    const BnConsts k = st.bn(6);
    VS_CHECK_HIP(hipMemsetAsync(st.stats, 0, sizeof(double) * VS_BN_STAT_SLOTS * 128, stream));
    // partial sums in the idle second gradient buffer: `part` may still be in use by the LSTM leaf GEMMs on the side stream
    // train mode: a7 was never written (see convs_nhwc): recomputed from z7 by the kernel
    if (int rc = vs_nhwc_conv_last_bwd_impl(st.at<float>(L.dfeat), p->conv[7].weight, st.train ? nullptr : st.at<void>(L.a[6]), gb[c], st.at<float>(L.grad1),
                                            g->conv[7].weight, B, T, F, st.at<void>(L.z[6]), st.conv_act, k.scale, k.shift, k.mean, k.invstd,
                                            st.stats, stream)) return rc;
  }
  if (int rc = from_dy(6, gb[c], stream, 0)) return rc;      // cnn7's BatchNorm backward: nothing to run beside yet
  for (int i = 5; i >= 0; --i) {
    const int l = i + 1;                                       // gb[c] = dz of layer l
    {
      VsProfScope ps(VS_PROF_BWD_DGRAD + i, stream);
      const void* pack_t = st.at<void>(L.conv_packed_t[i]);      // (written by vs_forward_train [r6])
      if (l == 1) {
        // cnn2's data gradient is the plain conv: the activation derivative of cnn1 needs z1, which cnn1's one-pass backward recomputes from x
        if (int rc = vs_nhwc_conv_impl(gb[c], pack_t, st.ones, st.zeros, gb[c ^ 1], B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, VS_ACT_NONE,
                                       nullptr, stream)) return rc;
      } else {
        const BnConsts k = st.bn(l - 1);
        VS_CHECK_HIP(hipMemsetAsync(st.stats, 0, sizeof(double) * VS_BN_STAT_SLOTS * 128, stream));
        if (int rc = vs_nhwc_conv_dy_impl(gb[c], pack_t, gb[c ^ 1], st.at<void>(L.z[l - 1]), st.conv_act, k.scale, k.shift, k.mean, k.invstd, st.stats,
                                          B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, stream)) return rc;
      }
    }
    if (int rc = sj.fork()) return rc;
    if (l >= 2) {
      if (int rc = from_dy(l - 1, gb[c ^ 1], sj.to(), sj.side ? 1 : 0)) return rc;
    } else {
      VsProfScope ps(VS_PROF_BWD_EDGE, sj.to());
      const BnConsts k = st.bn(0);
      // (deterministic mode's slot scratch: behind the turn words -- `part` belongs to the weight gradient beside it)
      if (int rc = vs_nhwc_first_bwd_impl(gb[c ^ 1], x, p->conv[0].weight, p->conv[0].bias, B, T, F, st.conv_act, st.train, k.scale, k.shift, k.mean, k.invstd,
                                          g->conv[0].bn_weight, g->conv[0].bn_bias, g->conv[0].bias, g->conv[0].weight,
                                          st.at<double>(L.first_acc) + 64, sj.to(), st.at<double>(L.first_acc),
                                          st.det ? st.at<double>(L.det_turn) + VS_TURN_WORDS * 4 / 8 : nullptr)) return rc;
    }
    if (int rc = sj.mark()) return rc;
    // the LSTM's leaf contractions on the side stream share the partial-sum scratch: long finished by now
    if (i == 5 && sj.side) VS_CHECK_HIP(hipStreamWaitEvent(stream, sj.side->leaves, 0));
    {
      VsProfScope ps(VS_PROF_BWD_WGRAD + i, stream);
      if (int rc = vs_nhwc_wgrad_impl(gb[c], st.at<void>(L.a[l - 1]), st.part, g->conv[l].weight, B, T, F, kMid[i].kt, kMid[i].kf,
                                      kMid[i].dil, stream)) return rc;
    }
    if (int rc = sj.wait()) return rc;      // (the pass beside it: done before the weight gradient is)
    c ^= 1;
  }
  return 0;
}

// cnn8 .. cnn1 backward of the NCHW route (fp32, split-f16); here the WEIGHT gradients are the side stream's
int convs_bwd_nchw(const Step& st, SideJoin& sj, const float* x, const vs_grads* g) {
  const vs_params* p = st.p;
  const vs_tape_layout& L = st.L;
  hipStream_t stream = st.stream;
  const int B = st.B, T = st.T, F = st.F;
  const bool f16x3 = st.d->math == VS_MATH_F16X3;
  float* dfeat = st.at<float>(L.dfeat);
  float* gbuf[2] = {st.at<float>(L.grad0), st.at<float>(L.grad1)};
  int cur = 0;
  auto bn_bwd = [&](int l) -> int {      // gbuf[cur] = dA_l -> dz_l, in place
    VsProfScope ps(VS_PROF_BWD_BN, stream);
    const BnConsts k = st.bn(l);
    unsigned* amax = (f16x3 && l >= 1) ? vs_amax_slot(st.cs + VS_SCALE_SLOT_FLOATS * (8 + l)) : nullptr;
    return vs_bn_act_bwd_impl(gbuf[cur], st.at<float>(L.z[l]), gbuf[cur], 64, (long long)B * 64, T * F, st.conv_act, st.train, k.scale, k.shift, k.mean,
                              k.invstd, g->conv[l].bn_weight, g->conv[l].bn_bias, g->conv[l].bias, st.stats, st.coef, amax, stream);
  };
  {
    // cnn8's weight gradient: a leaf as well, and the partial-sum scratch it shares with the side stream's other
    // users is then only ever touched there, in stream order
    if (int rc = sj.fork()) return rc;
    {
      VsProfScope ps(VS_PROF_BWD_EDGE, sj.to());
      if (int rc = vs_conv_last_wgrad_impl(dfeat, st.at<float>(L.a[6]), st.part, g->conv[7].weight, B, T, F, sj.to())) return rc;
    }
    VsProfScope ps(VS_PROF_BWD_EDGE, stream);
    if (int rc = vs_conv_last_dgrad_impl(dfeat, p->conv[7].weight, gbuf[cur], B, T, F, stream)) return rc;
  }
  for (int i = 5; i >= 0; --i) {
    const int l = i + 1;   // cnn(l+1), conv index l
    if (int rc = bn_bwd(l)) return rc;
    float* sc_bwd = st.cs + VS_SCALE_SLOT_FLOATS * (8 + l);
    // the weight gradient of the layer above, on the side stream, still reads the buffer this data gradient writes
    if (i < 5) { if (int rc = sj.wait()) return rc; }
    {
      VsProfScope ps(VS_PROF_BWD_DGRAD + i, stream);
      if (int rc = vs_conv64_layer_impl(st.d->math, gbuf[cur], p->conv[l].weight, st.at<float>(L.pack_tmp), sc_bwd, 1,
                                        st.ones, st.zeros, gbuf[cur ^ 1], B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, VS_ACT_NONE, 1,
                                        nullptr, stream)) return rc;
    }
    if (int rc = sj.fork()) return rc;
    {
      // after the data gradient: in split-f16 mode it reuses the scale of dz that launch derived
      // (sc_bwd[0..1]) and the scale of the layer input the forward derived (slot l)
      VsProfScope ps(VS_PROF_BWD_WGRAD + i, sj.to());
      if (f16x3) {
        if (int rc = vs_conv64_wgrad_f16x3_impl(gbuf[cur], st.at<float>(L.a[l - 1]), sc_bwd, st.cs + VS_SCALE_SLOT_FLOATS * l,
                                                st.part, g->conv[l].weight, B, T, F, kMid[i].kt, kMid[i].kf, kMid[i].dil, sj.to())) return rc;
      } else {
        if (int rc = vs_conv64_wgrad_impl(gbuf[cur], st.at<float>(L.a[l - 1]), st.part, g->conv[l].weight, B, T, F,
                                          kMid[i].kt, kMid[i].kf, kMid[i].dil, sj.to())) return rc;
      }
    }
    if (int rc = sj.mark()) return rc;
    cur ^= 1;
  }
  // cnn2's weight gradient reads gbuf[cur ^ 1], which cnn1's backward uses as scratch -- and the caller's stream has
  // to see everything the side stream produced: join here
  if (int rc = sj.join()) return rc;
  if (F < 4 || (long long)T * F >= (1 << 24)) {   // packs spanning >2 frames / float frame index: unfused path
    if (int rc = bn_bwd(0)) return rc;
    VsProfScope ps(VS_PROF_BWD_EDGE, stream);
    return vs_conv_first_wgrad_impl(gbuf[cur], x, st.at<double>(L.first_acc), g->conv[0].weight, B, T, F, stream);
  }
  // cnn1: BatchNorm backward and dW1 together; dZ1 is never stored.  The idle gradient buffer holds
  // the zero-padded input rows.
  VsProfScope ps(VS_PROF_BWD_BN, stream);
  const BnConsts k = st.bn(0);
  return vs_bn_act_bwd_first_impl(gbuf[cur], st.at<float>(L.z[0]), x, gbuf[cur ^ 1], B, T, F, st.conv_act, st.train, k.scale, k.shift, k.mean,
                                  k.invstd, g->conv[0].bn_weight, g->conv[0].bn_bias, g->conv[0].bias, g->conv[0].weight, st.stats, st.coef,
                                  st.at<double>(L.first_acc), stream);
}

}  // namespace

extern "C" {

int vs_tape_layout_query(const vs_dims* dims, vs_tape_layout* out) {
  VS_REQUIRE(out != nullptr, "tape layout out pointer is NULL");
  return tape_layout(dims, out);
}

size_t vs_tape_bytes(const vs_dims* dims) {
  vs_tape_layout L;
  if (tape_layout(dims, &L)) return 0;
  return L.total_bytes;
}

// ---------------------------------------------------------------------------------------------
// forward with tape
// ---------------------------------------------------------------------------------------------
int vs_forward_train(const vs_dims* d, const vs_params* p, const float* x, const float* dvec, int conv_act, int bn_mode,
                     void* tape, size_t tape_bytes, float* mask, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  vs_tape_layout L;
  if (int rc = check_tape(d, tape, tape_bytes, &L)) return rc;
  if (int rc = check_params(p)) return rc;
  VS_REQUIRE(x && dvec && mask, "forward_train: NULL argument");
  VS_REQUIRE(conv_act == VS_ACT_MISH || conv_act == VS_ACT_RELU, "forward_train: conv_act must be MISH or RELU");
  VS_REQUIRE(bn_mode == VS_BN_EVAL || bn_mode == VS_BN_TRAIN, "forward_train: unknown bn_mode %d", bn_mode);
  const Step st = make_step(d, p, tape, L, conv_act, bn_mode, stream);
  VsTurnScope turn_scope(st.turn());
  if (int rc = arm(st)) return rc;
  bool feat_bf16_ready = false;
  if (st.nhwc) {
    // the weight images beside cnn1 on the side stream (the prologue), or in front of it on the caller's
    SideLock side_lock;
    SideJoin sj;
    sj.stream = stream;
    if (g_bwd_overlap && vs_opt(VS_OPT_FWD_PROLOGUE)) {
      side_lock.lock();
      if (int rc = side_stream(&sj.side)) return rc;
    }
    if (int rc = sj.fork()) return rc;
    if (int rc = weight_images(st, dvec, sj.to())) return rc;
    if (int rc = sj.mark()) return rc;
    if (int rc = cnn1_nhwc(st, x)) return rc;
    if (int rc = sj.wait()) return rc;      // the weight images are needed from here on
    side_lock.unlock();
    if (int rc = convs_nhwc(st)) return rc;
  } else {
    if (int rc = convs_nchw(st, x)) return rc;
  }
  if (int rc = features_bn(st, &feat_bf16_ready)) return rc;
  if (int rc = lstm(st, dvec, feat_bf16_ready)) return rc;
  return head(st, mask);
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
extern "C" int vs_set_backward_overlap(int on) {
  if (on != 0 && on != 1) return -1;
  g_bwd_overlap = on;
  return 0;
}

int vs_backward(const vs_dims* d, const vs_params* p, const float* x, const float* dvec, int conv_act, int bn_mode,
                void* tape, size_t tape_bytes, const float* mask, const float* dmask, const vs_grads* g, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SideLock side_lock;
  if (g_bwd_overlap) side_lock.lock();
  vs_tape_layout L;
  if (int rc = check_tape(d, tape, tape_bytes, &L)) return rc;
  if (int rc = check_params(p)) return rc;
  VS_REQUIRE(x && dvec && mask && dmask && g, "backward: NULL argument");
  VS_REQUIRE(conv_act == VS_ACT_MISH || conv_act == VS_ACT_RELU, "backward: conv_act must be MISH or RELU");
  VS_REQUIRE(bn_mode == VS_BN_EVAL || bn_mode == VS_BN_TRAIN, "backward: unknown bn_mode %d", bn_mode);
  for (int l = 0; l < 8; ++l)
    VS_REQUIRE(g->conv[l].weight && g->conv[l].bias && g->conv[l].bn_weight && g->conv[l].bn_bias,
               "backward: conv layer %d has a NULL gradient pointer", l + 1);
  for (int dir = 0; dir < 2; ++dir)
    VS_REQUIRE(g->w_ih[dir] && g->w_hh[dir] && g->b_ih[dir] && g->b_hh[dir], "backward: NULL LSTM gradient pointer (dir %d)", dir);
  VS_REQUIRE(g->fc1_w && g->fc1_b && g->fc2_w && g->fc2_b, "backward: NULL head gradient pointer");

  const Step st = make_step(d, p, tape, L, conv_act, bn_mode, stream);
  VsTurnScope turn_scope(st.turn());      // (the words were armed by vs_forward_train and re-armed by every user)
  // the side stream: the leaves of the backward pass (weight gradients of the head, of the LSTM, of the convs) run there
  SideJoin sj;
  sj.stream = stream;
  if (g_bwd_overlap) { if (int rc = side_stream(&sj.side)) return rc; }
  if (int rc = head_bwd(st, sj, mask, dmask, g)) return rc;
  if (int rc = bptt(st)) return rc;
  if (int rc = dfeat_and_leaves(st, sj, dvec, g)) return rc;
  if (int rc = features_bn_bwd(st, g)) return rc;
  return st.nhwc ? convs_bwd_nhwc(st, sj, x, g) : convs_bwd_nchw(st, sj, x, g);
}

// Did the persistent BiLSTM kernels of the last calls on these buffers complete?  (A launch that could not be resident
// falls back to the step kernels before it starts; one whose bounded spin gave up anyway -- CUs taken away by another
// process mid-launch -- sets a word in its state buffer and poisons its output with NaN.)  Synchronises `stream`.
int vs_lstm_status(const vs_dims* d, const void* tape, size_t tape_bytes, const void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VS_REQUIRE(tape || workspace, "lstm_status: pass a tape and / or a workspace");
  unsigned words[3] = {0u, 0u, 0u};
  if (tape) {
    vs_tape_layout L;
    if (int rc = tape_layout(d, &L)) return rc;
    VS_REQUIRE(tape_bytes >= L.total_bytes, "lstm_status: tape too small");
    const char* t = static_cast<const char*>(tape);
    VS_CHECK_HIP(hipMemcpyAsync(&words[0], t + L.lstm_state + (vs_lstm_state_floats(d->B, d->H) - 64) * sizeof(float), 4, hipMemcpyDeviceToHost, stream));
    VS_CHECK_HIP(hipMemcpyAsync(&words[1], t + L.lstm_bwd_state + (vs_lstm_bwd_state_floats(d->B, d->H) - 64) * sizeof(float), 4, hipMemcpyDeviceToHost, stream));
  }
  if (workspace) {
    vs_ws_layout W;
    if (int rc = vs_workspace_layout(d, &W)) return rc;
    VS_REQUIRE(workspace_bytes >= W.total_bytes, "lstm_status: workspace too small");
    VS_CHECK_HIP(hipMemcpyAsync(&words[2], static_cast<const char*>(workspace) + W.lstm_state + (vs_lstm_state_floats(d->B, d->H) - 64) * sizeof(float), 4,
                                hipMemcpyDeviceToHost, stream));
  }
  VS_CHECK_HIP(hipStreamSynchronize(stream));
  return (words[0] == 1u || words[1] == 1u || words[2] == 1u) ? 1 : 0;
}

}  // extern "C"
