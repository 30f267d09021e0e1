/* voicesplit_hip.h -- C ABI of libvoicesplit_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of Edresson/VoiceSplit: the speaker-conditioned
 * mask-prediction forward pass
 *     mask = model(mixed_spec[B,T,F], dvec[B,E])          train.py:94
 *                                                         utils/generic_utils.py:495,545
 * i.e. VoiceSplit.forward  (models/voicesplit/model.py:66-89) and
 *      VoiceFilter.forward (models/voicefilter/model.py:67-90).
 * The reference has no native layer at all (it dispatches to torch.nn / cuDNN), so there is no
 * upstream FFI to mirror; every entry point below names the reference lines it replaces.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer (fp32 unless noted) owned by the
 *    caller: inputs, outputs, the inference workspace and the training tape.  The library never
 *    allocates device memory and keeps no caller pointer after return.
 *  - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no hidden
 *    synchronisation except where an entry point says so (vs_profile_end, vs_lstm_status).
 *  - library-owned state (all of it): (1) ONE side stream + three events per device, created on first use: vs_backward runs the
 *    leaf gradients there and one kernel of every [weight gradient || BatchNorm backward pass] pair, vs_forward_train (VS_MATH_BF16) the weight-only launches of the
 *    step beside cnn1; both join it before they return, and the enqueue phase of concurrent calls on one device is serialised by a
 *    mutex while it is in use (vs_set_backward_overlap(0) turns it off); (2) the process-wide switches: vs_set_conv_kernel /
 *    vs_set_wgrad_kernel / vs_set_lstm_kernel / vs_set_backward_overlap and the option table behind vs_set_option (enum vs_option
 *    lists every one of them; A/B timing and cross-checks: every choice gives the same results unless the option says "ablation";
 *    the library reads NO environment variable), and the opt-in profiler vs_profile_begin / _end; (3) the error word of the
 *    persistent recurrence behind vs_lstm_status and a 64-byte zero page in device memory (static __device__ data of the bf16 GEMM:
 *    source of out-of-range operand pieces).  Calls on different streams with disjoint buffers are otherwise independent.
 *  - return 0 on success, <0 on error (-1 bad argument, -2 HIP runtime error); the message is
 *    available from vs_last_error() (thread-local).  No exceptions cross the ABI.
 *  - tensors are dense row-major with the reference's layouts: spectrogram [B][T][F]
 *    (F contiguous), conv activations [B][C][T][F] (VS_MATH_BF16: channels-last bf16 [B][T][F][C]
 *    inside the workspace / tape), LSTM features [B][T][8F] with feature index c*F+f,
 *    nn.Linear / nn.LSTM weights [out][in].
 */
#ifndef VOICESPLIT_HIP_H
#define VOICESPLIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: these are its only exports */
#endif

#define VS_ABI_VERSION 11

/* activation codes */
#define VS_ACT_RELU 0     /* VoiceFilter conv stack (models/voicefilter/model.py:21..54), head */
#define VS_ACT_MISH 1     /* VoiceSplit conv stack  (utils/generic_utils.py:395-399)           */
#define VS_ACT_NONE 2
#define VS_ACT_SIGMOID 3

/* arithmetic of the 64->64 conv layers (cnn2..cnn7 forward and data gradient) */
#define VS_MATH_FP32 0    /* v_mfma_f32_32x32x2_f32: bitwise an fp32 fmaf chain                              */
#define VS_MATH_F16X3 1   /* fp32 operands split into two f16 halves, three v_mfma_f32_32x32x16_f16 per
                             product term set, fp32 accumulate: fp32-class accuracy at 3/16 of the matrix time */
#define VS_MATH_BF16 2    /* BASELINE configs[2]: the conv stack on channels-last bf16 tensors -- activations and the
                             training tape are STORED as bf16 [B][T][F][64] (half the bytes of every pass), bf16 MFMA
                             operands, fp32 accumulate; BatchNorm statistics, LSTM recurrence, head and master weights
                             stay fp32, the LSTM GEMMs round their operands to bf16.  NOT fp32-class (8-bit mantissa):
                             opt-in only, never a default (tests/test_gpu_bf16.py states its bounds)                  */

/* BatchNorm mode */
#define VS_BN_EVAL 0      /* running statistics (model.eval(), utils/generic_utils.py:479,533) */
#define VS_BN_TRAIN 1     /* batch statistics + running-stat update (model.train(), train.py:84) */

typedef struct vs_dims {
  int B;    /* utterances in the batch                                  */
  int T;    /* frames (301 for 3 s)                                     */
  int F;    /* config.audio[backend].num_freq (601)                     */
  int E;    /* config.model.emb_dim  (256)                              */
  int H;    /* config.model.lstm_dim (400); must be a multiple of 8     */
  int FC1;  /* config.model.fc1_dim  (600)                              */
  int FC2;  /* config.model.fc2_dim  (601)                              */
  int math; /* VS_MATH_FP32, VS_MATH_F16X3 or VS_MATH_BF16 (dense contractions) */
} vs_dims;

/* One Conv2d + BatchNorm2d pair of the nn.Sequential (state_dict conv.{i}.*, conv.{i+1}.*). */
typedef struct vs_conv_layer {
  const float* weight;        /* [Cout][Cin][KT][KF]                       */
  const float* bias;          /* [Cout]                                    */
  const float* bn_weight;     /* [Cout] gamma                              */
  const float* bn_bias;       /* [Cout] beta                               */
  float* bn_running_mean;     /* [Cout] read in eval, updated in train     */
  float* bn_running_var;      /* [Cout]                                    */
} vs_conv_layer;

/* Every parameter of VoiceSplit/VoiceFilter.__init__ (models/voicesplit/model.py:10-64). */
typedef struct vs_params {
  vs_conv_layer conv[8];      /* cnn1..cnn8 = conv.{1,5,9,13,17,21,25,28}          */
  const float* w_ih[2];       /* lstm.weight_ih_l0, _reverse   [4H][8F+E]          */
  const float* w_hh[2];       /* lstm.weight_hh_l0, _reverse   [4H][H]             */
  const float* b_ih[2];       /* lstm.bias_ih_l0, _reverse     [4H]                */
  const float* b_hh[2];       /* lstm.bias_hh_l0, _reverse     [4H]                */
  const float* fc1_w;         /* [FC1][2H] */
  const float* fc1_b;         /* [FC1]     */
  const float* fc2_w;         /* [FC2][FC1]*/
  const float* fc2_b;         /* [FC2]     */
} vs_params;

/* Byte offsets of the intermediates inside the caller-provided workspace (for inspection and
 * stage-level parity tests).  Filled by vs_workspace_layout(). */
typedef struct vs_ws_layout {
  size_t total_bytes;
  size_t act0, act1;          /* ping-pong [B][64][T][F]                           */
  size_t feat;                /* cnn8 output == LSTM features [B][T][8F]           */
  size_t dvbias;              /* dvec @ W_ih[:,8F:]^T + b_ih + b_hh   [B][8H]      */
  size_t xg;                  /* gate pre-activations [B][T][2*4H]                 */
  size_t lstm_out;            /* [B][T][2H]                                        */
  size_t fc1_out;             /* relu(fc1) [B*T][FC1]                              */
  size_t conv_packed[6];      /* fragment-ordered weights of cnn2..cnn7            */
  size_t bn_scale, bn_shift;  /* [8][64] folded BatchNorm                          */
  size_t bn_stats;            /* [8][64][2] double: sum, sum of squares (train)    */
  size_t lstm_packed;         /* fragment-ordered W_hh, both directions            */
  size_t lstm_state;          /* h ping/pong + c, [3][2][H][Bpad]                  */
  size_t conv_scales;         /* [8] scale slots of the split-f16 conv launches: operand scales + running |max| arrays */
  size_t gemm_scales;         /* operand scales of the split-f16 LSTM input GEMM */
} vs_ws_layout;

int vs_abi_version(void);
const char* vs_last_error(void);

/* Opt-in per-stage GPU timing (HIP events on the caller's stream, no synchronisation while
 * enabled).  Forward slots: cnn1..cnn8 conv kernels (0-7), LSTM input GEMMs (8), LSTM recurrence
 * (9), head (10), training-forward BatchNorm passes (11).  Backward slots: head (12), BPTT (13),
 * LSTM weight/input-gradient GEMMs (14), BatchNorm+activation backward (15), weight gradient of
 * cnn2..cnn7 (16-21), data gradient of cnn2..cnn7 (22-27), cnn1/cnn8 kernels (28).  A slot may be
 * entered several times per step; vs_profile_end returns the summed time and the entry count.
 * Instrumentation for bench.py only: process-global, not thread safe. */
#define VS_PROF_CNN1 0
#define VS_PROF_CNN2 1      /* cnn2..cnn7 = 1..6 */
#define VS_PROF_CNN8 7
#define VS_PROF_LSTM_GEMM 8
#define VS_PROF_LSTM_REC 9
#define VS_PROF_HEAD 10
#define VS_PROF_FWD_BN 11
#define VS_PROF_BWD_HEAD 12
#define VS_PROF_BWD_LSTM_REC 13
#define VS_PROF_BWD_LSTM_GEMM 14
#define VS_PROF_BWD_BN 15
#define VS_PROF_BWD_WGRAD 16   /* cnn2..cnn7 = 16..21 */
#define VS_PROF_BWD_DGRAD 22   /* cnn2..cnn7 = 22..27 */
#define VS_PROF_BWD_EDGE 28
#define VS_PROF_SLOTS 29
int vs_profile_begin(int max_calls);
int vs_profile_end(float* ms_total /* [VS_PROF_SLOTS] */, int* calls /* [VS_PROF_SLOTS] */);

/* Workspace the caller must provide to the stage / whole-forward calls. */
int vs_workspace_layout(const vs_dims* dims, vs_ws_layout* out);
size_t vs_workspace_bytes(const vs_dims* dims);

/* ---- whole path: replaces VoiceSplit.forward / VoiceFilter.forward ----------------------
 * x [B][T][F], dvec [B][E] -> mask [B][T][FC2].  conv_act = VS_ACT_MISH (VoiceSplit) or
 * VS_ACT_RELU (VoiceFilter). */
int vs_forward(const vs_dims* dims, const vs_params* params, const float* x, const float* dvec,
               int conv_act, int bn_mode, void* workspace, size_t workspace_bytes,
               float* mask, void* stream);

/* ---- eval-mode forward with the weight-only work done once ------------------------------------
 * validation() / serving call the model again and again with unchanged weights
 * (utils/generic_utils.py:476-558: sample by sample, B = 1).  vs_forward re-derives on every call what
 * depends on the parameters alone (~40 small launches: BatchNorm folded into scale/shift, conv weights
 * packed in MFMA fragment order with their power-of-two scale, W_ih split into f16 halves, W_hh packed);
 * vs_prepare_weights does it once into a caller-owned buffer (vs_prepared_bytes(dims): depends on F, E,
 * H and dims.math, not on B or T; 256-byte aligned) and vs_forward_prepared reads it.  The caller
 * re-prepares whenever a parameter, a BatchNorm running statistic or dims.math changes -- the library
 * cannot see that.  Results are bit-identical to vs_forward(..., VS_BN_EVAL, ...). */
size_t vs_prepared_bytes(const vs_dims* dims);
int vs_prepare_weights(const vs_dims* dims, const vs_params* params, void* prepared, size_t prepared_bytes, void* stream);
int vs_forward_prepared(const vs_dims* dims, const vs_params* params, const void* prepared, size_t prepared_bytes,
                        const float* x, const float* dvec, int conv_act, void* workspace, size_t workspace_bytes,
                        float* mask, void* stream);

/* ---- stages (each is what vs_forward runs, in order) --------------------------------------- */
/* self.conv(x.unsqueeze(1)) + transpose/view: models/voicesplit/model.py:68-74 -> feat [B][T][8F] */
int vs_conv_stack_fwd(const vs_dims* dims, const vs_params* params, const float* x, int conv_act,
                      int bn_mode, void* workspace, size_t workspace_bytes, float* feat, void* stream);
/* repeat/cat d-vector + self.lstm: models/voicesplit/model.py:77-82 -> lstm_out [B][T][2H] */
int vs_bilstm_fwd(const vs_dims* dims, const vs_params* params, const float* feat, const float* dvec,
                  void* workspace, size_t workspace_bytes, float* lstm_out, void* stream);
/* relu/fc1/relu/fc2/sigmoid: models/voicesplit/model.py:83-87; logits may be NULL */
int vs_head_fwd(const vs_dims* dims, const vs_params* params, const float* lstm_out,
                void* workspace, size_t workspace_bytes, float* logits, float* mask, void* stream);

/* ---- eval-mode forward of a padded batch of clips of unequal length, each as if alone ---------------
 * utils/generic_utils.py:476-558 runs validation / test sample by sample (B = 1) because its clips differ in length;
 * models/voicesplit/model.py:66-89 on x[b, :lengths[b]] alone is what every item of these calls computes.
 * x [B][T][F] with T = dims.T = the longest item, lengths [B]: DEVICE array, 1 <= lengths[b] <= T (the caller
 * checks the range: the library cannot without a synchronisation, and clamps to [0, T] on the device so that no
 * value can take a store out of bounds).  mask [B][T][FC2]: rows t < lengths[b] are those of the item alone (same
 * kernels as vs_forward_prepared; the split-f16 operand scales are batch-wide, as in any batch), rows t >= lengths[b]
 * are exactly 0.  The content of x's rows t >= lengths[b] is never read into the arithmetic (a copy of x with zeroed
 * tails is what cnn1 and the |max| pass see): NaN there changes no bit of the result.
 *   conv stack: the ZeroPad2d in time of cnn2..cnn7 (model.py:21-48) has to stand at each item's own end, so the
 *     outputs of cnn1..cnn6 get their rows t >= lengths[b] zeroed (vs_zero_tail_rows) before the next layer reads them;
 *   BiLSTM: nn.LSTM starts from a zero state at the item's first and LAST frame (model.py:82): the persistent
 *     recurrence holds h = c = 0 while t >= lengths[b], in both directions;
 *   head: runs over all B*T rows, then the mask's tail rows are zeroed.
 * Eval mode only (BatchNorm running statistics), dims.math = VS_MATH_F16X3 or VS_MATH_BF16; VS_MATH_FP32 and a
 * recurrence other than the tagged persistent kernel (H > 448, a grid that is not resident, a vs_set_lstm_kernel mode other than 0 or 2)
 * are refused with an error, never computed some other way.  workspace: vs_workspace_bytes(dims), as for B x T. */
int vs_forward_prepared_ragged(const vs_dims* dims, const vs_params* params, const void* prepared, size_t prepared_bytes,
                               const float* x, const float* dvec, const int* lengths, int conv_act,
                               void* workspace, size_t workspace_bytes, float* mask, void* stream);
/* the stages of it: model.py:68-74 -> feat [B][T][8F] (rows t >= lengths[b]: finite, unspecified) and
 * model.py:77-82 -> lstm_out [B][T][2H] (rows t >= lengths[b]: 0); weights derived per call, as in the stage calls above */
int vs_conv_stack_fwd_ragged(const vs_dims* dims, const vs_params* params, const float* x, const int* lengths, int conv_act,
                             void* workspace, size_t workspace_bytes, float* feat, void* stream);
int vs_bilstm_fwd_ragged(const vs_dims* dims, const vs_params* params, const float* feat, const float* dvec, const int* lengths,
                         void* workspace, size_t workspace_bytes, float* lstm_out, void* stream);
/* ptr [B][T] rows of row_bytes bytes each (a multiple of 4; ptr 16-byte aligned): rows t >= lengths[b] of item b := 0 */
int vs_zero_tail_rows(void* ptr, int B, int T, size_t row_bytes, const int* lengths, void* stream);

/* ---- eval-mode forward for K enrolled speakers per mixture with ONE conv pass ---------------------------------
 * models/voicesplit/model.py:70-81 concatenates the d-vector to the conv features only at the LSTM input, so for K
 * d-vectors of one mixture cnn1..cnn8 and the [B*T, 8F] x [8F, 8H] input GEMM are the same work K times over; only the
 * recurrence and the head depend on the speaker.  x [B][T][F], dvecs [B][K][E] (any norm) -> mask [B][K][T][FC2]; row
 * [b][k] is what vs_forward_prepared gives for x[b] with dvecs[b][k] (same kernels for the conv stack, the GEMM and the
 * head; not bit-identical: the row bias is added by the recurrence, not by the GEMM's epilogue).
 *   conv stack: once, for B; with lengths exactly as vs_forward_prepared_ragged runs it;
 *   input GEMM: once, WITHOUT row bias, into G [B][T][8H] (the workspace's gate pre-activation region);
 *   row biases: rb [B*K][8H] = dvecs @ W_ih[:, 8F:]^T + b_ih + b_hh, one small GEMM with M = B*K;
 *   BiLSTM: the tagged persistent recurrence over the N = B*K sequences n = b*K + k in its shared-input mode: the columns
 *     of a 32-column batch tile that belong to mixture b read the SAME row of G, each adds its own 16 values per lane of rb
 *     (held in registers for the whole sequence) in fp32 before the gate functions; same grid, hand-off, bounded spins and
 *     error word as the plain recurrence, launches of cus / (2*H/8) batch tiles;
 *   head: over the B*K*T rows.
 * lengths: NULL, or a DEVICE array [B] as in vs_forward_prepared_ragged -- per MIXTURE: every speaker k of mixture b is
 * computed on x[b, :lengths[b]] alone, mask rows t >= lengths[b] are exactly 0 for every k, and what x holds behind an item's
 * end changes no bit.
 * Eval mode only, no tape.  Refused with an error code and a message, never computed some other way: VS_MATH_FP32, a
 * recurrence other than the tagged persistent kernel (H > 448, vs_set_lstm_kernel not 0 or 2, a grid that is not resident),
 * K < 1, NULL dvecs.
 * workspace: vs_multi_workspace_bytes(dims, K) = vs_workspace_bytes(dims) (conv buffers, features and G for B -- NOT for B*K)
 * + row biases, recurrence state, LSTM output and fc1 scratch for B*K sequences; 256-byte aligned. */
size_t vs_multi_workspace_bytes(const vs_dims* dims, int K);
int vs_forward_prepared_multi(const vs_dims* dims, const vs_params* params, const void* prepared, size_t prepared_bytes,
                              const float* x, const float* dvecs, int K, const int* lengths_or_null, int conv_act,
                              void* workspace, size_t workspace_bytes, float* mask, void* stream);
/* the sequence stage of it: feat [B][T][8F] (vs_conv_stack_fwd / _ragged) -> lstm_out [B][K][T][2H] (rows t >= lengths[b]: 0);
 * weights derived per call, as in the stage calls above; the head is vs_head_fwd over dims with B := B*K */
int vs_bilstm_fwd_multi(const vs_dims* dims, const vs_params* params, const float* feat, const float* dvecs, int K,
                        const int* lengths_or_null, void* workspace, size_t workspace_bytes, float* lstm_out, void* stream);

/* ---- the sequence stage with a carried forward state: a stream separated chunk by chunk ---------------------------
 * The latency-controlled BiLSTM: one call runs model.py:77-82 over the T = dims.T frames [chunk | look-ahead] of a stream.
 *   forward direction: starts from state_in [B][2][H] (fp32; h, then c; NULL = zero state: the stream's first chunk) and
 *     hands h and c behind frame keep - 1 (the chunk's last frame, 1 <= keep <= T) to state_out [B][2][H]; rows t >= keep
 *     of its half of lstm_out are valid forward outputs over the look-ahead frames.  Given the previous call's state_out,
 *     rows t < keep continue the whole-stream recurrence: in the recurrence's own operand form the hand-over is exact (two
 *     calls over [0, a) and [a, T) give the forward half of one call over [0, T) bit for bit);
 *   reverse direction: from a zero state at frame T - 1, as in vs_bilstm_fwd.
 * state_in and state_out may be the same buffer (h is read by a launch in front of the recurrence, every value of c by the
 * lane that later writes it).  Input GEMM with row bias, then the tagged persistent
 * recurrence in its carry mode; with state_in = NULL and keep = T, lstm_out is bit-identical to vs_bilstm_fwd's.
 * Eval mode only.  Refused with an error code and a message, never computed some other way: VS_MATH_FP32, H > 448 (the flag
 * kernel), vs_set_lstm_kernel not 0 or 2, a grid that is not resident, keep outside [1, T], NULL state_out.
 * workspace: vs_workspace_bytes(dims). */
int vs_bilstm_fwd_carry(const vs_dims* dims, const vs_params* params, const float* feat, const float* dvec,
                        const float* state_in, float* state_out, int keep,
                        void* workspace, size_t workspace_bytes, float* lstm_out, void* stream);

/* ---- the same for K enrolled speakers of one live mixture: one conv window and one input GEMM per chunk -------------
 * feat [B][T][8F] (the chunk's features, computed once per mixture), dvecs [B][K][E] -> lstm_out [B][K][T][2H].  The two
 * forms above composed: the input GEMM runs once per mixture WITHOUT row bias into G [B][T][8H], the row biases
 * rb [B*K][8H] come from one small GEMM with M = B*K, and the tagged persistent recurrence runs the N = B*K sequences
 * n = b*K + k in its carry x shared-input mode: column n reads row b of G, adds its own resident row bias in fp32 before the
 * gate functions, starts its forward direction from state_in[n] and hands h and c behind frame keep - 1 to state_out[n]
 * (state_in, state_out [B*K][2][H] fp32: h, then c; state_in = NULL: zero state).  Reverse direction, rows t >= keep and the
 * meaning of keep as in vs_bilstm_fwd_carry.  Guarantees:
 *   (a) two calls over [0, a) and [a, T), the second given the first's state_out, give the forward half of one call over
 *       [0, T) bit for bit, per column;
 *   (b) with state_in = NULL and keep = T, lstm_out is bit-identical to vs_bilstm_fwd_multi's (lengths = NULL);
 *   (c) state_in and state_out may be the same buffer, as in vs_bilstm_fwd_carry;
 *   (d) row [b][k] is what vs_bilstm_fwd_carry gives for feat[b], dvecs[b][k], state_in[b*K + k] -- not bit-identical: the
 *       row bias is added by the recurrence, not by the GEMM's epilogue.
 * Eval mode only; weights derived per call, as in every stage call.  Refused with an error code and a message, never computed
 * some other way -- what vs_bilstm_fwd_carry and vs_bilstm_fwd_multi refuse: VS_MATH_FP32, H > 448, vs_set_lstm_kernel not 0
 * or 2, a grid that is not resident, keep outside [1, T], NULL state_out, K < 1, NULL dvecs.  No per-item lengths: a stream has
 * none.  workspace: vs_multi_workspace_bytes(dims, K).  The head is vs_head_fwd over dims with B := B*K. */
int vs_bilstm_fwd_carry_multi(const vs_dims* dims, const vs_params* params, const float* feat, const float* dvecs, int K,
                              const float* state_in, float* state_out, int keep,
                              void* workspace, size_t workspace_bytes, float* lstm_out, void* stream);

/* ---- kernels (unit-test surface) --------------------------------------------------------- */
/* BN(conv+bias) = conv*scale + shift */
int vs_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
               const float* conv_bias, float eps, int C, float* scale, float* shift, void* stream);
/* cnn1: [B][T][F] -> [B][64][T][F], weight [64][1][1][7] */
int vs_conv_first_fwd(const float* x, const float* w, const float* scale, const float* shift,
                      float* out, int B, int T, int F, int act, void* stream);
/* cnn2..cnn7: 64->64, (KT,KF) in {(7,1),(5,5)}, time dilation dil, "same" zero padding */
size_t vs_conv64_packed_floats(int KT, int KF);
int vs_conv64_pack(const float* w, float* packed, int KT, int KF, void* stream);
int vs_conv64_fwd(const float* in, const float* packed, const float* scale, const float* shift,
                  float* out, int B, int T, int F, int KT, int KF, int dil, int act, void* stream);
/* same layer in VS_MATH_F16X3 arithmetic: vs_pow2_scale gives {s, 1/s} for the input tensor,
 * vs_conv64_pack_f16 packs (and scales) the weights; amax_scratch = one uint32 of device scratch.
 * transpose_flip = 1 packs the data-gradient weights. */
size_t vs_conv64_packed_f16_floats(int KT, int KF);
int vs_pow2_scale(const float* x, long long n, void* amax_scratch, float* scale2, void* stream);
int vs_conv64_pack_f16(const float* w, void* packed, int KT, int KF, int transpose_flip, void* amax_scratch,
                       float* w_scale2, void* stream);
int vs_conv64_f16x3_fwd(const float* in, const void* packed, const float* scale, const float* shift,
                        const float* in_scale2, const float* w_scale2, float* out,
                        int B, int T, int F, int KT, int KF, int dil, int act, void* stream);
/* ---- channels-last bf16 form of the same layers: what VS_MATH_BF16 (BASELINE configs[2]) runs -----------------
 * Activations [B][T][F][64] bf16 (a pixel's 64 channels contiguous), fp32 accumulate, bf16 store.
 * vs_nhwc_conv_pack: weights [64][64][KT][KF] fp32 -> register-fragment order (vs_nhwc_conv_packed_bytes bytes);
 * transpose_flip = 1 packs the data-gradient weights.  vs_nhwc_conv: out = act(conv(in) * scale[co] + shift[co])
 * with 'same' zero padding and time dilation `dil`, (KT,KF) in {(7,1),(5,5)}; bn_stats (or NULL) = per-channel
 * {sum, sum of squares} of the outputs accumulated into [64 slots][64 channels][2] doubles the caller zeroed
 * (train-mode BatchNorm statistics; act must be VS_ACT_NONE then).  All buffers 16-byte aligned. */
size_t vs_nhwc_conv_packed_bytes(int KT, int KF);
int vs_nhwc_conv_pack(const float* w, void* packed, int KT, int KF, int transpose_flip, void* stream);
int vs_nhwc_conv(const void* in, const void* packed, const float* scale, const float* shift, void* out,
                 int B, int T, int F, int KT, int KF, int dil, int act, double* bn_stats, void* stream);
/* The same 64 -> 64 convs, FORWARD, in the fp32-class split-f16 arithmetic (VS_MATH_F16X3) on channels-last operands
 * (csrc/conv_nhwc_f16x3.hip; models/voicesplit/model.py:21-48 under model.eval()).  A tensor is two f16 planes [B][T][F][64]
 * (hi, lo) and a power-of-two scale pair scale2 = {s, 1/s} in device memory: x = (hi + lo) / s (vs_f16x3_split / vs_f16x3_merge
 * convert from / to fp32).  vs_nhwc_conv_f16x3_layer runs one layer from fp32 weights w [64][64][KT][KF] and folded BatchNorm
 * constants (y = act(conv(x) * bn_scale + bn_shift)): it splits and packs the weights into `scratch`
 * (vs_nhwc_conv_f16x3_scratch_bytes, 256-byte aligned; packed_ready != 0: a previous call with the same weights left them
 * there), derives the output scale from max |x| (amax_in: n_amax uints holding the bit patterns of non-negative floats, their
 * maximum = max |x|) and writes out_hi / out_lo / out_scale2 and, when amax_out is not NULL, folds max |y| into
 * amax_out[VS_AMAX_SLOTS = 1024] (zero it first; it is the next layer's amax_in with n_amax = 1024). */
size_t vs_nhwc_conv_f16x3_scratch_bytes(int KT, int KF);
int vs_nhwc_conv_f16x3_layer(const void* in_hi, const void* in_lo, const float* in_scale2, const unsigned* amax_in, int n_amax,
                             const float* w, const float* bn_scale, const float* bn_shift, void* scratch, int packed_ready,
                             void* out_hi, void* out_lo, float* out_scale2, unsigned* amax_out,
                             int B, int T, int F, int KT, int KF, int dil, int act, void* stream);
int vs_f16x3_split(const float* x, const float* scale2, void* hi, void* lo, long long n, void* stream);
int vs_f16x3_merge(const void* hi, const void* lo, const float* scale2, float* x, long long n, void* stream);
/* bf16 GEMM of the same configuration (the three LSTM contractions): C[M][N] (+)= op(A) op(B) (+ rowbias[m / group][n]);
 * A, B bf16; *_kmajor = 0: element (i, k) at i*ld + k, 1: at k*ld + i (no transposed copies: transposing LDS reads).
 * vs_cvt_rows_bf16: fp32 [rows][ld] (K valid columns) -> bf16 [rows][Kp], zero padded.  Row-form operands must be
 * padded to a multiple of 64 in k; ld multiples of 8; 16-byte aligned. */
int vs_cvt_rows_bf16(const float* src, long long rows, int K, int ld, void* dst, int Kp, void* stream);
int vs_gemm_bf16(int a_kmajor, int b_kmajor, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                 const float* rowbias, int ldrb, int group, int accumulate, void* stream);
/* The same contraction with its result rows stored into TWO matrices stacked along M: rows m < split_m go to C + m * ldc,
 * rows m >= split_m to C2 + (m - split_m) * ldc.  This is how vs_backward writes dW_ih of both LSTM directions from ONE
 * col x col contraction over K = B*T (dxg^T @ feat, M = 8H: rows < 4H -> lstm.weight_ih_l0.grad, the rest -> _reverse). */
int vs_gemm_bf16_split(int a_kmajor, int b_kmajor, const void* A, int lda, const void* B, int ldb, float* C, float* C2, int ldc, int split_m,
                       int M, int N, int K, int accumulate, void* stream);
/* The same contraction under a relu mask: C[m][n] = (op(A) op(B))[m][n] where gate[m * ldg + n] > 0, else 0.  This is how vs_backward
 * runs the head's two data gradients (models/voicesplit/model.py:83-85 backwards): dfc1 = (dlogits @ W2) * (h1 > 0) and
 * dlstm_out = (dfc1 @ W1) * (lstm_out > 0), A = the bf16 row copy of the incoming gradient, B = the bf16 weight in K-major form. */
int vs_gemm_bf16_gated(int a_kmajor, int b_kmajor, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                       const float* gate, int ldg, void* stream);
/* the memory-bound kernels around them.  cnn1: x [B][T][F] fp32 -> [B][T][F][64] bf16 (bn_stats as above);
 * BatchNorm + activation apply a = act(z * scale[c] + shift[c]) over npix pixels (a may alias z); cnn8 + transpose/view:
 * [B][T][F][64] bf16 -> [B][T][8][F] fp32. */
int vs_nhwc_conv_first(const float* x, const float* w, const float* scale, const float* shift, void* out,
                       int B, int T, int F, int act, double* bn_stats, void* stream);
/* cnn1 by recomputation (what vs_forward_train / vs_backward run in VS_MATH_BF16): cnn1 (models/voicesplit/model.py:17-19) is 7
 * multiply-adds per output and its input is 1/64 of its output, so neither its conv output z1 nor a separate BatchNorm apply
 * pass is needed.  vs_nhwc_first_moments: x [B][T][F] -> the 35 moments of its seven zero-padded shifts x_k = x[..][f + k - 3]
 * (doubles: S[k] = sum x_k, k = 0..6, then R[k][k'] = sum x_k x_k' for k <= k', row by row).  vs_nhwc_first_stats: the
 * per-channel {sum, sum of squares} of z1 = conv(x) + bias over count = B*T*F pixels that follow from them (stats [64][2],
 * one slot: feed vs_bn_finalize with slots = 1).  The forward is then ONE pass, vs_nhwc_conv_first with the BatchNorm folded
 * into its arguments: scale = bn scale, shift = bn shift + bias * bn scale.  vs_nhwc_first_bwd: the whole backward of cnn1 +
 * BatchNorm + activation in ONE pass over da1 [B][T][F][64] bf16 (z1 recomputed from x beside the derivative; the BatchNorm
 * backward is linear in dy and z, so the weight gradient follows from sum dy x_k and the moments): dgamma, dbeta, dbias [64],
 * dw [64][7] (all overwritten); scale / shift / mean / invstd = vs_bn_finalize's outputs (shift WITHOUT the bias fold);
 * scratch = vs_nhwc_first_bwd_scratch_doubles() doubles. */
int vs_nhwc_first_moments(const float* x, int B, int T, int F, double* moments /* [35] */, void* stream);
int vs_nhwc_first_stats(const double* moments, const float* w, const float* bias, double count, double* stats /* [64][2] */, void* stream);
int vs_nhwc_first_bwd_scratch_doubles(void);
int vs_nhwc_first_bwd(const void* da, const float* x, const float* w, const float* bias, int B, int T, int F, int act, int bn_mode,
                      const float* scale, const float* shift, const float* mean, const float* invstd,
                      float* dgamma, float* dbeta, float* dbias, float* dw, double* scratch, void* stream);
/* Train-mode nn.BatchNorm2d between a conv that accumulated statistics and the apply pass (models/voicesplit/model.py:19 under
 * model.train(), train.py:84): stats = [slots][C][2] doubles {sum, sum of squares} over `count` values per channel -- what
 * vs_nhwc_conv / vs_nhwc_conv_first / vs_nhwc_conv_last_pre leave in bn_stats (slots = 64, C = 64 resp. 8, count = B*T*F);
 * the slots are folded into slot 0 (stats is modified).  Out: scale[c] = gamma / sqrt(var + eps), shift[c] = beta - mean * scale
 * (biased variance: the operands of vs_nhwc_bn_apply, a = act(z * scale + shift)), mean_out / invstd_out (may be NULL: what the
 * backward kernels take as bn_mean / bn_invstd), and running_mean / running_var updated in place exactly as nn.BatchNorm2d
 * does: r = (1 - momentum) r + momentum * {mean, unbiased variance}; pass both as NULL for no update.  The reference uses
 * eps = 1e-5, momentum = 0.1 (nn.BatchNorm2d defaults).  num_batches_tracked is the caller's (host-side counter). */
int vs_bn_finalize(double* stats, int slots, double count, int C, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float eps, float momentum,
                   float* scale, float* shift, float* mean_out, float* invstd_out, void* stream);
int vs_nhwc_bn_apply(const void* z, void* a, long long npix, int act, const float* scale, const float* shift, void* stream);
int vs_nhwc_conv_last(const void* in, const float* w, const float* scale, const float* shift, float* out,
                      int B, int T, int F, int act, void* stream);
/* cnn8 straight on the un-normalised output z7 of cnn7 (train mode): a7 = pre_act(z7 * pre_scale + pre_shift) -- the
 * BatchNorm + Mish/ReLU of models/voicesplit/model.py:47-48 -- is formed in registers, rounded to bf16 exactly as
 * vs_nhwc_bn_apply would have stored it, and fed to the matrix pipe: no apply pass over cnn7's output and no a7 tensor.
 * out = conv * scale + shift, unactivated; bn_stats (may be NULL): [64 slots][8][2] doubles, zeroed by the caller,
 * receive the per-channel {sum, sum of squares} of out (cnn8's own train-mode BatchNorm). */
int vs_nhwc_conv_last_pre(const void* z7, const float* pre_scale, const float* pre_shift, int pre_act, const float* w,
                          const float* scale, const float* shift, float* out, double* bn_stats, int B, int T, int F, void* stream);
/* backward.  Weight gradient of cnn2..cnn7: dz, in [B][T][F][64] bf16 -> dw [64][64][KT][KF] fp32; partials =
 * vs_nhwc_conv_wgrad_partial_floats(KT, KF) floats of scratch.  BatchNorm + activation backward over npix pixels
 * (dz may alias da; stats = 64*64*2 doubles, coef = 192 floats of scratch), and the same fused with cnn1's 1x7 weight
 * gradient (dw [64][7], acc = 448 doubles; dz1 is never written).  cnn8 backward in one pass: dz8 [B][T][8][F] fp32,
 * a7 [B][T][F][64] bf16 -> din (bf16, layout of a7) and dw [8][64]; partials = vs_nhwc_conv_last_bwd_blocks() * 512 floats. */
size_t vs_nhwc_conv_wgrad_partial_floats(int KT, int KF);
int vs_nhwc_conv_wgrad(const void* dz, const void* in, float* partials, float* dw, int B, int T, int F, int KT, int KF, int dil,
                       void* stream);
int vs_nhwc_bn_act_bwd(const void* da, const void* z, void* dz, long long npix, int act, int bn_mode,
                       const float* scale, const float* shift, const float* mean, const float* invstd,
                       float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, void* stream);
int vs_nhwc_bn_act_bwd_first(const void* da, const void* z, const float* x, int B, int T, int F, int act, int bn_mode,
                             const float* scale, const float* shift, const float* mean, const float* invstd,
                             float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc, void* stream);
int vs_nhwc_conv_last_bwd_blocks(void);
int vs_nhwc_conv_last_bwd(const float* dz8, const float* w, const void* a7, void* din, float* partials, float* dw,
                          int B, int T, int F, void* stream);
/* The dy forms vs_backward chains: the kernel that produces a layer's input gradient da also applies the activation
 * derivative of the layer below, dy = da * act'(z * bn_scale + bn_shift) (z = that layer's conv + bias output), stores
 * dy instead of da and accumulates the per-channel {sum dy, sum dy * xhat} into bn_stats (64*64*2 doubles the caller
 * zeroed) -- the first of the two passes of vs_nhwc_bn_act_bwd, without reading the tensor again.
 * vs_nhwc_bn_bwd_from_dy / _first_from_dy are the second pass: parameter gradients + dz = cA dy + cB z + cC (dz may
 * alias dy).  act in {VS_ACT_MISH, VS_ACT_RELU}.  vs_nhwc_conv_last_bwd_dy: a7 may be NULL -- the layer input is then
 * recomputed from z7 and the BatchNorm constants (the counterpart of vs_nhwc_conv_last_pre). */
int vs_nhwc_conv_dy(const void* dz, const void* packed, void* dy, const void* z, int act,
                    const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd, double* bn_stats,
                    int B, int T, int F, int KT, int KF, int dil, void* stream);
int vs_nhwc_conv_last_bwd_dy(const float* dz8, const float* w, const void* a7, void* dy, float* partials, float* dw,
                             const void* z7, int act, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                             const float* bn_invstd, double* bn_stats, int B, int T, int F, void* stream);
int vs_nhwc_bn_bwd_from_dy(const void* dy, const void* z, void* dz, long long npix, int bn_mode,
                           const float* scale, const float* mean, const float* invstd,
                           float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, void* stream);
int vs_nhwc_bn_bwd_first_from_dy(const void* dy, const void* z, const float* x, int B, int T, int F, int bn_mode,
                                 const float* scale, const float* mean, const float* invstd,
                                 float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc, void* stream);
/* cnn8: [B][64][T][F] -> [B][T][8][F], weight [8][64][1][1] */
int vs_conv_last_fwd(const float* in, const float* w, const float* scale, const float* shift,
                     float* out, int B, int T, int F, int act, void* stream);
/* C[M][N] = act(opA(A)[M][K] @ W[N][K]^T + bias1[n] + bias2[n] + rowbias[m/group][n]) */
int vs_gemm_nt(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
               const float* bias1, const float* bias2, const float* rowbias, int ldrb, int group,
               int a_relu, int act, void* stream);
/* recurrence over precomputed gate inputs xg [B][T][8H] -> out [B][T][2H] */
size_t vs_lstm_packed_floats(int H);
size_t vs_lstm_state_floats(int B, int H);
int vs_lstm_pack(const float* w_hh_fwd, const float* w_hh_bwd, float* packed, int H, void* stream);
int vs_bilstm_recurrent(const float* xg, const float* packed_whh, float* state, float* out,
                        int B, int T, int H, void* stream);
/* The same with the arithmetic of the recurrent products h_{t-1} @ W_hh^T chosen by the caller -- what vs_forward* and
 * vs_backward pass from dims.math (models/voicesplit/model.py:82, nn.LSTM's recurrent GEMV): VS_MATH_FP32 = fp32 MFMA
 * (what the calls above use), VS_MATH_F16X3 = h and W_hh split into f16 hi + lo, three f16 MFMA products (fp32-class;
 * the BPTT keeps the fp32 MFMA), VS_MATH_BF16 = h / W_hh rounded to f16 in the forward, gate gradients / W_hh^T rounded
 * to bf16 in the BPTT, one product each.  Pack and recurrence must be given the same `math`; the packed buffers hold the
 * fp32 fragment form (used by the one-launch-per-step kernels in every arithmetic) followed by the 16-bit form.
 * gates_save / c_save may be NULL (inference). */
int vs_lstm_pack_math(const float* w_hh_fwd, const float* w_hh_bwd, float* packed, int H, int math, void* stream);
int vs_bilstm_recurrent_math(const float* xg, const float* packed_whh, float* state, float* out, float* gates_save, float* c_save,
                             int B, int T, int H, int math, void* stream);
/* The inference recurrence with a carried forward state (the raw form of vs_bilstm_fwd_carry above): state_in [B][2][H]
 * fp32 (h, then c) or NULL = zero, state_out [B][2][H], 1 <= keep <= T.  math = VS_MATH_F16X3 or VS_MATH_BF16 and H <= 448;
 * everything else is refused as vs_bilstm_fwd_carry refuses it. */
int vs_bilstm_recurrent_carry(const float* xg, const float* packed_whh, float* state, float* out, const float* state_in,
                              float* state_out, int keep, int B, int T, int H, int math, void* stream);
/* The raw form of vs_bilstm_fwd_carry_multi: N = M*K sequences, sequence n = m*K + k reads row m of xg [M][T][8H] (the input GEMM
 * WITHOUT row bias) and adds rowbias[n] of rowbias [N][8H]; state_in [N][2][H] or NULL = zero, state_out [N][2][H], out [N][T][2H],
 * state sized vs_lstm_state_floats(N, H).  Guarantees (a) and (c) there hold here; with K = 1 and a zero row bias it computes what
 * vs_bilstm_recurrent_carry computes.  Refused: what vs_bilstm_recurrent_carry refuses, K < 1, N not a multiple of K. */
int vs_bilstm_recurrent_carry_shared(const float* xg, const float* rowbias, int K, const float* packed_whh, float* state, float* out,
                                     const float* state_in, float* state_out, int keep, int N, int T, int H, int math, void* stream);

/* =============================================================================================
 * Training: forward that keeps what backward needs + the backward pass itself.
 * Replaces what autograd records/replays for `mask = model(x, emb)` ... `loss.backward()`
 * (train.py:94-110) through models/voicesplit/model.py:66-89: every Conv2d / BatchNorm2d / Mish|ReLU
 * / nn.LSTM / nn.Linear / sigmoid node of the reference graph.
 * ============================================================================================= */

/* d(loss)/d(parameter), same shapes as vs_params.  Every non-NULL pointer is OVERWRITTEN (the
 * caller -- torch.autograd -- accumulates into .grad itself). */
typedef struct vs_conv_layer_grad {
  float* weight;              /* [Cout][Cin][KT][KF]                       */
  float* bias;                /* [Cout]  (exactly 0 under batch-stat BN)   */
  float* bn_weight;           /* [Cout]  d/d gamma                         */
  float* bn_bias;             /* [Cout]  d/d beta                          */
} vs_conv_layer_grad;

typedef struct vs_grads {
  vs_conv_layer_grad conv[8];
  float* w_ih[2];             /* [4H][8F+E] */
  float* w_hh[2];             /* [4H][H]    */
  float* b_ih[2];             /* [4H]       */
  float* b_hh[2];             /* [4H]       */
  float* fc1_w; float* fc1_b; float* fc2_w; float* fc2_b;
  float* dvec;                /* [B][E] d/d speaker embedding, may be NULL */
  void* leaves_event;         /* ABI 9.  NULL, or a hipEvent_t of the caller: vs_backward records it when every gradient of the head and
                                 the BiLSTM (fc1 / fc2 / w_ih / w_hh / b_ih / b_hh: 73 of the 75.5 MB at config.json's sizes) is final --
                                 about 5 ms into the backward pass at B = 64, the conv stack's 25 ms still ahead.  A data-parallel caller
                                 lets its collective stream wait for it and starts the all-reduce of that part of its gradient bucket
                                 beside the conv backward (voicesplit_amd/trainer.py).  The event is recorded on the
                                 library's side stream when the backward overlap is on, else on `stream`. */
} vs_grads;

/* Byte offsets inside the caller-provided training tape.  vs_forward_train fills the "saved"
 * part; vs_backward reads it and uses the rest as scratch.  The tape must not be touched between
 * the two calls; one tape per in-flight forward. */
typedef struct vs_tape_layout {
  size_t total_bytes;
  /* saved by the forward */
  size_t z[7];                /* conv+bias outputs of cnn1..cnn7 before BatchNorm [B][64][T][F] (VS_MATH_BF16: z[0] is not
                                 kept -- cnn1 is recomputed from x -- and a[6] only under VS_BN_EVAL) */
  size_t a[7];                /* act(BN(z)) = input of the next layer                           */
  size_t z8;                  /* cnn8 conv+bias [B][T][8][F]                                    */
  size_t feat;                /* act(BN(z8)) = LSTM features [B][T][8F]                         */
  size_t bn_scale, bn_shift, bn_mean, bn_invstd;   /* [8][64] constants the forward used       */
  size_t gates;               /* [B][T][8H]: gate pre-activations -> activated gates i,f,g,o ->
                                 (backward) gradient wrt the gate pre-activations             */
  size_t cstate;              /* [B][T][2H] cell states                                         */
  size_t lstm_out;            /* [B][T][2H]                                                     */
  size_t fc1_out;             /* relu(fc1) [B*T][FC1]                                           */
  /* backward intermediates (kept for stage-level parity tests) */
  size_t dlogits;             /* [B*T][FC2] */
  size_t dfc1;                /* [B*T][FC1] gradient wrt fc1 pre-activation                     */
  size_t dlstm_out;           /* [B*T][2H]                                                      */
  size_t dsum;                /* [B][8H] sum over t of the gate gradients                       */
  size_t dfeat;               /* [B][T][8F] gradient wrt feat, then wrt z8 (in place)           */
  size_t grad0, grad1;        /* ping-pong [B][64][T][F] activation gradients                   */
  /* scratch */
  size_t dvbias, conv_packed[6], pack_tmp, lstm_packed, lstm_packed_t, lstm_state, lstm_bwd_state;
  size_t consts;              /* ones[64], zeros[64] */
  size_t bn_stats, bn_coef, first_acc, colsum_tmp, partials;
  size_t conv_scales;         /* [16] scale slots (8 forward, 8 backward): operand scales + running |max| arrays */
  size_t gemm_scales;         /* operand scales of the split-f16 LSTM GEMMs (feat, W_ih, gate gradients) */
  size_t lstm_bf16;           /* VS_MATH_BF16: feat [B*T][Kp], [W_ih; W_ih_reverse] [8H][Kp], gate gradients [B*T][8H] as bf16 */
  size_t det_turn;            /* ABI 9: the turn words of the deterministic mode (VS_OPT_DETERMINISTIC), then its slot scratch for cnn1's backward */
  size_t conv_packed_t[6];    /* ABI 9, VS_MATH_BF16: the data-gradient weight images of cnn2..cnn7 (transposed, tap-flipped); written by
                                 vs_forward_train beside its own images (and the transposed W_hh image, lstm_packed_t), read by vs_backward */
} vs_tape_layout;

int vs_tape_layout_query(const vs_dims* dims, vs_tape_layout* out);
size_t vs_tape_bytes(const vs_dims* dims);

/* Forward with the tape.  bn_mode VS_BN_TRAIN: batch statistics, running buffers updated
 * (model.train(), train.py:84); VS_BN_EVAL: running statistics (fine-tuning with frozen BN). */
int vs_forward_train(const vs_dims* dims, const vs_params* params, const float* x, const float* dvec,
                     int conv_act, int bn_mode, void* tape, size_t tape_bytes, float* mask, void* stream);

/* Backward: dmask [B][T][FC2] = d(loss)/d(mask) -> every gradient in `grads`.  `mask` is the
 * tensor vs_forward_train returned; conv_act / bn_mode / dims / params must be those of the forward
 * call and the parameters unchanged since (VS_MATH_BF16: the tape already holds this pass's weight
 * images -- conv_packed_t, lstm_packed_t, the bf16 W_ih -- written by vs_forward_train).  The
 * gradient wrt the spectrogram x is not produced (the reference never asks for it: x is data).
 * Constraint on the caller, not checked here: every weight, and under VS_BN_EVAL the BatchNorm
 * running statistics, must hold the values they had in the vs_forward_train call that filled this
 * tape.  Some are read live here and some from the tape's images, so an edit in between (optimizer
 * step, a VS_BN_TRAIN forward moving the running statistics) silently mixes old and new values
 * (voicesplit_amd/model.py puts them under torch's saved-tensor version check).  Several
 * tapes may be in flight; each backward needs only its own. */
int vs_backward(const vs_dims* dims, const vs_params* params, const float* x, const float* dvec,
                int conv_act, int bn_mode, void* tape, size_t tape_bytes,
                const float* mask, const float* dmask, const vs_grads* grads, void* stream);

/* ---- backward kernels (unit-test surface) -------------------------------------------------- */
/* data gradient of cnn2..cnn7 = vs_conv64_fwd with weights packed by this (transpose + tap flip) */
int vs_conv64_pack_dgrad(const float* w, float* packed, int KT, int KF, void* stream);
/* weight gradient of cnn2..cnn7: dz, in [B][64][T][F] -> dw [64][64][KT][KF]; partials scratch */
size_t vs_conv64_wgrad_partial_floats(int KT, int KF);
int vs_conv64_wgrad(const float* dz, const float* in, float* partials, float* dw,
                    int B, int T, int F, int KT, int KF, int dil, void* stream);
/* the same in VS_MATH_F16X3 arithmetic; scratch8 = 8 floats (operand scales are derived inside) */
int vs_conv64_wgrad_f16x3(const float* dz, const float* in, float* partials, float* dw, float* scratch8,
                          int B, int T, int F, int KT, int KF, int dil, void* stream);
/* which split-f16 weight-gradient kernel vs_conv64_wgrad_f16x3 / vs_backward launch: 0 = by problem
 * size (default: a ring kernel once every workgroup gets >= 2 columns -- the four-wave form for 5x5 --
 * else the kt-split kernel), 1 = eight-wave ring, 2 = kt-split, 3 = four-wave ring (5x5; 7x1 falls back
 * to the eight-wave ring).  Process-wide; returns -1 for any other mode and keeps the current one.  (The timing
 * ablations of the four-wave kernel are instances of `make ABLATION=1` libraries, selected by mode 3 + VS_OPT_ABLATION.) */
int vs_set_wgrad_kernel(int mode);
/* which 5x5 split-f16 forward / data-gradient kernel vs_conv64_f16x3_fwd and the whole-path calls
 * launch: 0 = default (the persistent pipelined kernel, csrc/conv_f16x3_pk.hip), 1 = one tile per
 * workgroup (csrc/conv_f16x3.hip), 2 = persistent.  Both give bit-identical results (same K order);
 * the switch exists for A/B timing and the bitwise cross-check.  Process-wide; returns -1 for any other mode and keeps
 * the current one.  (The timing ablations of the persistent kernel are instances of `make ABLATION=1` libraries, selected by
 * mode 2 + VS_OPT_ABLATION.) */
int vs_set_conv_kernel(int mode);
/* which BiLSTM recurrence / BPTT runs: 0 = default (the persistent kernels whenever all their workgroups
 * fit on the device at once, else one launch per time step), 1 = one launch per step (always the fp32 MFMA products),
 * 2 = persistent (error when the grid cannot be resident), 3 = persistent with the fp32 MFMA products whatever dims.math
 * says (A/B of the f16 / bf16 products), 4 = persistent with the flag hand-off of rounds 2-4 where the default is the tagged-data
 * hand-off (the f16 / split-f16 forward recurrence: same arithmetic).  In VS_MATH_FP32 both forms give bit-identical results.
 * Process-wide.
 * The persistent kernels keep an error word in the caller's state buffer (the first of its last 64
 * floats, both for the forward and the backward state) that becomes 1 when a bounded spin gave up
 * (a workgroup of the launch was not resident): results are then invalid. */
int vs_set_lstm_kernel(int mode);

/* Every remaining process-wide switch of the library, behind ONE call (ABI 8; the list shrank in ABI 9): the library itself reads NO
 * environment variable.  They exist for cross-checks (every on / off pair is compared by a GPU test); every value of every option gives
 * valid results unless the option says "timing ablation".  vs_set_option returns 0, or -1 for an unknown option / a value outside its range; vs_get_option returns
 * the current value (-1 for an unknown option).  Not thread-safe against concurrent calls into the library: set options before
 * work is enqueued.  (The Python package maps the environment variable named beside each option onto this call when it loads
 * the library: voicesplit_amd/_lib.py.) */
enum vs_option {
  VS_OPT_FWD_PROLOGUE = 0,    /* VS_MATH_BF16 vs_forward_train: 1 = the weight-only launches of the step (six conv weight packs, the bf16 copy of
                                 W_ih, the d-vector fold, the recurrent / head weight images) on the library's side stream beside cnn1; 0 = in
                                 line.  Default 1 (-0.15 ms per step).  Same values.  VOICESPLIT_FWD_PROLOGUE */
  VS_OPT_HEAD_LEAF_SIDE = 1,  /* 1: the head's two weight gradients and bias sums (leaves of vs_backward) on the side stream beside the BPTT;
                                 0: in front of it.  Default 1 (-0.3 ms per step).  Same values.  VOICESPLIT_HEAD_LEAF_SIDE */
  VS_OPT_FEAT_ROWS = 2,       /* whole-path eval forward (vs_forward, vs_forward_prepared): 1 = cnn8 writes the LSTM input GEMM's A operand
                                 itself (split-f16 hi / lo rows at a scale planned from the tracked |max| of its input, or bf16 rows): no fp32
                                 features in the workspace, no |max| / split passes over them; 0 = fp32 features, then the passes.  Default 1.
                                 Same values unless a lo half underflows (both scales are powers of two).  VOICESPLIT_FEAT_ROWS */
  VS_OPT_HEAD_BWD_GEMM = 3,   /* VS_MATH_BF16 vs_backward: 1 = the head's two data-gradient contractions (dfc1, dlstm_out) on the LSTM
                                 contractions' LDS-DMA kernel over bf16 copies of their operands (relu mask in the epilogue); 0 = the generic
                                 kernel (in-flight conversion).  Default 1.  Same operand roundings, fp32 summation order differs.
                                 VOICESPLIT_HEAD_BWD_GEMM */
  VS_OPT_ABLATION = 4,        /* libraries built with `make ABLATION=1` only (tools/wgrad_ablation.py, tools/split_conv_micro.py, tools/gemm_micro.py,
                                 tools/conv_bench): selects a TIMING-ABLATION instance of the weight-gradient / split-f16 conv / bf16 GEMM
                                 kernels (results are meaningless); the NCHW split-f16 kernels look at it only while pinned: the weight
                                 gradient under vs_set_wgrad_kernel(3) (its four-wave kernel), the 5x5 forward / data gradient under
                                 vs_set_conv_kernel(2) (its persistent kernel).  Ignored by the product build, except that these pinned kernels
                                 refuse to launch with a value other than 0 (the instances are not in the library).  VOICESPLIT_ABLATION */
  VS_OPT_DETERMINISTIC = 5,   /* VS_MATH_BF16 training step (vs_forward_train, vs_backward, vs_sisnr_loss): 1 = every partial sum that workgroups
                                 add to shared slots with fp64 atomics (BatchNorm statistics, their backward sums, cnn1's input moments,
                                 the loss head's moments) is added in WORKGROUP ORDER (the workgroups of such a launch that add to the same
                                 addresses take turns), so a rerun on the same inputs is bit-identical: masks, running statistics, loss, every gradient.
                                 0 (default) = arrival order: results agree to the last bits of fp64 sums only (SURVEY.md section 5:
                                 deterministic-rerun comparisons as the device-side sanitizer).  Costs 1.8 ms of a 46.0 ms step at B = 64
                                 (profiles/r06_experiments.md).  VOICESPLIT_DETERMINISTIC */
  VS_OPT_COUNT = 6
};
/* Round 6 (ABI 9) removed the switches whose alternative had been measured slower, with the code behind them: the NCHW eval route of the
 * fp32-class convs, the two-pass BatchNorm backward (VS_OPT_BWD_DY), the round-3 bf16 GEMM as an A/B arm and its DMA-row / band knobs,
 * the packed-fp32 epilogue builds, s_setprio / side-stream priorities, the eight-wave conv (VS_OPT_CONV8), the fused BatchNorm finalize
 * of the backward, the grid of the BatchNorm pass beside the weight gradient, the late starts of the LSTM's leaves.  The measurements
 * are in profiles/r04_*.md, profiles/r05_experiments.md and profiles/r06_experiments.md; kernels that were correct and slower are kept
 * as records under tools/attic/. */
int vs_set_option(int option, int value);
int vs_get_option(int option);

/* Did the persistent BiLSTM kernels of the last vs_forward_train / vs_backward on `tape` and / or the last vs_forward /
 * vs_bilstm_fwd on `workspace` complete?  0 = yes, 1 = a bounded spin gave up (another process took CUs away while the
 * launch ran; its output was overwritten with NaN so that no caller can use it by accident), < 0 = error.  Either
 * buffer may be NULL.  Synchronises `stream`.  The launches themselves are cooperative: a grid that cannot be resident
 * is refused by the runtime and the one-launch-per-step kernels run instead. */
int vs_lstm_status(const vs_dims* dims, const void* tape, size_t tape_bytes, const void* workspace, size_t workspace_bytes, void* stream);

/* vs_backward schedule: 1 (default) = the 64->64 weight gradients run on a second HIP stream of the library beside
 * the BatchNorm backward passes of the next layer (matrix-pipe kernel beside an HBM stream); 0 = everything in
 * order on the caller's stream.  Same kernels and summation order: results are bit-identical.  The caller's stream
 * is joined before vs_backward returns.  The side stream and its events are shared by all callers of a device, so
 * while this is on the ENQUEUE phase of concurrent vs_backward calls is serialized by a mutex (the GPU work is not).
 * Returns 0, or -1 for any other value. */
int vs_set_backward_overlap(int on);
/* BatchNorm+activation backward over rows [R][L] with channel = r % C (NCHW: R = B*C, L = T*F;
 * cnn8 feature layout: R = B*T*8, L = F).  dz may alias da.  stats: 2*C doubles, coef: 3*C floats. */
int vs_bn_act_bwd(const float* da, const float* z, float* dz, int C, long long R, int L, int act, int bn_mode,
                  const float* scale, const float* shift, const float* mean, const float* invstd,
                  float* dgamma, float* dbeta, float* dbias, double* stats, float* coef, void* stream);
/* cnn1: the same for da, z [B][64][T][F] fused with the 1x7 weight gradient dw [64][7] against the input
 * x [B][T][F] (dZ1 is consumed in registers, never written).  xpad: B*T*(F+6) floats of scratch;
 * stats: 128 doubles, coef: 192 floats, acc: 448 doubles. */
int vs_bn_act_bwd_first(const float* da, const float* z, const float* x, float* xpad, int B, int T, int F, int act, int bn_mode,
                        const float* scale, const float* shift, const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* dbias, float* dw, double* stats, float* coef, double* acc, void* stream);
/* cnn8 */
int vs_conv_last_dgrad(const float* dz, const float* w, float* din, int B, int T, int F, void* stream);
int vs_conv_last_wgrad_blocks(void);
int vs_conv_last_wgrad(const float* dz, const float* in, float* partials /* [blocks][512] */, float* dw,
                       int B, int T, int F, void* stream);
/* cnn1: dw [64][7]; acc = 448 doubles of scratch */
int vs_conv_first_wgrad(const float* dz, const float* x, double* acc, float* dw, int B, int T, int F, void* stream);
/* general GEMM: layouts 0 = K contiguous (A[m][k], W[n][k]), 1 = K-major (A[k][m], W[k][n]);
 * gate: C = gate[m][n] > 0 ? C : 0; w_shift/w_group: K-major W row k read from row k+w_shift,
 * zero when (k % w_group)+w_shift leaves [0,w_group); splits > 1: split-K via partials [splits][M][N] */
int vs_gemm(int layout_a, int layout_w, const float* A, int lda, const float* W, int ldw, float* C, int ldc,
            int M, int N, int K, const float* bias, const float* gate, int ldg, int a_relu, int w_relu, int act,
            int accumulate, int w_shift, int w_group, int splits, float* partials, void* stream);
/* the same GEMM in VS_MATH_F16X3 arithmetic (no split-K / w_shift); scratch8 = 8 floats; A and W must
 * be dense [rows][ld] buffers, 16-byte aligned (their power-of-two scales are derived inside) */
int vs_gemm_f16x3(int layout_a, int layout_w, const float* A, int lda, const float* W, int ldw, float* C, int ldc,
                  int M, int N, int K, const float* bias, const float* gate, int ldg, int a_relu, int w_relu, int act,
                  int accumulate, float* scratch8, void* stream);
/* BiLSTM recurrence that also saves the activated gates (may alias xg) and cell states */
int vs_bilstm_recurrent_train(const float* xg, const float* packed_whh, float* state, float* out,
                              float* gates_save, float* c_save, int B, int T, int H, void* stream);
/* BPTT: gates (activated, from the call above) are overwritten with d/d(gate pre-activations) */
size_t vs_lstm_packed_t_floats(int H);
size_t vs_lstm_bwd_state_floats(int B, int H);
int vs_lstm_pack_t(const float* w_hh_fwd, const float* w_hh_bwd, float* packed_t, int H, void* stream);
int vs_bilstm_recurrent_bwd(const float* packed_t, float* state, float* gates, const float* c_all,
                            const float* dout, int B, int T, int H, void* stream);
int vs_lstm_pack_t_math(const float* w_hh_fwd, const float* w_hh_bwd, float* packed_t, int H, int math, void* stream);
int vs_bilstm_recurrent_bwd_math(const float* packed_t, float* state, float* gates, const float* c_all,
                                 const float* dout, int B, int T, int H, int math, void* stream);
int vs_sigmoid_bwd(const float* dmask, const float* mask, float* dlogits, long long n, void* stream);
/* out[g][n] = sum over the g-th block of `rows` rows of X [groups*rows][ld] */
int vs_colsum(const float* x, int ld, int groups, int rows, int N, float* out, int ldo, void* stream);

/* =============================================================================================
 * The caller side of the mask during training: train.py:95-108
 *   output = mixed*mask -> ap.torch_inv_spectrogram(output, phase)   utils/audio_processor.py:498-509
 *   loss   = SiSNR_With_Pit()(wav, target_wav, seq_len)              utils/generic_utils.py:417-474
 * in one call, together with d(loss)/d(mask).  The iSTFT runs as a GEMM against the windowed inverse
 * real-DFT basis + a gather-form overlap-add; the reference's quirks are reproduced (complex
 * spectrum = mag*exp(cos phi) + i*mag*exp(sin phi); hann(win, periodic=False) window; centre
 * trimming; means divided by seq_len; eps 1e-16; loss = 20 - mean SI-SNR).
 * ============================================================================================= */
typedef struct vs_loss_dims {
  int B, T, F;               /* spectrogram [B][T][F], F = n_fft/2 + 1                         */
  int n_fft, hop, win;       /* config.audio.voicefilter: 1200, 160, 400                        */
  float min_level_db;        /* -100  (denormalisation, utils/audio_processor.py:501-502)       */
  float ref_level_db;        /*   20                                                            */
} vs_loss_dims;

size_t vs_sisnr_workspace_bytes(const vs_loss_dims* dims);
/* mixed, mask, target, phase: [B][T][F] fp32 (target = normalised target spectrogram, phase = the
 * mixture's phase, used for both waveforms as train.py:99-100 does); seq_len: [B] int32 sample
 * counts or NULL (= hop*(T-1)); loss: one device float; dmask [B][T][F] = d(loss)/d(mask) or NULL;
 * est_wav [B][hop*(T-1)] = the estimated waveform or NULL. */
int vs_sisnr_loss(const vs_loss_dims* dims, const float* mixed, const float* mask, const float* target,
                  const float* phase, const int* seq_len, void* workspace, size_t workspace_bytes,
                  float* loss, float* dmask, float* est_wav, void* stream);

/* The other criterion of train.py:74-75: PowerLaw_Compressed_Loss (utils/generic_utils.py:353-373,
 * loss_name 'power_law_compression', the voicefilter configuration; config.json: power 0.3,
 * complex_loss_ratio 0.113).  prediction = mixed*mask (train.py:95); mixed, mask, target: n = B*T*F
 * floats; scratch: 2 doubles on the device; loss: one device float; dmask = d(loss)/d(mask) or NULL. */
int vs_powerlaw_loss(const float* mixed, const float* mask, const float* target, long long n, float power,
                     float complex_loss_ratio, double* scratch, float* loss, float* dmask, void* stream);

/* ---- audio front / back end of inference: what test.py does around the model ----
 * wav [B][hop*(T-1)] -> spec [B][T][F] (normalised dB magnitude in [0,1]) and phase [B][T][F] (may be
 * NULL): librosa.stft(n_fft, hop, win, hann, center, reflect) + amp_to_db + normalize, transposed to
 * [time, freq]  (utils/audio_processor.py:469-476, 511-514, 537-544). */
size_t vs_audio_workspace_bytes(const vs_loss_dims* dims);
int vs_wav_to_spec(const vs_loss_dims* dims, const float* wav, float* spec, float* phase,
                   void* workspace, size_t workspace_bytes, void* stream);
/* (spec * mask), phase -> wav [B][hop*(T-1)]: denormalize + db_to_amp + mag*exp(i*phase) + librosa.istft
 * (utils/audio_processor.py:478-491; est_mask*mixed_spec from utils/generic_utils.py:496).  mask may be NULL. */
int vs_spec_to_wav(const vs_loss_dims* dims, const float* spec, const float* mask, const float* phase, float* wav,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The other branch of ap.inv_spectrogram (no phase given): Griffin-Lim, utils/audio_processor.py:492-496 and 516-523, with the
 * conventions of the two calls above (periodic Hann, reflect padding, centre trimming).
 *   S = (db_to_amp(denormalize(spec * mask) + ref_level_db)) ** power            (mask may be NULL)
 *   y = istft(S * exp(i * init_phase));  n_iter times:  D = stft(y),  y = istft(S * D / |D|)
 * A bin with |D| == 0 takes phase 0 (np.angle(0) == 0).  n_iter == 0 is the plain inverse.  init_phase [B][T][F] is required: random
 * starting angles are the caller's to draw.  wav [B][hop*(T-1)].  residual (may be NULL): [n_iter][B] doubles on the device,
 * residual[i][b] = || |D_i| - S ||_2 / || S ||_2 over item b, D_i = the STFT taken in iteration i (of the waveform entering it):
 * Griffin-Lim's own objective, non-increasing in exact arithmetic.  The waveform path uses no floating-point atomics (wav is
 * bit-identical across reruns); residual is summed with fp64 atomics (last bits may differ).  No host synchronisation, allocation or
 * copy inside the call; five launches per iteration (six with vs_set_griffin_lim_reframe(1)). */
size_t vs_griffin_lim_workspace_bytes(const vs_loss_dims* dims);
int vs_griffin_lim(const vs_loss_dims* dims, const float* spec, const float* mask, const float* init_phase, float power, int n_iter,
                   float* wav, double* residual, void* workspace, size_t workspace_bytes, void* stream);
/* How an iteration of vs_griffin_lim turns the frames of one inverse into the windowed frames of the next transform: 1 = the
 * overlap-add and framing kernels of the two calls above (through the waveform), 2 = one gather launch (every frame sample sums its
 * <= ceil(win/hop) source frames itself), 0 = the default (the gather form: one launch fewer; not yet measured against the other, tools/griffin_lim_time.py).  Same
 * sums in the same order: bit-identical results.  Process-wide, like vs_set_option.  Returns 0, or -1 for any other value. */
int vs_set_griffin_lim_reframe(int mode);

/* ---- ABI 11 (additive entries).  The wavernn and waveglow audio back ends (utils/audio_processor.py:61-438, utils/audio.py:49-135, utils/stft.py:36-99) ----
 * Both run the transform above (periodic Hann of `win` samples centred in the frame, reflect padding by n_fft/2, 1 + n/hop frames,
 * |D| = sqrt(re^2 + im^2); the Tacotron conv1d-basis transform is the same sum).  What differs is the codec: how a linear magnitude m
 * is stored and read back, a pre-emphasis in front of the transform and the padding of Griffin-Lim's inner transform.
 *   VS_CODEC_DB01    clip((20 log10(max(floor, m)) - ref) / -min_db, -1, 0) + 1                  (voicefilter: vs_wav_to_spec's own)
 *   VS_CODEC_DBNORM  S = 20 log10(max(floor, m)) - ref  (_amp_to_db :184-186), then _normalize :140-155 under the three flags;
 *                    decode = _denormalize :157-173 (clip first), 10^((S + ref) / 20)
 *   VS_CODEC_LOG     ln(max(floor, m)), decode exp(v)                                            (dynamic_range_compression, floor 1e-5)
 * floor is the caller's: exp(min_level_db / 20 * ln 10) evaluated in fp64 on the host for DBNORM (9.99999999999998e-06 for -100). */
#define VS_CODEC_DB01 0
#define VS_CODEC_DBNORM 1
#define VS_CODEC_LOG 2
#define VS_PAD_REFLECT 0
#define VS_PAD_ZERO 1
typedef struct vs_audio_codec {
  int kind;                                       /* VS_CODEC_*                                                               */
  int signal_norm, symmetric_norm, clip_norm;     /* DBNORM only                                                              */
  int gl_pad;                                     /* padding of Griffin-Lim's inner transform: VS_PAD_REFLECT (wavernn), _ZERO  */
  int reserved;
  double floor;                                   /* smallest magnitude the encoder sees                                      */
  double min_level_db, ref_level_db, max_norm;    /* DB01, DBNORM                                                             */
  double preemphasis;                             /* 0: none; else p[n] = x[n] - a x[n-1] in front of the transform (x[-1] = 0) */
} vs_audio_codec;

/* Front end with a codec: wav [B][hop*(T-1)] -> out, phase [B][T][F] (may be NULL).  The pre-emphasis is folded into the framing
 * gather (the difference formed in fp64 and rounded once; the reflect padding acts on p), the contraction is vs_wav_to_spec's.
 * mel_basis == NULL: out [B][T][F] = encode(|D|).  Otherwise mel_basis [n_mels][F] fp32 and out [B][T][n_mels] =
 * encode(mel_basis @ |D|) (melspectrogram / mel_spectrogram), the product as vs_project_floor forms it.  Workspace:
 * vs_audio_workspace_bytes. */
int vs_codec_wav_to_spec(const vs_loss_dims* dims, const vs_audio_codec* codec, const float* wav, const float* mel_basis, int n_mels,
                         float* out, float* phase, void* workspace, size_t workspace_bytes, void* stream);
/* n stored values (times mask, may be NULL) -> linear fp32 magnitudes, evaluated in fp64 and rounded once; and back. */
int vs_codec_decode(const vs_audio_codec* codec, const float* spec, const float* mask, long long n, float* mag, void* stream);
int vs_codec_encode(const vs_audio_codec* codec, const float* mag, long long n, float* spec, void* stream);
/* out [M][N] = max(floor, in [M][K] @ w [N][K]^T): the mel basis, its pseudo-inverse (floor 1e-10) and mag_to_mel.  fp32 FMAs in
 * the order k = 0 .. K-1 for every output: within (K + 2) 2^-24 (|w| @ |in|) of the exact product, the same bits for a row
 * wherever it stands.  in and out must not overlap. */
int vs_project_floor(const float* in, const float* w, float* out, long long M, int N, int K, float floor, void* stream);
/* Inverse legs on a LINEAR magnitude [B][T][F]: the iSTFT with a given phase (vs_spec_to_wav behind its decoder), and Griffin-Lim
 * with the target mag ** power (vs_griffin_lim behind its decoder; pad: the padding of the inner transform, VS_PAD_*; both
 * re-framing forms of vs_set_griffin_lim_reframe serve both).  Workspaces: vs_audio_workspace_bytes / vs_griffin_lim_workspace_bytes. */
int vs_mag_to_wav(const vs_loss_dims* dims, const float* mag, const float* phase, float* wav,
                  void* workspace, size_t workspace_bytes, void* stream);
int vs_griffin_lim_mag(const vs_loss_dims* dims, const float* mag, const float* init_phase, float power, int n_iter, int pad,
                       float* wav, double* residual, void* workspace, size_t workspace_bytes, void* stream);
/* Pre-emphasis y[n] = x[n] - a x[n-1] and its inverse y[n] = x[n] + a y[n-1] (scipy.signal.lfilter([1], [1, -a], x)), rows [B][N]
 * fp32 in and out, y[-1] = x[-1] = 0, the arithmetic in fp64 and rounded once.  The inverse is a parallel scan: the row is cut into
 * blocks of vs_deemphasis_block() samples, every block is swept from a zero state, the carries scan per row
 * (carry(k+1) = a^L carry(k) + last(k)) and a second sweep adds a^(j+1) carry.  The partition and every power of a depend on N and
 * the sample index alone: a row's bits do not depend on B, on its place in the batch or on where the buffers start.  x and y
 * must not overlap.  workspace: vs_deemphasis_workspace_bytes(B, N) bytes, 256-byte aligned. */
int vs_deemphasis_block(void);
size_t vs_deemphasis_workspace_bytes(int B, long long N);
int vs_deemphasis(const float* x, float* y, int B, long long N, double coef, void* workspace, size_t workspace_bytes, void* stream);
int vs_preemphasis(const float* x, float* y, int B, long long N, double coef, void* stream);

/* =============================================================================================
 * Evaluation metric: single-source BSS-eval SDR, the number the reference reports for every test item
 * (utils/generic_utils.py:476-530: mir_eval.separation.bss_eval_sources(clean_wav, est_wav, False)[0][0];
 * test.py "Mean Test SDR", test_all_checkpoints.py's best-checkpoint choice).  Per row, with the fixed
 * 512-tap distortion filter: C = G^-1 D (G: Toeplitz autocorrelation of the reference, lags 0..511;
 * D: reference x estimate cross-correlation), P = ref * C (N + 511 samples),
 * SDR = 10 log10(sum P^2 / sum ([est, 0] - P)^2), +inf when the denominator is 0.  fp64 throughout, sums in
 * an order fixed by N alone: bitwise reproducible, and a row's value does not depend on B.
 * ============================================================================================= */
/* bytes of workspace vs_sdr needs for B rows of N samples; 0 for B <= 0, N <= 0 or sizes beyond the limits of vs_sdr */
size_t vs_sdr_workspace_bytes(int B, long long N);
/* ref, est: [B][N] fp32 (1 <= B <= 2^20, 1 <= N <= 2^40); sdr: [B] doubles (dB); status: [B] ints, 0 = ok,
 * 1 = the reference or the estimate row is all zero (mir_eval raises ValueError), 2 = the Toeplitz solve failed
 * (a prediction error <= 0 or not finite); a row with status != 0 gets NaN.  ws: vs_sdr_workspace_bytes(B, N)
 * bytes, 256-byte aligned.  Five launches on `stream`, no synchronisation. */
int vs_sdr(const float* ref, const float* est, int B, long long N, double* sdr, int* status,
           void* workspace, size_t workspace_bytes, void* stream);

/* Multi-source BSS-eval, mir_eval.separation.bss_eval_sources(reference, estimate, compute_permutation): per item K
 * references s_j and K estimates e_q of N samples, the 512-tap filter as above, M = N + 511:
 *   P_all,q = projection of e_q on all K references delayed 0..511 (block-Toeplitz Gram matrix of K x K blocks, solved by
 *             the block Levinson recursion; never formed);  P_jq = vs_sdr's projection of e_q on s_j alone
 *   SDR[q][j] = |P_jq|^2 / |[e_q,0] - P_jq|^2,  SIR[q][j] = |P_jq|^2 / |P_all,q - P_jq|^2,
 *   SAR[q][j] = |P_all,q|^2 / |[e_q,0] - P_all,q|^2,  each 10 log10, +inf when the denominator is exactly 0.
 * compute_permutation != 0: all K x K pairs; popt maximises sum_j SIR[popt[j]][j] over the permutations in lexicographic
 * order (itertools.permutations), the first maximum wins, the sum taken for j = 0..K-1 in fp64; sdr[j] = SDR[popt[j]][j],
 * likewise sir and sar, perm = popt.  compute_permutation == 0: only the pairs (j, j), perm = 0..K-1.
 * status per item: 0 = ok; 1 = a reference or estimate row of the item is all zero; 2 = a solve failed (a singular or
 * non-finite R[0], I - e_B e_F or I - e_F e_B of the block recursion, or a prediction error <= 0 of a single-source solve).
 * An item with status != 0 gets NaN everywhere and perm -1.  fp64 throughout, sums in an order fixed by (K, N) alone: bitwise
 * reproducible, and an item's values do not depend on B.  K = 1: sdr is bit-equal to vs_sdr's, sir = +inf, sar = sdr. */
/* bytes of workspace vs_bss_eval needs; 0 for arguments out of range (B, N as vs_sdr, 1 <= K <= 6) */
size_t vs_bss_eval_workspace_bytes(int B, int K, long long N);
/* ref, est: [B][K][N] fp32; sdr, sir, sar: [B][K] doubles (dB); perm: [B][K] ints; status: [B] ints; pairs: NULL or
 * [B][3][K][K] doubles indexed [criterion sdr/sir/sar][estimate][reference], off-diagonal NaN when compute_permutation == 0.
 * ws: vs_bss_eval_workspace_bytes(B, K, N) bytes, 256-byte aligned.  All launches on `stream`, no synchronisation. */
int vs_bss_eval(const float* ref, const float* est, int B, int K, long long N, int compute_permutation,
                double* sdr, double* sir, double* sar, int* perm, int* status, double* pairs,
                void* workspace, size_t workspace_bytes, void* stream);

/* =============================================================================================
 * ABI 11.  The GE2E speaker encoder, inference only: reference audio -> the d-vector `dvec` that vs_forward* take
 * (notebooks/GE2E-Seungwonpark-ExtractSpeakerEmbedding-...py with ap.get_mel, utils/audio_processor.py:460-467, in front):
 *   mel  = log10(mel_basis @ |stft(wav)|^2 + 1e-6)                                               [n_mels][T], T = 1 + n / hop
 *   x    = nn.LSTM(n_mels -> hidden, layers)(mel.unfold(1, window, stride))[:, -1, :]            [N][hidden]
 *   proj = x @ proj_w^T + proj_b                                                                  [N][emb]
 *   dvec = mean over the utterance's windows of proj / |proj|_2                                   [emb]
 * nn.LSTM semantics: gate order i, f, g, o; bias b_ih + b_hh; zero initial state per window; layer l+1 reads layer l's h.
 * The encoder is frozen (the reference never trains it): there is no backward pass.
 * ============================================================================================= */
typedef struct vs_speaker_dims {
  int n_mels;   /* 40                                                                  */
  int hidden;   /* 768; must be a multiple of 8                                        */
  int layers;   /* 3; 1 .. 4                                                           */
  int emb;      /* 256                                                                 */
  int window;   /* 80 mel frames per window                                            */
  int stride;   /* 40                                                                  */
  int math;     /* VS_MATH_F16X3 (split-f16 products, fp32 accumulate) or VS_MATH_FP32 (plain fp32 FMA: the cross-check arm);
                   VS_MATH_BF16 is refused with an error (no single-product arm is built) */
} vs_speaker_dims;

typedef struct vs_speaker_params {
  const float* w_ih[4];       /* lstm.weight_ih_l{k}  [4 hidden][n_mels] (k = 0), [4 hidden][hidden] (k > 0) */
  const float* w_hh[4];       /* lstm.weight_hh_l{k}  [4 hidden][hidden]                                     */
  const float* b_ih[4];       /* lstm.bias_ih_l{k}    [4 hidden]                                             */
  const float* b_hh[4];       /* lstm.bias_hh_l{k}    [4 hidden]                                             */
  const float* proj_w;        /* proj.linear_layer.weight [emb][hidden]                                      */
  const float* proj_b;        /* proj.linear_layer.bias   [emb]                                              */
} vs_speaker_params;

/* Weights packed once (vs_prepare_weights' counterpart): fp32 copies of what the small launches read, and per layer
 * [W_ih | W_hh] as split-f16 planes in matrix-core fragment order with their power-of-two scale (VS_MATH_F16X3) or as fp32 rows
 * (VS_MATH_FP32).  vs_speaker_prepared_bytes depends on the dims alone (0 + vs_last_error for bad dims); the buffer is 256-byte
 * aligned; the caller re-prepares when a parameter or dims.math changes.  vs_speaker_embed reads the prepared buffer only. */
size_t vs_speaker_prepared_bytes(const vs_speaker_dims* dims);
int vs_speaker_prepare(const vs_speaker_dims* dims, const vs_speaker_params* params, void* prepared, size_t prepared_bytes, void* stream);
/* Workspace of vs_speaker_embed for N windows over total_frames mel frames (monotone in both, multiple of 256; 0 + vs_last_error for bad arguments). */
size_t vs_speaker_workspace_bytes(const vs_speaker_dims* dims, int N, int total_frames);
/* mel [n_mels][total_frames]: the log-mels of U utterances side by side along time.  utt_frames [U + 1] and utt_windows [U + 1]
 * (device int32): utterance u owns frames [utt_frames[u], utt_frames[u+1]) and windows [utt_windows[u], utt_windows[u+1]) of the N;
 * window n of utterance u covers frames utt_frames[u] + (n - utt_windows[u]) * stride + [0, window) -- the windows are gathered
 * here, no unfolded copy exists.  An utterance may own no window (shorter than `window`): its d-vector is all zero.
 * Outputs, each may be NULL: h_last [N][hidden] (last layer, last step), proj [N][emb] (un-normalised), dvec [U][emb].
 * window + layers - 1 step launches on `stream`, one per tick of the layer wavefront; nothing persistent, no synchronisation.
 * A window's h_last / proj do not depend on N or on its position in the batch (bitwise). */
int vs_speaker_embed(const vs_speaker_dims* dims, const void* prepared, size_t prepared_bytes, const float* mel, int total_frames,
                     const int* utt_frames, const int* utt_windows, int U, int N, float* h_last, float* proj, float* dvec,
                     void* workspace, size_t workspace_bytes, void* stream);
/* ap.get_mel for ONE clip of n samples, n > n_fft / 2 and otherwise any length (reflection at the clip's true end):
 * wav [n] -> mel [n_mels][1 + n / hop] = log10(mel_basis @ |D|^2 + 1e-6), D = librosa.stft(n_fft, hop, win, hann, center, reflect).
 * dims: n_fft, hop, win and F = n_fft / 2 + 1 are read (B, T and the dB levels are not).  mel_basis [n_mels][F]: the caller's
 * (librosa.filters.mel).  The STFT is vs_wav_to_spec's split-f16 contraction. */
size_t vs_logmel_workspace_bytes(const vs_loss_dims* dims, long long n, int n_mels);
int vs_wav_to_logmel(const vs_loss_dims* dims, const float* wav, long long n, const float* mel_basis, int n_mels, float* mel,
                     void* workspace, size_t workspace_bytes, void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  Training mixtures from a pool of clean utterances resident on the device: the arithmetic of mix_wavfiles
 * (utils/generic_utils.py:300-345: librosa.effects.trim(top_db=20), crop to audio_len, add, divide by 1.1 max|mixed|).
 * The pool is ONE flat fp32 buffer of `total` samples, 16-byte aligned; clip i is samples[offsets[i] : offsets[i+1]].
 *
 * vs_trim_bounds: bounds[i] = (start, end) of librosa.effects.trim(y, top_db=20) with its defaults frame_length = 2048,
 * hop_length = 512, ref = np.max (librosa 0.7: centred frames, reflect padding), defined as
 *   yp     = y (n samples) padded by 1024 samples on each side by reflection without the edge sample
 *   mse[f] = mean(yp[512 f : 512 f + 2048]^2), f = 0 .. n / 512
 *   frame f is non-silent when max(1e-10, mse[f]) / max(1e-10, max_f mse[f]) > 1e-2
 *   start  = 512 * first non-silent f, end = min(n, 512 * (last non-silent f + 1)); (0, 0) without one
 * (an all-zero clip has every frame at the clamp: ratio 1, bounds (0, n)).  Sums in fp64.  peak, when not NULL: [N] fp32,
 * max |y| over [start, end).  The padding reflects at the clip's own ends: a neighbouring clip is never read.
 * offsets: [N + 1] int64 on the device; offsets_host: the same values in HOST memory (the one host pointer of this ABI), checked
 * here before anything is launched: a clip shorter than 1025 samples (the reflection would wrap) or longer than 2^30 is refused
 * with -1 and a message.  workspace: vs_trim_workspace_bytes(total, N) bytes, 256-byte aligned.  One launch, a workgroup per clip.
 * ============================================================================================= */
size_t vs_trim_workspace_bytes(long long total, int N);
int vs_trim_bounds(const float* samples, long long total, const long long* offsets_host, const long long* offsets, int N,
                   int* bounds, float* peak, void* workspace, size_t workspace_bytes, void* stream);
/* One batch of mixtures.  clean_at, interf_at: [B] int64 on the device, the index in the flat buffer of each item's first sample
 * (clip offset + trim start + crop offset; any alignment).  Per item b, with c = samples[clean_at[b] : + L], i = samples[interf_at[b] : + L]:
 *   m = max_j |c[j] + i[j]| (sum in fp32),  norm[b] = float(1.1 * double(m)),
 *   mixed_wav[b] = (c + i) / norm,  target_wav[b] = c / norm   (IEEE fp32 division)
 * m == 0 (the reference divides by zero there): valid[b] = 0 and both rows are zero; otherwise valid[b] = 1.  An index outside
 * [0, total - L] is not read: valid[b] = -1, rows of zeros.  invalid_count, when not NULL: one int32 on the device, incremented
 * once per item with valid != 1 (never cleared here).  mixed_wav, target_wav [B][L] (16-byte aligned), norm [B], valid [B] int32.
 * 1 <= B <= 65535.  The maximum is order-independent: two calls give the same bits.  Four launches on `stream` (norm doubles as the
 * maximum's slot and is cleared first); nothing is allocated, no environment variable is read. */
int vs_mix_clips(const float* samples, long long total, const long long* clean_at, const long long* interf_at, int B, int L,
                 float* mixed_wav, float* target_wav, float* norm, int* valid, int* invalid_count, void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  The noisy training items WITHOUT voice overlay: the arithmetic of mix_wavfiles_without_voice_overlay
 * (utils/generic_utils.py:27-296).  The target speaker and the interferer take turns, two noise recordings run under the whole item,
 * and every triplet yields four items.  librosa.effects.split is RESTATED here as vs_trim_bounds restates trim: NOBODY HAS COMPARED
 * IT WITH A LIBROSA RUN.  This text is the contract for the C entries; tests/overlay_ref.py restates the whole recipe in fp64.
 *
 * vs_clip_range: range[i] = (min, max) of samples[offsets[i] + bounds[i][0] : offsets[i] + bounds[i][1]] in fp32, exact: what
 * sklearn.preprocessing.minmax_scale reads of a trimmed clip.  bounds [N][2] int32 on the device (vs_trim_bounds' output; clamped
 * to the clip), or NULL: the whole clip.  An empty region gives (0, 0).  offsets / offsets_host as for vs_trim_bounds (a clip may
 * have any length from 0 to 2^30 here).  One launch, a workgroup per clip; once per pool.
 * ============================================================================================= */
int vs_clip_range(const float* samples, long long total, const long long* offsets_host, const long long* offsets, const int* bounds,
                  int N, float* range, void* stream);
/* vs_split_point: librosa.effects.split(y, top_db) at its defaults (frame_length 2048, hop_length 512, ref = np.max) for B regions
 * y_b = samples[at_b : at_b + n_b] of the flat buffer (any alignment), with mse[f] and the clamp of vs_trim_bounds:
 *   frame f (0 .. n / 512) is non-silent when max(1e-10, mse[f]) / max(1e-10, max_f mse[f]) > ratio[b]
 *   an interval is a maximal run [f0, f1) of non-silent frames; in samples [512 f0, min(n, 512 f1))
 *   count[b] = number of intervals (>= 1: the loudest frame is never silent; an all-zero region is one interval (0, n))
 *   split[b] = end of interval number count / 2 (from 0): the reference's clip_idx = parts[int(len(parts) / 2)][1]
 * ratio [B] fp64 on the device: 10^(-top_db / 10), 1e-2 for the clean voice (top_db = 20), 10^-1.5 for the interferer (15).
 * The promises above hold for 0 < ratio < 1; the ratios live on the device and are not checked: with ratio >= 1 (or NaN) no
 * frame is non-silent, and count[b] = 0, split[b] = n, no interval is written.
 * regions [B][2] int64 on the device = (at, n); regions_host the same values in HOST memory, checked here before anything is
 * launched: 1025 <= n <= 2^30 and 0 <= at <= total - n, else -1 and a message.  The reflect padding reflects at the region's own
 * ends: no sample outside [at, at + n) is read.  intervals, when not NULL: [B][cap][2] int32, the first min(count, cap) intervals of
 * every region (the rest of a row is not written).  workspace: vs_split_workspace_bytes(n_max, B) bytes, 256-byte aligned, n_max >=
 * every n.  Sums in fp64.  1 <= B <= 2^24.  One launch, a workgroup per region. */
size_t vs_split_workspace_bytes(long long n_max, int B);
int vs_split_point(const float* samples, long long total, const long long* regions_host, const long long* regions,
                   const double* ratio, int B, int* count, int* split, int* intervals, int cap, void* workspace,
                   size_t workspace_bytes, void* stream);
/* vs_mix_sequence: one batch of items, each up to three segments end to end over one continuous noise bed.
 * Segment s of item b is samples[src_at[s] : src_at[s] + len[s]] (len 0: absent; the item's length n = len[0] + len[1] + len[2] <= L).
 * noise1_at / noise2_at: the index in `noise` (a second flat buffer, noise_total samples) that goes with OUTPUT sample 0 -- the
 * noise index always runs on with the output index ("noise without interruption", :134-137).  With s the segment of output sample
 * t, x its sample, and n1 = noise[noise1_at + t], n2 = noise[noise2_at + t], all fp32 and in this order:
 *   v = fmaf(gain[s], x, bias[s])
 *   if noise_sel[s] >= 0:  v = v + fmaf(ngain[noise_sel[s]], n1 + n2, nbias[noise_sel[s]])
 *   mixed[t] = v / norm,   target[t] = in_target[s] ? v / norm : 0.0f          (IEEE fp32 division)
 * ngain / nbias are formed on the device, nothing is read back: with (nmin, nmax) the fp32 minimum and maximum of
 * noise[range_at1 + j] + noise[range_at2 + j] (fp32 sum), j < range_len, and den = double(nmax) - double(nmin), or 1 when that is 0,
 *   scale_k = (double(hi[k]) - double(lo[k])) / den,  ngain[k] = float(scale_k),  nbias[k] = float(double(lo[k]) - double(nmin) * scale_k)
 * (fp64, no fused multiply-add): minmax_scale(noise, feature_range=(lo[k], hi[k])) for k = 0, the plain noise draw (:105-110),
 * and k = 1, the random-amplitude draw (:45-49).
 *   m = max_t |v|,  norm[b] = float(1.1 * double(m));  with norm_in ([B], device) the maximum is skipped and norm[b] = norm_in[b]
 * (kinds 2 and 3 divide by kind 1's norm_factor, :218-227).  Samples n .. L - 1 of both rows are 0.0f.
 * valid[b]: 1; 0 when norm[b] == 0 (rows of zeros); -1 and rows of zeros, with nothing of the item read, when a len is negative or
 * n > L, a segment leaves `samples`, noise_sel is outside -1 .. 1, or -- for an item with a noise_sel >= 0 -- [noise*_at, + n) or
 * [range_at*, + range_len) leaves `noise` or range_len is outside 1 .. R.  invalid_count as for vs_mix_clips.
 * aux [B][8] fp32: {nmin, nmax, m, ngain[0], nbias[0], ngain[1], nbias[1], 0} (zeros for an item without noise; m is 0 with
 * norm_in); it doubles as the call's scratch.  mixed_wav, target_wav [B][L], 16-byte aligned; BOTH NULL: only norm, aux and valid
 * are computed (the planner gets every triplet's kind-1 norm this way).  L, R: row capacity and the largest range_len, 1 .. 2^30.
 * 1 <= B <= 65535.  Minimum and maxima are order-independent: two calls give the same bits.  Passes on `stream`: clear (a memset),
 * noise range, maximum, scale, finalise; nothing is allocated, no environment variable is read. */
typedef struct vs_seq_item {
  long long src_at[3];              /* index in `samples` of each segment's first sample */
  long long noise1_at, noise2_at;   /* index in `noise` for output sample 0 */
  long long range_at1, range_at2;   /* the slice whose n1 + n2 minimum and maximum feed the noise affines */
  int len[3];
  int in_target[3];
  int noise_sel[3];                 /* -1: no noise, 0: the plain affine, 1: the random-amplitude affine */
  int range_len;
  float gain[3], bias[3];
  float lo[2], hi[2];               /* feature ranges: [0] plain, [1] random amplitude */
} vs_seq_item;                      /* 136 bytes: 7 int64, 10 int32, 10 fp32 */
int vs_mix_sequence(const float* samples, long long total, const float* noise, long long noise_total, const vs_seq_item* items,
                    int B, int L, int R, const float* norm_in, float* mixed_wav, float* target_wav, float* norm, float* aux,
                    int* valid, int* invalid_count, void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  Sample-rate conversion on the device: what librosa.load(path, sr=...) does on the CPU in front of
 * mix_wavfiles and of both audio processors' load_wav.  The filter is a Kaiser-windowed sinc with the constants of resampy's
 * kaiser_best AS REMEMBERED, its window evaluated analytically and not through resampy's interpolated table: RESTATED, NOT
 * COMPARED WITH A RESAMPY OR LIBROSA RUN (neither is available where this was written).  This text is the contract.
 *
 * For integer rates sr_in, sr_out:  g = gcd,  L = sr_out / g,  M = sr_in / g,  s = min(1, L / M),
 *   Z = 64,  H = ceil(Z / s),  T = 2 H + 1 taps,  beta = 14.769656459379492,  rho = 0.9475937167399596
 *   h(t)  = rho sinc(rho t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta)   for |t| < Z, else 0        (sinc(x) = sin(pi x) / (pi x))
 *   n_out = ceil(n_in L / M)                                                                      (librosa.load's fix_length)
 *   y[n]  = sum_{j = -H .. H}  s h(s (r / L - j)) x[b + j],   b = floor(n M / L),  r = (n M) mod L,  x[k] = 0 outside [0, n_in)
 * with n M in 64 bits.  The taps are a polyphase bank, bank[r][j + H] (L rows of T fp32), each tap evaluated in fp64 (the I0 series
 * included) and rounded once to fp32.  sr_in == sr_out is a copy: L = M = 1, H = 0, T = 1, the one tap 1.0.  A pair of rates with
 * L T 4 > 4 MiB is refused (16000 <-> 44101, for example); the pairs in use need at most 230 KB.
 *
 * POSITION INDEPENDENCE: y[n] = fmaf(tap[T-1], x[b+H], ... fmaf(tap[0], x[b-H], +0)), one fp32 chain in ascending j: its bits are
 * a function of n and of the T samples it reads, never of the tile, workgroup, row, clip, window or call that computed it.  A stream
 * resampled in pieces is therefore bit-identical to the stream resampled at once.
 *
 * vs_resample_plan: host only, no device.  Fills *dims (tile_periods and lds_bytes describe the launch, see csrc/resample.hip;
 * tile_periods == 0: the direct kernel); -1 and a message for non-positive rates and refused pairs.  Every other call checks the
 * dims it is given against a plan of its own.  vs_resample_out_len: ceil(n_in L / M), -1 for n_in < 0.
 * vs_resample_bank: fills bank (dims->bank_bytes bytes, 16-byte aligned, device) on `stream`; once per pair of rates.
 * ============================================================================================= */
typedef struct vs_resample_dims {
  int sr_in, sr_out;
  int L, M, H, T;
  int tile_periods;      /* periods (L outputs from M inputs) one workgroup owns */
  int lds_bytes;         /* of that workgroup */
  size_t bank_bytes;     /* L * T * 4 */
} vs_resample_dims;
int vs_resample_plan(int sr_in, int sr_out, vs_resample_dims* dims);
long long vs_resample_out_len(const vs_resample_dims* dims, long long n_in);
int vs_resample_bank(const vs_resample_dims* dims, float* bank, void* stream);
/* Outputs [y_first, y_first + y_count) of B streams.  x: row b at x + b * x_stride holds stream samples [x_first, x_first + x_count)
 * (x_first may be negative: the samples in front of the stream are zero anyway); y: row b at y + b * y_stride receives y_count
 * outputs.  stream_len: the stream's length, or -1 while its end is not known; samples outside [0, stream_len) are zero.  An
 * output that needs a sample inside the stream but outside the buffer is refused here, on the host (-1 and a message): the
 * kernels read nothing outside [x_first, x_first + x_count).  With stream_len >= 0, y_first + y_count <= ceil(stream_len L / M).
 * 1 <= B <= 65535, y_count >= 0 (0: nothing is launched).  Any alignment; rows are stored 16 bytes per lane where y allows it. */
int vs_resample(const vs_resample_dims* dims, const float* bank, const float* x, long long x_first, long long x_count,
                long long x_stride, long long stream_len, float* y, long long y_first, long long y_count, long long y_stride,
                int B, void* stream);
/* N clips of unequal length in flat buffers (the pool's layout), one launch sequence on `stream` for all of them.  clips [N][3]
 * int64 on the device, clips_host the same values in HOST memory (checked here before anything is launched): clip i is
 * in[c[0] : c[0] + c[1]] and its ceil(c[1] L / M) outputs go to out[c[2] : ...].  Any alignment; nothing outside a clip is read and
 * nothing outside its outputs is written.  Clips of no samples are allowed.  The output regions must not overlap (not checked). */
int vs_resample_clips(const vs_resample_dims* dims, const float* bank, const float* in, long long in_total, float* out,
                      long long out_total, const long long* clips_host, const long long* clips, int N, void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  Programme loudness on the device: the other half of the reference's scripts/normalise-resample.sh
 * (`ffmpeg-normalize <file> -ar 16000` per utterance; -ar is vs_resample_clips).  The measure is ITU-R BS.1770-4 integrated
 * loudness of a MONO signal; the normalisation is ONE LINEAR GAIN per clip with a peak cap, not ffmpeg's `loudnorm` in its dynamic
 * mode.  The K-weighting constants are libebur128's AS REMEMBERED (at 48 kHz they give the coefficient table of BS.1770 to 9e-16):
 * RESTATED, NOT COMPARED WITH AN FFMPEG OR LIBEBUR128 RUN (neither is available where this was written).  This text is the contract;
 * tests/loudness_ref.py restates it in fp64.
 *
 * Mono clip x[0 .. n) fp32 at the integer rate fs, 8000 <= fs <= 192000.  All arithmetic below is fp64.
 * K-weighting: two biquads re-derived per rate by the bilinear transform,
 *   stage 1 (shelf):     f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *     K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2
 *     b1 = {(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0},  a1 = {2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0}
 *   stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan(pi f0 / fs), d = 1 + K/Q + K^2
 *     b2 = {1, -2, 1},  a2 = {2 (K^2 - 1)/d, (1 - K/Q + K^2)/d}
 * both in transposed direct form II from a zero state s = (s1, s2, s3, s4), per sample:
 *   u = b1[0] x + s1;  s1 = b1[1] x - a1[0] u + s2;  s2 = b1[2] x - a1[1] u
 *   w = u + s3;        s3 = -2 u - a2[0] w + s4;      s4 = u - a2[1] w
 * Blocks: S = (fs + 5) / 10 (integer division) samples per 100 ms sub-block; m = floor(n / S) sub-blocks with energies
 *   e_k = sum of w^2 over [k S, (k + 1) S); samples from m S on are never counted; blocks j = 0 .. m - 4 have
 *   z_j = (e_j + e_{j+1} + e_{j+2} + e_{j+3}) / (4 S).
 * Gates: absolute z_j > 10^((-70 + 0.691) / 10); relative z_j > 0.1 * mean(z over the absolute-gated blocks) (-10 LU);
 *   lufs = -0.691 + 10 log10(mean(z over the blocks past both gates));
 *   counts = (number of blocks = max(m - 3, 0), past the absolute gate, past both).
 *   With m < 4, or with no block past the absolute gate: lufs = -inf, valid = 0; otherwise valid = 1.
 * Peak: peak = max |x| over all n samples in fp32, exact and order-independent (0 for n = 0).
 *
 * The device evaluates the recurrence in segments of S samples (csrc/loudness.hip): the state behind sub-block k is
 * s(k+1) = step s(k) + p(k), p(k) the state the sub-block leaves from a zero state.  The products and sums of the recurrence are
 * fused multiply-adds there, so e_k agrees with the serial fp64 filter to rounding (a few 1e-14 dB in lufs), not to the bit.
 * A clip's results are bit-identical whatever its offset in the buffer, its neighbours, N and the call.
 *
 * vs_loudness_plan: host only, no device; -1 and a message for a rate outside 8000 .. 192000.  step[r][c]: component r of the state
 * after S zero-input samples from the unit state c, built by running the recurrence itself S times (not by matrix powers).  Every
 * other call checks the dims it is given against a plan of its own.
 * vs_loudness: clips [N][2] int64 on the device = (at, n), clip i = samples[at : at + n], any alignment, 0 <= n <= 2^30;
 * clips_host the same values in HOST memory, checked here before anything is launched (-1 and a message for a clip that leaves
 * [0, total] or is longer than 2^30).  lufs [N] fp64, peak [N] fp32, counts [N][3] int32, valid [N] int32, all on the device.
 * energy: NULL, or the e_k of all clips, clip i's m_i values from energy[energy_at[i]] on (energy_at [N] int64 on the device; the
 * regions are the caller's and are not checked).  workspace: 256-byte aligned; vs_loudness_workspace_bytes(dims, total, N) bytes
 * serve any N clips of one buffer of `total` samples that do not overlap (clips that overlap may need more: a workspace too small
 * for the table is refused with a message; 0 from the size function is an error).  Nothing outside a clip is read, nothing is
 * allocated, no environment variable is read; NULL pointers are refused with a message.  Five launches on `stream` for up to 65535
 * clips (slots, zero-state sweep, scan, energy sweep, gate), two more per further 65535.
 * vs_scale_clips: x = x * gain[i] (one fp32 multiply) for every sample of clip i, in place; gain [N] fp32 on the device; the table as
 * above.  Nothing outside a clip is read or written; clips of a table must not overlap (not checked).  16-byte loads and stores where
 * the alignment allows, single floats at a clip's head and tail.
 * ============================================================================================= */
typedef struct vs_loudness_dims {
  int sample_rate, sub;                  /* sub = S */
  double b1[3], a1[2], b2[3], a2[2];
  double step[4][4];                     /* s(k+1) = step s(k) + p(k) */
} vs_loudness_dims;
int vs_loudness_plan(int sample_rate, vs_loudness_dims* dims);
size_t vs_loudness_workspace_bytes(const vs_loudness_dims* dims, long long total, int N);
int vs_loudness(const vs_loudness_dims* dims, const float* samples, long long total, const long long* clips_host,
                const long long* clips, int N, double* lufs, float* peak, int* counts, int* valid, double* energy,
                const long long* energy_at, void* workspace, size_t workspace_bytes, void* stream);
int vs_scale_clips(float* samples, long long total, const long long* clips_host, const long long* clips, const float* gain, int N,
                   void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  Speech intelligibility on the device: STOI (Taal, Hendriks, Heusdens, Jensen 2011) and its extended
 * form ESTOI (Jensen, Taal 2016), the scores reported beside the SDR.  The algorithm is pystoi's AS REMEMBERED: RESTATED, NOT
 * COMPARED WITH A PYSTOI RUN (pystoi is not available where this was written), so parity with pystoi's own numbers is unpinned; in
 * particular pystoi resamples to 10 kHz with an Octave-style filter and this project uses vs_resample.  This text is the contract;
 * tests/stoi_ref.py restates it in fp64.
 *
 * Both signals x (reference) and y (estimate) are fp32 at fs = 10000 Hz and share a length n.  Every sum and product below is fp64.
 * Constants: frame W = 256, hop 128, NFFT = 512, J = 15 bands, segment N = 30 frames, DYN = 40 dB, clip factor 1 + 10^(15/20),
 *   EPS = 2^-52, window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), i = 0 .. 255 (hanning(258) without its two zeros).
 * Frames: F = (n - 256) / 128 + 1 (integer division) for n >= 256, else 0; frame f = samples [128 f, 128 f + 256).
 * Silent-frame removal, decided by x alone: e_f = 20 log10(sqrt(sum (w x_f)^2) + EPS); frame f is kept iff max_f(e) - 40 - e_f < 0;
 *   q = 0 .. Mk - 1 indexes the kept frames in order.  Both signals are rebuilt by overlap-adding their own windowed kept frames at
 *   128 q (length (Mk - 1) 128 + 256).
 * Band envelopes: the rebuilt signals are framed again with the same W, hop and w (exactly Mk frames), every frame zero-padded to 512
 *   samples, P[k] = |DFT_512|^2; band j sums P[k] over lo_j <= k < hi_j, the edges being the bins of the 10000 / 512 Hz grid nearest
 *   to 150 * 2^((2 j -+ 1) / 6) Hz: (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43) (43,55) (55,69) (69,87) (87,109)
 *   (109,138) (138,174) (174,219); X[j][q] = sqrt(band sum) of x, Y[j][q] of y.
 * Segments: m = 30 .. Mk, the blocks X[:, m - 30 : m] and Y[:, m - 30 : m]; M = Mk - 29 of them.
 * STOI: per band row, c = |x| / (|y| + EPS), y' = min(c y, x (1 + 10^0.75)); the row means of x and y' are subtracted, each is
 *   divided by (its norm + EPS); d = sum x y' / (J M).
 * ESTOI: both blocks: subtract the row mean and divide by (row norm + EPS), then subtract the column mean and divide by (column norm
 *   + EPS); d = sum x y / (N M).
 * status 0 = ok; 1 = Mk < 30 (pystoi warns and returns 1e-5): d = 1e-5 exactly.
 * Every reduction has a fixed order (csrc/stoi.hip lists them); a clip's results are bit-identical whatever its offset in the
 * buffers, its neighbours, R and the call.  The device's sums are ordered differently from the restatement's and its products may be
 * fused, so d agrees with it to rounding, not to the bit; the keep mask is a threshold, exact unless a frame sits on it.
 *
 * vs_stoi_plan: host only, no device: the constants above and the band edges, computed (first nearest bin).  Every other call checks
 * the dims it is given against a plan of its own.
 * vs_stoi: ref and est are flat buffers of `total` samples; clips [R][2] int64 on the device = (at, n): pair i is ref[at : at + n]
 * and est[at : at + n], any alignment, 0 <= n <= 2^24; clips_host the same values in HOST memory, checked here before anything is
 * launched (-1 and a message for a clip that leaves [0, total] or is longer than 2^24).  extended: 0 = STOI, 1 = ESTOI.
 * d [R] fp64, frames [R][2] int32 = (F, Mk), status [R] int32, all on the device.  tob: NULL, or the envelopes of all clips, clip i's
 * X then Y as [2][15][Mk_i] from tob[tob_at[i]] on (tob_at [R] int64 on the device; 30 F_i values are always enough; the regions are
 * the caller's and are not checked).  workspace: 256-byte aligned; vs_stoi_workspace_bytes(dims, total, R) bytes serve any R clips of
 * buffers of `total` samples that do not overlap (clips that overlap may need more: a workspace too small for the table is refused
 * with a message; 0 from the size function is an error).  Nothing outside a clip is read, nothing is allocated, no environment
 * variable is read; NULL pointers are refused with a message.  At most six launches on `stream` for any R (frame slots, frame
 * energies, gate and compaction, band envelopes, segment correlations, fold); the launches without work for the table are left out.
 * ============================================================================================= */
typedef struct vs_stoi_dims {
  int frame, hop, nfft, bands, seg;
  int lo[15], hi[15];                    /* band j = bins lo[j] .. hi[j] - 1 */
  double clip, dyn_db;
} vs_stoi_dims;
int vs_stoi_plan(vs_stoi_dims* dims);
size_t vs_stoi_workspace_bytes(const vs_stoi_dims* dims, long long total, int R);
int vs_stoi(const vs_stoi_dims* dims, const float* ref, const float* est, long long total, const long long* clips_host,
            const long long* clips, int R, int extended, double* d, int* frames, int* status, double* tob, const long long* tob_at,
            void* workspace, size_t workspace_bytes, void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  Reverberation: room impulse responses of a shoebox room by the image method, a per-row FIR that applies
 * them, and the energy of a row (the level control of the reverberant mixtures).  The image method is RESTATED (Allen & Berkley 1979),
 * NOT COMPARED WITH A PYROOMACOUSTICS OR RIR-GENERATOR RUN: neither package was available where this was written.  This text is the
 * contract; tests/reverb_ref.py restates it in fp64.
 *
 * vs_room: one response.  size = (L_x, L_y, L_z) in metres, src = s and mic = m inside the room (0 < s < L, 0 < m < L per axis),
 * beta = reflection coefficients of the walls (x0, x1, y0, y1, z0, z1), each in -1 .. 1, c in m/s, fs in Hz, 1 <= nh <= 8192 taps,
 * max_order >= 0 or -1 = no limit.
 * Image sum: for parities q, j, k in {0, 1} and integers n, l, p
 *   R   = ((1 - 2q) s_x - m_x + 2 n L_x, (1 - 2j) s_y - m_y + 2 l L_y, (1 - 2k) s_z - m_z + 2 p L_z)
 *   d   = sqrt((R_x^2 + R_y^2) + R_z^2),  tau = d fs / c
 *   amp = beta_x0^|n - q| beta_x1^|n| beta_y0^|l - j| beta_y1^|l| beta_z0^|p - k| beta_z1^|p| / (4 pi d),  0^0 = 1
 * an image is dropped when max_order >= 0 and |2n - q| + |2l - j| + |2p - k| > max_order.
 *   h[t] = sum amp w(t - tau), t = 0 .. nh - 1;  w(u) = sinc(u) (1 + cos(pi u / 40)) / 2 for |u| < 40, else 0, sinc(u) = sin(pi u) / (pi u)
 * An image with tau - 40 >= nh adds nothing: |n| <= floor((nh + 40) c / (2 fs L_x)) + 1 covers every other one (likewise l, p).
 * Everything is fp64 and h[t] is rounded ONCE to fp32.  u is formed as (t - rint(tau)) - (tau - rint(tau)) and sin(pi u) as
 * -(-1)^(t - rint(tau)) sinpi(tau - rint(tau)): one sine per image.  Every tap adds its images in ONE order, the enumeration order of
 * (q, j, k, n, l, p) with p running fastest (an image whose window misses the tap adds exactly 0 and may be skipped), so the bits of a
 * response depend on its descriptor alone: not on its row, its neighbours, R or the call.  No atomics.
 * rooms_host [R] in HOST memory is checked before anything is launched; rooms [R] is the same table on the device.  Refused with -1
 * and a message: a non-positive size, a source or receiver outside the room, d = 0 (source on the receiver), beta outside -1 .. 1,
 * non-positive c or fs, nh outside 1 .. min(8192, H), max_order < -1, a room so small that the response has more than 2^24 images.
 * h [R][H] fp32 on the device, 1 <= H <= 8192: row r holds its nh taps, then zeros.  1 <= R <= 65535.  A memset and one launch.
 *
 * vs_fir_rows: y[b][i] = sum_{k < nh[b]} h[hrow[b]][k] x(at[b] + i - k), i = 0 .. L - 1, where x(p) = samples[p] of the flat buffer for
 * lo[b] <= p, and 0 below lo[b].  at, lo [B] int64 and nh, hrow [B] int32 on the device; h [R][H] fp32; y [B][L].  Any alignment of
 * at.  Nothing outside [lo[b], at[b] + L) is read.  A row with lo < 0, lo > at, at + L > total, hrow outside 0 .. R - 1 or nh outside
 * 1 .. H is not read: valid[b] = -1 and a row of zeros; otherwise valid[b] = 1.  Host-checkable argument errors (NULL, B outside
 * 1 .. 65535, L outside 1 .. 2^24, H outside 1 .. 8192, total < L, an unknown math) return -1 and a message.
 *   VS_MATH_FP32:  acc = 0; for k = 0 .. nh - 1 ascending: acc = fmaf(h[k], x(at + i - k), acc).  h = {1.0f} returns x bit for bit.
 *   VS_MATH_F16X3: with mx = max |x| over the samples the row reads ([max(lo, at - nh + 1), at + L)) and mh = max |h[0 .. nh)|,
 *     sx = 2^ex with 2^14 <= mx sx < 2^15 and sh likewise (exponents clamped to +-100; 1 for a maximum of 0); every x sx and h sh is
 *     split into f16 hi = f16(v), lo = f16(v - hi); y = (sum hi_x hi_h + sum (hi_x lo_h + lo_x hi_h)) / (sx sh), the products on
 *     v_mfma_f32_32x32x16_f16 with fp32 accumulation (lo lo is dropped).  K = nh + 32 is walked in one order that depends on neither
 *     B, the row index nor the tile, from zero accumulators.  The bits of a row depend on its own samples (those it reads) and its
 *     own filter alone; not on at mod 8, its position in the batch, B or the call.  Samples in [lo, at - nh + 1) belong to no product
 *     of the row: they do not enter mx and are not multiplied (whatever their size, they cannot overflow an f16 plane).
 *     Error against the exact sum, per output: <= (2^-20 + (nh + 32) 2^-23) sum_k |h_k| |x_{n-k}| + u, where u covers the lo planes
 *     that fall into the f16 subnormals (spacing 2^-24: an error of 2^-25 / s per element):  u = nh 2^-38 mx mh
 *     (2^-25 / sx <= 2^-39 mx per sample, times |h| <= mh, plus the same for the taps), for mx, mh above 2^-85.
 * scale [B][4] fp32 (output; also this call's scratch): sx, 1 / sx, sh, 1 / sh of the row (1 for an invalid row); computed in both
 * arithmetics, used by VS_MATH_F16X3 alone.  Two launches.
 *
 * vs_row_energy: energy[b] = sum_i double(y[b][i])^2 in fp64, y [B][L]: one workgroup per row, thread t adds samples t, t + 256, ..
 * in ascending order, then a fixed binary fold of the 256 partial sums.  No atomics: two calls give the same bits.
 * ============================================================================================= */
typedef struct vs_room {
  double size[3], src[3], mic[3];
  double beta[6];                        /* x0, x1, y0, y1, z0, z1 */
  double c, fs;
  int nh, max_order;
} vs_room;
int vs_rir_shoebox(const vs_room* rooms_host, const vs_room* rooms, int R, int H, float* h, void* stream);
int vs_fir_rows(const float* samples, long long total, const long long* at, const long long* lo, const int* nh, const int* hrow, int B,
                int L, const float* h, int R, int H, int math, float* y, int* valid, float* scale, void* stream);
int vs_row_energy(const float* y, int B, int L, double* energy, void* stream);

/* =============================================================================================
 * ABI 11 (additive entries).  The FFT form of the per-row FIR: uniformly partitioned overlap-save convolution in fp32 with kept filter
 * spectra, for responses of up to 32768 taps.  tests/fir_fft_ref.py restates this text.
 *
 * Bk = VS_FIR_FFT_BLOCK = 2048, N = 2 Bk, Bk + 1 bins.  A response of nh taps is cut into P = ceil(nh / Bk) partitions,
 *   H_p = rfft(h[p Bk .. (p + 1) Bk) zero-padded to N);  taps at k >= nh count as zero whatever the row holds.
 * For row b, with x(p) = samples[p] for lo[b] <= p < at[b] + L and 0 elsewhere:
 *   window q        w_q = x(at + (q - 1) Bk .. at + (q + 1) Bk)
 *   output block j  i = j Bk .. (j + 1) Bk - 1:  y_j = the last Bk samples of irfft(sum_{p = 0 .. P - 1, ascending, from zero} rfft(w_{j-p}) H_p)
 * which is vs_fir_rows' definition of y with nh = nh[hrow[b]], fixed when the spectra were made.  Nothing outside [lo[b], at[b] + L)
 * is read.  Twiddle factors come from a table computed in fp64 and rounded once to fp32 (no fast-math sincos anywhere); every sum
 * runs in one fixed order; no atomics.
 *
 * vs_fir_spectra_bytes(R, H): the size of the spectra blob of h [R][H], 1 <= H <= 32768; 0 and a message otherwise.
 * vs_fir_spectra: builds the blob -- opaque, caller-owned: the twiddle table, the partition count of every response and the spectra.
 *   The library keeps no lazily initialised state: everything a rows call needs beside its arguments is in the blob.  nh_host [R] in
 *   HOST memory is checked before anything is launched (1 <= nh <= H, else -1 and a message); nh [R] is the same table on the device.
 *   Two launches on the caller's stream.
 * vs_fir_fft_workspace_bytes(B, L, H): the size of a rows call's workspace (the window spectra); 0 and a message when out of range.
 * vs_fir_rows_fft: the convolution.  at, lo [B] int64 and hrow [B] int32 on the device; y [B][L]; any alignment of at.  Validity as in
 *   vs_fir_rows: a row with lo < 0, lo > at, at + L > total or hrow outside 0 .. R - 1 is not read: valid[b] = -1 and a row of zeros;
 *   otherwise valid[b] = 1.  Host-checkable argument errors (NULL, B outside 1 .. 65535, L outside 1 .. 2^24, H outside 1 .. 32768,
 *   R < 1, total < L, a blob or workspace that is too small) return -1 and a message naming the value.  R and H are those the blob
 *   was made with.  The workspace is scratch: what it held before changes nothing, and nothing in it outlives the call.  Two launches.
 *
 * What holds, and what tests/test_gpu_fir_fft.py holds it to:
 *   The bits of a row depend only on the samples it reads and on its response: not on B, the row's index, hrow's value, where the
 *   response sits in the table, R, at's alignment in the flat buffer, the call, or the bytes the workspace held before.
 *   A row of zero samples gives exact zeros.
 *   Error against the exact sum, per output of block j:  |y - y64| <= kappa 2^-24 log2(N) E_j,  E_j = sum_p ||w_{j-p}||_2 ||h_p||_2
 *   (h_p: the taps of partition p).  THE BOUND IS GLOBAL TO A BLOCK: the error of a transform is spread over its 2048 outputs, so a
 *   quiet output beside a loud one carries the block's error.  vs_fir_rows' bound is per output (a multiple of sum_k |h_k| |x_{n-k}|)
 *   and does not allow that: where the quiet passages of a row matter more than its loud ones, use the direct form.
 *   kappa = 8 kappa_ref, kappa_ref the same ratio of a float32 pocketfft restatement (scipy.fft) over the test's cases, computed
 *   from the reference alone; the figures are in DESIGN.md 6.8m.
 * ============================================================================================= */
#define VS_FIR_FFT_BLOCK 2048
size_t vs_fir_spectra_bytes(int R, int H);
int vs_fir_spectra(const float* h, const int* nh_host, const int* nh, int R, int H, void* spectra, size_t spectra_bytes, void* stream);
size_t vs_fir_fft_workspace_bytes(int B, int L, int H);
int vs_fir_rows_fft(const float* samples, long long total, const long long* at, const long long* lo, const int* hrow, int B, int L,
                    const void* spectra, size_t spectra_bytes, int R, int H, void* workspace, size_t workspace_bytes, float* y, int* valid,
                    void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* VOICESPLIT_HIP_H */
