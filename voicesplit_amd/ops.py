"""Thin torch-facing wrappers over the C ABI: torch supplies device buffers and the current HIP
stream, every FLOP happens inside libvoicesplit_hip.so.  Each wrapper checks its arguments and
crosses through ``_call.call``, which makes the tensors' device current for the call.

Stage functions mirror the reference forward (models/voicesplit/model.py:66-89):
``conv_stack`` (:68-74), ``bilstm`` (:77-82), ``head`` (:83-87), ``forward`` (all of it).
The kernel-level functions (``conv64`` ...) exist for the unit tests.
"""
import ctypes
import os
from typing import Dict, Optional, Sequence

import torch

from . import _call, _lib
from ._lib import (ACT_MISH, ACT_NONE, ACT_RELU, ACT_SIGMOID, BN_EVAL, BN_TRAIN, VsDims, VsParams,
                   VsWsLayout, check)

ACT_CODES = {"relu": ACT_RELU, "mish": ACT_MISH, "none": ACT_NONE, "sigmoid": ACT_SIGMOID}

# conv.{idx} of the reference nn.Sequential: (Conv2d index, BatchNorm2d index) for cnn1..cnn8
CONV_INDEX = ((1, 2), (5, 6), (9, 10), (13, 14), (17, 18), (21, 22), (25, 26), (28, 29))
# vs_params / vs_grads field <- state_dict key: per direction "lstm.{key}" + ("", "_reverse"), and the head
LSTM_FIELDS = (("w_ih", "weight_ih_l0"), ("w_hh", "weight_hh_l0"), ("b_ih", "bias_ih_l0"), ("b_hh", "bias_hh_l0"))
HEAD_FIELDS = (("fc1_w", "fc1.weight"), ("fc1_b", "fc1.bias"), ("fc2_w", "fc2.weight"), ("fc2_b", "fc2.bias"))

MATH_CODES = {"fp32": _lib.MATH_FP32, "f16x3": _lib.MATH_F16X3, "bf16": _lib.MATH_BF16}
_DEFAULT_MATH = os.environ.get("VOICESPLIT_CONV_MATH", "f16x3")


def set_conv_math(name: str):
    """Arithmetic of the dense contractions (64->64 convs forward / data / weight gradient, LSTM
    input GEMMs): "f16x3" (default) = fp32 operands split into two f16 halves, three products on
    the f16 matrix cores, fp32 accumulate -- fp32-class accuracy (same parity tolerances) at 3/16
    of the matrix-pipe time (csrc/conv_f16x3.hip); "fp32" = the f32 matrix cores, bitwise an fmaf
    chain; "bf16" (BASELINE configs[2], opt-in only) = operands rounded to bf16, ONE product on the
    bf16 matrix cores, fp32 accumulate and fp32 everywhere else -- a third of the matrix work of f16x3 at
    bf16 accuracy (not the 1e-4 contract: tests/test_gpu_bf16.py states what it holds).  Also
    selectable with VOICESPLIT_CONV_MATH."""
    global _DEFAULT_MATH
    if name not in MATH_CODES:
        raise ValueError(f"conv math must be one of {sorted(MATH_CODES)}")
    _DEFAULT_MATH = name


def get_conv_math() -> str:
    return _DEFAULT_MATH


def make_dims(B, T, F, E, H, FC1, FC2, math: Optional[str] = None) -> VsDims:
    return VsDims(int(B), int(T), int(F), int(E), int(H), int(FC1), int(FC2), MATH_CODES[math or _DEFAULT_MATH])


def workspace_layout(dims: VsDims) -> VsWsLayout:
    lay = VsWsLayout()
    check(_lib.load().vs_workspace_layout(ctypes.byref(dims), ctypes.byref(lay)), "vs_workspace_layout")
    return lay


def get_workspace(dims: VsDims, device) -> torch.Tensor:
    """Caller-owned scratch (the library never allocates): the "model" slot of the device, grown to these dims."""
    return _call.scratch("model", _call.sized("workspace_bytes", ctypes.byref(dims)), device)


def get_multi_workspace(dims: VsDims, K: int, device) -> torch.Tensor:
    """Scratch of the multi-speaker calls (vs_multi_workspace_bytes: conv buffers for B, sequence buffers for B*K): the "multi" slot
    of the device, grown to (dims, K).  At B = 64 it holds gigabytes; ``release_workspaces`` returns it."""
    return _call.scratch("multi", _call.sized("multi_workspace_bytes", ctypes.byref(dims), int(K)), device)


def release_workspaces():
    """Every scratch slot of every module and the free tapes go back to torch's allocator."""
    _call.release_scratch()
    _TAPE_POOL.clear()


def ws_view(ws: torch.Tensor, offset: int, shape: Sequence[int], dtype=torch.float32) -> torch.Tensor:
    n = 1
    for s in shape:
        n *= int(s)
    esz = torch.empty((), dtype=dtype).element_size()
    return ws[offset:offset + n * esz].view(dtype).view(*shape)


def pack_params(sd: Dict[str, torch.Tensor]) -> VsParams:
    """state_dict (reference key names) -> vs_params of raw device pointers."""
    p = VsParams()
    for l, (ci, bi) in enumerate(CONV_INDEX):
        names = {"weight": f"conv.{ci}.weight", "bias": f"conv.{ci}.bias",
                 "bn_weight": f"conv.{bi}.weight", "bn_bias": f"conv.{bi}.bias",
                 "bn_running_mean": f"conv.{bi}.running_mean", "bn_running_var": f"conv.{bi}.running_var"}
        for field, key in names.items():
            t = sd[key]
            _call.dev_check(t, key)
            setattr(p.conv[l], field, t.data_ptr())
    for d, suffix in enumerate(("", "_reverse")):
        for field, key in LSTM_FIELDS:
            t = sd[f"lstm.{key}{suffix}"]
            _call.dev_check(t, f"lstm.{key}{suffix}")
            getattr(p, field)[d] = t.data_ptr()
    for field, key in HEAD_FIELDS:
        _call.dev_check(sd[key], key)
        setattr(p, field, sd[key].data_ptr())
    return p


# ---------------------------------------------------------------------------------------------
# whole path and stages
# ---------------------------------------------------------------------------------------------

def _check_inputs(x, dvec, dims: VsDims):
    _call.dev_check(x, "x")
    _call.dev_check(dvec, "speaker_embedding")
    if x.dim() != 3 or x.shape[2] != dims.F:
        raise ValueError(f"x must be [B, T, num_freq={dims.F}] (F contiguous), got {tuple(x.shape)}")
    if dvec.dim() != 2 or dvec.shape[0] != x.shape[0] or dvec.shape[1] != dims.E:
        raise ValueError(f"speaker_embedding must be [B={x.shape[0]}, emb_dim={dims.E}], got {tuple(dvec.shape)}")


def forward(sd, x, dvec, dims: VsDims, conv_act: str, training: bool = False,
            workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mask = model(x, dvec): the whole reference forward in one C-ABI call."""
    _check_inputs(x, dvec, dims)
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_workspace(dims, x.device)
    mask = torch.empty(dims.B, dims.T, dims.FC2, dtype=torch.float32, device=x.device)
    _call.call("forward", x.device, ctypes.byref(dims), ctypes.byref(params), x, dvec, ACT_CODES[conv_act],
               BN_TRAIN if training else BN_EVAL, ws, ws.numel(), mask)
    return mask


class PreparedWeights:
    """What an eval-mode forward derives from the parameters alone (vs_prepare_weights), kept on the device
    together with the identity of the tensors it was derived from: ``matches(sd, dims)`` is False as soon as
    any parameter / BatchNorm buffer was replaced or modified in place (optimizer step, load_state_dict,
    ``.to()``), or the arithmetic changed.  The buffer is filled on the stream current at construction; ``forward_prepared`` and
    ``forward_prepared_multi`` make their own stream wait for that on the device (``_call.Built``), so the weights may be prepared
    under one stream and used under any other."""

    def __init__(self, sd, dims: VsDims):
        some = next(iter(sd.values()))
        self.buf = torch.empty(_call.sized("prepared_bytes", ctypes.byref(dims)), dtype=torch.uint8, device=some.device)
        self.key = self._key(sd, dims)
        params = pack_params(sd)
        _call.call("prepare_weights", some.device, ctypes.byref(dims), ctypes.byref(params), self.buf, self.buf.numel())
        self.built = _call.Built(some.device)

    @staticmethod
    def _key(sd, dims: VsDims):
        return (dims.F, dims.E, dims.H, dims.FC1, dims.FC2, dims.math,
                tuple((k, v.data_ptr(), v._version) for k, v in sorted(sd.items()) if not k.endswith("num_batches_tracked")))

    def matches(self, sd, dims: VsDims) -> bool:
        return self.key == self._key(sd, dims)


def device_lengths(lengths, B: int, T: int, device) -> torch.Tensor:
    """lengths (sequence or tensor, any device) -> int32 [B] on ``device`` after the range check the library leaves to its
    caller: every item has 1 <= length <= T.  (Reads the values on the host: a tensor on the device is synchronised.)"""
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(host) != B:
        raise ValueError(f"lengths: {len(host)} values for a batch of {B}")
    bad = [(i, v) for i, v in enumerate(host) if v < 1 or v > T]
    if bad:
        raise ValueError(f"lengths: every item needs 1 <= length <= T = {T}; got " + ", ".join(f"lengths[{i}] = {v}" for i, v in bad[:4]))
    return torch.tensor(host, dtype=torch.int32, device=device)


def forward_prepared(sd, prepared: PreparedWeights, x, dvec, dims: VsDims, conv_act: str,
                     workspace: Optional[torch.Tensor] = None, lengths=None) -> torch.Tensor:
    """Eval-mode mask = model(x, dvec) with the weight-only work read from ``prepared``; bit-identical to
    ``forward(..., training=False)``.  lengths (one per item, 1..T): the padded batch x holds clips of unequal length and
    every item is computed as if alone (vs_forward_prepared_ragged); mask rows past an item's length are 0."""
    _check_inputs(x, dvec, dims)
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_workspace(dims, x.device)
    mask = torch.empty(dims.B, dims.T, dims.FC2, dtype=torch.float32, device=x.device)
    prepared.built.wait()
    lead = (ctypes.byref(dims), ctypes.byref(params), prepared.buf, prepared.buf.numel(), x, dvec)
    if lengths is not None:
        lens = device_lengths(lengths, dims.B, dims.T, x.device)
        _call.call("forward_prepared_ragged", x.device, *lead, lens, ACT_CODES[conv_act], ws, ws.numel(), mask)
        return mask
    _call.call("forward_prepared", x.device, *lead, ACT_CODES[conv_act], ws, ws.numel(), mask)
    return mask


def _check_multi_inputs(x, dvecs, dims: VsDims):
    _call.dev_check(x, "x")
    _call.dev_check(dvecs, "speaker_embeddings")
    if x.dim() != 3 or x.shape[2] != dims.F:
        raise ValueError(f"x must be [B, T, num_freq={dims.F}] (F contiguous), got {tuple(x.shape)}")
    _check_multi_dvecs(dvecs, x.shape[0], dims)


def _check_multi_dvecs(dvecs, B: int, dims: VsDims):
    if dvecs.dim() != 3 or dvecs.shape[0] != B or dvecs.shape[1] < 1 or dvecs.shape[2] != dims.E:
        raise ValueError(f"speaker_embeddings must be [B={B}, K >= 1, emb_dim={dims.E}], got {tuple(dvecs.shape)}")


def forward_prepared_multi(sd, prepared: PreparedWeights, x, dvecs, dims: VsDims, conv_act: str,
                           workspace: Optional[torch.Tensor] = None, lengths=None) -> torch.Tensor:
    """Eval-mode masks [B, K, T, FC2] of K enrolled speakers per mixture (dvecs [B, K, E]) with one conv pass and one LSTM input
    GEMM (vs_forward_prepared_multi); lengths as in ``forward_prepared``, one per mixture."""
    _check_multi_inputs(x, dvecs, dims)
    K = int(dvecs.shape[1])
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_multi_workspace(dims, K, x.device)
    lens = device_lengths(lengths, dims.B, dims.T, x.device) if lengths is not None else None
    mask = torch.empty(dims.B, K, dims.T, dims.FC2, dtype=torch.float32, device=x.device)
    prepared.built.wait()
    _call.call("forward_prepared_multi", x.device, ctypes.byref(dims), ctypes.byref(params), prepared.buf, prepared.buf.numel(),
               x, dvecs, K, lens, ACT_CODES[conv_act], ws, ws.numel(), mask)
    return mask


def bilstm_multi(sd, feat, dvecs, dims: VsDims, lengths=None, workspace=None) -> torch.Tensor:
    """feat [B, T, 8F], dvecs [B, K, E] -> LSTM output [B, K, T, 2H]: one input GEMM per mixture, the shared-input recurrence over
    the B*K sequences (vs_bilstm_fwd_multi).  lengths (one per mixture): rows t >= lengths[b] are 0 for every k."""
    _call.dev_check(feat, "feat")
    _call.dev_check(dvecs, "speaker_embeddings")
    _check_multi_dvecs(dvecs, feat.shape[0], dims)
    K = int(dvecs.shape[1])
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_multi_workspace(dims, K, feat.device)
    lens = device_lengths(lengths, dims.B, dims.T, feat.device) if lengths is not None else None
    out = torch.empty(dims.B, K, dims.T, 2 * dims.H, dtype=torch.float32, device=feat.device)
    _call.call("bilstm_fwd_multi", feat.device, ctypes.byref(dims), ctypes.byref(params), feat, dvecs, K, lens, ws, ws.numel(), out)
    return out


def conv_stack(sd, x, dims: VsDims, conv_act: str, training: bool = False, workspace=None, lengths=None) -> torch.Tensor:
    """lengths (eval mode): a padded batch, rows t < lengths[b] as of the item alone (rows behind: finite, unspecified)."""
    _call.dev_check(x, "x")
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_workspace(dims, x.device)
    feat = torch.empty(dims.B, dims.T, 8 * dims.F, dtype=torch.float32, device=x.device)
    lead = (ctypes.byref(dims), ctypes.byref(params), x)
    tail = (ws, ws.numel(), feat)
    if lengths is not None:
        if training:
            raise ValueError("conv_stack: per-item lengths are an eval-mode form")
        lens = device_lengths(lengths, dims.B, dims.T, x.device)
        _call.call("conv_stack_fwd_ragged", x.device, *lead, lens, ACT_CODES[conv_act], *tail)
        return feat
    _call.call("conv_stack_fwd", x.device, *lead, ACT_CODES[conv_act], BN_TRAIN if training else BN_EVAL, *tail)
    return feat


def bilstm(sd, feat, dvec, dims: VsDims, workspace=None, lengths=None) -> torch.Tensor:
    """lengths: a padded batch, a zero state at each item's own first and last frame; rows t >= lengths[b] are 0."""
    _call.dev_check(feat, "feat")
    _call.dev_check(dvec, "speaker_embedding")
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_workspace(dims, feat.device)
    out = torch.empty(dims.B, dims.T, 2 * dims.H, dtype=torch.float32, device=feat.device)
    lead = (ctypes.byref(dims), ctypes.byref(params), feat, dvec)
    tail = (ws, ws.numel(), out)
    if lengths is not None:
        lens = device_lengths(lengths, dims.B, dims.T, feat.device)
        _call.call("bilstm_fwd_ragged", feat.device, *lead, lens, *tail)
        return out
    _call.call("bilstm_fwd", feat.device, *lead, *tail)
    return out


def _check_carry_state(state, B: int, H: int, device):
    if state is None:
        return None
    _call.dev_check(state, "state")
    if tuple(state.shape) != (B, 2, H) or state.device != device:
        raise ValueError(f"state must be [B, 2, H] = [{B}, 2, {H}] (h, then c) on {device}, got {tuple(state.shape)} on {state.device}")
    if state.data_ptr() % 16:
        raise ValueError("state must be 16-byte aligned (the kernels read it in float4 units)")
    return state


def bilstm_carry(sd, feat, dvec, dims: VsDims, state=None, keep: Optional[int] = None, workspace=None):
    """The sequence stage over one chunk of a stream (vs_bilstm_fwd_carry): feat [B, T, 8F] = [chunk | look-ahead], the forward
    direction continues from ``state`` [B, 2, H] (h, then c; None: zero, the stream's first chunk), the reverse direction starts
    from zero at frame T - 1.  Returns (lstm_out [B, T, 2H], state behind frame keep - 1 [B, 2, H]); keep defaults to T."""
    _call.dev_check(feat, "feat")
    _call.dev_check(dvec, "speaker_embedding")
    keep = dims.T if keep is None else int(keep)
    state = _check_carry_state(state, dims.B, dims.H, feat.device)
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_workspace(dims, feat.device)
    out = torch.empty(dims.B, dims.T, 2 * dims.H, dtype=torch.float32, device=feat.device)
    state_out = torch.empty(dims.B, 2, dims.H, dtype=torch.float32, device=feat.device)
    _call.call("bilstm_fwd_carry", feat.device, ctypes.byref(dims), ctypes.byref(params), feat, dvec, state, state_out, keep,
               ws, ws.numel(), out)
    return out, state_out


def bilstm_carry_multi(sd, feat, dvecs, dims: VsDims, state=None, keep: Optional[int] = None, workspace=None):
    """``bilstm_carry`` for K enrolled speakers per stream (vs_bilstm_fwd_carry_multi): feat [B, T, 8F] (once per mixture), dvecs
    [B, K, E]; one input GEMM per mixture, the carry x shared-input recurrence over the B*K sequences n = b*K + k, each continuing
    from its own row of ``state`` [B*K, 2, H] (h, then c; None: zero).  Returns (lstm_out [B, K, T, 2H], state behind frame
    keep - 1 [B*K, 2, H]); keep defaults to T."""
    _call.dev_check(feat, "feat")
    _call.dev_check(dvecs, "speaker_embeddings")
    _check_multi_dvecs(dvecs, feat.shape[0], dims)
    K = int(dvecs.shape[1])
    keep = dims.T if keep is None else int(keep)
    state = _check_carry_state(state, dims.B * K, dims.H, feat.device)
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_multi_workspace(dims, K, feat.device)
    out = torch.empty(dims.B, K, dims.T, 2 * dims.H, dtype=torch.float32, device=feat.device)
    state_out = torch.empty(dims.B * K, 2, dims.H, dtype=torch.float32, device=feat.device)
    _call.call("bilstm_fwd_carry_multi", feat.device, ctypes.byref(dims), ctypes.byref(params), feat, dvecs, K, state, state_out, keep,
               ws, ws.numel(), out)
    return out, state_out


def zero_tail_rows(t: torch.Tensor, lengths) -> torch.Tensor:
    """In place: rows t[b, lengths[b]:] := 0 of a contiguous [B, T, ...] tensor (vs_zero_tail_rows; unit-test surface)."""
    _call.dev_check(t, "t", t.dtype)
    B, T = t.shape[0], t.shape[1]
    row_bytes = (t[0, 0].numel() if t.dim() > 2 else 1) * t.element_size()
    lens = device_lengths(lengths, B, T, t.device)
    _call.call("zero_tail_rows", t.device, t, B, T, row_bytes, lens)
    return t


def head(sd, lstm_out, dims: VsDims, want_logits: bool = False, workspace=None):
    _call.dev_check(lstm_out, "lstm_out")
    params = pack_params(sd)
    ws = workspace if workspace is not None else get_workspace(dims, lstm_out.device)
    mask = torch.empty(dims.B, dims.T, dims.FC2, dtype=torch.float32, device=lstm_out.device)
    logits = torch.empty_like(mask) if want_logits else None
    _call.call("head_fwd", lstm_out.device, ctypes.byref(dims), ctypes.byref(params), lstm_out, ws, ws.numel(), logits, mask)
    return (mask, logits) if want_logits else mask


# ---------------------------------------------------------------------------------------------
# kernel-level wrappers (unit tests)
# ---------------------------------------------------------------------------------------------

def bn_fold(gamma, beta, mean, var, conv_bias, eps=1e-5):
    C = gamma.numel()
    scale, shift = torch.empty_like(gamma), torch.empty_like(gamma)
    _call.call("bn_fold", gamma.device, gamma, beta, mean, var, conv_bias, eps, C, scale, shift)
    return scale, shift


def conv_first(x, w, scale, shift, act: str):
    for n, t in (("x", x), ("w", w), ("scale", scale), ("shift", shift)):
        _call.dev_check(t, n)
    B, T, F = x.shape
    out = torch.empty(B, 64, T, F, dtype=torch.float32, device=x.device)
    _call.call("conv_first_fwd", x.device, x, w, scale, shift, out, B, T, F, ACT_CODES[act])
    return out


def _conv64_f16x3(x, w, scale, shift, dil: int, act_code: int, transpose_flip: int):
    B, C, T, F = x.shape
    KT, KF = w.shape[2], w.shape[3]
    packed = torch.empty(_lib.load().vs_conv64_packed_f16_floats(KT, KF), dtype=torch.float32, device=x.device)
    scales = torch.zeros(8, dtype=torch.float32, device=x.device)
    amax = scales[4:].view(torch.int32)
    _call.call("pow2_scale", x.device, x, x.numel(), amax, scales)
    _call.call("conv64_pack_f16", x.device, w, packed, KT, KF, transpose_flip, amax[1:], scales[2:])
    out = torch.empty_like(x)
    _call.call("conv64_f16x3_fwd", x.device, x, packed, scale, shift, scales, scales[2:], out, B, T, F, KT, KF, dil, act_code)
    return out


def conv64(x, w, scale, shift, dil: int, act: str, math: str = "fp32"):
    """x [B,64,T,F], w [64,64,KT,KF] -> [B,64,T,F] with 'same' zero padding and time dilation."""
    for n, t in (("x", x), ("w", w), ("scale", scale), ("shift", shift)):
        _call.dev_check(t, n)
    if math == "f16x3":
        return _conv64_f16x3(x, w, scale, shift, dil, ACT_CODES[act], 0)
    B, C, T, F = x.shape
    KT, KF = w.shape[2], w.shape[3]
    packed = torch.empty(_lib.load().vs_conv64_packed_floats(KT, KF), dtype=torch.float32, device=x.device)
    _call.call("conv64_pack", x.device, w, packed, KT, KF)
    out = torch.empty_like(x)
    _call.call("conv64_fwd", x.device, x, packed, scale, shift, out, B, T, F, KT, KF, dil, ACT_CODES[act])
    return out


def conv_last(x, w, scale, shift, act: str):
    for n, t in (("x", x), ("w", w), ("scale", scale), ("shift", shift)):
        _call.dev_check(t, n)
    B, C, T, F = x.shape
    out = torch.empty(B, T, 8 * F, dtype=torch.float32, device=x.device)
    _call.call("conv_last_fwd", x.device, x, w, scale, shift, out, B, T, F, ACT_CODES[act])
    return out


def gemm_nt(A, W, bias1=None, bias2=None, rowbias=None, group: int = 1, a_relu: bool = False, act: str = "none",
            K: Optional[int] = None):
    """act(opA(A)[:, :K] @ W[:, :K]^T + biases); A [M,lda], W [N,ldw] row-major."""
    _call.dev_check(A, "A")
    _call.dev_check(W, "W")
    M, lda = A.shape
    N, ldw = W.shape
    K = K if K is not None else min(lda, ldw)
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    ldrb = rowbias.shape[1] if rowbias is not None else 0
    _call.call("gemm_nt", A.device, A, lda, W, ldw, C, N, M, N, K, bias1, bias2, rowbias, ldrb, group, int(a_relu), ACT_CODES[act])
    return C


def bilstm_recurrent(xg, w_hh_f, w_hh_b, math=None):
    """xg [B,T,8H] (bias already added) -> [B,T,2H].  math: None = the fp32-MFMA entry points, else MATH_* through the
    *_math entry points (the recurrent products on the f16 matrix instructions)."""
    lib = _lib.load()
    for n, t in (("xg", xg), ("w_hh_f", w_hh_f), ("w_hh_b", w_hh_b)):
        _call.dev_check(t, n)
    B, T, H8 = xg.shape
    H = H8 // 8
    packed = torch.empty(lib.vs_lstm_packed_floats(H), dtype=torch.float32, device=xg.device)
    state = torch.empty(lib.vs_lstm_state_floats(B, H), dtype=torch.float32, device=xg.device)
    out = torch.empty(B, T, 2 * H, dtype=torch.float32, device=xg.device)
    if math is None:
        _call.call("lstm_pack", xg.device, w_hh_f, w_hh_b, packed, H)
        _call.call("bilstm_recurrent", xg.device, xg, packed, state, out, B, T, H)
    else:
        _call.call("lstm_pack_math", xg.device, w_hh_f, w_hh_b, packed, H, int(math))
        _call.call("bilstm_recurrent_math", xg.device, xg, packed, state, out, None, None, B, T, H, int(math))
    _lstm_check_err(state, state.numel() - 64, "vs_bilstm_recurrent")
    return out


def bilstm_recurrent_carry(xg, w_hh_f, w_hh_b, math, state=None, keep: Optional[int] = None):
    """The raw carry recurrence (vs_bilstm_recurrent_carry): xg [B,T,8H] (bias already added), the forward direction from ``state``
    [B,2,H] (h, then c; None: zero) -> (out [B,T,2H], state behind frame keep - 1 [B,2,H]); keep defaults to T.  math: MATH_F16X3 or
    MATH_BF16 (code or name); everything else is refused by the library."""
    lib = _lib.load()
    for n, t in (("xg", xg), ("w_hh_f", w_hh_f), ("w_hh_b", w_hh_b)):
        _call.dev_check(t, n)
    math = MATH_CODES[math] if isinstance(math, str) else int(math)
    B, T, H8 = xg.shape
    H = H8 // 8
    keep = T if keep is None else int(keep)
    state_in = _check_carry_state(state, B, H, xg.device)
    packed = torch.empty(lib.vs_lstm_packed_floats(H), dtype=torch.float32, device=xg.device)
    scratch = torch.empty(lib.vs_lstm_state_floats(B, H), dtype=torch.float32, device=xg.device)
    out = torch.empty(B, T, 2 * H, dtype=torch.float32, device=xg.device)
    state_out = torch.empty(B, 2, H, dtype=torch.float32, device=xg.device)
    _call.call("lstm_pack_math", xg.device, w_hh_f, w_hh_b, packed, H, math)
    _call.call("bilstm_recurrent_carry", xg.device, xg, packed, scratch, out, state_in, state_out, keep, B, T, H, math)
    _lstm_check_err(scratch, scratch.numel() - 64, "vs_bilstm_recurrent_carry")
    return out, state_out


def bilstm_recurrent_carry_shared(xg, rowbias, K: int, w_hh_f, w_hh_b, math, state=None, keep: Optional[int] = None, state_out=None):
    """The raw carry x shared-input recurrence (vs_bilstm_recurrent_carry_shared): xg [M,T,8H] WITHOUT row bias, rowbias [N,8H] with
    N = M*K; sequence n = m*K + k reads xg[m], adds rowbias[n] and continues from ``state`` [N,2,H] (h, then c; None: zero) ->
    (out [N,T,2H], state behind frame keep - 1 [N,2,H]); keep defaults to T.  state_out: the buffer to hand the state to (it may
    be ``state`` itself), else a new one."""
    lib = _lib.load()
    for n, t in (("xg", xg), ("rowbias", rowbias), ("w_hh_f", w_hh_f), ("w_hh_b", w_hh_b)):
        _call.dev_check(t, n)
    math = MATH_CODES[math] if isinstance(math, str) else int(math)
    M, T, H8 = xg.shape
    H = H8 // 8
    N = int(rowbias.shape[0])
    if rowbias.dim() != 2 or rowbias.shape[1] != H8:
        raise ValueError(f"rowbias must be [N, 8H = {H8}], got {tuple(rowbias.shape)}")
    if int(K) >= 1 and N != M * int(K):
        raise ValueError(f"rowbias has {N} rows, xg has M = {M} rows shared by K = {K} sequences each")
    keep = T if keep is None else int(keep)
    state_in = _check_carry_state(state, N, H, xg.device)
    packed = torch.empty(lib.vs_lstm_packed_floats(H), dtype=torch.float32, device=xg.device)
    scratch = torch.empty(lib.vs_lstm_state_floats(N, H), dtype=torch.float32, device=xg.device)
    out = torch.empty(N, T, 2 * H, dtype=torch.float32, device=xg.device)
    state_out = _check_carry_state(state_out, N, H, xg.device) if state_out is not None else \
        torch.empty(N, 2, H, dtype=torch.float32, device=xg.device)
    _call.call("lstm_pack_math", xg.device, w_hh_f, w_hh_b, packed, H, math)
    _call.call("bilstm_recurrent_carry_shared", xg.device, xg, rowbias, int(K), packed, scratch, out, state_in, state_out,
               keep, N, T, H, math)
    _lstm_check_err(scratch, scratch.numel() - 64, "vs_bilstm_recurrent_carry_shared")
    return out, state_out


def _lstm_check_err(state: torch.Tensor, word: int, what: str):
    """The persistent recurrences report a spin that gave up (a workgroup of the launch was not
    resident) through a word in the state buffer; the step kernels leave it 0.  Unit-test helper:
    synchronises."""
    if int(state.view(torch.int32)[word].item()) != 0:
        raise _lib.VoiceSplitHipError(f"{what}: the persistent LSTM kernel gave up waiting for a peer workgroup")


# ---------------------------------------------------------------------------------------------
# training: forward with tape, backward (train.py:94-110 through models/voicesplit/model.py:66-89)
# ---------------------------------------------------------------------------------------------

# vs_grads field <- state_dict key, in the order model.parameters() yields them is NOT assumed:
# gradients are returned as a dict keyed like the state_dict.
def tape_layout(dims: VsDims) -> "_lib.VsTapeLayout":
    lay = _lib.VsTapeLayout()
    check(_lib.load().vs_tape_layout_query(ctypes.byref(dims), ctypes.byref(lay)), "vs_tape_layout_query")
    return lay


_TAPE_POOL: Dict[int, list] = {}       # device index -> free tapes
_TAPE_POOL_MAX = int(os.environ.get("VOICESPLIT_TAPE_POOL", "1"))


def new_tape(dims: VsDims, device) -> torch.Tensor:
    """Caller-owned training tape (saved activations + backward scratch, 49 GB at B=64).  Tapes
    are recycled through a small per-device pool: a forward takes one, its backward hands it back
    (``recycle_tape``), so steady-state training touches no allocator at all.  Any free tape with
    enough capacity is reused (variable B / T: the largest shape seen so far serves the smaller
    ones); at most ``VOICESPLIT_TAPE_POOL`` (default 1) free tapes are retained per device, and
    free tapes that are too small are released before a larger one is allocated."""
    nbytes = _call.sized("tape_bytes", ctypes.byref(dims))
    free = _TAPE_POOL.setdefault(torch.device(device).index, [])
    fit = [t for t in free if t.numel() >= nbytes]
    if fit:
        t = min(fit, key=lambda u: u.numel())
        free.remove(t)
        return t
    free.clear()                                              # too small: let go before the big allocation
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def recycle_tape(tape: torch.Tensor):
    pool = _TAPE_POOL.setdefault(tape.device.index, [])
    if len(pool) < _TAPE_POOL_MAX:
        pool.append(tape)


def tape_pool_bytes(device=None) -> int:
    """Bytes held by free tapes (outside torch's caching allocator statistics of live tensors)."""
    idx = None if device is None else torch.device(device).index
    return sum(t.numel() for k, v in _TAPE_POOL.items() if idx is None or k == idx for t in v)


def forward_train(sd, x, dvec, dims: VsDims, conv_act: str, training: bool, tape: torch.Tensor) -> torch.Tensor:
    _check_inputs(x, dvec, dims)
    params = pack_params(sd)
    mask = torch.empty(dims.B, dims.T, dims.FC2, dtype=torch.float32, device=x.device)
    _call.call("forward_train", x.device, ctypes.byref(dims), ctypes.byref(params), x, dvec, ACT_CODES[conv_act],
               BN_TRAIN if training else BN_EVAL, tape, tape.numel(), mask)
    return mask


GRAD_KEYS_CONV = (("weight", "weight"), ("bias", "bias"))
GRAD_KEYS_BN = (("bn_weight", "weight"), ("bn_bias", "bias"))


def backward(sd, x, dvec, dims: VsDims, conv_act: str, training: bool, tape: torch.Tensor, mask, dmask,
             want_dvec: bool = False, sink: Optional[Dict[str, torch.Tensor]] = None,
             leaves_event: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """d(loss)/d(parameters) for dmask = d(loss)/d(mask); returns {state_dict key: gradient}
    (+ 'speaker_embedding' when want_dvec).  sink: {key: preallocated tensor} the library writes those gradients into
    (overwriting, vs_backward never accumulates) instead of fresh tensors -- the trainer's flat all-reduce bucket.
    leaves_event: raw hipEvent_t handle (``torch.cuda.Event.cuda_event``) the library records when the head's and the BiLSTM's
    gradients are final (vs_grads.leaves_event, ABI 9)."""
    _call.dev_check(dmask, "grad_mask")
    _call.dev_check(mask, "mask")
    params = pack_params(sd)
    grads = _lib.VsGrads()
    out: Dict[str, torch.Tensor] = {}

    def alloc(key):
        t = sink.get(key) if sink else None
        if t is None:
            t = torch.empty_like(sd[key])
        elif (t.shape != sd[key].shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != sd[key].device):
            raise ValueError(f"gradient sink for {key}: expected a contiguous float32 {tuple(sd[key].shape)} tensor on {sd[key].device}")
        out[key] = t
        return t.data_ptr()

    for l, (ci, bi) in enumerate(CONV_INDEX):
        for field, name in GRAD_KEYS_CONV:
            setattr(grads.conv[l], field, alloc(f"conv.{ci}.{name}"))
        for field, name in GRAD_KEYS_BN:
            setattr(grads.conv[l], field, alloc(f"conv.{bi}.{name}"))
    for d, suffix in enumerate(("", "_reverse")):
        for field, key in LSTM_FIELDS:
            getattr(grads, field)[d] = alloc(f"lstm.{key}{suffix}")
    for field, key in HEAD_FIELDS:
        setattr(grads, field, alloc(key))
    if want_dvec:
        out["speaker_embedding"] = torch.empty_like(dvec)
        grads.dvec = out["speaker_embedding"].data_ptr()
    if leaves_event:
        grads.leaves_event = int(leaves_event)
    _call.call("backward", x.device, ctypes.byref(dims), ctypes.byref(params), x, dvec, ACT_CODES[conv_act],
               BN_TRAIN if training else BN_EVAL, tape, tape.numel(), mask, dmask, ctypes.byref(grads))
    return out


# ---- backward kernels (unit tests) -------------------------------------------------------------

def conv64_dgrad(dz, w, dil: int, math: str = "fp32"):
    """dIn [B,64,T,F] = conv^T(dz, w): the forward kernel with transposed + tap-flipped weights."""
    _call.dev_check(dz, "dz")
    _call.dev_check(w, "w")
    if math == "f16x3":
        ones, zeros = torch.ones(64, device=dz.device), torch.zeros(64, device=dz.device)
        return _conv64_f16x3(dz, w, ones, zeros, dil, ACT_NONE, 1)
    B, C, T, F = dz.shape
    KT, KF = w.shape[2], w.shape[3]
    packed = torch.empty(_lib.load().vs_conv64_packed_floats(KT, KF), dtype=torch.float32, device=dz.device)
    _call.call("conv64_pack_dgrad", dz.device, w, packed, KT, KF)
    ones, zeros = torch.ones(64, device=dz.device), torch.zeros(64, device=dz.device)
    out = torch.empty_like(dz)
    _call.call("conv64_fwd", dz.device, dz, packed, ones, zeros, out, B, T, F, KT, KF, dil, ACT_NONE, what="vs_conv64_fwd(dgrad)")
    return out


def conv64_wgrad(dz, x, KT: int, KF: int, dil: int, math: str = "fp32"):
    _call.dev_check(dz, "dz")
    _call.dev_check(x, "x")
    B, C, T, F = dz.shape
    part = torch.empty(_lib.load().vs_conv64_wgrad_partial_floats(KT, KF), dtype=torch.float32, device=dz.device)
    dw = torch.empty(64, 64, KT, KF, dtype=torch.float32, device=dz.device)
    if math == "f16x3":
        scratch = torch.zeros(8, dtype=torch.float32, device=dz.device)
        _call.call("conv64_wgrad_f16x3", dz.device, dz, x, part, dw, scratch, B, T, F, KT, KF, dil)
        return dw
    _call.call("conv64_wgrad", dz.device, dz, x, part, dw, B, T, F, KT, KF, dil)
    return dw


def bn_act_bwd(da, z, C: int, act: str, training: bool, scale, shift, mean, invstd):
    """rows [R][L] view of da/z (channel = r % C) -> dz, dgamma, dbeta, dbias."""
    for n, t in (("da", da), ("z", z), ("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd)):
        _call.dev_check(t, n)
    L = da.shape[-1]
    R = da.numel() // L
    dev = da.device
    dz = torch.empty_like(da)
    dgamma, dbeta, dbias = (torch.empty(C, device=dev) for _ in range(3))
    stats = torch.empty(2 * C, dtype=torch.float64, device=dev)
    coef = torch.empty(3 * C, device=dev)
    _call.call("bn_act_bwd", dev, da, z, dz, C, R, L, ACT_CODES[act], BN_TRAIN if training else BN_EVAL,
               scale, shift, mean, invstd, dgamma, dbeta, dbias, stats, coef)
    return dz, dgamma, dbeta, dbias


def bn_act_bwd_first(da, z, x, act: str, training: bool, scale, shift, mean, invstd):
    """cnn1: da, z [B,64,T,F] and the input x [B,T,F] -> dgamma, dbeta, dbias, dw [64,1,1,7]
    (BatchNorm+activation backward fused with the 1x7 weight gradient; dZ1 is not materialised)."""
    for n, t in (("da", da), ("z", z), ("x", x), ("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd)):
        _call.dev_check(t, n)
    B, C, T, F = da.shape
    if C != 64 or tuple(x.shape) != (B, T, F) or z.shape != da.shape:
        raise ValueError(f"bn_act_bwd_first: da {tuple(da.shape)}, z {tuple(z.shape)}, x {tuple(x.shape)}")
    dev = da.device
    dgamma, dbeta, dbias = (torch.empty(64, device=dev) for _ in range(3))
    dw = torch.empty(64, 1, 1, 7, device=dev)
    xpad = torch.empty(B * T * (F + 6), device=dev)
    stats = torch.empty(128, dtype=torch.float64, device=dev)
    acc = torch.empty(448, dtype=torch.float64, device=dev)
    coef = torch.empty(192, device=dev)
    _call.call("bn_act_bwd_first", dev, da, z, x, xpad, B, T, F, ACT_CODES[act], BN_TRAIN if training else BN_EVAL,
               scale, shift, mean, invstd, dgamma, dbeta, dbias, dw, stats, coef, acc)
    return dgamma, dbeta, dbias, dw


def conv_last_dgrad(dz8, w, B, T, F):
    _call.dev_check(dz8, "dz8")
    _call.dev_check(w, "w")
    out = torch.empty(B, 64, T, F, dtype=torch.float32, device=dz8.device)
    _call.call("conv_last_dgrad", dz8.device, dz8, w, out, B, T, F)
    return out


def conv_last_wgrad(dz8, a7):
    _call.dev_check(dz8, "dz8")
    _call.dev_check(a7, "a7")
    B, C, T, F = a7.shape
    part = torch.empty(_lib.load().vs_conv_last_wgrad_blocks() * 512, dtype=torch.float32, device=a7.device)
    dw = torch.empty(8, 64, 1, 1, dtype=torch.float32, device=a7.device)
    _call.call("conv_last_wgrad", dz8.device, dz8, a7, part, dw, B, T, F)
    return dw


def conv_first_wgrad(dz1, x):
    _call.dev_check(dz1, "dz1")
    _call.dev_check(x, "x")
    B, T, F = x.shape
    acc = torch.empty(448, dtype=torch.float64, device=x.device)
    dw = torch.empty(64, 1, 1, 7, dtype=torch.float32, device=x.device)
    _call.call("conv_first_wgrad", dz1.device, dz1, x, acc, dw, B, T, F)
    return dw


def gemm(A, W, M: int, N: int, K: int, layout_a: int = 0, layout_w: int = 0, bias=None, gate=None,
         a_relu=False, w_relu=False, act="none", out=None, accumulate=False, w_shift=0, w_group=0, splits=1,
         math: str = "fp32"):
    """General GEMM (see vs_gemm in the header); A/W are 2-D row-major views with their own ld."""
    _call.dev_check(A, "A")
    _call.dev_check(W, "W")
    C = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=A.device)
    lead = (layout_a, layout_w, A, A.shape[1], W, W.shape[1], C, C.shape[1], M, N, K, bias, gate,
            gate.shape[1] if gate is not None else 0, int(a_relu), int(w_relu), ACT_CODES[act], int(accumulate))
    if math == "f16x3":
        scratch = torch.zeros(8, dtype=torch.float32, device=A.device)
        _call.call("gemm_f16x3", A.device, *lead, scratch)
        return C
    part = torch.empty(splits * M * N, dtype=torch.float32, device=A.device) if splits > 1 else None
    _call.call("gemm", A.device, *lead, w_shift, w_group, splits, part)
    return C


def bilstm_recurrent_train(xg, w_hh_f, w_hh_b, math=None):
    """xg [B,T,8H] -> (out [B,T,2H], gates [B,T,8H] activated, c [B,T,2H]).  math: see bilstm_recurrent."""
    lib = _lib.load()
    for n, t in (("xg", xg), ("w_hh_f", w_hh_f), ("w_hh_b", w_hh_b)):
        _call.dev_check(t, n)
    B, T, H8 = xg.shape
    H = H8 // 8
    packed = torch.empty(lib.vs_lstm_packed_floats(H), dtype=torch.float32, device=xg.device)
    state = torch.empty(lib.vs_lstm_state_floats(B, H), dtype=torch.float32, device=xg.device)
    out = torch.empty(B, T, 2 * H, dtype=torch.float32, device=xg.device)
    gates = xg.clone()
    c = torch.empty(B, T, 2 * H, dtype=torch.float32, device=xg.device)
    if math is None:
        _call.call("lstm_pack", xg.device, w_hh_f, w_hh_b, packed, H)
        _call.call("bilstm_recurrent_train", xg.device, gates, packed, state, out, gates, c, B, T, H)
    else:
        _call.call("lstm_pack_math", xg.device, w_hh_f, w_hh_b, packed, H, int(math))
        _call.call("bilstm_recurrent_math", xg.device, gates, packed, state, out, gates, c, B, T, H, int(math))
    _lstm_check_err(state, state.numel() - 64, "vs_bilstm_recurrent_train")
    return out, gates, c


def bilstm_recurrent_bwd(gates, c, dout, w_hh_f, w_hh_b, math=None):
    """BPTT: returns d(loss)/d(xg) [B,T,8H] (gates is not modified: works on a copy).  math: see bilstm_recurrent."""
    lib = _lib.load()
    for n, t in (("gates", gates), ("c", c), ("dout", dout), ("w_hh_f", w_hh_f), ("w_hh_b", w_hh_b)):
        _call.dev_check(t, n)
    B, T, H8 = gates.shape
    H = H8 // 8
    packed_t = torch.empty(lib.vs_lstm_packed_t_floats(H), dtype=torch.float32, device=gates.device)
    state = torch.empty(lib.vs_lstm_bwd_state_floats(B, H), dtype=torch.float32, device=gates.device)
    dxg = gates.clone()
    if math is None:
        _call.call("lstm_pack_t", gates.device, w_hh_f, w_hh_b, packed_t, H)
        _call.call("bilstm_recurrent_bwd", gates.device, packed_t, state, dxg, c, dout, B, T, H)
    else:
        _call.call("lstm_pack_t_math", gates.device, w_hh_f, w_hh_b, packed_t, H, int(math))
        _call.call("bilstm_recurrent_bwd_math", gates.device, packed_t, state, dxg, c, dout, B, T, H, int(math))
    _lstm_check_err(state, state.numel() - 64, "vs_bilstm_recurrent_bwd")
    return dxg


def sigmoid_bwd(dmask, mask):
    _call.dev_check(dmask, "dmask")
    _call.dev_check(mask, "mask")
    out = torch.empty_like(mask)
    _call.call("sigmoid_bwd", dmask.device, dmask, mask, out, mask.numel())
    return out


def colsum(x, groups: int, rows: int):
    _call.dev_check(x, "x")
    N = x.shape[-1]
    out = torch.empty(groups, N, dtype=torch.float32, device=x.device)
    _call.call("colsum", x.device, x, N, groups, rows, N, out, N)
    return out


# ---------------------------------------------------------------------------------------------
# channels-last bf16 kernels of the VS_MATH_BF16 path (csrc/conv_nhwc.hip); unit-test surface
# ---------------------------------------------------------------------------------------------
def nhwc_conv(x, w, scale, shift, dil: int, act: str, transpose_flip: bool = False, stats=False):
    """x [B,T,F,64] bf16 (channels last), w [64,64,KT,KF] fp32 -> act(conv(x) * scale + shift) as [B,T,F,64] bf16,
    'same' zero padding, time dilation `dil`.  stats: also return the per-channel {sum, sum of squares} of the
    outputs, [64, 2] float64 (train-mode BatchNorm statistics; act must be "none"); stats="raw": the 64 partial slots
    [64 slots, 64, 2] as the kernel left them (what vs_bn_finalize takes)."""
    _call.dev_check(x, "x", torch.bfloat16)
    for n, t in (("w", w), ("scale", scale), ("shift", shift)):
        _call.dev_check(t, n)
    B, T, F, C = x.shape
    if C != 64:
        raise ValueError("nhwc_conv: 64 channels expected")
    KT, KF = w.shape[2], w.shape[3]
    packed = nhwc_conv_pack(w, transpose_flip)
    out = torch.empty_like(x)
    st = torch.zeros(64, 64, 2, dtype=torch.float64, device=x.device) if stats else None
    _call.call("nhwc_conv", x.device, x, packed, scale, shift, out, B, T, F, KT, KF, dil, ACT_CODES[act], st)
    if stats == "raw":
        return out, st
    return (out, st.sum(0)) if stats else out


def f16x3_split(x, scale: float):
    """fp32 tensor -> (hi, lo) f16 planes of x * scale (scale a power of two) and the device scale pair {s, 1/s}."""
    _call.dev_check(x, "x")
    s2 = torch.tensor([scale, 1.0 / scale], dtype=torch.float32, device=x.device)
    hi = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    lo = torch.empty_like(hi)
    _call.call("f16x3_split", x.device, x, s2, hi, lo, x.numel())
    return hi, lo, s2


def f16x3_merge(hi, lo, scale2):
    x = torch.empty(hi.shape, dtype=torch.float32, device=hi.device)
    _call.call("f16x3_merge", hi.device, hi, lo, scale2, x, x.numel())
    return x


def nhwc_conv_f16x3(hi, lo, scale2, w, bn_scale, bn_shift, dil: int, act: str, amax_in=None, scratch=None):
    """One 64 -> 64 layer in the split-f16 arithmetic on channels-last planes (vs_nhwc_conv_f16x3_layer): hi / lo [B,T,F,64] f16,
    scale2 the device pair {s, 1/s}; -> (out_hi, out_lo, out_scale2, amax_out [1024] uint32 view as int32, scratch).
    amax_in: int32 tensor holding float bit patterns whose maximum is max |x| (default: computed here from the planes)."""
    _call.dev_check(hi, "hi", torch.float16)
    _call.dev_check(lo, "lo", torch.float16)
    for n, t in (("w", w), ("bn_scale", bn_scale), ("bn_shift", bn_shift), ("scale2", scale2)):
        _call.dev_check(t, n)
    B, T, F, C = hi.shape
    KT, KF = w.shape[2], w.shape[3]
    if amax_in is None:
        m = ((hi.float() + lo.float()) * scale2[1]).abs().max().reshape(1)
        amax_in = m.view(torch.int32)
    ready = scratch is not None
    if scratch is None:
        scratch = torch.empty(_lib.load().vs_nhwc_conv_f16x3_scratch_bytes(KT, KF), dtype=torch.uint8, device=hi.device)
    out_hi, out_lo = torch.empty_like(hi), torch.empty_like(lo)
    out_s2 = torch.empty(2, dtype=torch.float32, device=hi.device)
    amax_out = torch.zeros(1024, dtype=torch.int32, device=hi.device)
    _call.call("nhwc_conv_f16x3_layer", hi.device, hi, lo, scale2, amax_in, amax_in.numel(), w, bn_scale, bn_shift, scratch, int(ready),
               out_hi, out_lo, out_s2, amax_out, B, T, F, KT, KF, dil, ACT_CODES[act])
    return out_hi, out_lo, out_s2, amax_out, scratch


def nhwc_conv_pack(w, transpose_flip: bool = False):
    """w [64,64,KT,KF] fp32 -> the register-fragment order vs_nhwc_conv / vs_nhwc_conv_dy take (uint8 tensor)."""
    _call.dev_check(w, "w")
    KT, KF = w.shape[2], w.shape[3]
    packed = torch.empty(_lib.load().vs_nhwc_conv_packed_bytes(KT, KF), dtype=torch.uint8, device=w.device)
    _call.call("nhwc_conv_pack", w.device, w, packed, KT, KF, int(transpose_flip))
    return packed


def nhwc_conv_first(x, w, scale, shift, act: str, stats: bool = False):
    """cnn1: x [B,T,F] fp32, w [64,1,1,7] -> act(conv * scale + shift) as [B,T,F,64] bf16 (+ [64,2] statistics)."""
    for n, t in (("x", x), ("w", w), ("scale", scale), ("shift", shift)):
        _call.dev_check(t, n)
    B, T, F = x.shape
    out = torch.empty(B, T, F, 64, dtype=torch.bfloat16, device=x.device)
    st = torch.zeros(64, 64, 2, dtype=torch.float64, device=x.device) if stats else None
    _call.call("nhwc_conv_first", x.device, x, w, scale, shift, out, B, T, F, ACT_CODES[act], st)
    return (out, st.sum(0)) if stats else out


def bn_finalize(stats, count: float, gamma, beta, running_mean=None, running_var=None, eps: float = 1e-5, momentum: float = 0.1):
    """Train-mode BatchNorm2d constants from epilogue statistics (vs_bn_finalize): stats [slots, C, 2] float64 {sum, sum of
    squares} (folded in place) -> (scale, shift, mean, invstd); running_mean / running_var are updated in place when given."""
    _call.dev_check(stats, "stats", torch.float64)
    for n, t in (("gamma", gamma), ("beta", beta)):
        _call.dev_check(t, n)
    slots, C = stats.shape[0], stats.shape[1]
    scale, shift, mean, invstd = (torch.empty(C, dtype=torch.float32, device=stats.device) for _ in range(4))
    _call.call("bn_finalize", stats.device, stats, slots, float(count), C, gamma, beta, running_mean, running_var, eps, momentum,
               scale, shift, mean, invstd)
    return scale, shift, mean, invstd


def nhwc_first_moments(x):
    """x [B,T,F] fp32 -> the 35 float64 moments of its seven zero-padded shifts (vs_nhwc_first_moments)."""
    _call.dev_check(x, "x")
    B, T, F = x.shape
    mom = torch.empty(35, dtype=torch.float64, device=x.device)
    _call.call("nhwc_first_moments", x.device, x, B, T, F, mom)
    return mom


def nhwc_first_stats(mom, w, bias, count: float):
    """moments -> [1, 64, 2] float64 {sum, sum of squares} of z1 = conv(x) + bias (one slot of vs_bn_finalize)."""
    _call.dev_check(mom, "moments", torch.float64)
    stats = torch.empty(1, 64, 2, dtype=torch.float64, device=mom.device)
    _call.call("nhwc_first_stats", mom.device, mom, w, bias, float(count), stats)
    return stats


def nhwc_first_bwd(da, x, w, bias, act: str, training: bool, scale, shift, mean, invstd):
    """cnn1 + BatchNorm + activation backward in one pass over da [B,T,F,64] bf16 -> (dw [64,7], dgamma, dbeta, dbias)."""
    _call.dev_check(da, "da", torch.bfloat16)
    _call.dev_check(x, "x")
    B, T, F = x.shape
    dev = x.device
    dg, db, dbias = (torch.empty(64, dtype=torch.float32, device=dev) for _ in range(3))
    dw = torch.empty(64, 7, dtype=torch.float32, device=dev)
    scratch = torch.empty(_lib.load().vs_nhwc_first_bwd_scratch_doubles(), dtype=torch.float64, device=dev)
    _call.call("nhwc_first_bwd", da.device, da, x, w, bias, B, T, F, ACT_CODES[act], BN_TRAIN if training else BN_EVAL, scale, shift,
               mean, invstd, dg, db, dbias, dw, scratch)
    return dw, dg, db, dbias


def nhwc_bn_apply(z, scale, shift, act: str):
    _call.dev_check(z, "z", torch.bfloat16)
    a = torch.empty_like(z)
    _call.call("nhwc_bn_apply", z.device, z, a, z.numel() // 64, ACT_CODES[act], scale, shift)
    return a


def nhwc_conv_last(x, w, scale, shift, act: str):
    """cnn8 + transpose/view: x [B,T,F,64] bf16, w [8,64,1,1] -> [B,T,8F] fp32 (feature index c*F+f)."""
    _call.dev_check(x, "x", torch.bfloat16)
    B, T, F, _ = x.shape
    out = torch.empty(B, T, 8 * F, dtype=torch.float32, device=x.device)
    _call.call("nhwc_conv_last", x.device, x, w, scale, shift, out, B, T, F, ACT_CODES[act])
    return out


def nhwc_conv_last_pre(z7, pre_scale, pre_shift, pre_act: str, w, scale, shift, stats: bool = False):
    """cnn8 on the un-normalised cnn7 output z7 [B,T,F,64] bf16 (its BatchNorm + activation applied on the way in)
    -> [B,T,8F] fp32 unactivated (+ [8,2] float64 {sum, sum of squares} per output channel)."""
    _call.dev_check(z7, "z7", torch.bfloat16)
    B, T, F, _ = z7.shape
    out = torch.empty(B, T, 8 * F, dtype=torch.float32, device=z7.device)
    st = torch.zeros(64, 8, 2, dtype=torch.float64, device=z7.device) if stats else None
    _call.call("nhwc_conv_last_pre", z7.device, z7, pre_scale, pre_shift, ACT_CODES[pre_act], w, scale, shift, out, st, B, T, F)
    return (out, st.sum(0)) if stats else out


def nhwc_conv_wgrad(dz, x, KT: int, KF: int, dil: int):
    """dz, x [B,T,F,64] bf16 -> dw [64,64,KT,KF] fp32."""
    _call.dev_check(dz, "dz", torch.bfloat16)
    _call.dev_check(x, "x", torch.bfloat16)
    B, T, F, _ = x.shape
    part = torch.empty(_lib.load().vs_nhwc_conv_wgrad_partial_floats(KT, KF), dtype=torch.float32, device=x.device)
    dw = torch.empty(64, 64, KT, KF, dtype=torch.float32, device=x.device)
    _call.call("nhwc_conv_wgrad", dz.device, dz, x, part, dw, B, T, F, KT, KF, dil)
    return dw


def nhwc_bn_act_bwd(da, z, act: str, training: bool, scale, shift, mean, invstd):
    """da, z [.., 64] bf16 -> (dz bf16, dgamma, dbeta, dbias)."""
    _call.dev_check(da, "da", torch.bfloat16)
    _call.dev_check(z, "z", torch.bfloat16)
    dev = z.device
    dz = torch.empty_like(da)
    dg, db, dbias = (torch.empty(64, dtype=torch.float32, device=dev) for _ in range(3))
    stats = torch.empty(64 * 64 * 2, dtype=torch.float64, device=dev)
    coef = torch.empty(192, dtype=torch.float32, device=dev)
    _call.call("nhwc_bn_act_bwd", da.device, da, z, dz, z.numel() // 64, ACT_CODES[act], BN_TRAIN if training else BN_EVAL,
               scale, shift, mean, invstd, dg, db, dbias, stats, coef)
    return dz, dg, db, dbias


def nhwc_bn_act_bwd_first(da, z, x, act: str, training: bool, scale, shift, mean, invstd):
    """cnn1: da, z [B,T,F,64] bf16, x [B,T,F] fp32 -> (dw [64,7], dgamma, dbeta, dbias)."""
    dev = z.device
    B, T, F = x.shape
    dg, db, dbias = (torch.empty(64, dtype=torch.float32, device=dev) for _ in range(3))
    dw = torch.empty(64, 7, dtype=torch.float32, device=dev)
    stats = torch.empty(64 * 64 * 2, dtype=torch.float64, device=dev)
    coef = torch.empty(192, dtype=torch.float32, device=dev)
    acc = torch.empty(448, dtype=torch.float64, device=dev)
    _call.call("nhwc_bn_act_bwd_first", da.device, da, z, x, B, T, F, ACT_CODES[act], BN_TRAIN if training else BN_EVAL,
               scale, shift, mean, invstd, dg, db, dbias, dw, stats, coef, acc)
    return dw, dg, db, dbias


def nhwc_conv_last_bwd(dz8, w, a7):
    """dz8 [B,T,8F] fp32, w [8,64,1,1], a7 [B,T,F,64] bf16 -> (din [B,T,F,64] bf16, dw [8,64])."""
    _call.dev_check(dz8, "dz8")
    _call.dev_check(a7, "a7", torch.bfloat16)
    B, T, F, _ = a7.shape
    din = torch.empty_like(a7)
    part = torch.empty(_lib.load().vs_nhwc_conv_last_bwd_blocks() * 512, dtype=torch.float32, device=a7.device)
    dw = torch.empty(8, 64, dtype=torch.float32, device=a7.device)
    _call.call("nhwc_conv_last_bwd", dz8.device, dz8, w, a7, din, part, dw, B, T, F)
    return din, dw


def nhwc_conv_dy(dz, packed, z, act: str, bn_scale, bn_shift, bn_mean, bn_invstd, KT: int, KF: int, dil: int):
    """Data gradient with the dy epilogue: dz [B,T,F,64] bf16, packed = transposed/flipped weights, z = the lower layer's
    conv output -> (dy bf16, stats [64 slots, 64, 2] float64 with the per-channel sums of dy and dy * xhat)."""
    _call.dev_check(dz, "dz", torch.bfloat16)
    _call.dev_check(z, "z", torch.bfloat16)
    B, T, F, _ = dz.shape
    dy = torch.empty_like(dz)
    stats = torch.zeros(64, 64, 2, dtype=torch.float64, device=dz.device)
    _call.call("nhwc_conv_dy", dz.device, dz, packed, dy, z, ACT_CODES[act], bn_scale, bn_shift, bn_mean, bn_invstd, stats,
               B, T, F, KT, KF, dil)
    return dy, stats


def nhwc_conv_last_bwd_dy(dz8, w, a7, z7, act: str, bn_scale, bn_shift, bn_mean, bn_invstd):
    """cnn8 backward with the dy epilogue -> (dy7 bf16, dw [8,64], stats)."""
    _call.dev_check(dz8, "dz8")
    if a7 is not None:                      # None: recomputed from z7 inside the kernel
        _call.dev_check(a7, "a7", torch.bfloat16)
    _call.dev_check(z7, "z7", torch.bfloat16)
    B, T, F, _ = z7.shape
    dy = torch.empty_like(z7)
    part = torch.empty(_lib.load().vs_nhwc_conv_last_bwd_blocks() * 512, dtype=torch.float32, device=z7.device)
    dw = torch.empty(8, 64, dtype=torch.float32, device=z7.device)
    stats = torch.zeros(64, 64, 2, dtype=torch.float64, device=z7.device)
    _call.call("nhwc_conv_last_bwd_dy", dz8.device, dz8, w, a7, dy, part, dw, z7, ACT_CODES[act], bn_scale, bn_shift, bn_mean, bn_invstd,
               stats, B, T, F)
    return dy, dw, stats


def nhwc_bn_bwd_from_dy(dy, z, stats, training: bool, scale, mean, invstd):
    """Second pass of the BatchNorm backward from dy and its sums -> (dz bf16, dgamma, dbeta, dbias)."""
    _call.dev_check(dy, "dy", torch.bfloat16)
    _call.dev_check(z, "z", torch.bfloat16)
    dev = z.device
    dz = torch.empty_like(dy)
    dg, db, dbias = (torch.empty(64, dtype=torch.float32, device=dev) for _ in range(3))
    coef = torch.empty(192, dtype=torch.float32, device=dev)
    _call.call("nhwc_bn_bwd_from_dy", dy.device, dy, z, dz, z.numel() // 64, BN_TRAIN if training else BN_EVAL, scale, mean, invstd,
               dg, db, dbias, stats, coef)
    return dz, dg, db, dbias


def nhwc_bn_bwd_first_from_dy(dy, z, x, stats, training: bool, scale, mean, invstd):
    """cnn1, from dy -> (dw [64,7], dgamma, dbeta, dbias)."""
    dev = z.device
    B, T, F = x.shape
    dg, db, dbias = (torch.empty(64, dtype=torch.float32, device=dev) for _ in range(3))
    dw = torch.empty(64, 7, dtype=torch.float32, device=dev)
    coef = torch.empty(192, dtype=torch.float32, device=dev)
    acc = torch.empty(448, dtype=torch.float64, device=dev)
    _call.call("nhwc_bn_bwd_first_from_dy", dy.device, dy, z, x, B, T, F, BN_TRAIN if training else BN_EVAL, scale, mean, invstd,
               dg, db, dbias, dw, stats, coef, acc)
    return dw, dg, db, dbias


def gemm_bf16(A, B, M: int, N: int, K: int, a_kmajor: bool = False, b_kmajor: bool = False, rowbias=None, group: int = 1,
              out=None, accumulate: bool = False):
    """C[M,N] (+)= op(A) op(B) on bf16 operands (csrc/gemm_bf16.hip); A, B 2-D bf16 tensors (row form [rows, ld >= K padded
    to 64], K-major form [K, ld]); fp32 result."""
    _call.dev_check(A, "A", torch.bfloat16)
    _call.dev_check(B, "B", torch.bfloat16)
    C = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=A.device)
    _call.call("gemm_bf16", A.device, int(a_kmajor), int(b_kmajor), A, A.shape[1], B, B.shape[1], C, C.shape[1], M, N, K,
               rowbias, rowbias.shape[1] if rowbias is not None else 0, group, int(accumulate))
    return C


def gemm_bf16_gated(A, B, gate, M: int, N: int, K: int, a_kmajor: bool = False, b_kmajor: bool = False, out=None):
    """C = op(A) op(B) where gate > 0, else 0 (vs_gemm_bf16_gated: the head's data gradients of vs_backward); gate fp32 [M, ldg >= N];
    out: a preallocated [M, ldc >= N] fp32 result (columns >= N are left untouched)."""
    _call.dev_check(A, "A", torch.bfloat16)
    _call.dev_check(B, "B", torch.bfloat16)
    _call.dev_check(gate, "gate", torch.float32)
    C = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=A.device)
    _call.call("gemm_bf16_gated", A.device, int(a_kmajor), int(b_kmajor), A, A.shape[1], B, B.shape[1], C, C.shape[1], M, N, K,
               gate, gate.shape[1])
    return C


def gemm_bf16_split(A, B, M: int, N: int, K: int, split_m: int, a_kmajor: bool = False, b_kmajor: bool = False, ldc: Optional[int] = None):
    """The same contraction stored into two matrices stacked along M (vs_gemm_bf16_split: the dW_ih store of vs_backward):
    returns (C [split_m, ldc], C2 [M - split_m, ldc]); columns >= N are left untouched (NaN-filled here so a test sees a
    stray store)."""
    _call.dev_check(A, "A", torch.bfloat16)
    _call.dev_check(B, "B", torch.bfloat16)
    ldc = N if ldc is None else ldc
    C = torch.full((split_m, ldc), float("nan"), dtype=torch.float32, device=A.device)
    C2 = torch.full((M - split_m, ldc), float("nan"), dtype=torch.float32, device=A.device)
    _call.call("gemm_bf16_split", A.device, int(a_kmajor), int(b_kmajor), A, A.shape[1], B, B.shape[1], C, C2, ldc, split_m,
               M, N, K, 0)
    return C, C2


def cvt_rows_bf16(x, K: int, Kp: int):
    _call.dev_check(x, "x")
    out = torch.empty(x.shape[0], Kp, dtype=torch.bfloat16, device=x.device)
    _call.call("cvt_rows_bf16", x.device, x, x.shape[0], K, x.shape[1], out, Kp)
    return out


def lstm_status(dims: VsDims, tape: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> int:
    """vs_lstm_status: 0 = the persistent BiLSTM kernels that last ran on these buffers completed, 1 = one gave up
    (output NaN-poisoned).  Synchronises the current stream.  Its rc is an answer, not only an error code, so it is
    read here, not in ``_call.call``."""
    rc = _lib.load().vs_lstm_status(ctypes.byref(dims), _call.ptr(tape), tape.numel() if tape is not None else 0,
                                    _call.ptr(workspace), workspace.numel() if workspace is not None else 0, _call.stream())
    if rc < 0:
        check(rc, "vs_lstm_status")
    return rc
