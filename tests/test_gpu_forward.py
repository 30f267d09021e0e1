"""GPU parity tests proper: the nn.Module surface -> C ABI -> HIP kernels, compared with
(1) the committed golden tensors produced by the upstream reference module,
(2) the CPU oracle on seeded inputs,
(3) size-independent properties at BASELINE.json's full batch size.
Contract (BASELINE.json north_star): <= 1e-4 relative in fp32 and mask MSE <= 1e-4."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLDEN_CASES, load_golden
from oracle import reference_forward as R

pytestmark = pytest.mark.gpu
REL_TOL = 1e-4
MSE_TOL = 1e-4


def _rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def _module(g):
    import voicesplit_amd as V
    d = g["dims"]
    cls = V.VoiceSplit if g["model"] == "voicesplit" else V.VoiceFilter
    m = cls(V.default_config(d["num_freq"], d["emb_dim"], d["lstm_dim"], d["fc1_dim"], d["fc2_dim"]))
    sd = R.spread_logits(R.build_state_dict(d, g["seed"]), g["gain"])
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd


def _thin(name, arr, full):
    if not full:
        return arr
    if name == "cnn8":
        return arr[:, :, ::16, ::4]
    if name in ("lstm_out", "logits"):
        return arr[:, ::4]
    return arr


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_module_matches_upstream_golden(name):
    """Every stage the fixture recorded: cnn8 (conv stack), lstm_out, logits, mask."""
    from voicesplit_amd import _lib, ops
    g = load_golden(name)
    m, sd = _module(g)
    m.train(g["training"])
    x, dvec = R.synthetic_inputs(g["B"], g["T"], g["dims"], g["seed"])
    with torch.no_grad():
        mask = m(x.cuda(), dvec.cuda())
    torch.cuda.synchronize()
    d = g["dims"]
    dims = ops.make_dims(g["B"], g["T"], d["num_freq"], d["emb_dim"], d["lstm_dim"], d["fc1_dim"], d["fc2_dim"])
    lay = ops.workspace_layout(dims)
    ws = ops.get_workspace(dims, x.cuda().device)
    full = d["num_freq"] > 100
    B, T, Fq, H = g["B"], g["T"], d["num_freq"], d["lstm_dim"]
    if not g["training"] and ops.get_conv_math() == "f16x3" and _lib.get_option("FEAT_ROWS"):
        # the whole-path eval forward of this arithmetic holds the features only as the LSTM input GEMM's split operand (cnn8 writes it):
        # hi and lo f16 rows [B T][Kp] in the second ping-pong buffer, scale pair in gemm_scales; the K padding must be zero
        Kp = (8 * Fq + 63) // 64 * 64
        na = (B * T * Kp * 2 + 255) // 256 * 256
        hi = ops.ws_view(ws, lay.act1, (B * T, Kp), torch.float16).float()
        lo = ops.ws_view(ws, lay.act1 + na, (B * T, Kp), torch.float16).float()
        assert not hi[:, 8 * Fq:].any() and not lo[:, 8 * Fq:].any()
        inv = ops.ws_view(ws, lay.gemm_scales, (2,))[1]
        feat = ((hi + lo) * inv)[:, :8 * Fq].reshape(B, T, 8, Fq).cpu().permute(0, 2, 1, 3).numpy()
    else:
        feat = ops.ws_view(ws, lay.feat, (B, T, 8, Fq)).cpu().permute(0, 2, 1, 3).numpy()     # -> [B,8,T,F]
    lstm_out = ops.ws_view(ws, lay.lstm_out, (B, T, 2 * H)).cpu().numpy()
    assert _rel(_thin("cnn8", feat, full), g["cnn8"]) < REL_TOL
    assert _rel(_thin("lstm_out", lstm_out, full), g["lstm_out"]) < REL_TOL
    sdc = {k: v.cuda() for k, v in m.state_dict().items()}
    _, logits = ops.head(sdc, ops.ws_view(ws, lay.lstm_out, (B, T, 2 * H)).clone(), dims, want_logits=True)
    assert _rel(_thin("logits", logits.cpu().numpy(), full), g["logits"]) < REL_TOL
    mask = mask.cpu().numpy()
    assert mask.shape == g["mask"].shape
    assert _rel(mask, g["mask"]) < REL_TOL
    assert ((mask - g["mask"]) ** 2).mean() < MSE_TOL
    if g["training"]:
        after = m.state_dict()
        for k in after:
            if "running_" in k:
                assert _rel(after[k].cpu().numpy(), g["after/" + k]) < REL_TOL, k
            if "num_batches" in k:
                assert int(after[k]) == int(g["after/" + k])


@pytest.mark.parametrize("cls_name,act", [("VoiceSplit", "mish"), ("VoiceFilter", "relu")])
@pytest.mark.parametrize("B,T", [(2, 45), (5, 17)])
def test_stages_match_fp64_oracle(cls_name, act, B, T):
    """Per-stage comparison against the oracle run in fp64 (ground truth)."""
    import voicesplit_amd as V
    from voicesplit_amd import ops
    dims_d = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
    sd = R.spread_logits(R.build_state_dict(dims_d, 21), 6.0)
    x, dvec = R.synthetic_inputs(B, T, dims_d, 21)
    with torch.no_grad():
        ref = R.forward(R.cast_state_dict(sd, torch.float64), x.double(), dvec.double(), act=act, lstm_impl="loop")
    sdc = {k: v.cuda() for k, v in sd.items()}
    dims = ops.make_dims(B, T, 53, 24, 32, 44, 53)
    feat = ops.conv_stack(sdc, x.cuda(), dims, act)
    assert _rel(feat.cpu().numpy(), ref["lstm_in"][..., :8 * 53].numpy()) < REL_TOL
    lo = ops.bilstm(sdc, feat, dvec.cuda(), dims)
    assert _rel(lo.cpu().numpy(), ref["lstm_out"].numpy()) < REL_TOL
    mask, logits = ops.head(sdc, lo, dims, want_logits=True)
    assert _rel(logits.cpu().numpy(), ref["logits"].numpy()) < REL_TOL
    assert _rel(mask.cpu().numpy(), ref["mask"].numpy()) < REL_TOL


def test_full_batch_properties():
    """BASELINE config: B=64, [64,301,601] + [64,256], fp32, forward only.  The oracle would take
    ~40 s of CPU for this, so check size-independent properties instead:
    batch independence (eval BN): row i of the B=64 result == the same utterance run alone to fp32 rounding
    (no kernel's reduction order depends on B, but the split-f16 operands carry one power-of-two scale per
    TENSOR, derived from the batch's |max|: another scale moves which low parts fall under the f16 subnormal
    step.  Measured 6e-7 on masks in (0, 1) -- tools/batch_independence_probe.py, both conv routes; the NCHW
    route of rounds 1-3 is bit-exact only while the batch mates leave every layer's |max| in its binade),
    duplicated utterances of one batch give identical masks, outputs are finite and inside (0,1)."""
    import voicesplit_amd as V
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, 0), 8.0)
    m = V.VoiceSplit(V.default_config()).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    x, dvec = R.synthetic_inputs(64, 301, dims_d, 0)
    x1, d1 = R.synthetic_inputs(1, 301, dims_d, 0)      # the golden fixture's utterance
    x[0], dvec[0] = x1[0], d1[0]
    x[7], dvec[7] = x[3], dvec[3]
    xc, dc = x.cuda(), dvec.cuda()
    with torch.no_grad():
        big = m(xc, dc)
        one = m(xc[3:4].contiguous(), dc[3:4].contiguous())
        last = m(xc[63:64].contiguous(), dc[63:64].contiguous())
    torch.cuda.synchronize()
    assert big.shape == (64, 301, 601)
    assert torch.isfinite(big).all() and big.min() >= 0 and big.max() <= 1
    assert torch.equal(big[7], big[3])
    assert (big[3] - one[0]).abs().max().item() < 2e-6 and (big[63] - last[0]).abs().max().item() < 2e-6
    # and the B=1 result is the one pinned by the upstream golden (vs_full_b1 uses seed 0, x[0])
    g = load_golden("vs_full_b1")
    assert _rel(big[0:1].cpu().numpy(), g["mask"]) < REL_TOL


def test_library_is_the_loaded_native_code():
    from voicesplit_amd import _lib
    _lib.load()
    maps = open("/proc/self/maps").read()
    assert "libvoicesplit_hip.so" in maps


def test_long_form_windows_match_per_window_calls():
    """BASELINE configs[4]: a 30 s clip (3001 frames) cut into 10 independent 301-frame windows
    and run as one batch gives what the module gives window by window -- to fp32 rounding: the split-f16 operands'
    power-of-two scales are per tensor, i.e. per batch (test_full_batch_properties)."""
    import voicesplit_amd as V
    from voicesplit_amd.streaming import plan_windows, separate_long
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, 0), 8.0)
    m = V.VoiceSplit(V.default_config()).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    g = torch.Generator().manual_seed(9)
    spec = torch.rand(3001, 601, generator=g).cuda()
    dvec = R.synthetic_inputs(1, 301, dims_d, 9)[1][0].cuda()
    mask = separate_long(m, spec, dvec, window=301, halo=0)
    assert mask.shape == (3001, 601) and torch.isfinite(mask).all()
    plan = plan_windows(3001, 301, 0)
    assert len(plan) == 10
    with torch.no_grad():
        w3 = m(spec[903:1204][None].contiguous(), dvec[None])          # window 3 on its own
    assert (mask[903:1204] - w3[0]).abs().max().item() < 2e-6
    last = torch.zeros(1, 301, 601, device="cuda")
    last[0, :292] = spec[2709:]
    with torch.no_grad():
        w9 = m(last, dvec[None])
    assert (mask[2709:] - w9[0, :292]).abs().max().item() < 2e-6


def test_exact_long_form_equals_a_whole_clip_pass():
    """a 1000-frame clip as 6 windows of 301 frames with 65-frame halos through the conv stack,
    then ONE full-length BiLSTM + head pass (LSTM state carried across every window boundary), against (a) the
    module run on the whole clip and (b) the CPU oracle on the whole clip.  Residual error stated below."""
    import voicesplit_amd as V
    from voicesplit_amd.streaming import separate_long, separate_long_exact
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, 3), 8.0)
    m = V.VoiceSplit(V.default_config()).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    g = torch.Generator().manual_seed(11)
    T_long = 1000
    spec = torch.rand(T_long, 601, generator=g)
    dvec = R.synthetic_inputs(1, 301, dims_d, 11)[1][0]
    conv_stage, sequence_stage = m.long_form_stages()
    got = separate_long_exact(conv_stage, sequence_stage, spec.cuda(), dvec.cuda(), window=301, halo=65).cpu()
    with torch.no_grad():
        whole = m(spec[None].cuda(), dvec[None].cuda())[0].cpu()
        ref = R.forward(sd, spec[None], dvec[None], act="mish")["mask"][0]
    # (a) same kernels, same arithmetic; only the per-tensor power-of-two operand scales of the split-f16 convs
    #     can differ between a window batch and the whole clip: rounding level
    assert _rel(got.numpy(), whole.numpy()) < 2e-5
    # (b) the path's contract against the oracle, at 3.3x the training length
    assert _rel(got.numpy(), ref.numpy()) < REL_TOL
    assert ((got.numpy() - ref.numpy()) ** 2).mean() < MSE_TOL
    # restarting the BiLSTM in every window (BASELINE configs[4] as literally stated) is a different function
    restart = separate_long(m, spec.cuda(), dvec.cuda(), window=301, halo=65).cpu()
    assert _rel(restart.numpy(), ref.numpy()) > 10 * REL_TOL
    with pytest.raises(RuntimeError):
        m.train().long_form_stages()


@pytest.mark.parametrize("cls_name", ["VoiceSplit", "VoiceFilter"])
@pytest.mark.parametrize("math", ["f16x3", "fp32", "bf16"])
def test_prepared_weights_forward_is_bit_identical_and_tracks_the_parameters(cls_name, math):
    """Eval-mode calls go through vs_prepare_weights (once) + vs_forward_prepared: the same kernels on the same
    operands as vs_forward, so the mask is bit-identical; the prepared buffer is reused while the parameters are
    untouched and rebuilt as soon as one changes in place, is replaced, or a running statistic moves."""
    import voicesplit_amd as V
    from voicesplit_amd import ops
    dims_d = dict(num_freq=601, emb_dim=256, lstm_dim=48, fc1_dim=64, fc2_dim=601)
    sd = R.spread_logits(R.build_state_dict(dims_d, 11), 6.0)
    prev = ops.get_conv_math()
    ops.set_conv_math(math)
    try:
        m = getattr(V, cls_name)(V.default_config(601, 256, 48, 64, 601))
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        x, dvec = R.synthetic_inputs(2, 40, dims_d, 3)
        xc, dc = x.cuda(), dvec.cuda()

        def direct():
            t = {k: v.detach() for k, v in m._tensors().items()}
            return ops.forward(t, xc, dc, m._dims(2, 40), m.conv_act, training=False)

        with torch.no_grad():
            y1 = m(xc, dc)
            prep1 = m.__dict__["_prepared"]
            assert torch.equal(y1, direct())
            y2 = m(xc, dc)
            assert m.__dict__["_prepared"] is prep1 and torch.equal(y1, y2)          # reused
            y3 = m(xc[:1, :17].contiguous(), dc[:1])                                   # another B, T: same buffer
            assert m.__dict__["_prepared"] is prep1 and y3.shape == (1, 17, 601)
            m.conv[1].weight.mul_(1.5)                                                 # in-place update (optimizer step)
            y4 = m(xc, dc)
            assert m.__dict__["_prepared"] is not prep1
            assert torch.equal(y4, direct()) and not torch.equal(y4, y1)
            prep2 = m.__dict__["_prepared"]
            m.conv[2].running_var.add_(0.25)                                           # a BatchNorm buffer
            y5 = m(xc, dc)
            assert m.__dict__["_prepared"] is not prep2 and torch.equal(y5, direct()) and not torch.equal(y5, y4)
            m.load_state_dict(sd, strict=True)                                         # copy_ into the same storage
            assert torch.equal(m(xc, dc), y1)
        m.train()
        assert "_prepared" not in m.__dict__                                           # dropped when training starts
        m(xc, dc)
        assert "_prepared" not in m.__dict__                                           # training calls never build it
    finally:
        ops.set_conv_math(prev)


@pytest.mark.parametrize("amp", [0.0, 1e-4, 1e3])
def test_forward_tracks_the_input_range(amp):
    """Silence, a spectrogram four decades below and three above unit range: every layer of the fp32-class forward derives its
    operands' scales from tracked magnitudes on the device, so the mask stays at the oracle's (1e-4) for all of them."""
    import voicesplit_amd as V
    dims_d = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
    sd = R.spread_logits(R.build_state_dict(dims_d, 5), 6.0)
    x, dvec = R.synthetic_inputs(2, 40, dims_d, 5)
    x = x * amp
    m = V.VoiceSplit(V.default_config(53, 24, 32, 44, 53)).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    with torch.no_grad():
        got = m(x.cuda(), dvec.cuda()).double().cpu()
        ref = R.forward(R.cast_state_dict(sd, torch.float64), x.double(), dvec.double(), act="mish")["mask"]
    assert torch.isfinite(got).all()
    assert _rel(got.numpy(), ref.numpy()) < REL_TOL


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
@pytest.mark.parametrize("F,B,T", [(53, 3, 45), (601, 2, 40), (16, 2, 40), (16, 1, 5)])
def test_cnn8_writing_the_gemm_operand_agrees_with_the_separate_passes(F, B, T, math):
    """vs_set_option(VS_OPT_FEAT_ROWS): the whole-path eval forward lets cnn8 write the LSTM input GEMM's A operand itself (rows padded
    to the GEMM's K block) instead of fp32 features + passes over them.  fp32-class arithmetic: split-f16 hi / lo rows at a scale
    planned from a bound instead of the measured |max| -- both powers of two, so the halves are the same numbers unless a lo half
    underflows (usually bit-identical masks), both forms at the oracle's 1e-4.  bf16 arithmetic: the same bf16 rounding of the same
    values -- bit-identical.  Prepared and unprepared weights take the same route (a clip of 5 frames x 16 bins has no room for the
    unprepared split weights: there the unprepared forward keeps the fp32 features and the converting GEMM -- its own summation order)."""
    import voicesplit_amd as V
    from voicesplit_amd import _lib, ops
    dims_d = dict(num_freq=F, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=F)
    sd = R.spread_logits(R.build_state_dict(dims_d, 31), 6.0)
    x, dvec = R.synthetic_inputs(B, T, dims_d, 31)
    m = V.VoiceSplit(V.default_config(F, 24, 32, 44, F)).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    prev, prev_math = _lib.get_option("FEAT_ROWS"), ops.get_conv_math()
    got = {}
    try:
        ops.set_conv_math(math)
        for mode in (1, 0):
            _lib.set_option("FEAT_ROWS", mode)
            with torch.no_grad():
                t = {k: v.detach() for k, v in m._tensors().items()}
                direct = ops.forward(t, x.cuda(), dvec.cuda(), m._dims(B, T), m.conv_act, training=False)
                prepared = m(x.cuda(), dvec.cuda())
            if (F, B, T) != (16, 1, 5):
                assert torch.equal(direct, prepared)
            else:
                assert _rel(direct.double().cpu().numpy(), prepared.double().cpu().numpy()) < (2e-2 if math == "bf16" else 2e-6)
            got[mode] = prepared.double().cpu()
    finally:
        _lib.set_option("FEAT_ROWS", prev)
        ops.set_conv_math(prev_math)
    if math == "bf16":
        assert torch.isfinite(got[1]).all() and torch.equal(got[1], got[0])
        return
    ref = R.forward(R.cast_state_dict(sd, torch.float64), x.double(), dvec.double(), act="mish")["mask"]
    assert _rel(got[1].numpy(), ref.numpy()) < REL_TOL and _rel(got[0].numpy(), ref.numpy()) < REL_TOL
    assert _rel(got[1].numpy(), got[0].numpy()) < 2e-6


_TRAIN_REF = {}


def _train_mode_reference(B, T):
    """Seeded inputs and the fp64 oracle's train-mode forward on them: mask and the sixteen running statistics after the call.
    Computed once per shape and shared by the arithmetics; read only."""
    if (B, T) not in _TRAIN_REF:
        dims_d = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
        sd = R.spread_logits(R.build_state_dict(dims_d, 21), 6.0)
        x, dvec = R.synthetic_inputs(B, T, dims_d, 21)
        bn_out = {}
        with torch.no_grad():
            ref = R.forward(R.cast_state_dict(sd, torch.float64), x.double(), dvec.double(), act="mish", training=True, bn_out=bn_out,
                            lstm_impl="loop")
        stats = {k: v.numpy() for k, v in bn_out.items() if "running_" in k}
        assert len(stats) == 16
        _TRAIN_REF[(B, T)] = (sd, x, dvec, ref["mask"].numpy(), stats)
    return _TRAIN_REF[(B, T)]


@pytest.mark.parametrize("math", ["fp32", "f16x3", "bf16"])
@pytest.mark.parametrize("B,T", [(2, 45), (5, 17)])
def test_tapeless_train_mode_forward_matches_fp64_oracle(B, T, math):
    """model.train() under no_grad: vs_forward with batch-statistics BatchNorm and no tape, in every arithmetic (the bf16 one runs cnn1
    by recomputation, the in-place BatchNorm apply and the feature-layout BatchNorm of cnn8).  Mask and the sixteen running statistics
    after the call against the fp64 oracle.  Bounds: this file's for the fp32-class arithmetics; for bf16 the mask bounds that
    tests/test_gpu_bf16.py holds the training=True forward of the same fixture to (max abs 6e-2, MSE 1e-4), and for its running
    statistics the 2e-2 of tests/test_gpu_nhwc.py's train-mode conv stack (relative to the tensor's maximum, floor 1e-6)."""
    import voicesplit_amd as V
    from voicesplit_amd import ops
    sd, x, dvec, ref_mask, ref_stats = _train_mode_reference(B, T)
    prev = ops.get_conv_math()
    ops.set_conv_math(math)
    try:
        m = V.VoiceSplit(V.default_config(53, 24, 32, 44, 53))
        m.load_state_dict(sd, strict=True)
        m = m.cuda().train()
        with torch.no_grad():
            mask = m(x.cuda(), dvec.cuda())
        torch.cuda.synchronize()
    finally:
        ops.set_conv_math(prev)
    mask = mask.double().cpu().numpy()
    after = {k: v.double().cpu().numpy() for k, v in m.state_dict().items() if "running_" in k}
    assert sorted(after) == sorted(ref_stats)
    abs_err, mse = np.abs(mask - ref_mask).max(), ((mask - ref_mask) ** 2).mean()
    stat_err = {k: np.abs(after[k] - ref_stats[k]).max() / max(np.abs(ref_stats[k]).max(), 1e-6 if math == "bf16" else 1e-30) for k in after}
    print(f"tapeless train forward {math} B={B} T={T}: mask rel {_rel(mask, ref_mask):.3e} abs {abs_err:.3e} mse {mse:.3e}; "
          f"worst running statistic {max(stat_err.values()):.3e}")
    assert mask.shape == ref_mask.shape and np.isfinite(mask).all()
    if math == "bf16":
        assert abs_err < 6e-2 and mse < 1e-4
        assert max(stat_err.values()) < 2e-2, stat_err
    else:
        assert _rel(mask, ref_mask) < REL_TOL and mse < MSE_TOL
        assert max(stat_err.values()) < REL_TOL, stat_err
    assert all(int(v) == 1 for k, v in m.state_dict().items() if "num_batches" in k)
