"""GPU: several enrolled speakers out of one mixture with one conv pass (``model.forward_multi``, vs_forward_prepared_multi,
the shared-input mode of the tagged persistent recurrence).

Ground truth is the fp64 oracle (``oracle.reference_forward.forward``, eval mode) run once per speaker on that mixture alone (at
its own length where the batch is ragged).  Bounds are the project's own, unchanged: the fp32-class arithmetic is held to REL_TOL
on LSTM output, logits and mask and to MSE_TOL (tests/test_gpu_forward.py); VS_MATH_BF16 to LSTM_TOL, MASK_ABS_TOL and mask
MSE < 1e-4 (tests/test_gpu_bf16.py; it states no bound for logits, which are printed, not asserted, in that arithmetic).  Every
figure is printed before it is asserted.

Embeddings are L2-normalised random vectors times 8 (the ABI does not require unit norm): with plain unit-norm d-vectors and
these weights the speaker moves the mask by only 0.09-0.10 absolute (MSE 6.3e-4), which a mix-up of k or of b could survive
under the bf16 bounds.  Times 8, the fp64 oracle at B=2, T=20, K=3, seed 41 gives 0.52-0.56 absolute / MSE 2.2e-2 between two
speakers of one mixture and 0.96-1.23 relative on the LSTM output: over 200 times the bf16 MSE bound.  Every test asserts that
precondition on the oracle alone -- each pair of speakers of a mixture differs in mask MSE by more than 1e-3 -- before it
compares anything: a test that would pass with the speakers swapped shows nothing."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle import reference_audio as RA
from oracle import reference_forward as R
from test_gpu_bf16 import LSTM_TOL, MASK_ABS_TOL, _math
from test_gpu_forward import MSE_TOL, REL_TOL

pytestmark = pytest.mark.gpu
MODELS = [("VoiceSplit", "mish"), ("VoiceFilter", "relu")]
EMB_GAIN = 8.0
_ORACLE = {}


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _embeddings(B, K, E, seed):
    g = torch.Generator().manual_seed(seed + 177)
    e = torch.randn(B, K, E, generator=g)
    return EMB_GAIN * e / e.norm(dim=2, keepdim=True)


def _case(B, T, K, seed):
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, seed), 6.0)          # randomised BatchNorm statistics, spread logits
    x, _ = R.synthetic_inputs(B, T, dims_d, seed)
    return dims_d, sd, x, _embeddings(B, K, dims_d["emb_dim"], seed)


def _head64(sd64, lo):
    y = torch.relu(torch.nn.functional.linear(torch.relu(lo), sd64["fc1.weight"], sd64["fc1.bias"]))
    logits = torch.nn.functional.linear(y, sd64["fc2.weight"], sd64["fc2.bias"])
    return logits, torch.sigmoid(logits)


def _oracle(tag, sd, x, dvecs, act, lengths=None, conv_once=False):
    """ref[b][k] = {lstm_out, logits, mask} of mixture b alone (at its own length) with speaker k, fp64; cached, both arithmetics
    compare against it.  conv_once: the oracle's conv stack once per mixture, its BiLSTM and head per speaker (the d-vector
    enters at the LSTM input, models/voicesplit/model.py:70-81) -- the CPU time of many speakers per mixture."""
    key = (tag, act)
    if key not in _ORACLE:
        sd64 = R.cast_state_dict(sd, torch.float64)
        B, K = dvecs.shape[0], dvecs.shape[1]
        out = []
        with torch.no_grad():
            for b in range(B):
                n = x.shape[1] if lengths is None else lengths[b]
                xb = x[b:b + 1, :n].double()
                row = []
                if conv_once:
                    y = R.conv_stack(xb, sd64, act).transpose(1, 2).contiguous().view(1, n, -1)
                    for k in range(K):
                        e = dvecs[b, k].double().view(1, 1, -1).repeat(1, n, 1)
                        lo = R.bilstm(torch.cat((y, e), dim=2), sd64)
                        logits, mask = _head64(sd64, lo)
                        row.append({"lstm_out": lo[0].numpy(), "logits": logits[0].numpy(), "mask": mask[0].numpy()})
                else:
                    for k in range(K):
                        o = R.forward(sd64, xb, dvecs[b, k:k + 1].double(), act=act, lstm_impl="loop")
                        row.append({q: o[q][0].numpy() for q in ("lstm_out", "logits", "mask")})
                out.append(row)
        _ORACLE[key] = out
    return _ORACLE[key]


def _assert_speakers_differ(ref):
    """The precondition, on the oracle alone."""
    worst = min([float(((row[i]["mask"] - row[j]["mask"]) ** 2).mean()) for row in ref for i, j in itertools.combinations(range(len(row)), 2)]
                + [float("inf")])
    print(f"oracle: smallest mask MSE between two speakers of one mixture {worst:.3e}")
    assert worst > 1e-3
    return worst


def _model(cls_name, sd):
    import voicesplit_amd as V
    m = getattr(V, cls_name)(V.default_config())
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _dims(B, T):
    from voicesplit_amd import ops
    d = R.default_dims()
    return ops.make_dims(B, T, d["num_freq"], d["emb_dim"], d["lstm_dim"], d["fc1_dim"], d["fc2_dim"])


def _stages(m, sd, x, dvecs, act, lengths=None):
    """LSTM output [B,K,T,2H] through the stage entry point (``ops.bilstm_multi`` on the conv stage's features), logits through the
    head on it, mask through ``forward_multi``."""
    from voicesplit_amd import ops
    sdc = {k: v.cuda() for k, v in sd.items()}
    B, T, K = x.shape[0], x.shape[1], dvecs.shape[1]
    dims = _dims(B, T)
    xc, dc = x.cuda(), dvecs.cuda()
    feat = ops.conv_stack(sdc, xc, dims, act, lengths=lengths)
    lo = ops.bilstm_multi(sdc, feat, dc, dims, lengths=lengths)
    _, logits = ops.head(sdc, lo.view(B * K, T, -1), _dims(B * K, T), want_logits=True)
    with torch.no_grad():
        mask = m.forward_multi(xc, dc, lengths)
    torch.cuda.synchronize()
    assert tuple(lo.shape) == (B, K, T, 2 * dims.H) and tuple(mask.shape) == (B, K, T, dims.FC2)
    return lo.cpu().numpy(), logits.view(B, K, T, -1).cpu().numpy(), mask.cpu().numpy()


def _figures(lo, logits, mask, ref, lengths=None):
    B, K, T = mask.shape[0], mask.shape[1], mask.shape[2]
    items = [(b, k, T if lengths is None else lengths[b]) for b in range(B) for k in range(K)]
    table = {}
    if lo is not None:
        table["lstm_out"] = max(_rel(lo[b, k, :n], ref[b][k]["lstm_out"]) for b, k, n in items)
        table["lstm_tail_max"] = max([float(np.abs(lo[b, k, n:]).max()) for b, k, n in items if n < T] + [0.0])
    if logits is not None:
        table["logits"] = max(_rel(logits[b, k, :n], ref[b][k]["logits"]) for b, k, n in items)
    table["mask"] = max(_rel(mask[b, k, :n], ref[b][k]["mask"]) for b, k, n in items)
    table["mask_abs"] = max(float(np.abs(mask[b, k, :n] - ref[b][k]["mask"]).max()) for b, k, n in items)
    table["mask_mse"] = max(float(((mask[b, k, :n] - ref[b][k]["mask"]) ** 2).mean()) for b, k, n in items)
    table["tail_max"] = max([float(np.abs(mask[b, k, n:]).max()) for b, k, n in items if n < T] + [0.0])
    return table


def _judge(tag, math, act, table):
    print(f"multi parity {tag} {math} {act}: " + json.dumps(table, sort_keys=True))
    assert table["tail_max"] == 0.0 and table.get("lstm_tail_max", 0.0) == 0.0
    if math == "f16x3":
        assert table.get("lstm_out", 0.0) < REL_TOL and table.get("logits", 0.0) < REL_TOL, table
        assert table["mask"] < REL_TOL and table["mask_mse"] < MSE_TOL, table
    else:
        assert table.get("lstm_out", 0.0) < LSTM_TOL[act], table
        assert table["mask_abs"] < MASK_ABS_TOL[act] and table["mask_mse"] < 1e-4, table


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
@pytest.mark.parametrize("cls_name,act", MODELS)
def test_one_tile_and_k_does_not_divide_32(cls_name, act, math):
    """B=3, K=3, T=37: nine sequences in one 32-column tile, three columns per shared row; stage output and mask, both models."""
    dims_d, sd, x, dvecs = _case(3, 37, 3, 41)
    ref = _oracle("one_tile", sd, x, dvecs, act)
    _assert_speakers_differ(ref)
    with _math(math):
        lo, logits, mask = _stages(_model(cls_name, sd), sd, x, dvecs, act)
    assert np.isfinite(mask).all() and np.isfinite(lo).all()
    _judge("one_tile", math, act, _figures(lo, logits, mask, ref))


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_tiles_and_launches_split_inside_a_mixture(math):
    """B=5, K=13, T=12: 65 sequences = three 32-column tiles and, at H=400 on 256 CUs, a second launch.  Mixture 2's speakers
    (n = 26..38) straddle the first tile boundary; mixture 4's last speaker (n = 64) sits alone in the third tile."""
    dims_d, sd, x, dvecs = _case(5, 12, 13, 42)
    ref = _oracle("tiles", sd, x, dvecs, "mish", conv_once=True)
    _assert_speakers_differ(ref)
    with _math(math):
        lo, logits, mask = _stages(_model("VoiceSplit", sd), sd, x, dvecs, "mish")
    assert np.isfinite(mask).all() and np.isfinite(lo).all()
    _judge("tiles", math, "mish", _figures(lo, logits, mask, ref))


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_ragged_and_multi_together(math):
    """Lengths [37, 1, 20], K=2: every valid row against the oracle on the item alone at its own length, rows past the end exactly
    0 for both speakers, and NaN written into x's pad rows changes no bit."""
    lengths = [37, 1, 20]
    dims_d, sd, x, dvecs = _case(3, 37, 2, 43)
    ref = _oracle("ragged", sd, x, dvecs, "mish", lengths=lengths)
    _assert_speakers_differ(ref)
    m = _model("VoiceSplit", sd)
    with _math(math):
        lo, logits, mask = _stages(m, sd, x, dvecs, "mish", lengths=lengths)
        xn = x.clone()
        for b, n in enumerate(lengths):
            xn[b, n:] = float("nan")
        with torch.no_grad():
            mask_nan = m.forward_multi(xn.cuda(), dvecs.cuda(), lengths).cpu().numpy()
    assert np.isfinite(mask).all() and np.isfinite(lo).all()
    _judge("ragged", math, "mish", _figures(lo, logits, mask, ref, lengths))
    assert np.array_equal(mask, mask_nan)                 # bit-identical, NaN pads included
    for b, n in enumerate(lengths):
        assert not mask[b, :, n:].any() and not lo[b, :, n:].any()


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_long_form_sequence_stage_takes_k_dvectors(math):
    """``long_form_stages()``: sequence_stage(feat, dvec [B,K,E]) -> [B,K,T,fc2_dim] at B=1, K=2, T=40 against the oracle; the
    2-D form is what it was (same call as before, checked against the same oracle)."""
    dims_d, sd, x, dvecs = _case(1, 40, 2, 44)
    ref = _oracle("long_form", sd, x, dvecs, "mish")
    _assert_speakers_differ(ref)
    m = _model("VoiceSplit", sd)
    with _math(math), torch.no_grad():
        conv_stage, sequence_stage = m.long_form_stages()
        feat = conv_stage(x.cuda())
        mask = sequence_stage(feat, dvecs.cuda())
        single = sequence_stage(feat, dvecs[:, 1].cuda())
    assert tuple(mask.shape) == (1, 2, 40, dims_d["fc2_dim"]) and tuple(single.shape) == (1, 40, dims_d["fc2_dim"])
    _judge("long_form", math, "mish", _figures(None, None, mask.cpu().numpy(), ref))
    _judge("long_form_2d", math, "mish", _figures(None, None, single.cpu().numpy()[:, None], [[ref[0][1]]]))


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_k_equal_one_and_the_plain_forward(math):
    """K=1: ``forward_multi`` and ``model(x, emb)`` are both inside the bounds; their maximum difference is printed (bit identity is
    not required: the row bias is added by the recurrence here, by the input GEMM's epilogue there)."""
    dims_d, sd, x, dvecs = _case(2, 23, 1, 45)
    ref = _oracle("k1", sd, x, dvecs, "mish")
    m = _model("VoiceSplit", sd)
    with _math(math), torch.no_grad():
        multi = m.forward_multi(x.cuda(), dvecs.cuda())
        plain = m(x.cuda(), dvecs[:, 0].contiguous().cuda())
    assert tuple(multi.shape) == (2, 1, 23, dims_d["fc2_dim"])
    print(f"K = 1 ({math}): max |forward_multi - model(x, emb)| = {(multi[:, 0] - plain).abs().max().item():.3e}")
    _judge("k1_multi", math, "mish", _figures(None, None, multi.cpu().numpy(), ref))
    _judge("k1_plain", math, "mish", _figures(None, None, plain.cpu().numpy()[:, None], ref))


def test_refusals():
    """Error code + message through the Python surface; nothing is computed some other way."""
    from voicesplit_amd import _lib, ops
    from voicesplit_amd._lib import VoiceSplitHipError
    dims_d, sd, x, dvecs = _case(2, 9, 2, 46)
    m = _model("VoiceSplit", sd)
    xc, dc = x.cuda(), dvecs.cuda()
    with torch.no_grad():
        with _math("fp32"), pytest.raises(VoiceSplitHipError, match="VS_MATH_FP32"):
            m.forward_multi(xc, dc)
        with pytest.raises(ValueError, match="speaker_embeddings"):
            m.forward_multi(xc, dc[:1])
        with pytest.raises(ValueError, match="1 <= length"):
            m.forward_multi(xc, dc, [9, 0])
        assert torch.isfinite(m.forward_multi(xc, dc)).all()
    # a recurrence without the shared-input mode (per-step kernels, fp32 products, the flag kernel) refuses
    sdc = {k: v.cuda() for k, v in sd.items()}
    feat = torch.zeros(2, 9, 8 * dims_d["num_freq"], device="cuda")
    lib = _lib.load()
    for mode in (1, 3, 4):
        assert lib.vs_set_lstm_kernel(mode) == 0
        try:
            with pytest.raises(VoiceSplitHipError, match="shared-input"):
                ops.bilstm_multi(sdc, feat, dc, _dims(2, 9))
        finally:
            assert lib.vs_set_lstm_kernel(0) == 0
    assert torch.isfinite(ops.bilstm_multi(sdc, feat, dc, _dims(2, 9))).all()


def _istft_abs_bound(amp, hop=160, win=400):
    """Upper bound on |istft(D)[n]| over every D with |D| = amp [T, F] (oracle/reference_audio.py's istft with absolute values put
    through it): a frame's irfft is at most a[t] = (amp[t,0] + 2 sum amp[t,1:-1] + amp[t,-1]) / n_fft at any sample, the
    overlap-add weighs it with the padded window and divides by the overlap-added squared window."""
    T, F = amp.shape
    n_fft = 2 * (F - 1)
    w = RA._padded_hann(win, n_fft)
    a = (amp[:, 0] + 2.0 * amp[:, 1:-1].sum(axis=1) + amp[:, -1]) / n_fft
    y = np.zeros(n_fft + hop * (T - 1))
    wss = np.zeros_like(y)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += w * a[t]
        wss[t * hop:t * hop + n_fft] += w ** 2
    nz = wss > np.finfo(np.float64).tiny
    y[nz] /= wss[nz]
    return y[n_fft // 2:len(y) - n_fft // 2]


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_separate_speakers_rows_equal_separate(math):
    """``audio.separate_speakers`` on one demo mixture (its first second) with K=2: row k equals ``audio.separate`` with d-vector k.

    Tolerance = the mask tolerance of the arithmetic carried through the iSTFT, no new constant.  Both masks are within tol of
    the oracle's (f16x3: REL_TOL of max |mask| <= 1; bf16: MASK_ABS_TOL), so they differ by at most d = 2 tol per element, and so
    do the masked spectrograms (|spec| <= 1; the clip to [0, 1] is 1-Lipschitz).  utils/audio_processor.py:540-547 turns a
    normalised value v into the magnitude 10^(5 v - 4): the two magnitudes of a bin differ by at most a factor 10^(5 d), i.e. by
    at most g = 10^(5 d) - 1 of the plain route's magnitude.  The iSTFT is linear in the magnitudes at a given phase, so sample
    n differs by at most g times the iSTFT of absolute values (``_istft_abs_bound``) of the plain route's magnitudes.
    In bf16 g is about 3 -- the arithmetic's own latitude, too wide to tell the speakers apart -- so the order of the rows is
    asserted separately: row k is nearer to ``separate`` with d-vector k than with the other one."""
    import voicesplit_amd as V
    from voicesplit_amd import audio
    z = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    wav = torch.from_numpy(z["mixed"][0][:16000].astype(np.float32) / 32767.0)[None]
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, 7), 6.0)
    dvecs = _embeddings(1, 2, dims_d["emb_dim"], 47)
    m = _model("VoiceSplit", sd)
    acfg = V.default_config().audio["voicefilter"]
    spec, _ = audio.wav_to_spec(wav.cuda(), acfg)
    ref = _oracle("audio", sd, spec.cpu(), dvecs, "mish")
    _assert_speakers_differ(ref)
    with _math(math):
        est = audio.separate_speakers(m, wav.cuda(), dvecs.cuda(), acfg)
        plain = [audio.separate(m, wav.cuda(), dvecs[:, k].contiguous().cuda(), acfg) for k in range(2)]
        with torch.no_grad():
            masks = [m(spec, dvecs[:, k].contiguous().cuda())[0].cpu().double().numpy() for k in range(2)]
    assert tuple(est.shape) == (1, 2, 16000)
    d = 2.0 * (REL_TOL if math == "f16x3" else MASK_ABS_TOL["mish"])
    g = 10.0 ** (5.0 * d) - 1.0
    s = spec[0].cpu().double().numpy()
    for k in range(2):
        amp = np.power(10.0, 5.0 * np.clip(s * masks[k], 0.0, 1.0) - 4.0)
        bound = g * _istft_abs_bound(amp)
        diff = np.abs(est[0, k].cpu().double().numpy() - plain[k][0].cpu().double().numpy())
        other = np.abs(est[0, k].cpu().double().numpy() - plain[1 - k][0].cpu().double().numpy())
        print(f"separate_speakers row {k} ({math}): max |row - separate| {diff.max():.3e} (worst share of its bound {(diff / bound).max():.3e}, "
              f"g = {g:.3e}); max |row - separate with the other d-vector| {other.max():.3e}")
        assert (diff <= bound).all()
        assert diff.max() < other.max()
