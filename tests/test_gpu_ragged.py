"""GPU: clips of unequal length in one eval batch, each as if alone (``model.forward_ragged``, vs_forward_prepared_ragged).

Ground truth is the fp64 oracle on every item AT ITS OWN LENGTH; every row of every item is compared.  Bounds: the fp32-class
arithmetic is held to the project's contract (REL_TOL / MSE_TOL of tests/test_gpu_forward.py), VS_MATH_BF16 to the eval bounds
tests/test_gpu_bf16.py states for the same quantities (FEAT_TOL, LSTM_TOL, MASK_ABS_TOL, mask MSE < 1e-4; it states none for
logits, which are therefore printed, not asserted, in that arithmetic).  Every figure is printed before it is asserted."""
import json
import os
import random

import numpy as np
import pytest
import torch

import bss_eval_ref as BSS
from conftest import GOLDEN_DIR
from oracle import reference_audio as RA
from oracle import reference_forward as R
from oracle import reference_loss as RL
from test_gpu_bf16 import FEAT_TOL, LSTM_TOL, MASK_ABS_TOL, _math
from test_gpu_forward import MSE_TOL, REL_TOL

pytestmark = pytest.mark.gpu
MODELS = [("VoiceSplit", "mish"), ("VoiceFilter", "relu")]
LENGTHS_A = [131, 5, 301, 64, 1, 257, 33, 173]                 # [301, 257, 173, 131, 64, 33, 5, 1] shuffled; Tmax = 301
_rng = random.Random(11)
# more than one 32-column batch tile of the persistent recurrence, lengths from the demo clips' range (531..1142 frames) under Tmax = 700:
# dilation-16 tails of up to 169 rows
LENGTHS_B = [700] + [_rng.randint(531, 700) for _ in range(32)]
_ORACLE = {}


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _case(lengths, seed):
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, seed), 6.0)          # randomised BatchNorm statistics, spread logits
    x, dvec = R.synthetic_inputs(len(lengths), max(lengths), dims_d, seed)
    return dims_d, sd, x, dvec


def _oracle(tag, sd, x, dvec, lengths, act):
    """Per item at its own length, fp64: lstm_in[:8F], lstm_out, logits, mask (cached: both arithmetics compare against it)."""
    key = (tag, act)
    if key not in _ORACLE:
        sd64 = R.cast_state_dict(sd, torch.float64)
        out = []
        with torch.no_grad():
            for b, n in enumerate(lengths):
                o = R.forward(sd64, x[b:b + 1, :n].double(), dvec[b:b + 1].double(), act=act, lstm_impl="loop")
                out.append({k: o[k][0].numpy() for k in ("lstm_in", "lstm_out", "logits", "mask")})
        _ORACLE[key] = out
    return _ORACLE[key]


def _model(cls_name, sd):
    import voicesplit_amd as V
    m = getattr(V, cls_name)(V.default_config())
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _stages(m, sd, x, dvec, lengths, act):
    """features, LSTM output, logits and mask of the padded batch through the ragged stage entry points and forward_ragged."""
    from voicesplit_amd import ops
    sdc = {k: v.cuda() for k, v in sd.items()}
    d = R.default_dims()
    dims = ops.make_dims(x.shape[0], x.shape[1], d["num_freq"], d["emb_dim"], d["lstm_dim"], d["fc1_dim"], d["fc2_dim"])
    xc, dc = x.cuda(), dvec.cuda()
    feat = ops.conv_stack(sdc, xc, dims, act, lengths=lengths)
    lo = ops.bilstm(sdc, feat, dc, dims, lengths=lengths)
    _, logits = ops.head(sdc, lo, dims, want_logits=True)
    with torch.no_grad():
        mask = m.forward_ragged(xc, dc, lengths)
    torch.cuda.synchronize()
    return feat.cpu().numpy(), lo.cpu().numpy(), logits.cpu().numpy(), mask.cpu().numpy()


def _compare(tag, math, act, got, ref, lengths):
    feat, lo, logits, mask = got
    F8 = feat.shape[2]
    table = {}
    for name, g, key in (("feat", feat, "lstm_in"), ("lstm_out", lo, "lstm_out"), ("logits", logits, "logits"), ("mask", mask, "mask")):
        table[name] = max(_rel(g[b, :n], ref[b][key][:, :F8] if key == "lstm_in" else ref[b][key]) for b, n in enumerate(lengths))
    table["mask_abs"] = max(float(np.abs(mask[b, :n] - ref[b]["mask"]).max()) for b, n in enumerate(lengths))
    table["mask_mse"] = max(float(((mask[b, :n] - ref[b]["mask"]) ** 2).mean()) for b, n in enumerate(lengths))
    table["tail_max"] = max([float(np.abs(mask[b, n:]).max()) for b, n in enumerate(lengths) if n < mask.shape[1]] + [0.0])
    table["lstm_tail_max"] = max([float(np.abs(lo[b, n:]).max()) for b, n in enumerate(lengths) if n < lo.shape[1]] + [0.0])
    print(f"ragged parity {tag} {math} {act}: " + json.dumps(table, sort_keys=True))
    assert np.isfinite(mask).all() and np.isfinite(lo).all()
    assert table["tail_max"] == 0.0 and table["lstm_tail_max"] == 0.0
    if math == "f16x3":
        assert table["feat"] < REL_TOL and table["lstm_out"] < REL_TOL, table            # stage parity
        assert table["logits"] < REL_TOL and table["mask"] < REL_TOL and table["mask_mse"] < MSE_TOL, table
    else:
        assert table["feat"] < FEAT_TOL and table["lstm_out"] < LSTM_TOL[act], table
        assert table["mask_abs"] < MASK_ABS_TOL[act] and table["mask_mse"] < 1e-4, table


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
@pytest.mark.parametrize("cls_name,act", MODELS)
def test_every_item_matches_the_fp64_oracle_at_its_own_length(cls_name, act, math):
    """Full width, Tmax = 301, lengths from 1 frame to the whole batch: every stage, every row of every item; rows behind an item's
    end are exactly 0 in the LSTM output and in the mask."""
    dims_d, sd, x, dvec = _case(LENGTHS_A, 31)
    ref = _oracle("a", sd, x, dvec, LENGTHS_A, act)
    with _math(math):
        got = _stages(_model(cls_name, sd), sd, x, dvec, LENGTHS_A, act)
    _compare("a", math, act, got, ref, LENGTHS_A)


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_two_batch_tiles_and_long_tails(math):
    """33 items (two 32-column tiles of the persistent recurrence), Tmax = 700, lengths 531..700: dilation-16 tails."""
    dims_d, sd, x, dvec = _case(LENGTHS_B, 32)
    ref = _oracle("b", sd, x, dvec, LENGTHS_B, "mish")
    with _math(math):
        got = _stages(_model("VoiceSplit", sd), sd, x, dvec, LENGTHS_B, "mish")
    _compare("b", math, "mish", got, ref, LENGTHS_B)


def test_the_padded_batch_through_the_plain_forward_is_wrong_and_forward_ragged_is_right():
    """What the feature is for.  The same zero-padded batch through ``model(x, emb)``: the last 65 valid rows of a short item sit
    inside the conv stack's reach of the pad (and its reverse LSTM state starts in the pad), so they differ from the item alone
    by more than the tolerance; ``forward_ragged`` is within it."""
    lengths = LENGTHS_A
    dims_d, sd, x, dvec = _case(lengths, 31)
    ref = _oracle("a", sd, x, dvec, lengths, "mish")
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
    m = _model("VoiceSplit", sd)
    b = lengths.index(173)
    with torch.no_grad():
        plain = m(x.cuda(), dvec.cuda()).cpu().numpy()
        ragged = m.forward_ragged(x.cuda(), dvec.cuda(), lengths).cpu().numpy()
    want = ref[b]["mask"]
    lo, hi = 173 - 65, 173
    err_plain, err_ragged = _rel(plain[b, lo:hi], want[lo:hi]), _rel(ragged[b, lo:hi], want[lo:hi])
    print(f"last 65 valid rows of the 173-frame item: plain padded forward {err_plain:.3e}, forward_ragged {err_ragged:.3e}")
    assert err_plain > REL_TOL
    assert err_ragged < REL_TOL


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_pad_content_does_not_matter(math):
    lengths = LENGTHS_A
    dims_d, sd, x, dvec = _case(lengths, 31)
    m = _model("VoiceSplit", sd)
    outs = []
    with _math(math), torch.no_grad():
        for fill in (0.0, float("nan"), 1e3):
            xp = x.clone()
            for b, n in enumerate(lengths):
                xp[b, n:] = fill
            outs.append(m.forward_ragged(xp.cuda(), dvec.cuda(), torch.tensor(lengths)))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])          # bit-identical, NaN pads included
    for b, n in enumerate(lengths):
        assert not outs[1][b, n:].any()                                               # rows >= len: exactly 0
        assert outs[1][b, :n].min() >= 0 and outs[1][b, :n].max() <= 1


@pytest.mark.parametrize("math", ["f16x3", "bf16"])
def test_lengths_all_equal_to_tmax(math):
    """No tails: the same kernels as ``model(x, emb)`` plus a copy of x and sweeps that find nothing to do -- bit-equal to it
    (DESIGN.md 6.8b states this as a property), and within tolerance of the oracle."""
    B, T = 3, 45
    dims_d, sd, x, dvec = _case([T] * B, 33)
    m = _model("VoiceSplit", sd)
    with torch.no_grad():
        ref = R.forward(R.cast_state_dict(sd, torch.float64), x.double(), dvec.double(), act="mish", lstm_impl="loop")["mask"].numpy()
        with _math(math):
            ragged = m.forward_ragged(x.cuda(), dvec.cuda(), [T] * B)
            plain = m(x.cuda(), dvec.cuda())
    print(f"lengths == Tmax ({math}): max |forward_ragged - model(x, emb)| = {(ragged - plain).abs().max().item():.3e}")
    assert torch.equal(ragged, plain)
    got = ragged.cpu().numpy()
    if math == "f16x3":
        assert _rel(got, ref) < REL_TOL and ((got - ref) ** 2).mean() < MSE_TOL
    else:
        assert np.abs(got - ref).max() < MASK_ABS_TOL["mish"] and ((got - ref) ** 2).mean() < 1e-4


def test_zero_tail_rows_kernel_on_rows_that_are_no_multiple_of_16_bytes():
    from voicesplit_amd import ops
    g = torch.Generator().manual_seed(5)
    for shape, lengths in (((5, 7, 601), [7, 1, 3, 6, 2]), ((3, 4, 1), [1, 4, 2]), ((2, 9, 64, 64), [4, 9])):
        t = torch.rand(*shape, generator=g) + 1.0
        want = t.clone()
        for b, n in enumerate(lengths):
            want[b, n:] = 0.0
        assert torch.equal(ops.zero_tail_rows(t.cuda(), lengths).cpu(), want), shape
    h = (torch.rand(4, 6, 37, 64, generator=g) + 1.0).to(torch.bfloat16)
    want = h.clone()
    want[0, 2:], want[1, 5:], want[3, 1:] = 0, 0, 0
    assert torch.equal(ops.zero_tail_rows(h.cuda(), [2, 5, 6, 1]).cpu(), want)


def test_refusals():
    from voicesplit_amd._lib import VoiceSplitHipError
    lengths = [9, 4]
    dims_d, sd, x, dvec = _case(lengths, 34)
    m = _model("VoiceSplit", sd)
    xc, dc = x.cuda(), dvec.cuda()
    with torch.no_grad():
        with pytest.raises(ValueError, match="1 <= length"):
            m.forward_ragged(xc, dc, [9, 0])
        with pytest.raises(ValueError, match="1 <= length"):
            m.forward_ragged(xc, dc, [10, 4])
        with _math("fp32"), pytest.raises(VoiceSplitHipError, match="VS_MATH_FP32"):
            m.forward_ragged(xc, dc, lengths)
        assert torch.isfinite(m.forward_ragged(xc, dc, lengths)).all()
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_ragged(xc, dc, lengths)
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval mode"):
        m.forward_ragged(xc, dc, lengths)
    # a recurrence that does not take lengths (here: the per-step kernels) refuses; it is never run on the padded batch instead
    from voicesplit_amd import _lib, ops
    d = R.default_dims()
    dims = ops.make_dims(2, 9, d["num_freq"], d["emb_dim"], d["lstm_dim"], d["fc1_dim"], d["fc2_dim"])
    sdc = {k: v.cuda() for k, v in sd.items()}
    feat = torch.zeros(2, 9, 8 * d["num_freq"], device="cuda")
    lib = _lib.load()
    for mode in (1, 3, 4):
        assert lib.vs_set_lstm_kernel(mode) == 0
        try:
            with pytest.raises(VoiceSplitHipError, match="per-item lengths"):
                ops.bilstm(sdc, feat, dc, dims, lengths=lengths)
        finally:
            assert lib.vs_set_lstm_kernel(0) == 0
    assert torch.isfinite(ops.bilstm(sdc, feat, dc, dims, lengths=lengths)).all()


def _demo_clips():
    z = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    return z["target"].astype(np.float32) / 32767.0, z["mixed"].astype(np.float32) / 32767.0


def test_separate_many_on_demo_clips_of_unequal_length():
    """Three demo mixtures cropped to 3 s, 2 s and 2.5 s.  Per clip, with the bounds of tests/test_gpu_audio.py: the mask the
    ragged batch gave it against the fp64 oracle on the ORACLE's spectrogram of that clip alone (end to end: MSE < 1e-4, 99.9 %
    of the values within 1e-2), and the returned waveform against the oracle's iSTFT of the same masked spectrogram (2e-5)."""
    import voicesplit_amd as V
    from voicesplit_amd import audio
    _, mixed = _demo_clips()
    crops = [48000, 32000, 40000]
    dims_d = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims_d, 7), 6.0)
    m = _model("VoiceSplit", sd)
    acfg = V.default_config().audio["voicefilter"]
    dvec = R.synthetic_inputs(3, 8, dims_d, 7)[1]
    wavs = [torch.from_numpy(mixed[i][:n].copy()).cuda() for i, n in enumerate(crops)]
    est = audio.separate_many(m, wavs, dvec.cuda(), acfg)
    specs = [audio.wav_to_spec(w[None], acfg) for w in wavs]
    masks = audio.masks_ragged(m, [s[0][0] for s in specs], dvec.cuda())
    sd64 = R.cast_state_dict(sd, torch.float64)
    for i, n in enumerate(crops):
        assert est[i].shape == (n,)
        spec_ref, _ = RA.wav2spec(mixed[i][:n].astype(np.float64))
        with torch.no_grad():
            ref = R.forward(sd64, torch.from_numpy(spec_ref)[None], dvec[i:i + 1].double(), act="mish", lstm_impl="loop")["mask"][0].numpy()
        got = masks[i].cpu().double().numpy()
        mse, q = float(((got - ref) ** 2).mean()), float(np.quantile(np.abs(got - ref), 0.999))
        spec, phase = (t[0].cpu().double().numpy() for t in specs[i])
        want = RA.spec2wav(spec * got, phase)
        werr = float(np.abs(est[i].cpu().double().numpy() - want).max() / np.abs(want).max())
        print(f"separate_many clip {i} ({n} samples): mask mse {mse:.3e}, q99.9 {q:.3e}, waveform rel {werr:.3e}")
        assert mse < 1e-4 and q < 1e-2
        assert werr <= 2e-5


def test_evaluate_ragged_scores_every_item_at_its_own_length(tmp_path, capsys):
    """``python -m voicesplit_amd.evaluate --ragged`` on four items of 3 / 2 / 2.5 / 3 s, batch_size 4, against per-item values:
    the fp64 oracle forward on each item's spectrogram alone, oracle/reference_loss.py for the loss and tests/bss_eval_ref.py
    for the SDR of oracle/reference_audio.py's waveform.  Bounds: the loss 2e-4 relative (tests/test_gpu_loss.py's bound for
    this criterion against the same oracle); the SDR restated on the GPU's OWN per-item estimates 1e-6 dB (tests/test_gpu_evaluate.py,
    tests/test_gpu_sdr.py); the SDR of the oracle's estimate 5e-3 dB: a relative waveform error e moves 10 log10(|s|^2 / |n|^2) by at
    most (20 / ln 10) e sqrt(1 + |s|^2 / |n|^2) -- 8.7 e x 3.3 at 10 dB -- and e is 1e-4 (mask) + 2e-5 (iSTFT) by the bounds above,
    i.e. 3.5e-3 dB."""
    import voicesplit_amd as V
    from test_gpu_evaluate import _small_cfg, _write_dataset
    from voicesplit_amd import audio, evaluate
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg("voicesplit", "si_snr")
    data = tmp_path / "test"
    data.mkdir()
    lengths = [48000, 32000, 40000, 48000]
    _write_dataset(str(data), lengths)
    c.dataset = {"train_dir": str(data), "test_dir": str(data),
                 "format": {"emb": "*-emb.pt", "mixed": "*-mixed.pt", "target": "*-target.pt",
                            "target_wav": "*-target.wav", "mixed_wav": "*-mixed.wav"}}
    c["test_config"] = {"batch_size": 4, "num_workers": 1}
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({k: (dict(v) if isinstance(v, dict) else v) for k, v in c.items()}, indent=1))
    torch.manual_seed(1)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    ck = tmp_path / "checkpoint_1.pt"
    tr.save_checkpoint(str(ck))
    args = ["-c", str(cfg), "-d", str(data), "--checkpoint_path", str(ck)]
    with pytest.raises(ValueError, match="must share a length"):                   # without the flag nothing changes
        evaluate.main(args)
    mean_loss, mean_sdr = evaluate.main(args + ["--ragged"])
    assert f"Mean Test SDR: {mean_sdr}" in capsys.readouterr().out
    # per item, alone
    acfg = c.audio[c.audio["backend"]]
    ds = evaluate.EvalDataset(c, str(data))
    sd64 = R.cast_state_dict({k: v.detach().cpu() for k, v in tr.model.state_dict().items()}, torch.float64)
    tr.model.eval()
    losses, sdr_oracle = [], []
    kw = dict(n_fft=acfg["n_fft"], hop_length=acfg["hop_length"], win_length=acfg["win_length"])
    for i in range(len(ds)):
        emb, tw, mw, _ = ds[i]
        mixed, phase = audio.wav_to_spec(mw.cuda()[None], acfg)
        target, _ = audio.wav_to_spec(tw.cuda()[None], acfg, want_phase=False)
        with torch.no_grad():
            ref = R.forward(sd64, mixed.cpu().double(), emb.double().reshape(1, -1), act="mish", lstm_impl="loop")["mask"]
        loss, _ = RL.training_loss(ref, mixed.cpu().double(), target.cpu().double(), phase.cpu().double(), torch.tensor([mw.shape[0]]), **kw)
        losses.append(float(loss))
        est_ref = RA.spec2wav((mixed[0].cpu().double() * ref[0]).numpy(), phase[0].cpu().double().numpy())
        sdr_oracle.append(float(BSS.sdr_rows(tw.numpy()[None].astype(np.float64), est_ref[None])[0][0]))
    # the restatement applied to the GPU's own per-item estimates (the same ragged batches)
    sdr_own = []
    with torch.no_grad():
        for emb, _t, mixed, _s, tws, phase, frames in evaluate.eval_batches(c, ds, "cuda", ragged=True):
            mask = tr.model.forward_ragged(mixed, emb, frames)
            for b, n in enumerate(frames):
                est = audio.spec_to_wav(mixed[b:b + 1, :n], phase[b:b + 1, :n], acfg, mask=mask[b:b + 1, :n]).cpu().numpy()
                sdr_own.append(float(BSS.sdr_rows(tws[b].numpy()[None], est)[0][0]))
    assert len(sdr_own) == 4
    print(f"evaluate --ragged: loss {mean_loss} vs per-item oracle {np.mean(losses)}; SDR {mean_sdr} vs own {np.mean(sdr_own)} / oracle {np.mean(sdr_oracle)}")
    assert abs(mean_loss - np.mean(losses)) < 2e-4 * max(1.0, abs(np.mean(losses)))
    assert abs(mean_sdr - np.mean(sdr_own)) <= 1e-6
    assert abs(mean_sdr - np.mean(sdr_oracle)) <= 5e-3
