"""CPU: the host side of stream separation chunk by chunk (streaming.plan_stream / StreamingMasker, the two carry entries of
the C ABI, the module surface).  The masker is run with fp64 oracle stages at a reduced width: what it must compute is defined
by the whole-stream oracle (conv features, forward LSTM half) and by the chunked definition of the reverse half
(``lstm_direction(reverse=True)`` over lstm_in[kC : min((k+1)C + R, T)])."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from oracle import reference_forward as R

HALO = 65


def _pushes(T, sizes):
    """T frames in pieces that cycle through `sizes`."""
    out, i = [], 0
    while sum(out) < T:
        out.append(min(sizes[i % len(sizes)], T - sum(out)))
        i += 1
    return out


@pytest.mark.parametrize("T,C,R", [(1, 16, 8), (15, 16, 8), (200, 16, 8), (200, 1, 0), (200, 50, 32), (301, 100, 32), (97, 7, 40),
                                   (131, 16, 0), (400, 300, 200)])
@pytest.mark.parametrize("sizes", [(1,), (3, 1, 40, 7), (1000,)])
def test_plan_stream_properties(T, C, R, sizes):
    from voicesplit_amd.streaming import CONV_RECEPTIVE_HALO, plan_stream
    assert CONV_RECEPTIVE_HALO == HALO
    pushed = feat_done = chunks_done = 0
    spans, emitted_at = [], {}
    steps = [(n, False) for n in _pushes(T, sizes)] + [(0, True)]
    for n, fin in steps:
        pushed += n
        plan = plan_stream(pushed, fin, C, R, HALO, feat_done, chunks_done)
        if plan.feat_hi > plan.feat_lo:
            assert plan.feat_lo == feat_done                                           # no feature frame is finalised twice
            assert 0 <= plan.win_lo <= plan.feat_lo and plan.feat_hi <= plan.win_hi <= pushed      # the window lies inside the stream
            assert plan.win_lo == 0 or plan.feat_lo - plan.win_lo >= HALO              # halo at every edge that is not a stream edge
            assert (fin and plan.win_hi == pushed) or plan.win_hi - plan.feat_hi >= HALO
            spans.append((plan.feat_lo, plan.feat_hi))
            feat_done = plan.feat_hi
        else:
            assert plan.feat_lo == plan.feat_hi == feat_done
        for k, lo, hi, e in plan.chunks:
            assert k == chunks_done and lo == k * C and hi == min((k + 1) * C, T if fin else hi)
            assert e == (min((k + 1) * C + R, T) if fin else (k + 1) * C + R) and e <= feat_done
            emitted_at[k] = (pushed, fin)
            chunks_done += 1
    # kept feature spans tile [0, T), chunks tile [0, T)
    assert spans[0][0] == 0 and spans[-1][1] == T and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert chunks_done == -(-T // C)
    # chunk k is out at exactly (k + 1) C + R + 65 pushed frames (the first push that reaches it), or at finish()
    counts = [0]
    for n, _ in steps[:-1]:
        counts.append(counts[-1] + n)
    for k, (at, fin) in emitted_at.items():
        due = (k + 1) * C + R + HALO
        if due <= T:
            assert not fin and at == min(c for c in counts if c >= due), (k, at, due)
        else:
            assert fin and at == T, (k, at, due)


def test_plan_stream_rejects_bad_arguments():
    from voicesplit_amd.streaming import plan_stream
    for bad in ((10, False, 0, 8), (10, False, 16, -1)):
        with pytest.raises(ValueError, match="plan_stream"):
            plan_stream(*bad)
    with pytest.raises(ValueError, match="inconsistent"):
        plan_stream(10, False, 16, 8, HALO, feat_done=11)


# ---- StreamingMasker with fp64 oracle stages ---------------------------------------------------------------------------
DIMS = dict(num_freq=13, emb_dim=8, lstm_dim=16, fc1_dim=20, fc2_dim=13)
_CACHE = {}


def _oracle():
    if not _CACHE:
        sd = R.cast_state_dict(R.spread_logits(R.build_state_dict(DIMS, 5), 6.0), torch.float64)
        x, dvec = R.synthetic_inputs(2, 200, DIMS, 5, dtype=torch.float64)
        with torch.no_grad():
            ref = R.forward(sd, x, dvec, act="mish", lstm_impl="loop")
        _CACHE.update(sd=sd, x=x, dvec=dvec, ref=ref)
    return _CACHE["sd"], _CACHE["x"], _CACHE["dvec"], _CACHE["ref"]


def _forward_direction_from(xs, sd, state):
    """nn.LSTM's forward direction from a given (h, c): the fp64 loop of oracle.lstm_direction with an initial state."""
    H = DIMS["lstm_dim"]
    w_ih, w_hh = sd["lstm.weight_ih_l0"], sd["lstm.weight_hh_l0"]
    xg = xs @ w_ih.t() + (sd["lstm.bias_ih_l0"] + sd["lstm.bias_hh_l0"])
    h, c = (state[:, 0], state[:, 1]) if state is not None else (xs.new_zeros(xs.shape[0], H), xs.new_zeros(xs.shape[0], H))
    out, states = [], []
    for t in range(xs.shape[1]):
        i, f, g, o = (xg[:, t] + h @ w_hh.t()).split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
        states.append(torch.stack((h, c), dim=1))
    return torch.stack(out, dim=1), states


def _reverse(xs, sd):
    return R.lstm_direction(xs, sd["lstm.weight_ih_l0_reverse"], sd["lstm.weight_hh_l0_reverse"], sd["lstm.bias_ih_l0_reverse"],
                            sd["lstm.bias_hh_l0_reverse"], True)


def _oracle_stages(sd, calls=None):
    def conv_stage(xw):
        y = R.conv_stack(xw, sd, "mish").transpose(1, 2).contiguous()
        if calls is not None:
            calls.append(xw.shape[1])
        return y.view(y.size(0), y.size(1), -1)

    def carry_stage(feat, dvec, state, keep):
        xs = torch.cat((feat, dvec.unsqueeze(1).repeat(1, feat.size(1), 1)), dim=2)
        fwd, states = _forward_direction_from(xs, sd, state)
        return torch.cat((fwd, _reverse(xs, sd)), dim=2), states[keep - 1]

    def head_stage(lstm_out):
        y = torch.relu(torch.nn.functional.linear(torch.relu(lstm_out), sd["fc1.weight"], sd["fc1.bias"]))
        logits = torch.nn.functional.linear(y, sd["fc2.weight"], sd["fc2.bias"])
        return torch.sigmoid(logits), logits

    return conv_stage, carry_stage, head_stage


def _stream(masker, x, sizes):
    outs, pos, log = [], 0, []
    for n in _pushes(x.shape[1], sizes):
        outs.append(masker.push(x[:, pos:pos + n]))
        pos += n
        log.append((pos, masker.emitted))
    outs.append(masker.finish())
    return torch.cat(outs, dim=1), log


@pytest.mark.parametrize("sizes", [(5, 1, 33, 2, 90), (1,), (200,)])
def test_masker_equals_the_whole_stream_oracle_and_the_chunked_definition(sizes):
    from voicesplit_amd.streaming import StreamingMasker
    sd, x, dvec, ref = _oracle()
    T, C, Rl, H = 200, 16, 8, DIMS["lstm_dim"]
    calls = []
    masker = StreamingMasker(*_oracle_stages(sd, calls), dvec, C, Rl, trace=True)
    assert masker.latency_frames == C + Rl + HALO
    mask, log = _stream(masker, x, sizes)
    assert mask.shape == (2, T, DIMS["fc2_dim"])
    lstm = torch.cat([c["lstm_out"] for c in masker.trace], dim=1)
    logits = torch.cat([c["logits"] for c in masker.trace], dim=1)
    fwd_err = (lstm[..., :H] - ref["lstm_out"][..., :H]).abs().max().item()
    # the chunked definition, from the WHOLE-stream lstm_in (so the conv windows are checked too)
    want_rev = torch.cat([_reverse(ref["lstm_in"][:, k * C:min((k + 1) * C + Rl, T)], sd)[:, :min(C, T - k * C)]
                          for k in range(-(-T // C))], dim=1)
    rev_err = (lstm[..., H:] - want_rev).abs().max().item()
    want = torch.cat((ref["lstm_out"][..., :H], want_rev), dim=2)
    y = torch.relu(torch.nn.functional.linear(torch.relu(want), sd["fc1.weight"], sd["fc1.bias"]))
    want_logits = torch.nn.functional.linear(y, sd["fc2.weight"], sd["fc2.bias"])
    head_err = max((logits - want_logits).abs().max().item(), (mask - torch.sigmoid(want_logits)).abs().max().item())
    print(f"forward half {fwd_err:.2e}  reverse half {rev_err:.2e}  logits / mask {head_err:.2e}  conv windows {calls}")
    assert fwd_err < 1e-12 and rev_err < 1e-12 and head_err < 1e-11
    # the reverse half is NOT the whole-stream one (the look-ahead is 8 frames): the chunked definition is a different function
    assert (want_rev - ref["lstm_out"][..., H:]).abs().max().item() > 1e-3
    # emission: after every push exactly the chunks whose (k + 1) C + R + 65 frames have arrived are out
    for pushed, emitted in log:
        assert emitted == C * max(0, (pushed - Rl - HALO) // C), (pushed, emitted)
        assert pushed - emitted < masker.latency_frames or emitted == 0
    # every feature frame once: the kept spans add up to T, each conv window adds at most its halos
    assert sum(calls) <= T + 2 * HALO * len(calls)


def test_masker_with_the_whole_stream_in_one_chunk_is_the_plain_forward():
    from voicesplit_amd.streaming import StreamingMasker
    sd, x, dvec, ref = _oracle()
    for C, Rl in ((200, 0), (120, 80), (16, 184)):
        masker = StreamingMasker(*_oracle_stages(sd), dvec, C, Rl, trace=True)
        mask, _ = _stream(masker, x, (37, 1, 64))
        err = (mask - ref["mask"]).abs().max().item()
        lerr = (torch.cat([c["lstm_out"] for c in masker.trace], dim=1) - ref["lstm_out"]).abs().max().item()
        print(f"C = {C}, R = {Rl}: mask {err:.2e}  lstm_out {lerr:.2e}")
        assert err < 1e-12 and lerr < 1e-12


def test_a_stream_shorter_than_one_chunk_comes_out_at_finish():
    from voicesplit_amd.streaming import StreamingMasker
    sd, x, dvec, _ = _oracle()
    with torch.no_grad():
        ref = R.forward(sd, x[:, :11], dvec, act="mish", lstm_impl="loop")["mask"]
    masker = StreamingMasker(*_oracle_stages(sd), dvec, 16, 8)
    a = masker.push(x[:, :4])
    b = masker.push(x[:, 4:11])
    assert a.shape == (2, 0, DIMS["num_freq"]) and b.shape[1] == 0
    out = masker.finish()
    err = (out - ref).abs().max().item()
    print(f"11-frame stream at finish(): {err:.2e}")
    assert out.shape == ref.shape and err < 1e-12
    with pytest.raises(RuntimeError, match="finished"):
        masker.push(x[:, :1])
    with pytest.raises(RuntimeError, match="never received"):
        StreamingMasker(*_oracle_stages(sd), dvec, 16, 8).finish()


# ---- C ABI and module surface -----------------------------------------------------------------------------------------
CARRY_EXPORTS = {"vs_bilstm_recurrent_carry": 12, "vs_bilstm_fwd_carry": 11}


def test_header_library_and_ctypes_table_agree_on_the_carry_entry_points():
    from voicesplit_amd import _lib
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, nargs in CARRY_EXPORTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == nargs and restype is _lib.c_int, name
        for want in (r"const float\s*\*\s*state_in", r"float\s*\*\s*state_out", r"int\s+keep"):
            assert any(re.fullmatch(want, a) for a in args), (name, want)
        assert hasattr(lib, name)
    assert lib.vs_abi_version() == 11                       # additive entries under the same ABI number


def _raw(lib, keep=3, T=5, H=24, math=1, state_out=256):
    return lib.vs_bilstm_recurrent_carry(256, 256, 256, 256, None, state_out, keep, 2, T, H, math, None)


def _stage(lib, keep=3, T=5, H=24, math="f16x3", state_out=256):
    from voicesplit_amd import ops
    d = ops.make_dims(2, T, 37, 16, H, 40, 37, math=math)
    return lib.vs_bilstm_fwd_carry(ctypes.byref(d), None, 256, 256, None, state_out, keep, None, 0, 256, None)


@pytest.mark.parametrize("call", [_raw, _stage], ids=["vs_bilstm_recurrent_carry", "vs_bilstm_fwd_carry"])
def test_carry_argument_errors_are_codes_and_messages(call):
    """Before any launch (this host has no device): each refusal is a non-zero code with its own message."""
    from voicesplit_amd import _lib
    lib = _lib.load()
    for keep in (0, 6, -1):
        assert call(lib, keep=keep) != 0 and b"keep=" in lib.vs_last_error() and b"1 <= keep <= T = 5" in lib.vs_last_error()
    fp32 = 0 if call is _raw else "fp32"
    assert call(lib, math=fp32) != 0 and b"VS_MATH_FP32 has no carry recurrence" in lib.vs_last_error()
    assert call(lib, H=456) != 0 and b"H=456" in lib.vs_last_error() and b"H <= 448" in lib.vs_last_error()
    assert call(lib, state_out=None) != 0 and b"state_out is NULL" in lib.vs_last_error()
    for mode in (1, 3, 4):
        try:
            assert lib.vs_set_lstm_kernel(mode) == 0
            assert call(lib) != 0 and b"vs_set_lstm_kernel" in lib.vs_last_error()
        finally:
            lib.vs_set_lstm_kernel(0)


def test_module_surface_and_train_mode_refusal():
    import inspect
    import voicesplit_amd as V
    from voicesplit_amd import audio, ops, streaming
    assert callable(ops.bilstm_recurrent_carry) and callable(ops.bilstm_carry)
    assert list(inspect.signature(streaming.plan_stream).parameters)[:5] == ["pushed", "finished", "C", "R", "halo"]
    assert {"push", "finish"} <= set(dir(streaming.StreamingMasker)) and {"push", "finish", "latency_samples"} <= set(dir(audio.StreamingSeparator))
    for cls in (V.VoiceSplit, V.VoiceFilter):
        m = cls(V.default_config(13, 8, 16, 20, 13))
        with pytest.raises(RuntimeError, match="eval mode"):
            m.train().stream_stages()
        assert len(m.eval().stream_stages()) == 3
    with pytest.raises(_lib_error(), match="no CPU fallback"):
        ops.bilstm_recurrent_carry(torch.zeros(1, 2, 64), torch.zeros(32, 8), torch.zeros(32, 8), "f16x3")


def _lib_error():
    from voicesplit_amd import _lib
    return _lib.VoiceSplitHipError


# ---- audio.StreamingSeparator's host arithmetic, with fp64 transforms standing in for the two device legs ------------------------
class _FrameModel:
    """stream_stages() of a mask that depends on the frame alone, so the streamed masks are the whole clip's whatever the chunks."""

    def stream_stages(self):
        return (lambda x: x, lambda feat, dvec, state, keep: (torch.cat((feat, feat), dim=2), state),
                lambda lstm_out: torch.sigmoid(4.0 * lstm_out[..., :lstm_out.shape[2] // 2] - 2.0))


def _fp64_legs(monkeypatch):
    """audio.wav_to_spec / spec_to_wav answered by oracle.reference_audio per clip, with the library's refusal of a segment that
    is not longer than the reflect padding; returns the list of segment lengths the separator asked for."""
    import numpy as np
    from oracle import reference_audio as RA
    from voicesplit_amd import audio
    asked = []

    def wav_to_spec(wav, cfg, want_phase=True):
        n_fft, hop, win = int(cfg["n_fft"]), int(cfg["hop_length"]), int(cfg["win_length"])
        asked.append(wav.shape[1])
        if wav.shape[1] <= n_fft // 2:
            raise _lib_error()("vs_wav_to_spec failed (rc=-1): wav_to_spec: clip shorter than the reflect padding")
        out = [RA.wav2spec(w.numpy(), n_fft, hop, win) for w in wav.double()]
        return (torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1] for o in out])))

    def spec_to_wav(spec, phase, cfg, mask=None):
        v = spec if mask is None else spec * mask
        return torch.from_numpy(np.stack([RA.spec2wav(s.numpy(), p.numpy(), int(cfg["hop_length"]), int(cfg["win_length"]))
                                          for s, p in zip(v, phase)]))

    monkeypatch.setattr(audio, "wav_to_spec", wav_to_spec)
    monkeypatch.setattr(audio, "spec_to_wav", spec_to_wav)
    return asked


@pytest.mark.parametrize("n_fft,hop,win", [(1200, 160, 400), (64, 16, 64), (256, 64, 255), (64, 11, 64), (64, 32, 64), (402, 100, 200)])
@pytest.mark.parametrize("sizes", [(1,), (2, 40, 1, 17, 9), (1, 1, 3, 200)])
def test_separator_glue_returns_the_whole_clip_synthesis_at_every_geometry(monkeypatch, n_fft, hop, win, sizes):
    """Where hop divides n_fft / 2 (64 / 16, 256 / 64, 64 / 32) ``margin`` hops are exactly as long as the reflect padding: the
    separator must not hand such a segment to wav_to_spec, neither at the start of the stream nor at finish().  In fp64 the streamed
    output is the whole-clip synthesis with the streamed masks to rounding, every pushed sample comes back, and nothing stays
    withheld longer than latency_samples."""
    from voicesplit_amd import audio
    asked = _fp64_legs(monkeypatch)
    cfg = {"n_fft": n_fft, "hop_length": hop, "win_length": win, "min_level_db": -100.0, "ref_level_db": 20.0}
    C, Rl, hops = 4, 2, 110
    S = hops * hop
    g = torch.Generator().manual_seed(n_fft + hop)
    wav = 0.1 * torch.randn(2, S, generator=g, dtype=torch.float64)
    spec, phase = audio.wav_to_spec(wav, cfg)
    sep = audio.StreamingSeparator(_FrameModel(), torch.zeros(2, 4), cfg, C, Rl, trace=True)
    assert sep.latency_samples == (C + Rl + 65 + 2 * -(-(n_fft // 2) // hop)) * hop
    del asked[:]
    outs, pos, i, worst, at_emission = [], 0, 0, 0, set()
    while pos < S:
        n = min(sizes[i % len(sizes)] * hop, S - pos)
        returned = sum(o.shape[1] for o in outs)
        out = sep.push(wav[:, pos:pos + n].contiguous())
        pos, i = pos + n, i + 1
        if out.shape[1] and returned:
            at_emission.add(pos - returned)
        outs.append(out)
        worst = max(worst, pos - returned - out.shape[1])
    outs.append(sep.finish())
    got, masks = torch.cat(outs, dim=1), torch.cat(sep.mask_trace, dim=1)
    assert got.shape == (2, S) and masks.shape == spec.shape
    assert (masks - torch.sigmoid(4.0 * spec - 2.0)).abs().max().item() < 1e-12      # every frame analysed exactly: the whole clip's spectrogram
    ref = audio.spec_to_wav(spec, phase, cfg, mask=masks)
    assert ((got - ref).abs().max() / ref.abs().max()).item() < 1e-12
    assert asked and min(asked) > n_fft // 2 and worst < sep.latency_samples
    if sizes == (1,):
        assert at_emission == {sep.latency_samples} and worst == sep.latency_samples - hop


def test_separator_glue_on_a_stream_no_longer_than_the_reflect_padding(monkeypatch):
    from voicesplit_amd import audio
    asked = _fp64_legs(monkeypatch)
    cfg = {"n_fft": 64, "hop_length": 16, "win_length": 64, "min_level_db": -100.0, "ref_level_db": 20.0}
    sep = audio.StreamingSeparator(_FrameModel(), torch.zeros(1, 4), cfg, 4, 2)
    for _ in range(2):
        assert sep.push(torch.zeros(1, 16, dtype=torch.float64)).shape == (1, 0)
    assert asked == []                                                     # 32 samples pending: nothing to transform yet
    with pytest.raises(_lib_error(), match="reflect padding"):
        sep.finish()
