"""CPU: several enrolled speakers streamed from one mixture -- the host side.  ``streaming.StreamingMasker`` with d-vectors
[B, K, E] against K single-speaker maskers (stand-in stages in fp64 built from row-independent, element-wise operations, so a call
over B*K rows equals the per-row calls bit for bit), its shape errors, and the two new C entry points' exports and no-device
refusals (vs_bilstm_recurrent_carry_shared, vs_bilstm_fwd_carry_multi)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

B, K, T, F, E, H = 2, 3, 50, 6, 8, 6
HALO = 2


def _stages(log=None):
    """Stand-ins with the stages' contracts.  conv: frame t from frames t - 1 .. t + 1 (zero padded at the window's ends, so a window
    must give every kept frame its halo).  carry: a leaky recurrence whose input gain and offset come from the d-vector, forward from
    ``state``, reverse from zero.  head: a gate over both halves.  Element-wise throughout: no reduction whose order could depend
    on the batch, and + - * / alone (correctly rounded whatever the vector width; a library tanh need not be the same function on
    a tensor's vector body and on its scalar tail)."""
    def squash(v):
        return v / (1.0 + v.abs())

    def conv_stage(xw):
        p = torch.nn.functional.pad(xw, (0, 0, 1, 1))
        return squash(xw) + 0.5 * p[:, :-2] + 0.25 * p[:, 2:]

    def rows(feat, d, state, keep):
        gain, off = 1.0 + 0.1 * d[:, :H], 0.3 * d[:, E - H:]
        n = feat.shape[1]
        h = state[:, 0] if state is not None else feat.new_zeros(feat.shape[0], H)
        c = state[:, 1] if state is not None else feat.new_zeros(feat.shape[0], H)
        fwd, handed = [], None
        for t in range(n):
            c = 0.9 * c + gain * feat[:, t] + 0.05 * h
            h = squash(c + off)
            fwd.append(h)
            if t == keep - 1:
                handed = torch.stack((h, c), dim=1)
        rc, rev = feat.new_zeros(feat.shape[0], H), [None] * n
        for t in range(n - 1, -1, -1):
            rc = 0.8 * rc + gain * feat[:, t]
            rev[t] = squash(rc - off)
        return torch.cat((torch.stack(fwd, 1), torch.stack(rev, 1)), dim=2), handed

    def carry_stage(feat, dvec, state, keep):
        if log is not None:
            log.append((tuple(feat.shape), tuple(dvec.shape), None if state is None else tuple(state.shape), keep))
        if dvec.dim() == 3:
            b, k, n = dvec.shape[0], dvec.shape[1], feat.shape[1]
            wide = feat[:, None].expand(b, k, n, feat.shape[2]).reshape(b * k, n, -1)
            out, st = rows(wide, dvec.reshape(b * k, -1), state, keep)
            return out.view(b, k, n, -1), st
        return rows(feat, dvec, state, keep)

    def head_stage(lstm_out):
        logits = 3.0 * lstm_out[..., :H] - 2.0 * lstm_out[..., H:]
        return 0.5 + 0.5 * squash(logits), logits

    return conv_stage, carry_stage, head_stage


def _inputs():
    g = torch.Generator().manual_seed(11)
    return torch.randn(B, T, F, generator=g, dtype=torch.float64), torch.randn(B, K, E, generator=g, dtype=torch.float64)


def _run(masker, x, sizes, tdim):
    outs, pos, i = [], 0, 0
    while pos < x.shape[1]:
        n = min(sizes[i % len(sizes)], x.shape[1] - pos)
        outs.append(masker.push(x[:, pos:pos + n]))
        pos, i = pos + n, i + 1
    outs.append(masker.finish())
    return torch.cat(outs, dim=tdim), outs


@pytest.mark.parametrize("sizes", [(1,), (3, 1, 17, 2), (1000,)], ids=["one frame at a time", "uneven", "all at once"])
def test_k_speaker_masker_is_k_single_speaker_maskers(sizes):
    from voicesplit_amd.streaming import StreamingMasker
    x, dvecs = _inputs()
    C, R = 5, 3
    log = []
    multi = StreamingMasker(*_stages(log), dvecs, C, R, halo=HALO, trace=True)
    got, pieces = _run(multi, x, sizes, 2)
    assert got.shape == (B, K, T, H)
    assert all(p.dim() == 4 and p.shape[:2] == (B, K) and p.shape[2] % C == 0 for p in pieces[:-1])      # empty pieces carry the K axis too
    assert multi._state.shape == (B * K, 2, H)
    # the stage saw the features once per mixture, the 3-D d-vectors, and from the second chunk on a state per sequence
    assert all(f[0] == B and d == (B, K, E) for f, d, _, _ in log)
    assert log[0][2] is None and all(s == (B * K, 2, H) for _, _, s, _ in log[1:])
    assert all(c["lstm_out"].shape[:2] == (B, K) and c["logits"].shape[:2] == (B, K) for c in multi.trace)
    assert multi.latency_frames == C + R + HALO
    for k in range(K):
        single = StreamingMasker(*_stages(), dvecs[:, k], C, R, halo=HALO, trace=True)
        ref, _ = _run(single, x, sizes, 1)
        assert ref.shape == (B, T, H)                                   # a 2-D d-vector: no K axis, as before
        diff = (got[:, k] - ref).abs().max().item()
        print(f"speaker {k}: max |K-speaker masker - single masker| = {diff:.3e} (0.0 expected)")
        assert torch.equal(got[:, k], ref)
        assert torch.equal(multi._state.view(B, K, 2, H)[:, k], single._state)
        assert single.latency_frames == multi.latency_frames and single.emitted == multi.emitted
        lstm = torch.cat([c["lstm_out"] for c in multi.trace], dim=2)
        assert torch.equal(lstm[:, k], torch.cat([c["lstm_out"] for c in single.trace], dim=1))
    # the speakers are told apart: no slice equals another
    assert all((got[:, a] - got[:, b]).abs().max().item() > 1e-2 for a in range(K) for b in range(a))


def test_shape_errors():
    from voicesplit_amd.streaming import StreamingMasker
    x, dvecs = _inputs()
    with pytest.raises(ValueError, match=r"\[B, K, E\]"):
        StreamingMasker(*_stages(), dvecs[:, :0], 5, 3, halo=HALO)              # K = 0
    with pytest.raises(ValueError, match="dvec must be"):
        StreamingMasker(*_stages(), dvecs[0, 0], 5, 3, halo=HALO)
    masker = StreamingMasker(*_stages(), dvecs, 5, 3, halo=HALO)
    with pytest.raises(ValueError, match="frames must be"):
        masker.push(torch.cat((x, x[:1]), dim=0)[:, :4])                        # B = 3 frames for B = 2 d-vectors
    with pytest.raises(ValueError, match="frames must be"):
        masker.push(x[:1, :4])


def test_audio_shape_checks_need_no_device():
    from voicesplit_amd import audio
    assert callable(audio.StreamingSeparator.with_reference)
    with pytest.raises(ValueError, match="lists of reference waveforms"):
        audio._embed_references(None, [[torch.zeros(10)]], 2, {})
    with pytest.raises(ValueError, match="same number K >= 1"):
        audio._embed_references(None, [[torch.zeros(10)], []], 2, {})


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
EXPORTS = {"vs_bilstm_recurrent_carry_shared": 14, "vs_bilstm_fwd_carry_multi": 12}


def test_header_library_and_ctypes_table_agree_on_the_new_entry_points():
    from voicesplit_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in EXPORTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == nargs and restype is _lib.c_int, name
        for want in (r"const float\s*\*\s*state_in", r"float\s*\*\s*state_out", r"int\s+keep", r"int\s+K"):
            assert any(re.fullmatch(want, a) for a in args), (name, want)
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.vs_abi_version() == _lib.ABI_VERSION
    assert callable(ops.bilstm_recurrent_carry_shared) and callable(ops.bilstm_carry_multi)


def _raw(lib, keep=3, T=5, H=24, math=1, state_out=256, K=2, N=4, dvecs=256):
    return lib.vs_bilstm_recurrent_carry_shared(256, dvecs, K, 256, 256, 256, None, state_out, keep, N, T, H, math, None)


def _stage(lib, keep=3, T=5, H=24, math="f16x3", state_out=256, K=2, N=None, dvecs=256):
    from voicesplit_amd import ops
    d = ops.make_dims(2, T, 37, 16, H, 40, 37, math=math)
    return lib.vs_bilstm_fwd_carry_multi(ctypes.byref(d), None, 256, dvecs, K, None, state_out, keep, None, 0, 256, None)


@pytest.mark.parametrize("call", [_raw, _stage], ids=list(EXPORTS))
def test_argument_errors_are_codes_and_messages(call):
    """Before any launch (this host has no device): each refusal is a non-zero code with its own message."""
    from voicesplit_amd import _lib
    lib = _lib.load()
    for keep in (0, 6, -1):
        assert call(lib, keep=keep) != 0 and b"keep=" in lib.vs_last_error() and b"1 <= keep <= T = 5" in lib.vs_last_error()
    assert call(lib, math=0 if call is _raw else "fp32") != 0 and b"VS_MATH_FP32" in lib.vs_last_error()
    assert call(lib, H=456) != 0 and b"H=456" in lib.vs_last_error() and b"H <= 448" in lib.vs_last_error()
    assert call(lib, state_out=None) != 0 and b"state_out is NULL" in lib.vs_last_error()
    for k in (0, -2):
        assert call(lib, K=k) != 0 and b"K=%d" % k in lib.vs_last_error()
    if call is _raw:
        assert call(lib, K=3, N=4) != 0 and b"not a multiple of K=3" in lib.vs_last_error()
        assert call(lib, dvecs=None) != 0 and b"NULL argument" in lib.vs_last_error()
    else:
        assert call(lib, dvecs=None) != 0 and b"dvecs is NULL" in lib.vs_last_error()
        assert call(lib) != 0 and b"workspace is NULL" in lib.vs_last_error()          # every argument check passed
    for mode in (1, 3, 4):
        try:
            assert lib.vs_set_lstm_kernel(mode) == 0
            assert call(lib) != 0 and b"vs_set_lstm_kernel" in lib.vs_last_error()
        finally:
            lib.vs_set_lstm_kernel(0)


def test_python_wrappers_check_the_state_and_have_no_cpu_fallback():
    from voicesplit_amd import _lib, ops
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        ops.bilstm_recurrent_carry_shared(torch.zeros(1, 2, 64), torch.zeros(2, 64), 2, torch.zeros(32, 8), torch.zeros(32, 8), "f16x3")
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        ops.bilstm_carry_multi({}, torch.zeros(1, 2, 64), torch.zeros(1, 2, 16), ops.make_dims(1, 2, 8, 16, 8, 8, 8, "f16x3"))


def test_carry_refusal_no_longer_says_one_speaker_per_mixture():
    """The message of the refusals that remain (carry with per-item lengths, a recurrence other than the tagged one)."""
    src = open(os.path.join(ROOT, "voicesplit_amd", "csrc", "lstm_fwd.hip")).read()
    claim = re.search(r"kCarryOnly\{(.*?)\};", src, flags=re.S).group(1)
    assert "no lengths" in claim and "one speaker per mixture" not in claim
