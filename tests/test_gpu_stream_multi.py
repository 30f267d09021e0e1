"""GPU: several enrolled speakers streamed from one live mixture -- the carry x shared-input form of the tagged persistent recurrence
(csrc/lstm_fwd.hip, vs_bilstm_recurrent_carry_shared), the sequence stage built on it (vs_bilstm_fwd_carry_multi),
streaming.StreamingMasker and audio.StreamingSeparator with d-vectors [B, K, E], in both arithmetics.

Oracles are fp64: the explicit recurrence of tests/test_gpu_stream.py restated with ``xg[n // K] + rowbias[n]`` and an initial state
per column for the raw kernel; for the stages the oracle's conv stack once per mixture, its whole-stream BiLSTM per speaker for the
forward half, ``lstm_direction(reverse=True)`` over lstm_in[kC : min((k+1)C + R, T)] for the reverse half of chunk k, the oracle's
head on top.

No bound is new: KTOL and the bf16 envelope (tests/test_gpu_lstm16.py / test_gpu_stream.py) for the raw recurrence, ``_judge_stream``
of tests/test_gpu_stream.py (REL_TOL / MSE_TOL, LSTM_TOL / MASK_ABS_TOL / mask MSE < 1e-4) for stages and masks.  Every figure is
printed before it is asserted.  Each comparison is preceded by a precondition on the oracle alone which makes sure that a mix-up
of the speakers of a mixture could not pass it."""
import itertools

import pytest
import torch

from oracle import reference_forward as R
from test_gpu_multi import _assert_speakers_differ, _case, _head64
from test_gpu_stream import (AUDIO, KTOL, MASK_ABS_TOL, MATHS, REL_TOL, _judge, _judge_stream, _loop, _math, _wav, dev, rel_err)

pytestmark = pytest.mark.gpu


# ---- the raw carry x shared-input recurrence -----------------------------------------------------------------------------------
# (M, K, T, H).  (1, 1, 1, 400): the smallest case; (3, 3, 9, 24): nine columns in one tile, K does not divide 32, a half-empty last
# K chunk; (3, 11, 6, 40): N = 33, mixture 2 straddles the tile boundary, one column alone in the second tile; (2, 2, 12, 400): full
# width; (5, 13, 4, 400): N = 65, three tiles and, at 2 * H / 8 = 100 workgroups on 256 CUs, a second launch
RAW_SHAPES = [(1, 1, 1, 400), (3, 3, 9, 24), (3, 11, 6, 40), (2, 2, 12, 400), (5, 13, 4, 400)]
_RAW = {}


def _raw_case(M, K, T, H, scale=1.5):
    """Inputs and the fp64 references of one shape for every keep, computed once and shared (read-only)."""
    key = (M, K, T, H)
    if key not in _RAW:
        N = M * K
        g = torch.Generator().manual_seed(1000 * M + 100 * K + T + 7 * H)
        xg = torch.randn(M, T, 8 * H, generator=g)
        rowbias = torch.randn(N, 8 * H, generator=g)
        whh = [torch.randn(4 * H, H, generator=g) * (scale / H ** 0.5) for _ in range(2)]
        h0 = torch.rand(N, H, generator=g) * 2 - 1
        c0 = torch.rand(N, H, generator=g) * 6 - 3
        state = torch.stack((h0, c0), dim=1).contiguous()
        # what column n computes: the loop of tests/test_gpu_stream.py over xg[n // K] + rowbias[n]
        wide = xg.double().repeat_interleave(K, dim=0) + rowbias.double()[:, None, :]
        refs = {}
        for keep in sorted({1, T // 2 or 1, T}):
            refs[keep] = (_loop(wide, whh, state, keep, False), _loop(wide, whh, state, keep, True))
        _RAW[key] = dict(xg=xg, rowbias=rowbias, whh=whh, state=state, refs=refs)
    return _RAW[key]


def _assert_columns_differ(ref, K):
    """The precondition, on the fp64 loop alone: any two columns of one mixture differ by more than 1e-1 of the output's range --
    100 times the loosest bound below (1e-3) -- so a swap of k cannot pass."""
    N = ref.shape[0]
    span = ref.abs().max().item()
    worst = min([(ref[m * K + i] - ref[m * K + j]).abs().max().item() / span
                 for m in range(N // K) for i, j in itertools.combinations(range(K), 2)] + [float("inf")])
    print(f"  fp64 loop: smallest max |column i - column j| / max |out| inside one mixture {worst:.3e} (must exceed 1e-1)")
    assert worst > 1e-1
    return worst


@pytest.mark.parametrize("M,K,T,H", RAW_SHAPES)
def test_raw_precondition_columns_of_a_mixture_differ(M, K, T, H):
    """Needs no device; kept beside the comparison it guards (the module is marked gpu as a whole)."""
    c = _raw_case(M, K, T, H)
    for keep, ((ref, _), _) in c["refs"].items():
        _assert_columns_differ(ref, K)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("M,K,T,H", RAW_SHAPES)
def test_carry_shared_recurrence_matches_the_fp64_loop(M, K, T, H, math):
    from voicesplit_amd import ops
    c = _raw_case(M, K, T, H)
    d = dev()
    xg, rb, state = c["xg"].to(d), c["rowbias"].to(d), c["state"].to(d)
    w = (c["whh"][0].to(d), c["whh"][1].to(d))
    for keep, ((ref, ref_state), (rmod, rmod_state)) in c["refs"].items():
        print(f"M={M} K={K} N={M * K} T={T} H={H} {math} keep={keep}")
        _assert_columns_differ(ref, K)
        mod, mod_state = (rmod, rmod_state) if math == "bf16" else (ref, ref_state)
        out, state_out = ops.bilstm_recurrent_carry_shared(xg, rb, K, *w, math, state=state, keep=keep)
        assert out.shape == (M * K, T, 2 * H) and state_out.shape == (M * K, 2, H)
        assert torch.isfinite(out).all() and torch.isfinite(state_out).all()
        _judge(math, "forward half", out[..., :H], ref[..., :H], mod[..., :H])
        _judge(math, "reverse half", out[..., H:], ref[..., H:], mod[..., H:])
        _judge(math, "state_out h", state_out[:, 0], ref_state[:, 0], mod_state[:, 0])
        _judge(math, "state_out c", state_out[:, 1], ref_state[:, 1], mod_state[:, 1])
        # the state handed out is the recurrence's own row keep - 1
        assert torch.equal(state_out[:, 0], out[:, keep - 1, :H])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("M,K,T,H", [(3, 11, 6, 40), (2, 2, 12, 400)])
def test_two_carried_calls_give_the_forward_half_of_one(M, K, T, H, math):
    """[0, a) then [a, T), the second call's state_in ALIASED to the first's state_out: the forward half of one call, bit for bit,
    in every column."""
    from voicesplit_amd import ops
    c = _raw_case(M, K, T, H)
    d = dev()
    xg, rb = c["xg"], c["rowbias"].to(d)
    w = (c["whh"][0].to(d), c["whh"][1].to(d))
    whole, whole_state = ops.bilstm_recurrent_carry_shared(xg.to(d), rb, K, *w, math, state=c["state"].to(d), keep=T)
    for a in (1, T - 1):
        buf = c["state"].to(d).clone()
        first, mid = ops.bilstm_recurrent_carry_shared(xg[:, :a].contiguous().to(d), rb, K, *w, math, state=buf, keep=a, state_out=buf)
        assert mid.data_ptr() == buf.data_ptr()
        second, last = ops.bilstm_recurrent_carry_shared(xg[:, a:].contiguous().to(d), rb, K, *w, math, state=buf, keep=T - a, state_out=buf)
        got = torch.cat((first[..., :H], second[..., :H]), dim=1)
        diff = (got - whole[..., :H]).abs().max().item()
        sdiff = (last - whole_state).abs().max().item()
        print(f"M={M} K={K} T={T} H={H} {math} a={a}: max |two calls - one call| forward half {diff:.3e}, final state {sdiff:.3e} (0.0 expected)")
        assert torch.equal(got, whole[..., :H]) and torch.equal(last, whole_state)


# ---- the stages at full width -------------------------------------------------------------------------------------------------
B_S, K_S, T_S, C_S, R_S, SEED = 2, 3, 100, 16, 8, 41
_FULL = {}


def _full(cls_name):
    """Model, inputs and fp64 references of one class, computed once and shared (read-only): tests/test_gpu_multi.py's ``_case``
    (d-vectors of norm EMB_GAIN = 8), conv stack once per mixture, forward half of the whole stream and chunked reverse half per
    speaker."""
    if cls_name not in _FULL:
        import voicesplit_amd as V
        act = "mish" if cls_name == "VoiceSplit" else "relu"
        dims_d, sd, x, dvecs = _case(B_S, T_S, K_S, SEED)
        sd64 = R.cast_state_dict(sd, torch.float64)
        H, T, C, Rl = dims_d["lstm_dim"], T_S, C_S, R_S
        rw = [sd64[f"lstm.{n}_l0_reverse"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        fwd, rev, whole = [], [], []
        with torch.no_grad():
            for b in range(B_S):
                y = R.conv_stack(x[b:b + 1].double(), sd64, act).transpose(1, 2).contiguous().view(1, T, -1)
                for k in range(K_S):
                    lstm_in = torch.cat((y, dvecs[b, k].double().view(1, 1, -1).repeat(1, T, 1)), dim=2)
                    lo = R.bilstm(lstm_in, sd64)
                    fwd.append(lo[0, :, :H])
                    whole.append(_head64(sd64, lo)[1][0])
                    rev.append(torch.cat([R.lstm_direction(lstm_in[:, j * C:min((j + 1) * C + Rl, T)], *rw, True)[0, :min(C, T - j * C)]
                                          for j in range(-(-T // C))], dim=0))
            shape = (B_S, K_S, T)
            fwd, rev, whole = (torch.stack(v).view(*shape, -1) for v in (fwd, rev, whole))
            logits, mask = _head64(sd64, torch.cat((fwd, rev), dim=3))
        m = getattr(V, cls_name)(V.default_config()).eval()
        m.load_state_dict(sd)
        _FULL[cls_name] = dict(model=m.cuda(), x=x, dvecs=dvecs, H=H, fwd=fwd, rev=rev, logits=logits, mask=mask, whole_mask=whole)
    return _FULL[cls_name]


def _assert_streamed_speakers_differ(f):
    """``_assert_speakers_differ`` of tests/test_gpu_multi.py on the chunked oracle, whole stream; per 16-frame chunk printed."""
    rows = [[{"mask": f["mask"][b, k].numpy()} for k in range(K_S)] for b in range(B_S)]
    _assert_speakers_differ(rows)
    per_chunk = min(float(((f["mask"][b, i, lo:lo + C_S] - f["mask"][b, j, lo:lo + C_S]) ** 2).mean())
                    for b in range(B_S) for i, j in itertools.combinations(range(K_S), 2) for lo in range(0, T_S, C_S))
    print(f"oracle: smallest mask MSE between two speakers of one mixture within one {C_S}-frame chunk {per_chunk:.3e}")
    assert per_chunk > 1e-3


def _run_stream(model, x, dvecs, C, Rl, sizes, want_logits=True):
    from voicesplit_amd.streaming import StreamingMasker
    masker = StreamingMasker(*model.stream_stages(want_logits=want_logits), dvecs.cuda(), C, Rl, trace=True)
    outs, pos, i, log = [], 0, 0, []
    while pos < x.shape[1]:
        n = min(sizes[i % len(sizes)], x.shape[1] - pos)
        outs.append(masker.push(x[:, pos:pos + n].cuda()))
        pos, i = pos + n, i + 1
        log.append((pos, masker.emitted))
    outs.append(masker.finish())
    assert all(o.dim() == 4 and o.shape[:2] == dvecs.shape[:2] for o in outs)
    lstm = torch.cat([c["lstm_out"] for c in masker.trace], dim=2).cpu()
    logits = torch.cat([c["logits"] for c in masker.trace], dim=2).cpu() if want_logits else None
    return torch.cat(outs, dim=2).cpu(), lstm, logits, log, masker


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cls_name", ["VoiceSplit", "VoiceFilter"])
def test_streamed_stages_match_the_oracle_on_every_frame(cls_name, math):
    """B = 2, K = 3, T = 100, C = 16, R = 8 at full width, every frame of every speaker.  Uneven pushes: chunk 0 is due at frame 89 in
    mid-stream, the rest at finish(); one push of everything gives the same masks bit for bit."""
    f = _full(cls_name)
    _assert_streamed_speakers_differ(f)
    with _math(math):
        uneven = _run_stream(f["model"], f["x"], f["dvecs"], C_S, R_S, (7, 30, 1, 19))
        once = _run_stream(f["model"], f["x"], f["dvecs"], C_S, R_S, (T_S,))
    print(f"{cls_name}")
    for tag, (mask, lstm, logits, log, masker) in (("uneven pushes", uneven), ("all at once", once)):
        assert mask.shape == (B_S, K_S, T_S, 601) and torch.isfinite(mask).all()
        assert masker._state.shape == (B_S * K_S, 2, f["H"])
        _judge_stream(math, tag, mask, lstm, logits, f)
    both = (uneven[0] - once[0]).abs().max().item()
    print(f"  uneven pushes vs all at once: max |mask difference| {both:.3e} (0.0 expected)")
    assert both == 0.0
    # emission: chunk k is out with the push that brings the stream to (k + 1) C + R + 65 frames
    for pushed, emitted in uneven[3]:
        assert emitted == C_S * max(0, (pushed - R_S - 65) // C_S), (pushed, emitted)
    assert any(0 < emitted < T_S for _, emitted in uneven[3])           # chunk 0 left in mid-stream
    assert uneven[4].latency_frames == C_S + R_S + 65


@pytest.mark.parametrize("math", MATHS)
def test_zero_state_stage_is_the_multi_speaker_stage(math):
    """ops.bilstm_carry_multi(state = None, keep = T) against ops.bilstm_multi, full width, B = 3, K = 3, T = 12: bit for bit."""
    from voicesplit_amd import ops
    dims_d, sd, x, dvecs = _case(3, 12, 3, SEED)
    sdc = {k: v.cuda() for k, v in sd.items()}
    with _math(math):
        dims = ops.make_dims(3, 12, dims_d["num_freq"], dims_d["emb_dim"], dims_d["lstm_dim"], dims_d["fc1_dim"], dims_d["fc2_dim"])
        feat = ops.conv_stack(sdc, x.cuda(), dims, "mish")
        plain = ops.bilstm_multi(sdc, feat, dvecs.cuda(), dims)
        for state in (None, torch.zeros(9, 2, dims.H, device=dev())):
            out, state_out = ops.bilstm_carry_multi(sdc, feat, dvecs.cuda(), dims, state, 12)
            diff = (out - plain).abs().max().item()
            print(f"{math} state={'None' if state is None else 'zeros'}: max |carry_multi - bilstm_multi| = {diff:.3e} (0.0 expected)")
            assert out.shape == (3, 3, 12, 2 * dims.H) and state_out.shape == (9, 2, dims.H)
            assert torch.equal(out, plain)
            assert torch.equal(state_out[:, 0], out.view(9, 12, -1)[:, 11, :dims.H])
    # the speakers are told apart at this shape too
    assert min((plain[b, i] - plain[b, j]).abs().max().item() for b in range(3) for i, j in itertools.combinations(range(3), 2)) \
        > 1e-1 * plain.abs().max().item()


@pytest.mark.parametrize("math", MATHS)
def test_one_chunk_with_the_whole_stream_is_forward_multi(math):
    """C + R >= T: the streamed masks against model.forward_multi(x, dvecs), within the arithmetic's mask bound; whether the difference
    is exactly 0.0 is printed (DESIGN.md 6.8d-2 records it)."""
    f = _full("VoiceSplit")
    _assert_streamed_speakers_differ(f)
    with _math(math), torch.no_grad():
        whole = f["model"].forward_multi(f["x"].cuda(), f["dvecs"].cuda()).cpu()
        mask, _, _, _, _ = _run_stream(f["model"], f["x"], f["dvecs"], 70, 30, (7, 64, 1), want_logits=False)
    rel, ab = rel_err(mask, whole), (mask - whole).abs().max().item()
    mse = ((mask.double() - f["whole_mask"]) ** 2).mean().item()
    print(f"{math}: streamed (C = 70, R = 30) vs forward_multi(): rel {rel:.3e} abs {ab:.3e} (exactly 0.0: {ab == 0.0}); "
          f"MSE vs the whole-stream oracle {mse:.3e}")
    if math == "f16x3":
        assert rel < REL_TOL and mse < 1e-4
    else:
        assert ab < MASK_ABS_TOL and mse < 1e-4


# ---- audio ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", MATHS)
def test_streaming_separator_equals_the_whole_clip_synthesis_per_speaker(math):
    """2 s synthetic mixture, dvec [2, 3, E], C = 16, R = 8: the concatenated [B, K, n] output against spec_to_wav of the whole clip's
    spectrogram and phase repeated per speaker with the streamed masks (difference 0.0), for uneven and hop-sized pushes; every
    block after the first starts latency_samples behind the newest sample."""
    from voicesplit_amd import audio
    f = _full("VoiceSplit")
    hop, S, C, Rl = 160, 32000, 16, 8
    wav = _wav(B_S, S, 4).cuda()
    with _math(math):
        spec, phase = audio.wav_to_spec(wav, AUDIO)
        Tn, F = spec.shape[1], spec.shape[2]

        def per_speaker(t):
            return t[:, None].expand(B_S, K_S, Tn, F).reshape(B_S * K_S, Tn, F).contiguous()

        for tag, sizes in (("uneven pushes", (3, 40, 1, 17, 9)), ("hop-sized pushes", (1,))):
            sep = audio.StreamingSeparator(f["model"], f["dvecs"].cuda(), AUDIO, C, Rl, trace=True)
            assert sep.latency_samples == (C + Rl + 65 + 2 * 4) * hop
            outs, pos, i, worst, at_emission = [], 0, 0, 0, set()
            while pos < S:
                n = min(sizes[i % len(sizes)] * hop, S - pos)
                returned = sum(o.shape[2] for o in outs)
                out = sep.push(wav[:, pos:pos + n].contiguous())
                assert out.dim() == 3 and out.shape[:2] == (B_S, K_S)
                pos, i = pos + n, i + 1
                if out.shape[2] and returned:
                    at_emission.add(pos - returned)                      # behind the newest sample when a block leaves
                outs.append(out)
                worst = max(worst, pos - returned - out.shape[2])        # still withheld when the push returns
            outs.append(sep.finish())
            got = torch.cat(outs, dim=2)
            masks = torch.cat(sep.mask_trace, dim=2)
            assert got.shape == (B_S, K_S, S) and masks.shape == (B_S, K_S, Tn, F)
            ref = audio.spec_to_wav(per_speaker(spec), per_speaker(phase), AUDIO, mask=masks.reshape(B_S * K_S, Tn, F).contiguous())
            ref = ref.view(B_S, K_S, S)
            diff = (got - ref).abs().max().item()
            apart = min((ref[b, a] - ref[b, c]).abs().max().item() for b in range(B_S) for a, c in itertools.combinations(range(K_S), 2))
            print(f"{math} {tag}: max |streamed - whole-clip synthesis| = {diff:.3e} (0.0 expected; max |whole| {ref.abs().max().item():.3e}, "
                  f"two speakers of a mixture differ by at least {apart:.3e}); a block starts {sorted(at_emission)} samples behind the "
                  f"newest one, at most {worst} stay withheld behind a push, reported latency {sep.latency_samples}")
            assert apart > 1e-3 * ref.abs().max().item()                 # the speakers' waveforms are told apart
            assert diff == 0.0
            assert worst < sep.latency_samples
            if sizes == (1,):          # hop by hop: every block after the first starts exactly latency_samples behind the newest sample
                assert at_emission == {sep.latency_samples} and worst == sep.latency_samples - hop


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_carry_shared_is_refused_where_no_kernel_serves_it():
    from voicesplit_amd import _lib, ops
    c = _raw_case(3, 3, 9, 24)
    d = dev()
    lib = _lib.load()
    args = (c["xg"].to(d), c["rowbias"].to(d), 3, c["whh"][0].to(d), c["whh"][1].to(d))
    with pytest.raises(_lib.VoiceSplitHipError, match="VS_MATH_FP32"):
        ops.bilstm_recurrent_carry_shared(*args, "fp32", state=c["state"].to(d))
    with pytest.raises(_lib.VoiceSplitHipError, match="keep=10"):
        ops.bilstm_recurrent_carry_shared(*args, "f16x3", state=c["state"].to(d), keep=10)
    g = torch.Generator().manual_seed(3)
    H = 456
    wide = (torch.randn(1, 2, 8 * H, generator=g).to(d), torch.randn(2, 8 * H, generator=g).to(d), 2,
            (torch.randn(4 * H, H, generator=g) * 0.05).to(d), (torch.randn(4 * H, H, generator=g) * 0.05).to(d))
    with pytest.raises(_lib.VoiceSplitHipError, match="H <= 448"):
        ops.bilstm_recurrent_carry_shared(*wide, "f16x3", state=torch.zeros(2, 2, H, device=d))
    for mode in (1, 3, 4):
        try:
            assert lib.vs_set_lstm_kernel(mode) == 0
            with pytest.raises(_lib.VoiceSplitHipError, match="vs_set_lstm_kernel"):
                ops.bilstm_recurrent_carry_shared(*args, "f16x3", state=c["state"].to(d))
        finally:
            lib.vs_set_lstm_kernel(0)
    # the Python layer: a state that is not [B*K, 2, H]
    with pytest.raises(ValueError, match="state must be"):
        ops.bilstm_recurrent_carry_shared(*args, "f16x3", state=c["state"][:3].to(d))
