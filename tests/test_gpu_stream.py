"""GPU: stream separation chunk by chunk -- the carry mode of the tagged persistent recurrence (csrc/lstm_fwd.hip), the sequence stage
built on it, streaming.StreamingMasker on the HIP stages and audio.StreamingSeparator, in both arithmetics.

Oracles are fp64: an explicit recurrence with an initial state for the raw kernel; ``oracle.reference_forward.forward`` of the
WHOLE stream for the conv features and the forward LSTM half; ``lstm_direction(reverse=True)`` over lstm_in[kC : min((k+1)C + R, T)]
for the reverse half of chunk k (the chunked definition), with the oracle's head on top for logits and mask.

Bounds are the project's own: KTOL and the bf16 envelope of tests/test_gpu_lstm16.py for the raw recurrence, REL_TOL / MSE_TOL
(tests/test_gpu_forward.py) for f16x3 stages and masks, LSTM_TOL / MASK_ABS_TOL / mask MSE < 1e-4 (tests/test_gpu_bf16.py) for bf16
stages and masks (that file names no bound for bf16 logits: they are printed, the mask they give is asserted), 2e-5 of the
waveform's range for the iSTFT leg (tests/test_gpu_audio.py).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from oracle import reference_forward as R

pytestmark = pytest.mark.gpu

KTOL = 3e-5                 # tests/test_gpu_lstm16.py
REL_TOL = 1e-4              # tests/test_gpu_forward.py
MSE_TOL = 1e-4
LSTM_TOL = 8e-2             # tests/test_gpu_bf16.py (mish and relu)
MASK_ABS_TOL = 6e-2
WAV_TOL = 2e-5              # tests/test_gpu_audio.py, vs_spec_to_wav leg
MATHS = ["f16x3", "bf16"]
AUDIO = {"n_fft": 1200, "hop_length": 160, "win_length": 400, "min_level_db": -100.0, "ref_level_db": 20.0}


def dev():
    return torch.device("cuda:0")


def rel_err(got, ref):
    ref = ref.detach().to(torch.float64).cpu()
    got = got.detach().to(torch.float64).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


class _math:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from voicesplit_amd import ops
        self.prev = ops.get_conv_math()
        ops.set_conv_math(self.name)

    def __exit__(self, *exc):
        from voicesplit_amd import ops
        ops.set_conv_math(self.prev)


# ---- the raw carry recurrence ------------------------------------------------------------------------------------------
def _f16(t):
    return t.to(torch.float16).to(t.dtype)


def _loop(xg, whh, state, keep, rounded):
    """nn.LSTM's recurrence in fp64 over precomputed gate inputs: the forward direction from ``state`` [B, 2, H] (h, c), the reverse
    one from zero.  rounded: h and W_hh to f16 in front of the recurrent product (the VS_MATH_BF16 kernel's roundings).
    -> (out [B, T, 2H], state of the forward direction behind frame keep - 1)."""
    B, T, H8 = xg.shape
    H = H8 // 8
    xg = xg.double()
    outs, handed = [], None
    for dirn in range(2):
        W = whh[dirn].double()
        W = _f16(W) if rounded else W
        h = state[:, 0].double() if dirn == 0 else torch.zeros(B, H, dtype=torch.float64)
        c = state[:, 1].double() if dirn == 0 else torch.zeros(B, H, dtype=torch.float64)
        out = [None] * T
        for t in (range(T - 1, -1, -1) if dirn else range(T)):
            pre = xg[:, t, dirn * 4 * H:(dirn + 1) * 4 * H] + (_f16(h) if rounded else h) @ W.t()
            i, f, g, o = pre.split(H, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[t] = h
            if dirn == 0 and t == keep - 1:
                handed = torch.stack((h, c), dim=1)
        outs.append(torch.stack(out, 1))
    return torch.cat(outs, 2), handed


def _case(B, T, H, scale=1.5):
    g = torch.Generator().manual_seed(B * 100 + T + 7 * H)
    xg = torch.randn(B, T, 8 * H, generator=g)
    whh = [torch.randn(4 * H, H, generator=g) * (scale / H ** 0.5) for _ in range(2)]
    h0 = torch.rand(B, H, generator=g) * 2 - 1
    c0 = torch.rand(B, H, generator=g) * 6 - 3
    return xg, whh, torch.stack((h0, c0), dim=1).contiguous()


def _judge(math, what, got, ref, model):
    """f16x3: fp32-class, KTOL.  bf16: at most 2x the error of the fp64 model with the kernel's f16 roundings + 1e-4, inside 1e-3."""
    e = rel_err(got, ref)
    if math == "f16x3":
        print(f"  {what}: rel {e:.3e} (bound {KTOL:.0e})")
        assert e < KTOL, (what, e)
    else:
        ideal = rel_err(model, ref)
        print(f"  {what}: rel {e:.3e} (rounded fp64 model {ideal:.3e}; bound min(1e-3, 2x + 1e-4))")
        assert e < 1e-3 and e <= 2.0 * ideal + 1e-4, (what, e, ideal)


# H = 400: full width; H = 24 / 40: a half-empty last K chunk; B = 33 / 70: a second / a partly filled third batch tile
RAW_SHAPES = [(1, 1, 400), (2, 9, 24), (33, 6, 40), (3, 12, 400), (70, 4, 16)]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("B,T,H", RAW_SHAPES)
def test_carry_recurrence_matches_the_fp64_loop(B, T, H, math):
    from voicesplit_amd import ops
    xg, whh, state = _case(B, T, H)
    d = dev()
    for keep in sorted({1, T // 2 or 1, T}):
        ref, ref_state = _loop(xg, whh, state, keep, False)
        mod, mod_state = _loop(xg, whh, state, keep, True) if math == "bf16" else (ref, ref_state)
        out, state_out = ops.bilstm_recurrent_carry(xg.to(d), whh[0].to(d), whh[1].to(d), math, state=state.to(d), keep=keep)
        assert torch.isfinite(out).all() and torch.isfinite(state_out).all()
        print(f"B={B} T={T} H={H} {math} keep={keep}")
        _judge(math, "forward half", out[..., :H], ref[..., :H], mod[..., :H])
        _judge(math, "reverse half", out[..., H:], ref[..., H:], mod[..., H:])
        _judge(math, "state_out h", state_out[:, 0], ref_state[:, 0], mod_state[:, 0])
        _judge(math, "state_out c", state_out[:, 1], ref_state[:, 1], mod_state[:, 1])
        # the state handed out is the recurrence's own row keep - 1
        assert torch.equal(state_out[:, 0], out[:, keep - 1, :H])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("B,T,H", [(2, 9, 24), (3, 12, 400), (70, 4, 16)])
def test_carry_recurrence_from_a_zero_state_is_the_plain_recurrence(B, T, H, math):
    from voicesplit_amd import ops
    xg, whh, _ = _case(B, T, H)
    d = dev()
    plain = ops.bilstm_recurrent(xg.to(d), whh[0].to(d), whh[1].to(d), math=ops.MATH_CODES[math])
    for state in (None, torch.zeros(B, 2, H, device=d)):
        out, state_out = ops.bilstm_recurrent_carry(xg.to(d), whh[0].to(d), whh[1].to(d), math, state=state, keep=T)
        diff = (out - plain).abs().max().item()
        e = rel_err(out, plain)
        print(f"B={B} T={T} H={H} {math} state={'None' if state is None else 'zeros'}: max |carry - plain| = {diff:.3e} (0.0 expected)")
        assert e < (KTOL if math == "f16x3" else 1e-3), e
        assert torch.equal(state_out[:, 0], out[:, T - 1, :H])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("B,T,H", [(33, 6, 40), (3, 12, 400)])
def test_two_carried_calls_give_the_forward_half_of_one(B, T, H, math):
    """[0, a) then [a, T) with the first call's state: the hand-over is in the recurrence's own operand form, so the forward half is
    that of the single call bit for bit."""
    from voicesplit_amd import ops
    xg, whh, state = _case(B, T, H)
    d = dev()
    w = (whh[0].to(d), whh[1].to(d))
    whole, whole_state = ops.bilstm_recurrent_carry(xg.to(d), *w, math, state=state.to(d), keep=T)
    for a in (1, T - 1):
        first, mid = ops.bilstm_recurrent_carry(xg[:, :a].contiguous().to(d), *w, math, state=state.to(d), keep=a)
        second, last = ops.bilstm_recurrent_carry(xg[:, a:].contiguous().to(d), *w, math, state=mid, keep=T - a)
        got = torch.cat((first[..., :H], second[..., :H]), dim=1)
        diff = (got - whole[..., :H]).abs().max().item()
        sdiff = (last - whole_state).abs().max().item()
        print(f"B={B} T={T} H={H} {math} a={a}: max |two calls - one call| forward half {diff:.3e}, final state {sdiff:.3e} (0.0 expected)")
        assert diff == 0.0 and sdiff == 0.0
        # look-ahead rows: the forward rows t >= keep of a call are valid forward outputs too, and keep only moves the hand-out
        look, look_state = ops.bilstm_recurrent_carry(xg.to(d), *w, math, state=state.to(d), keep=a)
        assert torch.equal(look, whole) and torch.equal(look_state, mid)


def test_carry_is_refused_where_no_kernel_serves_it():
    from voicesplit_amd import _lib, ops
    xg, whh, state = _case(2, 5, 24)
    d = dev()
    lib = _lib.load()
    with pytest.raises(_lib.VoiceSplitHipError, match="VS_MATH_FP32"):
        ops.bilstm_recurrent_carry(xg.to(d), whh[0].to(d), whh[1].to(d), "fp32", state=state.to(d))
    with pytest.raises(_lib.VoiceSplitHipError, match="keep=6"):
        ops.bilstm_recurrent_carry(xg.to(d), whh[0].to(d), whh[1].to(d), "f16x3", state=state.to(d), keep=6)
    xg2, whh2, state2 = _case(1, 2, 456)
    with pytest.raises(_lib.VoiceSplitHipError, match="H <= 448"):
        ops.bilstm_recurrent_carry(xg2.to(d), whh2[0].to(d), whh2[1].to(d), "f16x3", state=state2.to(d))
    for mode in (1, 3, 4):
        try:
            assert lib.vs_set_lstm_kernel(mode) == 0
            with pytest.raises(_lib.VoiceSplitHipError, match="vs_set_lstm_kernel"):
                ops.bilstm_recurrent_carry(xg.to(d), whh[0].to(d), whh[1].to(d), "f16x3", state=state.to(d))
        finally:
            lib.vs_set_lstm_kernel(0)


# ---- full width: the masker on the HIP stages ------------------------------------------------------------------------------
B_FULL, T_FULL, C_FULL, R_FULL = 2, 200, 32, 16
_FULL = {}


def _full(cls_name):
    """Model, inputs and the fp64 references of one class, computed once and shared (read-only) by the tests below."""
    if cls_name not in _FULL:
        import voicesplit_amd as V
        act = "mish" if cls_name == "VoiceSplit" else "relu"
        dims_d = R.default_dims()
        sd = R.spread_logits(R.build_state_dict(dims_d, 3), 8.0)
        x, dvec = R.synthetic_inputs(B_FULL, T_FULL, dims_d, 13)
        sd64 = R.cast_state_dict(sd, torch.float64)
        with torch.no_grad():
            ref = R.forward(sd64, x.double(), dvec.double(), act=act, lstm_impl="loop")
        H, T, C, Rl = dims_d["lstm_dim"], T_FULL, C_FULL, R_FULL
        rev = torch.cat([R.lstm_direction(ref["lstm_in"][:, k * C:min((k + 1) * C + Rl, T)], sd64["lstm.weight_ih_l0_reverse"],
                                          sd64["lstm.weight_hh_l0_reverse"], sd64["lstm.bias_ih_l0_reverse"],
                                          sd64["lstm.bias_hh_l0_reverse"], True)[:, :min(C, T - k * C)] for k in range(-(-T // C))], dim=1)
        lstm = torch.cat((ref["lstm_out"][..., :H], rev), dim=2)
        y = torch.relu(torch.nn.functional.linear(torch.relu(lstm), sd64["fc1.weight"], sd64["fc1.bias"]))
        logits = torch.nn.functional.linear(y, sd64["fc2.weight"], sd64["fc2.bias"])
        m = getattr(V, cls_name)(V.default_config()).eval()
        m.load_state_dict(sd)
        _FULL[cls_name] = dict(model=m.cuda(), x=x, dvec=dvec, H=H, fwd=ref["lstm_out"][..., :H], rev=rev, logits=logits,
                               mask=torch.sigmoid(logits), whole_mask=ref["mask"], whole_rev=ref["lstm_out"][..., H:])
    return _FULL[cls_name]


def _run_stream(model, x, dvec, C, Rl, sizes, want_logits=True):
    from voicesplit_amd.streaming import StreamingMasker
    masker = StreamingMasker(*model.stream_stages(want_logits=want_logits), dvec.cuda(), C, Rl, trace=True)
    outs, pos, i, log = [], 0, 0, []
    while pos < x.shape[1]:
        n = min(sizes[i % len(sizes)], x.shape[1] - pos)
        outs.append(masker.push(x[:, pos:pos + n].cuda()))
        pos, i = pos + n, i + 1
        log.append((pos, masker.emitted))
    outs.append(masker.finish())
    lstm = torch.cat([c["lstm_out"] for c in masker.trace], dim=1).cpu()
    logits = torch.cat([c["logits"] for c in masker.trace], dim=1).cpu() if want_logits else None
    return torch.cat(outs, dim=1).cpu(), lstm, logits, log, masker


def _judge_stream(math, tag, mask, lstm, logits, f):
    H = f["H"]
    fig = {"fwd": rel_err(lstm[..., :H], f["fwd"]), "rev": rel_err(lstm[..., H:], f["rev"]), "logits": rel_err(logits, f["logits"]),
           "mask_rel": rel_err(mask, f["mask"]), "mask_abs": (mask.double() - f["mask"]).abs().max().item(),
           "mask_mse": ((mask.double() - f["mask"]) ** 2).mean().item()}
    print(f"  {tag} {math}: " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    if math == "f16x3":
        assert fig["fwd"] < REL_TOL and fig["rev"] < REL_TOL and fig["logits"] < REL_TOL, fig
        assert fig["mask_rel"] < REL_TOL and fig["mask_mse"] < MSE_TOL, fig
    else:
        assert fig["fwd"] < LSTM_TOL and fig["rev"] < LSTM_TOL, fig
        assert fig["mask_abs"] < MASK_ABS_TOL and fig["mask_mse"] < 1e-4, fig
    return fig


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cls_name", ["VoiceSplit", "VoiceFilter"])
def test_streamed_stages_match_the_oracle_on_every_frame(cls_name, math):
    """B = 2, T = 200, C = 32, R = 16 at full width: forward half against the whole-stream oracle, reverse half, logits and mask against
    the chunked definition, every frame; the stream pushed 1 frame at a time and all at once."""
    f = _full(cls_name)
    # the chunked reverse half is not the whole-stream one: the two definitions are told apart at the fp32-class tolerance
    assert rel_err(f["rev"], f["whole_rev"]) > 10 * REL_TOL
    with _math(math):
        one = _run_stream(f["model"], f["x"], f["dvec"], C_FULL, R_FULL, (1,))
        once = _run_stream(f["model"], f["x"], f["dvec"], C_FULL, R_FULL, (T_FULL,))
    print(f"{cls_name}")
    for tag, (mask, lstm, logits, log, masker) in (("1 frame at a time", one), ("all at once", once)):
        assert mask.shape == (B_FULL, T_FULL, 601) and torch.isfinite(mask).all()
        _judge_stream(math, tag, mask, lstm, logits, f)
    both = rel_err(one[0], once[0]) if math == "f16x3" else (one[0] - once[0]).abs().max().item()
    print(f"  1 frame at a time vs all at once: mask {'rel' if math == 'f16x3' else 'abs'} {both:.3e}")
    assert both < (REL_TOL if math == "f16x3" else MASK_ABS_TOL)
    # emission, 1 frame at a time: chunk k is out at exactly (k + 1) C + R + 65 pushed frames
    for pushed, emitted in one[3]:
        assert emitted == C_FULL * max(0, (pushed - R_FULL - 65) // C_FULL), (pushed, emitted)
    assert one[4].latency_frames == C_FULL + R_FULL + 65


@pytest.mark.parametrize("math", MATHS)
def test_one_chunk_with_the_whole_stream_is_the_model(math):
    """C + R >= T: the streamed mask against model(x, emb) (and the whole-stream oracle)."""
    f = _full("VoiceSplit")
    with _math(math), torch.no_grad():
        whole = f["model"](f["x"].cuda(), f["dvec"].cuda()).cpu()
        mask, _, _, _, _ = _run_stream(f["model"], f["x"], f["dvec"], 150, 50, (7, 64, 1), want_logits=False)
    rel, ab = rel_err(mask, whole), (mask - whole).abs().max().item()
    mse = ((mask.double() - f["whole_mask"]) ** 2).mean().item()
    print(f"{math}: streamed (C = 150, R = 50) vs model(): rel {rel:.3e} abs {ab:.3e}; MSE vs the whole-stream oracle {mse:.3e}")
    if math == "f16x3":
        assert rel < REL_TOL and mse < MSE_TOL
    else:
        assert ab < MASK_ABS_TOL and mse < 1e-4


@pytest.mark.parametrize("math", MATHS)
def test_carried_state_is_what_running_the_model_chunk_by_chunk_lacks(math):
    """What the feature is for.  The model on each 32-frame chunk alone restarts the forward LSTM direction: from the second chunk on its
    forward half misses the whole-stream oracle by far more than the tolerance; the streamed forward half is within it."""
    from voicesplit_amd import ops
    f = _full("VoiceSplit")
    m, H, C = f["model"], f["H"], C_FULL
    tol = REL_TOL if math == "f16x3" else LSTM_TOL
    with _math(math), torch.no_grad():
        sd = {k: v.detach() for k, v in m._tensors().items()}
        alone = []
        for k in range(-(-T_FULL // C)):
            xk = f["x"][:, k * C:(k + 1) * C].contiguous().cuda()
            dims = m._dims(xk.shape[0], xk.shape[1])
            alone.append(ops.bilstm(sd, ops.conv_stack(sd, xk, dims, m.conv_act), f["dvec"].cuda(), dims)[..., :H].cpu())
        _, lstm, _, _, _ = _run_stream(m, f["x"], f["dvec"], C, R_FULL, (C,), want_logits=False)
    alone_err = [rel_err(a, f["fwd"][:, k * C:(k + 1) * C]) for k, a in enumerate(alone)]
    stream_err = [rel_err(lstm[:, k * C:(k + 1) * C, :H], f["fwd"][:, k * C:(k + 1) * C]) for k in range(len(alone))]
    print(f"{math}: forward half per chunk vs the whole-stream oracle (tolerance {tol:.0e})")
    print("  model() chunk by chunk: " + " ".join(f"{e:.2e}" for e in alone_err))
    print("  streamed              : " + " ".join(f"{e:.2e}" for e in stream_err))
    assert all(e > tol for e in alone_err[1:]), alone_err
    assert all(e < tol for e in stream_err), stream_err


# ---- audio ------------------------------------------------------------------------------------------------------------------
def _wav(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S) / 16000.0
    tones = sum(a * torch.sin(2 * np.pi * fr * t + p) for a, fr, p in [(0.05, 220.0, 0.1), (0.03, 1750.0, 1.0), (0.01, 5300.0, 2.0)])
    return (tones[None] + 0.004 * torch.randn(B, S, generator=g)).float()


@pytest.mark.parametrize("math", MATHS)
def test_streaming_separator_equals_the_whole_clip_synthesis(math):
    """2 s synthetic mixture, C = 16, R = 8: the concatenated output against spec_to_wav(spec, phase, mask = the streamed masks) of the
    whole clip, for uneven pushes and hop-sized pushes; the reported latency against the samples actually withheld."""
    from voicesplit_amd import audio
    f = _full("VoiceSplit")
    hop, S, C, Rl = 160, 32000, 16, 8
    wav = _wav(2, S, 4).cuda()
    with _math(math):
        spec, phase = audio.wav_to_spec(wav, AUDIO)
        for tag, sizes in (("uneven pushes", (3, 40, 1, 17, 9)), ("hop-sized pushes", (1,))):
            sep = audio.StreamingSeparator(f["model"], f["dvec"].cuda(), AUDIO, C, Rl, trace=True)
            assert sep.latency_samples == (C + Rl + 65 + 2 * 4) * hop
            outs, pos, i, worst, at_emission = [], 0, 0, 0, set()
            while pos < S:
                n = min(sizes[i % len(sizes)] * hop, S - pos)
                returned = sum(o.shape[1] for o in outs)
                out = sep.push(wav[:, pos:pos + n].contiguous())
                pos, i = pos + n, i + 1
                if out.shape[1] and returned:
                    at_emission.add(pos - returned)                      # behind the newest sample when a block leaves
                outs.append(out)
                worst = max(worst, pos - returned - out.shape[1])        # still withheld when the push returns
            outs.append(sep.finish())
            got = torch.cat(outs, dim=1)
            masks = torch.cat(sep.mask_trace, dim=1)
            assert got.shape == (2, S) and masks.shape == spec.shape
            ref = audio.spec_to_wav(spec, phase, AUDIO, mask=masks.contiguous())
            err = ((got - ref).abs().max() / ref.abs().max()).item()
            print(f"{math} {tag}: max |streamed - whole-clip synthesis| / max |whole| = {err:.3e} (bound {WAV_TOL:.0e}); "
                  f"a block starts {sorted(at_emission)} samples behind the newest one, at most {worst} stay withheld behind a push, "
                  f"reported latency {sep.latency_samples}")
            assert err < WAV_TOL
            # no sample stays withheld once latency_samples more have arrived (a push of several hops arrives at once)
            assert worst < sep.latency_samples
            if sizes == (1,):          # hop by hop: every block after the first starts exactly latency_samples behind the newest sample
                assert at_emission == {sep.latency_samples} and worst == sep.latency_samples - hop


# ---- the separator where hop divides n_fft / 2 -----------------------------------------------------------------------------------
_SMALL = {}


def _small(n_fft):
    """A VoiceSplit with num_freq = fc2_dim = n_fft / 2 + 1 (lstm_dim 24: a width of RAW_SHAPES) and two d-vectors, built once."""
    if n_fft not in _SMALL:
        import voicesplit_amd as V
        dims = dict(num_freq=n_fft // 2 + 1, emb_dim=16, lstm_dim=24, fc1_dim=40, fc2_dim=n_fft // 2 + 1)
        m = V.VoiceSplit(V.default_config(**dims)).eval()
        m.load_state_dict(R.spread_logits(R.build_state_dict(dims, 2), 6.0))
        _SMALL[n_fft] = (m.cuda(), R.synthetic_inputs(2, 8, dims, 2)[1].cuda())
    return _SMALL[n_fft]


@pytest.mark.parametrize("n_fft,hop,win", [(64, 16, 64), (256, 64, 255)], ids=["64-16-64", "256-64-255"])
def test_streaming_separator_where_hop_divides_half_the_frame(n_fft, hop, win):
    """The body of test_streaming_separator_equals_the_whole_clip_synthesis at 64 / 16 / 64 and 256 / 64 / 255 (an odd window), C = 4,
    R = 2, 160 hops.  Here margin * hop == n_fft / 2 exactly, so the segment pending when the stream reaches ``margin`` hops is
    as long as the reflect padding and vs_wav_to_spec refuses it: the separator must hold the first analysis back until more
    than n_fft / 2 samples are pending.  The uneven pushes start with exactly ``margin`` hops; the hop-sized ones reach it at push
    number ``margin``."""
    from voicesplit_amd import audio
    cfg = dict(AUDIO, n_fft=n_fft, hop_length=hop, win_length=win)
    model, dvec = _small(n_fft)
    S, C, Rl, margin = 160 * hop, 4, 2, n_fft // 2 // hop
    assert margin * hop == n_fft // 2
    wav = _wav(2, S, 6).cuda()
    spec, phase = audio.wav_to_spec(wav, cfg)
    for tag, sizes in (("uneven pushes", (margin, 40, 1, 17, 9)), ("hop-sized pushes", (1,))):
        sep = audio.StreamingSeparator(model, dvec, cfg, C, Rl, trace=True)
        assert sep.margin == margin and sep.latency_samples == (C + Rl + 65 + 2 * margin) * hop
        outs, pos, i, worst, at_emission, blocks = [], 0, 0, 0, set(), 0
        while pos < S:
            n = min(sizes[i % len(sizes)] * hop, S - pos)
            returned = sum(o.shape[1] for o in outs)
            out = sep.push(wav[:, pos:pos + n].contiguous())
            pos, i = pos + n, i + 1
            if out.shape[1] and returned:
                at_emission.add(pos - returned)
            blocks += bool(out.shape[1])
            outs.append(out)
            worst = max(worst, pos - returned - out.shape[1])
        outs.append(sep.finish())
        got = torch.cat(outs, dim=1)
        masks = torch.cat(sep.mask_trace, dim=1)
        assert got.shape == (2, S) and masks.shape == spec.shape          # every pushed sample is returned
        ref = audio.spec_to_wav(spec, phase, cfg, mask=masks.contiguous())
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"{n_fft}/{hop}/{win} {tag}: max |streamed - whole-clip synthesis| / max |whole| = {err:.3e} (bound {WAV_TOL:.0e}); "
              f"{blocks} blocks before finish(), a block starts {sorted(at_emission)} samples behind the newest one, at most {worst} "
              f"stay withheld behind a push, reported latency {sep.latency_samples}")
        assert blocks >= 3                                                 # several chunks came out while the stream ran
        assert err < WAV_TOL
        assert worst < sep.latency_samples
        if sizes == (1,):
            assert at_emission == {sep.latency_samples} and worst == sep.latency_samples - hop


def test_streaming_separator_finish_on_a_stream_no_longer_than_the_reflect_padding():
    """A stream that ends with n_fft / 2 samples or fewer: push() holds them back and returns nothing, finish() raises what the
    whole-clip call raises, VoiceSplitHipError."""
    from voicesplit_amd import _lib, audio
    cfg = dict(AUDIO, n_fft=64, hop_length=16, win_length=64)
    model, dvec = _small(64)
    wav = _wav(2, 32, 7).cuda()
    with pytest.raises(_lib.VoiceSplitHipError, match="reflect padding"):
        audio.wav_to_spec(wav, cfg)
    sep = audio.StreamingSeparator(model, dvec, cfg, 4, 2)
    for k in range(2):
        assert sep.push(wav[:, 16 * k:16 * (k + 1)].contiguous()).shape == (2, 0)
    with pytest.raises(_lib.VoiceSplitHipError, match="reflect padding"):
        sep.finish()
