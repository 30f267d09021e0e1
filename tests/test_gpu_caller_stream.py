"""GPU: the stream contract of include/voicesplit_hip.h off the null stream -- "all work is enqueued asynchronously on `stream`",
"calls on different streams with disjoint buffers are otherwise independent", the side stream's fork and join.

Every other GPU test runs under torch's default current stream, the legacy null stream, where a launch on stream 0 instead of
``stream`` is the same stream and nothing can show.  Here one call of every family runs under a fresh non-blocking stream that is
still busy with a bounded delay (tests/stream_helpers.py): its floating-point inputs are NaN until a copy queued on that stream
behind the delay brings the real values, and its results are cloned on that stream with no synchronisation.  A launch, fill or
copy on another stream runs at once and reads NaN; a missing join lets the clone run early.  The criterion is bit equality with
the run under the null stream.  Integer inputs (lengths, offsets, descriptors, tables) are written and synchronised before the
delay and never poisoned: a racing kernel may see a wrong float, never a wrong index.

Then: objects that build device data once and keep it (``Resampler``, ``SpeakerEncoder``'s packed weights, the model's prepared
weights, ``RirPool``) are built under one held stream and used at once under a second one (``_call.Built`` orders the two), and two
callers run at once on two held streams.  The shapes are the smallest ones the other tests judge."""
import contextlib

import numpy as np
import pytest
import torch

import griffin_lim_ref as G
import reverb_ref as RR
from oracle import reference_forward as R
from stream_helpers import assert_same, held_stream, held_streams, keep, probe
from test_gpu_audio_backend import _foreign_blocks
from test_gpu_bss_eval import _case as bss_case
from test_gpu_griffin_lim import _dev as griffin_inputs
from test_gpu_loss import _case as loss_case
from test_gpu_overlay import hand_item
from test_gpu_resample import _signal
from test_gpu_reverb import FILTERS, TOTAL, _rows as fir_rows_case
from test_gpu_sdr import _demo_batch
from test_gpu_speaker import AUDIO as SPEAKER_AUDIO, build as build_encoder, demo_wavs, seeded_mel
from test_gpu_stft_geometry import clips
from test_gpu_stoi import _speech16
from test_gpu_stream import _wav

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SMOKE = dict(num_freq=37, emb_dim=16, lstm_dim=24, fc1_dim=40, fc2_dim=37)          # __graft_entry__.smoke
SMALL_BF16 = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
G1 = G.GEOMETRIES["G1"]
G1_CFG = {"n_fft": G1[0], "hop_length": G1[1], "win_length": G1[2], "min_level_db": -100.0, "ref_level_db": 20.0}
NAMES = ("num_freq", "emb_dim", "lstm_dim", "fc1_dim", "fc2_dim")


@contextlib.contextmanager
def _math(name, deterministic=False):
    from voicesplit_amd import _lib, ops
    prev = ops.get_conv_math()
    prev_det = _lib.get_option("DETERMINISTIC")
    ops.set_conv_math(name)
    _lib.set_option("DETERMINISTIC", 1 if deterministic else prev_det)
    try:
        yield
    finally:
        ops.set_conv_math(prev)
        _lib.set_option("DETERMINISTIC", prev_det)


def _floats(tensors):
    return [t for t in tensors if t.is_floating_point()]


def _module(dims, seed=2, training=False):
    import voicesplit_amd as V
    m = V.VoiceSplit(V.default_config(*(dims[k] for k in NAMES)))
    m.load_state_dict(R.spread_logits(R.build_state_dict(dims, seed), 6.0), strict=True)
    return m.cuda().train(training)


def _module_state(m):
    """(floats, ints) of a module: parameters and buffers; the train-mode forward moves the BatchNorm buffers in place."""
    tensors = [p.data for p in m.parameters()] + list(m.buffers())
    return _floats(tensors), [t for t in tensors if not t.is_floating_point()]


# ---- eval forward ---------------------------------------------------------------------------------------------------------------------
def _eval_case():
    sd = {k: v.cuda().contiguous() for k, v in R.build_state_dict(SMOKE, 2).items()}
    x, dvec = (t.cuda() for t in R.synthetic_inputs(2, 40, SMOKE, 2))
    return sd, x, dvec


@pytest.mark.parametrize("math", ["fp32", "f16x3", "bf16"])
def test_forward(math):
    from voicesplit_amd import ops
    sd, x, dvec = _eval_case()
    dims = ops.make_dims(2, 40, *(SMOKE[k] for k in NAMES), math=math)
    probe(f"ops.forward {math}", lambda: ops.forward(sd, x, dvec, dims, "mish"), _floats(sd.values()) + [x, dvec])


def test_forward_prepared_with_lengths():
    """The weights are prepared under the held stream too, behind the copy that brings them."""
    from voicesplit_amd import ops
    sd, x, dvec = _eval_case()
    dims = ops.make_dims(2, 40, *(SMOKE[k] for k in NAMES), math="f16x3")
    probe("forward_prepared(lengths)", lambda: ops.forward_prepared(sd, ops.PreparedWeights(sd, dims), x, dvec, dims, "mish", lengths=[40, 23]),
          _floats(sd.values()) + [x, dvec], wrapper="forward_prepared(lengths)")


def test_forward_prepared_multi():
    from voicesplit_amd import ops
    sd, x, dvec = _eval_case()
    dvecs = torch.stack((dvec, R.synthetic_inputs(2, 40, SMOKE, 3)[1].cuda()), dim=1).contiguous()
    dims = ops.make_dims(2, 40, *(SMOKE[k] for k in NAMES), math="f16x3")
    probe("forward_prepared_multi K=2", lambda: ops.forward_prepared_multi(sd, ops.PreparedWeights(sd, dims), x, dvecs, dims, "mish"),
          _floats(sd.values()) + [x, dvecs])


# ---- training step through the autograd module ----------------------------------------------------------------------------------------
@contextlib.contextmanager
def _side_stream(on: bool):
    """Backward overlap, VS_OPT_FWD_PROLOGUE and VS_OPT_HEAD_LEAF_SIDE: all on (the defaults, which use the side stream) or all off."""
    from voicesplit_amd import _lib
    lib = _lib.load()
    prev = {k: _lib.get_option(k) for k in ("FWD_PROLOGUE", "HEAD_LEAF_SIDE")}
    try:
        assert lib.vs_set_backward_overlap(int(on)) == 0
        for k in prev:
            _lib.set_option(k, int(on))
        yield
    finally:
        lib.vs_set_backward_overlap(1)
        for k, v in prev.items():
            _lib.set_option(k, v)


def _train_case(dims, B, T, seed):
    """A module in train mode and one batch of the loss's inputs at the geometry n_fft = 2 (F - 1), hop = win / 4."""
    n_fft = 2 * (dims["num_freq"] - 1)
    _, mixed, target, phase, lens, audio = loss_case(B, T, n_fft, n_fft // 4, n_fft, seed)
    dvec = R.synthetic_inputs(B, T, dims, seed)[1]
    m = _module(dims, seed, training=True)
    return m, [t.cuda() for t in (mixed, target, phase, dvec)], lens.to(torch.int32).cuda(), audio


def _train_step(m, mixed, target, phase, dvec, lens, audio):
    """forward_train, losses.sisnr_loss, backward -> the mask, the loss and every gradient."""
    from voicesplit_amd import losses
    m.zero_grad(set_to_none=True)
    mask = m(mixed, dvec)
    loss = losses.sisnr_loss(mask, mixed, target, phase, lens, audio)
    loss.backward()
    return {"mask": mask, "loss": loss, "grad": {k: p.grad for k, p in m.named_parameters()},
            "buffers": {k: b for k, b in m.named_buffers()}}


@pytest.mark.parametrize("side", [True, False], ids=["side-stream-on", "side-stream-off"])
@pytest.mark.parametrize("math", ["fp32", "f16x3", "bf16"])
def test_training_step(math, side):
    """bf16 in arrival order is not bit-repeatable by contract (VS_OPT_DETERMINISTIC): that arm runs with the option at 1."""
    dims, B, T = (SMALL_BF16, 3, 37) if math == "bf16" else (SMOKE, 2, 40)
    with _math(math, deterministic=math == "bf16"), _side_stream(side):
        m, data, lens, audio = _train_case(dims, B, T, 4)
        floats, ints = _module_state(m)
        want = probe(f"training step {math} side={int(side)}", lambda: _train_step(m, *data, lens, audio), floats + data, ints)
    names = {n for n, _ in want}
    assert {"out.mask", "out.loss", "out.buffers.conv.2.running_mean"} <= names
    assert {"out.grad." + k for k, _ in m.named_parameters()} <= names                    # every gradient was there to compare


# ---- audio ----------------------------------------------------------------------------------------------------------------------------
def test_wav_to_spec():
    from voicesplit_amd import audio
    wav = clips("G1", 2, 4, 1.0).cuda()
    probe("wav_to_spec G1", lambda: audio.wav_to_spec(wav, G1_CFG), [wav])


def test_spec_to_wav():
    from voicesplit_amd import audio
    spec, phase = audio.wav_to_spec(clips("G1", 2, 4, 1.0).cuda(), G1_CFG)
    mask = torch.rand(spec.shape, generator=torch.Generator().manual_seed(35)).cuda()
    probe("spec_to_wav G1", lambda: audio.spec_to_wav(spec, phase, G1_CFG, mask=mask), [spec, phase, mask])


def test_griffin_lim():
    from voicesplit_amd import audio
    spec, phase, _ = griffin_inputs(2, 4, "mixture", G1)
    probe("griffin_lim G1 n=4", lambda: audio.griffin_lim(spec, G.audio_cfg(G1), n_iter=4, power=1.0, init_phase=phase, return_residual=True),
          [spec, phase])


def test_wavernn_inv_spectrogram():
    from voicesplit_amd import audio
    ap = audio.AudioProcessor(dict(_foreign_blocks(), backend="wavernn", mel_spec=False))
    spec = ap.get_spec_from_audio(clips("G1", 2, 4, 1.0).cuda())
    angles = (2.0 * np.pi * torch.rand(spec.shape, generator=torch.Generator().manual_seed(11))).cuda()
    probe("wavernn inv_spectrogram G1", lambda: ap.inv_spectrogram(spec, init_phase=angles), [spec, angles])


def test_deemphasis():
    from voicesplit_amd import audio
    wav = (0.1 * torch.randn(2, 2 * audio.deemphasis_block() + 3, generator=torch.Generator().manual_seed(3))).cuda()
    probe("deemphasis", lambda: audio.deemphasis(wav, 0.97), [wav])


# ---- metrics --------------------------------------------------------------------------------------------------------------------------
def test_bss_sdr():
    from voicesplit_amd import metrics
    ref, est = (torch.from_numpy(a).cuda() for a in _demo_batch(B=4, N=20000))
    probe("bss_sdr 4 x 20000", lambda: metrics.bss_sdr(ref, est), [ref, est])


def test_bss_eval():
    from voicesplit_amd import metrics
    ref, est = (torch.from_numpy(np.array(a, dtype=np.float32)).cuda() for a in bss_case(2, 6001)[:2])
    probe("bss_eval K=2 N=6001", lambda: metrics.bss_eval(ref, est), [ref, est])


def test_stoi_at_16k():
    """16 kHz: both signals go through the cached 16000 -> 10000 resampler of metrics._stoi_resampler."""
    from voicesplit_amd import metrics
    x, y = _speech16(14000, (1, 2))
    probe("stoi 16 kHz", lambda: metrics.stoi(x, y, 16000), [x, y], wrapper="stoi")


def test_loudness():
    from voicesplit_amd.loudness import LoudnessMeter
    meter = LoudnessMeter(16000, DEV)
    wav = (0.1 * torch.randn(2, 8000, generator=torch.Generator().manual_seed(8))).cuda()
    probe("loudness 2 x 8000", lambda: meter(wav), [wav], wrapper="loudness")


# ---- speaker --------------------------------------------------------------------------------------------------------------------------
def test_logmel():
    from voicesplit_amd import speaker
    wav = demo_wavs()[0][16000:16000 + 601].contiguous().cuda()
    probe("logmel 601 samples", lambda: speaker.logmel(wav, SPEAKER_AUDIO), [wav])


def _encoder_case():
    enc = build_encoder(8, 1, 24, 16, 10, 5, seed=1).to(DEV)
    return enc, [seeded_mel(8, T, 10 + T).cuda() for T in (10, 23, 57, 9)]


def test_embed_many():
    """The parameters are poisoned too, and the packed weights are dropped in front of every call: they are built again under the
    held stream, behind the copy that brings the parameters."""
    enc, mels = _encoder_case()

    def embed():
        enc.__dict__.pop("_prepared", None)
        return enc.embed_many(mels)

    probe("embed_many", embed, [p.data for p in enc.parameters()] + mels, wrapper="embed_many")


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def test_resampler():
    from voicesplit_amd.resample import Resampler
    rs = Resampler(16000, 10000, DEV)
    x = _signal(2, 3000, 5).cuda()
    probe("Resampler 16000 -> 10000", lambda: rs(x), [x])


def test_mix_clips():
    """The small pool of tests/test_gpu_mixing.py: every alignment mod 4, the maxima at both ends, a silent sum."""
    from voicesplit_amd.mixing import mix_clips
    L, B = 1600, 5
    rng = np.random.default_rng(5)
    flat = (rng.standard_normal(2 * B * (L + 8)) * 0.1).astype(np.float32)
    clean_at = [b * (L + 8) + r for b, r in enumerate((0, 1, 2, 3, 1))]
    interf_at = [(B + b) * (L + 8) + r for b, r in enumerate((3, 0, 1, 2, 2))]
    flat[clean_at[1]], flat[interf_at[1]] = 3.0, 0.5
    flat[interf_at[4]:interf_at[4] + L] = -flat[clean_at[4]:clean_at[4] + L]
    flat = torch.from_numpy(flat).cuda()
    ca, ia = (torch.tensor(v, dtype=torch.int64, device=DEV) for v in (clean_at, interf_at))
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    probe("mix_clips", lambda: (mix_clips(flat, ca, ia, L, count), count), [flat], [count])


def test_mix_sequence():
    """The hand-built descriptors of tests/test_gpu_overlay.py (segments of every length mod 4, three affines, absent segments)."""
    from voicesplit_amd.mixing import mix_sequence
    rng = np.random.default_rng(9)
    flat = torch.from_numpy((rng.standard_normal(30000) * 0.2).astype(np.float32)).cuda()
    noise = torch.from_numpy((rng.standard_normal(20000) * 0.05).astype(np.float32)).cuda()
    rows = [hand_item((3, 5002, 9001), (2049, 1023, 2050), (1, 6), (1, 6), 5122, sel=(0, 1, 0), gain=(0.9, -1.3, 0.5), bias=(0.01, -0.02, 0.0)),
            hand_item((10, 20, 30), (1, 2, 3), (7, 2), (7, 2), 6, sel=(1, -1, 1)),
            hand_item((0, 0, 4097), (0, 0, 4099), (3, 0), (0, 3), 4099, sel=(0, 0, 0), in_target=(0, 0, 1)),
            hand_item((6, 0, 0), (2047, 0, 0), sel=(-1, 0, 0)),
            hand_item((0, 12001, 0), (0, 2047, 0), (5, 5), (4, 4), 3001, sel=(-1, 1, -1), in_target=(0, 1, 0), gain=(1, 0.25, 1), bias=(0, 0.125, 0))]
    desc = torch.from_numpy(np.stack(rows)).to(DEV)
    probe("mix_sequence", lambda: mix_sequence(flat, noise, desc, 5124, 5122), [flat, noise])


def test_shoebox_rir():
    """No floating-point device input: the descriptors go up inside the call.  What is left to see is the clone behind the call."""
    from voicesplit_amd import reverb
    rooms = torch.from_numpy(RR.gpu_test_rooms())
    probe("shoebox_rir five rooms", lambda: reverb.shoebox_rir(rooms, DEV), [], wrapper="shoebox_rir")


@pytest.mark.parametrize("math", ["f16x3", "fp32"])
def test_fir_rows(math):
    from voicesplit_amd import reverb
    rng = np.random.default_rng(5)
    flat = torch.from_numpy((0.1 * rng.standard_normal(TOTAL)).astype(np.float32)).cuda()
    h = np.zeros((len(FILTERS), 2049), dtype=np.float32)
    for r, n in enumerate(FILTERS):
        h[r, :n] = (rng.standard_normal(n) * np.exp(-np.arange(n) / 300.0)).astype(np.float32)
    h = torch.from_numpy(h).cuda()
    at, lo, hrow, nh = fir_rows_case(1000, 0)
    at, lo = (torch.tensor(v, dtype=torch.int64, device=DEV) for v in (at, lo))
    nh, hrow = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (nh, hrow))
    probe(f"fir_rows L=1000 {math}", lambda: reverb.fir_rows(flat, at, lo, nh, hrow, h, 1000, math), [flat, h])


# ---- one streaming push ---------------------------------------------------------------------------------------------------------------
def test_streaming_separator_push():
    """64 / 16 / 64, C = 4, R = 2: one push of 160 hops, more than the separator's latency, so samples come back."""
    from voicesplit_amd import audio
    dims = dict(num_freq=33, emb_dim=16, lstm_dim=24, fc1_dim=40, fc2_dim=33)
    m = _module(dims, 2)
    dvec = R.synthetic_inputs(2, 8, dims, 2)[1].cuda()
    cfg = dict(G1_CFG, n_fft=64, hop_length=16, win_length=64)
    wav = _wav(2, 160 * 16, 6).cuda()

    def push():
        out = audio.StreamingSeparator(m, dvec, cfg, 4, 2).push(wav)
        assert out.shape[1] > 0
        return out

    with torch.no_grad():
        probe("StreamingSeparator.push", push, _module_state(m)[0] + [dvec, wav])


# ---- build on one stream, use on another ----------------------------------------------------------------------------------------------
def _build_then_use(label, build, use, want, sizes=(), blocking=None):
    """``build()`` under a held stream A, so that its kernels sit behind the delay; at once ``use(built)`` under a second fresh
    stream B that runs past A; the result, cloned on B, against ``want`` (the null-stream run).  A must still be held when the
    builder is called and, unless the builder or the use blocks the host (``blocking``: its name in HOST_BLOCKING), when the use
    has been enqueued.  sizes: the bytes of the buffers the builder allocates (``stream_helpers.poison_pool``)."""
    with held_stream(label, poison=sizes, free=1) as a:
        b = a.free[0]
        with torch.cuda.stream(a.stream):
            a.before()
            built = build()
        with torch.cuda.stream(b):
            got = keep(use(built))
        a.after(blocking)
        b.synchronize()
    assert_same(label, got, want)


def _resampler_want(x):
    from voicesplit_amd.resample import Resampler
    ref = Resampler(16000, 10000, DEV)
    want = keep(ref(x))
    torch.cuda.synchronize()
    return ref, want


def test_audio_resampler_built_under_one_stream_and_used_under_another():
    from voicesplit_amd import audio
    x = _signal(2, 3000, 5).cuda()
    ref, want = _resampler_want(x)                       # kept alive: its bank must not be the block the new one is handed
    audio._RESAMPLERS.clear()
    try:
        _build_then_use("audio.resampler: build on A, use on B", lambda: audio.resampler(16000, 10000, DEV), lambda rs: rs(x), want,
                        sizes=[ref.bank.numel() * 4])
    finally:
        audio._RESAMPLERS.clear()


def test_stoi_resampler_built_under_one_stream_and_used_under_another():
    from voicesplit_amd import metrics
    x, y = _speech16(14000, (1, 2))
    want = keep(metrics.stoi(x, y, 16000))
    torch.cuda.synchronize()
    held = dict(metrics._STOI_RESAMPLERS)                # kept alive, as above
    metrics._STOI_RESAMPLERS.clear()
    try:
        _build_then_use("metrics._stoi_resampler: build on A, use on B", lambda: metrics._stoi_resampler(16000, DEV),
                        lambda rs: metrics.stoi(x, y, 16000), want, sizes=[next(iter(held.values())).bank.numel() * 4],
                        blocking="stoi")
    finally:
        metrics._STOI_RESAMPLERS.clear()


def test_speaker_weights_prepared_under_one_stream_and_used_under_another():
    """The consumer takes no index out of the packed weights: their header holds the layers' |max| bits and power-of-two scales,
    all floats (csrc/speaker.hip, vs_speaker_prepare / vs_speaker_embed)."""
    enc, mels = _encoder_case()
    want = keep(enc.embed_many(mels))
    torch.cuda.synchronize()
    size = enc.__dict__.pop("_prepared")[1].numel()
    _build_then_use("SpeakerEncoder._prepare: build on A, use on B", lambda: enc._prepare(DEV), lambda _: enc.embed_many(mels), want,
                    sizes=[size], blocking="embed_many")


def test_model_weights_prepared_under_one_stream_and_used_under_another():
    m = _module(SMOKE, 2)
    x, dvec = (t.cuda() for t in R.synthetic_inputs(2, 40, SMOKE, 2))
    with torch.no_grad():
        want = keep(m(x, dvec))
        torch.cuda.synchronize()
        size = m.__dict__.pop("_prepared").buf.numel()
        _build_then_use("model._prepared_for: build on A, use on B", lambda: m._prepared_for(m._tensors(), m._dims(2, 40)),
                        lambda _: m(x, dvec), want, sizes=[size])


@pytest.mark.parametrize("how", ["construction", "redraw"])
def test_rir_pool_drawn_under_one_stream_and_used_under_another(how):
    """``shoebox_rir`` uploads the rooms with a blocking copy in front of its kernel, so the builder's kernel cannot be held behind
    the delay: what the case keeps is that the use under B follows the build under A with nothing between them but the event."""
    from voicesplit_amd import reverb
    wav = _signal(4, 2000, 7).cuda()
    first = reverb.RirPool(2, DEV, seed=3, nh=256)
    make = (lambda: reverb.RirPool(2, DEV, seed=3, nh=256)) if how == "construction" else (lambda: first.redraw(1))
    ref = make()
    want = keep(reverb.apply(wav, ref.h, nh=ref.nh))
    torch.cuda.synchronize()
    _build_then_use(f"RirPool {how}: build on A, use on B", make, lambda pool: reverb.apply(wav, pool.h, nh=pool.nh), want,
                    sizes=[ref.h.numel() * 4], blocking="RirPool")


# ---- two callers at once --------------------------------------------------------------------------------------------------------------
def _poison(floats):
    stage = [t.detach().clone() for t in floats]
    for t in floats:
        t.detach().fill_(float("nan"))
    return stage


def _bring(floats, stage):
    with torch.no_grad():
        for t, s in zip(floats, stage):
            t.detach().copy_(s)


def test_audio_legs_beside_bss_sdr():
    """Two held streams, disjoint buffers, different scratch slots ("audio" and "metric"), calls enqueued alternately from one host
    thread: each caller gets the bits of its run alone."""
    from voicesplit_amd import audio, metrics
    wav = clips("G1", 2, 4, 1.0).cuda()
    mask = torch.rand(2, 4, G1[0] // 2 + 1, generator=torch.Generator().manual_seed(35)).cuda()
    ref, est = (torch.from_numpy(a).cuda() for a in _demo_batch(B=4, N=20000))

    def legs_1():
        return audio.wav_to_spec(wav, G1_CFG)

    def legs_2(spec, phase):
        return audio.spec_to_wav(spec, phase, G1_CFG, mask=mask)

    spec, phase = legs_1()
    want_1 = keep((spec, phase, legs_2(spec, phase)))
    want_2 = keep((metrics.bss_sdr(ref, est), metrics.bss_sdr(est, ref)))
    torch.cuda.synchronize()
    stage_1, stage_2 = _poison([wav, mask]), _poison([ref, est])
    torch.cuda.synchronize()
    with held_streams(["two callers (a): audio legs", "two callers (a): bss_sdr"]) as (h1, h2):
        with torch.cuda.stream(h1.stream):
            _bring([wav, mask], stage_1)
        with torch.cuda.stream(h2.stream):
            _bring([ref, est], stage_2)
        h1.before(), h2.before()
        with torch.cuda.stream(h1.stream):
            spec, phase = legs_1()
        with torch.cuda.stream(h2.stream):
            sdr_a = metrics.bss_sdr(ref, est)
        with torch.cuda.stream(h1.stream):
            got_1 = keep((spec, phase, legs_2(spec, phase)))
        with torch.cuda.stream(h2.stream):
            got_2 = keep((sdr_a, metrics.bss_sdr(est, ref)))
        h1.after(), h2.after()
        h1.stream.synchronize(), h2.stream.synchronize()
    assert_same("two callers (a): audio legs", got_1, want_1)
    assert_same("two callers (a): bss_sdr", got_2, want_2)


def test_two_training_steps_at_once():
    """Two modules, two tapes, one library-owned side stream: forward, forward, backward, backward, alternately from one host
    thread.  The recurrence is pinned to the per-step kernels (vs_set_lstm_kernel(1)): the persistent, cooperatively launched one is
    not meant to run on two streams at once (a bounded spin giving up there is documented behaviour).  The loss is a weighted sum
    of the mask: ``losses.sisnr_loss`` works in the device's one "loss" scratch slot, which serves one stream at a time."""
    from voicesplit_amd import _lib
    lib = _lib.load()

    def forward(m, x, dvec):
        m.zero_grad(set_to_none=True)
        return m(x, dvec)

    def results(m, mask):
        return {"mask": mask, "grad": {k: p.grad for k, p in m.named_parameters()}, "buffers": {k: b for k, b in m.named_buffers()}}

    try:
        assert lib.vs_set_lstm_kernel(1) == 0
        with _math("f16x3"):
            callers = []
            for seed in (4, 5):
                m = _module(SMOKE, seed, training=True)
                x, dvec = (t.cuda() for t in R.synthetic_inputs(2, 40, SMOKE, seed))
                w = torch.randn(2, 40, SMOKE["fc2_dim"], generator=torch.Generator().manual_seed(seed)).cuda()
                floats, ints = _module_state(m)
                callers.append(dict(m=m, x=x, dvec=dvec, w=w, floats=floats + [x, dvec, w], ints=ints))
            for c in callers:                                                   # each alone, under the null stream
                c["ints0"] = [t.clone() for t in c["ints"]]
                c["stage"] = [t.detach().clone() for t in c["floats"]]
                mask = forward(c["m"], c["x"], c["dvec"])
                (mask * c["w"]).sum().backward()
                c["want"] = keep(results(c["m"], mask))
                del mask                                                        # the graph goes: its nodes belong to the null stream
                torch.cuda.synchronize()
            for c in callers:
                _bring(c["ints"], c["ints0"])
                _poison(c["floats"])
            torch.cuda.synchronize()
            with held_streams(["two callers (b): training step 1", "two callers (b): training step 2"]) as (h1, h2):
                for c, h in zip(callers, (h1, h2)):
                    c["s"] = h.stream
                    with torch.cuda.stream(c["s"]):
                        _bring(c["floats"], c["stage"])
                h1.before(), h2.before()
                for c in callers:
                    with torch.cuda.stream(c["s"]):
                        c["mask"] = forward(c["m"], c["x"], c["dvec"])
                for c in callers:
                    with torch.cuda.stream(c["s"]):
                        (c["mask"] * c["w"]).sum().backward()
                        c["got"] = keep(results(c["m"], c["mask"]))
                h1.after(), h2.after()
                h1.stream.synchronize(), h2.stream.synchronize()
    finally:
        lib.vs_set_lstm_kernel(0)
    for i, c in enumerate(callers):
        assert_same(f"two callers (b): training step {i + 1}", c["got"], c["want"])
