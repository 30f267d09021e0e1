"""GPU: the wavernn and waveglow audio back ends (csrc/audio_codec.hip and the linear-target entries of griffin_lim.hip) against
the fp64 restatement tests/audio_backend_ref.py, with the bounds tests/test_gpu_audio.py and tests/griffin_lim_ref.py already use.
The restatement is not pinned to a run of the reference (its module docstring says why)."""
import os

import numpy as np
import pytest
import torch

import audio_backend_ref as A
import griffin_lim_ref as G

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(t):
    return t.cpu().double().numpy()


# ---- front end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.FRONT_CASES, ids=[f"{c[0]}-B{c[1]}-T{c[2]}-{c[4]}-a{c[5]}" for c in A.FRONT_CASES])
def test_front_end_decodes_to_the_restated_magnitude_and_phase(case):
    """Stored values decoded on the host in fp64: linear magnitude within 2e-5 ref + 3e-6 of the frame's maximum with the codec's
    floor on both sides, phase within 1e-3 on the bins above 1e-2 of the maximum."""
    from voicesplit_amd import audio
    tag, B, T, gain, name, a = case
    geom, c = G.GEOMETRIES[tag], A.front_codec(name, a)
    block = A.front_block(tag, name, a)
    assert audio.codec_of(block) == c
    x = A.clips(tag, B, T, gain)
    spec, phase = audio.wav_to_spec(_cuda(x), block)
    assert spec.shape == phase.shape == (B, T, geom[0] // 2 + 1)
    floor = A.effective_floor(c)
    for b in range(B):
        mag, ph = A.analysis(x[b], geom, a)
        got, ref = np.maximum(floor, A.decode(_np(spec[b]), c)), np.maximum(floor, mag)
        ratio = (np.abs(got - ref) / (2e-5 * ref + 3e-6 * mag.max(axis=1, keepdims=True))).max()
        strong = mag > 1e-2 * mag.max()
        dph = np.abs(np.angle(np.exp(1j * (_np(phase[b]) - ph))))[strong].max()
        print(f"{tag} B{B} T{T} {name} a={a} clip {b}: magnitude ratio {ratio:.3g}  phase {dph:.3g}")
        assert ratio <= 1.0 and dph < 1e-3


@pytest.mark.parametrize("tag,B,T,gain,name,a,n_mels", [("G4", 3, 9, 0.25, "log", 0.0, 80), ("G1", 3, 4, 1.0, "plain", 0.97, 7),
                                                        ("G1", 2, 9, 1.0, "symmetric4", 0.0, 7)])
def test_front_end_with_a_mel_basis(tag, B, T, gain, name, a, n_mels):
    """Decoded mel magnitudes within basis @ (2e-5 ref + 3e-6 rowmax) + (F + 2) 2^-24 (basis @ ref)."""
    from voicesplit_amd import audio
    geom, c = G.GEOMETRIES[tag], A.front_codec(name, a)
    block = dict(A.front_block(tag, name, a), mel_spec=True)
    block["n_mel_channels" if name == "log" else "num_mels"] = n_mels
    cfg = audio.resolve(block)
    basis = A.mel_basis(cfg["sample_rate"], geom[0], n_mels, cfg["mel_fmin"], cfg["mel_fmax"])
    assert np.array_equal(_np(audio.mel_basis(cfg, "cuda")), basis)
    x = A.clips(tag, B, T, gain)
    mel, phase = audio.wav_to_spec(_cuda(x), block)
    assert mel.shape == (B, T, n_mels) and phase.shape == (B, T, geom[0] // 2 + 1)
    assert torch.equal(mel, audio.wav_to_mel(_cuda(x), dict(block, mel_spec=False)))
    F, floor = geom[0] // 2 + 1, A.effective_floor(c)
    for b in range(B):
        mag, _ = A.analysis(x[b], geom, a)
        ref = mag @ basis.T
        bound = (2e-5 * mag + 3e-6 * mag.max(axis=1, keepdims=True)) @ basis.T + (F + 2) * U * ref
        got = np.maximum(floor, A.decode(_np(mel[b]), c))
        ratio = (np.abs(got - np.maximum(floor, ref)) / bound).max()
        print(f"{tag} mel {n_mels} {name} clip {b}: ratio {ratio:.3g}")
        assert A.top(c) is None or A.encode(ref, c).max() < A.top(c)
        assert ratio <= 1.0


# ---- projections alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,F,n_mels,M", [("basis", 513, 80, 27), ("basis", 33, 7, 5), ("pinv", 513, 80, 27)])
def test_projection_is_within_the_fma_chain_bound(which, F, n_mels, M):
    """fp32 inputs: within (K + 2) 2^-24 (|W| @ |in|) of the fp64 product, the floor applied after."""
    from voicesplit_amd import audio
    n_fft = 2 * (F - 1)
    basis = A.mel_basis(22050 if F == 513 else 1000, n_fft, n_mels, 0.0, 8000.0 if F == 513 else None)
    W = basis if which == "basis" else A.mel_pinv(basis)
    floor = 0.0 if which == "basis" else 1e-10
    if which == "pinv":
        assert (W < 0).any()
    x = np.abs(np.random.default_rng(F + M).standard_normal((M, W.shape[1]))).astype(np.float32) * (10.0 ** np.random.default_rng(M).uniform(-3, 1, (M, 1))).astype(np.float32)
    got = _np(audio.project(_cuda(x), _cuda(W), floor))
    assert got.shape == (M, W.shape[0])
    exact = x.astype(np.float64) @ W.T
    bound = (W.shape[1] + 2) * U * (np.abs(x.astype(np.float64)) @ np.abs(W).T)
    ref = np.maximum(float(np.float32(floor)), exact)                 # the floor is an fp32 argument; max is 1-Lipschitz
    print(f"{which} F={F}: worst ratio {(np.abs(got - ref) / np.maximum(bound, 1e-300)).max():.3g}")
    assert (np.abs(got - ref) <= bound).all()
    # a row's bits do not depend on the rows around it
    assert torch.equal(audio.project(_cuda(x[3:4]), _cuda(W), floor)[0], audio.project(_cuda(x), _cuda(W), floor)[3])


# ---- de-emphasis ----------------------------------------------------------------------------------------------------------------
def _de_sizes():
    L = 128                      # vs_deemphasis_block(): asserted below
    return [1, L - 1, L, L + 1, 2 * L + 3, 48000]


@pytest.mark.parametrize("a", [0.97, 0.98])
@pytest.mark.parametrize("N", _de_sizes())
def test_deemphasis_matches_lfilter_and_a_rows_bits_stand_alone(N, a):
    """|got - ref| <= 2^-24 |ref| + 64 d, ref = scipy.signal.lfilter in fp64, d = its distance to the restatement's segmented form
    at the kernel's block length; a row's bits equal alone, as row 0 or 2 of a batch of 3 and at a buffer offset of one float."""
    from voicesplit_amd import audio
    L = audio.deemphasis_block()
    assert L == 128
    speech = G._clips()[0]
    rows = speech[:3, :N].astype(np.float32)
    x = _cuda(rows)
    got = audio.deemphasis(x, a)
    assert got.shape == x.shape
    for b in range(3):
        xr = rows[b].astype(np.float64)
        ref = A.deemphasis(xr, a)
        d = A.segment_distance(xr, a, L)
        err = np.abs(_np(got[b]) - ref)
        print(f"N={N} a={a} row {b}: max err {err.max():.3g}  d {d:.3g}  worst ratio {(err / (U * np.abs(ref) + 64 * d + 1e-300)).max():.3g}")
        assert d < 5e-15 and (err <= U * np.abs(ref) + 64 * d).all()
        # the kernel's sums are the segmented restatement's, one rounding each: its fp64 values rounded once to fp32
        assert np.array_equal(got[b].cpu().numpy(), A.deemphasis_segmented(xr, a, L).astype(np.float32))
    alone = audio.deemphasis(x[1].contiguous(), a)
    assert alone.shape == (N,) and torch.equal(alone, got[1])
    for pos in (0, 2):
        batch = x[[0, 2, 0]].clone()
        batch[pos] = x[1]
        assert torch.equal(audio.deemphasis(batch.contiguous(), a)[pos], got[1])
    buf = torch.zeros(N + 1, device="cuda")
    buf[1:] = x[1]
    assert buf[1:].data_ptr() % 8 == 4 and torch.equal(audio.deemphasis(buf[1:], a), got[1])
    # and the forward filter undoes it up to fp32 rounding of both
    back = audio.preemphasis(got, a)
    assert torch.equal(back[:, :1], got[:, :1]) and (back - x).abs().max() <= 4 * U * float(got.abs().max()) + 1e-30


def test_preemphasis_is_the_fp64_difference_rounded_once():
    """Half an ulp of p (2^-24 |p|), not of x: the difference of two close samples is far smaller than either."""
    from voicesplit_amd import audio
    x = A.clips("G5", 2, 11, 0.25)
    for a in (0.97, 0.98):
        want = np.stack([A.preemphasis(r, a) for r in x])
        got = _np(audio.preemphasis(_cuda(x), a))
        assert (np.abs(got - want) <= U * np.abs(want) * (1 + 1e-9)).all()


# ---- inversion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,B,T,gain,name,a", [("G4", 2, 9, 0.25, "log", 0.0), ("G5", 2, 11, 0.25, "plain", 0.98), ("G1", 2, 4, 1.0, "plain", 0.97)])
def test_phase_given_inverse_of_a_decoded_magnitude(tag, B, T, gain, name, a):
    """(a) decode, then the iSTFT with the given phase, before de-emphasis: within 2e-5 max|ref| of the restatement; the decoded
    magnitude itself within an fp32 rounding of the fp64 decode."""
    from voicesplit_amd import audio
    geom, c = G.GEOMETRIES[tag], A.front_codec(name, a)
    block = A.front_block(tag, name, a)
    x = A.clips(tag, B, T, gain)
    pairs = [A.analysis(x[b], geom, a) for b in range(B)]
    spec = np.stack([A.encode(m, c) for m, _ in pairs]).astype(np.float32)
    phase = np.stack([p for _, p in pairs]).astype(np.float32)
    mag = audio.decode(_cuda(spec), block)
    want = A.decode(spec.astype(np.float64), c)
    assert (np.abs(_np(mag) - want) <= U * want * (1 + 1e-6)).all()
    wav = audio.mag_to_wav(mag, _cuda(phase), block)
    assert wav.shape == (B, geom[1] * (T - 1))
    for b in range(B):
        ref = A.inverse_with_phase(want[b], phase[b].astype(np.float64), geom)
        err = np.abs(_np(wav[b]) - ref).max() / np.abs(ref).max()
        print(f"{tag} {name} clip {b}: inverse err {err:.3g}")
        assert err <= 2e-5
    # the public call: the same stages, then de-emphasis where the block has one
    full = audio.spec_to_wav(_cuda(spec), _cuda(phase), block)
    assert torch.equal(full, audio.deemphasis(wav, a) if a else wav)
    # a mask multiplies the stored value, as in the voicefilter leg
    mask = torch.rand(spec.shape, generator=torch.Generator().manual_seed(5)).cuda()
    want_m = A.decode(spec.astype(np.float64) * _np(mask), c)           # the product is taken in fp64 too, as gl_target_kernel takes it
    assert (np.abs(_np(audio.decode(_cuda(spec), block, mask)) - want_m) <= U * want_m * (1 + 1e-6)).all()


@pytest.mark.parametrize("case,init,power,n_iter", A.gl_cases()[0], ids=A.gl_cases()[1])
def test_griffin_lim_on_a_linear_target(case, init, power, n_iter):
    """(b) the rule of griffin_lim_ref.tolerances with the pad mode as a parameter; both re-framing forms give the same bits."""
    from voicesplit_amd import _lib, audio
    tag, B, T, gain, pad, a = case
    geom = G.GEOMETRIES[tag]
    cfg = G.audio_cfg(geom)
    x = A.gl_inputs(tag, B, T, gain, a)
    mag, ph = _cuda(x["mag"]), _cuda(x[init])
    wav, res = audio.griffin_lim_mag(mag, cfg, n_iter=n_iter, power=power, init_phase=ph, pad=pad, return_residual=True)
    ref_wav, ref_res = A.reference(case, init, power, n_iter)
    tol_w, tol_r = A.tolerances(case, init, power, n_iter)
    assert wav.shape == ref_wav.shape and res.shape == ref_res.shape and (tol_w < A.MAX_TOLERANCE).all()
    for b in range(B):
        err = np.abs(_np(wav[b]) - ref_wav[b]).max() / np.abs(ref_wav[b]).max()
        rerr = np.abs(_np(res[:, b]) - ref_res[:, b]).max() if n_iter else 0.0
        print(f"{tag} {pad} {init} p{power} n{n_iter} item {b}: wav {err:.3g} (tol {tol_w[b]:.3g})  residual {rerr:.3g} (tol {tol_r[b]:.3g})")
        assert err <= tol_w[b] and rerr <= tol_r[b]
    if n_iter == 4:
        lib = _lib.load()
        try:
            _lib.check(lib.vs_set_griffin_lim_reframe(1), "vs_set_griffin_lim_reframe")
            other = audio.griffin_lim_mag(mag, cfg, n_iter=n_iter, power=power, init_phase=ph, pad=pad)
        finally:
            lib.vs_set_griffin_lim_reframe(0)
        assert torch.equal(other, wav)


def _foreign_blocks():
    return {"wavernn": A.wavernn_block(*G.GEOMETRIES["G1"], preemphasis=0.97, num_mels=7, griffin_lim_iters=3),
            "waveglow": A.waveglow_block(*G.GEOMETRIES["G1"], n_mel_channels=7, sample_rate=1000, mel_fmax=None, griffin_lim_iters=3)}


@pytest.mark.parametrize("backend", ["wavernn", "waveglow"])
@pytest.mark.parametrize("mel_spec", [False, True])
def test_inv_spectrogram_is_its_stages_composed_by_hand(backend, mel_spec):
    """(c) AudioProcessor.inv_spectrogram and spec_to_wav(spec, None, cfg): decode -> (mel -> linear) -> Griffin-Lim with the same
    angles -> de-emphasis; (d) mag_to_mel: decode -> project -> encode."""
    from voicesplit_amd import audio
    section = dict(_foreign_blocks(), backend=backend, mel_spec=mel_spec)
    ap = audio.AudioProcessor(section)
    cfg = ap.cfg
    assert ap.mel_spec is mel_spec and (ap.n_fft, ap.hop_length, ap.win_length) == G.GEOMETRIES["G1"]
    x = _cuda(A.clips("G1", 2, 9, 1.0))
    spec, phase = ap.get_spec_from_audio(x, return_phase=True)
    assert spec.shape == (2, 9, 7 if mel_spec else 33) and phase.shape == (2, 9, 33)
    assert ap.get_spec_from_audio(x[0]).shape == spec.shape[1:]                          # one clip, [time, freq]
    angles = 2.0 * np.pi * torch.rand(2, 9, 33, generator=torch.Generator().manual_seed(11)).cuda()
    mag = audio.decode(spec, cfg)
    if mel_spec:
        mag = audio.project(mag, audio.mel_pinv(cfg, "cuda"), 1e-10)
        assert torch.equal(mag, audio.mel_to_linear(audio.decode(spec, cfg), cfg))
    by_hand = audio.griffin_lim_mag(mag, cfg, n_iter=3, power=1.5, init_phase=angles, pad="reflect" if backend == "wavernn" else "zero")
    if backend == "wavernn":
        by_hand = audio.deemphasis(by_hand, 0.97)
    assert torch.equal(ap.inv_spectrogram(spec, init_phase=angles), by_hand)
    assert ap.inv_spectrogram(spec[1], init_phase=angles[1]).shape == by_hand.shape[1:]
    # spec_to_wav(spec, None, cfg) draws its angles from the generator: the same draw by hand
    gen = torch.Generator(device="cuda").manual_seed(21)
    drawn = 2.0 * np.pi * torch.rand(mag.shape, device="cuda", dtype=torch.float32, generator=gen)
    want = audio.griffin_lim_mag(mag, cfg, init_phase=drawn)
    want = audio.deemphasis(want, 0.97) if backend == "wavernn" else want
    assert torch.equal(audio.spec_to_wav(spec, None, section, generator=torch.Generator(device="cuda").manual_seed(21)), want)
    assert torch.isfinite(want).all() and want.shape == x.shape
    # (d)
    lin = ap.get_spec_from_audio(x) if not mel_spec else audio.wav_to_spec(x, dict(section, mel_spec=False))[0]
    mel = ap.mag_to_mel(lin)
    assert mel.shape == (2, 9, 7)
    assert torch.equal(mel, audio.encode(audio.project(audio.decode(lin, cfg), audio.mel_basis(cfg, "cuda")), cfg))
    assert torch.equal(ap.get_mel(x), audio.wav_to_mel(x, cfg))


# ---- unchanged bits -------------------------------------------------------------------------------------------------------------
def test_voicefilter_block_routes_to_the_same_bits():
    import voicesplit_amd as V
    from voicesplit_amd import audio
    c = V.default_config()
    block = c.audio["voicefilter"]
    assert audio.resolve(block) is block and audio.resolve(block) == dict(block)
    x = G.inputs(3, 21)
    spec, phase = _cuda(x["spec"][:2]), _cuda(x["mixture"][:2])
    wav = _cuda(G._clips()[0][:2, 16000:16000 + 160 * 20])
    ap = audio.AudioProcessor(c.audio)
    s0, p0 = audio.wav_to_spec(wav, block)
    s1, p1 = ap.get_spec_from_audio(wav, return_phase=True)
    s2, p2 = audio.wav_to_spec(wav, audio.resolve(c.audio))
    assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(s0, s2) and torch.equal(p0, p2)
    y0 = audio.spec_to_wav(spec, phase, block)
    assert torch.equal(y0, ap.inv_spectrogram(spec, phase)) and torch.equal(y0, audio.spec_to_wav(spec, phase, c.audio))
    g0 = audio.griffin_lim(spec, block, n_iter=3, init_phase=phase)
    assert torch.equal(g0, audio.griffin_lim(spec, c.audio, n_iter=3, init_phase=phase))
    block3 = dict(block, griffin_lim_iters=3)
    assert torch.equal(audio.griffin_lim(spec, block3, init_phase=phase), g0)
    assert torch.equal(audio.AudioProcessor(dict(c.audio, voicefilter=block3)).inv_spectrogram(spec, init_phase=phase), g0)
    # the DB01 codec through the new entries states the same decode (not the same bits: fp64 here, fp32 inside vs_spec_to_wav)
    lin = audio.decode(spec, block)
    want = G.target_magnitude(x["spec"][:2].astype(np.float64))
    assert (np.abs(_np(lin) - want) <= U * want * (1 + 1e-6)).all()
    assert np.abs(_np(audio.mag_to_wav(lin, phase, block)) - _np(y0)).max() <= 4e-5 * float(y0.abs().max())


# ---- surface --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [0, 2])
def test_separate_under_a_wavernn_block(refine):
    import voicesplit_amd as V
    from oracle import reference_forward as R
    from voicesplit_amd import audio
    dims = dict(num_freq=33, emb_dim=16, lstm_dim=24, fc1_dim=40, fc2_dim=33)
    m = V.VoiceSplit(V.default_config(**dims)).cuda().eval()
    block = _foreign_blocks()["wavernn"]
    wav = _cuda(A.clips("G1", 2, 9, 1.0))
    dvec = R.synthetic_inputs(2, 9, dims, 4)[1].cuda()
    est = audio.separate(m, wav, dvec, block, refine_iters=refine)
    assert est.shape == wav.shape and torch.isfinite(est).all()


def test_eval_batches_take_a_wavernn_config(tmp_path):
    from scipy.io import wavfile
    import voicesplit_amd as V
    from voicesplit_amd import config, evaluate
    c = V.default_config()
    c.audio.update(config.reference_audio_blocks())
    c.audio["backend"], c.audio["mel_spec"] = "wavernn", False
    c["dataset"] = {"format": {"emb": "*-emb.pt", "target_wav": "*-target.wav", "mixed_wav": "*-mixed.wav"}}
    c["test_config"] = {"batch_size": 2}
    clips = np.load(os.path.join(G.GOLDEN_DIR, "demo_clips.npz"))
    n = 200 * 10
    for i in range(2):
        stem = os.path.join(str(tmp_path), "%06d" % i)
        wavfile.write(stem + "-target.wav", 16000, clips["target"][i, 16000:16000 + n])
        wavfile.write(stem + "-mixed.wav", 16000, clips["mixed"][i, 16000:16000 + n])
        torch.save(torch.randn(256, generator=torch.Generator().manual_seed(i)), stem + "-emb.pt")
    batches = list(evaluate.eval_batches(c, evaluate.EvalDataset(c, str(tmp_path)), "cuda"))
    assert len(batches) == 1
    emb, target, mixed, seq_len, target_wav, phase = batches[0]
    assert mixed.shape == target.shape == phase.shape == (2, 11, 1025) and emb.shape == (2, 256) and target_wav.shape == (2, n)
    assert torch.isfinite(mixed).all() and float(mixed.min()) >= 0.0 and float(mixed.max()) <= 1.0 and seq_len.tolist() == [n, n]
