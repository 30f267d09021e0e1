"""GPU: vs_griffin_lim / audio.griffin_lim against the fp64 restatement of the reference loop (tests/griffin_lim_ref.py: restated
in numpy, not compared with a librosa run), on real speech.  The tolerance is that module's rule: twice the envelope of four fp64
runs perturbed by what tests/test_gpu_audio.py allows the two device transforms, below a cap of 5e-2."""
import functools

import numpy as np
import pytest
import torch

import griffin_lim_ref as G

pytestmark = pytest.mark.gpu
CASES = G.cases()
_ids = [f"B{B}-T{T}-{init}-p{power}-n{n}" for B, T, init, power, n in CASES]
GEOM_CASES, _geom_ids = G.geometry_cases()          # (B, T, init, power, n, geom) at G1 .. G5
ALL_CASES, _all_ids = CASES + GEOM_CASES, _ids + _geom_ids


def _geom(case):
    return case[5] if len(case) > 5 else G.DEFAULT_GEOM


def _dev(B, T, init, geom=G.DEFAULT_GEOM):
    x = G.inputs(B, T, geom)
    spec, phase = torch.from_numpy(x["spec"]).cuda(), torch.from_numpy(x[init]).cuda()
    mask = None if x["mask"] is None else torch.from_numpy(x["mask"]).cuda()
    return spec, phase, mask


@functools.lru_cache(maxsize=None)
def _run(case):
    """One device run of a case and its rerun -> (wav [B, S], residual [n, B], rerun wav) as fp64 / fp32 numpy."""
    from voicesplit_amd import audio
    B, T, init, power, n = case[:5]
    cfg = G.audio_cfg(_geom(case))
    spec, phase, mask = _dev(B, T, init, _geom(case))
    wav, res = audio.griffin_lim(spec, cfg, n_iter=n, power=power, init_phase=phase, mask=mask, return_residual=True)
    again = audio.griffin_lim(spec, cfg, n_iter=n, power=power, init_phase=phase, mask=mask)
    assert wav.shape == (B, cfg["hop_length"] * (T - 1)) and res.shape == (n, B) and res.dtype == torch.float64
    return wav.cpu().numpy(), res.cpu().numpy(), again.cpu().numpy()


@pytest.mark.parametrize("case", ALL_CASES, ids=_all_ids)
def test_waveform_and_residual_match_the_fp64_loop(case):
    B, T, init, power, n = case[:5]
    wav, res, _ = _run(case)
    ref_wav, ref_res = G.reference(*case)
    tol_wav, tol_res = G.tolerances(*case)
    assert (tol_wav < G.MAX_TOLERANCE).all()
    assert np.isfinite(wav).all() and np.isfinite(res).all()
    err = np.abs(wav.astype(np.float64) - ref_wav).max(axis=1) / np.abs(ref_wav).max(axis=1)
    rerr = np.abs(res - ref_res).max(axis=0) if n else np.zeros(B)
    print(f"{_all_ids[ALL_CASES.index(case)]}: wav err/tol " + " ".join(f"{e:.2e}/{t:.2e}" for e, t in zip(err, tol_wav))
          + " | residual err/tol " + " ".join(f"{e:.2e}/{t:.2e}" for e, t in zip(rerr, tol_res)))
    assert (err <= tol_wav).all(), (err, tol_wav)
    assert (rerr <= tol_res).all(), (rerr, tol_res)


@pytest.mark.parametrize("case", ALL_CASES, ids=_all_ids)
def test_rerun_is_bit_identical_and_finite(case):
    wav, res, again = _run(case)
    assert np.isfinite(wav).all() and np.isfinite(res).all()          # the all-zero-mask item included
    assert np.array_equal(wav, again)


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[4] > 1], ids=[i for i, c in zip(_all_ids, ALL_CASES) if c[4] > 1])
def test_residual_does_not_rise(case):
    """The fp64 residual never rises; the device's stays within the tolerance rule of it, so between two iterations it may rise by
    no more than both values' allowance.  At the other geometries the fp64 residual itself is allowed for: at G1 it creeps up by
    1e-5 .. 2e-4 from random angles (tests/test_griffin_lim_cpu.py), and the device may rise by that plus both allowances."""
    _, res, _ = _run(case)
    _, tol_res = G.tolerances(*case)
    rise = np.maximum(np.diff(G.reference(*case)[1], axis=0), 0.0) if len(case) > 5 else 0.0
    assert (np.diff(res, axis=0) <= rise + 2.0 * tol_res[None]).all(), np.diff(res, axis=0).max(axis=0)
    assert (res[-1] < res[0]).all() and (res > 0).all() and (res < 1.0).all()


@pytest.mark.parametrize("B,T,tag", [(1, 5, None), (3, 21, None), (2, 4, "G1"), (2, 12, "G2")],
                         ids=["1-5", "3-21", "G1-2-4", "G2-2-12"])
def test_no_iteration_at_power_one_is_spec_to_wav(B, T, tag):
    from voicesplit_amd import audio
    geom = G.GEOMETRIES[tag] if tag else G.DEFAULT_GEOM
    cfg = G.audio_cfg(geom)
    spec, phase, mask = _dev(B, T, "mixture", geom)
    if mask is None:
        mask = torch.rand(spec.shape, generator=torch.Generator().manual_seed(3)).cuda()
    got = audio.griffin_lim(spec, cfg, n_iter=0, power=1.0, init_phase=phase, mask=mask)
    want = audio.spec_to_wav(spec, phase, cfg, mask=mask)
    assert (got - want).abs().max().item() <= 2e-5 * want.abs().max().item()
    wav, res = audio.griffin_lim(spec, cfg, n_iter=0, power=1.0, init_phase=phase, mask=mask, return_residual=True)
    assert torch.equal(wav, got) and res.shape == (0, B)


def test_spec_to_wav_without_a_phase_is_griffin_lim_with_the_config():
    from voicesplit_amd import audio
    spec, _, mask = _dev(3, 21, "mixture")
    torch.cuda.manual_seed(11)                                        # spec_to_wav takes no generator: the device's default one
    a = audio.spec_to_wav(spec, None, G.AUDIO, mask=mask)
    torch.cuda.manual_seed(11)
    b = audio.griffin_lim(spec, G.AUDIO, mask=mask)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    # an explicit seeded generator: the same angles, the same samples; another seed, another waveform
    c = audio.griffin_lim(spec, G.AUDIO, mask=mask, generator=torch.Generator(device="cuda").manual_seed(12))
    d = audio.griffin_lim(spec, G.AUDIO, n_iter=60, power=1.5, mask=mask, generator=torch.Generator(device="cuda").manual_seed(12))
    assert torch.equal(c, d) and not torch.equal(c, a)


def test_separate_with_and_without_refinement():
    from voicesplit_amd import audio
    _, mixed = G._clips()
    wav = torch.from_numpy(mixed[:3, 16000:16000 + 160 * 20].astype(np.float32)).cuda()
    dvec = torch.zeros(3, 256).cuda()
    model = lambda spec, dvec: torch.sigmoid(6.0 * spec - 3.0)          # a deterministic stand-in for the mask network
    spec, phase = audio.wav_to_spec(wav, G.AUDIO)
    mask = model(spec, dvec)
    today = audio.spec_to_wav(spec, phase, G.AUDIO, mask=mask)
    assert torch.equal(audio.separate(model, wav, dvec, G.AUDIO), today)
    assert torch.equal(audio.separate(model, wav, dvec, G.AUDIO, refine_iters=0), today)
    want = audio.griffin_lim(spec, G.AUDIO, n_iter=4, power=1.0, init_phase=phase, mask=mask)
    got = audio.separate(model, wav, dvec, G.AUDIO, refine_iters=4)
    assert torch.equal(got, want) and not torch.equal(got, today) and torch.isfinite(got).all()
    # the refinement moves towards a consistent spectrogram: its magnitude is closer to the masked one than the plain inverse's
    _, res = audio.griffin_lim(spec, G.AUDIO, n_iter=5, power=1.0, init_phase=phase, mask=mask, return_residual=True)
    assert (res[4] < res[0]).all()


def test_separate_refines_the_real_model_end_to_end():
    import voicesplit_amd as V
    from voicesplit_amd import audio
    _, mixed = G._clips()
    m = V.VoiceSplit(V.default_config()).cuda().eval()
    wav = torch.from_numpy(mixed[:2, 16000:16000 + 160 * 20].astype(np.float32)).cuda()
    dvec = torch.randn(2, 256, generator=torch.Generator().manual_seed(4)).cuda()
    est = audio.separate(m, wav, dvec, V.default_config().audio["voicefilter"], refine_iters=2)
    assert est.shape == wav.shape and torch.isfinite(est).all()


def _reframing_forms(B, T, geom):
    from voicesplit_amd import _lib, audio
    lib = _lib.load()
    cfg = G.audio_cfg(geom)
    spec, phase, mask = _dev(B, T, "random", geom)
    out = {}
    try:
        for mode in (1, 2, 0):
            assert lib.vs_set_griffin_lim_reframe(mode) == 0
            out[mode] = audio.griffin_lim(spec, cfg, n_iter=4, power=1.5, init_phase=phase, mask=mask, return_residual=True)
    finally:
        lib.vs_set_griffin_lim_reframe(0)
    assert torch.equal(out[1][0], out[2][0]) and torch.equal(out[0][0], out[1][0])
    assert (out[1][1] - out[2][1]).abs().max().item() < 1e-12


def test_both_reframing_forms_give_the_same_bits():
    """vs_set_griffin_lim_reframe: overlap-add + framing through the waveform against the one-launch gather."""
    _reframing_forms(3, 21, G.DEFAULT_GEOM)


@pytest.mark.parametrize("tag", ["G1", "G3"])
def test_both_reframing_forms_give_the_same_bits_at_other_geometries(tag):
    """G1: the reflection at its limit (S = n_fft / 2 + 1, the reflected index lands on S - 1 and on 0); G3: an odd window."""
    _reframing_forms(*G.GEOM_SHAPES[tag], G.GEOMETRIES[tag])


def test_device_tensors_only():
    from voicesplit_amd import _lib, audio
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        audio.griffin_lim(torch.rand(1, 5, 601), G.AUDIO)
    with pytest.raises(_lib.VoiceSplitHipError, match="griffin_lim"):
        audio.griffin_lim(torch.rand(1, 4, 601).cuda(), G.AUDIO, n_iter=1)      # 480 samples: shorter than the reflect padding
