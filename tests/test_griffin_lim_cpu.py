"""CPU: the Griffin-Lim entry points (vs_griffin_lim, audio.griffin_lim) as far as they go without a device -- prototypes, argument
checks, Python dispatch with a stub library -- and the fp64 restatement the device tests compare against (tests/griffin_lim_ref.py):
its plain inverse, its monotone residual and the sensitivity cap on every test input."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import griffin_lim_ref as G
from conftest import ROOT
from oracle import reference_audio as RA


def _dims(B=2, T=21, hop=160, win=400):
    from voicesplit_amd import _lib
    return _lib.VsLossDims(B, T, 601, 1200, hop, win, -100.0, 20.0)


def test_prototypes_in_header_library_and_ctypes_table():
    from voicesplit_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("vs_griffin_lim_workspace_bytes", "vs_griffin_lim", "vs_set_griffin_lim_reframe"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+VS_ABI_VERSION\s+11\b", text)
    assert lib.vs_abi_version() == 11 == _lib.ABI_VERSION
    restype, args = _lib.SIGNATURES["vs_griffin_lim"]
    assert restype is ctypes.c_int and len(args) == 11 and args[4] is ctypes.c_float and args[5] is ctypes.c_int


def test_every_argument_check_returns_its_error_code():
    from voicesplit_amd import _lib
    lib = _lib.load()
    d = _dims()
    need = lib.vs_griffin_lim_workspace_bytes(ctypes.byref(d))
    assert need > 0 and need % 256 == 0 and need == lib.vs_audio_workspace_bytes(ctypes.byref(d))
    assert lib.vs_griffin_lim_workspace_bytes(ctypes.byref(_lib.VsLossDims(2, 21, 600, 1200, 160, 400, -100.0, 20.0))) == 0
    p, ws = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)        # never dereferenced: every call below is refused first

    def call(dims=d, spec=p, mask=None, init=p, power=1.0, n_iter=4, wav=p, res=None, w=ws, nbytes=need):
        rc = lib.vs_griffin_lim(ctypes.byref(dims), spec, mask, init, power, n_iter, wav, res, w, nbytes, None)
        return rc, lib.vs_last_error()

    for kw in ({"spec": None}, {"init": None}, {"wav": None}):
        rc, msg = call(**kw)
        assert rc == -1 and b"griffin_lim: NULL" in msg, (kw, msg)
    rc, msg = call(n_iter=-1)
    assert rc == -1 and b"n_iter=-1" in msg
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(power=bad)
        assert rc == -1 and b"power" in msg, bad
    rc, msg = call(w=None)
    assert rc == -1 and b"workspace" in msg
    rc, msg = call(nbytes=need - 1)
    assert rc == -1 and b"workspace too small" in msg
    rc, msg = call(w=ctypes.c_void_p((1 << 20) + 128))
    assert rc == -1 and b"misaligned" in msg
    short = _dims(T=4)                                              # 480 samples <= n_fft / 2
    rc, msg = call(dims=short, nbytes=1 << 30)
    assert rc == -1 and b"reflect padding" in msg
    rc, msg = call(dims=_dims(hop=400, win=400), nbytes=1 << 30)    # no overlap: the Hann envelope reaches 0
    assert rc == -1 and b"envelope" in msg
    rc, msg = call(dims=_lib.VsLossDims(0, 21, 601, 1200, 160, 400, -100.0, 20.0))
    assert rc == -1 and b"bad dims" in msg
    assert lib.vs_set_griffin_lim_reframe(3) == -1 and b"reframe" in lib.vs_last_error()
    assert lib.vs_set_griffin_lim_reframe(-1) == -1
    for mode in (1, 2, 0):
        assert lib.vs_set_griffin_lim_reframe(mode) == 0


def test_reference_without_iterations_is_spec2wav():
    x = G.inputs(3, 21)
    for b in range(3):
        spec, mask, phase = (x[k][b].astype(np.float64) for k in ("spec", "mask", "mixture"))
        ys, res = G.griffin_lim(G.target_magnitude(spec, mask, 1.0), phase, 0)
        want = RA.spec2wav(spec * mask, phase)
        assert ys.shape == (1, 160 * 20) and res.shape == (0,)
        assert np.abs(ys[0] - want).max() <= 1e-12 * np.abs(want).max()
    # the power is applied to the amplitude
    S1, S15 = G.target_magnitude(x["spec"][0].astype(np.float64)), G.target_magnitude(x["spec"][0].astype(np.float64), None, 1.5)
    assert np.allclose(S15, S1 ** 1.5, rtol=1e-14, atol=0)


@pytest.mark.parametrize("init", G.INITS)
@pytest.mark.parametrize("power", G.POWERS)
def test_clean_reference_residual_never_rises(init, power):
    for (ys, res), _ in G.runs(3, 21, init, power):
        assert res.shape == (60,) and ys.shape == (61, 160 * 20) and np.isfinite(ys).all()
        assert (np.diff(res) <= 1e-12).all(), np.diff(res).max()
        assert res[-1] < res[0]


def test_every_test_input_is_below_the_sensitivity_cap():
    """The tolerance rule must not hide a failure: twice the envelope of the perturbed fp64 runs stays below 5e-2."""
    worst = {}
    for case in G.cases():
        B, T, init, power, n = case
        tw, tr = G.tolerances(*case)
        print(case, "tol_wav", " ".join(f"{v:.2e}" for v in tw), "tol_res", " ".join(f"{v:.2e}" for v in tr))
        assert (tw < G.MAX_TOLERANCE).all(), (case, tw)
        if n:
            assert (tw > 0).all() and (tr > 0).all() and (tr < G.MAX_TOLERANCE).all(), (case, tw, tr)
            worst[n] = max(worst.get(n, 0.0), float(tw.max()))
    assert worst[60] > worst[4] > worst[1]        # the envelope grows with the iteration count: it is not a constant in disguise


@pytest.mark.parametrize("tag", list(G.GEOMETRIES))
def test_every_geometry_input_is_below_the_sensitivity_cap_and_its_residual_falls(tag):
    """The same two conditions on the inputs of the other STFT geometries (G.GEOMETRIES): the doubled envelope of the perturbed
    fp64 runs below the cap, the clean residual falling, inside (0, 1) as tests/test_gpu_griffin_lim.py asks of the device's.
    One exception, which that file allows for: at G1 (a 33-sample clip under 64-sample frames, so most of every frame is reflect
    padding and stft(istft(.)) is no orthogonal projection) the fp64 residual of item 0 from random angles creeps up once it has
    stalled, by 1.1e-5 (power 1) and 2.2e-4 (power 1.5).  From the mixture's phase it falls everywhere."""
    geom = G.GEOMETRIES[tag]
    B, T = G.GEOM_SHAPES[tag]
    n_fft, hop, win = geom
    assert G.inputs(B, T, geom)["spec"].shape == (B, T, n_fft // 2 + 1) and hop * (T - 1) > n_fft // 2
    assert G.inputs(B, T, geom)["spec"].max() > 0.5          # speech, not a pause
    for case in G.cases(geom):
        _, _, init, power, n, _ = case
        tw, tr = G.tolerances(*case)
        print(tag, case[:5], "tol_wav", " ".join(f"{v:.2e}" for v in tw), "tol_res", " ".join(f"{v:.2e}" for v in tr))
        assert (tw < G.MAX_TOLERANCE).all(), (case, tw)
        if n:
            assert (tw > 0).all() and (tr > 0).all() and (tr < G.MAX_TOLERANCE).all(), (case, tw, tr)
        ref_wav, ref_res = G.reference(*case)
        assert ref_wav.shape == (B, hop * (T - 1)) and ref_res.shape == (n, B) and np.isfinite(ref_wav).all()
    for init in G.INITS:
        for power in G.POWERS:
            for (ys, res), _ in G.runs(B, T, init, power, geom):
                assert res.shape == (max(G.GEOM_ITERS),) and res[-1] < res[0]
                assert (np.diff(res) <= 1e-12).all() or (tag == "G1" and init == "random" and np.diff(res).max() < 1e-3), (tag, init, power, res)
                assert (res > 0).all() and (res < 1.0).all(), (tag, init, power, res)


def test_default_geometry_cases_and_inputs_are_what_they_were():
    """The geometry argument changes nothing at 1200 / 160 / 400: the case list, and inputs / reference with and without it."""
    assert G.cases() == G.cases(G.DEFAULT_GEOM) and len(G.cases()) == 4 * (3 + 4 + 1) and all(len(c) == 5 for c in G.cases())
    assert G.audio_cfg() == G.AUDIO
    a, b = G.inputs(1, 5), G.inputs(1, 5, G.DEFAULT_GEOM)
    assert all(np.array_equal(a[k], b[k]) for k in ("spec", "mixture", "random")) and a["mask"] is None
    assert np.array_equal(a["spec"][0], RA.wav2spec(G._clips()[0][0, 16000:16000 + 640])[0].astype(np.float32))
    assert np.array_equal(G.reference(1, 5, "mixture", 1.0, 4)[0], G.reference(1, 5, "mixture", 1.0, 4, G.DEFAULT_GEOM)[0])
    cases, ids = G.geometry_cases()
    assert len(cases) == len(set(ids)) == 5 * 2 * 2 * 3 and ids[0] == "G1-B2-T4-random-p1.0-n0"


class _StubLib:
    """Stands in for the loaded library: records what the Python layer passes down."""

    def __init__(self):
        self.calls = []

    def vs_audio_workspace_bytes(self, d):
        return 256

    vs_griffin_lim_workspace_bytes = vs_audio_workspace_bytes

    def vs_wav_to_spec(self, d, wav, spec, phase, ws, n, stream):
        self.calls.append(("vs_wav_to_spec", {"spec": spec.value, "phase": phase.value}))
        return 0

    def vs_spec_to_wav(self, d, spec, mask, phase, wav, ws, n, stream):
        self.calls.append(("vs_spec_to_wav", {"spec": spec.value, "mask": mask.value, "phase": phase.value}))
        return 0

    def vs_griffin_lim(self, d, spec, mask, init, power, n_iter, wav, res, ws, n, stream):
        dd = d._obj
        count = dd.B * dd.T * dd.F
        self.calls.append(("vs_griffin_lim", {"spec": spec.value, "mask": mask.value, "init": init.value, "power": power, "n_iter": n_iter,
                                              "res": res.value, "dims": (dd.B, dd.T, dd.F, dd.n_fft, dd.hop, dd.win),
                                              "angles": np.ctypeslib.as_array((ctypes.c_float * count).from_address(init.value)).copy()}))
        return 0


@pytest.fixture
def stub(monkeypatch):
    from voicesplit_amd import _call
    lib = _StubLib()
    monkeypatch.setattr(_call._lib, "load", lambda path=None: lib)
    monkeypatch.setattr(_call, "dev_check", lambda t, name, dtype=torch.float32: None)
    monkeypatch.setattr(_call, "stream", lambda: None)
    monkeypatch.setattr(_call, "_SCRATCH", {})
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return lib


def test_spec_to_wav_and_griffin_lim_dispatch(stub):
    from voicesplit_amd import audio
    spec, phase, mask = torch.rand(2, 6, 601), torch.rand(2, 6, 601), torch.rand(2, 6, 601)
    # no phase: the reference's ap.inv_spectrogram(spec) = Griffin-Lim with the config's power and iteration count
    wav = audio.spec_to_wav(spec, None, G.AUDIO)
    (name, c), = stub.calls
    assert name == "vs_griffin_lim" and wav.shape == (2, 800)
    assert c["power"] == 1.5 and c["n_iter"] == 60 and c["spec"] == spec.data_ptr() and c["mask"] is None and c["res"] is None
    assert c["dims"] == (2, 6, 601, 1200, 160, 400)
    assert c["angles"].min() >= 0.0 and c["angles"].max() < 6.2832 and c["angles"].std() > 1.0      # 2 pi U[0, 1)
    # with a phase: exactly the existing call
    stub.calls.clear()
    audio.spec_to_wav(spec, phase, G.AUDIO, mask=mask)
    assert stub.calls == [("vs_spec_to_wav", {"spec": spec.data_ptr(), "mask": mask.data_ptr(), "phase": phase.data_ptr()})]
    # griffin_lim's own arguments override the config; a seeded generator fixes the starting angles; the residual is [n_iter, B] fp64
    stub.calls.clear()
    g = torch.Generator().manual_seed(5)
    _, res = audio.griffin_lim(spec, G.AUDIO, n_iter=7, power=1.0, mask=mask, generator=g, return_residual=True)
    a = stub.calls[0][1]
    assert (a["n_iter"], a["power"], a["mask"]) == (7, 1.0, mask.data_ptr()) and res.shape == (7, 2) and res.dtype == torch.float64
    assert a["res"] == res.data_ptr()
    audio.spec_to_wav(spec, None, G.AUDIO)
    audio.griffin_lim(spec, G.AUDIO, generator=torch.Generator().manual_seed(5))
    assert np.array_equal(stub.calls[-1][1]["angles"], a["angles"]) and not np.array_equal(stub.calls[-2][1]["angles"], a["angles"])
    stub.calls.clear()
    audio.griffin_lim(spec, G.AUDIO, init_phase=phase)
    assert stub.calls[0][1]["init"] == phase.data_ptr()
    with pytest.raises(ValueError, match="shape of spec"):
        audio.griffin_lim(spec, G.AUDIO, init_phase=phase[:1].contiguous())
    with pytest.raises(KeyError):
        audio.griffin_lim(spec, {k: v for k, v in G.AUDIO.items() if k != "griffin_lim_iters"})


def test_separate_dispatches_on_refine_iters(stub):
    from voicesplit_amd import audio
    mask = torch.rand(2, 6, 601)
    wav, dvec = torch.rand(2, 800), torch.rand(2, 256)
    model = lambda spec, dvec: mask
    audio.separate(model, wav, dvec, G.AUDIO)
    (n0, front), (n1, back) = stub.calls
    assert (n0, n1) == ("vs_wav_to_spec", "vs_spec_to_wav")
    assert back == {"spec": front["spec"], "mask": mask.data_ptr(), "phase": front["phase"]}
    stub.calls.clear()
    audio.separate(model, wav, dvec, G.AUDIO, refine_iters=3)
    (n0, front), (n1, back) = stub.calls
    assert (n0, n1) == ("vs_wav_to_spec", "vs_griffin_lim")
    assert (back["spec"], back["mask"], back["init"]) == (front["spec"], mask.data_ptr(), front["phase"])
    assert back["power"] == 1.0 and back["n_iter"] == 3


def test_default_config_carries_the_reference_fields():
    import voicesplit_amd as V
    a = V.default_config().audio["voicefilter"]
    assert a["power"] == 1.5 and a["griffin_lim_iters"] == 60
