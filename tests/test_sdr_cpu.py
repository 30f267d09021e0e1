"""CPU: the fp64 BSS-eval restatement (tests/bss_eval_ref.py) against its fixture and, when it is installed, against
mir_eval itself; argument checks of vs_sdr and of metrics.bss_sdr that run without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bss_eval_ref as R
from conftest import GOLDEN_DIR


def _fixture():
    return np.load(os.path.join(GOLDEN_DIR, "sdr_bss_eval.npz"))


def _groups(z):
    yield "demo", z["demo_ref"], z["demo_est"], z["demo_sdr"]
    for n in z["syn_lengths"]:
        yield f"syn{n}", z[f"syn{n}_ref"], z[f"syn{n}_est"], z[f"syn{n}_sdr"]


def test_restatement_reproduces_the_fixture():
    z = _fixture()
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    got, st = R.sdr_rows(clips["target"].astype(np.float32) / 32767.0, clips["mixed"].astype(np.float32) / 32767.0)
    assert not st.any() and np.allclose(got, z["demo_clips_sdr"], rtol=0, atol=1e-9)
    for name, ref, est, want in _groups(z):
        assert ref.dtype == est.dtype == np.float32
        got, st = R.sdr_rows(ref, est)
        assert not st.any(), name
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), name
        assert np.allclose(got[fin], want[fin], rtol=0, atol=1e-9), (name, got, want)
    # realistic values: the reference's own model output scores a few to ~16 dB against the clean speech
    assert 2.0 < z["demo_sdr"].min() and z["demo_sdr"].max() < 20.0


def test_restatement_rejects_silent_rows_and_shape_mismatch():
    x = np.random.default_rng(0).standard_normal(600).astype(np.float32)
    with pytest.raises(ValueError):
        R.sdr(np.zeros(600, np.float32), x)
    with pytest.raises(ValueError):
        R.sdr(x, np.zeros(600, np.float32))
    with pytest.raises(ValueError):
        R.sdr(x, x[:599])
    sdr, st = R.sdr_rows(np.stack([x, np.zeros_like(x)]), np.stack([x, x]))
    assert st.tolist() == [0, 1] and np.isnan(sdr[1]) and sdr[0] > 200


def test_restatement_matches_mir_eval_when_installed():
    sep = pytest.importorskip("mir_eval.separation")
    z = _fixture()
    for name, ref, est, want in _groups(z):
        for i in range(ref.shape[0]):
            if not np.isfinite(want[i]) or want[i] > 60:
                continue
            got = sep.bss_eval_sources(ref[i].astype(np.float64), est[i].astype(np.float64), False)[0][0]
            assert abs(got - want[i]) <= 1e-6, (name, i, got, want[i])


def test_vs_sdr_argument_errors_without_a_gpu():
    from voicesplit_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)                      # never dereferenced: every call below fails its argument checks first
    assert lib.vs_sdr_workspace_bytes(0, 100) == 0 and lib.vs_sdr_workspace_bytes(4, 0) == 0
    assert lib.vs_sdr_workspace_bytes(1, 1) > 0
    need = lib.vs_sdr_workspace_bytes(2, 1000)
    cases = [((p, p, 0, 1000, p, p, p, need), "B="), ((p, p, 2, 0, p, p, p, need), "N="),
             ((None, p, 2, 1000, p, p, p, need), "NULL"), ((p, p, 2, 1000, None, p, p, need), "NULL"),
             ((p, p, 2, 1000, p, None, p, need), "NULL"), ((p, p, 2, 1000, p, p, None, need), "NULL"),
             ((p, p, 2, 1000, p, p, p, need - 1), "workspace too small")]
    for args, msg in cases:
        assert lib.vs_sdr(*args, None) == -1, args
        assert msg in lib.vs_last_error().decode(), (args, lib.vs_last_error())


def test_bss_sdr_rejects_bad_dtype_and_shape():
    from voicesplit_amd import metrics
    x = torch.zeros(2, 100)
    with pytest.raises(TypeError):
        metrics.bss_sdr(x.double(), x)
    with pytest.raises(TypeError):
        metrics.bss_sdr(x, x.half())
    with pytest.raises(TypeError):
        metrics.bss_sdr(x.numpy(), x)
    with pytest.raises(ValueError):
        metrics.bss_sdr(x, torch.zeros(2, 99))
    with pytest.raises(ValueError):
        metrics.bss_sdr(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
