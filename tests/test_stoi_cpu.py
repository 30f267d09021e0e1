"""CPU: the intelligibility contract of include/voicesplit_hip.h -- the host planner inside the library (vs_stoi_plan: constants and
band edges) against the fp64 restatement (tests/stoi_ref.py) and the pinned list, the restatement's own sanity, the distance between its
two forms on the signals of the GPU tests (what the GPU tolerances are derived from), the condition that no frame of those signals sits on
the keep threshold, and what the entries refuse before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import stoi_ref as SR
from conftest import ROOT

PINNED = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
          (109, 138), (138, 174), (174, 219))


def _plan():
    from voicesplit_amd import metrics
    return metrics.stoi_plan()


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def test_plan_band_edges_and_constants():
    d = _plan()
    got = tuple(zip(list(d.lo), list(d.hi)))
    assert got == PINNED, got
    assert SR.edges() == PINNED and SR.EDGES == PINNED
    assert (d.frame, d.hop, d.nfft, d.bands, d.seg) == (256, 128, 512, 15, 30) == (SR.W, SR.HOP, SR.NFFT, SR.J, SR.N)
    assert d.clip == 1.0 + 10.0 ** (15.0 / 20.0) == SR.CLIP and d.dyn_db == 40.0 == SR.DYN
    assert SR.EPS == 2.0 ** -52 == np.finfo(np.float64).eps
    w = SR.window()
    assert w.shape == (256,) and np.abs(w - np.hanning(258)[1:-1]).max() <= 1e-15 and w.min() > 0


def test_header_signatures_and_abi():
    from voicesplit_amd import _lib
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    for name in ("vs_stoi_plan", "vs_stoi_workspace_bytes", "vs_stoi"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "RESTATED, NOT\n * COMPARED WITH A PYSTOI RUN" in text and "typedef struct vs_stoi_dims" in text
    for lo, hi in PINNED:
        assert f"({lo},{hi})" in text
    assert re.search(r"#define\s+VS_ABI_VERSION\s+11\b", text)
    assert _lib.ABI_VERSION == 11 and _lib.load().vs_abi_version() == 11
    assert ctypes.sizeof(_lib.VsStoiDims) == 35 * 4 + 4 + 2 * 8
    assert "stoi.hip" in open(os.path.join(ROOT, "voicesplit_amd", "csrc", "Makefile")).read()
    for doc in ("README.md", "DESIGN.md", os.path.join("voicesplit_amd", "metrics.py")):
        assert "restated, not compared with a pystoi run" in " ".join(open(os.path.join(ROOT, doc)).read().split()), doc


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
def test_reference_sanity():
    """Identity, scale invariance, and both scores falling strictly as white noise goes from 20 to 5 to -5 dB SNR, on the synthetic
    harmonic speech with a silent gap at 8000 samples."""
    x = SR.clip(1)
    assert len(x) == 8000
    for form in (1, 2):
        same = SR.score(x, x, False, form)
        assert same["status"] == 0 and abs(same["d"] - 1.0) <= 1e-12
        quiet = SR.score(x, (0.01 * x.astype(np.float64)).astype(np.float32), False, form)
        print(f"form {form}: stoi(x, x) - 1 = {same['d'] - 1.0:.2e}, stoi(x, 0.01 x) - stoi(x, x) = {quiet['d'] - same['d']:.2e}")
        assert abs(quiet["d"] - same["d"]) <= 1e-12
        for extended in (False, True):
            d = [SR.score(x, SR.noisy(x, snr, 3), extended, form)["d"] for snr in SR.SNRS]
            print(f"form {form} extended {extended}: {d[0]:.3f} / {d[1]:.3f} / {d[2]:.3f} at 20 / 5 / -5 dB")
            assert 1.0 > d[0] > d[1] > d[2] > 0.0, d


def test_short_clip_is_status_1():
    x = SR.clip(3)
    for extended in (False, True):
        r = SR.score(x, SR.noisy(x, 5.0, 1), extended)
        assert (r["F"], r["Mk"], r["status"]) == (49, 26, 1) and r["d"] == 1e-5
    for name, x, y in SR.edge_pairs():
        r = SR.score(x, y)
        assert r["F"] == SR.frames_of(len(x)) == r["Mk"], name
        assert (r["status"], r["d"] == 1e-5) == ((1, True) if r["Mk"] < 30 else (0, False)), name
    assert [SR.frames_of(n) for n in SR.EDGE_LENGTHS] == [0, 1, 1, 2, 29, 30]


def test_clip_counts_are_what_the_gpu_test_is_about():
    for i, (n, _, F, Mk) in enumerate(SR.CLIPS):
        r = SR.score(SR.clip(i), SR.clip(i))
        assert (len(SR.clip(i)), r["F"], r["Mk"]) == (n, F, Mk), (i, r["F"], r["Mk"])


def test_form_distance_and_gate_margin_on_the_gpu_tests_signals():
    """The largest distance between the two forms over the inputs of tests/test_gpu_stoi.py, printed (DESIGN.md 7a-3 quotes it): the
    device tolerances are 64 times these, as measured there again.  And the condition that makes any comparison meaningful: no frame
    within 1e-6 dB of the keep threshold, in either form, with identical keep masks."""
    long = SR.score(*SR.long_pairs()[0][1:])
    assert long["F"] == 311 > 256 and long["F"] > long["Mk"] > 64 + 29 and long["status"] == 0, (long["F"], long["Mk"])
    dist_d, dist_env, margin = SR.form_distance(SR.gpu_test_pairs() + SR.edge_pairs() + SR.long_pairs())
    print(f"form 1 against form 2: max |d1 - d2| = {dist_d:.3e}, max relative envelope distance = {dist_env:.3e}, "
          f"smallest gate margin = {margin:.3f} dB")
    assert margin >= 1e-6
    assert 0.0 < 64 * dist_d <= 1e-10 and 0.0 < 64 * dist_env <= 1e-10


# ---- refusals before any launch -----------------------------------------------------------------------------------------------------
def _call(lib, d, table, total, ws_bytes, ref=256, est=256, out=256, ws=256, clips_dev=256, extended=0):
    """vs_stoi with dummy device pointers that are never dereferenced: every call here is refused on the host."""
    t = (ctypes.c_longlong * len(table))(*table)
    p = lambda v: ctypes.c_void_p(v) if v else None
    rc = lib.vs_stoi(ctypes.byref(d), p(ref), p(est), total, t, p(clips_dev), len(table) // 2, extended, p(out), p(out), p(out), None, None,
                     p(ws), ws_bytes, None)
    return rc, lib.vs_last_error()


def test_stoi_refusals():
    from voicesplit_amd import _lib
    lib, d = _lib.load(), _plan()
    big = 1 << 40
    for kw in ({"ref": 0}, {"est": 0}, {"out": 0}, {"ws": 0}, {"clips_dev": 0}):
        rc, msg = _call(lib, d, [0, 1000], 1000, big, **kw)
        assert rc == -1 and b"NULL" in msg, (kw, msg)
    one = ctypes.c_void_p(256)
    assert lib.vs_stoi(ctypes.byref(d), one, one, 1000, None, one, 1, 0, one, one, one, None, None, one, big, None) == -1
    assert b"NULL" in lib.vs_last_error()
    assert lib.vs_stoi(None, None, None, 0, None, None, 1, 0, None, None, None, None, None, None, 0, None) == -1
    assert lib.vs_stoi_plan(None) == -1 and b"NULL" in lib.vs_last_error()
    # envelopes without their offsets; a flag that is neither form
    t = (ctypes.c_longlong * 2)(0, 1000)
    assert lib.vs_stoi(ctypes.byref(d), one, one, 1000, t, one, 1, 0, one, one, one, one, None, one, big, None) == -1
    assert b"tob_at" in lib.vs_last_error()
    rc, msg = _call(lib, d, [0, 1000], 1000, big, extended=2)
    assert rc == -1 and b"extended" in msg
    # the clip table
    for table, text in (([0, 1001], b"leaves the buffers"), ([-1, 10], b"leaves the buffers"), ([500, 501], b"leaves the buffers"),
                        ([0, 1000, 1000, 1], b"clip 1"), ([0, -1], b"0 .. 2^24")):
        rc, msg = _call(lib, d, table, 1000, big)
        assert rc == -1 and text in msg, (table, msg)
    rc, msg = _call(lib, d, [0, (1 << 24) + 1], 1 << 25, big)
    assert rc == -1 and b"0 .. 2^24" in msg, msg
    # a short workspace: less than these clips need, and the size function's answer is enough for them
    total, R = 30000, 3
    need = lib.vs_stoi_workspace_bytes(ctypes.byref(d), total, R)
    assert need > 0 and need % 256 == 0
    table = [0, 10000, 10000, 10000, 20000, 10000]
    for short in (0, 255, 4096):
        rc, msg = _call(lib, d, table, total, short)
        assert rc == -1 and b"workspace too small" in msg, msg
    m = re.search(rb"need (\d+)", _call(lib, d, table, total, 0)[1])
    assert m and int(m.group(1)) <= need
    # R, dims that are not a plan, the size function's own refusals
    rc, msg = _call(lib, d, [], 1000, big)
    assert rc == -1 and b"R=0" in msg
    bad = _lib.VsStoiDims.from_buffer_copy(d)
    bad.lo[3] = 15
    rc, msg = _call(lib, bad, [0, 1000], 1000, big)
    assert rc == -1 and b"vs_stoi_plan" in msg
    assert lib.vs_stoi_workspace_bytes(ctypes.byref(bad), 1000, 1) == 0 and b"vs_stoi_plan" in lib.vs_last_error()
    assert lib.vs_stoi_workspace_bytes(ctypes.byref(d), -1, 1) == 0 and lib.vs_stoi_workspace_bytes(ctypes.byref(d), 1000, 0) == 0
    assert lib.vs_stoi_workspace_bytes(None, 1000, 1) == 0


def test_python_layer_refusals_without_a_device():
    from voicesplit_amd import _lib, metrics
    x = torch.zeros(2, 16000)
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        metrics.stoi(x, x)
    with pytest.raises(TypeError, match="float32"):
        metrics.stoi(x.double(), x.double())
    with pytest.raises(TypeError, match="tensor"):
        metrics.stoi(x.numpy(), x)
    with pytest.raises(ValueError, match="shape"):
        metrics.stoi(x, x[:, :-1])
    with pytest.raises(ValueError, match="expected"):
        metrics.stoi(x[None, None], x[None, None])
    with pytest.raises(ValueError, match="lengths"):
        metrics.stoi(x, x, lengths=[16000])
    with pytest.raises(ValueError, match="lengths"):
        metrics.stoi(x, x, lengths=[16000, 16001])
