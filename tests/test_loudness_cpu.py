"""CPU: the loudness contract of include/voicesplit_hip.h -- the host planner inside the library (vs_loudness_plan: coefficients,
sub-block length, the zero-input step) against the fp64 restatement (tests/loudness_ref.py) and the coefficient table of BS.1770,
what the entries refuse before any launch, the gain arithmetic on CPU tensors, the restatement's own calibration, and d_ref: how far
the segmented evaluation (the device's algorithm) is from the serial filter on the signals of the GPU tests."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loudness_ref as LR
from conftest import ROOT


def _plan(fs):
    from voicesplit_amd import loudness
    return loudness.plan(fs)


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def test_plan_gives_the_bs1770_table_at_48k():
    d = _plan(48000)
    assert d.sub == 4800 and d.sample_rate == 48000
    for name, want in LR.BS1770_48K.items():
        got = list(getattr(d, name))
        err = max(abs(g - w) for g, w in zip(got, want))
        print(f"{name}: max |plan - BS.1770 table| = {err:.2e} (bound 1e-12)")
        assert err <= 1e-12, (name, got, want)
    assert list(d.b2) == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("fs", LR.RATES)
def test_plan_equals_the_restatement(fs):
    d = _plan(fs)
    assert d.sub == LR.sub_block(fs) == (fs + 5) // 10
    for name, want in zip(("b1", "a1", "b2", "a2"), LR.coefficients(fs)):
        got = np.array(list(getattr(d, name)))
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"{fs} {name}: rel {rel:.2e} (bound 1e-15)")
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), (fs, name, got, want)
    step = np.array([list(r) for r in d.step])
    want = LR.step_matrix(fs)
    rel = np.abs(step - want).max() / np.abs(want).max()
    print(f"{fs} step: rel {rel:.2e} (bound 1e-12)")
    assert rel <= 1e-12


def test_plan_refuses_rates_outside_the_contract():
    from voicesplit_amd import _lib, loudness
    for fs in (7999, 192001, 0, -16000):
        with pytest.raises(_lib.VoiceSplitHipError, match="outside 8000"):
            loudness.plan(fs)
    with pytest.raises(ValueError, match="integers"):
        loudness.plan(44100.5)
    assert loudness.plan(8000).sub == 800 and loudness.plan(192000).sub == 19200
    assert _lib.load().vs_loudness_plan(16000, None) == -1 and b"NULL" in _lib.load().vs_last_error()


# ---- refusals before any launch -----------------------------------------------------------------------------------------------------
def _call(lib, d, table, total, ws_bytes, samples=256, out=256, ws=256, clips_dev=256):
    """vs_loudness with dummy device pointers that are never dereferenced: every call here is refused on the host."""
    t = (ctypes.c_longlong * len(table))(*table)
    p = lambda v: ctypes.c_void_p(v) if v else None
    rc = lib.vs_loudness(ctypes.byref(d), p(samples), total, t, p(clips_dev), len(table) // 2, p(out), p(out), p(out), p(out), None, None,
                         p(ws), ws_bytes, None)
    return rc, lib.vs_last_error()


def test_loudness_refusals():
    from voicesplit_amd import _lib
    lib, d = _lib.load(), _plan(16000)
    big = 1 << 40
    for kw in ({"samples": 0}, {"out": 0}, {"ws": 0}, {"clips_dev": 0}):
        rc, msg = _call(lib, d, [0, 100], 100, big, **kw)
        assert rc == -1 and b"NULL" in msg, (kw, msg)
    assert lib.vs_loudness(ctypes.byref(d), ctypes.c_void_p(256), 100, None, ctypes.c_void_p(256), 1, *([ctypes.c_void_p(256)] * 4), None, None,
                           ctypes.c_void_p(256), big, None) == -1 and b"NULL" in lib.vs_last_error()
    assert lib.vs_loudness(None, None, 0, None, None, 1, None, None, None, None, None, None, None, 0, None) == -1
    # energy without its offsets
    t = (ctypes.c_longlong * 2)(0, 100)
    one = ctypes.c_void_p(256)
    assert lib.vs_loudness(ctypes.byref(d), one, 100, t, one, 1, one, one, one, one, one, None, one, big, None) == -1
    assert b"energy_at" in lib.vs_last_error()
    # the clip table
    for table, text in (([0, 101], b"leaves the buffer"), ([-1, 10], b"leaves the buffer"), ([50, 51], b"leaves the buffer"),
                        ([0, 100, 100, 1], b"clip 1"), ([0, -1], b"0 .. 2^30")):
        rc, msg = _call(lib, d, table, 100, big)
        assert rc == -1 and text in msg, (table, msg)
    rc, msg = _call(lib, d, [0, (1 << 30) + 1], 1 << 31, big)
    assert rc == -1 and b"0 .. 2^30" in msg, msg
    # a short workspace: one byte less than the size function's answer for this very table
    total, N = 16000 * 9, 3
    need = lib.vs_loudness_workspace_bytes(ctypes.byref(d), total, N)
    assert need > 0 and need % 256 == 0
    table = [0, 48000, 48000, 48000, 96000, 48000]
    rc, msg = _call(lib, d, table, total, 255)
    assert rc == -1 and b"workspace too small" in msg, msg
    rc, msg = _call(lib, d, table, total, 0)
    assert rc == -1 and b"workspace too small" in msg, msg
    # N, dims that are not a plan, the size function's own refusals
    rc, msg = _call(lib, d, [], 100, big)
    assert rc == -1 and b"N=0" in msg
    bad = _lib.VsLoudnessDims.from_buffer_copy(d)
    bad.sub = 1601
    rc, msg = _call(lib, bad, [0, 100], 100, big)
    assert rc == -1 and b"vs_loudness_plan" in msg
    assert lib.vs_loudness_workspace_bytes(ctypes.byref(bad), 100, 1) == 0 and b"vs_loudness_plan" in lib.vs_last_error()
    assert lib.vs_loudness_workspace_bytes(ctypes.byref(d), -1, 1) == 0 and lib.vs_loudness_workspace_bytes(ctypes.byref(d), 100, 0) == 0
    assert lib.vs_loudness_workspace_bytes(None, 100, 1) == 0


def test_scale_clips_refusals():
    from voicesplit_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    t = (ctypes.c_longlong * 2)(0, 100)
    for args in ((None, 100, t, one, one, 1), (one, 100, None, one, one, 1), (one, 100, t, None, one, 1), (one, 100, t, one, None, 1)):
        assert lib.vs_scale_clips(*args, None) == -1 and b"NULL" in lib.vs_last_error(), args
    assert lib.vs_scale_clips(one, 100, t, one, one, 0, None) == -1 and b"N=0" in lib.vs_last_error()
    assert lib.vs_scale_clips(one, 99, t, one, one, 1, None) == -1 and b"leaves the buffer" in lib.vs_last_error()
    t = (ctypes.c_longlong * 2)(0, (1 << 30) + 1)
    assert lib.vs_scale_clips(one, 1 << 31, t, one, one, 1, None) == -1 and b"0 .. 2^30" in lib.vs_last_error()


def test_python_layer_refuses_the_cpu():
    from voicesplit_amd import _lib, loudness
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        loudness.LoudnessMeter(16000, "cpu")
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        loudness.normalize(torch.zeros(2, 16000), 16000)
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        loudness.scale_clips_(torch.zeros(10), torch.tensor([[0, 10]]), torch.ones(1))


# ---- the gain ------------------------------------------------------------------------------------------------------------------------
def test_gains_on_cpu_tensors():
    from voicesplit_amd import loudness
    lufs = torch.tensor([-30.0, -20.0, -30.0, float("-inf"), -23.0, -40.0], dtype=torch.float64)
    peak = torch.tensor([0.1, 0.1, 0.5, 0.2, 0.0, 0.3])
    valid = torch.tensor([1, 1, 1, 0, 1, 1], dtype=torch.int32)
    g = loudness.gains(lufs, peak, valid)
    assert g.dtype == torch.float32 and g.shape == (6,)
    cap = 10.0 ** (-2.0 / 20.0)
    want = [10.0 ** (7.0 / 20.0), 10.0 ** (-3.0 / 20.0), cap / float(np.float32(0.5)), 1.0, 1.0, cap / float(np.float32(0.3))]
    assert torch.equal(g, torch.tensor(want, dtype=torch.float64).to(torch.float32)), (g.tolist(), want)
    # the target: 7 dB up; the cap: 0.5 * 10^(7/20) would be 1.12, so the peak lands at -2 dBFS instead
    assert abs(float(g[2]) * 0.5 - cap) < 1e-7 and float(g[2]) < 10.0 ** (7.0 / 20.0)
    # no cap, another target
    g = loudness.gains(lufs, peak, valid, target=-16.0, peak_db=None)
    want = [10.0 ** (14.0 / 20.0), 10.0 ** (4.0 / 20.0), 10.0 ** (14.0 / 20.0), 1.0, 1.0, 10.0 ** (24.0 / 20.0)]
    assert torch.equal(g, torch.tensor(want, dtype=torch.float64).to(torch.float32))
    assert torch.isfinite(g).all()


# ---- header, signatures, ABI ---------------------------------------------------------------------------------------------------------
def test_header_signatures_and_abi():
    from voicesplit_amd import _lib
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    for name in ("vs_loudness_plan", "vs_loudness_workspace_bytes", "vs_loudness", "vs_scale_clips"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "NOT COMPARED WITH AN FFMPEG OR LIBEBUR128 RUN" in text and "not ffmpeg's `loudnorm` in its dynamic" in text
    assert "1681.974450955533" in text and "38.13547087602444" in text and "typedef struct vs_loudness_dims" in text
    assert re.search(r"#define\s+VS_ABI_VERSION\s+11\b", text)
    assert _lib.ABI_VERSION == 11 and _lib.load().vs_abi_version() == 11
    assert ctypes.sizeof(_lib.VsLoudnessDims) == 8 + 10 * 8 + 16 * 8
    assert "loudness.hip" in open(os.path.join(ROOT, "voicesplit_amd", "csrc", "Makefile")).read()


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", LR.RATES)
def test_reference_calibration_997_hz(fs):
    """A full-scale 997 Hz sine reads -3.01 LUFS; +- 0.1 LU is EBU Tech 3341's tolerance."""
    r = LR.serial(LR.sine(fs, 3.0), fs)
    print(f"{fs}: {r['lufs']:.4f} LUFS, counts {r['counts']}")
    assert r["valid"] == 1 and abs(r["lufs"] - (-3.01)) <= 0.1
    blocks = int(3.0 * fs) // LR.sub_block(fs) - 3
    assert r["counts"] == (blocks, blocks, blocks) and blocks in (26, 27)


def test_gate_signal_exercises_both_gates():
    """What the GPU gate test relies on: 34 blocks, 26-27 past the absolute gate, 15 past both, and the three candidate means (no gate,
    absolute only, both) more than 1 dB apart, so a missing gate shows."""
    for fs in LR.GATE_RATES:
        S = LR.sub_block(fs)
        for dc in LR.GATE_DC:
            r = LR.serial(LR.gate_clip(fs, dc), fs)
            e = r["energy"]
            z = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * S)
            means = [10 * np.log10(z.mean()), 10 * np.log10(z[z > LR.ABS_GATE].mean()), r["lufs"] + 0.691]
            print(f"{fs} dc {dc}: counts {r['counts']}, means {means[0]:.2f} / {means[1]:.2f} / {means[2]:.2f} dB")
            assert r["counts"][0] == 34 and r["counts"][1] in (26, 27) and r["counts"][2] == 15, r["counts"]
            assert means[1] - means[0] > 1.0 and means[2] - means[1] > 1.0


def test_segmented_against_serial_on_the_gpu_tests_signals():
    """d_ref: the largest |lufs(segmented) - lufs(serial)| over the signals of tests/test_gpu_loudness.py, printed (DESIGN.md 6.8i
    quotes it).  The GPU test's tolerance is max(64 d_ref, 1e-12 dB) and must stay below 1e-10 dB."""
    d_ref = 0.0
    for name, fs, x in LR.gpu_test_signals():
        a, b = LR.serial(x, fs), LR.segmented(x, fs)
        assert a["counts"] == b["counts"] and a["valid"] == b["valid"] and a["peak"] == b["peak"], name
        if a["valid"]:
            d_ref = max(d_ref, abs(a["lufs"] - b["lufs"]))
        else:
            assert a["lufs"] == b["lufs"] == -np.inf
        if len(a["energy"]):
            assert np.all(np.abs(a["energy"] - b["energy"]) <= 1e-12 * np.abs(a["energy"]).max()), name
    print(f"d_ref = {d_ref:.3e} dB")
    assert max(64 * d_ref, 1e-12) <= 1e-10
