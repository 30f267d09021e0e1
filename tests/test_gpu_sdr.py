"""GPU: metrics.bss_sdr (vs_sdr: fp64 correlations, Levinson solve, fp64 projection) against the fp64 restatement of
mir_eval's single-source BSS-eval (tests/bss_eval_ref.py) -- fixture rows, a B = 64 x 3 s batch of realistic variants,
a 2^22-sample row, silent rows, and bitwise reproducibility."""
import os

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

import bss_eval_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def _gpu(ref, est):
    from voicesplit_amd import metrics
    sdr, st = metrics.bss_sdr(torch.from_numpy(np.ascontiguousarray(ref, np.float32)).cuda(),
                              torch.from_numpy(np.ascontiguousarray(est, np.float32)).cuda())
    return sdr.cpu().numpy(), st.cpu().numpy()


def _agree(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if w <= 60:
            assert abs(g - w) <= 1e-6, (what, i, g, w)
        else:
            assert w >= 200 and g >= 100, (what, i, g, w)      # est = ref: roundoff-limited on both sides


def test_fixture_rows_match_the_restatement():
    z = np.load(os.path.join(GOLDEN_DIR, "sdr_bss_eval.npz"))
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    groups = [("demo_clips", clips["target"].astype(np.float32) / 32767.0, clips["mixed"].astype(np.float32) / 32767.0,
               z["demo_clips_sdr"]), ("demo", z["demo_ref"], z["demo_est"], z["demo_sdr"])]
    groups += [(f"syn{n}", z[f"syn{n}_ref"], z[f"syn{n}_est"], z[f"syn{n}_sdr"]) for n in z["syn_lengths"]]
    for name, ref, est, want in groups:
        got, st = _gpu(ref, est)
        assert (st == 0).all(), (name, st)
        _agree(got, want, name)


def _demo_batch(B=64, N=48000, seed=5):
    """Realistic rows from the demo clips: gains, FIR-filtered and noisy variants of the target as estimates, and the
    mixture itself."""
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    tgt = clips["target"][:, :N].astype(np.float64) / 32767.0
    mix = clips["mixed"][:, :N].astype(np.float64) / 32767.0
    rng = np.random.default_rng(seed)
    ref, est = np.empty((B, N), np.float32), np.empty((B, N), np.float32)
    for b in range(B):
        i = b % 4
        s = tgt[i]
        kind = (b // 4) % 4
        if kind == 0:
            e = mix[i] * rng.uniform(0.5, 2.0)
        elif kind == 1:
            fir = rng.standard_normal(32) * np.exp(-np.arange(32) / 5.0)
            e = lfilter(fir, [1.0], s) + 10 ** rng.uniform(-3, -1) * np.std(s) * rng.standard_normal(N)
        elif kind == 2:
            e = rng.uniform(0.3, 3.0) * s + rng.uniform(0.01, 0.5) * (mix[i] - s)
        else:
            e = 0.7 * s + 0.05 * np.std(s) * rng.standard_normal(N)
        ref[b], est[b] = s, e
    return ref, est


def test_b64_batch_and_a_2_22_row_match_the_restatement():
    ref, est = _demo_batch()
    got, st = _gpu(ref, est)
    want, wst = R.sdr_rows(ref, est)
    assert (st == 0).all() and (wst == 0).all()
    _agree(got, want, "b64")
    rng = np.random.default_rng(11)
    n = 1 << 22
    s = lfilter([1.0], [1.0, -1.2, 0.5], rng.standard_normal(n)).astype(np.float32)
    e = (lfilter([0.8, 0.1, -0.05], [1.0], s) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    got, st = _gpu(s, e)
    assert st.tolist() == [0]
    _agree(got, [R.sdr(s, e)], "2^22")


def test_silent_rows_get_nan_and_status_1_and_leave_the_others_alone():
    ref, est = _demo_batch(B=8, N=20000)
    base, st0 = _gpu(ref, est)
    assert (st0 == 0).all()
    ref2, est2 = ref.copy(), est.copy()
    ref2[2] = 0.0
    est2[5] = 0.0
    ref2[7] = 0.0
    est2[7] = 0.0
    got, st = _gpu(ref2, est2)
    assert st.tolist() == [0, 0, 1, 0, 0, 1, 0, 1]
    assert np.isnan(got[[2, 5, 7]]).all()
    keep = [0, 1, 3, 4, 6]
    assert np.array_equal(got[keep], base[keep])                  # bitwise


def test_repeatable_bitwise_and_independent_of_the_batch():
    ref, est = _demo_batch(B=16, N=48000, seed=9)
    a, sa = _gpu(ref, est)
    b, sb = _gpu(ref, est)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    one = np.array([_gpu(ref[i], est[i])[0][0] for i in range(16)])
    assert np.array_equal(a, one)
    # 1-D input, fp32 only, shapes must agree
    from voicesplit_amd import metrics
    x = torch.from_numpy(ref[0]).cuda()
    with pytest.raises(TypeError):
        metrics.bss_sdr(x.double(), x.double())
    with pytest.raises(ValueError):
        metrics.bss_sdr(x, x[:-1])
