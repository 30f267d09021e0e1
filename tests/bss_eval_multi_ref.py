"""fp64 numpy / scipy restatement of multi-source BSS-eval (SDR, SIR, SAR and the best permutation), in the form mir_eval's
``separation.bss_eval_sources`` implements the definition of Vincent, Gribonval, Fevotte (IEEE TASLP 14(4), 2006):

* FFT correlations of the zero-padded references with each other and with every estimate, lags 0 .. flen - 1 (flen = 512);
* the dense block matrix G (unknowns lag-major, source-minor: G[(a, i), (b, j)] = c_ij[a - b]) and ``np.linalg.solve`` for the
  all-source projection of every estimate; ``bss_eval_ref.project`` (a Toeplitz solve) for the single-source projections;
* ``fftconvolve`` for the projected signals; the criteria from the projected signals' norms, +inf for a zero denominator;
* the permutation that maximises the mean SIR, candidates in ``itertools.permutations`` order, the first maximum wins.

Also the recipe of the test inputs that the CPU and GPU tests share (``make_item`` / ``make_batch``).
Pure numpy / scipy: no GPU, no mir_eval (tests/test_bss_eval_cpu.py compares against it when it is installed).
"""
import itertools
import os

import numpy as np
from scipy.signal import fftconvolve, lfilter

import bss_eval_ref as R1

FLEN = R1.FLEN


def _correlations(ref, est, flen):
    """c[i, j, m] = sum_n s_i[n] s_j[n + m] for m = -(flen-1) .. flen-1 (index m + flen - 1); d[i, q, m] likewise, m >= 0."""
    K, n = ref.shape
    n_fft = int(2 ** np.ceil(np.log2(n + flen - 1.0)))
    sf = np.fft.fft(ref, n=n_fft, axis=1)
    ef = np.fft.fft(est, n=n_fft, axis=1)
    c = np.empty((K, K, 2 * flen - 1))
    d = np.empty((K, est.shape[0], flen))
    for i in range(K):
        for j in range(K):
            x = np.real(np.fft.ifft(np.conj(sf[i]) * sf[j]))
            c[i, j] = np.concatenate([x[-(flen - 1):], x[:flen]])
        for q in range(est.shape[0]):
            d[i, q] = np.real(np.fft.ifft(np.conj(sf[i]) * ef[q]))[:flen]
    return c, d


def project_all(ref, est, flen=FLEN):
    """P_all[q] [N + flen - 1]: the projection of every estimate on the span of all references delayed 0 .. flen - 1."""
    ref = np.asarray(ref, np.float64)
    est = np.asarray(est, np.float64)
    K, n = ref.shape
    c, d = _correlations(ref, est, flen)
    lag = np.arange(flen)[:, None] - np.arange(flen)[None, :] + flen - 1
    G = np.ascontiguousarray(np.transpose(c[:, :, lag], (2, 0, 3, 1)))          # G[a, i, b, j] = c_ij[a - b]
    D = np.transpose(d, (2, 0, 1)).reshape(flen * K, est.shape[0])              # D[(a, i), q] = d_iq[a]
    C = np.linalg.solve(G.reshape(flen * K, flen * K), D).reshape(flen, K, est.shape[0])
    sp = np.concatenate([ref, np.zeros((K, flen - 1))], axis=1)
    P = np.zeros((est.shape[0], n + flen - 1))
    for q in range(est.shape[0]):
        for i in range(K):
            P[q] += fftconvolve(C[:, i, q], sp[i])[: n + flen - 1]
    return P


def criteria(P_all_q, s_j, e_q, flen=FLEN):
    """(sdr, sir, sar) of estimate q against reference j, given the all-source projection of q."""
    P_j, ep, _ = R1.project(s_j, e_q, flen)
    return (R1.safe_db(float(np.sum(P_j ** 2)), float(np.sum((ep - P_j) ** 2))),
            R1.safe_db(float(np.sum(P_j ** 2)), float(np.sum((P_all_q - P_j) ** 2))),
            R1.safe_db(float(np.sum(P_all_q ** 2)), float(np.sum((ep - P_all_q) ** 2))))


def best_permutation(sir):
    """popt maximising sum_j sir[popt[j], j]: itertools.permutations order, the first maximum wins; (popt, sums)."""
    K = sir.shape[0]
    perms = list(itertools.permutations(range(K)))
    sums = np.empty(len(perms))
    for p, perm in enumerate(perms):
        acc = 0.0
        for j in range(K):
            acc += float(sir[perm[j], j])
        sums[p] = acc
    return np.array(perms[int(np.argmax(sums))], dtype=np.int32), sums


def bss_eval_item(ref, est, compute_permutation=True, flen=FLEN):
    """One item, ref and est [K, N]: (sdr [K], sir [K], sar [K], perm [K], pairs [3, K, K] indexed [criterion][estimate][reference]);
    ValueError for an all-zero row, as mir_eval's validate.  Without compute_permutation the off-diagonal pairs are NaN."""
    ref = np.atleast_2d(np.asarray(ref, np.float64))
    est = np.atleast_2d(np.asarray(est, np.float64))
    if ref.shape != est.shape:
        raise ValueError(f"reference shape {ref.shape} != estimate shape {est.shape}")
    K = ref.shape[0]
    for k in range(K):
        R1.validate(ref[k], est[k])
    P_all = project_all(ref, est, flen) if K > 1 else None
    pairs = np.full((3, K, K), np.nan)
    for q in range(K):
        for j in (range(K) if compute_permutation else [q]):
            Pq = P_all[q] if K > 1 else R1.project(ref[0], est[0], flen)[0]
            pairs[:, q, j] = criteria(Pq, ref[j], est[q], flen)
    if compute_permutation:
        perm, _ = best_permutation(pairs[1])
    else:
        perm = np.arange(K, dtype=np.int32)
    idx = np.arange(K)
    return pairs[0][perm, idx], pairs[1][perm, idx], pairs[2][perm, idx], perm, pairs


def bss_eval_batch(ref, est, compute_permutation=True, flen=FLEN):
    """[B, K, N] with the GPU's conventions: (sdr, sir, sar [B, K], perm [B, K], status [B], pairs [B, 3, K, K]); status 1 with
    NaN and perm -1 for an item that validate rejects."""
    B, K, _ = ref.shape
    sdr, sir, sar = (np.full((B, K), np.nan) for _ in range(3))
    perm = np.full((B, K), -1, np.int32)
    status = np.zeros(B, np.int32)
    pairs = np.full((B, 3, K, K), np.nan)
    for b in range(B):
        try:
            sdr[b], sir[b], sar[b], perm[b], pairs[b] = bss_eval_item(ref[b], est[b], compute_permutation, flen)
        except ValueError:
            status[b] = 1
    return sdr, sir, sar, perm, status, pairs


# ---------------------------------------------------------------------------------------------------------------------
# test inputs
def _signals(N):
    from conftest import GOLDEN_DIR
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    tgt = clips["target"].astype(np.float64)[:, 8000:8000 + N] / 32767.0
    mix = clips["mixed"].astype(np.float64)[:, 8000:8000 + N] / 32767.0
    out = []
    for i in range(4):
        out += [tgt[i], mix[i] - tgt[i]]                                       # [t0, i0, t1, i1, t2, i2, t3, i3]
    return out


def make_item(K, N, seed=None, roll=True):
    """(ref, est) fp32 [K, N]: K demo signals at rms 0.05; estimate q = gain * FIR16(s_q) + leaks of the others + noise, and
    the estimates rolled by one, so that the best permutation is (1, 2, .., K-1, 0)."""
    rng = np.random.default_rng(100 + K if seed is None else seed)
    sig = _signals(N)[:K]
    ref = np.stack([(0.05 * s / np.sqrt(np.mean(s ** 2))) for s in sig]).astype(np.float32)
    s = ref.astype(np.float64)
    est = np.empty((K, N))
    for q in range(K):
        fir = np.concatenate([[1.0], 0.3 * rng.standard_normal(15) * np.exp(-np.arange(15) / 4.0)])
        e = rng.uniform(0.5, 1.5) * lfilter(fir, [1.0], s[q])
        for j in range(K):
            if j != q:
                leak = rng.standard_normal(8) * np.exp(-np.arange(8) / 2.0)
                e = e + rng.uniform(0.05, 0.3) * lfilter(leak, [1.0], s[j])
        est[q] = e + 0.05 * np.std(s[q]) * rng.standard_normal(N)
    est = est.astype(np.float32)
    if roll:
        est = np.roll(est, 1, axis=0)                                           # est[k] estimates s_{k-1}: popt[j] = j + 1
    return ref, est


def make_batch(K, N, B=3):
    """Item 0 is the guarded recipe (seed 100 + K); the others are fresh seeds of the same recipe."""
    items = [make_item(K, N)] + [make_item(K, N, seed=1000 * b + 100 + K) for b in range(1, B)]
    return np.stack([r for r, _ in items]), np.stack([e for _, e in items])


def guards(sdr, sir, sar, perm, status, pairs):
    """What the issue asks of the restatement's values before the GPU's are looked at: status 0, every criterion <= 40 dB,
    and the best permutation's SIR sum at least K * 1 dB (mean: 1 dB) above the second best."""
    assert (status == 0).all(), status
    assert np.isfinite(pairs).all() and pairs.max() <= 40.0, pairs.max()
    K = pairs.shape[-1]
    for b in range(pairs.shape[0]):
        if K > 1:
            _, sums = best_permutation(pairs[b, 1])
            top = np.sort(sums / K)[::-1]
            assert top[0] - top[1] >= 1.0, (b, top[:2])
