"""numpy restatements of the FFT form of the per-row FIR (voicesplit_amd/csrc/fir_fft.hip; a helper module, not a test).  The
contract is the text in include/voicesplit_hip.h.

``fir64(..)``            the exact sum in fp64: ``reverb_ref.fir``'s definition, y[i] = sum_{k < nh} h[k] x(at + i - k);
``partitioned32(..)``    the contract's partitioned overlap-save form in float32 through ``scipy.fft`` (pocketfft keeps float32),
                         with the block Bk as a parameter: H_p = rfft(h[p Bk .. (p + 1) Bk) padded to N = 2 Bk), windows
                         w_q = x(at + (q - 1) Bk .. at + (q + 1) Bk), y_j = the last Bk samples of irfft(sum_p rfft(w_{j-p}) H_p),
                         p ascending from zero;
``block_energy(..)``     E_j = sum_p ||w_{j-p}||_2 ||h_p||_2 in fp64, one number per output block;
``bound(E, L, Bk, k)``   the contract's bound per output, k 2^-24 log2(N) E_j;
``cases()``              the rows tests/test_gpu_fir_fft.py judges, each with its fp64 sum, its float32 restatement and its E_j,
                         computed once;
``kappa_ref()``          the largest |y32_ref - y64| / (2^-24 log2(N) E_j) over those rows at Bk = 2048: what pocketfft's float32
                         transforms need.  It is computed from the reference alone, never from the kernel; the kernel is held to
                         KAPPA_MARGIN = 8 times that (its radix order, its real-transform split and its table differ from
                         pocketfft's, and two fp32 orderings of one transform differ by a small factor in their worst element; a
                         table from fp32 sincos or a dropped partition lands far outside);
``batch(..)``            ``reverb_ref.batch`` with this form's bound in place of the direct form's.
x(p) = flat[p] for lo <= p < at + L, else 0."""
import functools
import math
from unittest import mock

import numpy as np
import scipy.fft as sfft

import reverb_ref as RR

BK = 2048
KAPPA_MARGIN = 8.0
TOTAL = 20000
FILTERS = (1, BK - 1, BK, BK + 1, 3 * BK + 5)             # the table of five responses
LENGTHS = (BK // 2 + 3, 2 * BK + 17)
LONG_NH, LONG_L = 32768, BK + 5                          # the long response: P = 16


def fir64(flat, at, lo, L, h, nh):
    return RR.fir(flat, at, lo, L, h, nh)[0]


def _x(flat, at, lo, L, first, count):
    """x(first .. first + count) as float32."""
    out = np.zeros(count, dtype=np.float32)
    a, b = max(first, lo), min(first + count, at + L)
    if b > a:
        out[a - first:b - first] = flat[a:b]
    return out


def _partitions(h, nh, Bk):
    P = -(-nh // Bk)
    hz = np.zeros(P * Bk, dtype=np.float32)
    hz[:nh] = np.asarray(h[:nh], dtype=np.float32)
    return hz.reshape(P, Bk)


def partitioned32(flat, at, lo, L, h, nh, Bk=BK):
    flat = np.asarray(flat)
    assert flat.dtype == np.float32
    N, J = 2 * Bk, -(-L // Bk)
    parts = _partitions(h, nh, Bk)
    H = [sfft.rfft(np.concatenate([p, np.zeros(Bk, dtype=np.float32)])) for p in parts]
    X = {q: sfft.rfft(_x(flat, at, lo, L, at + (q - 1) * Bk, N)) for q in range(-(len(parts) - 1), J)}
    assert H[0].dtype == np.complex64 and X[0].dtype == np.complex64
    y = np.zeros(J * Bk, dtype=np.float32)
    for j in range(J):
        acc = np.zeros(Bk + 1, dtype=np.complex64)
        for p in range(len(parts)):
            acc = acc + X[j - p] * H[p]
        out = sfft.irfft(acc, n=N)
        assert out.dtype == np.float32
        y[j * Bk:(j + 1) * Bk] = out[Bk:]
    return y[:L]


def block_energy(flat, at, lo, L, h, nh, Bk=BK):
    flat = np.asarray(flat)
    N, J = 2 * Bk, -(-L // Bk)
    hn = np.sqrt((_partitions(h, nh, Bk).astype(np.float64) ** 2).sum(axis=1))
    wn = {q: math.sqrt(float((_x(flat, at, lo, L, at + (q - 1) * Bk, N).astype(np.float64) ** 2).sum())) for q in range(-(len(hn) - 1), J)}
    return np.array([sum(wn[j - p] * hn[p] for p in range(len(hn))) for j in range(J)])


def bound(E, L, Bk, kappa):
    return np.repeat(kappa * 2.0 ** -24 * math.log2(2 * Bk) * np.asarray(E), Bk)[:L]


def ratio(y, y64, E, L, Bk):
    """max |y - y64| / (2^-24 log2(N) E_j) over the outputs; an output of a block with E_j = 0 must be exact."""
    unit = bound(E, L, Bk, 1.0)
    err = np.abs(np.asarray(y, dtype=np.float64) - y64)
    assert not err[unit == 0.0].any()
    return float((err[unit > 0.0] / unit[unit > 0.0]).max()) if (unit > 0.0).any() else 0.0


# ---- the rows of tests/test_gpu_fir_fft.py ----------------------------------------------------------------------------------------------
def rows(L):
    """three rows: an odd start with history back to sample 13; no history (lo = at, odd); the row that ends with the buffer, with
    100 samples of history"""
    return [7001, 9403, TOTAL - L], [13, 9403, TOTAL - L - 100]


@functools.lru_cache(maxsize=None)
def data():
    """(flat [TOTAL], h [5][3 Bk + 5], the long response [1][32768]) as float32: 0.1 randn samples, randn exp(-k / 300) taps (the
    long response decays over 6000 taps, so that its last partitions still hold something)."""
    rng = np.random.default_rng(17)
    flat = (0.1 * rng.standard_normal(TOTAL)).astype(np.float32)
    h = np.zeros((len(FILTERS), max(FILTERS)), dtype=np.float32)
    for r, n in enumerate(FILTERS):
        h[r, :n] = (rng.standard_normal(n) * np.exp(-np.arange(n) / 300.0)).astype(np.float32)
    long_h = (rng.standard_normal(LONG_NH) * np.exp(-np.arange(LONG_NH) / 6000.0)).astype(np.float32)[None]
    return flat, h, long_h


@functools.lru_cache(maxsize=None)
def cases():
    """{(r, L): [row dicts]} for the five responses and two lengths, and {("long", LONG_L): [one row]}; a row holds at, lo, y64, y32, E
    and, for the cross-check with the direct form, sum_k |h_k| |x_{n-k}|, max |x| and max |h|."""
    flat, h, long_h = data()
    out = {}

    def row(at, lo, L, taps, nh):
        y64, mag, mx, mh = RR.fir(flat, at, lo, L, taps, nh)
        return dict(at=at, lo=lo, L=L, nh=nh, y64=y64, mag=mag, mx=mx, mh=mh, y32=partitioned32(flat, at, lo, L, taps, nh),
                    E=block_energy(flat, at, lo, L, taps, nh))

    for r, nh in enumerate(FILTERS):
        for L in LENGTHS:
            out[(r, L)] = [row(a, l, L, h[r], nh) for a, l in zip(*rows(L))]
    out[("long", LONG_L)] = [row(TOTAL - LONG_L, 0, LONG_L, long_h[0], LONG_NH)]
    return out


@functools.lru_cache(maxsize=None)
def kappa_ref():
    return max(ratio(c["y32"], c["y64"], c["E"], c["L"], BK) for group in cases().values() for c in group)


# ---- one whole batch ---------------------------------------------------------------------------------------------------------------------
class _Mag(np.ndarray):
    """sum |h| |x| of a row, carrying the row's FFT-form bound to where reverb_ref.batch asks for it"""


def batch(flat, at, lo, hrow, nh, h, L, sir, kappa, Bk=BK):
    """``reverb_ref.batch`` for rows made by the FFT form: the same fp64 batch, with kappa 2^-24 log2(N) E_j as every row's FIR bound."""
    plain = RR.fir

    def fir(flat_, at_, lo_, L_, h_, nh_):
        y, mag, mx, mh = plain(flat_, at_, lo_, L_, h_, nh_)
        mag = mag.view(_Mag)
        mag.bound = bound(block_energy(flat_, at_, lo_, L_, h_, nh_, Bk), L_, Bk, kappa)
        return y, mag, mx, mh

    with mock.patch.object(RR, "fir", fir), mock.patch.object(RR, "fir_bound", lambda mag, *_: (mag.bound, 0.0)):
        return RR.batch(flat, at, lo, hrow, nh, h, L, sir, None, "fft")
