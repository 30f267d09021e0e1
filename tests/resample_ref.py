"""fp64 numpy restatement of the resampling contract in include/voicesplit_hip.h (a Kaiser-windowed sinc with resampy's kaiser_best
constants as remembered; restated, not compared with a resampy or librosa run).  Shared by tests/test_resample_cpu.py and
tests/test_gpu_resample.py."""
import math

import numpy as np
from scipy.special import i0

Z = 64
BETA = 14.769656459379492
RHO = 0.9475937167399596

PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 48000), (16000, 44100), (48000, 44100)]
# sr_in, sr_out -> L, M, T (the issue's table)
PLAN_TABLE = {(48000, 16000): (1, 3, 385), (44100, 16000): (160, 441, 355), (22050, 16000): (320, 441, 179), (8000, 16000): (2, 1, 129),
              (16000, 48000): (3, 1, 129), (16000, 44100): (441, 160, 129), (48000, 44100): (147, 160, 141)}


def plan(sr_in, sr_out):
    """(L, M, s, H, T); equal rates are a copy: H = 0, T = 1."""
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    if L == M == 1:
        return 1, 1, 1.0, 0, 1
    s = min(1.0, L / M)
    H = -(-Z * M // L) if M > L else Z                   # ceil(Z / s) in integers
    return L, M, s, H, 2 * H + 1


def h(t):
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) < Z
    u = np.where(inside, t / Z, 0.0)
    return np.where(inside, RHO * np.sinc(RHO * t) * i0(BETA * np.sqrt(1.0 - u * u)) / i0(BETA), 0.0)


_BANKS = {}


def bank(sr_in, sr_out):
    """[L, T] float64 (not rounded to fp32): bank[r, j + H] = s h(s (r / L - j))."""
    key = (sr_in, sr_out)
    if key not in _BANKS:
        L, M, s, H, T = plan(sr_in, sr_out)
        if H == 0:
            _BANKS[key] = np.ones((1, 1))
        else:
            r = np.arange(L, dtype=np.float64)[:, None]
            j = np.arange(-H, H + 1, dtype=np.float64)[None, :]
            _BANKS[key] = s * h(s * (r / L - j))
    return _BANKS[key]


def out_len(sr_in, sr_out, n_in):
    L, M = plan(sr_in, sr_out)[:2]
    return -(-n_in * L // M)


def window(buf, x_first, stream_len, y_first, y_count, sr_in, sr_out, with_A=False):
    """Outputs [y_first, y_first + y_count) of the streams of which buf [B, k] (or [k]) holds samples [x_first, x_first + k);
    stream_len None while the end is unknown.  Raises when an output needs a sample of the stream that the buffer does not hold.
    with_A: also A[n] = sum |tap x|."""
    buf = np.asarray(buf, dtype=np.float64)
    one = buf.ndim == 1
    buf = buf[None] if one else buf
    L, M, s, H, T = plan(sr_in, sr_out)
    taps = bank(sr_in, sr_out)
    y = np.zeros((buf.shape[0], y_count))
    A = np.zeros((buf.shape[0], y_count))
    jj = np.arange(-H, H + 1, dtype=np.int64)[None, :]
    step = max(1, 2_000_000 // T)
    for lo in range(0, y_count, step):
        n = np.arange(y_first + lo, y_first + min(y_count, lo + step), dtype=np.int64)          # n M in 64 bits
        b, r = (n * M) // L, (n * M) % L
        k = b[:, None] + jj
        exists = (k >= 0) & ((k < stream_len) if stream_len is not None else True)
        held = (k >= x_first) & (k < x_first + buf.shape[1])
        if np.any(exists & ~held):
            raise IndexError(f"outputs [{n[0]}, {n[-1]}] need stream samples outside the buffer [{x_first}, {x_first + buf.shape[1]})")
        idx = np.clip(k - x_first, 0, max(buf.shape[1] - 1, 0))
        for row in range(buf.shape[0]):
            xs = np.where(exists, buf[row][idx] if buf.shape[1] else 0.0, 0.0)
            prod = taps[r] * xs
            y[row, lo:lo + len(n)] = prod.sum(axis=1)
            A[row, lo:lo + len(n)] = np.abs(prod).sum(axis=1)
    if one:
        y, A = y[0], A[0]
    return (y, A) if with_A else y


def resample(x, sr_in, sr_out, with_A=False):
    """The whole signal x [n] or [B, n]: ceil(n L / M) outputs."""
    n_in = np.asarray(x).shape[-1]
    return window(x, 0, n_in, 0, out_len(sr_in, sr_out, n_in), sr_in, sr_out, with_A)


def fir(sr_in, sr_out):
    """The same filter as one FIR at the rate L sr_in, for scipy.signal.resample_poly: fir[m + H L] = s h(s m / L)."""
    L, M, s, H, T = plan(sr_in, sr_out)
    m = np.arange(-H * L, H * L + 1, dtype=np.float64)
    return s * h(s * m / L)
