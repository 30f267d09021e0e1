"""fp64 restatement of the intelligibility contract of include/voicesplit_hip.h (STOI and ESTOI at 10 kHz: pystoi's algorithm as
remembered, not compared with a pystoi run), in two forms that differ in how the sums that dominate the rounding are ordered:

    form 1   np.fft.rfft for the 512-point DFT, every sum in natural order
    form 2   an explicit cosine / sine matrix product with the samples reversed, the frame energies summed over reversed samples and
             the band sums taken over reversed bins, one bin at a time

``score(x, y, extended, form)`` returns a dict: d, status, F, Mk, X, Y ([15][Mk] envelopes), margin (the smallest
|max(e) - 40 - e_f| in dB: how far the nearest frame is from the keep threshold).  The signals of the GPU tests are built here too, so
that the CPU test can measure the distance between the two forms on exactly them.
"""
import numpy as np

FS, W, HOP, NFFT, J, N, DYN = 10000, 256, 128, 512, 15, 30, 40.0
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
EPS = 2.0 ** -52
EDGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))


def window():
    i = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 1.0) / 257.0)


def frames_of(n):
    return (n - W) // HOP + 1 if n >= W else 0


def edges():
    """The band edges as bins: the first bin of the 10000 / 512 Hz grid nearest to 150 * 2^((2 j -+ 1) / 6) Hz."""
    f = np.arange(NFFT // 2 + 1, dtype=np.float64) * FS / NFFT
    out = []
    for j in range(J):
        lo = int(np.argmin((f - 150.0 * 2.0 ** ((2.0 * j - 1.0) / 6.0)) ** 2))
        hi = int(np.argmin((f - 150.0 * 2.0 ** ((2.0 * j + 1.0) / 6.0)) ** 2))
        out.append((lo, hi))
    return tuple(out)


def _frames(s, count):
    idx = HOP * np.arange(count)[:, None] + np.arange(W)[None, :]
    return s[idx] if count else np.zeros((0, W))


def gate(x, form=1):
    """(energies e [F], keep mask [F]) from the reference alone."""
    F = frames_of(len(x))
    xf = _frames(x, F) * window()
    sq = xf * xf
    power = sq.sum(axis=1) if form == 1 else sq[:, ::-1].sum(axis=1)
    e = 20.0 * np.log10(np.sqrt(power) + EPS)
    if F == 0:
        return e, np.zeros(0, dtype=bool)
    return e, (e.max() - DYN - e) < 0


def rebuild(s, keep):
    kept = np.flatnonzero(keep)
    out = np.zeros((len(kept) - 1) * HOP + W if len(kept) else 0)
    w = window()
    for q, f in enumerate(kept):
        out[HOP * q:HOP * q + W] += w * s[HOP * f:HOP * f + W]
    return out


def _dft_matrices():
    n = np.arange(W, dtype=np.float64)[:, None]
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)[None, :]
    t = np.mod(n * k, NFFT)                                  # exact in fp64
    return np.cos(2.0 * np.pi * t / NFFT), np.sin(2.0 * np.pi * t / NFFT)


_COS_SIN = None


def envelopes(rebuilt, Mk, form=1):
    """[15][Mk]: square roots of the one-third-octave band sums of |DFT_512|^2 of the windowed frames of the rebuilt signal."""
    global _COS_SIN
    fr = _frames(rebuilt, Mk) * window()
    if form == 1:
        spec = np.fft.rfft(fr, n=NFFT, axis=1)
        P = spec.real ** 2 + spec.imag ** 2
    else:
        if _COS_SIN is None:
            _COS_SIN = _dft_matrices()
        C, S = _COS_SIN
        re, im = fr[:, ::-1] @ C[::-1], fr[:, ::-1] @ S[::-1]
        P = re * re + im * im
    out = np.zeros((J, Mk))
    for j, (lo, hi) in enumerate(EDGES):
        if form == 1:
            out[j] = np.sqrt(P[:, lo:hi].sum(axis=1))
        else:
            acc = np.zeros(Mk)
            for k in reversed(range(lo, hi)):
                acc = acc + P[:, k]
            out[j] = np.sqrt(acc)
    return out


def _segments(E):
    """[J][Mk] -> [M][J][N]: the blocks E[:, m - 30 : m] for m = 30 .. Mk."""
    return np.lib.stride_tricks.sliding_window_view(E, N, axis=1).transpose(1, 0, 2)


def _normalise(a, axis):
    a = a - a.mean(axis=axis, keepdims=True)
    return a / (np.sqrt((a * a).sum(axis=axis, keepdims=True)) + EPS)


def correlate(X, Y, extended):
    Mk = X.shape[1]
    if Mk < N:
        return 1e-5, 1
    xs, ys = _segments(X), _segments(Y)
    M = xs.shape[0]
    if extended:
        xn, yn = _normalise(_normalise(xs, 2), 1), _normalise(_normalise(ys, 2), 1)
        return float((xn * yn).sum() / (N * M)), 0
    c = np.sqrt((xs * xs).sum(axis=2, keepdims=True)) / (np.sqrt((ys * ys).sum(axis=2, keepdims=True)) + EPS)
    yp = np.minimum(c * ys, xs * CLIP)
    return float((_normalise(xs, 2) * _normalise(yp, 2)).sum() / (J * M)), 0


def score(x, y, extended=False, form=1):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    assert x.shape == y.shape and x.ndim == 1
    e, keep = gate(x, form)
    F, Mk = len(e), int(keep.sum())
    X, Y = envelopes(rebuild(x, keep), Mk, form), envelopes(rebuild(y, keep), Mk, form)
    d, status = correlate(X, Y, extended)
    margin = float(np.abs(e.max() - DYN - e).min()) if F else np.inf
    return {"d": d, "status": status, "F": F, "Mk": Mk, "X": X, "Y": Y, "margin": margin, "keep": keep}


def form_distance(pairs):
    """(max |d1 - d2| over STOI and ESTOI, max relative envelope distance, smallest gate margin in dB) of form 1 against form 2 over
    [(name, x, y)]; the two forms must agree on every count and keep mask."""
    dist_d = dist_env = 0.0
    margin = np.inf
    for name, x, y in pairs:
        for extended in (False, True):
            a, b = score(x, y, extended, 1), score(x, y, extended, 2)
            assert (a["F"], a["Mk"], a["status"]) == (b["F"], b["Mk"], b["status"]) and np.array_equal(a["keep"], b["keep"]), name
            dist_d = max(dist_d, abs(a["d"] - b["d"]))
            margin = min(margin, a["margin"], b["margin"])
            for key in ("X", "Y"):
                if a["Mk"]:
                    dist_env = max(dist_env, float((np.abs(a[key] - b[key]) / np.abs(a[key])).max()))
    return dist_d, dist_env, margin


# ---- the signals of the tests ----------------------------------------------------------------------------------------------------------
def speech(n, gap=None, seed=0):
    """Synthetic harmonic 'speech' at 10 kHz: a gliding 120 Hz fundamental with 20 harmonics under a 4 Hz syllable envelope and a
    slowly moving spectral tilt, a noise floor 50 dB down; ``gap`` = (first, last) samples of near silence (80 dB further down)."""
    g = np.random.default_rng(1000 + seed)
    t = np.arange(n, dtype=np.float64) / FS
    f0 = 120.0 + 25.0 * np.sin(2.0 * np.pi * 0.7 * t + seed)
    phase = 2.0 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(n)
    for h in range(1, 21):
        tilt = 1.0 / h ** (1.0 + 0.5 * np.sin(2.0 * np.pi * 1.3 * t + 0.4 * h))
        x += tilt * np.sin(h * phase + g.uniform(0, 2 * np.pi))
    x *= 0.55 + 0.45 * np.sin(2.0 * np.pi * 4.0 * t + 0.3 * seed)
    x = 0.1 * x / np.abs(x).max() + 3e-4 * g.standard_normal(n)
    if gap is not None:
        x[gap[0]:gap[1]] *= 1e-4
    return x.astype(np.float32)


def noisy(x, snr_db, seed):
    """x plus white noise at the given SNR (dB) over the whole clip."""
    g = np.random.default_rng(77 + seed)
    x = np.asarray(x, dtype=np.float64)
    noise = g.standard_normal(len(x))
    noise *= np.sqrt((x * x).mean() / (noise * noise).mean()) * 10.0 ** (-snr_db / 20.0)
    return (x + noise).astype(np.float32)


SNRS = (20.0, 5.0, -5.0)
# (samples, gap, F, Mk) of the GPU test's clips: every frame kept and two segments; a silent gap; a silent gap; too few kept frames
CLIPS = ((4100, None, 31, 31), (8000, (2300, 6100), 61, 33), (9000, (3000, 7300), 69, 37), (6500, (2000, 5200), 49, 26))
EDGE_LENGTHS = (255, 256, 383, 384, 3967, 3968)


def clip(i):
    n, gap, _, _ = CLIPS[i]
    if gap is None:                                          # noisy throughout: no frame is 40 dB below the loudest
        return noisy(speech(n, None, i), 10.0, 50 + i)
    return speech(n, gap, i)


def gpu_test_pairs():
    """[(name, x, y)]: each clip of CLIPS with its three noisy estimates."""
    out = []
    for i in range(len(CLIPS)):
        x = clip(i)
        out += [(f"clip{len(x)}@{snr:+.0f}dB", x, noisy(x, snr, 10 * i + k)) for k, snr in enumerate(SNRS)]
    return out


LONG = (40000, (12000, 20000))


def long_pairs():
    """[(name, x, y)]: one clip of 311 frames -- more than the 256 frames of one compaction step and more than 64 segments, the two
    sizes at which the device's gate and fold loop a second time -- with a silent gap, and a 5 dB estimate."""
    x = speech(LONG[0], LONG[1], 9)
    return [(f"clip{len(x)}@+5dB", x, noisy(x, 5.0, 99))]


def edge_pairs():
    """[(name, x, y)]: non-silent noise at the frame-count edges: the first frame, the first hop, 29 against 30 frames."""
    out = []
    for n in EDGE_LENGTHS:
        g = np.random.default_rng(n)
        x = (0.1 * g.standard_normal(n)).astype(np.float32)
        out.append((f"noise{n}", x, noisy(x, 5.0, n)))
    return out
