"""fp64 numpy restatement of the two definitions behind voicesplit_amd/csrc/mix.hip (a helper module, not a test):

``trim_bounds(y)``: ``librosa.effects.trim(y, top_db=20)`` with its defaults frame_length = 2048, hop_length = 512, ref = np.max,
as include/voicesplit_hip.h states it (librosa is not a dependency; nobody has compared this with a librosa run);
``mix(c, i)``: the arithmetic of mix_wavfiles (utils/generic_utils.py:320-329) with the roundings vs_mix_clips states;
``margin(y)``: how far the closest frame of ``y`` is from the silence threshold, relative to the threshold."""
import numpy as np

FRAME, HOP, PAD = 2048, 512, 1024
AMIN, RATIO = 1e-10, 1e-2


def frame_mse(y) -> np.ndarray:
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    if n < PAD + 1:
        raise ValueError(f"clip of {n} samples: the reflect padding needs {PAD + 1}")
    k = np.arange(1, PAD + 1)
    yp = np.concatenate([y[k[::-1]], y, y[n - 1 - k]])    # yp[1024 - k] = y[k], yp[1024 + n - 1 + k] = y[n - 1 - k]
    assert yp.shape[0] == n + 2 * PAD
    sq = yp * yp
    return np.array([sq[HOP * f:HOP * f + FRAME].mean() for f in range(n // HOP + 1)])


def _ratios(y) -> np.ndarray:
    mse = frame_mse(y)
    return np.maximum(AMIN, mse) / max(AMIN, mse.max())


def trim_bounds(y):
    n = len(y)
    loud = np.flatnonzero(_ratios(y) > RATIO)
    if loud.size == 0:
        return 0, 0
    return HOP * int(loud[0]), min(n, HOP * (int(loud[-1]) + 1))


def margin(y) -> float:
    """min over the frames of |ratio / 1e-2 - 1|: a computation whose relative error is below this decides every frame alike."""
    return float(np.abs(_ratios(y) / RATIO - 1.0).min())


def mix(c, i):
    """c, i: float32 arrays of equal length -> (mixed fp64, target fp64, norm float32, valid): the quotients are exact fp64
    quotients of the fp32 sum / the fp32 clean sample by the fp32 ``norm = float32(1.1 * float64(m))``."""
    c, i = np.asarray(c, dtype=np.float32), np.asarray(i, dtype=np.float32)
    s = c + i                                             # fp32 sums
    m = np.float32(np.abs(s).max())
    norm = np.float32(1.1 * np.float64(m))
    if m == 0:
        z = np.zeros(c.shape, dtype=np.float64)
        return z, z.copy(), norm, 0
    return s.astype(np.float64) / np.float64(norm), c.astype(np.float64) / np.float64(norm), norm, 1
