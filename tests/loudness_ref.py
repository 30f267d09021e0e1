"""fp64 restatement of the loudness contract of include/voicesplit_hip.h (ITU-R BS.1770-4 integrated loudness of a mono clip), with
scipy.signal.lfilter (which IS transposed direct form II) in two forms:

    serial(x, fs)      the whole clip through the two biquads, then blocks and gates
    segmented(x, fs)   the device's algorithm: zero-state end states per sub-block, `step` built by the recurrence itself, the
                       propagated start states, then every sub-block from its own start state

Both return a dict: lufs, peak, counts (blocks, past the absolute gate, past both), valid, energy [m].  The signals of the GPU
tests are built here too, so that the CPU test can measure d_ref (segmented against serial) on exactly them.
"""
import numpy as np
from scipy.signal import lfilter

RATES = (8000, 11025, 16000, 22050, 44100, 48000, 96000)
GATE_RATES = (8000, 11025, 16000, 22050, 44100, 48000)
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
BS1770_48K = {"b1": (1.53512485958697, -2.69169618940638, 1.19839281085285), "a1": (-1.69065929318241, 0.73248077421585),
              "a2": (-1.99004745483398, 0.99007225036621)}


def coefficients(fs):
    """(b1 [3], a1 [2], b2 [3], a2 [2]) of the two K-weighting biquads at the rate fs."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d])
    return b1, a1, b2, a2


def sub_block(fs):
    return (fs + 5) // 10


def _run(x, fs, state):
    """The cascade over x from state (s1, s2, s3, s4) -> (w, end state)."""
    b1, a1, b2, a2 = coefficients(fs)
    state = np.asarray(state, dtype=np.float64)
    u, z1 = lfilter(b1, np.concatenate(([1.0], a1)), x, zi=state[:2])
    w, z2 = lfilter(b2, np.concatenate(([1.0], a2)), u, zi=state[2:])
    return w, np.concatenate((z1, z2))


def step_matrix(fs):
    """step[r][c]: component r of the state after S zero-input samples from the unit state c -- the recurrence run S times."""
    S = sub_block(fs)
    step = np.zeros((4, 4))
    for c in range(4):
        unit = np.zeros(4)
        unit[c] = 1.0
        step[:, c] = _run(np.zeros(S), fs, unit)[1]
    return step


def gate(energy, S):
    """Blocks and gates over the sub-block energies: (lufs, counts, valid)."""
    m = len(energy)
    if m < 4:
        return -np.inf, (0, 0, 0), 0
    z = (((energy[:-3] + energy[1:-2]) + energy[2:-1]) + energy[3:]) / (4.0 * S)
    past_abs = z > ABS_GATE
    if not past_abs.any():
        return -np.inf, (m - 3, 0, 0), 0
    past_both = past_abs & (z > 0.1 * z[past_abs].mean())
    return -0.691 + 10.0 * np.log10(z[past_both].mean()), (m - 3, int(past_abs.sum()), int(past_both.sum())), 1


def _result(x, energy, S):
    lufs, counts, valid = gate(energy, S)
    x32 = np.asarray(x, dtype=np.float32)
    return {"lufs": lufs, "peak": np.float32(np.abs(x32).max()) if len(x32) else np.float32(0), "counts": counts, "valid": valid,
            "energy": energy}


def serial(x, fs):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    S = sub_block(fs)
    m = len(x) // S
    w = _run(x[:m * S], fs, np.zeros(4))[0]
    return _result(x, (w * w).reshape(m, S).sum(axis=1) if m else np.zeros(0), S)


def segmented(x, fs):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    S = sub_block(fs)
    m = len(x) // S
    rows = x[:m * S].reshape(m, S)
    ends = [_run(r, fs, np.zeros(4))[1] for r in rows]
    step = step_matrix(fs)
    s, energy = np.zeros(4), np.zeros(m)
    for k in range(m):
        w = _run(rows[k], fs, s)[0]
        energy[k] = (w * w).sum()
        s = step @ s + ends[k]
    return _result(x, energy, S)


# ---- the signals of tests/test_gpu_loudness.py ---------------------------------------------------------------------------------------
def sine(fs, seconds, amplitude=1.0, freq=997.0, phase=0.0):
    t = np.arange(int(round(fs * seconds)), dtype=np.float64)
    return (amplitude * np.sin(2.0 * np.pi * freq * t / fs + phase)).astype(np.float32)


def length_clips(S, limit=None):
    """Seeded noise at the lengths of the length test (all of them for S = 1600; up to 65 S + 7 otherwise)."""
    lengths = [0, 1, 4 * S - 1, 4 * S, 4 * S + 1, 5 * S - 1, 5 * S, 64 * S, 65 * S + 7, 257 * S + 3]
    if limit is not None:
        lengths = [n for n in lengths if n <= limit]
    g = np.random.default_rng(1770 + S)
    return [(0.1 * g.standard_normal(n)).astype(np.float32) for n in lengths]


def gate_clip(fs, dc=0.0):
    """12 sub-blocks of noise at amplitude 0.1, 8 of digital silence, 8 at 0.01, 6 at 3e-5, 3 at 0.1, S / 2 + 3 more samples."""
    S = sub_block(fs)
    g = np.random.default_rng(fs)
    parts = [0.1 * g.standard_normal(12 * S), np.zeros(8 * S), 0.01 * g.standard_normal(8 * S), 3e-5 * g.standard_normal(6 * S),
             0.1 * g.standard_normal(3 * S), 0.1 * g.standard_normal(S // 2 + 3)]
    return (np.concatenate(parts) + dc).astype(np.float32)


GATE_DC = (0.0, 0.05, 0.5)


def gpu_test_signals():
    """(name, fs, x) for every signal whose lufs the GPU tests compare with `serial`."""
    out = []
    for S, fs, limit in ((1600, 16000, None), (4800, 48000, 65 * 4800 + 7)):
        out += [(f"len{len(x)}@{fs}", fs, x) for x in length_clips(S, limit)]
    for fs in GATE_RATES:
        out += [(f"gate@{fs}+{dc}", fs, gate_clip(fs, dc)) for dc in GATE_DC]
    return out
