"""fp64 restatement of the phase-less branch of ``openVoiceFilterAudioProcessor.spec2wav`` (utils/audio_processor.py:492-496) and
of ``_griffin_lim`` (:516-523), on ``oracle.reference_audio.stft`` / ``istft``.  TEST INFRASTRUCTURE ONLY.

The reference loop is *restated* in numpy, not compared with a librosa run (librosa is not installed here; the two transforms are
the restatements ``tests/test_oracle.py`` pins).  Two departures from the upstream lines, both forced: the starting angles are an
argument (``np.random.rand`` inside ``_griffin_lim`` cannot be reproduced on the device) and every iterate and the residual
``|| |D_i| - S || / || S ||`` are returned.

**The tolerance of the device tests is defined here** (``tolerances``).  An element-wise comparison of a Griffin-Lim output with
a clean fp64 run has no fixed bound: a near-empty bin can turn its phase under an fp32-sized error and the loop feeds that back.
So the loop is run again in fp64 with every transform perturbed by what ``tests/test_gpu_audio.py`` already allows the device
transforms: after every STFT complex Gaussian noise of standard deviation ``3e-6 x`` that frame's largest ``|D|`` (E|z|^2 =
sigma^2: each component sigma / sqrt 2), after every iSTFT real Gaussian noise of standard deviation ``2e-5 x max|y|``.  The allowed
``max|y_gpu - y_ref| / max|y_ref|`` is TWICE the largest deviation of four such runs (seeds 0..3) from the clean run at the same
iteration count (four draws under-sample the tail; the sigmas are worst-case bounds used as standard deviations, which is
already generous), and the allowed ``|res_gpu - res_ref|`` is twice the largest deviation of their residuals over the iterations
run.  With no iteration the bound is the existing ``2e-5 x max|ref|``.  An input whose doubled envelope reaches ``5e-2`` is too
sensitive to test with (``MAX_TOLERANCE``; tests/test_griffin_lim_cpu.py holds every input below to it).
"""
import functools
import os

import numpy as np

from oracle import reference_audio as RA

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AUDIO = {"n_fft": 1200, "num_freq": 601, "sample_rate": 16000, "hop_length": 160, "win_length": 400, "min_level_db": -100.0,
         "ref_level_db": 20.0, "power": 1.5, "griffin_lim_iters": 60}
STFT_SIGMA, ISTFT_SIGMA = 3e-6, 2e-5          # the bounds tests/test_gpu_audio.py holds wav_to_spec / spec_to_wav to
PLAIN_TOLERANCE = 2e-5                        # n_iter == 0: spec_to_wav's own bound
MAX_TOLERANCE = 5e-2
SEEDS = (0, 1, 2, 3)

# (B, T) -> the iteration counts tested there; every shape is crossed with INITS and POWERS
SHAPES = {(1, 5): (0, 1, 4), (3, 21): (0, 1, 4, 60), (2, 301): (2,)}
INITS = ("random", "mixture")
POWERS = (1.0, 1.5)
CLIPS = {(1, 5): (0,), (3, 21): (0, 1, 2), (2, 301): (2, 3)}
ZERO_MASK_ITEM = {(3, 21): 2}                 # one item of the M = 63 case takes an all-zero mask

# Other STFT geometries (n_fft, hop, win); every function below takes one as ``geom`` and defaults to the reference's
# 1200 / 160 / 400, whose cases and values are the ones above.
#   G1: win == n_fft, an odd hop that does not divide it (6 frames per sample); T = 4 is the shortest legal clip
#       (S = 33 = n_fft / 2 + 1: both reflections at their limit)
#   G2: n_fft = 2 (mod 4): K = 2 F = 404 needs no row padding; hop = win / 2
#   G3: an odd window one short of the frame (lead = 128, win % 4 != 0); hop divides n_fft / 2
#   G4, G5: the waveglow and wavernn blocks of the reference's config.json
DEFAULT_GEOM = (1200, 160, 400)
GEOMETRIES = {"G1": (64, 11, 64), "G2": (402, 100, 200), "G3": (256, 64, 255), "G4": (1024, 256, 1024), "G5": (2048, 200, 800)}
GEOM_SHAPES = {"G1": (2, 4), "G2": (2, 12), "G3": (2, 7), "G4": (2, 9), "G5": (2, 11)}      # (B, T), clips 0 and 1
GEOM_ITERS = (0, 1, 4)


def audio_cfg(geom=DEFAULT_GEOM):
    """AUDIO with the geometry's n_fft / hop / win (and num_freq)."""
    n_fft, hop, win = geom
    return dict(AUDIO, n_fft=n_fft, num_freq=n_fft // 2 + 1, hop_length=hop, win_length=win)


def _iters(B, T, geom):
    return SHAPES[(B, T)] if geom == DEFAULT_GEOM else GEOM_ITERS


def target_magnitude(spec, mask=None, power=1.0, min_level_db=-100.0, ref_level_db=20.0):
    """S = (db_to_amp(denormalize(spec * mask) + ref_level_db)) ** power, [T, F]   (:494-496, :540-541, :546-547)."""
    v = spec if mask is None else spec * mask
    S = (np.clip(v, 0.0, 1.0) - 1.0) * -min_level_db
    return np.power(10.0, (S + ref_level_db) * 0.05) ** power


def griffin_lim(S, init_phase, n_iter, n_fft=1200, hop=160, win=400, noise_seed=None):
    """S, init_phase [T, F] -> (iterates [n_iter + 1, hop * (T - 1)], residual [n_iter]).  iterates[0] is the plain inverse
    ``istft(S * exp(1j * init_phase))``; iterates[k] the waveform after k rounds of :520-522.  residual[i] is taken on the STFT of
    iteration i, that is of iterates[i].  noise_seed: the perturbation mode of the module docstring."""
    rng = None if noise_seed is None else np.random.default_rng(noise_seed)
    St = np.abs(S.T).astype(np.complex128)                                           # :518, [F, T]
    norm = np.sqrt((np.abs(St) ** 2).sum())

    def inv(D):
        y = RA.istft(D, hop, win)
        if rng is not None:
            y = y + ISTFT_SIGMA * np.abs(y).max() * rng.standard_normal(y.shape)
        return y

    def fwd(y):
        D = RA.stft(y, n_fft, hop, win)
        if rng is not None:
            sigma = STFT_SIGMA * np.abs(D).max(axis=0, keepdims=True) / np.sqrt(2.0)
            D = D + sigma * (rng.standard_normal(D.shape) + 1j * rng.standard_normal(D.shape))
        return D

    y = inv(St * np.exp(1j * init_phase.T))                                          # :517-519 with the given angles
    ys, res = [y], []
    for _ in range(n_iter):                                                          # :520
        D = fwd(y)
        res.append(np.sqrt(((np.abs(D) - np.abs(St)) ** 2).sum()) / norm)
        y = inv(St * np.exp(1j * np.angle(D)))                                       # :521-522 (np.angle(0) == 0)
        ys.append(y)
    return np.stack(ys), np.asarray(res)


@functools.lru_cache(maxsize=None)
def _clips():
    z = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    return z["target"].astype(np.float64) / 32768.0, z["mixed"].astype(np.float64) / 32768.0


@functools.lru_cache(maxsize=None)
def inputs(B, T, geom=DEFAULT_GEOM):
    """The device inputs of a shape, as float32 arrays (the reference runs on exactly these values): spec [B, T, F] = wav2spec
    of the target clips, mixture [B, T, F] = the phase of the mixtures, random [B, T, F] = 2 pi U[0, 1) angles (seeded),
    mask [B, T, F] or None.  Samples 16000 : 16000 + hop (T - 1) of the clips, from sample 0 where that would run past their end.
    Another geometry than the default takes clips 0 .. B - 1 and no mask."""
    target, mixed = _clips()
    n_fft, hop, win = geom
    clips = CLIPS[(B, T)] if geom == DEFAULT_GEOM else tuple(range(B))
    lo = 16000 if 16000 + hop * (T - 1) <= target.shape[1] else 0          # T = 301 is the whole 3 s clip: it cannot start 1 s in
    hi = lo + hop * (T - 1)
    spec = np.ascontiguousarray(np.stack([RA.wav2spec(target[c, lo:hi], n_fft, hop, win)[0] for c in clips]), dtype=np.float32)
    mixture = np.ascontiguousarray(np.stack([RA.wav2spec(mixed[c, lo:hi], n_fft, hop, win)[1] for c in clips]), dtype=np.float32)
    random = (2.0 * np.pi * np.random.default_rng(1000 * B + T).random(spec.shape)).astype(np.float32)
    mask = None
    if geom == DEFAULT_GEOM and (B, T) in ZERO_MASK_ITEM:
        mask = np.ones_like(spec)
        mask[ZERO_MASK_ITEM[(B, T)]] = 0.0
    return {"spec": spec, "mixture": mixture, "random": random, "mask": mask}


@functools.lru_cache(maxsize=None)
def runs(B, T, init, power, geom=DEFAULT_GEOM):
    """Per item: the clean run and the four perturbed runs at the largest iteration count of the shape (a run with fewer
    iterations is a prefix: the noise stream is drawn in order).  -> list of (clean (ys, res), [perturbed (ys, res)])."""
    x = inputs(B, T, geom)
    n = max(_iters(B, T, geom))
    n_fft, hop, win = geom
    out = []
    for b in range(B):
        m = None if x["mask"] is None else x["mask"][b].astype(np.float64)
        S = target_magnitude(x["spec"][b].astype(np.float64), m, power)
        ph = x[init][b].astype(np.float64)
        out.append((griffin_lim(S, ph, n, n_fft, hop, win), [griffin_lim(S, ph, n, n_fft, hop, win, noise_seed=s) for s in SEEDS]))
    return out


def reference(B, T, init, power, n_iter, geom=DEFAULT_GEOM):
    """-> (wav [B, hop*(T-1)], residual [n_iter, B]) of the clean fp64 run."""
    r = runs(B, T, init, power, geom)
    return np.stack([c[0][n_iter] for c, _ in r]), np.stack([c[1][:n_iter] for c, _ in r], axis=1)


def tolerances(B, T, init, power, n_iter, geom=DEFAULT_GEOM):
    """-> (tol_wav [B] relative to max|y_ref| of the item, tol_res [B] absolute): the rule of the module docstring."""
    if n_iter == 0:
        return np.full(B, PLAIN_TOLERANCE), np.zeros(B)
    tw, tr = [], []
    for (cy, cr), pert in runs(B, T, init, power, geom):
        ref = cy[n_iter]
        tw.append(2.0 * max(np.abs(py[n_iter] - ref).max() for py, _ in pert) / np.abs(ref).max())
        tr.append(2.0 * max(np.abs(pr[:n_iter] - cr[:n_iter]).max() for _, pr in pert))
    return np.asarray(tw), np.asarray(tr)


def cases(geom=DEFAULT_GEOM):
    """Every (B, T, init, power, n_iter) the tests run at the default geometry; for another one (B, T, init, power, n_iter, geom),
    so that ``reference(*case)`` and ``tolerances(*case)`` serve both."""
    if geom == DEFAULT_GEOM:
        return [(B, T, init, power, n) for (B, T), iters in SHAPES.items() for init in INITS for power in POWERS for n in iters]
    B, T = GEOM_SHAPES[{v: k for k, v in GEOMETRIES.items()}[geom]]
    return [(B, T, init, power, n, geom) for init in INITS for power in POWERS for n in GEOM_ITERS]


def geometry_cases():
    """The cases of every geometry of GEOMETRIES, with their ids."""
    out = [(tag, c) for tag, geom in GEOMETRIES.items() for c in cases(geom)]
    return [c for _, c in out], [f"{tag}-B{c[0]}-T{c[1]}-{c[2]}-p{c[3]}-n{c[4]}" for tag, c in out]
