"""fp64 restatement of the wavernn and waveglow audio back ends of ``WrapperAudioProcessor``: utils/audio_processor.py:61-438
(WaveRNNAudioProcessor, WaveGlowAudioProcessor), utils/audio.py:49-135 (WaveGlowSTFT, dynamic range compression) and
utils/stft.py:36-99 (the Tacotron conv1d-basis transform).  TEST INFRASTRUCTURE ONLY.

This is a *restatement*, not a comparison with a run of the reference: librosa is not installed here and neither reference
processor imports without it, so nothing below is pinned to the upstream classes the way ``oracle/reference_audio.py`` is pinned to
``openVoiceFilterAudioProcessor``.  What is restated, line by line:

  geometry       ``_stft_parameters`` :175-182 (Python's ``int()`` on the fp64 product); waveglow names its own
  transform      ``librosa.stft`` (:270-276, :411-418) on ``oracle.reference_audio``'s restatement, with the pad mode as a
                 parameter; ``STFT.transform`` of utils/stft.py is the same sum (reflect padding by filter_length / 2, the
                 periodic Hann window padded to the frame, stride hop): its basis scale touches the inverse only
  codecs         ``_amp_to_db`` :184-186, ``_normalize`` :140-155, ``_denormalize`` :157-173, ``_db_to_amp`` :188-189;
                 ``dynamic_range_compression`` / ``_decompression`` utils/audio.py:49-61; DB01 is oracle.reference_audio's
  pre-emphasis   ``apply_preemphasis`` / ``apply_inv_preemphasis`` :191-199 (scipy.signal.lfilter)
  mel            ``_linear_to_mel`` :121-123, ``_mel_to_linear`` :125-127 / :404-405, ``mag_to_mel_spectrogram`` utils/audio.py:119-135,
                 on ``voicesplit_amd.speaker.mel_filterbank`` (librosa.filters.mel restated; unpinned as well)
  inversion      ``_griffin_lim`` :261-268 / :420-427 with the starting angles as an argument, as ``griffin_lim_ref`` does

The codecs clip: with ``clip_norm`` (and for DB01) the smallest stored value stands for ``10 ** ((min_level_db + ref_level_db) / 20)``
(1e-4 for -100 / 20), above the encoder's ``floor``; ``effective_floor`` names the magnitude below which a codec cannot tell two
inputs apart, and ``decode(encode(m)) == max(effective_floor, m)`` below the top clip.

The tolerance rule of the Griffin-Lim tests is ``griffin_lim_ref.tolerances`` rebuilt with the pad mode as a parameter (``tolerances``
below): twice the worst deviation of four perturbed fp64 runs, capped by ``MAX_TOLERANCE``.
"""
import functools

import numpy as np
from scipy.signal import lfilter

import griffin_lim_ref as G
from oracle import reference_audio as RA

MAX_TOLERANCE = G.MAX_TOLERANCE
GEOM_ITERS = (0, 1, 4)

# the two foreign blocks of the reference's config.json:47-82
WAVEGLOW = {"segment_length": 16000, "sample_rate": 22050, "filter_length": 1024, "num_freq": 513, "n_mel_channels": 80,
            "hop_length": 256, "win_length": 1024, "mel_fmin": 0.0, "mel_fmax": 8000.0, "power": 1.5, "griffin_lim_iters": 60}
WAVERNN = {"force_convert_SR": True, "num_mels": 80, "num_freq": 1025, "sample_rate": 16000, "frame_length_ms": 50,
           "frame_shift_ms": 12.5, "preemphasis": 0.98, "min_level_db": -100, "ref_level_db": 20, "signal_norm": True,
           "symmetric_norm": False, "max_norm": 1, "clip_norm": True, "mel_fmin": 0.0, "mel_fmax": 8000.0,
           "do_trim_silence": True, "power": 1.5, "griffin_lim_iters": 60}


def wavernn_geometry(block):
    """:175-182 -> (n_fft, hop, win)."""
    sr = block["sample_rate"]
    return (block["num_freq"] - 1) * 2, int(block["frame_shift_ms"] / 1000.0 * sr), int(block["frame_length_ms"] / 1000.0 * sr)


def wavernn_block(n_fft, hop, win, **over):
    """A wavernn block whose times give (n_fft, hop, win) at 1 kHz (1 ms per sample), the reference's other values kept."""
    b = dict(WAVERNN, num_freq=n_fft // 2 + 1, sample_rate=1000, frame_shift_ms=hop, frame_length_ms=win, mel_fmax=None)
    b.update(over)
    assert wavernn_geometry(b) == (n_fft, hop, win)
    return b


def waveglow_block(n_fft, hop, win, **over):
    b = dict(WAVEGLOW, filter_length=n_fft, num_freq=n_fft // 2 + 1, hop_length=hop, win_length=win)
    b.update(over)
    return b


# ---- codecs ---------------------------------------------------------------------------------------------------------------------
def log_codec():
    return {"kind": "LOG", "floor": 1e-5, "min_level_db": -100.0, "ref_level_db": 20.0, "signal_norm": False, "symmetric_norm": False,
            "clip_norm": False, "max_norm": 1.0, "preemphasis": 0.0, "gl_pad": "zero"}


def dbnorm_codec(min_level_db=-100.0, ref_level_db=20.0, signal_norm=True, symmetric_norm=False, clip_norm=True, max_norm=1.0,
                 preemphasis=0.0):
    return {"kind": "DBNORM", "floor": float(np.exp(min_level_db / 20 * np.log(10))), "min_level_db": float(min_level_db),
            "ref_level_db": float(ref_level_db), "signal_norm": signal_norm, "symmetric_norm": symmetric_norm, "clip_norm": clip_norm,
            "max_norm": float(max_norm), "preemphasis": float(preemphasis), "gl_pad": "reflect"}


def db01_codec(min_level_db=-100.0, ref_level_db=20.0):
    return {"kind": "DB01", "floor": 1e-5, "min_level_db": float(min_level_db), "ref_level_db": float(ref_level_db), "signal_norm": False,
            "symmetric_norm": False, "clip_norm": False, "max_norm": 1.0, "preemphasis": 0.0, "gl_pad": "reflect"}


# the DBNORM variants of the device tests: name -> codec
DBNORM_VARIANTS = {
    "plain": dbnorm_codec(),
    "symmetric4": dbnorm_codec(symmetric_norm=True, max_norm=4.0),
    "noclip": dbnorm_codec(clip_norm=False),
    "nonorm": dbnorm_codec(signal_norm=False),
}


def encode(m, c):
    """Linear magnitude -> stored value."""
    m = np.asarray(m, dtype=np.float64)
    if c["kind"] == "LOG":
        return np.log(np.maximum(m, c["floor"]))                                             # utils/audio.py:49-54, C = 1
    S = 20 * np.log10(np.maximum(c["floor"], m)) - c["ref_level_db"]                           # :184-186, :206
    if c["kind"] == "DB01":
        return np.clip(S / -c["min_level_db"], -1.0, 0.0) + 1.0                                # :537-544
    if not c["signal_norm"]:
        return S
    n = (S - c["min_level_db"]) / -c["min_level_db"]                                           # :143
    if c["symmetric_norm"]:
        n = ((2 * c["max_norm"]) * n) - c["max_norm"]
        return np.clip(n, -c["max_norm"], c["max_norm"]) if c["clip_norm"] else n
    n = c["max_norm"] * n
    return np.clip(n, 0, c["max_norm"]) if c["clip_norm"] else n


def decode(v, c):
    """Stored value -> linear magnitude."""
    S = np.asarray(v, dtype=np.float64)
    if c["kind"] == "LOG":
        return np.exp(S)                                                                     # utils/audio.py:56-61
    if c["kind"] == "DB01":
        S = (np.clip(S, 0.0, 1.0) - 1.0) * -c["min_level_db"]                                  # :546-547
    elif c["signal_norm"]:
        if c["symmetric_norm"]:                                                              # :161-165
            if c["clip_norm"]:
                S = np.clip(S, -c["max_norm"], c["max_norm"])
            S = ((S + c["max_norm"]) * -c["min_level_db"] / (2 * c["max_norm"])) + c["min_level_db"]
        else:                                                                                # :166-171
            if c["clip_norm"]:
                S = np.clip(S, 0, c["max_norm"])
            S = (S * -c["min_level_db"] / c["max_norm"]) + c["min_level_db"]
    return np.power(10.0, (S + c["ref_level_db"]) * 0.05)                                      # :188-189, :243


def effective_floor(c):
    """The magnitude the smallest stored value of a codec stands for (module docstring)."""
    clipped = c["kind"] == "DB01" or (c["kind"] == "DBNORM" and c["signal_norm"] and c["clip_norm"])
    return max(c["floor"], 10.0 ** ((c["min_level_db"] + c["ref_level_db"]) / 20.0)) if clipped else c["floor"]


def top(c):
    """The largest stored value (None: the codec has no top clip)."""
    if c["kind"] == "DB01":
        return 1.0
    return c["max_norm"] if c["kind"] == "DBNORM" and c["signal_norm"] and c["clip_norm"] else None


# ---- pre-emphasis ---------------------------------------------------------------------------------------------------------------
def preemphasis(x, a):
    return lfilter([1, -a], [1], np.asarray(x, dtype=np.float64))                             # :191-194


def deemphasis(x, a):
    return lfilter([1], [1, -a], np.asarray(x, dtype=np.float64))                             # :196-199


def deemphasis_segmented(x, a, L):
    """The same recurrence cut into blocks of L samples, as csrc/audio_codec.hip runs it: every block swept from a zero state,
    carry(k+1) = a^L carry(k) + last(k), then y[j] = z[j] + a^(j+1) carry (the powers by repeated multiplication)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.empty_like(x)
    aL = 1.0
    for _ in range(L):
        aL *= a
    carry = 0.0
    for lo in range(0, len(x), L):
        z, ap = 0.0, 1.0
        for j in range(lo, min(lo + L, len(x))):
            z = x[j] + a * z
            ap *= a
            y[j] = z + ap * carry
        carry = aL * carry + z
    return y


def segment_distance(x, a, L):
    """d of the de-emphasis bound: the largest distance between ``deemphasis`` and its segmented form at block length L."""
    return float(np.abs(deemphasis(x, a) - deemphasis_segmented(x, a, L)).max())


# ---- transform, features, inverse -----------------------------------------------------------------------------------------------
def stft(y, n_fft, hop, win, pad="reflect"):
    """``librosa.stft(y, n_fft, hop, win, pad_mode=...)`` -> complex [F, T]; pad "reflect" is ``oracle.reference_audio.stft``."""
    if pad == "reflect":
        return RA.stft(y, n_fft, hop, win)
    w = RA._padded_hann(win, n_fft)
    yp = np.pad(y, n_fft // 2, mode="constant")
    T = 1 + (len(yp) - n_fft) // hop
    return np.fft.rfft(np.stack([yp[t * hop:t * hop + n_fft] * w for t in range(T)], axis=1), axis=0)


def mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """fp64 [n_mels, F] of the fp32-rounded basis the device multiplies with."""
    from voicesplit_amd.speaker import mel_filterbank
    return mel_filterbank(sr, n_fft, n_mels, fmin, fmax).numpy().astype(np.float32).astype(np.float64)


def mel_pinv(basis):
    """fp64 [F, n_mels] of the fp32-rounded pseudo-inverse (``np.linalg.pinv`` :126, :405)."""
    return np.linalg.pinv(basis).astype(np.float32).astype(np.float64)


def analysis(y, geom, a=0.0):
    """One clip -> (|D| [T, F], angle(D) [T, F]) of the (pre-emphasised, a != 0) clip: ``spectrogram`` :201-207 up to the codec."""
    y = np.asarray(y, dtype=np.float64)
    D = stft(preemphasis(y, a) if a != 0 else y, *geom)
    return np.abs(D).T, np.angle(D).T


def inverse_with_phase(mag, phase, geom):
    """Linear magnitude and phase [T, F] -> waveform, before any de-emphasis (our extension: the reference drops the phase)."""
    return RA.istft(mag.T * np.exp(1j * phase.T), geom[1], geom[2])


def griffin_lim(S, init_phase, n_iter, geom, pad="reflect", noise_seed=None):
    """``griffin_lim_ref.griffin_lim`` with the pad mode of the inner transform as a parameter (``_librosa_stft`` :411-418 pads with
    zeros).  S [T, F] is the target ITSELF (``mag ** power`` taken by the caller).  -> (iterates [n_iter + 1, n], residual)."""
    n_fft, hop, win = geom
    rng = None if noise_seed is None else np.random.default_rng(noise_seed)
    St = np.abs(S.T).astype(np.complex128)
    norm = np.sqrt((np.abs(St) ** 2).sum())

    def inv(D):
        y = RA.istft(D, hop, win)
        if rng is not None:
            y = y + G.ISTFT_SIGMA * np.abs(y).max() * rng.standard_normal(y.shape)
        return y

    def fwd(y):
        D = stft(y, n_fft, hop, win, pad)
        if rng is not None:
            sigma = G.STFT_SIGMA * np.abs(D).max(axis=0, keepdims=True) / np.sqrt(2.0)
            D = D + sigma * (rng.standard_normal(D.shape) + 1j * rng.standard_normal(D.shape))
        return D

    y = inv(St * np.exp(1j * init_phase.T))
    ys, res = [y], []
    for _ in range(n_iter):
        D = fwd(y)
        res.append(np.sqrt(((np.abs(D) - np.abs(St)) ** 2).sum()) / norm)
        y = inv(St * np.exp(1j * np.angle(D)))
        ys.append(y)
    return np.stack(ys), np.asarray(res)


# ---- the inputs and cases of the device tests -----------------------------------------------------------------------------------
# Griffin-Lim on a linear target: (tag, B, T, gain, pad, pre-emphasis of the clip the target is taken from)
GL_CASES = [("G4", 2, 9, 0.25, "zero", 0.0), ("G1", 2, 4, 1.0, "zero", 0.0), ("G5", 2, 11, 0.25, "reflect", 0.98)]
INITS = ("random", "mixture")
POWERS = (1.0, 1.5)


@functools.lru_cache(maxsize=None)
def clips(tag, B, T, gain):
    """``test_gpu_stft_geometry.clips`` as a float32 array [B, hop (T - 1)] (the tone recipe, then demo speech)."""
    from test_gpu_stft_geometry import clips as geometry_clips
    return np.ascontiguousarray(geometry_clips(tag, B, T, gain).numpy())


@functools.lru_cache(maxsize=None)
def gl_inputs(tag, B, T, gain, a):
    """float32 arrays the device and the reference both start from: mag [B, T, F] = |D| of the clips (pre-emphasised by a),
    mixture [B, T, F] = the phase of the demo MIXTURES over the same samples, random [B, T, F] = 2 pi U[0, 1)."""
    geom = G.GEOMETRIES[tag]
    x = clips(tag, B, T, gain)
    mixed = G._clips()[1][:B, 16000:16000 + x.shape[1]] * gain
    mag = np.stack([analysis(x[b], geom, a)[0] for b in range(B)]).astype(np.float32)
    mixture = np.stack([analysis(mixed[b], geom, a)[1] for b in range(B)]).astype(np.float32)
    random = (2.0 * np.pi * np.random.default_rng(7000 + 100 * B + T).random(mag.shape)).astype(np.float32)
    return {"mag": mag, "mixture": mixture, "random": random}


@functools.lru_cache(maxsize=None)
def runs(tag, B, T, gain, pad, a, init, power):
    """Per item: the clean run and the four perturbed runs at the largest iteration count (``griffin_lim_ref.runs``)."""
    x = gl_inputs(tag, B, T, gain, a)
    geom = G.GEOMETRIES[tag]
    n = max(GEOM_ITERS)
    out = []
    for b in range(B):
        S = x["mag"][b].astype(np.float64) ** power
        ph = x[init][b].astype(np.float64)
        out.append((griffin_lim(S, ph, n, geom, pad), [griffin_lim(S, ph, n, geom, pad, noise_seed=s) for s in G.SEEDS]))
    return out


def reference(case, init, power, n_iter):
    """-> (wav [B, n], residual [n_iter, B]) of the clean fp64 run."""
    r = runs(*case, init, power)
    return np.stack([c[0][n_iter] for c, _ in r]), np.stack([c[1][:n_iter] for c, _ in r], axis=1)


def tolerances(case, init, power, n_iter):
    """``griffin_lim_ref.tolerances``: (tol_wav [B] relative to max|y_ref|, tol_res [B] absolute)."""
    B = case[1]
    if n_iter == 0:
        return np.full(B, G.PLAIN_TOLERANCE), np.zeros(B)
    tw, tr = [], []
    for (cy, cr), pert in runs(*case, init, power):
        ref = cy[n_iter]
        tw.append(2.0 * max(np.abs(py[n_iter] - ref).max() for py, _ in pert) / np.abs(ref).max())
        tr.append(2.0 * max(np.abs(pr[:n_iter] - cr[:n_iter]).max() for _, pr in pert))
    return np.asarray(tw), np.asarray(tr)


def gl_cases():
    out = [(c, init, p, n) for c in GL_CASES for init in INITS for p in POWERS for n in GEOM_ITERS]
    return out, [f"{c[0]}-B{c[1]}-T{c[2]}-{c[4]}-{init}-p{p}-n{n}" for c, init, p, n in out]


# front end: (tag, B, T, gain, codec name, pre-emphasis).  G1 at T = 4 is the shortest legal clip: the reflection of the
# pre-emphasised clip lands on samples 0 and S - 1.
FRONT_CASES = [("G4", 3, 9, 0.25, "log", 0.0), ("G4", 3, 63, 0.25, "log", 0.0), ("G5", 2, 11, 0.25, "plain", 0.98)] + \
              [("G1", B, T, 1.0, v, a) for (B, T) in ((3, 4), (2, 9)) for v in DBNORM_VARIANTS for a in (0.0, 0.97)]


def front_codec(name, a):
    return log_codec() if name == "log" else dict(DBNORM_VARIANTS[name], preemphasis=float(a))


def front_block(tag, name, a):
    """The config block of a front-end case: waveglow for "log", else a wavernn block with the variant's flags."""
    geom = G.GEOMETRIES[tag]
    if name == "log":
        return waveglow_block(*geom)
    c = DBNORM_VARIANTS[name]
    if tag == "G5":
        return dict(WAVERNN, preemphasis=a)
    return wavernn_block(*geom, preemphasis=a, signal_norm=c["signal_norm"], symmetric_norm=c["symmetric_norm"], clip_norm=c["clip_norm"],
                         max_norm=c["max_norm"])
