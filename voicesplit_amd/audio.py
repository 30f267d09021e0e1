"""Audio front / back end of inference on the GPU: what test.py does around the
model for the "voicefilter" audio backend,

    mixed_spec, mixed_phase = ap.get_spec_from_audio(wav)              utils/audio_processor.py:469-476
    est_mask = model(mixed_spec, emb)                                   utils/generic_utils.py:495
    est_wav  = ap.inv_spectrogram(est_mask * mixed_spec, mixed_phase)   :496-504, audio_processor.py:478-491

as calls into libvoicesplit_hip.so: the STFT / iSTFT run as one GEMM against a windowed DFT basis
plus a gather (the analysis window is 400 of the 1200 frame samples, so the dense basis is small).

The other two back ends of ``WrapperAudioProcessor`` (``wavernn``, ``waveglow``: utils/audio_processor.py:61-438) run the same
transform with another codec around it (csrc/audio_codec.hip): every entry point below passes its ``audio_cfg`` through ``resolve``,
and ``AudioProcessor`` mirrors the wrapper class on device tensors.
"""
import ctypes
import math

import torch

import numpy as np

from . import _call, _lib
from .config import resolve_audio as resolve
from .losses import loss_dims


def frames_for(n_samples: int, hop: int) -> int:
    """librosa.stft(center=True): 1 + n_samples // hop frames."""
    return 1 + n_samples // hop


def wav_to_spec(wav: torch.Tensor, audio_cfg, want_phase: bool = True):
    """wav [B, hop*(T-1)] -> (spec [B,T,F] normalised dB magnitude in [0,1], phase [B,T,F] or None)."""
    audio_cfg = resolve(audio_cfg)
    if _foreign(audio_cfg):
        return _codec_wav_to_spec(wav, audio_cfg, want_phase, bool(audio_cfg["mel_spec"]))
    _call.dev_check(wav, "wav")
    B, S = wav.shape
    hop = int(audio_cfg["hop_length"])
    if S % hop:
        raise ValueError(f"wav length {S} must be a multiple of hop_length {hop} (crop or pad the clip)")
    T, F = S // hop + 1, int(audio_cfg["n_fft"]) // 2 + 1
    d = loss_dims(B, T, F, audio_cfg)
    ws = _call.scratch("audio", _call.sized("audio_workspace_bytes", ctypes.byref(d)), wav.device)
    spec = torch.empty(B, T, F, device=wav.device)
    phase = torch.empty(B, T, F, device=wav.device) if want_phase else None
    _call.call("wav_to_spec", wav.device, ctypes.byref(d), wav, spec, phase, ws, ws.numel())
    return spec, phase


def spec_to_wav(spec: torch.Tensor, phase: torch.Tensor = None, audio_cfg=None, mask: torch.Tensor = None,
                generator: torch.Generator = None) -> torch.Tensor:
    """(spec * mask), phase [B,T,F] -> wav [B, hop*(T-1)] (ap.inv_spectrogram with the given phase).  phase=None is the
    reference's ``ap.inv_spectrogram(spec)``: ``griffin_lim`` with the config's ``power`` and ``griffin_lim_iters`` (its random
    starting angles drawn from ``generator``).

    Under a wavernn or waveglow block the reference's ``inv_spectrogram`` DROPS the phase argument and always runs Griffin-Lim
    (utils/audio_processor.py:217-222, 394-402); here a given phase inverts with it (decode -> [mel -> linear] -> iSTFT ->
    de-emphasis where the block has a pre-emphasis).  That is this package's extension: pass phase=None for the reference's result."""
    if audio_cfg is None:
        raise TypeError("spec_to_wav: audio_cfg is required")
    audio_cfg = resolve(audio_cfg)
    if phase is None:
        return griffin_lim(spec, audio_cfg, mask=mask, generator=generator)
    if _foreign(audio_cfg):
        return _deemphasised(mag_to_wav(_linear_target(spec, audio_cfg, mask), phase, audio_cfg), audio_cfg)
    for n, t in (("spec", spec), ("phase", phase)):
        _call.dev_check(t, n)
    if mask is not None:
        _call.dev_check(mask, "mask")
    B, T, F = spec.shape
    d = loss_dims(B, T, F, audio_cfg)
    ws = _call.scratch("audio", _call.sized("audio_workspace_bytes", ctypes.byref(d)), spec.device)
    wav = torch.empty(B, d.hop * (T - 1), device=spec.device)
    _call.call("spec_to_wav", spec.device, ctypes.byref(d), spec, mask, phase, wav, ws, ws.numel())
    return wav


def griffin_lim(spec: torch.Tensor, audio_cfg, n_iter: int = None, power: float = None, init_phase: torch.Tensor = None,
                mask: torch.Tensor = None, generator: torch.Generator = None, return_residual: bool = False):
    """(spec * mask) [B,T,F] -> wav [B, hop*(T-1)] without a phase: ``_griffin_lim(S**power)`` of utils/audio_processor.py:492-496,
    516-523 in one resident loop on the device (vs_griffin_lim).  n_iter / power default to ``audio_cfg["griffin_lim_iters"]`` /
    ``audio_cfg["power"]``; init_phase=None draws ``2*pi*torch.rand`` on the device from ``generator`` (the reference's
    ``np.random.rand`` angles).  Started from a mixture's phase with power=1 it is the consistency refinement of a masked
    spectrogram.  return_residual: also ``|| |stft(y_i)| - S || / || S ||`` per iteration and item, fp64 [n_iter, B].
    Under a wavernn or waveglow block: decode -> [mel -> linear] -> ``griffin_lim_mag`` (the inner transform pads as the block's
    processor does) -> de-emphasis where the block has a pre-emphasis (inv_linear_spectrogram / inv_mel_spectrogram)."""
    audio_cfg = resolve(audio_cfg)
    if _foreign(audio_cfg):
        out = griffin_lim_mag(_linear_target(spec, audio_cfg, mask), audio_cfg, n_iter=n_iter, power=power, init_phase=init_phase,
                              generator=generator, return_residual=return_residual)
        return (_deemphasised(out[0], audio_cfg), out[1]) if return_residual else _deemphasised(out, audio_cfg)
    _call.dev_check(spec, "spec")
    if mask is not None:
        _call.dev_check(mask, "mask")
    n_iter = int(audio_cfg["griffin_lim_iters"] if n_iter is None else n_iter)
    power = float(audio_cfg["power"] if power is None else power)
    if init_phase is None:
        init_phase = 2.0 * math.pi * torch.rand(spec.shape, device=spec.device, dtype=torch.float32, generator=generator)
    _call.dev_check(init_phase, "init_phase")
    if init_phase.shape != spec.shape or (mask is not None and mask.shape != spec.shape):
        raise ValueError(f"init_phase / mask must have the shape of spec {tuple(spec.shape)}")
    B, T, F = spec.shape
    d = loss_dims(B, T, F, audio_cfg)
    ws = _call.scratch("audio", _call.sized("griffin_lim_workspace_bytes", ctypes.byref(d)), spec.device)
    wav = torch.empty(B, d.hop * (T - 1), device=spec.device)
    res = torch.empty(max(n_iter, 0), B, dtype=torch.float64, device=spec.device) if return_residual else None
    _call.call("griffin_lim", spec.device, ctypes.byref(d), spec, mask, init_phase, power, n_iter, wav, res, ws, ws.numel())
    return (wav, res) if return_residual else wav


# ---- the wavernn and waveglow back ends: codec, mel projection, inverse legs on a linear magnitude (csrc/audio_codec.hip) -----------
_CODEC_KINDS = {"DB01": _lib.CODEC_DB01, "DBNORM": _lib.CODEC_DBNORM, "LOG": _lib.CODEC_LOG}
_PADS = {"reflect": _lib.PAD_REFLECT, "zero": _lib.PAD_ZERO}
_MEL = {}


def _foreign(cfg) -> bool:
    return cfg.get("backend", "voicefilter") != "voicefilter"


def _refuse_foreign(audio_cfg, who: str):
    cfg = resolve(audio_cfg)
    if _foreign(cfg):
        raise ValueError(f"{who}: the {cfg['backend']} audio back end is not streamed (its inverse is Griffin-Lim over the whole clip); "
                         "use the voicefilter block")


def codec_of(audio_cfg) -> dict:
    """The codec of a block: ``resolve(block)['codec']``, or the voicefilter processor's DB01 (amp_to_db, normalize :537-547)."""
    cfg = resolve(audio_cfg)
    if "codec" in cfg:
        return cfg["codec"]
    return {"kind": "DB01", "floor": 1e-5, "min_level_db": float(cfg.get("min_level_db", -100.0)),
            "ref_level_db": float(cfg.get("ref_level_db", 20.0)), "signal_norm": False, "symmetric_norm": False, "clip_norm": False,
            "max_norm": 1.0, "preemphasis": 0.0, "gl_pad": "reflect"}


def _codec_struct(codec) -> "_lib.VsAudioCodec":
    return _lib.VsAudioCodec(_CODEC_KINDS[codec["kind"]], int(bool(codec["signal_norm"])), int(bool(codec["symmetric_norm"])),
                             int(bool(codec["clip_norm"])), _PADS[codec["gl_pad"]], 0, float(codec["floor"]),
                             float(codec["min_level_db"]), float(codec["ref_level_db"]), float(codec["max_norm"]),
                             float(codec["preemphasis"]))


def mel_basis(audio_cfg, device) -> torch.Tensor:
    """[num_mels, F] fp32 on ``device``: ``librosa.filters.mel(sample_rate, n_fft, num_mels, mel_fmin, mel_fmax)`` as
    ``speaker.mel_filterbank`` restates it, rounded to fp32 (kept per device and settings)."""
    return _mel(audio_cfg, device)[0]


def mel_pinv(audio_cfg, device) -> torch.Tensor:
    """[F, num_mels] fp32: ``np.linalg.pinv`` of the fp32 basis, taken in fp64 and rounded (``_mel_to_linear``)."""
    return _mel(audio_cfg, device)[1]


def _mel(audio_cfg, device):
    from .speaker import mel_filterbank
    cfg = resolve(audio_cfg)
    key = (torch.device(device).index, int(cfg.get("sample_rate", 16000)), int(cfg["n_fft"]), int(cfg.get("num_mels", 80)),
           float(cfg.get("mel_fmin") or 0.0), cfg.get("mel_fmax"))
    if key not in _MEL:
        w = mel_filterbank(key[1], key[2], key[3], key[4], key[5]).to(torch.float32)
        inv = torch.from_numpy(np.linalg.pinv(w.double().numpy())).to(torch.float32)
        _MEL[key] = (w.to(device).contiguous(), inv.to(device).contiguous())
    return _MEL[key]


def decode(spec: torch.Tensor, audio_cfg, mask: torch.Tensor = None) -> torch.Tensor:
    """Stored values (times mask) -> linear fp32 magnitudes of the same shape, under the block's codec; evaluated in fp64 on the
    device and rounded once."""
    _call.dev_check(spec, "spec")
    if mask is not None:
        _call.dev_check(mask, "mask")
        if mask.shape != spec.shape:
            raise ValueError(f"mask must have the shape of spec {tuple(spec.shape)}")
    c = _codec_struct(codec_of(audio_cfg))
    out = torch.empty_like(spec)
    _call.call("codec_decode", spec.device, ctypes.byref(c), spec, mask, spec.numel(), out)
    return out


def encode(mag: torch.Tensor, audio_cfg) -> torch.Tensor:
    """Linear magnitudes -> stored values of the block's codec (``max(floor, .)`` first)."""
    _call.dev_check(mag, "mag")
    c = _codec_struct(codec_of(audio_cfg))
    out = torch.empty_like(mag)
    _call.call("codec_encode", mag.device, ctypes.byref(c), mag, mag.numel(), out)
    return out


def project(x: torch.Tensor, w: torch.Tensor, floor: float = 0.0) -> torch.Tensor:
    """``max(floor, x @ w.T)``: x [..., K], w [N, K] -> [..., N], one fp32 FMA chain per output in the order of K."""
    _call.dev_check(x, "x")
    _call.dev_check(w, "w")
    if w.dim() != 2 or x.shape[-1] != w.shape[1]:
        raise ValueError(f"project: x {tuple(x.shape)} against w {tuple(w.shape)}")
    out = torch.empty(*x.shape[:-1], w.shape[0], device=x.device)
    _call.call("project_floor", x.device, x, w, out, x.numel() // x.shape[-1], w.shape[0], w.shape[1], float(floor))
    return out


def mel_to_linear(mel_mag: torch.Tensor, audio_cfg) -> torch.Tensor:
    """``np.maximum(1e-10, pinv(mel_basis) @ S)`` on linear mel magnitudes [..., num_mels] -> [..., F]."""
    return project(mel_mag, mel_pinv(audio_cfg, mel_mag.device), 1e-10)


def _linear_target(spec, cfg, mask=None):
    """The linear magnitude [B,T,F] the inverse legs start from: decode, then mel -> linear under ``mel_spec``."""
    mag = decode(spec, cfg, mask)
    return mel_to_linear(mag, cfg) if cfg.get("mel_spec") else mag


def _deemphasised(wav, cfg):
    a = float(codec_of(cfg)["preemphasis"])
    return deemphasis(wav, a) if a != 0.0 else wav


def _codec_wav_to_spec(wav, cfg, want_phase, mel):
    _call.dev_check(wav, "wav")
    B, S = wav.shape
    hop = int(cfg["hop_length"])
    if S % hop:
        raise ValueError(f"wav length {S} must be a multiple of hop_length {hop} (crop or pad the clip)")
    T, F = S // hop + 1, int(cfg["n_fft"]) // 2 + 1
    d = loss_dims(B, T, F, cfg)
    c = _codec_struct(codec_of(cfg))
    ws = _call.scratch("audio", _call.sized("audio_workspace_bytes", ctypes.byref(d)), wav.device)
    basis = mel_basis(cfg, wav.device) if mel else None
    n_mels = int(basis.shape[0]) if mel else 0
    spec = torch.empty(B, T, n_mels if mel else F, device=wav.device)
    phase = torch.empty(B, T, F, device=wav.device) if want_phase else None
    _call.call("codec_wav_to_spec", wav.device, ctypes.byref(d), ctypes.byref(c), wav, basis, n_mels, spec, phase, ws, ws.numel())
    return spec, phase


def wav_to_mel(wav: torch.Tensor, audio_cfg):
    """wav [B, hop*(T-1)] -> [B, T, num_mels] = encode(mel_basis @ |D|) (melspectrogram / mel_spectrogram), whatever ``mel_spec``."""
    cfg = resolve(audio_cfg)
    if not _foreign(cfg):
        raise ValueError("wav_to_mel: the voicefilter block has no mel spectrogram of this form; speaker.logmel is its get_mel")
    return _codec_wav_to_spec(wav, cfg, False, True)[0]


def mag_to_wav(mag: torch.Tensor, phase: torch.Tensor, audio_cfg) -> torch.Tensor:
    """A LINEAR magnitude and a phase [B,T,F] -> wav [B, hop*(T-1)]: ``spec_to_wav`` behind its decoder (no de-emphasis)."""
    for n, t in (("mag", mag), ("phase", phase)):
        _call.dev_check(t, n)
    if phase.shape != mag.shape:
        raise ValueError(f"phase must have the shape of mag {tuple(mag.shape)}")
    B, T, F = mag.shape
    d = loss_dims(B, T, F, audio_cfg)
    ws = _call.scratch("audio", _call.sized("audio_workspace_bytes", ctypes.byref(d)), mag.device)
    wav = torch.empty(B, d.hop * (T - 1), device=mag.device)
    _call.call("mag_to_wav", mag.device, ctypes.byref(d), mag, phase, wav, ws, ws.numel())
    return wav


def griffin_lim_mag(mag: torch.Tensor, audio_cfg, n_iter: int = None, power: float = None, init_phase: torch.Tensor = None,
                    pad: str = None, generator: torch.Generator = None, return_residual: bool = False):
    """``_griffin_lim(mag ** power)`` on a LINEAR magnitude [B,T,F] -> wav [B, hop*(T-1)] (no de-emphasis).  pad: "reflect" or "zero",
    the padding of the inner transform (None: the block's own: zeros for waveglow, utils/audio_processor.py:411-418).  The other
    arguments as in ``griffin_lim``."""
    cfg = resolve(audio_cfg)
    _call.dev_check(mag, "mag")
    n_iter = int(cfg["griffin_lim_iters"] if n_iter is None else n_iter)
    power = float(cfg["power"] if power is None else power)
    pad = codec_of(cfg)["gl_pad"] if pad is None else pad
    if pad not in _PADS:
        raise ValueError(f"griffin_lim_mag: pad {pad!r} is not one of {tuple(_PADS)}")
    if init_phase is None:
        init_phase = 2.0 * math.pi * torch.rand(mag.shape, device=mag.device, dtype=torch.float32, generator=generator)
    _call.dev_check(init_phase, "init_phase")
    if init_phase.shape != mag.shape:
        raise ValueError(f"init_phase must have the shape of mag {tuple(mag.shape)}")
    B, T, F = mag.shape
    d = loss_dims(B, T, F, cfg)
    ws = _call.scratch("audio", _call.sized("griffin_lim_workspace_bytes", ctypes.byref(d)), mag.device)
    wav = torch.empty(B, d.hop * (T - 1), device=mag.device)
    res = torch.empty(max(n_iter, 0), B, dtype=torch.float64, device=mag.device) if return_residual else None
    _call.call("griffin_lim_mag", mag.device, ctypes.byref(d), mag, init_phase, power, n_iter, _PADS[pad], wav, res, ws, ws.numel())
    return (wav, res) if return_residual else wav


def deemphasis_block() -> int:
    """Samples per block of the de-emphasis scan (``vs_deemphasis_block``)."""
    return int(_lib.load().vs_deemphasis_block())


def _rows(wav):
    if wav.dim() not in (1, 2) or wav.numel() == 0:
        raise ValueError(f"wav must be [n] or [B, n] and not empty, got {tuple(wav.shape)}")
    return wav.reshape(-1, wav.shape[-1])


def deemphasis(wav: torch.Tensor, coef: float) -> torch.Tensor:
    """y[n] = wav[n] + coef * y[n-1], y[-1] = 0 (``scipy.signal.lfilter([1], [1, -coef], wav)``, apply_inv_preemphasis) on wav [n] or
    [B, n]: a two-sweep scan in fp64 (vs_deemphasis); a row's bits do not depend on the batch around it."""
    _call.dev_check(wav, "wav")
    x = _rows(wav)
    B, N = x.shape
    ws = _call.scratch("deemph", _call.sized("deemphasis_workspace_bytes", B, N), wav.device)
    y = torch.empty_like(wav)
    _call.call("deemphasis", wav.device, x, y, B, N, float(coef), ws, ws.numel())
    return y


def preemphasis(wav: torch.Tensor, coef: float) -> torch.Tensor:
    """y[n] = wav[n] - coef * wav[n-1], wav[-1] = 0 (``lfilter([1, -coef], [1], wav)``, apply_preemphasis) on wav [n] or [B, n]; the
    difference in fp64, rounded once.  (The front end forms it inside its framing gather; this is the stand-alone filter.)"""
    _call.dev_check(wav, "wav")
    x = _rows(wav)
    y = torch.empty_like(wav)
    _call.call("preemphasis", wav.device, x, y, x.shape[0], x.shape[1], float(coef))
    return y


class AudioProcessor:
    """``WrapperAudioProcessor(config.audio)`` (utils/audio_processor.py:19-59) on device tensors, for the three back ends.
    Spectrograms are [time, freq] as the reference returns them; a waveform is [n] (one clip, as the reference takes it) or [B, n]
    with n a multiple of hop_length, and a batch dimension is carried through.  ``mel_spec`` (``config.audio['mel_spec']``) is
    honoured: ``get_spec_from_audio`` then returns mel features and ``inv_spectrogram`` takes them.

    Departures: ``get_spec_from_audio(wav, return_phase=True)`` returns the transform's phase for every back end (the reference
    returns None for wavernn / waveglow), and ``inv_spectrogram`` inverts with a phase when one is given (the reference drops it
    for those two); ``init_phase`` / ``generator`` choose Griffin-Lim's starting angles (``np.random.rand`` in the reference).
    Not here: load_wav, save_wav, do_trim_silence, the mu-law / quantisation helpers and the [-1, 1] input asserts."""

    def __init__(self, config_audio):
        self.cfg = resolve(config_audio)
        self.backend = self.cfg.get("backend", "voicefilter")
        self.mel_spec = bool(self.cfg.get("mel_spec", False)) and self.backend != "voicefilter"
        self.sample_rate = int(self.cfg.get("sample_rate", 16000))
        self.n_fft, self.hop_length, self.win_length = (int(self.cfg[k]) for k in ("n_fft", "hop_length", "win_length"))

    @staticmethod
    def _batched(t, dims):
        return (t, False) if t.dim() == dims else (t[None], True)

    def get_spec_from_audio(self, wav: torch.Tensor, return_phase: bool = False):
        x, one = self._batched(wav, 2)
        spec, phase = wav_to_spec(x.contiguous(), self.cfg, want_phase=return_phase)
        if one:
            spec, phase = spec[0], (phase[0] if phase is not None else None)
        return (spec, phase) if return_phase else spec

    def inv_spectrogram(self, spec: torch.Tensor, phase: torch.Tensor = None, init_phase: torch.Tensor = None,
                        generator: torch.Generator = None) -> torch.Tensor:
        s, one = self._batched(spec, 3)
        if phase is not None:
            wav = spec_to_wav(s.contiguous(), self._batched(phase, 3)[0].contiguous(), self.cfg)
        else:
            ip = None if init_phase is None else self._batched(init_phase, 3)[0].contiguous()
            wav = griffin_lim(s.contiguous(), self.cfg, init_phase=ip, generator=generator)
        return wav[0] if one else wav

    def get_mel(self, wav: torch.Tensor) -> torch.Tensor:
        """waveglow ``get_mel`` / wavernn ``melspectrogram``: [T, num_mels]; voicefilter: the log-mel of ``speaker.logmel``."""
        if self.backend == "voicefilter":
            from .speaker import logmel
            return logmel(wav, self.cfg, int(self.cfg.get("num_mels", 40)))
        x, one = self._batched(wav, 2)
        mel = wav_to_mel(x.contiguous(), self.cfg)
        return mel[0] if one else mel

    def mag_to_mel(self, y: torch.Tensor) -> torch.Tensor:
        """Stored linear-frequency values [T, F] -> stored mel values [T, num_mels]: encode(mel_basis @ decode(y))
        (mag_to_mel_spectrogram, utils/audio.py:119-135)."""
        if self.backend == "voicefilter":
            raise ValueError("mag_to_mel: the voicefilter audio back end has no mel form of its spectrogram")
        return encode(project(decode(y.contiguous(), self.cfg), mel_basis(self.cfg, y.device)), self.cfg)


_RESAMPLERS = {}


def resampler(sr_in: int, sr_out: int, device):
    """The ``resample.Resampler`` of this pair of rates on this device (its tap bank is built once and kept)."""
    from .resample import Resampler
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sr_in), int(sr_out), device)
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = Resampler(sr_in, sr_out, device)
    return _RESAMPLERS[key]


def resample(wav: torch.Tensor, sr_in: int, sr_out: int) -> torch.Tensor:
    """wav [n] or [B, n] at ``sr_in`` -> [.., ceil(n sr_out / sr_in)] at ``sr_out`` (``librosa.load(path, sr=sr_out)``'s conversion,
    csrc/resample.hip)."""
    return resampler(sr_in, sr_out, wav.device)(wav)


def separate(model, wav: torch.Tensor, dvec: torch.Tensor, audio_cfg, refine_iters: int = 0, sample_rate: int = None,
             loudness: float = None) -> torch.Tensor:
    """Target-speaker waveform for a batch of 3 s mixtures, all on the device:
    wav [B, hop*(T-1)], dvec [B, emb_dim] -> est_wav [B, hop*(T-1)]   (test.py's loop body).  refine_iters > 0: that many
    Griffin-Lim rounds on the masked spectrogram, started from the mixture's phase (``griffin_lim`` with power 1).
    sample_rate: the rate of ``wav`` when it is not ``audio_cfg["sample_rate"]`` (16000 when the config names none); wav is then
    [B, n] for any n: converted to the configured rate, padded with zeros to a multiple of hop_length, separated, converted back
    and cut to n samples.
    loudness: None, or the level in LUFS of the corpus the network was trained on: every row is first brought there
    (``loudness.normalize_clips_`` at the rate of ``wav``: BS.1770 integrated loudness, one linear gain g under a -2 dB peak cap) and
    the estimate is returned at the input's own level, multiplied by fp32(1 / g).  Rows without a loudness keep g = 1."""
    audio_cfg = resolve(audio_cfg)
    own = int(audio_cfg.get("sample_rate", 16000))
    if loudness is not None:
        from .loudness import _rows_table, normalize_clips_
        x = wav.contiguous().clone()
        gain = normalize_clips_(*_rows_table(x), int(sample_rate) if sample_rate is not None else own, float(loudness))[1]
        return separate(model, x, dvec, audio_cfg, refine_iters, sample_rate) * (1.0 / gain)[:, None]
    if sample_rate is not None and int(sample_rate) != own:
        n, hop = wav.shape[1], int(audio_cfg["hop_length"])
        x = resample(wav, int(sample_rate), own)
        x = torch.nn.functional.pad(x, (0, -x.shape[1] % hop))
        est = separate(model, x, dvec, audio_cfg, refine_iters)
        return resample(est, own, int(sample_rate))[:, :n]
    spec, phase = wav_to_spec(wav, audio_cfg)
    with torch.no_grad():
        mask = model(spec, dvec)
    if refine_iters > 0:
        return griffin_lim(spec, audio_cfg, n_iter=refine_iters, power=1.0, init_phase=phase, mask=mask)
    return spec_to_wav(spec, phase, audio_cfg, mask=mask)


def _multi_shapes(wav_shape, dvecs_shape):
    """(B, n, K) of ``separate_speakers`` after the shape checks that need no device."""
    if len(wav_shape) != 2:
        raise ValueError(f"wav must be [B, n], got {tuple(wav_shape)}")
    if len(dvecs_shape) != 3 or dvecs_shape[0] != wav_shape[0] or dvecs_shape[1] < 1:
        raise ValueError(f"dvecs must be [B={wav_shape[0]}, K >= 1, emb_dim], got {tuple(dvecs_shape)}")
    return int(wav_shape[0]), int(wav_shape[1]), int(dvecs_shape[1])


def separate_speakers(model, wav: torch.Tensor, dvecs: torch.Tensor, audio_cfg) -> torch.Tensor:
    """K enrolled speakers out of every mixture: wav [B, hop*(T-1)], dvecs [B, K, emb_dim] -> est_wav [B, K, hop*(T-1)]; row [b, k]
    is ``separate(model, wav[b:b+1], dvecs[b:b+1, k])``.  One STFT, one ``model.forward_multi`` (one conv pass), one iSTFT over
    the B*K rows with the mixture's spectrogram and phase repeated."""
    B, n, K = _multi_shapes(wav.shape, dvecs.shape)
    spec, phase = wav_to_spec(wav, audio_cfg)
    with torch.no_grad():
        masks = model.forward_multi(spec, dvecs)
    T, F = spec.shape[1], spec.shape[2]
    if tuple(masks.shape) != (B, K, T, F):
        raise ValueError(f"forward_multi returned {tuple(masks.shape)}, expected {(B, K, T, F)}")

    def per_speaker(t):          # [B, T, F] -> [B*K, T, F], row b*K + k = mixture b
        return t[:, None].expand(B, K, T, F).reshape(B * K, T, F).contiguous()

    est = spec_to_wav(per_speaker(spec), per_speaker(phase), audio_cfg, mask=masks.reshape(B * K, T, F).contiguous())
    return est.view(B, K, n)


def separate_speakers_with_reference(model, encoder, wav: torch.Tensor, ref_wavs, audio_cfg) -> torch.Tensor:
    """``separate_speakers`` with the d-vectors computed here: ref_wavs[b] = a list of K reference waveforms (1-D, the same K for
    every mixture; lengths as in ``separate_with_reference``), embedded in one ``encoder.embed_many`` call."""
    return separate_speakers(model, wav, _embed_references(encoder, ref_wavs, wav.shape[0], audio_cfg), audio_cfg)


def _embed_references(encoder, ref_wavs, B: int, audio_cfg) -> torch.Tensor:
    """d-vectors [B, K, emb_dim] of B lists of K reference waveforms each, in one ``encoder.embed_many`` call."""
    from .speaker import logmel
    if len(ref_wavs) != B:
        raise ValueError(f"{len(ref_wavs)} lists of reference waveforms for {B} mixtures")
    K = len(ref_wavs[0]) if len(ref_wavs) else 0
    if K < 1 or any(len(r) != K for r in ref_wavs):
        raise ValueError(f"every mixture needs the same number K >= 1 of reference waveforms, got {[len(r) for r in ref_wavs]}")
    flat = [r for refs in ref_wavs for r in refs]
    dvec, valid = encoder.embed_many([logmel(r, audio_cfg, encoder.num_mels) for r in flat])
    if not bool(valid.all()):
        short = [(i // K, i % K) for i, v in enumerate(valid.tolist()) if not v]
        raise ValueError(f"reference waveforms {short} (mixture, speaker) are shorter than one encoder window of {encoder.window} frames")
    return dvec.view(B, K, -1).contiguous()


class StreamingSeparator:
    """``separate`` on a live stream: ``push(samples [B, n * hop_length])`` returns the separated samples that became final
    ([B, k * hop_length], k >= 0), ``finish()`` the rest; the concatenation covers every pushed sample.  Host glue over
    ``wav_to_spec`` / ``spec_to_wav`` and ``streaming.StreamingMasker`` (chunks of ``C`` frames, ``R`` frames of look-ahead):

    * STFT: the pending samples are transformed as one segment; its reflect padding reaches ``margin = ceil(n_fft / 2 / hop)``
      frames in from each end, so frames that close to a segment edge that is not a stream edge are dropped, and the samples
      they need are kept and transformed again with the next segment.  ``wav_to_spec`` takes a segment only if it is longer
      than n_fft / 2 samples, so a segment has at least ``hold = n_fft / 2 // hop + 1`` hops: ``margin`` of them, or one more
      where hop divides n_fft / 2 and ``margin`` hops are exactly as long as the padding.  Until the stream has ``hold`` hops no
      frame is taken, and that many hops are kept in front of the first frame still to come;
    * iSTFT: the masked frames are inverted as one segment; the overlap-add of a sample within ``margin`` frames of a segment
      edge that is not a stream edge misses frames, so those samples are dropped and their frames are inverted again later.

    A sample is returned once ``latency_samples`` more have been pushed (or at ``finish()``).

    Several enrolled speakers per stream: ``dvec [B, K, emb_dim]`` -> ``push`` / ``finish`` return ``[B, K, n]``; row [b, k] is the
    stream b separated for ``dvec[b, k]``.  STFT, conv windows and the LSTM input GEMM run once per mixture (the K-speaker
    ``StreamingMasker``); spectrogram and phase are kept once per mixture and repeated per speaker only for ``spec_to_wav``, as
    in ``separate_speakers``.  ``latency_samples`` is that of one speaker.  ``with_reference`` embeds the K reference waveforms."""

    def __init__(self, model, dvec: torch.Tensor, audio_cfg, C: int, R: int, trace: bool = False):
        from .streaming import StreamingMasker
        _refuse_foreign(audio_cfg, "StreamingSeparator")
        self.K = int(dvec.shape[1]) if dvec.dim() == 3 else None      # None: one speaker per stream, [B, n] out
        self.mask_trace = [] if trace else None  # trace: every block of mask rows, in order
        self.cfg = audio_cfg
        self.hop = int(audio_cfg["hop_length"])
        self.margin = -(-(int(audio_cfg["n_fft"]) // 2) // self.hop)
        self.hold = int(audio_cfg["n_fft"]) // 2 // self.hop + 1      # the fewest hops wav_to_spec takes: hold * hop > n_fft / 2
        self.masker = StreamingMasker(*model.stream_stages(), dvec, C, R)
        self.finished = False
        self._wav, self._w0 = None, 0            # samples from frame _w0 (sample _w0 * hop) on
        self._hops = 0                           # pushed samples / hop
        self._frames = 0                         # STFT frames handed to the masker
        self._spec = self._phase = None          # frames [_s0, _frames)
        self._mask = None                        # rows [_s0, _rows); K speakers: [B*K, rows, F], row b*K + k
        self._s0 = self._rows = 0
        self._out = 0                            # returned samples / hop

    @classmethod
    def with_reference(cls, model, encoder, ref_wavs, audio_cfg, C: int, R: int, trace: bool = False):
        """The K-speaker separator with the d-vectors computed here, once: ref_wavs[b] = a list of K reference waveforms (1-D, the
        same K for every stream; lengths as in ``separate_with_reference``), embedded in one ``encoder.embed_many`` call, as
        ``separate_speakers_with_reference`` does."""
        return cls(model, _embed_references(encoder, ref_wavs, len(ref_wavs), audio_cfg), audio_cfg, C, R, trace=trace)

    @property
    def latency_samples(self) -> int:
        """A returned block starts ``latency_samples`` behind the newest pushed sample: frames the STFT holds back (margin), the
        masker's chunk, look-ahead and conv halo, and the frames the iSTFT holds back (margin + the frame that closes a hop).
        Where the first analysis waits for one hop more than ``margin`` (see ``hold``) the frames it withheld arrive with that hop,
        long before the masker's first chunk is due, so the bound is the same."""
        return (self.masker.latency_frames + 2 * self.margin) * self.hop

    def push(self, samples: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingSeparator: the stream has been finished")
        if samples.dim() != 2 or samples.shape[1] % self.hop:
            raise ValueError(f"samples must be [B, n * hop_length = n * {self.hop}], got {tuple(samples.shape)}")
        self._wav = samples if self._wav is None else torch.cat((self._wav, samples), dim=1)
        self._hops += samples.shape[1] // self.hop
        return self._advance()

    def finish(self) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingSeparator: the stream has been finished")
        if self._wav is None:
            raise RuntimeError("StreamingSeparator: finish() on a stream that never received a sample")
        self.finished = True
        return self._advance()

    def _advance(self) -> torch.Tensor:
        m, hop = self.margin, self.hop
        # analysis: frames [_frames, n_valid) are exact now (a segment of fewer than hold hops is too short to transform: wait)
        if self.finished:
            n_valid = self._hops + 1
        else:
            n_valid = max(0, self._hops - m + 1) if self._hops - self._w0 >= self.hold else self._frames
        masks = []
        if n_valid > self._frames and self._hops > self._w0:
            spec, phase = wav_to_spec(self._wav.contiguous(), self.cfg)                  # frames [_w0, _hops]
            spec = spec[:, self._frames - self._w0:n_valid - self._w0]
            phase = phase[:, self._frames - self._w0:n_valid - self._w0]
            self._spec = spec if self._spec is None else torch.cat((self._spec, spec), dim=1)
            self._phase = phase if self._phase is None else torch.cat((self._phase, phase), dim=1)
            self._frames = n_valid
            w0 = max(0, self._frames - self.hold)
            self._wav, self._w0 = self._wav[:, (w0 - self._w0) * hop:], w0
            masks.append(self.masker.push(spec.contiguous()))
        if self.finished and self._frames:
            masks.append(self.masker.finish())
        for mk in masks:
            if mk.shape[-2]:
                if self.mask_trace is not None:
                    self.mask_trace.append(mk)
                if self.K is not None:       # [B, K, m, F] -> [B*K, m, F], row b*K + k
                    mk = mk.reshape(-1, mk.shape[2], mk.shape[3])
                self._mask = mk if self._mask is None else torch.cat((self._mask, mk), dim=1)
                self._rows += mk.shape[1]
        # synthesis: samples [_out * hop, done * hop) are exact now
        done = self._hops if self.finished else self._rows - 1 - m
        B = self._wav.shape[0]
        if done <= self._out or self._mask is None:
            return self._wav.new_empty(B, 0) if self.K is None else self._wav.new_empty(B, self.K, 0)
        fa = max(0, self._out - m)
        lo, hi = fa - self._s0, self._rows - self._s0

        def rows(t):             # the mixture's frames, K speakers: repeated per speaker, [B*K, n, F] with row b*K + k = mixture b
            t = t[:, lo:hi]
            return t.contiguous() if self.K is None else t[:, None].expand(B, self.K, *t.shape[1:]).reshape(B * self.K, *t.shape[1:]).contiguous()

        wav = spec_to_wav(rows(self._spec), rows(self._phase), self.cfg,
                          mask=self._mask[:, lo:hi].contiguous())                        # samples [fa * hop, (_rows - 1) * hop)
        out = wav[:, (self._out - fa) * hop:(done - fa) * hop]
        if self.K is not None:
            out = out.reshape(B, self.K, -1)
        self._out = done
        s0 = max(0, self._out - m)
        self._spec, self._phase, self._mask = self._spec[:, s0 - self._s0:], self._phase[:, s0 - self._s0:], self._mask[:, s0 - self._s0:]
        self._s0 = s0
        return out


class StreamingSeparatorAtRate:
    """``StreamingSeparator`` for a stream at ``sample_rate`` instead of the configured rate (a sound card's 48000 or 44100):
    ``push(samples [B, k])`` for any k returns the separated samples that became final ([B, m], m >= 0, at ``sample_rate``),
    ``finish()`` the rest; the concatenation has exactly the pushed length.  A ``resample.StreamingResampler`` on each side; the
    converted samples wait here until a multiple of hop_length is pending (at ``finish()`` the last block is padded with zeros).
    What it returns is ``StreamingSeparator`` fed the whole converted stream (so padded), converted back and cut.
    ``dvec [B, K, emb_dim]``: ``[B, K, m]`` out; the conversion back runs on the B*K rows (a row's output does not depend on the
    others: the resampler's own guarantee)."""

    def __init__(self, model, dvec: torch.Tensor, audio_cfg, C: int, R: int, sample_rate: int):
        from .resample import StreamingResampler
        _refuse_foreign(audio_cfg, "StreamingSeparatorAtRate")
        own = int(audio_cfg.get("sample_rate", 16000))
        self.sample_rate, self.own_rate = int(sample_rate), own
        self.hop = int(audio_cfg["hop_length"])
        self.sep = StreamingSeparator(model, dvec, audio_cfg, C, R)
        self.K = self.sep.K
        self.down = StreamingResampler(self.sample_rate, own, dvec.device, resampler=resampler(self.sample_rate, own, dvec.device))
        self.up = StreamingResampler(own, self.sample_rate, dvec.device, resampler=resampler(own, self.sample_rate, dvec.device))
        self.finished = False
        self._pending = None                     # converted samples not yet handed to the separator (fewer than hop after a push)
        self._pushed = self._returned = 0        # at sample_rate

    @property
    def latency_samples(self) -> int:
        """At ``sample_rate``: a sample is returned once this many more have been pushed.  Its converted sample exists H_down
        pushed samples later; at the configured rate it then waits for its hop to fill (hop_length), for the separator
        (``StreamingSeparator.latency_samples``) and for the H_up samples behind it that the conversion back reads."""
        own = self.hop + self.sep.latency_samples + self.up.dims.H
        return self.down.dims.H + -(-own * self.sample_rate // self.own_rate)

    def _feed(self, x: torch.Tensor, last: bool) -> torch.Tensor:
        self._pending = x if self._pending is None else torch.cat((self._pending, x), dim=1)
        if last:
            self._pending = torch.nn.functional.pad(self._pending, (0, -self._pending.shape[1] % self.hop))
        n = self._pending.shape[1] // self.hop * self.hop
        block, self._pending = self._pending[:, :n].contiguous(), self._pending[:, n:]

        def flat(t):             # [B, K, n] -> the up-resampler's rows [B*K, n]
            return t if self.K is None else t.reshape(-1, t.shape[2])

        outs = [self.up.push(flat(self.sep.push(block)))] if n else []
        if last:
            outs += [self.up.push(flat(self.sep.finish())), self.up.finish()]
        if not outs:
            return x.new_empty(x.shape[0], 0) if self.K is None else x.new_empty(x.shape[0], self.K, 0)
        out = torch.cat(outs, dim=1)[:, :self._pushed - self._returned]
        self._returned += out.shape[1]
        return out if self.K is None else out.reshape(x.shape[0], self.K, -1)

    def push(self, samples: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingSeparatorAtRate: the stream has been finished")
        if samples.dim() != 2:
            raise ValueError(f"samples must be [B, k], got {tuple(samples.shape)}")
        self._pushed += samples.shape[1]
        return self._feed(self.down.push(samples.contiguous()), False)

    def finish(self) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingSeparatorAtRate: the stream has been finished")
        if self._pushed == 0:
            raise RuntimeError("StreamingSeparatorAtRate: finish() on a stream that never received a sample")
        self.finished = True
        return self._feed(self.down.finish(), True)


# frames a ragged batch may occupy (items * longest item): 64 clips of 3 s, the batch the workspace of the 3 s path is sized for anyway
RAGGED_MAX_ITEMS = 64
RAGGED_MAX_FRAMES = 64 * 301


def pad_specs(specs, device=None):
    """List of [T_i, F] (or [1, T_i, F]) spectrograms -> (x [B, Tmax, F] zero padded, lengths list)."""
    specs = [s.reshape(-1, s.shape[-1]) for s in specs]
    lengths = [int(s.shape[0]) for s in specs]
    x = torch.zeros(len(specs), max(lengths), specs[0].shape[1], dtype=specs[0].dtype, device=device or specs[0].device)
    for b, s in enumerate(specs):
        x[b, :lengths[b]] = s
    return x, lengths


def masks_ragged(model, specs, dvecs, max_items: int = RAGGED_MAX_ITEMS, max_frames: int = RAGGED_MAX_FRAMES):
    """Masks of clips of unequal length through ``model.forward_ragged`` in planner batches: specs = list of [T_i, F],
    dvecs [N, emb_dim] -> list of masks [T_i, fc2_dim], each what the model gives for that clip alone."""
    from .streaming import plan_ragged_batches
    lengths = [int(s.shape[0]) for s in specs]
    out = [None] * len(specs)
    with torch.no_grad():
        for batch in plan_ragged_batches(lengths, max_items, max_frames):
            x, lens = pad_specs([specs[i] for i in batch])
            mask = model.forward_ragged(x, dvecs[batch].contiguous(), lens)
            for b, i in enumerate(batch):
                out[i] = mask[b, :lens[b]]
    return out


def separate_many(model, wavs, dvecs: torch.Tensor, audio_cfg, max_items: int = RAGGED_MAX_ITEMS, max_frames: int = RAGGED_MAX_FRAMES):
    """``separate`` for clips of unequal length: wavs = list of 1-D waveforms (each a multiple of hop_length samples),
    dvecs [N, emb_dim] -> list of estimated waveforms, each equal to ``separate`` on that clip alone.  The STFT reflects at each
    clip's own ends and the iSTFT's envelope ends there, so front and back end run per group of clips of equal length; the
    network runs on ragged batches of the whole list (``streaming.plan_ragged_batches``).  max_items / max_frames bound a batch
    (clips, and clips x longest clip in frames): the workspace grows with the latter, about 0.36 MB per frame at full width."""
    if len(wavs) != dvecs.shape[0]:
        raise ValueError(f"{len(wavs)} waveforms for {dvecs.shape[0]} d-vectors")
    audio_cfg = resolve(audio_cfg)
    if audio_cfg.get("mel_spec"):
        raise ValueError("separate_many: forward_ragged takes linear spectrograms; the audio block has mel_spec set")
    groups = {}
    for i, w in enumerate(wavs):
        if w.dim() != 1:
            raise ValueError(f"wavs[{i}]: expected a 1-D waveform, got {tuple(w.shape)}")
        groups.setdefault(int(w.shape[0]), []).append(i)
    specs, phases = [None] * len(wavs), [None] * len(wavs)
    for idx in groups.values():
        spec, phase = wav_to_spec(torch.stack([wavs[i] for i in idx]).contiguous(), audio_cfg)
        for k, i in enumerate(idx):
            specs[i], phases[i] = spec[k], phase[k]
    masks = masks_ragged(model, specs, dvecs, max_items, max_frames)
    out = [None] * len(wavs)
    for idx in groups.values():
        est = spec_to_wav(torch.stack([specs[i] for i in idx]), torch.stack([phases[i] for i in idx]), audio_cfg,
                          mask=torch.stack([masks[i] for i in idx]))
        for k, i in enumerate(idx):
            out[i] = est[k]
    return out


def separate_with_reference(model, encoder, wav: torch.Tensor, ref_wavs, audio_cfg) -> torch.Tensor:
    """``separate`` with the d-vectors computed here from reference audio of the wanted speakers: ref_wavs = one 1-D
    waveform per row of wav (any length above n_fft / 2 samples and at least one encoder window of frames);
    encoder = a ``speaker.SpeakerEncoder`` on the device."""
    from .speaker import logmel
    if len(ref_wavs) != wav.shape[0]:
        raise ValueError(f"{len(ref_wavs)} reference waveforms for {wav.shape[0]} mixtures")
    dvec, valid = encoder.embed_many([logmel(r, audio_cfg, encoder.num_mels) for r in ref_wavs])
    if not bool(valid.all()):
        short = [i for i, v in enumerate(valid.tolist()) if not v]
        raise ValueError(f"reference waveforms {short} are shorter than one encoder window of {encoder.window} frames")
    return separate(model, wav, dvec, audio_cfg)
