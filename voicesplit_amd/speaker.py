"""GE2E speaker encoder on the GPU: reference audio -> the 256-d d-vector every other path here takes as ``dvec``.

What the reference does in notebooks/GE2E-Seungwonpark-ExtractSpeakerEmbedding-...py, as calls into
libvoicesplit_hip.so (csrc/speaker.hip):

    mel  = ap.get_mel(wav)                        ->  logmel(wav, audio_cfg)                 utils/audio_processor.py:460-467
    dvec = embedder(mel)                          ->  SpeakerEncoder()(mel)                  notebook :63-85
    the loop over ``*-ref_emb.wav``               ->  python -m voicesplit_amd.speaker       notebook :128-152

``SpeakerEncoder`` has the notebook class's ``state_dict`` (``lstm.*``, ``proj.linear_layer.*``), so the published
``embedder.pt`` loads with ``strict=True``.  Inference only: the reference never trains the encoder, so nothing here
records an autograd graph.  There is no CPU fallback.
"""
import argparse
import ctypes
import glob
import os
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _call, _lib
from .config import resolve_audio
from .losses import loss_dims
from .ops import MATH_CODES

_BASIS = {}


# ---- mel filterbank: librosa.filters.mel(sr, n_fft, n_mels) with its defaults, restated in fp64 ---------------------------
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = 15.0                         # 1000 Hz at 200/3 Hz per mel
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    """Slaney scale: linear at 200/3 Hz per mel below 1 kHz, logarithmic with step ln(6.4)/27 above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    log = _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP
    return np.where(f >= _MIN_LOG_HZ, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    lin = m * 200.0 / 3.0
    log = _MIN_LOG_HZ * np.exp(_LOGSTEP * (np.maximum(m, _MIN_LOG_MEL) - _MIN_LOG_MEL))
    return np.where(m >= _MIN_LOG_MEL, log, lin)


def mel_band_edges(sr: int, n_mels: int, fmin: float = 0.0, fmax: float = None) -> np.ndarray:
    """The n_mels + 2 band edges in Hz: equally spaced in mel from fmin (0) to fmax (None: sr / 2)."""
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(sr / 2.0 if fmax is None else fmax), n_mels + 2))


def mel_filterbank(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: float = None) -> torch.Tensor:
    """[n_mels, n_fft // 2 + 1] float64: triangles on the FFT bin centres between consecutive Slaney band edges, each row scaled
    by 2 / (f_hi - f_lo) (the "slaney" area norm).  fmin / fmax: librosa.filters.mel's keywords (the wavernn and waveglow blocks
    set 0 and 8000).  librosa is not a dependency; parity with its own array is not pinned by a test."""
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    edges = mel_band_edges(sr, n_mels, fmin, fmax)
    fdiff = np.diff(edges)
    ramps = edges[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return torch.from_numpy(w)


def _basis_on(device, sr: int, n_fft: int, n_mels: int) -> torch.Tensor:
    key = (torch.device(device).index, sr, n_fft, n_mels)
    b = _BASIS.get(key)
    if b is None:
        b = mel_filterbank(sr, n_fft, n_mels).to(torch.float32).to(device).contiguous()
        _BASIS[key] = b
    return b


def logmel(wav: torch.Tensor, audio_cfg, num_mels: int = 40) -> torch.Tensor:
    """ap.get_mel on the device: wav [n] (any n > n_fft / 2) -> [num_mels, 1 + n // hop_length] log10 mel power."""
    _call.dev_check(wav, "wav")
    if wav.dim() != 1:
        raise ValueError(f"wav: expected one clip [n], got {tuple(wav.shape)}")
    n = wav.numel()
    audio_cfg = resolve_audio(audio_cfg)
    n_fft, hop = int(audio_cfg["n_fft"]), int(audio_cfg["hop_length"])
    d = loss_dims(1, 1 + n // hop, n_fft // 2 + 1, audio_cfg)
    ws = _call.scratch("logmel", _call.sized("logmel_workspace_bytes", ctypes.byref(d), n, int(num_mels)), wav.device)
    basis = _basis_on(wav.device, int(audio_cfg.get("sample_rate", 16000)), n_fft, int(num_mels))
    mel = torch.empty(int(num_mels), 1 + n // hop, device=wav.device)
    _call.call("wav_to_logmel", wav.device, ctypes.byref(d), wav, n, basis, int(num_mels), mel, ws, ws.numel())
    return mel


# ---- window plan ------------------------------------------------------------------------------------------------------------
def window_count(T: int, window: int = 80, stride: int = 40) -> int:
    """Windows of ``mel.unfold(1, window, stride)``: (T - window) // stride + 1, 0 for a clip shorter than one window."""
    return (T - window) // stride + 1 if T >= window else 0


def window_plan(frame_counts: Sequence[int], window: int = 80, stride: int = 40):
    """Offsets of a ragged batch laid side by side along time: (frame offsets [U + 1], window offsets [U + 1])."""
    frames, wins = [0], [0]
    for T in frame_counts:
        frames.append(frames[-1] + int(T))
        wins.append(wins[-1] + window_count(int(T), window, stride))
    return frames, wins


class LinearNorm(nn.Module):
    def __init__(self, lstm_hidden, emb_dim):
        super().__init__()
        self.linear_layer = nn.Linear(lstm_hidden, emb_dim)


class SpeakerEncoder(nn.Module):
    """The notebook's encoder: 3-layer LSTM(40 -> 768) over sliding windows of 80 mel frames (stride 40), last frame,
    Linear(768 -> 256), L2 normalisation per window, mean over the windows.  The packed weights are built once per set of
    parameters, on the stream current at that moment; every later use makes its own stream wait for that on the device
    (``_call.Built``), so the encoder may be prepared under one stream and used under any other."""

    _TRANSIENT = ("_prepared",)

    def __init__(self, num_mels=40, lstm_layers=3, lstm_hidden=768, emb_dim=256, window=80, stride=40):
        super().__init__()
        self.lstm = nn.LSTM(num_mels, lstm_hidden, num_layers=lstm_layers, batch_first=True)
        self.proj = LinearNorm(lstm_hidden, emb_dim)
        self.num_mels, self.lstm_layers, self.lstm_hidden, self.emb_dim = num_mels, lstm_layers, lstm_hidden, emb_dim
        self.window, self.stride = window, stride
        self.math = "f16x3"          # or "fp32" (the cross-check arm); "bf16" is refused by the library

    def __getstate__(self):
        state = dict(self.__dict__)
        for k in self._TRANSIENT:
            state.pop(k, None)
        return state

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update({k: copy.deepcopy(v, memo) for k, v in self.__getstate__().items()})
        return new

    def _dims(self) -> "_lib.VsSpeakerDims":
        if self.math not in MATH_CODES:
            raise ValueError(f"math must be one of {sorted(MATH_CODES)}")
        return _lib.VsSpeakerDims(self.num_mels, self.lstm_hidden, self.lstm_layers, self.emb_dim, self.window, self.stride,
                                  MATH_CODES[self.math])

    def _param_list(self) -> List[torch.Tensor]:
        ps = []
        for k in range(self.lstm_layers):
            ps += [getattr(self.lstm, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return ps + [self.proj.linear_layer.weight, self.proj.linear_layer.bias]

    def _prepare(self, device):
        """The packed weights, rebuilt when a parameter was replaced, edited in place (version counter) or the arithmetic changed."""
        ps = self._param_list()
        for p in ps:
            _call.dev_check(p.detach(), "SpeakerEncoder parameter")
            if p.device != device:
                raise ValueError(f"SpeakerEncoder parameters are on {p.device}, the input on {device}")
        key = (self.math,) + tuple((p.data_ptr(), p._version) for p in ps)
        prep = self.__dict__.get("_prepared")
        if prep is not None and prep[0] == key:
            prep[2].wait()
            return prep[1]
        d = self._dims()
        buf = torch.empty(_call.sized("speaker_prepared_bytes", ctypes.byref(d)), dtype=torch.uint8, device=device)
        sp = _lib.VsSpeakerParams()
        for k in range(self.lstm_layers):
            sp.w_ih[k], sp.w_hh[k], sp.b_ih[k], sp.b_hh[k] = (p.data_ptr() for p in ps[4 * k:4 * k + 4])
        sp.proj_w, sp.proj_b = ps[-2].data_ptr(), ps[-1].data_ptr()
        _call.call("speaker_prepare", device, ctypes.byref(d), ctypes.byref(sp), buf, buf.numel())
        self.__dict__["_prepared"] = (key, buf, _call.Built(device))
        return buf

    @torch.no_grad()
    def embed_many(self, mels: Sequence[torch.Tensor], return_stages: bool = False):
        """All windows of all utterances as ONE batch.  mels: list of [num_mels, T_u] device tensors.
        Returns (dvec [U, emb_dim], valid [U] bool): a clip shorter than one window has valid = False and a zero row.
        return_stages: also h_last [N, lstm_hidden], proj [N, emb_dim] (un-normalised) and the window offsets [U + 1]."""
        if len(mels) == 0:
            raise ValueError("embed_many: empty list")
        for m in mels:
            _call.dev_check(m, "mel")
            if m.dim() != 2 or m.shape[0] != self.num_mels:
                raise ValueError(f"mel: expected [{self.num_mels}, T], got {tuple(m.shape)}")
        device = mels[0].device
        frames, wins = window_plan([m.shape[1] for m in mels], self.window, self.stride)
        U, N, total = len(mels), wins[-1], frames[-1]
        valid = torch.tensor([wins[u + 1] > wins[u] for u in range(U)], dtype=torch.bool)
        dvec = torch.zeros(U, self.emb_dim, device=device)
        if N == 0:
            empty = (torch.empty(0, self.lstm_hidden, device=device), torch.empty(0, self.emb_dim, device=device), wins)
            return (dvec, valid) + (empty if return_stages else ())
        prepared = self._prepare(device)
        mel = (mels[0] if U == 1 else torch.cat(list(mels), dim=1)).detach().contiguous()
        d = self._dims()
        ws = _call.scratch("embed", _call.sized("speaker_workspace_bytes", ctypes.byref(d), N, total), device)
        offs = torch.tensor([frames, wins], dtype=torch.int32).to(device)
        h_last = torch.empty(N, self.lstm_hidden, device=device) if return_stages else None
        proj = torch.empty(N, self.emb_dim, device=device) if return_stages else None
        _call.call("speaker_embed", device, ctypes.byref(d), prepared, prepared.numel(), mel, total, offs[0], offs[1], U, N,
                   h_last, proj, dvec, ws, ws.numel())
        return (dvec, valid) + ((h_last, proj, wins) if return_stages else ())

    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        """mel [num_mels, T] -> d-vector [emb_dim] (the notebook's forward)."""
        _call.dev_check(mel, "mel")
        if mel.dim() != 2 or mel.shape[0] != self.num_mels:
            raise ValueError(f"mel: expected [{self.num_mels}, T], got {tuple(mel.shape)}")
        if mel.shape[1] < self.window:
            raise ValueError(f"mel has {mel.shape[1]} frames, fewer than one window of {self.window}")
        return self.embed_many([mel])[0][0]


# ---- the notebook's preprocessing loop -------------------------------------------------------------------------------------
REF_WAV_SUFFIX = "-ref_emb.wav"
EMB_SUFFIX = "-emb.pt"


def emb_path(ref_file: str) -> str:
    """``X-ref_emb.wav`` -> ``X-emb.pt`` (notebook :151)."""
    return ref_file.replace(REF_WAV_SUFFIX, "") + EMB_SUFFIX


def mels_to_files(encoder, mels: Sequence[torch.Tensor], out_paths: Sequence[str]) -> int:
    """One batch: embed, write a 1-D float tensor per item, or the reference's ``[0]`` marker (notebook :147-152) for a clip too
    short for one window (``evaluate.eval_batches`` and ``BatchFeeder`` drop such items).  Returns the number of real embeddings."""
    dvec, valid = encoder.embed_many(list(mels))[:2]
    dvec = dvec.cpu()
    good = 0
    for row, ok, path in zip(dvec, valid.tolist(), out_paths):
        torch.save(row.clone().reshape(-1) if ok else torch.zeros(1, dtype=torch.int64), path)
        good += int(ok)
    return good


def embed_directory(encoder, data_dir: str, audio_cfg, batch: int = 64, device="cuda:0", root: str = "..",
                    load_wav=None, mel_fn=None) -> int:
    """For every ``*-ref_emb.wav`` of data_dir (a TEXT file naming the reference utterance, notebook :141-143, relative to
    ``root``): read the utterance, log-mel, embed in batches of ``batch`` utterances, write ``*-emb.pt`` beside it."""
    if load_wav is None:
        from .trainer import load_wav
    mel_fn = mel_fn or (lambda w: logmel(w, audio_cfg, encoder.num_mels))
    files = sorted(glob.glob(os.path.join(data_dir, "*" + REF_WAV_SUFFIX)))
    sr = int(audio_cfg.get("sample_rate", 16000))
    audio_cfg = resolve_audio(audio_cfg)
    min_len = int(audio_cfg["n_fft"]) // 2
    good = 0
    for i in range(0, len(files), batch):
        mels, outs = [], []
        for f in files[i:i + batch]:
            with open(f, "r") as fh:
                wav_path = fh.readline().strip()
            wav = load_wav(os.path.join(root, wav_path), sr)
            if wav.numel() <= min_len:                       # shorter than the STFT's reflect padding: no mel, so no window either
                torch.save(torch.zeros(1, dtype=torch.int64), emb_path(f))
                continue
            mels.append(mel_fn(wav.to(device)))
            outs.append(emb_path(f))
        if mels:
            good += mels_to_files(encoder, mels, outs)
    return good


def resampling_loader(device="cuda:0", resample: bool = True, normalize: Optional[float] = None):
    """A ``load_wav(path, sample_rate)`` for ``embed_directory`` that accepts a file at any rate and converts it on the device
    (``librosa.load(path, sr=sample_rate)``); one ``resample.Resampler`` per source rate.  resample=False: a file at another rate is
    an error, as with ``trainer.load_wav``.  normalize: None, or the target in LUFS the clip is brought to on the device
    (``loudness.normalize``: one linear gain with a peak cap) behind the conversion."""
    from .resample import Resampler
    from .trainer import load_wav as load_at_rate, load_wav_native
    resamplers = {}

    def load(path, sample_rate):
        if not resample:
            wav = load_at_rate(path, sample_rate)
        else:
            wav, native = load_wav_native(path)
            if native != sample_rate:
                if native not in resamplers:
                    resamplers[native] = Resampler(native, sample_rate, device)
                wav = resamplers[native](wav.to(device))
        if normalize is not None and wav.numel():
            from .loudness import normalize as to_level
            wav = to_level(wav.to(device), sample_rate, float(normalize))
        return wav
    return load


def main(argv=None):
    from .config import default_config, load_config
    ap = argparse.ArgumentParser(description="Write the *-emb.pt speaker embeddings of a data directory")
    ap.add_argument("--checkpoint", required=True, help="embedder.pt: the state_dict of the GE2E speaker encoder")
    ap.add_argument("-d", "--data-dir", required=True, action="append", help="directory with *-ref_emb.wav (repeatable)")
    ap.add_argument("--config", default=None, help="config.json (audio settings); default: the reference's")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--root", default="..", help="directory the paths inside *-ref_emb.wav are relative to")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--resample", action="store_true", help="convert reference clips at another rate to the configured one on the device")
    ap.add_argument("--normalize", nargs="?", type=float, const=-23.0, default=None, metavar="LUFS",
                    help="bring every reference clip to this BS.1770 integrated loudness on the device first (default target -23; one "
                    "linear gain with a -2 dB peak cap, not ffmpeg's dynamic loudnorm)")
    args = ap.parse_args(argv)
    c = load_config(args.config) if args.config else default_config()
    audio_cfg = resolve_audio(c.audio)
    enc = SpeakerEncoder(num_mels=int(audio_cfg.get("num_mels", 40)))
    enc.load_state_dict(torch.load(args.checkpoint, map_location="cpu"), strict=True)
    enc = enc.eval().to(args.device)
    loader = resampling_loader(args.device, args.resample, args.normalize) if args.resample or args.normalize is not None else None
    for d in args.data_dir:
        n = embed_directory(enc, d, audio_cfg, batch=args.batch, device=args.device, root=args.root, load_wav=loader)
        print(f"{d}: {n} embeddings written")


if __name__ == "__main__":
    main()
