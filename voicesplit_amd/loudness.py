"""Programme loudness on the device (csrc/loudness.hip): the ``ffmpeg-normalize <file> -ar 16000`` of the reference's
``scripts/normalise-resample.sh`` without the outside tool.  The measure is ITU-R BS.1770-4 integrated loudness of a mono clip
(K-weighting, 400 ms blocks at 75 % overlap, an absolute and a relative gate); the contract is the text in
include/voicesplit_hip.h.  Its constants are libebur128's as remembered: restated, NOT compared with an ffmpeg or libebur128 run.

    LoudnessMeter(sample_rate, device)      ``clips(flat, table)`` -> (lufs, peak, counts, valid) on the device
    integrated_loudness(wav, sample_rate)   fp64 LUFS of a waveform [n], a batch [B, n] or a list of waveforms
    gains(lufs, peak, valid, ...)           the linear gain to a target loudness under a peak cap, torch arithmetic, no read-back
    normalize(wav, sample_rate, ...)        a new tensor at the target; normalize_clips_(flat, table, ...) in place on a pool

The normalisation is ONE LINEAR GAIN per clip with a peak cap.  It is NOT ffmpeg's ``loudnorm`` in its dynamic mode, and nobody
has compared the two.  The defaults -23 LUFS / -2 dB are ``ffmpeg-normalize``'s as remembered.

``python -m voicesplit_amd.loudness --root ROOT`` writes ``<name>-norm.wav`` beside every ``<name>.wav`` under ROOT, which is what
every corpus hook of this package reads (``read_triplet_csv(librispeech=True)``).  There is no FLAC decoder here.

The plan (coefficients, sub-block length, the zero-input step) is host arithmetic inside the library and needs no device;
everything else has no CPU fallback.
"""
import argparse
import ctypes
import os
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _call, _lib

TARGET_LUFS, PEAK_DB = -23.0, -2.0
TRUE_PEAK_GROUP_BYTES = 256 << 20       # the 4x oversampled temporary of normalize(true_peak=True), per group of clips

_PLANS = {}


def plan(sample_rate: int) -> _lib.VsLoudnessDims:
    """``vs_loudness_plan``, cached per rate; raises for a rate outside 8000 .. 192000."""
    if int(sample_rate) != sample_rate:
        raise ValueError(f"sample_rate={sample_rate!r}: rates are integers")
    sr = int(sample_rate)
    if sr not in _PLANS:
        d = _lib.VsLoudnessDims()
        _lib.check(_lib.load().vs_loudness_plan(sr, ctypes.byref(d)), "vs_loudness_plan")
        _PLANS[sr] = d
    return _PLANS[sr]


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.VoiceSplitHipError(f"loudness on {device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _table(table: torch.Tensor) -> torch.Tensor:
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != 2 or table.dtype != torch.int64 or table.is_cuda:
        raise ValueError("table: expected [N, 2] int64 on the host = (first sample, samples) per clip")
    if table.shape[0] == 0:
        raise ValueError("table: no clips")
    return table.contiguous()


def _flat(flat: torch.Tensor, device: torch.device) -> torch.Tensor:
    if not isinstance(flat, torch.Tensor) or flat.dim() != 1 or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("flat: expected a contiguous 1-D float32 tensor")
    if flat.device != device:
        raise _lib.VoiceSplitHipError(f"flat is on {flat.device}, the meter on {device}: there is no CPU fallback")
    return flat


class LoudnessMeter:
    """One sample rate on one device."""

    def __init__(self, sample_rate: int, device="cuda:0"):
        self.dims = plan(sample_rate)
        self.sample_rate = int(sample_rate)
        self.device = _device(device)

    @property
    def sub(self) -> int:
        """S: samples per 100 ms sub-block."""
        return self.dims.sub

    def clips(self, flat: torch.Tensor, table: torch.Tensor, energy: bool = False):
        """``vs_loudness``: (lufs [N] fp64, peak [N] fp32, counts [N, 3] int32, valid [N] int32) on the device for the clips
        ``table`` [N, 2] int64 on the host = (first sample in ``flat``, samples).  energy=True: a fifth value, the list of every
        clip's sub-block energies e_k (fp64 views of one device buffer)."""
        flat, table = _flat(flat, self.device), _table(table)
        N, dev = table.shape[0], self.device
        if int(table[:, 1].min()) < 0:
            raise ValueError("table: a clip has a negative length")
        m = table[:, 1] // self.dims.sub
        laid_out = int(m.sum()) * self.dims.sub                       # sized as if the clips lay end to end (they may overlap)
        nbytes = _call.sized("loudness_workspace_bytes", ctypes.byref(self.dims), max(laid_out, flat.numel()), N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lufs = torch.empty(N, dtype=torch.float64, device=dev)
        peak = torch.empty(N, dtype=torch.float32, device=dev)
        counts = torch.empty(N, 3, dtype=torch.int32, device=dev)
        valid = torch.empty(N, dtype=torch.int32, device=dev)
        e = e_at = e_at_dev = None
        if energy:
            e_at = m.cumsum(0) - m
            e = torch.empty(max(1, int(m.sum())), dtype=torch.float64, device=dev)
            e_at_dev = e_at.to(dev)
        table_dev = table.to(dev)
        _call.call("loudness", dev, ctypes.byref(self.dims), flat, flat.numel(), table, table_dev, N, lufs, peak, counts, valid,
                   e, e_at_dev, ws, ws.numel())
        if energy:
            return lufs, peak, counts, valid, [e[o:o + k] for o, k in zip(e_at.tolist(), m.tolist())]
        return lufs, peak, counts, valid

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [n] or [B, n] on the device -> fp64 LUFS, a scalar tensor or [B]."""
        if wav.dim() == 1:
            return self(wav[None])[0]
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError(f"wav: expected float32 [n] or [B, n], got {tuple(wav.shape)} {wav.dtype}")
        flat, table = _rows_table(wav.contiguous())
        return self.clips(flat, table)[0]


def _rows_table(wav: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    B, n = wav.shape
    table = torch.stack((torch.arange(B, dtype=torch.int64) * n, torch.full((B,), n, dtype=torch.int64)), dim=1)
    return wav.reshape(-1), table


def _concat(wavs: Sequence[torch.Tensor], device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    for k, w in enumerate(wavs):
        if w.dim() != 1 or w.dtype != torch.float32:
            raise ValueError(f"clip {k}: expected a 1-D float32 waveform, got {tuple(w.shape)} {w.dtype}")
    n = torch.tensor([w.numel() for w in wavs], dtype=torch.int64)
    table = torch.stack((n.cumsum(0) - n, n), dim=1)
    flat = torch.empty(max(1, int(n.sum())), dtype=torch.float32, device=device)
    for o, w in zip(table[:, 0].tolist(), wavs):
        flat[o:o + w.numel()].copy_(w)
    return flat, table


def integrated_loudness(wav: Union[torch.Tensor, Sequence[torch.Tensor]], sample_rate: int, device=None) -> torch.Tensor:
    """fp64 LUFS (-inf where BS.1770 defines none: shorter than 400 ms, or nothing above -70 LUFS): a scalar tensor for wav [n],
    [B] for a batch [B, n] or a list of 1-D waveforms of unequal length.  ``device``: where to measure when the input is on the
    host (default cuda:0)."""
    if isinstance(wav, torch.Tensor):
        dev = wav.device if wav.is_cuda else torch.device(device or "cuda:0")
        return LoudnessMeter(sample_rate, dev)(wav.to(dev))
    if len(wav) == 0:
        raise ValueError("integrated_loudness: no clips")
    dev = torch.device(device) if device is not None else next((w.device for w in wav if w.is_cuda), torch.device("cuda:0"))
    meter = LoudnessMeter(sample_rate, dev)
    flat, table = _concat(wav, meter.device)
    return meter.clips(flat, table)[0]


def gains(lufs: torch.Tensor, peak: torch.Tensor, valid: torch.Tensor, target: float = TARGET_LUFS,
          peak_db: Optional[float] = PEAK_DB) -> torch.Tensor:
    """[N] fp32 on the inputs' device, computed in fp64 without a host round trip:
    g = min(10^((target - lufs) / 20), 10^(peak_db / 20) / peak); g = 1 where valid == 0 or peak == 0.  peak_db=None: no cap."""
    lufs64, peak64 = lufs.to(torch.float64), peak.to(torch.float64)
    off = (valid == 0) | (peak64 == 0)
    g = torch.pow(10.0, (float(target) - torch.where(off, torch.full_like(lufs64, float(target)), lufs64)) / 20.0)
    if peak_db is not None:
        cap = 10.0 ** (float(peak_db) / 20.0) / torch.where(off, torch.ones_like(peak64), peak64)
        g = torch.minimum(g, cap)
    return torch.where(off, torch.ones_like(g), g).to(torch.float32)


def scale_clips_(flat: torch.Tensor, table: torch.Tensor, gain: torch.Tensor) -> None:
    """``vs_scale_clips``: flat[at : at + n] *= gain[i] for every clip of ``table`` [N, 2] (host), in place; gain [N] fp32 on the
    device.  Nothing outside the clips is touched."""
    dev = _device(flat.device)
    flat, table = _flat(flat, dev), _table(table)
    N = table.shape[0]
    if gain.shape != (N,) or gain.dtype != torch.float32 or gain.device != dev or not gain.is_contiguous():
        raise ValueError(f"gain: expected a contiguous float32 [{N}] tensor on {dev}")
    table_dev = table.to(dev)
    _call.call("scale_clips", dev, flat, flat.numel(), table, table_dev, gain, N)


def true_peaks(flat: torch.Tensor, table: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """[N] fp32 on the device: max |y| of every clip converted to 4 x ``sample_rate`` (``Resampler.clips_into`` into a temporary of
    at most TRUE_PEAK_GROUP_BYTES per group of clips, then ``vs_clip_range``).  No new kernel: what exists, composed."""
    from .resample import Resampler
    dev = _device(flat.device)
    flat, table = _flat(flat, dev), _table(table)
    rs = Resampler(int(sample_rate), 4 * int(sample_rate), dev)
    N = table.shape[0]
    n_out = torch.tensor([rs.out_len(int(n)) for n in table[:, 1]], dtype=torch.int64)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    lo = 0
    while lo < N:
        hi, size = lo, 0
        while hi < N and (hi == lo or (size + int(n_out[hi])) * 4 <= TRUE_PEAK_GROUP_BYTES):
            size += int(n_out[hi])
            hi += 1
        k = n_out[lo:hi]
        offsets = torch.zeros(hi - lo + 1, dtype=torch.int64)
        offsets[1:] = k.cumsum(0)
        tmp = torch.empty(max(1, size), dtype=torch.float32, device=dev)
        rs.clips_into(flat, tmp, torch.cat((table[lo:hi], offsets[:-1, None]), dim=1))
        rng = torch.empty(hi - lo, 2, dtype=torch.float32, device=dev)
        offsets_dev = offsets.to(dev)
        _call.call("clip_range", dev, tmp, tmp.numel(), offsets, offsets_dev, None, hi - lo, rng)
        out[lo:hi] = rng.abs().max(dim=1).values
        lo = hi
    return out


def normalize_clips_(flat: torch.Tensor, table: torch.Tensor, sample_rate: int, target: float = TARGET_LUFS,
                     peak_db: Optional[float] = PEAK_DB, true_peak: bool = False):
    """The clips ``table`` [N, 2] (host) of ``flat`` brought to ``target`` LUFS under the peak cap, in place: ``vs_loudness``,
    ``gains``, ``vs_scale_clips``, nothing read back.  Returns (lufs [N] fp64, gain [N] fp32) on the device: the loudness BEFORE the
    gain and the gain applied.  Clips without a loudness (valid == 0) and all-zero clips keep gain 1."""
    meter = LoudnessMeter(sample_rate, flat.device)
    lufs, peak, _, valid = meter.clips(flat, table)
    if true_peak and peak_db is not None:
        peak = true_peaks(flat, table, sample_rate)
    g = gains(lufs, peak, valid, target, peak_db)
    scale_clips_(flat, table, g)
    return lufs, g


def normalize(wav: torch.Tensor, sample_rate: int, target: float = TARGET_LUFS, peak_db: Optional[float] = PEAK_DB,
              true_peak: bool = False) -> torch.Tensor:
    """wav [n] or [B, n] (device) -> a new tensor, every row at ``target`` LUFS or, where that would lift its peak above
    ``peak_db`` dBFS, at the cap.  One linear gain per row -- not ffmpeg's dynamic ``loudnorm``, and not compared with it.
    true_peak=True caps the peak of the row oversampled four times instead of its sample peak."""
    if wav.dim() == 1:
        return normalize(wav[None], sample_rate, target, peak_db, true_peak)[0]
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError(f"wav: expected float32 [n] or [B, n], got {tuple(wav.shape)} {wav.dtype}")
    _device(wav.device)
    out = wav.contiguous().clone()
    flat, table = _rows_table(out)
    normalize_clips_(flat, table, sample_rate, target, peak_db, true_peak)
    return out


# ---------------------------------------------------------------------------------------------
# python -m voicesplit_amd.loudness: the -norm.wav files of scripts/normalise-resample.sh
# ---------------------------------------------------------------------------------------------
def find_wavs(root: str, suffix: str) -> List[str]:
    """Every ``*.wav`` under ``root`` that is not itself an output (does not end in ``suffix``), sorted."""
    out = []
    for dirpath, _, files in os.walk(root):
        out += [os.path.join(dirpath, f) for f in files if f.lower().endswith(".wav") and not f.endswith(suffix)]
    return sorted(out)


def write_normalized(paths: Sequence[str], suffix: str = "-norm.wav", sample_rate: Optional[int] = None, device="cuda:0",
                     target: float = TARGET_LUFS, peak_db: Optional[float] = PEAK_DB, batch: int = 512) -> int:
    """``<name><suffix>`` beside every ``<name>.wav`` of ``paths``: read, converted to ``sample_rate`` on the device when it is
    given and the file has another rate, normalised, written as float32.  ``batch`` files per pool.  Returns the number written."""
    import numpy as np
    from scipy.io import wavfile
    from .mixing import ClipPool
    from .trainer import load_wav_native
    written = 0
    for lo in range(0, len(paths), batch):
        group = list(paths[lo:lo + batch])
        rates = [load_wav_native(p)[1] for p in group] if sample_rate is None else None
        for sr in sorted(set(rates)) if rates else [int(sample_rate)]:
            files = [p for k, p in enumerate(group) if rates is None or rates[k] == sr]
            pool = ClipPool.from_files(files, sr, device, resample=sample_rate is not None, trim=False, normalize=target, peak_db=peak_db)
            host = pool.flat.cpu()
            for k, p in enumerate(files):
                a, b = int(pool.offsets[k]), int(pool.offsets[k + 1])
                wavfile.write(p[:-len(".wav")] + suffix, sr, host[a:b].numpy().astype(np.float32))
                written += 1
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description="Write <name>-norm.wav beside every .wav under a corpus root: BS.1770 loudness "
                                 "normalisation (one linear gain with a peak cap; not ffmpeg's dynamic loudnorm) on the GPU")
    ap.add_argument("--root", required=True, help="the corpus; every *.wav below it is read (there is no FLAC decoder here)")
    ap.add_argument("--suffix", default="-norm.wav")
    ap.add_argument("--resample", action="store_true", help="convert every file to --sample-rate on the device first")
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--target", type=float, default=TARGET_LUFS, help="LUFS")
    ap.add_argument("--peak-db", type=float, default=PEAK_DB, help="dBFS cap of the sample peak")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    paths = find_wavs(args.root, args.suffix)
    n = write_normalized(paths, args.suffix, args.sample_rate if args.resample else None, args.device, args.target, args.peak_db)
    print(f"{n} files written with the suffix {args.suffix} under {args.root}")


if __name__ == "__main__":
    main()
