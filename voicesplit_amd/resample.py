"""Sample-rate conversion on the device (csrc/resample.hip): what ``librosa.load(path, sr=sample_rate)`` does on the CPU in
``mix_wavfiles`` and in both audio processors' ``load_wav``.  The definition -- a Kaiser-windowed sinc with resampy's ``kaiser_best``
constants as remembered, restated and not compared with a resampy or librosa run -- is the text in include/voicesplit_hip.h.

    Resampler(sr_in, sr_out, device)            a whole waveform [n] or batch [B, n]; ``clips`` for waveforms of unequal length
    StreamingResampler(sr_in, sr_out, device)   ``push`` chunks of any size, ``finish``: bit-identical to the one call on the whole stream

The plan (L, M, H, T) is host arithmetic inside the library (``vs_resample_plan``) and needs no device; everything else has no CPU
fallback.
"""
import ctypes
from typing import Callable, List, Optional, Sequence

import torch

from . import _call, _lib


def plan(sr_in: int, sr_out: int) -> _lib.VsResampleDims:
    """``vs_resample_plan``: L, M, H, T, bank_bytes (and the launch's tile) for a pair of integer rates; raises for refused pairs."""
    for name, v in (("sr_in", sr_in), ("sr_out", sr_out)):
        if int(v) != v:
            raise ValueError(f"{name}={v!r}: rates are integers")
    d = _lib.VsResampleDims()
    _lib.check(_lib.load().vs_resample_plan(int(sr_in), int(sr_out), ctypes.byref(d)), "vs_resample_plan")
    return d


def out_len(d: _lib.VsResampleDims, n_in: int) -> int:
    """ceil(n_in L / M)."""
    n = _lib.load().vs_resample_out_len(ctypes.byref(d), int(n_in))
    if n < 0:
        _lib.check(-1, "vs_resample_out_len")
    return int(n)


def ready_outputs(d: _lib.VsResampleDims, received: int) -> int:
    """How many outputs of a stream are final once ``received`` samples are known: output n reads up to sample
    floor(n M / L) + H, so n is final when n M < (received - H) L."""
    have = int(received) - d.H
    return -(-(have * d.L) // d.M) if have > 0 else 0


def first_needed(d: _lib.VsResampleDims, n: int) -> int:
    """The first stream sample output n reads (not below 0)."""
    return max(0, (int(n) * d.M) // d.L - d.H)


class Resampler:
    """One pair of rates on one device: the polyphase bank (built once by ``vs_resample_bank``) and the calls that use it.  The bank
    is filled on the stream current at construction; every call that reads it makes its own stream wait for that on the device
    (``_call.Built``), so an instance may be built under one stream and used under any other."""

    def __init__(self, sr_in: int, sr_out: int, device="cuda:0"):
        self.dims = plan(sr_in, sr_out)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VoiceSplitHipError(f"Resampler on {self.device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.bank = torch.empty(self.dims.L * self.dims.T, dtype=torch.float32, device=self.device)
        _call.call("resample_bank", self.device, ctypes.byref(self.dims), self.bank)
        self._built = _call.Built(self.device)

    def out_len(self, n_in: int) -> int:
        return out_len(self.dims, n_in)

    def _rows(self, t: torch.Tensor, name: str):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError(f"{name}: expected a float32 [B, n] tensor")
        if t.device != self.device:
            raise _lib.VoiceSplitHipError(f"{name} is on {t.device}, the resampler on {self.device}: there is no CPU fallback")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{name}: the samples of a row must be contiguous (the rows may be strided)")
        return t

    def window(self, buf: torch.Tensor, x_first: int, stream_len: int, y_first: int, y_count: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``vs_resample``: outputs [y_first, y_first + y_count) of the B streams of which ``buf`` [B, k] holds samples
        [x_first, x_first + k); ``stream_len`` -1 while the end is unknown.  ``out`` [B, y_count] may be a strided view."""
        buf = self._rows(buf, "buf")
        B = buf.shape[0]
        if out is None:
            out = torch.empty(B, int(y_count), dtype=torch.float32, device=self.device)
        out = self._rows(out, "out")
        if out.shape != (B, int(y_count)):
            raise ValueError(f"out: expected [{B}, {y_count}], got {tuple(out.shape)}")
        self._built.wait()
        _call.call("resample", self.device, ctypes.byref(self.dims), self.bank, buf, int(x_first), buf.shape[1], buf.stride(0),
                   int(stream_len), out, int(y_first), int(y_count), out.stride(0), B)
        return out

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [n] or [B, n] -> [ceil(n L / M)] or [B, ceil(n L / M)]."""
        if wav.dim() == 1:
            return self(wav[None])[0]
        n = wav.shape[1]
        return self.window(wav, 0, n, 0, self.out_len(n))

    def clips_into(self, flat_in: torch.Tensor, out: torch.Tensor, table: torch.Tensor) -> None:
        """``vs_resample_clips``: table [N, 3] int64 on the host = (first input sample in ``flat_in``, samples, first output sample
        in ``out``) per clip; both buffers 1-D float32 on the device."""
        for name, t in (("flat_in", flat_in), ("out", out)):
            if t.dim() != 1 or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous 1-D float32 tensor on {self.device}")
        if table.dim() != 2 or table.shape[1] != 3 or table.dtype != torch.int64 or table.is_cuda:
            raise ValueError("table: expected [N, 3] int64 on the host")
        table = table.contiguous()
        table_dev = table.to(self.device)
        self._built.wait()
        _call.call("resample_clips", self.device, ctypes.byref(self.dims), self.bank, flat_in, flat_in.numel(), out, out.numel(),
                   table, table_dev, table.shape[0])

    def clips(self, wavs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """1-D waveforms of unequal length (host or device) -> their resampled versions, views into one flat device buffer, from
        one launch sequence."""
        if len(wavs) == 0:
            return []
        for k, w in enumerate(wavs):
            if w.dim() != 1 or w.dtype != torch.float32:
                raise ValueError(f"clip {k}: expected a 1-D float32 waveform, got {tuple(w.shape)} {w.dtype}")
        n_in = torch.tensor([w.numel() for w in wavs], dtype=torch.int64)
        n_out = torch.tensor([self.out_len(int(n)) for n in n_in], dtype=torch.int64)
        table = torch.stack((n_in.cumsum(0) - n_in, n_in, n_out.cumsum(0) - n_out), dim=1)
        flat = torch.empty(max(1, int(n_in.sum())), dtype=torch.float32, device=self.device)
        for o, w in zip(table[:, 0].tolist(), wavs):
            flat[o:o + w.numel()].copy_(w)
        out = torch.empty(max(1, int(n_out.sum())), dtype=torch.float32, device=self.device)
        self.clips_into(flat, out, table)
        return [out[o:o + n] for o, n in zip(table[:, 2].tolist(), n_out.tolist())]


class StreamingResampler:
    """A live stream through ``vs_resample``: ``push(samples [B, k])`` returns every output whose last input has arrived
    ([B, m], m >= 0), ``finish()`` the rest, up to ceil(n_in L / M) in all.  The state is the stream position and the last samples
    still needed, kept as a tensor; the kernel is stateless and its results do not depend on the window asked for, so the
    concatenation is bit-identical to ``Resampler`` on the whole stream for any chunking.

    compute(buf, x_first, stream_len, y_first, y_count) -> [B, y_count] replaces ``Resampler.window`` (the bookkeeping can then be
    exercised without a device); by default a ``Resampler`` (or the one passed as ``resampler``) does it."""

    def __init__(self, sr_in: int, sr_out: int, device="cuda:0", compute: Optional[Callable] = None, resampler: Optional[Resampler] = None):
        if compute is None:
            resampler = resampler or Resampler(sr_in, sr_out, device)
            if (resampler.sr_in, resampler.sr_out) != (int(sr_in), int(sr_out)):
                raise ValueError(f"the resampler given converts {resampler.sr_in} -> {resampler.sr_out}, not {sr_in} -> {sr_out}")
            compute = resampler.window
            self.dims = resampler.dims
        else:
            self.dims = plan(sr_in, sr_out)
        self._compute = compute
        self.received = 0                        # stream samples pushed so far
        self.emitted = 0                         # outputs returned so far
        self._tail, self._first = None, 0        # stream samples [_first, received)
        self.finished = False

    @property
    def latency_inputs(self) -> int:
        """An output leaves once the H samples behind its centre have been pushed."""
        return self.dims.H

    def _emit(self, upto: int, stream_len: int) -> torch.Tensor:
        count = upto - self.emitted
        if count <= 0:
            return self._tail.new_empty(self._tail.shape[0], 0)
        out = self._compute(self._tail, self._first, stream_len, self.emitted, count)
        self.emitted = upto
        keep = first_needed(self.dims, upto)
        if keep > self._first:
            self._tail, self._first = self._tail[:, keep - self._first:], keep
        return out

    def push(self, samples: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingResampler: the stream has been finished")
        if samples.dim() != 2:
            raise ValueError(f"samples must be [B, k], got {tuple(samples.shape)}")
        if self._tail is not None and samples.shape[0] != self._tail.shape[0]:
            raise ValueError(f"samples has {samples.shape[0]} rows, the stream {self._tail.shape[0]}")
        self._tail = samples if self._tail is None else torch.cat((self._tail, samples), dim=1)
        self.received += samples.shape[1]
        return self._emit(ready_outputs(self.dims, self.received), -1)

    def finish(self) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingResampler: the stream has been finished")
        if self._tail is None:
            raise RuntimeError("StreamingResampler: finish() on a stream that never received a sample")
        self.finished = True
        return self._emit(out_len(self.dims, self.received), self.received)
