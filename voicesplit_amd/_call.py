"""How a call crosses into libvoicesplit_hip.so: the device guard, the stream, the pointer conversion, the error check and the
caller-owned scratch the library is handed.  ``_lib`` declares the C ABI; the wrappers (``ops``, ``losses``, ``audio``, ...) validate
their arguments and call through here.  A test that fakes the library patches this module: ``_lib.load``, ``dev_check``, ``stream``
and ``_SCRATCH``.
"""
import ctypes
from typing import Dict, Optional, Tuple

import torch

from . import _lib

# The scratch slots: one grow-only buffer per (slot, device).  Calls that share a slot run on one stream, one after the other.
SLOTS = (
    "model",    # vs_workspace_bytes: the eval forward and its stages (ops.get_workspace)
    "multi",    # vs_multi_workspace_bytes: the K-speaker forward and stages (ops.get_multi_workspace)
    "loss",     # vs_sisnr_workspace_bytes
    "audio",    # vs_audio_workspace_bytes / vs_griffin_lim_workspace_bytes: STFT, iSTFT, Griffin-Lim
    "deemph",   # vs_deemphasis_workspace_bytes
    "metric",   # vs_sdr_workspace_bytes / vs_bss_eval_workspace_bytes
    "logmel",   # vs_logmel_workspace_bytes
    "embed",    # vs_speaker_workspace_bytes
)
_SCRATCH: Dict[Tuple[str, Optional[int]], torch.Tensor] = {}


def dev_check(t: torch.Tensor, name: str, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise _lib.VoiceSplitHipError(
            f"{name} is on {t.device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


def ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Built:
    """The order between the stream that built device data and the streams that read it later.  An object that fills a device buffer
    once and keeps it past the call (a resampler's tap bank, prepared weights, a pool of room responses) makes one of these right
    behind the launches that fill the buffer -- it records an event on the building stream -- and calls ``wait()`` in front of every
    use: the stream current at that moment waits for the event on the device; the host never blocks.  Once the event has completed
    it is dropped, and ``wait()`` costs one attribute test from then on."""
    __slots__ = ("_event", "_device")

    def __init__(self, device):
        self._device = torch.device(device)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(self._device))

    def wait(self):
        ev = self._event
        if ev is None:
            return
        if ev.query():
            self._event = None
        else:
            torch.cuda.current_stream(self._device).wait_event(ev)


def call(name: str, device, *args, what: Optional[str] = None):
    """``vs_<name>(*args, stream)`` with ``device`` current, on that device's current stream; tensors go down as their data pointer,
    None as NULL, everything else as it is.  Raises VoiceSplitHipError (labelled ``what``, default the symbol) on a non-zero rc."""
    fn = getattr(_lib.load(), "vs_" + name)
    args = [ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(device):
        rc = fn(*args, stream())
    if rc:
        _lib.check(rc, what or "vs_" + name)


def sized(name: str, *args, what: Optional[str] = None) -> int:
    """``vs_<name>(*args)`` of a size_t-returning sizer; 0 is its refusal (the reason is in vs_last_error)."""
    n = getattr(_lib.load(), "vs_" + name)(*args)
    if not n:
        _lib.check(-1, what or "vs_" + name)
    return n


def scratch(slot: str, nbytes: int, device) -> torch.Tensor:
    """The uint8 buffer of ``slot`` on ``device``, at least ``nbytes`` long: the held one if it is large enough, else a new one (the
    old one is dropped first, so the two never coexist)."""
    if slot not in SLOTS:
        raise KeyError(f"scratch slot {slot!r} is not one of {SLOTS}")
    key = (slot, torch.device(device).index)
    ws = _SCRATCH.get(key)
    if ws is None or ws.numel() < nbytes:
        _SCRATCH.pop(key, None)
        del ws
        ws = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def scratch_bytes(device=None) -> int:
    idx = None if device is None else torch.device(device).index
    return sum(t.numel() for (_, d), t in _SCRATCH.items() if idx is None or d == idx)


def release_scratch():
    _SCRATCH.clear()
