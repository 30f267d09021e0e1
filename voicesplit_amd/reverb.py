"""Reverberation on the device (csrc/reverb.hip): room impulse responses of shoebox rooms by the image method, the per-row FIR
that applies them, and the pool of responses the training mixtures draw from.  The contracts are the text in
include/voicesplit_hip.h.  The image method is restated (Allen & Berkley 1979), NOT compared with a pyroomacoustics or
rir-generator run.

    shoebox_rir(rooms)                h [R, H] fp32 on the device for the room table ``rooms`` (``vs_rir_shoebox``)
    fir_rows(flat, at, lo, nh, ..)    ``vs_fir_rows`` on a flat buffer: every row its own filter, history and start
    fir_spectra(h, nh)                ``vs_fir_spectra``: the kept spectra of a table of responses of up to 32768 taps (csrc/fir_fft.hip)
    fir_rows_fft(flat, at, lo, ..)    ``vs_fir_rows_fft``: the same rows by partitioned overlap-save FFT convolution in fp32
    apply(wav, h, hrow, nh, math)     wav [B, N] convolved row by row (zero history), same length
    row_energy(y)                     [B] fp64 sums of squares (``vs_row_energy``)
    draw_rooms(R, generator, ..)      host fp64: R random rooms, one receiver and TWO sources each -> a table of 2 R responses
    RirPool(R, ..)                    the responses of R drawn rooms resident on one device; ``redraw(epoch)`` makes a fresh pool;
                                      ``RirPool.from_responses`` / ``from_files``: measured responses instead of drawn rooms

A room table is a float64 tensor [R, 19] on the host, one response per row:
size (3) | source (3) | receiver (3) | beta x0 x1 y0 y1 z0 z1 (6) | c | fs | nh | max_order (-1 = no limit).
The draws are host arithmetic and need no device; everything else has no CPU fallback.
"""
import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _call, _lib

MAX_TAPS = 8192                         # the direct form (vs_fir_rows) and the image method (vs_rir_shoebox)
MAX_TAPS_FFT = 32768                    # the FFT form (vs_fir_rows_fft)
FFT_BLOCK = 2048                        # VS_FIR_FFT_BLOCK
ROOM_COLS = 19
SPEED_OF_SOUND = 343.0
EARLY_SECONDS = 0.05                    # target="early": the response is cut this far behind the direct path
MATH = {"fp32": _lib.MATH_FP32, "f16x3": _lib.MATH_F16X3}
_COL = {"size": 0, "src": 3, "mic": 6, "beta": 9, "c": 15, "fs": 16, "nh": 17, "max_order": 18}


def room_row(size, src, mic, beta, fs=16000.0, nh=4096, max_order=-1, c=SPEED_OF_SOUND) -> torch.Tensor:
    """One row of a room table.  beta: one number for all six walls, or (x0, x1, y0, y1, z0, z1)."""
    beta = [float(beta)] * 6 if isinstance(beta, (int, float)) else [float(v) for v in beta]
    if len(beta) != 6 or len(size) != 3 or len(src) != 3 or len(mic) != 3:
        raise ValueError("room_row: size, src and mic have three entries, beta one or six")
    return torch.tensor([*size, *src, *mic, *beta, c, fs, nh, max_order], dtype=torch.float64)


def _table(rooms: torch.Tensor) -> torch.Tensor:
    if not isinstance(rooms, torch.Tensor) or rooms.dim() != 2 or rooms.shape[1] != ROOM_COLS or rooms.dtype != torch.float64 \
            or rooms.is_cuda or rooms.shape[0] == 0:
        raise ValueError(f"rooms: expected a float64 [R, {ROOM_COLS}] table on the host with R > 0")
    return rooms


def room_structs(rooms: torch.Tensor):
    """The ``vs_room`` array of a room table (host memory)."""
    rooms = _table(rooms)
    arr = (_lib.VsRoom * rooms.shape[0])()
    for k, row in enumerate(rooms.tolist()):
        r = arr[k]
        r.size[:], r.src[:], r.mic[:], r.beta[:] = row[0:3], row[3:6], row[6:9], row[9:15]
        r.c, r.fs = row[15], row[16]
        if row[17] != int(row[17]) or row[18] != int(row[18]):
            raise ValueError(f"room {k}: nh and max_order are integers")
        r.nh, r.max_order = int(row[17]), int(row[18])
    return arr


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.VoiceSplitHipError(f"reverb on {device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def shoebox_rir(rooms: torch.Tensor, device="cuda:0", H: Optional[int] = None) -> torch.Tensor:
    """``vs_rir_shoebox``: h [R, H] fp32 on ``device``; row r holds the ``nh`` taps of room r, then zeros.  H defaults to the largest
    ``nh`` of the table."""
    arr = room_structs(rooms)
    device = _device(device)
    R = rooms.shape[0]
    H = int(rooms[:, _COL["nh"]].max()) if H is None else int(H)
    raw = torch.frombuffer(bytearray(ctypes.string_at(arr, ctypes.sizeof(arr))), dtype=torch.uint8).to(device)
    h = torch.empty(R, max(H, 1), dtype=torch.float32, device=device)
    _call.call("rir_shoebox", device, arr, raw, R, H, h)
    return h


def fir_rows(flat: torch.Tensor, at: torch.Tensor, lo: torch.Tensor, nh: torch.Tensor, hrow: torch.Tensor, h: torch.Tensor, L: int,
             math: str = "f16x3", out: Optional[torch.Tensor] = None):
    """``vs_fir_rows``: (y [B, L], valid [B] int32, scale [B, 4]) with y[b][i] = sum_{k < nh[b]} h[hrow[b]][k] x(at[b] + i - k) and
    x(p) = flat[p] for p >= lo[b], else 0.  at, lo: [B] int64; nh, hrow: [B] int32; all on the device of ``flat``."""
    if math not in MATH:
        raise ValueError(f"math must be one of {sorted(MATH)}, got {math!r}")
    _call.dev_check(flat, "flat")
    _call.dev_check(h, "h")
    dev = flat.device
    if flat.dim() != 1 or h.dim() != 2:
        raise ValueError("flat is 1-D, h is [R, H]")
    B = at.numel()
    for name, t, dt in (("at", at, torch.int64), ("lo", lo, torch.int64), ("nh", nh, torch.int32), ("hrow", hrow, torch.int32)):
        if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.dim() != 1 or t.numel() != B:
            raise ValueError(f"{name}: expected a contiguous 1-D {dt} tensor of {B} entries on {dev}")
    if h.device != dev:
        raise ValueError(f"h is on {h.device}, the samples on {dev}")
    y = torch.empty(B, int(L), dtype=torch.float32, device=dev) if out is None else out
    if y.shape != (B, int(L)) or y.dtype != torch.float32 or not y.is_contiguous() or y.device != dev:
        raise ValueError(f"out: expected a contiguous float32 [{B}, {L}] tensor on {dev}")
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    scale = torch.empty(B, 4, dtype=torch.float32, device=dev)
    _call.call("fir_rows", dev, flat, flat.numel(), at, lo, nh, hrow, B, int(L), h, h.shape[0], h.shape[1], MATH[math], y, valid, scale)
    return y, valid, scale


class FirSpectra:
    """What ``fir_spectra`` made: ``blob`` (uint8 on the device: twiddle table, partition counts, spectra -- opaque), ``nh`` [R] int32
    on the device, ``nh_host`` its host copy, ``R`` and ``H``.  ``wait()`` orders the stream current at that moment behind the
    launches that filled the blob (``_call.Built``)."""
    __slots__ = ("blob", "nh", "nh_host", "R", "H", "device", "_built")

    def __init__(self, blob, nh, nh_host, R, H):
        self.blob, self.nh, self.nh_host, self.R, self.H, self.device = blob, nh, nh_host, R, H, blob.device
        self._built = _call.Built(blob.device)

    def wait(self):
        self._built.wait()


def fir_spectra(h: torch.Tensor, nh, nh_device: Optional[torch.Tensor] = None) -> FirSpectra:
    """``vs_fir_spectra``: the spectra of the responses h [R, H <= 32768] (fp32, on the device), response r cut at nh[r] taps
    (taps behind nh[r] count as zero whatever the row holds).  nh: R integers on the host (a device tensor is read back, which
    blocks).  nh_device: the same table as int32 on the device of ``h`` when the caller holds one; without it the table goes up
    from pageable host memory, which blocks the host until the current stream has drained.  Make the spectra once for a table
    that stays, and hand them to every ``fir_rows_fft`` call."""
    _call.dev_check(h, "h")
    if h.dim() != 2 or not 1 <= h.shape[1] <= MAX_TAPS_FFT or h.shape[0] == 0:
        raise ValueError(f"h: expected [R, H] with R > 0 and 1 <= H <= {MAX_TAPS_FFT}, got {tuple(h.shape)}")
    R, H = h.shape
    nh = torch.as_tensor(nh)
    if nh.dim() != 1 or nh.numel() != R or nh.dtype.is_floating_point:
        raise ValueError(f"nh: expected {R} integers, one per response")
    nh_host = nh.to("cpu", torch.int32).contiguous()
    if nh_device is None:
        nh_device = nh_host.to(h.device)
    elif nh_device.dtype != torch.int32 or nh_device.device != h.device or nh_device.shape != (R,) or not nh_device.is_contiguous():
        raise ValueError(f"nh_device: expected a contiguous int32 tensor of {R} entries on {h.device}")
    nbytes = _call.sized("fir_spectra_bytes", R, H)
    blob = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    _call.call("fir_spectra", h.device, h, nh_host, nh_device, R, H, blob, nbytes)
    return FirSpectra(blob, nh_device, nh_host, R, H)


def fir_rows_fft(flat: torch.Tensor, at: torch.Tensor, lo: torch.Tensor, hrow: torch.Tensor, spectra: FirSpectra, L: int,
                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``vs_fir_rows_fft``: (y [B, L], valid [B] int32), ``fir_rows``' y with nh = spectra.nh[hrow[b]], by partitioned overlap-save
    convolution in fp32.  workspace: None (made here) or a uint8 tensor of at least ``vs_fir_fft_workspace_bytes`` on the device;
    what it holds changes nothing."""
    if not isinstance(spectra, FirSpectra):
        raise TypeError("spectra: expected what fir_spectra returned")
    _call.dev_check(flat, "flat")
    dev = flat.device
    if flat.dim() != 1:
        raise ValueError("flat is 1-D")
    if spectra.device != dev:
        raise ValueError(f"the spectra are on {spectra.device}, the samples on {dev}")
    B = at.numel()
    for name, t, dt in (("at", at, torch.int64), ("lo", lo, torch.int64), ("hrow", hrow, torch.int32)):
        if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.dim() != 1 or t.numel() != B:
            raise ValueError(f"{name}: expected a contiguous 1-D {dt} tensor of {B} entries on {dev}")
    y = torch.empty(B, int(L), dtype=torch.float32, device=dev) if out is None else out
    if y.shape != (B, int(L)) or y.dtype != torch.float32 or not y.is_contiguous() or y.device != dev:
        raise ValueError(f"out: expected a contiguous float32 [{B}, {L}] tensor on {dev}")
    need = _call.sized("fir_fft_workspace_bytes", B, int(L), spectra.H)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if workspace is None else workspace
    if ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"workspace: expected a contiguous uint8 tensor of at least {need} bytes on {dev}")
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    spectra.wait()
    _call.call("fir_rows_fft", dev, flat, flat.numel(), at, lo, hrow, B, int(L), spectra.blob, spectra.blob.numel(), spectra.R, spectra.H,
               ws, ws.numel(), y, valid)
    return y, valid


def apply(wav: torch.Tensor, h: torch.Tensor, hrow: Optional[torch.Tensor] = None, nh: Optional[torch.Tensor] = None,
          math: str = "f16x3") -> torch.Tensor:
    """wav [B, N] convolved with one response per row, truncated to N samples (silence in front of every row).  h [R, H]; hrow [B]
    picks each row's response (default: row b takes h[b], so R must be B), nh [B] its number of taps (default: all H).
    math="fft": the FFT form (H up to 32768); its spectra are made on the fly, so nh is then one entry per RESPONSE, [R]."""
    if wav.dim() != 2 or h.dim() != 2:
        raise ValueError(f"wav: expected [B, N], h [R, H]; got {tuple(wav.shape)} and {tuple(h.shape)}")
    _call.dev_check(wav, "wav")
    B, N = wav.shape
    dev = wav.device
    if hrow is None:
        if h.shape[0] != B:
            raise ValueError(f"h has {h.shape[0]} responses for {B} rows: pass hrow")
        hrow = torch.arange(B, dtype=torch.int32, device=dev)
    if nh is None and math != "fft":
        nh = torch.full((B,), h.shape[1], dtype=torch.int32, device=dev)
    at = torch.arange(B, dtype=torch.int64, device=dev) * N
    if math == "fft":
        _call.dev_check(h, "h")
        table = torch.full((h.shape[0],), h.shape[1], dtype=torch.int32) if nh is None else nh
        y, _ = fir_rows_fft(wav.reshape(-1), at, at, hrow.to(dev, torch.int32).contiguous(), fir_spectra(h, table), N)
        return y
    y, _, _ = fir_rows(wav.reshape(-1), at, at, nh.to(dev, torch.int32).contiguous(), hrow.to(dev, torch.int32).contiguous(), h, N, math)
    return y


def row_energy(y: torch.Tensor) -> torch.Tensor:
    """``vs_row_energy``: [B] fp64, the sum of squares of every row of y [B, L]."""
    _call.dev_check(y, "y")
    if y.dim() != 2 or y.shape[1] == 0:
        raise ValueError(f"y: expected [B, L], got {tuple(y.shape)}")
    e = torch.empty(y.shape[0], dtype=torch.float64, device=y.device)
    _call.call("row_energy", y.device, y, y.shape[0], y.shape[1], e)
    return e


# ---------------------------------------------------------------------------------------------
# random rooms (host)
# ---------------------------------------------------------------------------------------------
DRAWS_PER_ROOM = 13                     # size 3, rt60 1, receiver 3, per source: azimuth, cos(elevation), distance


def sabine_beta(size: Sequence[float], rt60: float) -> float:
    """The uniform reflection coefficient of a room with this reverberation time: Sabine's alpha = 0.161 V / (S rt60), clamped to
    0.01 .. 0.99, beta = sqrt(1 - alpha)."""
    lx, ly, lz = (float(v) for v in size)
    V, S = lx * ly * lz, 2.0 * (lx * ly + ly * lz + lx * lz)
    alpha = min(0.99, max(0.01, 0.161 * V / (S * float(rt60))))
    return math.sqrt(1.0 - alpha)


def draw_rooms(R: int, generator: torch.Generator, size=((3.0, 3.0, 2.4), (8.0, 6.0, 3.5)), rt60=(0.15, 0.5), distance=(0.5, 3.0),
               margin: float = 0.5, fs: int = 16000, nh: Optional[int] = None, c: float = SPEED_OF_SOUND, max_order: int = -1,
               max_taps: int = MAX_TAPS):
    """R random rooms from ``generator`` (ONE block of R x 13 uniform fp64 draws, then plain arithmetic): the table [2 R, 19] -- rows
    2 r and 2 r + 1 are the target and the interferer source of room r, heard at the same receiver -- and the reverberation times [R].
    Per room: the size uniform in the box ``size``, rt60 uniform in ``rt60``, the receiver uniform in the room at least ``margin``
    from every wall; each source on a uniformly drawn line through the receiver, on the side with more room, at a
    distance uniform in ``distance``, shortened to 0.95 of what that side allows inside the margins.  All walls share Sabine's beta (``sabine_beta``).  nh: taps per response, default
    min(max_taps, ceil(rt60 fs)) of each room.  max_taps (at most 8192, what the image method is built for) says where a response
    that rings longer than that is CUT: the default cuts at 0.51 s at 16 kHz, whatever rt60 asks for."""
    if R <= 0:
        raise ValueError(f"draw_rooms: R={R}")
    lo3, hi3 = [float(v) for v in size[0]], [float(v) for v in size[1]]
    if any(l <= 2.0 * margin or h < l for l, h in zip(lo3, hi3)):
        raise ValueError(f"draw_rooms: every room size must exceed twice the margin {margin}, and size[0] <= size[1]")
    if not (0.0 < rt60[0] <= rt60[1]) or not (0.0 < distance[0] <= distance[1]):
        raise ValueError("draw_rooms: rt60 and distance are (low, high) with 0 < low <= high")
    if nh is not None and not (1 <= int(nh) <= MAX_TAPS):
        raise ValueError(f"draw_rooms: nh={nh} (1 .. {MAX_TAPS})")
    if not (1 <= int(max_taps) <= MAX_TAPS):
        raise ValueError(f"draw_rooms: max_taps={max_taps} (1 .. {MAX_TAPS}: longer image-method responses are not built)")
    U = torch.rand(R, DRAWS_PER_ROOM, dtype=torch.float64, generator=generator).tolist()
    rows, times = [], []
    for u in U:
        L = [lo3[d] + u[d] * (hi3[d] - lo3[d]) for d in range(3)]
        t60 = rt60[0] + u[3] * (rt60[1] - rt60[0])
        mic = [margin + u[4 + d] * (L[d] - 2.0 * margin) for d in range(3)]
        beta = sabine_beta(L, t60)
        taps = min(int(max_taps), int(math.ceil(t60 * fs))) if nh is None else int(nh)
        for s in range(2):
            az, ce, dist = 2.0 * math.pi * u[7 + 3 * s], 2.0 * u[8 + 3 * s] - 1.0, distance[0] + u[9 + 3 * s] * (distance[1] - distance[0])
            se = math.sqrt(max(0.0, 1.0 - ce * ce))
            direction = [se * math.cos(az), se * math.sin(az), ce]
            reach = [math.inf, math.inf]                                           # along the direction, and along its opposite
            for d in range(3):
                if direction[d] != 0.0:
                    up, down = (L[d] - margin - mic[d]) / abs(direction[d]), (mic[d] - margin) / abs(direction[d])
                    reach[0] = min(reach[0], up if direction[d] > 0.0 else down)
                    reach[1] = min(reach[1], down if direction[d] > 0.0 else up)
            if reach[1] > reach[0]:                                                # the side with more room
                direction, reach = [-v for v in direction], reach[::-1]
            dist = min(dist, 0.95 * reach[0])
            src = [mic[d] + dist * direction[d] for d in range(3)]
            rows.append(room_row(L, src, mic, beta, float(fs), taps, max_order, c))
        times.append(t60)
    return torch.stack(rows), torch.tensor(times, dtype=torch.float64)


def direct_delay(rooms: torch.Tensor) -> torch.Tensor:
    """[R] fp64: the direct path's delay |s - m| fs / c in samples."""
    rooms = _table(rooms)
    d = (rooms[:, 3:6] - rooms[:, 6:9]).pow(2).sum(dim=1).sqrt()
    return d * rooms[:, _COL["fs"]] / rooms[:, _COL["c"]]


def early_taps(rooms: torch.Tensor, seconds: float = EARLY_SECONDS) -> torch.Tensor:
    """[R] int32: the number of taps of the response cut ``seconds`` behind the direct path (at most nh)."""
    rooms = _table(rooms)
    n = torch.floor(direct_delay(rooms)) + 1 + torch.floor(rooms[:, _COL["fs"]] * seconds)
    return torch.minimum(n, rooms[:, _COL["nh"]]).to(torch.int32)


POOL_SALT = 0x5EB0_0001                 # the pool's rooms: crop_seed(seed, epoch, 0) ^ POOL_SALT
ITEM_SALT = 0x5EB0_0002                 # a batch's response and level draws: crop_seed(seed, epoch, rank) ^ ITEM_SALT


class RirPool:
    """The responses of R drawn rooms resident on one device: ``h`` [2 R, H] fp32, ``nh`` [2 R] int32 (device; ``nh_host`` on the
    host), ``nh_early`` the taps of the response cut 50 ms behind the direct path, ``rooms`` the table [2 R, 19] and ``rt60`` [R].
    Response 2 r is room r's target source, 2 r + 1 its interferer.  The rooms come from a generator of their own, seeded from
    (seed, epoch); ``redraw(epoch)`` makes a fresh pool with the same settings.  The device tensors are filled on the stream
    current at construction (and at ``redraw``); reading ``h``, ``nh`` or ``nh_early`` makes the stream current at that moment wait
    for that on the device (``_call.Built``), so a pool may be drawn under one stream and used under any other.
    ``spectra``: the ``FirSpectra`` of ``h`` for the FFT form, made at the first read, kept for the pool's life and ordered the same
    way; a redrawn pool is a new object and makes its own.  ``from_responses`` / ``from_files``: measured responses of up to 32768
    taps; such pools are fixed and never redrawn."""

    def __init__(self, R: int, device="cuda:0", seed: int = 0, epoch: int = 0, **draw):
        from .mixing import crop_seed
        self.R, self.seed, self.epoch, self.draw = int(R), int(seed), int(epoch), dict(draw)
        g = torch.Generator().manual_seed(crop_seed(self.seed, self.epoch, 0) ^ POOL_SALT)
        rooms, rt60 = draw_rooms(self.R, g, **draw)
        self._adopt(rooms, rt60, shoebox_rir(rooms, device))

    def _resident(self, h, nh, nh_early):
        self._h, self._nh, self._nh_early, self.device = h, nh, nh_early, h.device
        self._built = _call.Built(h.device)
        self._spectra = self._h_early = None

    @property
    def spectra(self) -> FirSpectra:
        if self._spectra is None:
            self._spectra = fir_spectra(self.h, self.nh_host, self.nh)
        return self._spectra

    @property
    def h_early(self) -> torch.Tensor:
        """The table the direct form reads for the early responses: ``h`` itself, or for rows longer than the direct form takes
        (measured responses) a copy cut behind the longest early response."""
        if self._h.shape[1] <= MAX_TAPS:
            return self.h
        if self._h_early is None:
            self._h_early = self.h[:, :int(self.nh_early_host.max())].contiguous()
            self._built = _call.Built(self.device)
        return self._ordered(self._h_early)

    def _ordered(self, t):
        self._built.wait()
        return t

    h = property(lambda self: self._ordered(self._h))
    nh = property(lambda self: self._ordered(self._nh))
    nh_early = property(lambda self: self._ordered(self._nh_early))

    def _adopt(self, rooms, rt60, h):
        self.rooms, self.rt60 = rooms, rt60
        self.nh_host = rooms[:, _COL["nh"]].to(torch.int32)
        self.nh_early_host = early_taps(rooms)
        self._resident(h, self.nh_host.to(h.device), self.nh_early_host.to(h.device))

    @classmethod
    def from_rooms(cls, rooms: torch.Tensor, device="cuda:0") -> "RirPool":
        """A pool of the given responses; rows 2 r and 2 r + 1 must be the two sources of room r."""
        if _table(rooms).shape[0] % 2:
            raise ValueError("from_rooms: two responses per room")
        self = cls.__new__(cls)
        self.R, self.seed, self.epoch, self.draw = rooms.shape[0] // 2, 0, 0, None
        self._adopt(rooms, None, shoebox_rir(rooms, device))
        return self

    @classmethod
    def impulses(cls, device="cuda:0") -> "RirPool":
        """One room whose two responses are the unit impulse h = {1}: the mixture without a room (what serves ``sir_db`` alone)."""
        self = cls.__new__(cls)
        self.R, self.seed, self.epoch, self.draw = 1, 0, 0, None
        self.rooms = self.rt60 = None
        self.nh_host = self.nh_early_host = torch.ones(2, dtype=torch.int32)
        nh = self.nh_host.to(_device(device))
        self._resident(torch.ones(2, 1, dtype=torch.float32, device=nh.device), nh, nh)
        return self

    @staticmethod
    def measured_early_taps(h: torch.Tensor, nh: torch.Tensor, fs: int = 16000, seconds: float = EARLY_SECONDS) -> torch.Tensor:
        """[R] int32: argmax |h| over the first nh taps (the direct path of a measured response) + 1 + floor(seconds fs), at most nh."""
        idx = torch.arange(h.shape[1])[None, :]
        peak = torch.where(idx < nh[:, None], h.abs().cpu(), torch.full((), -1.0)).argmax(dim=1)
        return torch.minimum(peak + 1 + int(math.floor(seconds * fs)), nh.to(torch.int64)).to(torch.int32)

    @classmethod
    def from_responses(cls, h: torch.Tensor, nh=None, fs: int = 16000, device="cuda:0") -> "RirPool":
        """A pool of measured responses h [2 R, H <= 32768] (fp32, host or device): rows 2 r and 2 r + 1 are the two sources of
        room r.  nh [2 R]: the taps of each (default H).  ``nh_early`` = argmax |h| + 1 + floor(0.05 fs), at most nh.  The direct
        form takes 8192 taps: longer pools go through ``math="fft"``."""
        if not isinstance(h, torch.Tensor) or h.dim() != 2 or h.dtype != torch.float32 or h.shape[0] == 0 or h.shape[0] % 2:
            raise ValueError("from_responses: h is float32 [2 R, H], two responses per room")
        if not 1 <= h.shape[1] <= MAX_TAPS_FFT:
            raise ValueError(f"from_responses: H={h.shape[1]} taps (1 .. {MAX_TAPS_FFT})")
        nh_host = torch.full((h.shape[0],), h.shape[1], dtype=torch.int32) if nh is None else torch.as_tensor(nh).to("cpu", torch.int32)
        if nh_host.shape != (h.shape[0],) or int(nh_host.min()) < 1 or int(nh_host.max()) > h.shape[1]:
            raise ValueError(f"from_responses: nh is {h.shape[0]} integers in 1 .. H = {h.shape[1]}")
        device = _device(device)
        self = cls.__new__(cls)
        self.R, self.seed, self.epoch, self.draw = h.shape[0] // 2, 0, 0, None
        self.rooms = self.rt60 = None
        self.nh_host, self.nh_early_host = nh_host, cls.measured_early_taps(h, nh_host, fs)
        self._resident(h.to(device).contiguous(), nh_host.to(device), self.nh_early_host.to(device))
        return self

    @classmethod
    def from_files(cls, pairs: Sequence[Tuple[str, str]], sample_rate: int, device="cuda:0", resample: bool = True) -> "RirPool":
        """A pool of measured responses read from pairs of files (target response, interferer response) of one room each.
        resample=True: a file at another rate is converted on the device (``audio.resample``); False: it is an error
        (``load_wav``).  Every response keeps its own length; the table is as wide as the longest."""
        from . import audio
        from .trainer import load_wav, load_wav_native
        device = _device(device)
        rows = []
        for path in (p for pair in pairs for p in pair):
            if resample:
                wav, sr = load_wav_native(path)
                wav = wav.to(device)
                rows.append(wav if sr == sample_rate else audio.resample(wav.contiguous(), sr, sample_rate))
            else:
                rows.append(load_wav(path, sample_rate).to(device))
        if not rows:
            raise ValueError("from_files: no responses")
        H = max(r.numel() for r in rows)
        if H > MAX_TAPS_FFT:
            raise ValueError(f"from_files: a response has {H} samples at {sample_rate} Hz, more than {MAX_TAPS_FFT}: cut it first")
        h = torch.zeros(len(rows), H, dtype=torch.float32, device=device)
        for k, r in enumerate(rows):
            h[k, :r.numel()] = r
        return cls.from_responses(h, [r.numel() for r in rows], sample_rate, device)

    def __len__(self) -> int:
        return self.R

    def redraw(self, epoch: int) -> "RirPool":
        if self.draw is None:
            return self                                                            # fixed responses: nothing to draw
        return RirPool(self.R, self.device, self.seed, epoch, **self.draw)


def item_draws(seed: int, epoch: int, rank: int, n: int, rooms: int, sir_db: Optional[Tuple[float, float]]):
    """The per-item draws of one epoch, from a generator of their own (the crop generator's stream is not touched): room [n] int64
    uniform over ``rooms``, sir [n] fp64 uniform in ``sir_db`` (None: no level control, zeros)."""
    from .mixing import crop_seed
    g = torch.Generator().manual_seed(crop_seed(seed, epoch, rank) ^ ITEM_SALT)
    u = torch.rand(n, 2, dtype=torch.float64, generator=g)
    room = torch.clamp((u[:, 0] * rooms).to(torch.int64), max=rooms - 1)
    sir = torch.zeros(n, dtype=torch.float64) if sir_db is None else sir_db[0] + u[:, 1] * (sir_db[1] - sir_db[0])
    return room, sir
