"""Reverberation on the device (csrc/reverb.hip): room impulse responses of shoebox rooms by the image method, the per-row FIR
that applies them, and the pool of responses the training mixtures draw from.  The contracts are the text in
include/voicesplit_hip.h.  The image method is restated (Allen & Berkley 1979), NOT compared with a pyroomacoustics or
rir-generator run.

    shoebox_rir(rooms)                h [R, H] fp32 on the device for the room table ``rooms`` (``vs_rir_shoebox``)
    fir_rows(flat, at, lo, nh, ..)    ``vs_fir_rows`` on a flat buffer: every row its own filter, history and start
    apply(wav, h, hrow, nh, math)     wav [B, N] convolved row by row (zero history), same length
    row_energy(y)                     [B] fp64 sums of squares (``vs_row_energy``)
    draw_rooms(R, generator, ..)      host fp64: R random rooms, one receiver and TWO sources each -> a table of 2 R responses
    RirPool(R, ..)                    the responses of R drawn rooms resident on one device; ``redraw(epoch)`` makes a fresh pool

A room table is a float64 tensor [R, 19] on the host, one response per row:
size (3) | source (3) | receiver (3) | beta x0 x1 y0 y1 z0 z1 (6) | c | fs | nh | max_order (-1 = no limit).
The draws are host arithmetic and need no device; everything else has no CPU fallback.
"""
import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _call, _lib

MAX_TAPS = 8192
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


def apply(wav: torch.Tensor, h: torch.Tensor, hrow: Optional[torch.Tensor] = None, nh: Optional[torch.Tensor] = None,
          math: str = "f16x3") -> torch.Tensor:
    """wav [B, N] convolved with one response per row, truncated to N samples (silence in front of every row).  h [R, H]; hrow [B]
    picks each row's response (default: row b takes h[b], so R must be B), nh [B] its number of taps (default: all H)."""
    if wav.dim() != 2 or h.dim() != 2:
        raise ValueError(f"wav: expected [B, N], h [R, H]; got {tuple(wav.shape)} and {tuple(h.shape)}")
    _call.dev_check(wav, "wav")
    B, N = wav.shape
    dev = wav.device
    if hrow is None:
        if h.shape[0] != B:
            raise ValueError(f"h has {h.shape[0]} responses for {B} rows: pass hrow")
        hrow = torch.arange(B, dtype=torch.int32, device=dev)
    if nh is None:
        nh = torch.full((B,), h.shape[1], dtype=torch.int32, device=dev)
    at = torch.arange(B, dtype=torch.int64, device=dev) * N
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
               margin: float = 0.5, fs: int = 16000, nh: Optional[int] = None, c: float = SPEED_OF_SOUND, max_order: int = -1):
    """R random rooms from ``generator`` (ONE block of R x 13 uniform fp64 draws, then plain arithmetic): the table [2 R, 19] -- rows
    2 r and 2 r + 1 are the target and the interferer source of room r, heard at the same receiver -- and the reverberation times [R].
    Per room: the size uniform in the box ``size``, rt60 uniform in ``rt60``, the receiver uniform in the room at least ``margin``
    from every wall; each source on a uniformly drawn line through the receiver, on the side with more room, at a
    distance uniform in ``distance``, shortened to 0.95 of what that side allows inside the margins.  All walls share Sabine's beta (``sabine_beta``).  nh: taps per response, default
    min(8192, ceil(rt60 fs)) of each room."""
    if R <= 0:
        raise ValueError(f"draw_rooms: R={R}")
    lo3, hi3 = [float(v) for v in size[0]], [float(v) for v in size[1]]
    if any(l <= 2.0 * margin or h < l for l, h in zip(lo3, hi3)):
        raise ValueError(f"draw_rooms: every room size must exceed twice the margin {margin}, and size[0] <= size[1]")
    if not (0.0 < rt60[0] <= rt60[1]) or not (0.0 < distance[0] <= distance[1]):
        raise ValueError("draw_rooms: rt60 and distance are (low, high) with 0 < low <= high")
    if nh is not None and not (1 <= int(nh) <= MAX_TAPS):
        raise ValueError(f"draw_rooms: nh={nh} (1 .. {MAX_TAPS})")
    U = torch.rand(R, DRAWS_PER_ROOM, dtype=torch.float64, generator=generator).tolist()
    rows, times = [], []
    for u in U:
        L = [lo3[d] + u[d] * (hi3[d] - lo3[d]) for d in range(3)]
        t60 = rt60[0] + u[3] * (rt60[1] - rt60[0])
        mic = [margin + u[4 + d] * (L[d] - 2.0 * margin) for d in range(3)]
        beta = sabine_beta(L, t60)
        taps = min(MAX_TAPS, int(math.ceil(t60 * fs))) if nh is None else int(nh)
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
    for that on the device (``_call.Built``), so a pool may be drawn under one stream and used under any other."""

    def __init__(self, R: int, device="cuda:0", seed: int = 0, epoch: int = 0, **draw):
        from .mixing import crop_seed
        self.R, self.seed, self.epoch, self.draw = int(R), int(seed), int(epoch), dict(draw)
        g = torch.Generator().manual_seed(crop_seed(self.seed, self.epoch, 0) ^ POOL_SALT)
        rooms, rt60 = draw_rooms(self.R, g, **draw)
        self._adopt(rooms, rt60, shoebox_rir(rooms, device))

    def _resident(self, h, nh, nh_early):
        self._h, self._nh, self._nh_early, self.device = h, nh, nh_early, h.device
        self._built = _call.Built(h.device)

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
