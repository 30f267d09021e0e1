"""Training mixtures built on the device from a pool of clean utterances: what ``preprocess_by_csv.py`` + ``mix_wavfiles``
(utils/generic_utils.py:300-345) prepare on the CPU, one triplet at a time into files, as two calls into
libvoicesplit_hip.so (csrc/mix.hip) in front of the GPU front end that is already there.

    emb_audio / clean_audio / interference, _ = librosa.effects.trim(.., top_db=20)   ->  ClipPool (vs_trim_bounds, once per pool)
    if clean < audio_len or interference < audio_len: return                          ->  plan_triplets
    mixed = clean[:L] + interference[:L]; norm = max|mixed| * 1.1; x / norm           ->  vs_mix_clips (one launch sequence per batch)
    ap.get_spec_from_audio_path(..)                                                   ->  audio.wav_to_spec
    the d-vector of the trimmed reference utterance                                   ->  ClipPool.embed (speaker.logmel + embed_many)

``MixtureBatches.epoch(e)`` yields ``BatchFeeder.epoch``'s tuples straight from the resident pool -- no file and no host round trip per
batch -- and ``python -m voicesplit_amd.mixing`` writes the reference's on-disk dataset with the same code.  The planner (which
triplets, which crop offsets) is host integer arithmetic, done once per epoch.  There is no CPU fallback for the device half.
"""
import argparse
import csv
import os
import warnings
from typing import Iterator, List, Optional, Sequence, Tuple

import torch

from . import _call, _lib
from .config import resolve_audio

MIN_CLIP = 1025                       # vs_trim_bounds: the reflect padding of 1024 samples needs y[1024]
DEFAULT_FORMAT = {"emb": "*-emb.pt", "mixed": "*-mixed.pt", "target": "*-target.pt", "target_wav": "*-target.wav",
                  "mixed_wav": "*-mixed.wav", "emb_wav": "*-emb.wav"}
Triplet = Tuple[int, int, int]        # pool ids of (clean, reference, interferer): the CSV's column order


# ---------------------------------------------------------------------------------------------
# the pool
# ---------------------------------------------------------------------------------------------
class ClipPool:
    """Clean utterances resident on one device as ONE flat fp32 buffer.

    ``flat`` [total] (device), ``offsets`` [N + 1] int64 (host; ``offsets_dev`` its device copy), and per clip, computed once at
    construction by ``vs_trim_bounds`` and copied to the host once: ``bounds`` [N, 2] int32 = ``librosa.effects.trim(y, top_db=20)``'s
    (start, end) and ``peak`` [N] = max |y| over the trimmed region."""

    def __init__(self, waveforms: Sequence[torch.Tensor], device="cuda:0", trim: bool = True, normalize: Optional[float] = None,
                 sample_rate: int = 16000, peak_db: Optional[float] = -2.0):
        """trim=False (a pool of noise recordings, which are used whole): no ``vs_trim_bounds`` pass and no minimum length;
        ``bounds`` is (0, n) for every clip and ``peak`` is None.
        normalize: None, or the target in LUFS: every clip (at ``sample_rate``) is brought to it by ``loudness.normalize_clips_``
        (BS.1770 integrated loudness, one linear gain, peak cap ``peak_db``) before the trim pass, so ``bounds``, ``peak`` and
        ``range`` are those of the normalised clips; ``lufs`` [N] fp64 (before the gain) and ``gain`` [N] fp32 are kept on the host."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.VoiceSplitHipError(f"ClipPool on {device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
        if len(waveforms) == 0:
            raise ValueError("ClipPool: no clips")
        sizes = []
        for k, w in enumerate(waveforms):
            if w.dim() != 1 or w.dtype != torch.float32:
                raise ValueError(f"clip {k}: expected a 1-D float32 waveform, got {tuple(w.shape)} {w.dtype}")
            if trim and w.numel() < MIN_CLIP:
                raise ValueError(f"clip {k} has {w.numel()} samples, fewer than {MIN_CLIP}: silence trimming is not defined for it")
            sizes.append(w.numel())
        self.device = device
        self.offsets = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.tensor(sizes, dtype=torch.int64).cumsum(0)
        self.total = int(self.offsets[-1])
        self.flat = torch.empty(self.total, dtype=torch.float32, device=device)
        for o, w in zip(self.offsets.tolist(), waveforms):
            self.flat[o:o + w.numel()].copy_(w)
        self.offsets_dev = self.offsets.to(device)
        self._normalize(normalize, sample_rate, peak_db)
        self._trim() if trim else self._whole()

    @classmethod
    def from_files(cls, paths: Sequence[str], sample_rate: int, device="cuda:0", resample: bool = False, trim: bool = True,
                   normalize: Optional[float] = None, peak_db: Optional[float] = -2.0) -> "ClipPool":
        """resample=False: every file must be at ``sample_rate`` (``load_wav`` raises otherwise).  resample=True: what
        ``librosa.load(path, sr=sample_rate)`` does -- the files are grouped by their own rate, every off-rate group is uploaded as it
        is and converted by one ``vs_resample_clips`` call straight into the pool's flat buffer, files at ``sample_rate`` are copied.
        normalize: None, or the target in LUFS (see ``__init__``); the gain is applied after the conversion and before the trim pass."""
        from .trainer import load_wav, load_wav_native
        if not resample:
            return cls([load_wav(p, sample_rate) for p in paths], device, trim, normalize, sample_rate, peak_db)
        from .resample import Resampler, out_len, plan
        loaded = [load_wav_native(p) for p in paths]
        plans = {sr: plan(sr, sample_rate) for sr in sorted({sr for _, sr in loaded})}
        # the pool's clips are the converted ones: lay them out first (ClipPool checks their sizes), then fill them group by group
        sizes = [out_len(plans[sr], w.numel()) for w, sr in loaded]
        self = cls.__new__(cls)
        self._layout(sizes, device, trim)
        for sr in plans:
            group = [k for k, (_, r) in enumerate(loaded) if r == sr]
            if sr == sample_rate:
                for k in group:
                    o = int(self.offsets[k])
                    self.flat[o:o + sizes[k]].copy_(loaded[k][0])
                continue
            n_in = torch.tensor([loaded[k][0].numel() for k in group], dtype=torch.int64)
            table = torch.stack((n_in.cumsum(0) - n_in, n_in, self.offsets[group]), dim=1)
            staged = torch.empty(int(n_in.sum()), dtype=torch.float32, device=self.device)
            for o, k in zip(table[:, 0].tolist(), group):
                staged[o:o + loaded[k][0].numel()].copy_(loaded[k][0])
            Resampler(sr, sample_rate, self.device).clips_into(staged, self.flat, table)
        self._normalize(normalize, sample_rate, peak_db)
        self._trim() if trim else self._whole()
        return self

    def _normalize(self, target: Optional[float], sample_rate: int, peak_db: Optional[float]) -> None:
        """normalize=None leaves the pool as it is (``lufs`` and ``gain`` are None)."""
        self.lufs = self.gain = None
        if target is None:
            return
        from .loudness import normalize_clips_
        table = torch.stack((self.offsets[:-1], self.offsets[1:] - self.offsets[:-1]), dim=1)
        lufs, gain = normalize_clips_(self.flat, table, int(sample_rate), float(target), peak_db)
        self.lufs, self.gain = lufs.cpu(), gain.cpu()

    def _layout(self, sizes: Sequence[int], device, trim: bool = True) -> None:
        """offsets / total / an uninitialised ``flat`` for clips of ``sizes`` samples."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.VoiceSplitHipError(f"ClipPool on {device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
        if len(sizes) == 0:
            raise ValueError("ClipPool: no clips")
        for k, n in enumerate(sizes):
            if trim and n < MIN_CLIP:
                raise ValueError(f"clip {k} has {n} samples, fewer than {MIN_CLIP}: silence trimming is not defined for it")
        self.device = device
        self.offsets = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.tensor(list(sizes), dtype=torch.int64).cumsum(0)
        self.total = int(self.offsets[-1])
        self.flat = torch.empty(self.total, dtype=torch.float32, device=device)
        self.offsets_dev = self.offsets.to(device)

    @classmethod
    def planned(cls, lengths: Sequence[int], bounds: Sequence[Sequence[int]], peak: Optional[Sequence[float]] = None,
                value_range: Optional[Sequence[Sequence[float]]] = None) -> "ClipPool":
        """A pool without audio: the per-clip numbers the host planner reads (dry runs, tests without a device).  value_range: [N][2]
        (min, max) of every trimmed region, what ``ClipPool.range`` computes on the device (the overlay planner reads it)."""
        self = cls.__new__(cls)
        self.device, self.flat, self.offsets_dev = None, None, None
        self.lufs = self.gain = None
        self.offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.tensor(list(lengths), dtype=torch.int64).cumsum(0)
        self.total = int(self.offsets[-1])
        self.bounds = torch.tensor([list(b) for b in bounds], dtype=torch.int32).reshape(-1, 2)
        self.peak = torch.ones(len(lengths)) if peak is None else torch.tensor(list(peak), dtype=torch.float32)
        if not (len(self.bounds) == len(self.peak) == len(lengths)):
            raise ValueError("planned: lengths, bounds and peak must describe the same clips")
        if value_range is not None:
            self._range = torch.tensor([list(r) for r in value_range], dtype=torch.float32).reshape(-1, 2)
            if len(self._range) != len(lengths):
                raise ValueError("planned: lengths and value_range must describe the same clips")
        return self

    def _whole(self):
        """the untrimmed pool: every clip is its own region"""
        n = self.offsets[1:] - self.offsets[:-1]
        self.bounds = torch.stack((torch.zeros_like(n), n), dim=1).to(torch.int32)
        self.peak = None

    def _trim(self):
        n = len(self)
        ws = torch.empty(_call.sized("trim_workspace_bytes", self.total, n), dtype=torch.uint8, device=self.device)
        bounds = torch.empty(n, 2, dtype=torch.int32, device=self.device)
        peak = torch.empty(n, dtype=torch.float32, device=self.device)
        _call.call("trim_bounds", self.device, self.flat, self.total, self.offsets, self.offsets_dev, n, bounds, peak, ws, ws.numel())
        self.bounds, self.peak = bounds.cpu(), peak.cpu()

    def __len__(self) -> int:
        return self.offsets.numel() - 1

    @property
    def range(self) -> torch.Tensor:
        """[N, 2] float32 on the host: (min, max) of every trimmed region, exact -- what ``minmax_scale`` reads of a trimmed clip.
        Computed by ``vs_clip_range`` at first use and copied to the host once."""
        if getattr(self, "_range", None) is None:
            if self.flat is None:
                raise _lib.VoiceSplitHipError("this pool holds no audio (ClipPool.planned without value_range=): the value ranges are "
                                              "computed on an MI355X (HIP) device only")
            out = torch.empty(len(self), 2, dtype=torch.float32, device=self.device)
            bounds = self.bounds.to(self.device)
            _call.call("clip_range", self.device, self.flat, self.total, self.offsets, self.offsets_dev, bounds, len(self), out)
            self._range = out.cpu()
        return self._range

    @property
    def lengths(self) -> torch.Tensor:
        """[N] int64 on the host: the untrimmed lengths."""
        return self.offsets[1:] - self.offsets[:-1]

    @property
    def trimmed_lengths(self) -> torch.Tensor:
        """[N] int64 on the host."""
        return (self.bounds[:, 1] - self.bounds[:, 0]).to(torch.int64)

    @property
    def trimmed_starts(self) -> torch.Tensor:
        """[N] int64 on the host: index in ``flat`` of every clip's first sample after trimming."""
        return self.offsets[:-1] + self.bounds[:, 0].to(torch.int64)

    def trimmed_length(self, i: int) -> int:
        return int(self.bounds[i, 1]) - int(self.bounds[i, 0])

    def trimmed(self, i: int) -> torch.Tensor:
        """The trimmed clip: a view into ``flat``."""
        o = int(self.offsets[i])
        return self.flat[o + int(self.bounds[i, 0]):o + int(self.bounds[i, 1])]

    @torch.no_grad()
    def embed(self, encoder, audio_cfg, ids: Sequence[int], batch: int = 64) -> torch.Tensor:
        """[len(ids), emb_dim] d-vectors of the TRIMMED clips (the reference embeds the trimmed utterance it writes as ``*-emb.wav``):
        ``speaker.logmel`` per clip, ``encoder.embed_many`` per ``batch`` clips.  A clip too short for one encoder window (or for
        the STFT's reflect padding) gets a zero row, the counterpart of the ``[0]`` marker of the ``*-emb.pt`` files."""
        from .speaker import logmel
        ids = [int(i) for i in ids]
        out = torch.zeros(len(ids), encoder.emb_dim, device=self.device)
        audio_cfg = resolve_audio(audio_cfg)
        min_len = int(audio_cfg["n_fft"]) // 2
        for lo in range(0, len(ids), batch):
            rows = [(k, i) for k, i in enumerate(ids[lo:lo + batch], lo) if self.trimmed_length(i) > min_len]
            if not rows:
                continue
            dvec = encoder.embed_many([logmel(self.trimmed(i), audio_cfg, encoder.num_mels) for _, i in rows])[0]
            out[torch.tensor([k for k, _ in rows], device=self.device)] = dvec
        return out


# ---------------------------------------------------------------------------------------------
# the host planner
# ---------------------------------------------------------------------------------------------
def samples_for(audio_cfg, audio_len) -> int:
    """``int(sample_rate * audio_len)`` (mix_wavfiles:314)."""
    return int(audio_cfg["sample_rate"] * audio_len)


def keep_mask(pool: ClipPool, triplets: Sequence[Triplet], L: int, emb_ok: Optional[Sequence[bool]] = None) -> List[bool]:
    tl, peak = pool.trimmed_lengths.tolist(), pool.peak.tolist()
    ok = [tl[k] >= L and peak[k] > 0.0 for k in range(len(tl))]
    return [bool(ok[c] and ok[i] and (emb_ok is None or emb_ok[r])) for c, r, i in triplets]


def plan_triplets(pool: ClipPool, triplets: Sequence[Triplet], L: int, emb_ok: Optional[Sequence[bool]] = None):
    """(kept triplets, number dropped).  Dropped: a clean or interferer clip shorter than ``L`` after trimming (mix_wavfiles:317-318),
    a clean or interferer clip whose trimmed region is all zero (it cannot be normalised: ``valid == 0`` of vs_mix_clips becomes an
    assertion instead of a per-batch filter), and, with ``emb_ok`` [N] given, a reference clip without an embedding (the ``[0]``
    items the reference's collate drops, utils/dataset.py:93-95)."""
    keep = keep_mask(pool, triplets, L, emb_ok)
    kept = [tuple(t) for t, k in zip(triplets, keep) if k]
    return kept, len(triplets) - len(kept)


def crop_seed(seed: int, epoch: int, rank: int) -> int:
    return ((int(seed) * 1000003 + int(epoch)) * 1000003 + int(rank)) % (2 ** 63)


def crop_offsets(room: torch.Tensor, crop: str, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Crop offsets for items with ``room`` = trimmed length - L >= 0 samples to spare (int64, any shape): "head" -> 0 (the
    reference's ``[:L]``), "random" -> uniform on 0 .. room from ``generator``."""
    if crop == "head":
        return torch.zeros_like(room)
    if crop != "random":
        raise ValueError(f"crop must be 'head' or 'random', got {crop!r}")
    if room.numel() and int(room.min()) < 0:
        raise ValueError("a clip is shorter than the crop (run plan_triplets first)")
    u = torch.rand(room.shape, dtype=torch.float64, generator=generator)
    return torch.minimum((u * (room + 1).to(torch.float64)).to(torch.int64), room)


def read_triplet_csv(path: str, root: str, librispeech: bool = False):
    """The path rules of preprocess_by_csv.py:74-99 for a CSV with a header line and rows [clean, embedding, interference]:
    ``root/name``, or with ``librispeech`` ``root/<speaker>/<chapter>/<name>-norm.wav`` from ``name = speaker-chapter-utterance``.
    Returns (paths, triplets, numbers, skipped): the distinct files in order of first use, the triplets as indices into them, each
    triplet's row number in the CSV (its ``%06d`` file name) and how many rows named a missing file (the reference prints and goes on)."""
    def full(name):
        if librispeech:
            s = name.split("-")
            return os.path.join(root, s[0], s[1], name + "-norm.wav")
        return os.path.join(root, name)

    paths, index, triplets, numbers, skipped = [], {}, [], [], 0
    exists = {}
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))[1:]                    # pd.read_csv: the first line is the header
    for num, row in enumerate(r for r in rows if r):
        if len(row) != 3:
            raise ValueError(f"{path}: row {num} has {len(row)} fields, expected clean,embedding,interference")
        files = [full(name.strip()) for name in row]
        for f in files:
            if f not in exists:
                exists[f] = os.path.isfile(f)
        if not all(exists[f] for f in files):
            skipped += 1
            continue
        for f in files:
            if f not in index:
                index[f] = len(paths)
                paths.append(f)
        triplets.append(tuple(index[f] for f in files))
        numbers.append(num)
    return paths, triplets, numbers, skipped


def output_name(out_dir: str, pattern: str, num: int) -> str:
    """glob_re_to_filename (utils/generic_utils.py:347-350)."""
    return os.path.join(out_dir, pattern.replace("*", "%06d" % num))


# ---------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------
def mix_clips(flat: torch.Tensor, clean_at: torch.Tensor, interf_at: torch.Tensor, L: int, invalid_count: Optional[torch.Tensor] = None):
    """vs_mix_clips: (mixed_wav [B, L], target_wav [B, L], norm [B], valid [B] int32) for the items starting at the absolute sample
    indices ``clean_at`` / ``interf_at`` ([B] int64 on the device) of ``flat``."""
    if not flat.is_cuda:
        raise _lib.VoiceSplitHipError(f"the pool is on {flat.device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
    for name, t in (("clean_at", clean_at), ("interf_at", interf_at)):
        if t.dtype != torch.int64 or t.device != flat.device or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"{name}: expected a contiguous 1-D int64 tensor on {flat.device}")
    B = clean_at.numel()
    if interf_at.numel() != B:
        raise ValueError("clean_at and interf_at differ in length")
    dev = flat.device
    mixed = torch.empty(B, L, device=dev)
    target = torch.empty(B, L, device=dev)
    norm = torch.empty(B, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _call.call("mix_clips", dev, flat, flat.numel(), clean_at, interf_at, B, int(L), mixed, target, norm, valid, invalid_count)
    return mixed, target, norm, valid


class MixtureBatches:
    """``BatchFeeder`` for a resident pool: ``epoch(e)`` yields (emb, target, mixed, seq_len, target_wav, phase) in ``shard``'s order,
    every batch made on the device from its (clean, reference, interferer) triplets.

    triplets: what ``plan_triplets`` kept (every clean / interferer clip at least ``audio_len`` long after trimming);
    ``shard.n`` must be their number.  emb_table: [N, emb_dim] on the pool's device, row = pool id of the reference clip
    (``pool.embed(encoder, audio_cfg, range(len(pool)))``), or with ``emb_rows="triplet"`` one row per triplet (precomputed
    ``*-emb.pt`` files).  crop: "head" = the reference's ``[:L]``; "random" = both crop offsets uniform over what the trimmed clip
    allows, from a generator seeded by (seed, epoch, shard.rank): the same three numbers give bit-identical batches.
    Per epoch the host plans every batch's indices and copies them to the device once; per batch it enqueues vs_mix_clips, the two
    front-end calls and the embedding gather -- no ``.item()``, no blocking copy.  ``target_wav`` stays on the device.
    Items that vs_mix_clips marks invalid (a crop whose sum is all zero: rows of zeros) are counted on the device; the count is
    read once behind every epoch (``invalid_items``) and reported as a warning.

    rir_pool (a ``reverb.RirPool``) and / or sir_db = (low, high): the two talkers in a room and / or at a drawn target-to-interferer
    ratio (``_reverberant``); with both None, the default, the path above is the one that runs.  history: "clip" = the reverberation
    of what the clip holds in front of the crop (from its trimmed start) rings into the crop, "zero" = silence in front of the crop.
    target: "reverberant" = the clean talker with the full response, "early" = with the response cut 50 ms behind the direct path
    (the mixture keeps the full response).  math: the FIR's arithmetic, "f16x3" (matrix cores), "fp32", or "fft": the full-response
    rows go through ``vs_fir_rows_fft`` with the pool's kept spectra (responses of up to 32768 taps; made once per pool), the
    ``target="early"`` rows stay on the f16x3 direct form (about 900 taps, where the direct form wins).
    A drawn pool belongs to ONE epoch: when ``items`` / ``epoch`` is asked for another epoch than ``rir_pool.epoch``, ``self.rir_pool``
    is replaced by ``rir_pool.redraw(epoch)`` (the object that was passed in is left as it is) -- a host loop over the rooms and one
    ``vs_rir_shoebox`` call, tens of milliseconds for a few hundred responses, once per epoch.  This holds for epoch 0 too: a pool
    built with ``epoch=3`` and used for epoch 0 (``write_dataset``) is redrawn.  ``RirPool.from_rooms`` pools are fixed and never redrawn."""

    def __init__(self, pool: ClipPool, triplets: Sequence[Triplet], emb_table: torch.Tensor, audio_cfg, audio_len, shard,
                 crop: str = "head", seed: int = 0, emb_rows: str = "clip", rir_pool=None, sir_db=None, history: str = "clip",
                 target: str = "reverberant", math: str = "f16x3"):
        if crop not in ("head", "random"):
            raise ValueError(f"crop must be 'head' or 'random', got {crop!r}")
        if history not in ("clip", "zero"):
            raise ValueError(f"history must be 'clip' or 'zero', got {history!r}")
        if target not in ("reverberant", "early"):
            raise ValueError(f"target must be 'reverberant' or 'early', got {target!r}")
        if math not in ("f16x3", "fp32", "fft"):
            raise ValueError(f"math must be 'f16x3', 'fp32' or 'fft', got {math!r}")
        if sir_db is not None:
            sir_db = (float(sir_db[0]), float(sir_db[1]))
            if not sir_db[0] <= sir_db[1]:
                raise ValueError(f"sir_db must be (low, high) in dB with low <= high, got {sir_db}")
        self.rir_pool, self.sir_db, self.history, self.target, self.math = rir_pool, sir_db, history, target, math
        self._gain_tables = {}
        if emb_rows not in ("clip", "triplet"):
            raise ValueError(f"emb_rows must be 'clip' or 'triplet', got {emb_rows!r}")
        self.pool, self.acfg, self.shard, self.crop, self.seed = pool, audio_cfg, shard, crop, int(seed)
        self.L = samples_for(audio_cfg, audio_len)
        audio_cfg = resolve_audio(audio_cfg)
        hop = int(audio_cfg["hop_length"])
        if self.L <= 0 or self.L % hop:
            raise ValueError(f"audio_len {audio_len} s = {self.L} samples must be a positive multiple of hop_length {hop}")
        self.tri = torch.tensor([list(t) for t in triplets], dtype=torch.int64).reshape(-1, 3)
        if shard is not None and shard.n != len(self.tri):
            raise ValueError(f"the shard walks {shard.n} items, there are {len(self.tri)} triplets")
        if len(self.tri) and (int(self.tri.min()) < 0 or int(self.tri.max()) >= len(pool)):
            raise ValueError("a triplet names a clip outside the pool")
        tl = pool.trimmed_lengths
        self.room = torch.stack([tl[self.tri[:, 0]], tl[self.tri[:, 2]]], dim=1) - self.L          # [n, 2]: clean, interferer
        if len(self.tri) and int(self.room.min()) < 0:
            raise ValueError(f"a clean or interferer clip is shorter than {self.L} samples after trimming (run plan_triplets first)")
        starts = pool.trimmed_starts
        self.start = torch.stack([starts[self.tri[:, 0]], starts[self.tri[:, 2]]], dim=1)          # [n, 2]
        self.emb_table, self.emb_rows = emb_table, emb_rows
        rows = len(pool) if emb_rows == "clip" else len(self.tri)
        if emb_table.dim() != 2 or emb_table.shape[0] != rows or emb_table.dtype != torch.float32:
            raise ValueError(f"emb_table: expected float32 [{rows}, emb_dim], got {tuple(emb_table.shape)} {emb_table.dtype}")
        self.device = emb_table.device if pool.device is None else pool.device
        if pool.device is not None and emb_table.device != pool.device:
            raise ValueError(f"emb_table is on {emb_table.device}, the pool on {pool.device}")
        self._invalid = torch.zeros(1, dtype=torch.int32, device=self.device) if pool.device is not None else None
        self.invalid_items = 0

    # -- host: one epoch's (or any list of batches') indices -------------------------------------------------------------------------
    def plan(self, index_batches: Sequence[Sequence[int]], epoch: int = 0):
        """(positions, at, emb_row) for the triplet positions of ``index_batches`` laid end to end: at [2, total] int64 = absolute
        index in ``pool.flat`` of every item's first clean / interferer sample; emb_row [total] = row of ``emb_table``."""
        pos = torch.tensor([int(p) for b in index_batches for p in b], dtype=torch.int64)
        rank = self.shard.rank if self.shard is not None else 0
        g = torch.Generator().manual_seed(crop_seed(self.seed, epoch, rank))
        at = (self.start[pos] + crop_offsets(self.room[pos], self.crop, g)).t().contiguous()
        emb_row = self.tri[pos, 1] if self.emb_rows == "clip" else pos
        return pos, at, emb_row.contiguous()

    # -- device ----------------------------------------------------------------------------------------------------------------------
    def items(self, index_batches: Sequence[Sequence[int]], epoch: int = 0) -> Iterator[dict]:
        """One dict per batch of ``index_batches`` (lists of triplet positions, any sizes): the six tensors of ``epoch`` under their
        names plus ``mixed_wav``, ``norm``, ``valid`` and ``positions``."""
        from . import audio
        if self.pool.flat is None:
            raise _lib.VoiceSplitHipError("this pool holds no audio (ClipPool.planned): batches are made on an MI355X (HIP) device only")
        index_batches = [list(b) for b in index_batches]
        pos, at, emb_row = self.plan(index_batches, epoch)
        at_dev, row_dev = at.to(self.device), emb_row.to(self.device)              # once per epoch
        lo = 0
        reverberant = self.rir_pool is not None or self.sir_db is not None
        if reverberant:
            draws = self._reverb_plan(pos, epoch)
        for b in index_batches:
            hi = lo + len(b)
            if reverberant:
                mixed_wav, target_wav, norm, valid, rows = self._reverberant(at_dev[:, lo:hi], {k: v[..., lo:hi] for k, v in draws.items()})
            else:
                mixed_wav, target_wav, norm, valid = mix_clips(self.pool.flat, at_dev[0, lo:hi], at_dev[1, lo:hi], self.L, self._invalid)
            mixed, phase = audio.wav_to_spec(mixed_wav, self.acfg, want_phase=True)
            target, _ = audio.wav_to_spec(target_wav, self.acfg, want_phase=False)
            emb = self.emb_table.index_select(0, row_dev[lo:hi])
            seq_len = torch.full((len(b),), self.L, dtype=torch.int64, device=self.device)
            item = {"emb": emb, "target": target, "mixed": mixed, "seq_len": seq_len, "target_wav": target_wav, "phase": phase,
                    "mixed_wav": mixed_wav, "norm": norm, "valid": valid, "positions": pos[lo:hi]}
            if reverberant:
                item["rows"] = rows                                                # [2 B, L]: the clean and the scaled interferer rows
            yield item
            lo = hi
        self._report_invalid()

    # -- the two talkers in a room, at a drawn level ----------------------------------------------------------------------------------
    def _reverb_plan(self, pos: torch.Tensor, epoch: int) -> dict:
        """One epoch's per-item draws (a generator of their own: the crops are those of the epoch without reverberation) and row
        tables, on the device: hrow / nh / nh_early [2, n] (clean, interferer), lo [2, n] and sir [n]."""
        from . import reverb
        if self.rir_pool is None:
            self.rir_pool = reverb.RirPool.impulses(self.device)
        elif self.rir_pool.epoch != epoch:
            self.rir_pool = self.rir_pool.redraw(epoch)                            # fresh rooms every epoch (a fixed pool returns itself)
        pool = self.rir_pool
        rank = self.shard.rank if self.shard is not None else 0
        room, sir = reverb.item_draws(self.seed, epoch, rank, pos.numel(), len(pool), self.sir_db)
        hrow = torch.stack((2 * room, 2 * room + 1))
        d = {"hrow": hrow.to(torch.int32), "nh": pool.nh_host[hrow], "nh_early": pool.nh_early_host[hrow], "sir": sir[None]}
        if self.history == "clip":
            d["lo"] = self.start[pos].t().contiguous()
        return {k: v.contiguous().to(self.device) for k, v in d.items()}

    def _reverberant(self, at: torch.Tensor, d: dict):
        """One batch: vs_fir_rows writes the clean rows, the interferer rows (and for target="early" the clean rows once more, with
        the cut response) into a scratch [2 B (+ B), L]; vs_row_energy; the interferer rows times g = sqrt(E_c / E_i 10^(-sir / 10));
        then the unchanged vs_mix_clips on the scratch.  Returns its four tensors and the 2 B rows it mixed."""
        from . import reverb
        B, L, pool, dev = at.shape[1], self.L, self.rir_pool, self.device
        early = self.target == "early"
        rows = 3 * B if early else 2 * B
        at2 = at.reshape(-1)
        lo2 = d["lo"].reshape(-1) if "lo" in d else at2
        hrow, nh = d["hrow"].reshape(-1), d["nh"].reshape(-1)
        if early:
            at2, lo2 = torch.cat((at2, at2[:B])), torch.cat((lo2, lo2[:B]))
            hrow, nh = torch.cat((hrow, hrow[:B])), torch.cat((nh, d["nh_early"][0]))
        if self.math == "fft":
            scratch = torch.empty(rows, L, dtype=torch.float32, device=dev)
            reverb.fir_rows_fft(self.pool.flat, at2[:2 * B].contiguous(), lo2[:2 * B].contiguous(), hrow[:2 * B].contiguous(), pool.spectra, L,
                                out=scratch[:2 * B])
            if early:
                reverb.fir_rows(self.pool.flat, at2[2 * B:].contiguous(), lo2[2 * B:].contiguous(), nh[2 * B:].contiguous(),
                                hrow[2 * B:].contiguous(), pool.h_early, L, "f16x3", out=scratch[2 * B:])
        else:
            scratch, _, _ = reverb.fir_rows(self.pool.flat, at2.contiguous(), lo2.contiguous(), nh.contiguous(), hrow.contiguous(), pool.h, L,
                                            self.math)
        if self.sir_db is not None:
            e = reverb.row_energy(scratch[:2 * B])
            ratio = e[:B] / e[B:] * torch.pow(10.0, -d["sir"][0] / 10.0)
            g = torch.where(e[B:] > 0, ratio.sqrt(), torch.ones_like(ratio)).to(torch.float32)
            if B not in self._gain_tables:                                         # the interferer rows of the scratch as a clip table
                table = torch.stack((torch.arange(B, 2 * B, dtype=torch.int64) * L, torch.full((B,), L, dtype=torch.int64)), dim=1)
                self._gain_tables[B] = (table.contiguous(), table.to(dev))
            table, table_dev = self._gain_tables[B]
            _call.call("scale_clips", dev, scratch, scratch.numel(), table, table_dev, g, B)
        row_at = torch.arange(2 * B, dtype=torch.int64, device=dev) * L
        mixed_wav, target_wav, norm, valid = mix_clips(scratch.reshape(-1), row_at[:B], row_at[B:], L, self._invalid)
        if early:
            ok = (valid == 1)[:, None]
            target_wav = torch.where(ok, scratch[2 * B:] / norm[:, None], torch.zeros_like(target_wav))
        return mixed_wav, target_wav, norm, valid, scratch[:2 * B]

    def _report_invalid(self):
        n = int(self._invalid.item())                                              # once per epoch
        if n > self.invalid_items:
            warnings.warn(f"{n - self.invalid_items} mixtures of this epoch were all zero (crops that cancel or are silent): "
                          f"their rows are zero", RuntimeWarning)
        self.invalid_items = n

    def epoch(self, epoch: int):
        for it in self.items(self.shard.epoch(epoch), epoch):
            yield it["emb"], it["target"], it["mixed"], it["seq_len"], it["target_wav"], it["phase"]


# ---------------------------------------------------------------------------------------------
# items without voice overlay (preprocess_by_csv_without_voice_overlay.py + mix_wavfiles_without_voice_overlay)
# ---------------------------------------------------------------------------------------------
OVERLAY_DROPS = ("emb_short", "noise_short", "voice_short", "silent")
RATIO_CLEAN, RATIO_INTERF = 1e-2, 10.0 ** -1.5          # librosa.effects.split(top_db=20) / (top_db=15), :123 / :169
SEQ_ITEM_BYTES = 136                                   # vs_seq_item: 7 int64, 10 int32, 10 fp32
EMB_MIN_SAMPLES = 1.1 * 80 * 160                       # :74-78 a reference utterance shorter than this is discarded


def _minmax_affine(lo, hi, xmin, xmax):
    """fp64 tensors -> (scale, bias) of minmax_scale(x, feature_range=(lo, hi)): scale = (hi - lo) / (xmax - xmin), with 1 for the
    denominator of a constant signal, bias = lo - xmin * scale."""
    den = xmax - xmin
    den = torch.where(den == 0, torch.ones_like(den), den)
    scale = (hi - lo) / den
    return scale, lo - xmin * scale


class OverlayPlan:
    """What ``plan_overlay`` decided, host tensors over the n kept triplets: ``tri`` [n, 3] pool ids (clean, reference, interferer),
    ``positions`` [n] their index in the planner's input, ``noise_ids`` [n, 2], ``Lc`` / ``Li`` [n] samples, ``two_clean`` [n] bool,
    ``noise_start`` [n], the feature ranges ``amp`` [n, 3, 2] (emb, clean, interferer), ``range_random`` / ``range_plain`` [n, 2]
    (fp64), the random-amplitude voice affines ``gain`` / ``bias`` [n, 3] (fp64), the absolute indices ``clean_at`` / ``interf_at``
    (pool) and ``noise_at`` [n, 2] (noise pool), the regions ``split_regions`` [n, 2] (at, n) and ``split_ratio`` [n] whose split
    points the items need, and the expansion into items: ``item_trip`` / ``item_kind`` / ``item_len`` [m].  ``dropped``: a count per
    rule of OVERLAY_DROPS."""


def plan_overlay(pool: ClipPool, noise_pool: ClipPool, triplets: Sequence[Triplet], sample_rate: int, generator: torch.Generator,
                 kinds: Sequence[int] = (1, 2, 3, 4), seconds: Sequence[int] = (2, 3, 4)) -> OverlayPlan:
    """The draws of mix_wavfiles_without_voice_overlay for every triplet, the reference's drop rules, and the expansion of every
    surviving triplet into the requested kinds (1 the mixture, 2 clean in / clean out, 3 interferer in / silence out, 4 the mixture
    at random amplitudes).  Host arithmetic on ``pool.bounds``, ``pool.peak``, ``pool.range`` and the noise pool's lengths.

    The draws come from ``generator`` (seed it with ``crop_seed(seed, epoch, rank)``): they have the reference's DISTRIBUTIONS, not
    Python's Mersenne sequence -- the reference draws from the global ``random`` inside worker processes and is not reproducible
    itself.  Per triplet, all drawn before anything is dropped: the three (min_amp, extra) pairs and the random-amplitude noise pair
    (:30-46), two_clean (:80), the two lengths out of ``seconds`` (:83-86), noise_start (:94), the plain noise pair (:105-106), and
    two noise ids as the script draws them, ``files[randint(0, n) - 1]`` (the last file twice as likely as any other).
    Dropped, and counted in ``plan.dropped``: "emb_short" the reference clip's trimmed length is below 1.1 * 80 * 160 (:77);
    "noise_short" a noise recording is shorter than Lc + Li + 1 (:94 raises there); "voice_short" the clean or interferer clip is
    shorter than its drawn seconds after trimming (:99); "silent" a clean or interferer clip whose trimmed region is all zero."""
    kinds = tuple(int(k) for k in kinds)
    if not kinds or any(k not in (1, 2, 3, 4) for k in kinds):
        raise ValueError(f"kinds must be a non-empty subset of (1, 2, 3, 4), got {kinds}")
    if len(seconds) == 0 or any(int(sample_rate * s) < MIN_CLIP for s in seconds):
        raise ValueError(f"seconds {tuple(seconds)} at {sample_rate} Hz: every length must be at least {MIN_CLIP} samples")
    tri = torch.tensor([list(t) for t in triplets], dtype=torch.int64).reshape(-1, 3)
    n = len(tri)
    if n and (int(tri.min()) < 0 or int(tri.max()) >= len(pool)):
        raise ValueError("a triplet names a clip outside the pool")
    f64 = dict(dtype=torch.float64, generator=generator)
    u_amp = torch.rand(n, 3, 2, **f64)
    u_random = torch.rand(n, 2, **f64)
    two_clean = torch.randint(0, 2, (n,), generator=generator) == 0                  # not getrandbits(1)
    sec = torch.tensor([int(sample_rate * s) for s in seconds], dtype=torch.int64)[torch.randint(0, len(seconds), (n, 2), generator=generator)]
    u_start = torch.rand(n, **f64)
    u_plain = torch.rand(n, 2, **f64)
    noise_ids = (torch.randint(0, len(noise_pool) + 1, (n, 2), generator=generator) - 1) % len(noise_pool)

    Lc, Li = sec[:, 0], sec[:, 1]
    tl, peak, rng = pool.trimmed_lengths, pool.peak, pool.range.to(torch.float64)
    c, r, i = tri[:, 0], tri[:, 1], tri[:, 2]
    room = noise_pool.lengths[noise_ids].min(dim=1).values - (Lc + Li + 1)           # randint(0, room), both ends included
    drop = {"emb_short": tl[r].to(torch.float64) < EMB_MIN_SAMPLES}
    drop["noise_short"] = ~drop["emb_short"] & (room < 0)
    seen = drop["emb_short"] | drop["noise_short"]
    drop["voice_short"] = ~seen & ((tl[c] < Lc) | (tl[i] < Li))
    seen = seen | drop["voice_short"]
    drop["silent"] = ~seen & ((peak[c] <= 0) | (peak[i] <= 0))
    keep = ~(seen | drop["silent"])

    p = OverlayPlan()
    p.dropped = {k: int(v.sum()) for k, v in drop.items()}
    p.n_input, p.sample_rate, p.kinds = n, int(sample_rate), kinds
    p.positions = torch.nonzero(keep).flatten()
    k = p.positions
    p.tri, p.noise_ids, p.Lc, p.Li, p.two_clean = tri[k], noise_ids[k], Lc[k], Li[k], two_clean[k]
    p.noise_start = torch.minimum((u_start[k] * (room[k] + 1).to(torch.float64)).to(torch.int64), room[k])
    # feature ranges: a + (b - a) * u, also for a > b (:105 has a > b for a clip whose minimum is above -0.1)
    lo = -1.0 + 0.7 * u_amp[k, :, 0]
    p.amp = torch.stack((lo, -lo + 0.02 * u_amp[k, :, 1]), dim=2)                    # [n, 3, 2]
    a = torch.minimum(lo[:, 1], lo[:, 2])
    lo_r = a + (-0.1 - a) * u_random[k, 0]
    p.range_random = torch.stack((lo_r, -lo_r - 0.02 * u_random[k, 1]), dim=1)
    ck, rk, ik = p.tri[:, 0], p.tri[:, 1], p.tri[:, 2]
    a = torch.minimum(rng[ck, 0], rng[ik, 0])
    lo_p = a + (-0.1 - a) * u_plain[k, 0]
    p.range_plain = torch.stack((lo_p, -lo_p - 0.02 * u_plain[k, 1]), dim=1)
    # minmax_scale of the three voices over their whole trimmed clips, before the crop (:33-43)
    vr = torch.stack((rng[rk], rng[ck], rng[ik]), dim=1)                             # [n, 3, 2]
    p.gain, p.bias = _minmax_affine(p.amp[:, :, 0], p.amp[:, :, 1], vr[:, :, 0], vr[:, :, 1])
    starts = pool.trimmed_starts
    p.clean_at, p.interf_at = starts[ck], starts[ik]
    p.noise_at = noise_pool.offsets[:-1][p.noise_ids] + p.noise_start[:, None]
    p.split_regions = torch.stack((torch.where(p.two_clean, p.clean_at, p.interf_at), torch.where(p.two_clean, p.Lc, p.Li)), dim=1).contiguous()
    p.split_ratio = torch.where(p.two_clean, torch.tensor(RATIO_CLEAN, dtype=torch.float64), torch.tensor(RATIO_INTERF, dtype=torch.float64))
    # the items, triplet by triplet in the order of `kinds`
    m = len(k)
    p.item_trip = torch.arange(m, dtype=torch.int64).repeat_interleave(len(kinds))
    p.item_kind = torch.tensor(kinds, dtype=torch.int64).repeat(m)
    t = p.item_trip
    p.item_len = torch.where(p.item_kind == 2, p.Lc[t], torch.where(p.item_kind == 3, p.Li[t], p.Lc[t] + p.Li[t]))
    return p


def overlay_items(plan: OverlayPlan, split_points: torch.Tensor, counts: torch.Tensor, item_trip: Optional[torch.Tensor] = None,
                  item_kind: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[m, 136] uint8 on ``split_points``' device: one ``vs_seq_item`` per item (default: the plan's items; ``item_trip`` /
    ``item_kind`` [m] name others).  split_points, counts: [n] int32 per kept triplet, ``vs_split_point`` over
    ``plan.split_regions`` -- they stay on the device.  Everything the draws decide is assembled on the host (gains and biases in
    fp64, rounded once); the four things that depend on the split are patched in by a handful of tensor operations where the split
    points live, with no read-back: the lengths of the outer segments and the third segment's source, the noise offset of kinds
    2 and 3, and the two noise quirks below.

    With X the speaker that is split (clean when two_clean, else the interferer), Y the other, p the split point for more than one
    interval and len(X) for a single one (one formula for both branches):
      kinds 1, 4   segments X[:p], Y, X[p:]; the noise index runs on with the output index (:134-137, "noise without interruption");
                   the target holds the clean speaker's segments WITH their noise and is zero where the other speaker talks;
                   kind 4 takes the random-amplitude affines, except that the clean half of the single-interval interferer-first
                   branch gets the PLAIN noise (:212 adds noise_audio, not noise_audio_random)
      kind 2       the cropped clean clip as input and target, divided by kind 1's norm (:218-227); kind 3 the cropped interferer
                   as input, zeros as target.  Three of the four branches reassign clean_audio / interference to their noisy
                   versions (:157-158, :179, :205-206): the one that is NOT split carries the noise of its place in the mixture
                   (offset p), the split one carries noise from offset 0 in the single-interval branches and none otherwise."""
    dev = split_points.device
    t = plan.item_trip if item_trip is None else item_trip.to(torch.int64)
    kind = plan.item_kind if item_kind is None else item_kind.to(torch.int64)
    m = len(t)
    tc = plan.two_clean[t]
    Lc, Li = plan.Lc[t], plan.Li[t]
    x_at, y_at = torch.where(tc, plan.clean_at[t], plan.interf_at[t]), torch.where(tc, plan.interf_at[t], plan.clean_at[t])
    LX, LY = torch.where(tc, Lc, Li), torch.where(tc, Li, Lc)
    full, k2, k3, k4 = (kind == 1) | (kind == 4), kind == 2, kind == 3, kind == 4
    zero = torch.zeros(m, dtype=torch.int64)
    one = torch.ones(m, dtype=torch.int64)
    i64 = torch.stack((torch.where(full, x_at, torch.where(k2, plan.clean_at[t], plan.interf_at[t])), torch.where(full, y_at, zero), zero,
                       plan.noise_at[t, 0], plan.noise_at[t, 1], plan.noise_at[t, 0], plan.noise_at[t, 1]), dim=1)
    tci = tc.to(torch.int64)
    sel = torch.where(k4, one, zero)
    i32 = torch.stack((torch.where(full, LX, torch.where(k2, Lc, Li)), torch.where(full, LY, zero), zero,
                       torch.where(full, tci, k2.to(torch.int64)), torch.where(full, 1 - tci, zero), torch.where(full, tci, zero),
                       sel, sel, sel, Lc + Li), dim=1)
    # kind 4: the random-amplitude affine of X for segments 0 and 2, of Y for segment 1 (plan.gain columns: emb, clean, interferer)
    gx, gy = torch.where(tc, plan.gain[t, 1], plan.gain[t, 2]), torch.where(tc, plan.gain[t, 2], plan.gain[t, 1])
    bx, by = torch.where(tc, plan.bias[t, 1], plan.bias[t, 2]), torch.where(tc, plan.bias[t, 2], plan.bias[t, 1])
    o64, z64 = torch.ones(m, dtype=torch.float64), torch.zeros(m, dtype=torch.float64)
    f32 = torch.stack((torch.where(k4, gx, o64), torch.where(k4, gy, o64), torch.where(k4, gx, o64),
                       torch.where(k4, bx, z64), torch.where(k4, by, z64), torch.where(k4, bx, z64),
                       plan.range_plain[t, 0], plan.range_random[t, 0], plan.range_plain[t, 1], plan.range_random[t, 1]),
                      dim=1).to(torch.float32)                                      # rounded once
    flags = torch.stack((full, (k2 & ~tc) | (k3 & tc), (k2 & tc) | (k3 & ~tc), k4 & ~tc), dim=1)
    # ---- on the device of the split points ----
    i64, i32, f32, flags, t_d, LX_d = (x.to(dev) for x in (i64, i32.to(torch.int32), f32, flags, t, LX))
    multi = counts.to(dev)[t_d] > 1
    p = torch.where(multi, split_points[t_d].to(torch.int64), LX_d)                 # the split point, or len(X) for a single interval
    split_seg, shift, off_if_multi, plain_if_single = flags.unbind(dim=1)
    p32 = p.to(torch.int32)
    i32[:, 0] = torch.where(split_seg, p32, i32[:, 0])
    i32[:, 2] = torch.where(split_seg, LX_d.to(torch.int32) - p32, i32[:, 2])
    i64[:, 2] = torch.where(split_seg, i64[:, 0] + p, i64[:, 2])
    i64[:, 3] += torch.where(shift, p, torch.zeros_like(p))
    i64[:, 4] += torch.where(shift, p, torch.zeros_like(p))
    i32[:, 6] = torch.where(off_if_multi & multi, torch.full_like(p32, -1), i32[:, 6])
    i32[:, 7] = torch.where(plain_if_single & ~multi, torch.zeros_like(p32), i32[:, 7])
    return torch.cat((i64.contiguous().view(torch.uint8).view(m, -1), i32.contiguous().view(torch.uint8).view(m, -1),
                      f32.contiguous().view(torch.uint8).view(m, -1)), dim=1).contiguous()


def split_points(flat: torch.Tensor, regions: torch.Tensor, ratio: torch.Tensor, cap: int = 0):
    """vs_split_point: (count [B] int32, split [B] int32, intervals [B, cap, 2] int32 or None) on the device for the regions
    ``regions`` [B, 2] int64 = (at, n) of ``flat`` and ``ratio`` [B] float64 (host tensors; the library checks the regions on the
    host before it launches anything)."""
    if not flat.is_cuda:
        raise _lib.VoiceSplitHipError(f"the pool is on {flat.device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
    regions = regions.to(torch.int64).cpu().contiguous()
    ratio = ratio.to(torch.float64).cpu().contiguous()
    B = len(regions)
    if regions.shape != (B, 2) or ratio.shape != (B,) or B == 0:
        raise ValueError("split_points: regions [B, 2] and ratio [B], B > 0")
    dev = flat.device
    ws = torch.empty(_call.sized("split_workspace_bytes", max(int(regions[:, 1].max()), 0), B), dtype=torch.uint8, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    split = torch.empty(B, dtype=torch.int32, device=dev)
    intervals = torch.full((B, cap, 2), -1, dtype=torch.int32, device=dev) if cap > 0 else None
    regions_dev, ratio_dev = regions.to(dev), ratio.to(dev)
    _call.call("split_point", dev, flat, flat.numel(), regions, regions_dev, ratio_dev, B, count, split, intervals, int(cap),
               ws, ws.numel())
    return count, split, intervals


def mix_sequence(flat: torch.Tensor, noise: torch.Tensor, items: torch.Tensor, L: int, R: int, norm_in: Optional[torch.Tensor] = None,
                 rows: bool = True, invalid_count: Optional[torch.Tensor] = None):
    """vs_mix_sequence: (mixed_wav [B, L], target_wav [B, L], norm [B], aux [B, 8], valid [B] int32) for the ``vs_seq_item`` rows
    ``items`` [B, 136] uint8 on the device.  rows=False: the maximum only (mixed_wav and target_wav are None)."""
    if not flat.is_cuda:
        raise _lib.VoiceSplitHipError(f"the pool is on {flat.device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
    dev = flat.device
    if items.dtype != torch.uint8 or items.dim() != 2 or items.shape[1] != SEQ_ITEM_BYTES or items.device != dev or not items.is_contiguous():
        raise ValueError(f"items: expected a contiguous uint8 [B, {SEQ_ITEM_BYTES}] tensor on {dev}")
    if noise.device != dev or noise.dtype != torch.float32 or flat.dtype != torch.float32:
        raise ValueError(f"noise: expected a float32 buffer on {dev}")
    B = items.shape[0]
    if norm_in is not None and (norm_in.dtype != torch.float32 or norm_in.shape != (B,) or norm_in.device != dev or not norm_in.is_contiguous()):
        raise ValueError(f"norm_in: expected a contiguous float32 [{B}] tensor on {dev}")
    mixed = torch.empty(B, L, device=dev) if rows else None
    target = torch.empty(B, L, device=dev) if rows else None
    norm = torch.empty(B, device=dev)
    aux = torch.empty(B, 8, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _call.call("mix_sequence", dev, flat, flat.numel(), noise, noise.numel(), items, B, int(L), int(R), norm_in, mixed, target, norm,
               aux, valid, invalid_count)
    return mixed, target, norm, aux, valid


def pack_by_length(lengths: Sequence[int], groups: Sequence[int], batch: int, drop_last: bool = True) -> List[List[int]]:
    """Batches of ``batch`` item indices, every batch of one (length, group): the items are walked in order, a batch is emitted when
    its bucket is full, and what is left in a bucket at the end is dropped (``drop_last`` per length) or emitted as short batches."""
    buckets, out = {}, []
    for k, key in enumerate(zip(lengths, groups)):
        b = buckets.setdefault(key, [])
        b.append(k)
        if len(b) == batch:
            out.append(b)
            buckets[key] = []
    if not drop_last:
        out += [b for b in buckets.values() if b]
    return out


class OverlayBatches:
    """``BatchFeeder`` for the items without voice overlay: ``epoch(e)`` yields (emb, target, mixed, seq_len, target_wav, phase),
    every batch made on the device from a resident pool of voices and a second, untrimmed pool of noise recordings.

    triplets: (clean, reference, interferer) pool ids; ``shard.n`` must be their number.  Per epoch ``plan_overlay`` draws, drops
    what the reference drops (``dropped`` accumulates the counts) and expands into ``kinds``.  The training forward is not ragged, so
    a batch holds ``shard.b`` items of ONE output length (2 to 8 s with the default ``seconds``), packed in item order; kinds 2 and 3
    (which divide by their triplet's kind-1 norm) and kinds 1 and 4 are packed apart; incomplete batches are dropped per length.
    ``seq_len`` is that length.  emb_table: [N, emb_dim] on the pool's device, row = pool id of the reference clip.

    SEVERAL RANKS.  The number of batches depends on the draws, and every rank of a training job must see the same number (the step
    ends in a collective).  So every rank plans the WHOLE epoch alike -- the triplets of all ranks in the order of ``shard``'s global
    batches, one generator seeded by ``crop_seed(seed, epoch, 0)`` whatever the rank -- packs global batches of ``world * shard.b``
    items, and takes its own ``shard.b`` of each: the counts agree by construction, without a collective, and the union over the
    ranks of the k-th batches is the k-th global batch.  The same (seed, epoch) gives bit-identical batches.  The price: every rank
    computes the split points and kind-1 norms of all ranks' triplets (microseconds per thousand).

    Per epoch: one vs_split_point call for every kept triplet, the descriptor assembly (``overlay_items``), and maximum-only
    vs_mix_sequence calls for the kind-1 norms, all before the first batch; per batch: two gathers, vs_mix_sequence, the two
    front-end calls and the embedding gather -- no ``.item()``, no blocking copy.  What the kernel marks is counted on the device
    and reported once behind every epoch, also one that is abandoned early: ``invalid_items`` (valid == 0: all-zero items, rows of
    zeros) and ``refused_items`` (valid == -1: an index outside a buffer, which only a planner bug can produce)."""

    def __init__(self, pool: ClipPool, noise_pool: ClipPool, triplets: Sequence[Triplet], emb_table: torch.Tensor, audio_cfg, shard,
                 seed: int = 0, kinds: Sequence[int] = (1, 2, 3, 4), seconds: Sequence[int] = (2, 3, 4), batch: Optional[int] = None,
                 drop_last: bool = True):
        self.pool, self.noise_pool, self.acfg, self.shard, self.seed = pool, noise_pool, audio_cfg, shard, int(seed)
        self.drop_last = bool(drop_last)
        self.kinds, self.seconds = tuple(kinds), tuple(seconds)
        audio_cfg = resolve_audio(audio_cfg)
        self.sr, hop = int(audio_cfg["sample_rate"]), int(audio_cfg["hop_length"])
        if any(int(self.sr * s) % hop for s in self.seconds):
            raise ValueError(f"seconds {self.seconds} at {self.sr} Hz must be multiples of hop_length {hop}")
        self.triplets = [tuple(int(x) for x in t) for t in triplets]
        if shard is not None and shard.n != len(self.triplets):
            raise ValueError(f"the shard walks {shard.n} items, there are {len(self.triplets)} triplets")
        self.rank, self.world = (shard.rank, shard.world) if shard is not None else (0, 1)
        if self.world > 1 and not self.drop_last:
            raise ValueError("drop_last=False leaves short batches, whose number would differ between ranks: one rank only")
        self.batch = int(batch if batch is not None else shard.b)
        if emb_table.dim() != 2 or emb_table.shape[0] != len(pool) or emb_table.dtype != torch.float32:
            raise ValueError(f"emb_table: expected float32 [{len(pool)}, emb_dim], got {tuple(emb_table.shape)} {emb_table.dtype}")
        if pool.device is not None and (emb_table.device != pool.device or noise_pool.device != pool.device):
            raise ValueError(f"emb_table is on {emb_table.device}, the noise pool on {noise_pool.device}, the pool on {pool.device}")
        self.emb_table, self.device = emb_table, pool.device
        self._marked = None                                                        # [2] on the device: valid == 0, valid == -1
        self.invalid_items = self.refused_items = 0
        self.dropped = {k: 0 for k in OVERLAY_DROPS}

    # -- host ------------------------------------------------------------------------------------------------------------------------
    def global_positions(self, epoch: int) -> List[int]:
        """The triplets of ALL ranks for this epoch, global batch by global batch (the k-th ``shard.b`` of a global batch are rank
        k's): the same list on every rank."""
        from .trainer import EpochShard
        sh = self.shard
        whole = EpochShard(sh.n, sh.b * sh.world, 0, 1, sh.seed, sh.shuffle)
        return [p for b in whole.epoch(epoch) for p in b]

    def plan(self, positions: Sequence[int], epoch: int = 0) -> OverlayPlan:
        g = torch.Generator().manual_seed(crop_seed(self.seed, epoch, 0))          # the same on every rank
        return plan_overlay(self.pool, self.noise_pool, [self.triplets[p] for p in positions], self.sr, g, self.kinds, self.seconds)

    def rank_batches(self, plan: OverlayPlan, rank: Optional[int] = None) -> List[List[int]]:
        """This rank's batches as lists of item indices into ``plan``: its ``batch`` items of every global batch of ``world * batch``."""
        rank = self.rank if rank is None else int(rank)
        whole = pack_by_length(plan.item_len.tolist(), ((plan.item_kind == 2) | (plan.item_kind == 3)).tolist(), self.batch * self.world,
                               self.drop_last)
        return [b[rank * self.batch:(rank + 1) * self.batch] for b in whole]

    # -- device ----------------------------------------------------------------------------------------------------------------------
    def items(self, positions: Sequence[int], epoch: int = 0) -> Iterator[dict]:
        """One dict per batch of this rank for the triplets at ``positions`` (those of all ranks: ``global_positions``): the six
        tensors of ``epoch`` under their names plus ``mixed_wav``, ``norm``, ``aux``, ``valid``, ``desc`` (the batch's
        ``vs_seq_item`` rows), and on the host ``item_trip`` (index into ``plan.tri``) and ``item_kind``; ``plan`` itself too."""
        from . import audio
        if self.pool.flat is None or self.noise_pool.flat is None:
            raise _lib.VoiceSplitHipError("a pool holds no audio (ClipPool.planned): batches are made on an MI355X (HIP) device only")
        plan = self.plan([int(p) for p in positions], epoch)
        for k, v in plan.dropped.items():
            self.dropped[k] += v
        batches = self.rank_batches(plan) if len(plan.tri) else []
        if not batches:
            return
        dev, flat, noise = self.device, self.pool.flat, self.noise_pool.flat
        if self._marked is None:
            self._marked = torch.zeros(2, dtype=torch.int64, device=dev)
        count, split, _ = split_points(flat, plan.split_regions, plan.split_ratio)
        desc = overlay_items(plan, split, count)
        R = int((plan.Lc + plan.Li).max())
        norm1 = None
        if any(k in (2, 3) for k in self.kinds):                                   # every triplet's kind-1 norm, maximum only
            n = len(plan.tri)
            kind1 = overlay_items(plan, split, count, torch.arange(n), torch.ones(n, dtype=torch.int64))
            norm1 = torch.cat([mix_sequence(flat, noise, kind1[lo:lo + 65535], R, R, rows=False)[2] for lo in range(0, n, 65535)])
        order = torch.tensor([k for b in batches for k in b], dtype=torch.int64)
        order_dev = order.to(dev)                                                  # once per epoch
        trip_dev = plan.item_trip[order].to(dev)
        row_dev = plan.tri[plan.item_trip[order], 1].to(dev)
        lo = 0
        try:
            for b in batches:
                hi = lo + len(b)
                L = int(plan.item_len[b[0]])
                needs_norm = int(plan.item_kind[b[0]]) in (2, 3)
                norm_in = norm1.index_select(0, trip_dev[lo:hi]) if needs_norm else None
                rows = desc.index_select(0, order_dev[lo:hi])
                mixed_wav, target_wav, norm, aux, valid = mix_sequence(flat, noise, rows, L, R, norm_in)
                self._marked += torch.stack(((valid == 0).sum(), (valid == -1).sum()))
                mixed, phase = audio.wav_to_spec(mixed_wav, self.acfg, want_phase=True)
                target, _ = audio.wav_to_spec(target_wav, self.acfg, want_phase=False)
                emb = self.emb_table.index_select(0, row_dev[lo:hi])
                seq_len = torch.full((len(b),), L, dtype=torch.int64, device=dev)
                yield {"emb": emb, "target": target, "mixed": mixed, "seq_len": seq_len, "target_wav": target_wav, "phase": phase,
                       "mixed_wav": mixed_wav, "norm": norm, "aux": aux, "valid": valid, "desc": rows,
                       "item_trip": plan.item_trip[b], "item_kind": plan.item_kind[b], "plan": plan}
                lo = hi
        finally:
            self._report_marked()                                                  # also behind an epoch that is abandoned early

    def _report_marked(self):
        zero, refused = self._marked.tolist()                                      # once per epoch
        if zero > self.invalid_items:
            warnings.warn(f"{zero - self.invalid_items} items of this epoch were all zero: their rows are zero", RuntimeWarning)
        if refused > self.refused_items:
            warnings.warn(f"{refused - self.refused_items} items of this epoch had an index outside the voice or the noise buffer "
                          f"(valid == -1: a fault of the planner, not silence): their rows are zero", RuntimeWarning)
        self.invalid_items, self.refused_items = zero, refused

    def epoch(self, epoch: int):
        for it in self.items(self.global_positions(epoch), epoch):
            yield it["emb"], it["target"], it["mixed"], it["seq_len"], it["target_wav"], it["phase"]


# ---------------------------------------------------------------------------------------------
# the reference's on-disk dataset (preprocess_by_csv.py)
# ---------------------------------------------------------------------------------------------
def write_dataset(pool: ClipPool, triplets: Sequence[Triplet], numbers: Sequence[int], out_dir: str, audio_cfg, audio_len,
                  form=None, batch: int = 64, encoder=None, reverb: Optional[dict] = None) -> int:
    """What mix_wavfiles leaves in ``out_dir`` for every kept triplet, named by its CSV row number: ``*-mixed.wav``, ``*-target.wav``,
    ``*-emb.wav`` (float32 wavs), ``*-mixed.pt``, ``*-target.pt`` ([T, F] spectrograms), and with ``encoder`` ``*-emb.pt``.  Triplets
    with a too short clean or interferer clip leave no files, as in the reference.  Returns the number of triplets written.
    reverb: None, or the ``rir_pool`` / ``sir_db`` / ``history`` / ``target`` / ``seed`` arguments of ``MixtureBatches`` (epoch 0)."""
    import numpy as np
    from scipy.io import wavfile
    form = dict(DEFAULT_FORMAT, **(form or {}))
    L = samples_for(audio_cfg, audio_len)
    sr = int(audio_cfg["sample_rate"])
    keep = keep_mask(pool, triplets, L)
    kept = [t for t, k in zip(triplets, keep) if k]
    nums = [n for n, k in zip(numbers, keep) if k]
    if not kept:
        return 0
    os.makedirs(out_dir, exist_ok=True)
    if encoder is not None:
        refs = sorted({t[1] for t in kept})
        row_of = {r: k for k, r in enumerate(refs)}
        table = pool.embed(encoder, audio_cfg, refs, batch)
        has_emb = (table.abs().sum(dim=1) > 0).tolist()
        table = table.cpu()
    emb_table = torch.zeros(len(pool), 1, device=pool.device)                      # the writer does not use the yielded embedding
    mb = MixtureBatches(pool, kept, emb_table, audio_cfg, audio_len, None, crop="head", **(reverb or {}))
    batches = [list(range(lo, min(lo + batch, len(kept)))) for lo in range(0, len(kept), batch)]
    for it in mb.items(batches):
        host = {k: it[k].cpu() for k in ("mixed_wav", "target_wav", "mixed", "target")}
        for row, p in enumerate(it["positions"].tolist()):
            num, ref = nums[p], kept[p][1]
            wavfile.write(output_name(out_dir, form["mixed_wav"], num), sr, host["mixed_wav"][row].numpy().astype(np.float32))
            wavfile.write(output_name(out_dir, form["target_wav"], num), sr, host["target_wav"][row].numpy().astype(np.float32))
            wavfile.write(output_name(out_dir, form["emb_wav"], num), sr, pool.trimmed(ref).cpu().numpy().astype(np.float32))
            torch.save(host["mixed"][row].clone(), output_name(out_dir, form["mixed"], num))
            torch.save(host["target"][row].clone(), output_name(out_dir, form["target"], num))
            if encoder is not None:
                k = row_of[ref]
                torch.save(table[k].clone() if has_emb[k] else torch.zeros(1, dtype=torch.int64), output_name(out_dir, form["emb"], num))
    return len(kept)


def output_name_sub(out_dir: str, pattern: str, num: int, sub: int) -> str:
    """glob_re_to_filename(..., sub=k) (utils/generic_utils.py:347-349)."""
    return os.path.join(out_dir, pattern.replace("*", "%06d_%d" % (num, sub)))


def read_noise_csv(path: str, root: str) -> List[str]:
    """preprocess_by_csv_without_voice_overlay.py:69: one noise file per line (no header), relative to ``root``."""
    with open(path) as fh:
        names = [line.strip() for line in fh]
    paths = [os.path.join(root, n) for n in names if n]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing or not paths:
        raise FileNotFoundError(f"{path}: {len(missing)} of {len(paths)} noise files are missing" + (f", first {missing[0]}" if missing else ""))
    return paths


def write_overlay_dataset(pool: ClipPool, noise_pool: ClipPool, triplets: Sequence[Triplet], numbers: Sequence[int], out_dir: str,
                          audio_cfg, form=None, batch: int = 16, encoder=None, seed: int = 0, kinds: Sequence[int] = (1, 2, 3, 4),
                          seconds: Sequence[int] = (2, 3, 4)):
    """What mix_wavfiles_without_voice_overlay leaves in ``out_dir`` for every kept triplet, under the ``%06d_%d`` names of
    ``glob_re_to_filename(..., sub=kind)``: ``*-mixed.wav``, ``*-target.wav``, ``*-emb.wav`` (float32 wavs), ``*-mixed.pt``,
    ``*-target.pt`` ([T, F] spectrograms), and with ``encoder`` ``*-emb.pt``.  The emb wav is the trimmed reference utterance divided
    by the item's norm (:220), for sub 4 the min-max-scaled one (:33, :231).  The draws are those of ``plan_overlay`` under
    ``crop_seed(seed, 0, 0)``.  Returns (triplets written, the planner's drop counts)."""
    import numpy as np
    from scipy.io import wavfile
    form = dict(DEFAULT_FORMAT, **(form or {}))
    sr = int(audio_cfg["sample_rate"])
    os.makedirs(out_dir, exist_ok=True)
    emb_table = torch.zeros(len(pool), 1, device=pool.device)                      # the writer does not use the yielded embedding
    ob = OverlayBatches(pool, noise_pool, triplets, emb_table, audio_cfg, None, seed=seed, kinds=kinds, seconds=seconds, batch=batch,
                        drop_last=False)
    table = row_of = has_emb = None
    written, ref_audio = set(), {}
    for it in ob.items(range(len(triplets))):
        plan = it["plan"]
        if encoder is not None and table is None:
            refs = sorted(set(plan.tri[:, 1].tolist()))
            row_of = {r: k for k, r in enumerate(refs)}
            table = pool.embed(encoder, audio_cfg, refs, batch)
            has_emb = (table.abs().sum(dim=1) > 0).tolist()
            table = table.cpu()
        host = {k: it[k].cpu() for k in ("mixed_wav", "target_wav", "mixed", "target", "norm")}
        for row, (t, kind) in enumerate(zip(it["item_trip"].tolist(), it["item_kind"].tolist())):
            num, ref = numbers[int(plan.positions[t])], int(plan.tri[t, 1])
            written.add(num)
            if ref not in ref_audio:                                               # one device-to-host copy per reference clip
                ref_audio[ref] = pool.trimmed(ref).cpu().to(torch.float64)
            emb_audio = ref_audio[ref]
            if kind == 4:
                emb_audio = emb_audio * plan.gain[t, 0] + plan.bias[t, 0]
            norm = float(host["norm"][row])
            emb_audio = (emb_audio / norm if norm != 0 else torch.zeros_like(emb_audio)).to(torch.float32)
            name = lambda key: output_name_sub(out_dir, form[key], num, kind)
            wavfile.write(name("mixed_wav"), sr, host["mixed_wav"][row].numpy().astype(np.float32))
            wavfile.write(name("target_wav"), sr, host["target_wav"][row].numpy().astype(np.float32))
            wavfile.write(name("emb_wav"), sr, emb_audio.numpy())
            torch.save(host["mixed"][row].clone(), name("mixed"))
            torch.save(host["target"][row].clone(), name("target"))
            if encoder is not None:
                k = row_of[ref]
                torch.save(table[k].clone() if has_emb[k] else torch.zeros(1, dtype=torch.int64), name("emb"))
    return len(written), dict(ob.dropped)


def add_reverb_arguments(ap) -> None:
    ap.add_argument("--reverb-rooms", type=int, default=0, metavar="R", help="put the two talkers of every mixture in one of R random "
                    "shoebox rooms (image-method responses made on the device, two sources and one receiver per room)")
    ap.add_argument("--rt60", type=float, nargs=2, default=(0.15, 0.5), metavar=("LO", "HI"), help="--reverb-rooms: the rooms' "
                    "reverberation times in seconds, uniform in LO .. HI")
    ap.add_argument("--sir-db", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="scale the interferer so that the "
                    "target-to-interferer energy ratio of every mixture is uniform in LO .. HI dB")
    ap.add_argument("--reverb-csv", default=None, metavar="FILE", help="measured room responses instead of drawn rooms: one room per "
                    "line, two columns [target_response,interferer_response] (wav files of up to 32768 samples at the configured "
                    "rate; names relative to the CSV's directory); responses longer than 8192 taps need --reverb-math fft")
    ap.add_argument("--reverb-math", choices=("f16x3", "fp32", "fft"), default=None, help="the FIR's arithmetic (default f16x3, the "
                    "direct form on the matrix cores; fft: partitioned FFT convolution with kept spectra, responses of up to 32768 taps)")


def reverb_arguments(args, sample_rate: int, device, seed: int) -> Optional[dict]:
    """The ``MixtureBatches`` arguments of --reverb-rooms / --rt60 / --sir-db; None without them (the path that runs is then the
    one without reverberation, line for line)."""
    csv_path, math = getattr(args, "reverb_csv", None), getattr(args, "reverb_math", None)
    if not args.reverb_rooms and args.sir_db is None and not csv_path:
        return None
    out = {"sir_db": None if args.sir_db is None else tuple(args.sir_db), "seed": seed}
    if csv_path and args.reverb_rooms:
        raise ValueError("--reverb-csv and --reverb-rooms both name the pool of responses: give one")
    if args.reverb_rooms:
        from .reverb import RirPool
        out["rir_pool"] = RirPool(args.reverb_rooms, device, seed=seed, rt60=tuple(args.rt60), fs=sample_rate)
    if csv_path:
        from .reverb import RirPool
        out["rir_pool"] = RirPool.from_files(read_reverb_csv(csv_path), sample_rate, device)
    if math is not None:
        out["math"] = math
    return out


def read_reverb_csv(path: str):
    """The (target response, interferer response) file pairs of --reverb-csv; names are relative to the CSV's directory."""
    root = os.path.dirname(os.path.abspath(path))
    pairs = []
    with open(path, newline="") as f:
        for k, row in enumerate(csv.reader(f)):
            row = [c.strip() for c in row if c.strip()]
            if not row:
                continue
            if len(row) != 2:
                raise ValueError(f"{path}:{k + 1}: expected two columns [target_response,interferer_response], got {len(row)}")
            pairs.append(tuple(c if os.path.isabs(c) else os.path.join(root, c) for c in row))
    if not pairs:
        raise ValueError(f"{path}: no rooms")
    return pairs


def main(argv=None):
    from .config import load_config
    ap = argparse.ArgumentParser(description="Write the training / test triplet datasets of preprocess_by_csv.py, mixed on the GPU")
    ap.add_argument("-c", "--config", required=True, help="config.json")
    ap.add_argument("-r", "--dataset_root_dir", required=True, help="directory the CSV's names are relative to")
    ap.add_argument("-d", "--train_data_csv", default=None, help="rows [clean_utterance,embedding_utterance,interference_utterance]")
    ap.add_argument("-t", "--test_data_csv", default=None)
    ap.add_argument("-o", "--out_dir", required=True, help="output directory: train/ and test/ are made inside it")
    ap.add_argument("-l", "--librispeech", nargs="?", const=True, default=False, help="the CSV holds LibriSpeech utterance ids")
    ap.add_argument("--speaker-checkpoint", default=None, help="embedder.pt: also write *-emb.pt with the GE2E speaker encoder")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--resample", action="store_true", help="convert files at another rate to the configured one on the device "
                    "(librosa.load(path, sr=sample_rate)); without it such a file is an error")
    ap.add_argument("--normalize", nargs="?", type=float, const=-23.0, default=None, metavar="LUFS",
                    help="bring every utterance to this BS.1770 integrated loudness on the device first (default target -23; one "
                    "linear gain with a -2 dB peak cap, not ffmpeg's dynamic loudnorm); the noise recordings are left as they are")
    ap.add_argument("--no-overlay", action="store_true", help="preprocess_by_csv_without_voice_overlay.py: the speakers take turns "
                    "over two noise recordings, four items (%%06d_1 .. _4) per triplet; needs --noise-csv")
    ap.add_argument("--noise-csv", default=None, help="--no-overlay: one noise file per line, relative to the dataset root")
    ap.add_argument("--seed", type=int, default=0, help="--no-overlay, --reverb-rooms, --sir-db: seed of the draws")
    add_reverb_arguments(ap)
    args = ap.parse_args(argv)
    if args.no_overlay != bool(args.noise_csv):
        ap.error("--no-overlay and --noise-csv go together")
    if args.no_overlay and (args.reverb_rooms or args.sir_db or args.reverb_csv):
        ap.error("--reverb-rooms, --reverb-csv and --sir-db serve the overlaid mixtures only, not --no-overlay")
    c = load_config(args.config)
    audio_cfg = resolve_audio(c.audio)
    form = c.dataset["format"] if "dataset" in c and "format" in c.dataset else None
    encoder = None
    if args.speaker_checkpoint:
        from .speaker import SpeakerEncoder
        encoder = SpeakerEncoder(num_mels=int(audio_cfg.get("num_mels", 40)))
        encoder.load_state_dict(torch.load(args.speaker_checkpoint, map_location="cpu"), strict=True)
        encoder = encoder.eval().to(args.device)
    for name, path in (("train", args.train_data_csv), ("test", args.test_data_csv)):
        if not path:
            continue
        out = os.path.join(args.out_dir, name)
        os.makedirs(out, exist_ok=True)
        paths, triplets, numbers, skipped = read_triplet_csv(path, args.dataset_root_dir, bool(args.librispeech))
        written = 0
        if triplets and args.no_overlay:
            sr = int(audio_cfg["sample_rate"])
            pool = ClipPool.from_files(paths, sr, args.device, resample=args.resample, normalize=args.normalize)
            noise_pool = ClipPool.from_files(read_noise_csv(args.noise_csv, args.dataset_root_dir), sr, args.device, resample=args.resample,
                                             trim=False)
            written, dropped = write_overlay_dataset(pool, noise_pool, triplets, numbers, out, audio_cfg, form, args.batch, encoder, args.seed)
            print(f"{name}: {written} triplets written to {out} without voice overlay, dropped {dropped}, "
                  f"{skipped} skipped for a missing file")
            continue
        if triplets:
            pool = ClipPool.from_files(paths, int(audio_cfg["sample_rate"]), args.device, resample=args.resample, normalize=args.normalize)
            written = write_dataset(pool, triplets, numbers, out, audio_cfg, c.audio["audio_len"], form, args.batch, encoder,
                                    reverb_arguments(args, int(audio_cfg["sample_rate"]), args.device, args.seed))
        print(f"{name}: {written} triplets written to {out}, {len(triplets) - written} too short or silent, "
              f"{skipped} skipped for a missing file")


if __name__ == "__main__":
    main()
