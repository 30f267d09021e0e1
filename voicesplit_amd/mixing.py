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

from . import _lib
from .ops import _p, _stream

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

    def __init__(self, waveforms: Sequence[torch.Tensor], device="cuda:0"):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.VoiceSplitHipError(f"ClipPool on {device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
        if len(waveforms) == 0:
            raise ValueError("ClipPool: no clips")
        sizes = []
        for k, w in enumerate(waveforms):
            if w.dim() != 1 or w.dtype != torch.float32:
                raise ValueError(f"clip {k}: expected a 1-D float32 waveform, got {tuple(w.shape)} {w.dtype}")
            if w.numel() < MIN_CLIP:
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
        self._trim()

    @classmethod
    def from_files(cls, paths: Sequence[str], sample_rate: int, device="cuda:0", resample: bool = False) -> "ClipPool":
        """resample=False: every file must be at ``sample_rate`` (``load_wav`` raises otherwise).  resample=True: what
        ``librosa.load(path, sr=sample_rate)`` does -- the files are grouped by their own rate, every off-rate group is uploaded as it
        is and converted by one ``vs_resample_clips`` call straight into the pool's flat buffer, files at ``sample_rate`` are copied."""
        from .trainer import load_wav, load_wav_native
        if not resample:
            return cls([load_wav(p, sample_rate) for p in paths], device)
        from .resample import Resampler, out_len, plan
        loaded = [load_wav_native(p) for p in paths]
        plans = {sr: plan(sr, sample_rate) for sr in sorted({sr for _, sr in loaded})}
        # the pool's clips are the converted ones: lay them out first (ClipPool checks their sizes), then fill them group by group
        sizes = [out_len(plans[sr], w.numel()) for w, sr in loaded]
        self = cls.__new__(cls)
        self._layout(sizes, device)
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
        self._trim()
        return self

    def _layout(self, sizes: Sequence[int], device) -> None:
        """offsets / total / an uninitialised ``flat`` for clips of ``sizes`` samples."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.VoiceSplitHipError(f"ClipPool on {device}: this path only runs on an MI355X (HIP) device; there is no CPU fallback")
        if len(sizes) == 0:
            raise ValueError("ClipPool: no clips")
        for k, n in enumerate(sizes):
            if n < MIN_CLIP:
                raise ValueError(f"clip {k} has {n} samples, fewer than {MIN_CLIP}: silence trimming is not defined for it")
        self.device = device
        self.offsets = torch.zeros(len(sizes) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.tensor(list(sizes), dtype=torch.int64).cumsum(0)
        self.total = int(self.offsets[-1])
        self.flat = torch.empty(self.total, dtype=torch.float32, device=device)
        self.offsets_dev = self.offsets.to(device)

    @classmethod
    def planned(cls, lengths: Sequence[int], bounds: Sequence[Sequence[int]], peak: Optional[Sequence[float]] = None) -> "ClipPool":
        """A pool without audio: the per-clip numbers the host planner reads (dry runs, tests without a device)."""
        self = cls.__new__(cls)
        self.device, self.flat, self.offsets_dev = None, None, None
        self.offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.tensor(list(lengths), dtype=torch.int64).cumsum(0)
        self.total = int(self.offsets[-1])
        self.bounds = torch.tensor([list(b) for b in bounds], dtype=torch.int32).reshape(-1, 2)
        self.peak = torch.ones(len(lengths)) if peak is None else torch.tensor(list(peak), dtype=torch.float32)
        if not (len(self.bounds) == len(self.peak) == len(lengths)):
            raise ValueError("planned: lengths, bounds and peak must describe the same clips")
        return self

    def _trim(self):
        lib = _lib.load()
        n = len(self)
        nbytes = lib.vs_trim_workspace_bytes(self.total, n)
        if nbytes == 0:
            _lib.check(-1, "vs_trim_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        bounds = torch.empty(n, 2, dtype=torch.int32, device=self.device)
        peak = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = lib.vs_trim_bounds(_p(self.flat), self.total, _p(self.offsets), _p(self.offsets_dev), n, _p(bounds), _p(peak),
                                    _p(ws), ws.numel(), _stream())
        _lib.check(rc, "vs_trim_bounds")
        self.bounds, self.peak = bounds.cpu(), peak.cpu()

    def __len__(self) -> int:
        return self.offsets.numel() - 1

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
    lib = _lib.load()
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
    with torch.cuda.device(dev):
        rc = lib.vs_mix_clips(_p(flat), flat.numel(), _p(clean_at), _p(interf_at), B, int(L), _p(mixed), _p(target), _p(norm), _p(valid),
                              _p(invalid_count), _stream())
    _lib.check(rc, "vs_mix_clips")
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
    read once behind every epoch (``invalid_items``) and reported as a warning."""

    def __init__(self, pool: ClipPool, triplets: Sequence[Triplet], emb_table: torch.Tensor, audio_cfg, audio_len, shard,
                 crop: str = "head", seed: int = 0, emb_rows: str = "clip"):
        if crop not in ("head", "random"):
            raise ValueError(f"crop must be 'head' or 'random', got {crop!r}")
        if emb_rows not in ("clip", "triplet"):
            raise ValueError(f"emb_rows must be 'clip' or 'triplet', got {emb_rows!r}")
        self.pool, self.acfg, self.shard, self.crop, self.seed = pool, audio_cfg, shard, crop, int(seed)
        self.L = samples_for(audio_cfg, audio_len)
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
        for b in index_batches:
            hi = lo + len(b)
            mixed_wav, target_wav, norm, valid = mix_clips(self.pool.flat, at_dev[0, lo:hi], at_dev[1, lo:hi], self.L, self._invalid)
            mixed, phase = audio.wav_to_spec(mixed_wav, self.acfg, want_phase=True)
            target, _ = audio.wav_to_spec(target_wav, self.acfg, want_phase=False)
            emb = self.emb_table.index_select(0, row_dev[lo:hi])
            seq_len = torch.full((len(b),), self.L, dtype=torch.int64, device=self.device)
            yield {"emb": emb, "target": target, "mixed": mixed, "seq_len": seq_len, "target_wav": target_wav, "phase": phase,
                   "mixed_wav": mixed_wav, "norm": norm, "valid": valid, "positions": pos[lo:hi]}
            lo = hi
        self._report_invalid()

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
# the reference's on-disk dataset (preprocess_by_csv.py)
# ---------------------------------------------------------------------------------------------
def write_dataset(pool: ClipPool, triplets: Sequence[Triplet], numbers: Sequence[int], out_dir: str, audio_cfg, audio_len,
                  form=None, batch: int = 64, encoder=None) -> int:
    """What mix_wavfiles leaves in ``out_dir`` for every kept triplet, named by its CSV row number: ``*-mixed.wav``, ``*-target.wav``,
    ``*-emb.wav`` (float32 wavs), ``*-mixed.pt``, ``*-target.pt`` ([T, F] spectrograms), and with ``encoder`` ``*-emb.pt``.  Triplets
    with a too short clean or interferer clip leave no files, as in the reference.  Returns the number of triplets written."""
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
    mb = MixtureBatches(pool, kept, emb_table, audio_cfg, audio_len, None, crop="head")
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
    args = ap.parse_args(argv)
    c = load_config(args.config)
    audio_cfg = c.audio[c.audio["backend"]]
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
        if triplets:
            pool = ClipPool.from_files(paths, int(audio_cfg["sample_rate"]), args.device, resample=args.resample)
            written = write_dataset(pool, triplets, numbers, out, audio_cfg, c.audio["audio_len"], form, args.batch, encoder)
        print(f"{name}: {written} triplets written to {out}, {len(triplets) - written} too short or silent, "
              f"{skipped} skipped for a missing file")


if __name__ == "__main__":
    main()
