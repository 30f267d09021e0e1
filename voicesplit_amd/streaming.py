"""Long-form inference (BASELINE.json configs[4]): a clip longer than the 301-frame training window
is cut into windows that become items of one batch, the mask-prediction path runs once, and the
per-window masks are stitched back.  The reference only ever runs whole utterances through the
model (test.py feeds the full spectrogram, utils/generic_utils.py:533-546); windowing is what makes
a 30 s clip a data-parallel job: windows are independent, so they shard across GPUs with no
collective (voicesplit_amd/sharding.py).

halo = 0 reproduces BASELINE's "independent 301-frame windows" exactly.  halo > 0 gives every
window `halo` extra frames of context on both sides (65 covers the conv stack's 131-frame
receptive field) and keeps only the centre frames; in ``separate_long`` the BiLSTM still restarts
in every window.

``separate_long_exact`` is the variant that equals a whole-clip pass (what the reference computes,
utils/generic_utils.py:495 feeds any T): only the conv stack -- 95 % of the work and all of the
activation memory -- is windowed (halo >= 65: every kept frame sees its full receptive field, clip
edges are zero-padded exactly as the whole-clip convolution pads them), the stitched feature
sequence then goes through the BiLSTM and the head ONCE at full length, so the recurrent state is
carried across every window boundary in both directions by construction.

``StreamingMasker`` is the live form: frames arrive a few at a time and mask rows leave a bounded number of frames later (the
latency-controlled BiLSTM).  The conv stack is exact (every feature frame is computed once, from a window that gives it its full
receptive field or ends at a true stream edge), the forward LSTM direction carries its state from chunk to chunk and so is the
whole-stream recurrence, the reverse direction of a chunk of ``C`` frames starts from a zero state ``R`` look-ahead frames behind
the chunk's end.  With ``C + R`` at least the stream length it is the plain forward.
"""
from collections import namedtuple
from typing import Callable, List, Optional, Tuple

import torch

CONV_RECEPTIVE_HALO = 65      # (131 - 1) / 2 frames: 1 + 6 + 4*(1 + 2 + 4 + 8 + 16) = 131 (models/voicesplit/model.py:17-48)


def plan_windows(n_frames: int, window: int = 301, halo: int = 0) -> List[Tuple[int, int, int, int]]:
    """[(src_lo, src_hi, keep_lo, keep_hi)]: window w reads frames [src_lo, src_hi) of the clip
    (clipped to it; the rest of the `window` frames is zero padding) and contributes its local
    frames [keep_lo, keep_hi) to the output.  The kept spans tile [0, n_frames) exactly."""
    if n_frames <= 0:
        raise ValueError("n_frames must be positive")
    if window <= 2 * halo:
        raise ValueError("window must be larger than 2*halo")
    step = window - 2 * halo
    out = []
    start = 0
    while start < n_frames:
        src_lo = start - halo
        lo = max(src_lo, 0)
        hi = min(src_lo + window, n_frames)
        keep_lo = start - src_lo                      # == halo, also for the first window (left pad)
        keep_hi = min(keep_lo + step, hi - src_lo)
        out.append((lo, hi, keep_lo, keep_hi))
        start += step
    return out


def separate_long(model: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], spec: torch.Tensor,
                  dvec: torch.Tensor, window: int = 301, halo: int = 0, max_batch: int = 256) -> torch.Tensor:
    """mask [T_long, F] for one clip: spec [T_long, F] (same normalisation as training inputs),
    dvec [E].  `model` is the VoiceSplit/VoiceFilter module (or any (x[B,T,F], emb[B,E]) -> mask).
    Windows are processed `max_batch` at a time (BASELINE configs[4]: 256 windows per batch)."""
    if spec.dim() != 2 or dvec.dim() != 1:
        raise ValueError("spec must be [T, F] and dvec [E]")
    T_long, F = spec.shape
    plan = plan_windows(T_long, window, halo)
    batch = spec.new_zeros(len(plan), window, F)
    for w, (lo, hi, keep_lo, _) in enumerate(plan):
        dst = lo - (w * (window - 2 * halo) - halo)   # where frame `lo` lands inside the window
        batch[w, dst:dst + (hi - lo)] = spec[lo:hi]
    emb = dvec.unsqueeze(0)
    out = spec.new_empty(T_long, 0)
    pieces = []
    with torch.no_grad():
        for b0 in range(0, len(plan), max_batch):
            xb = batch[b0:b0 + max_batch].contiguous()
            mb = model(xb, emb.expand(xb.shape[0], -1).contiguous())
            pieces.append(mb)
    masks = torch.cat(pieces, dim=0)
    out = spec.new_empty(T_long, masks.shape[2])
    pos = 0
    for w, (_, _, keep_lo, keep_hi) in enumerate(plan):
        n = keep_hi - keep_lo
        out[pos:pos + n] = masks[w, keep_lo:keep_hi]
        pos += n
    assert pos == T_long
    return out



def separate_long_many(model: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], specs: torch.Tensor,
                       dvecs: torch.Tensor, window: int = 301, max_batch: int = 256) -> torch.Tensor:
    """BASELINE configs[4] as a batch job: specs [N, T_long, F] (N clips of equal length), dvecs [N, E] ->
    masks [N, T_long, F2].  Every clip is cut into independent `window`-frame items (the last one zero padded),
    the windows of ALL clips form one list that goes through the model `max_batch` at a time (256 windows per
    batch in the configuration), and the masks are cut back to T_long.  Same result as ``separate_long`` with
    halo = 0 clip by clip; it exists so that a batch never runs half empty at a clip boundary."""
    if specs.dim() != 3 or dvecs.dim() != 2 or specs.shape[0] != dvecs.shape[0]:
        raise ValueError("specs must be [N, T, F] and dvecs [N, E]")
    N, T_long, F = specs.shape
    nw = -(-T_long // window)
    pad = nw * window - T_long
    x = torch.nn.functional.pad(specs, (0, 0, 0, pad)) if pad else specs
    x = x.reshape(N * nw, window, F)
    emb = dvecs.unsqueeze(1).expand(N, nw, dvecs.shape[1]).reshape(N * nw, -1)
    out = None
    with torch.no_grad():
        for b0 in range(0, N * nw, max_batch):
            mb = model(x[b0:b0 + max_batch].contiguous(), emb[b0:b0 + max_batch].contiguous())
            if out is None:
                out = mb.new_empty(N * nw, window, mb.shape[2])
            out[b0:b0 + mb.shape[0]] = mb
    return out.reshape(N, nw * window, -1)[:, :T_long]


def plan_windows_exact(n_frames: int, window: int = 301, halo: int = CONV_RECEPTIVE_HALO) -> List[Tuple[int, int, int]]:
    """[(start, keep_lo, keep_hi)] for ``separate_long_exact``: every window lies INSIDE the clip (a frame
    outside the clip must stay a zero-padded activation in every conv layer, which a zero input frame
    inside a window is not: bias, BatchNorm shift and the activation make it non-zero after cnn1), the
    first starts at frame 0, the last ends at the last frame, interior windows advance by window - 2*halo.
    Window w covers frames [start, start + min(window, n_frames)) and contributes its local frames
    [keep_lo, keep_hi): at least `halo` frames away from every window edge that is not a clip edge."""
    if n_frames <= 0:
        raise ValueError("n_frames must be positive")
    if window <= 2 * halo:
        raise ValueError("window must be larger than 2*halo")
    if n_frames <= window:
        return [(0, 0, n_frames)]
    step = window - 2 * halo
    starts = [0]
    while starts[-1] + window < n_frames:
        starts.append(min(starts[-1] + step, n_frames - window))
    out, pos = [], 0
    for k, st in enumerate(starts):
        hi_abs = n_frames if k == len(starts) - 1 else st + window - halo
        out.append((st, pos - st, hi_abs - st))
        pos = hi_abs
    return out


def separate_long_exact(conv_stage: Callable[[torch.Tensor], torch.Tensor],
                        sequence_stage: Callable[[torch.Tensor, torch.Tensor], torch.Tensor],
                        spec: torch.Tensor, dvec: torch.Tensor, window: int = 301, halo: int = CONV_RECEPTIVE_HALO,
                        max_batch: int = 256) -> torch.Tensor:
    """mask [T_long, F2] equal to one whole-clip pass.  ``conv_stage(x[B,Tw,F]) -> feat[B,Tw,C]`` is the
    conv stack in eval mode (frame t of its output depends on input frames t-halo..t+halo only);
    ``sequence_stage(feat[1,T_long,C], dvec[1,E]) -> mask[1,T_long,F2]`` is everything behind it
    (d-vector concat, BiLSTM, head).  ``VoiceSplit.long_form_stages()`` returns the two for the HIP path."""
    if spec.dim() != 2 or dvec.dim() != 1:
        raise ValueError("spec must be [T, F] and dvec [E]")
    if halo < 0:
        raise ValueError("halo must be >= 0")
    T_long, F = spec.shape
    plan = plan_windows_exact(T_long, window, halo)
    wlen = min(window, T_long)
    batch = torch.stack([spec[st:st + wlen] for st, _k0, _k1 in plan])
    feats = []
    with torch.no_grad():
        for b0 in range(0, len(plan), max_batch):
            feats.append(conv_stage(batch[b0:b0 + max_batch].contiguous()))
        feat_w = torch.cat(feats, dim=0)
        full = feat_w.new_empty(1, T_long, feat_w.shape[2])
        pos = 0
        for w, (_st, keep_lo, keep_hi) in enumerate(plan):
            n = keep_hi - keep_lo
            full[0, pos:pos + n] = feat_w[w, keep_lo:keep_hi]
            pos += n
        assert pos == T_long
        return sequence_stage(full, dvec.unsqueeze(0).contiguous())[0]


def plan_ragged_batches(lengths, max_items: int, max_frames: int) -> List[List[int]]:
    """Batches for ``model.forward_ragged`` over clips of unequal length: lists of indices into ``lengths`` such that every
    index appears exactly once, no batch holds more than ``max_items`` clips and ``len(batch) * max(length in batch)`` -- the
    frames the padded batch occupies -- stays within ``max_frames``.  Clips are sorted by length (longest first, ties by index)
    and batches filled greedily, so batch mates differ little in length and few frames are padding.  A single clip longer
    than ``max_frames`` still gets a batch of its own.  Pure host arithmetic, deterministic."""
    if max_items < 1 or max_frames < 1:
        raise ValueError(f"plan_ragged_batches: max_items = {max_items} and max_frames = {max_frames} must be positive")
    lens = [int(n) for n in lengths]
    if any(n < 1 for n in lens):
        raise ValueError("plan_ragged_batches: every length must be at least 1")
    order = sorted(range(len(lens)), key=lambda i: (-lens[i], i))
    batches: List[List[int]] = []
    for i in order:
        cur = batches[-1] if batches else None
        # longest first: the batch's first clip is its Tmax, so one more clip costs exactly that many frames
        if cur is not None and len(cur) < max_items and (len(cur) + 1) * lens[cur[0]] <= max_frames:
            cur.append(i)
        else:
            batches.append([i])
    return batches


def padded_frame_share(lengths, batches) -> float:
    """Share of the frames of a plan's padded batches that is padding (0 = all clips of a batch share a length)."""
    lens = [int(n) for n in lengths]
    total = sum(len(b) * max(lens[i] for i in b) for b in batches)
    return 1.0 - sum(lens) / total if total else 0.0


# ---- a stream, chunk by chunk ---------------------------------------------------------------------------------------------
# feat_lo, feat_hi: the feature frames [feat_lo, feat_hi) that are finalised now; win_lo, win_hi: the input frames [win_lo, win_hi)
# the conv stack runs on for that (empty when no feature frame is due); chunks: [(k, lo, hi, e)] emitted now, in order -- chunk k
# keeps mask rows [lo, hi) and its recurrence runs over feature frames [lo, e)
StreamPlan = namedtuple("StreamPlan", "feat_lo feat_hi win_lo win_hi chunks")


def plan_stream(pushed: int, finished: bool, C: int, R: int, halo: int = CONV_RECEPTIVE_HALO,
                feat_done: int = 0, chunks_done: int = 0) -> StreamPlan:
    """What a stream of which ``pushed`` frames have arrived (``finished``: no more will) can do now, given that feature frames
    [0, feat_done) are final and chunks [0, chunks_done) are out.  Pure host arithmetic.

    Chunk k covers frames [kC, (k+1)C) and needs the features of [kC, (k+1)C + R); feature frame t is final once frame t + halo
    has arrived, so chunk k is due at exactly (k+1)C + R + halo pushed frames.  At the end of the stream everything is clipped
    to its length T = pushed and every remaining chunk is due.  Features are finalised when a chunk needs them, never twice:
    [feat_done, e of the last due chunk), from a conv window that starts ``halo`` frames earlier (or at frame 0) and ends
    ``halo`` frames later (or at the true end of the stream) -- always inside the stream, as in ``plan_windows_exact``."""
    if C < 1 or R < 0 or halo < 0:
        raise ValueError(f"plan_stream: C = {C} must be >= 1, R = {R} and halo = {halo} >= 0")
    if pushed < 0 or not 0 <= feat_done <= pushed or chunks_done < 0 or chunks_done * C > feat_done:
        raise ValueError(f"plan_stream: inconsistent state pushed = {pushed}, feat_done = {feat_done}, chunks_done = {chunks_done}")
    due = -(-pushed // C) if finished else max(0, (pushed - R - halo) // C)
    chunks = []
    for k in range(chunks_done, due):
        hi, e = (k + 1) * C, (k + 1) * C + R
        chunks.append((k, k * C, min(hi, pushed), min(e, pushed)) if finished else (k, k * C, hi, e))
    feat_hi = max(feat_done, chunks[-1][3]) if chunks else feat_done
    if feat_hi == feat_done:
        return StreamPlan(feat_done, feat_done, feat_done, feat_done, chunks)
    return StreamPlan(feat_done, feat_hi, max(0, feat_done - halo), pushed if finished else feat_hi + halo, chunks)


class StreamingMasker:
    """Masks of ``B`` streams that advance in lockstep, emitted chunk by chunk.

    ``conv_stage(x [B, Tw, F]) -> feat [B, Tw, Cf]`` is the eval-mode conv stack, ``carry_stage(feat [B, n, Cf], dvec [B, E],
    state or None, keep) -> (lstm_out [B, n, 2H], state)`` the sequence stage whose forward direction starts from ``state``
    (None: zero) and returns its state behind frame ``keep - 1``, ``head_stage(lstm_out [B, n, 2H]) -> mask [B, n, F2]`` (or
    ``(mask, logits)``) the head.  ``VoiceSplit.stream_stages()`` returns the HIP ones.  The d-vectors are fixed for the life of
    the object.  ``push(frames [B, n, F])`` returns the mask rows that became due, [B, m, F2] with m >= 0 a multiple of ``C``;
    ``finish()`` returns the rest.  Kept between calls: the input frames the next conv window needs, the finalised features of the
    chunks not yet out, the forward state.  ``trace=True`` keeps every chunk's ``lstm_out`` rows (and logits) in ``self.trace``.

    Several enrolled speakers per stream: ``dvec [B, K, E]``.  Input frames, conv windows, finalised features and the plan stay per
    mixture (one conv window per arrival, whatever K); ``carry_stage`` is given the 3-D d-vectors and returns ``lstm_out [B, K, n,
    2H]`` with the state of the B*K sequences ``[B*K, 2, H]``, ``head_stage`` takes ``[B, K, n, 2H]`` and returns ``[B, K, n, F2]``,
    and ``push`` / ``finish`` return ``[B, K, m, F2]``; trace rows carry the K axis.  Emission times and ``latency_frames`` are those
    of one speaker.
    """

    def __init__(self, conv_stage: Callable, carry_stage: Callable, head_stage: Callable, dvec: torch.Tensor, C: int, R: int,
                 halo: int = CONV_RECEPTIVE_HALO, trace: bool = False):
        if dvec.dim() not in (2, 3) or 0 in dvec.shape:
            raise ValueError(f"dvec must be [B, E], or [B, K, E] with K >= 1 speakers per stream, got {tuple(dvec.shape)}")
        plan_stream(0, False, C, R, halo)                      # range checks
        self.conv_stage, self.carry_stage, self.head_stage = conv_stage, carry_stage, head_stage
        self.dvec = dvec.contiguous()
        self.K = int(dvec.shape[1]) if dvec.dim() == 3 else None      # None: one speaker per stream, outputs without a K axis
        self._tdim = 1 if self.K is None else 2                        # the time axis of lstm_out and of the masks
        self.C, self.R, self.halo = int(C), int(R), int(halo)
        self.pushed = self.feat_done = self.chunks_done = 0
        self.finished = False
        self.trace = [] if trace else None
        self._x = None          # input frames [_x0, pushed)
        self._x0 = 0
        self._feat = None       # final features [_f0, feat_done)
        self._f0 = 0
        self._state = None
        self._out_dim = None

    @property
    def latency_frames(self) -> int:
        """Mask row t is returned by the push that brings the number of pushed frames to (t // C + 1) * C + R + halo <= t +
        latency_frames, or by ``finish()``."""
        return self.C + self.R + self.halo

    @property
    def emitted(self) -> int:
        return min(self.chunks_done * self.C, self.pushed)

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingMasker: the stream has been finished")
        if frames.dim() != 3 or frames.shape[0] != self.dvec.shape[0]:
            raise ValueError(f"frames must be [B = {self.dvec.shape[0]}, n, F], got {tuple(frames.shape)}")
        if self._x is not None and frames.shape[2] != self._x.shape[2]:
            raise ValueError(f"frames have {frames.shape[2]} bins, the stream has {self._x.shape[2]}")
        self._x = frames if self._x is None else torch.cat((self._x, frames), dim=1)
        self.pushed += frames.shape[1]
        return self._advance()

    def finish(self) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("StreamingMasker: the stream has been finished")
        if self._x is None:
            raise RuntimeError("StreamingMasker: finish() on a stream that never received a frame")
        self.finished = True
        return self._advance()

    def _advance(self) -> torch.Tensor:
        plan = plan_stream(self.pushed, self.finished, self.C, self.R, self.halo, self.feat_done, self.chunks_done)
        pieces = []
        with torch.no_grad():
            if plan.feat_hi > plan.feat_lo:
                window = self._x[:, plan.win_lo - self._x0:plan.win_hi - self._x0].contiguous()
                new = self.conv_stage(window)[:, plan.feat_lo - plan.win_lo:plan.feat_hi - plan.win_lo]
                self._feat = new if self._feat is None or self._feat.shape[1] == 0 else torch.cat((self._feat, new), dim=1)
                self.feat_done = plan.feat_hi
                keep_from = max(0, self.feat_done - self.halo)          # left edge of the next conv window
                self._x, self._x0 = self._x[:, keep_from - self._x0:], keep_from
            for k, lo, hi, e in plan.chunks:
                seg = self._feat[:, lo - self._f0:e - self._f0].contiguous()
                lstm_out, self._state = self.carry_stage(seg, self.dvec, self._state, hi - lo)
                rows = lstm_out.narrow(self._tdim, 0, hi - lo).contiguous()
                out = self.head_stage(rows)
                mask, logits = out if isinstance(out, tuple) else (out, None)
                if self.trace is not None:
                    self.trace.append({"chunk": k, "lo": lo, "hi": hi, "e": e, "lstm_out": rows, "logits": logits})
                pieces.append(mask)
                self._out_dim = mask.shape[-1]
                self._feat, self._f0 = self._feat[:, hi - self._f0:], hi
                self.chunks_done = k + 1
        if pieces:
            return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=self._tdim)
        lead = (self._x.shape[0],) if self.K is None else (self._x.shape[0], self.K)
        return self._x.new_empty(*lead, 0, self._out_dim if self._out_dim is not None else self._x.shape[2])
