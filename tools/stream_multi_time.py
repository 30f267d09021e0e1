#!/usr/bin/env python3
"""Times K enrolled speakers streamed from one live mixture (streaming.StreamingMasker with d-vectors [B, K, E] on the HIP stages)
against K single-speaker maskers, at full width, one process.

A stream of --frames frames (10 ms each) arrives C = 16 frames at a time, R = 32, for B in {1, 16}, K in {2, 4}, in both
arithmetics.  At every arrival two arms are timed with device events, alternating:

  multi   : ``masker.push(the C new frames)`` of ONE K-speaker masker -- one conv window of C + 2 x 65 frames and one LSTM input
            GEMM per mixture, the carry x shared-input recurrence over the B*K sequences, the head over B*K*C rows.
  singles : the same push into K single-speaker maskers, one after the other inside one pair of events -- K conv windows, K input
            GEMMs, K carry recurrences over B sequences, K heads over B*C rows.

Only arrivals that emit a chunk count (the first (R + 65) / C do not).  One pass = one whole stream; the figure of a pass is the
mean over its emitting arrivals (the same arrivals for both arms).  Pass 0 warms every shape up and is dropped; the medians, minima
and maxima of the other --passes passes are written.  Both arms derive their weights per call, as every stage entry point does (a
prepared-weights form of the stream stages is not built), so both carry that cost -- K times in the singles arm.

The per-stage split of the multi arm (conv window, carry stage, head) comes from passes of their own, with device events around
every stage call; their sum is not the arm's figure (host work between the stages is outside the events).

    python tools/stream_multi_time.py [--out profiles/stream_multi_time.json] [--passes 5] [--frames 601]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_MS = 10.0          # hop_length 160 at 16 kHz
C_CHUNK = 16
R_LOOKAHEAD = 32
STAGES = ("conv_window", "carry_stage", "head")


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def one_pass(model, x, dvecs, C, R):
    """-> (multi ms, singles ms) per emitting arrival, number of emitting arrivals."""
    from voicesplit_amd.streaming import StreamingMasker
    K = dvecs.shape[1]
    multi = StreamingMasker(*model.stream_stages(), dvecs, C, R)
    singles = [StreamingMasker(*model.stream_stages(), dvecs[:, k].contiguous(), C, R) for k in range(K)]
    t_multi, t_singles = [], []
    for pos in range(0, x.shape[1], C):
        frames = x[:, pos:pos + C].contiguous()
        ms_m, rows = device_ms(lambda: multi.push(frames))
        ms_s, each = device_ms(lambda: [s.push(frames) for s in singles])
        assert all(e.shape[1] == rows.shape[2] for e in each)
        if rows.shape[2]:
            t_multi.append(ms_m)
            t_singles.append(ms_s)
    multi.finish()
    for s in singles:
        s.finish()
    torch.cuda.synchronize()
    return sum(t_multi) / len(t_multi), sum(t_singles) / len(t_singles), len(t_multi)


def split_pass(model, x, dvecs, C, R):
    """-> {stage: ms per emitting arrival} of the K-speaker masker, device events around every stage call (pushes only)."""
    from voicesplit_amd.streaming import StreamingMasker
    marks = {s: [] for s in STAGES}

    def timed(name, fn):
        def run(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(*args)
            b.record()
            marks[name].append((a, b))
            return out
        return run

    masker = StreamingMasker(*(timed(n, f) for n, f in zip(STAGES, model.stream_stages())), dvecs, C, R)
    emitting = 0
    for pos in range(0, x.shape[1], C):
        emitting += bool(masker.push(x[:, pos:pos + C].contiguous()).shape[2])
    torch.cuda.synchronize()
    out = {s: sum(a.elapsed_time(b) for a, b in marks[s]) / emitting for s in STAGES}
    masker.finish()
    torch.cuda.synchronize()
    return out


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_multi_time.json"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=601)
    args = ap.parse_args()
    if args.passes < 5:
        ap.error("--passes: at least 5")
    if not torch.cuda.is_available():
        sys.exit("stream_multi_time: needs an MI355X; nothing is measured without one")
    import voicesplit_amd as V
    from voicesplit_amd import ops
    dev = "cuda:0"
    torch.manual_seed(0)
    model = V.VoiceSplit(V.default_config()).eval().to(dev)
    result = {"device": torch.cuda.get_device_name(0), "stream_frames": args.frames, "frame_ms": FRAME_MS, "C": C_CHUNK, "R": R_LOOKAHEAD,
              "passes": args.passes, "weights": "derived per call in both arms (no prepared-weights form of the stream stages)",
              "arms": {"multi": "one K-speaker masker", "singles": "K single-speaker maskers advanced at the same arrivals"},
              "cases": []}
    prev = ops.get_conv_math()
    try:
        for math in ("f16x3", "bf16"):
            ops.set_conv_math(math)
            for B in (1, 16):
                for K in (2, 4):
                    g = torch.Generator().manual_seed(100 * B + K)
                    x = torch.rand(B, args.frames, 601, generator=g).to(dev)
                    dvecs = torch.nn.functional.normalize(torch.randn(B, K, 256, generator=g), dim=2).to(dev)
                    with torch.no_grad():
                        runs = [one_pass(model, x, dvecs, C_CHUNK, R_LOOKAHEAD) for _ in range(args.passes + 1)][1:]
                        splits = [split_pass(model, x, dvecs, C_CHUNK, R_LOOKAHEAD) for _ in range(args.passes + 1)][1:]
                    multi, singles = stats([r[0] for r in runs]), stats([r[1] for r in runs])
                    case = {"math": math, "B": B, "K": K, "chunk_audio_ms": C_CHUNK * FRAME_MS,
                            "latency_frames": C_CHUNK + R_LOOKAHEAD + 65, "emitting_arrivals": runs[0][2],
                            "multi_per_chunk": multi, "singles_per_chunk": singles,
                            "singles_over_multi_of_medians": singles["median_ms"] / multi["median_ms"],
                            "multi_stage_split": {s: stats([sp[s] for sp in splits]) for s in STAGES}}
                    result["cases"].append(case)
                    print(json.dumps(case), flush=True)
    finally:
        ops.set_conv_math(prev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
