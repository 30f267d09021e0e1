#!/usr/bin/env python3
"""Times stream separation chunk by chunk (streaming.StreamingMasker on the HIP stages) at full width, one process.

A stream of --frames frames (10 ms each) arrives C frames at a time, for B in {1, 16}, C in {16, 50, 100}, R = 32, in both
arithmetics.  At every arrival two things are timed with device events, alternating:

  stream : ``masker.push(the C new frames)`` -- a conv window of C + 2 x 65 frames, the carry recurrence over C + R frames, the
           head over C rows.  Only arrivals that emit a chunk count (the first (R + 65) / C do not).
  rerun  : ``model(everything received so far)`` -- what a caller without a carried state has to do to get the same rows with
           the forward LSTM direction intact; its cost grows with the stream.

One pass = one whole stream; the figure of a pass is the mean over its emitting arrivals (the same arrivals for both arms).
Pass 0 warms every shape up and is dropped; the medians, minima and maxima of the other --passes passes are written, next to the
audio a chunk holds and the rerun's time at the last arrival.

    python tools/stream_time.py [--out profiles/stream_time.json] [--passes 5] [--frames 601]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_MS = 10.0          # hop_length 160 at 16 kHz
R_LOOKAHEAD = 32


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def one_pass(model, x, dvec, C, R):
    from voicesplit_amd.streaming import StreamingMasker
    masker = StreamingMasker(*model.stream_stages(), dvec, C, R)
    stream, rerun, last = [], [], None
    for pos in range(0, x.shape[1], C):
        frames = x[:, pos:pos + C].contiguous()
        ms, rows = device_ms(lambda: masker.push(frames))
        so_far = x[:, :pos + frames.shape[1]].contiguous()
        ms_b, _ = device_ms(lambda: model(so_far, dvec))
        last = ms_b
        if rows.shape[1]:
            stream.append(ms)
            rerun.append(ms_b)
    masker.finish()
    torch.cuda.synchronize()
    return sum(stream) / len(stream), sum(rerun) / len(rerun), last, len(stream)


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_time.json"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=601)
    args = ap.parse_args()
    if args.passes < 5:
        ap.error("--passes: at least 5")
    if not torch.cuda.is_available():
        sys.exit("stream_time: needs an MI355X; nothing is measured without one")
    import voicesplit_amd as V
    from voicesplit_amd import ops
    dev = "cuda:0"
    torch.manual_seed(0)
    model = V.VoiceSplit(V.default_config()).eval().to(dev)
    result = {"device": torch.cuda.get_device_name(0), "stream_frames": args.frames, "frame_ms": FRAME_MS, "R": R_LOOKAHEAD,
              "passes": args.passes, "cases": []}
    prev = ops.get_conv_math()
    try:
        for math in ("f16x3", "bf16"):
            ops.set_conv_math(math)
            for B in (1, 16):
                g = torch.Generator().manual_seed(B)
                x = torch.rand(B, args.frames, 601, generator=g).to(dev)
                dvec = torch.nn.functional.normalize(torch.randn(B, 256, generator=g), dim=1).to(dev)
                for C in (16, 50, 100):
                    with torch.no_grad():
                        runs = [one_pass(model, x, dvec, C, R_LOOKAHEAD) for _ in range(args.passes + 1)][1:]
                    case = {"math": math, "B": B, "C": C, "chunk_audio_ms": C * FRAME_MS,
                            "latency_frames": C + R_LOOKAHEAD + 65, "emitting_arrivals": runs[0][3],
                            "stream_per_chunk": stats([r[0] for r in runs]),
                            "rerun_model_per_chunk": stats([r[1] for r in runs]),
                            "rerun_model_at_last_arrival": stats([r[2] for r in runs])}
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
