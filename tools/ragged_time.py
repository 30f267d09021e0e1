"""Time of an eval pass over clips of unequal length, three ways, alternated inside one process per arithmetic:

  (a) one_by_one  the B = 1 loop ``model(x_b, emb_b)`` over every clip -- the only correct way before ``forward_ragged``;
  (b) ragged      ``model.forward_ragged`` on the batches of ``streaming.plan_ragged_batches``;
  (c) padded      the same batches, zero padded to their Tmax, through plain ``model(x, emb)``: WRONG masks (every layer reads the pad);
                  timed only as the floor of what (b) could cost without its tail sweeps (and as the ceiling that skipping tail row
                  groups in the convs would have to beat).

    python tools/ragged_time.py [--clips 64] [--reps 5] [--max-items 16] [--out profiles/ragged_time.json]

64 clips with the demo set's spread of lengths (531 .. 1142 frames, fixed seed), full-width model.  Each arithmetic (f16x3, bf16) runs
in a child process of its own under a time limit; the first failure ends the run.  Inside a child every shape is warmed up first, then
each repetition times (a), (b), (c) in turn with device events around the whole pass: the spread over repetitions of the SAME arm is
reported next to the medians, so a difference between arms can be judged against it.  One JSON line per arithmetic on stdout.
"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _child(args):
    import numpy as np
    import torch
    import voicesplit_amd as V
    from voicesplit_amd import audio, ops
    from voicesplit_amd.streaming import padded_frame_share, plan_ragged_batches
    if not torch.cuda.is_available():
        raise SystemExit("ragged_time.py measures the GPU: no device here")
    ops.set_conv_math(args.child)
    rng = random.Random(args.seed)
    lengths = [rng.randint(531, 1142) for _ in range(args.clips)]
    g = torch.Generator().manual_seed(args.seed)
    torch.manual_seed(args.seed)
    m = V.VoiceSplit(V.default_config()).cuda().eval()
    F, E = 601, 256
    specs = [torch.rand(n, F, generator=g).cuda() for n in lengths]
    dvec = torch.randn(args.clips, E, generator=g).cuda()
    plan = plan_ragged_batches(lengths, args.max_items, args.max_items * 1142)
    batches = []
    for b in plan:
        x, lens = audio.pad_specs([specs[i] for i in b])
        batches.append((x, dvec[b].contiguous(), lens))
    singles = [(specs[i][None].contiguous(), dvec[i:i + 1].contiguous()) for i in range(args.clips)]

    def one_by_one():
        for x, e in singles:
            m(x, e)

    def ragged():
        for x, e, lens in batches:
            m.forward_ragged(x, e, lens)

    def padded():
        for x, e, _ in batches:
            m(x, e)

    arms = {"one_by_one": one_by_one, "ragged": ragged, "padded": padded}
    ms = {k: [] for k in arms}
    with torch.no_grad():
        for fn in arms.values():              # every shape of the timed window, twice
            fn()
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        # what was timed is what is right: one clip of the last batch against its B = 1 result
        x, e, lens = batches[-1]
        got = m.forward_ragged(x, e, lens)[0, :lens[0]]
        want = m(x[0:1, :lens[0]].contiguous(), e[0:1])[0]
        check = float((got - want).abs().max())
    row = {"math": args.child, "device": torch.cuda.get_device_name(0), "clips": args.clips, "frames": sum(lengths),
           "batches": len(plan), "max_items": args.max_items, "padded_frame_share": padded_frame_share(lengths, plan), "reps": args.reps,
           "max_abs_ragged_vs_one_by_one_mask": check}
    for k, v in ms.items():
        row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = float(np.median(v)), float(np.min(v)), float(np.max(v))
    row["speedup_ragged_over_one_by_one"] = row["one_by_one_ms_median"] / row["ragged_ms_median"]
    row["ragged_over_padded"] = row["ragged_ms_median"] / row["padded_ms_median"]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-items", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one arithmetic's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return _child(args)
    rows = []
    for math in ("f16x3", "bf16"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", math, "--clips", str(args.clips), "--reps", str(args.reps),
               "--max-items", str(args.max_items), "--seed", str(args.seed)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"ragged_time.py: the {math} step ran into its time limit of {args.step_timeout} s; nothing further is started")
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"ragged_time.py: the {math} step failed with status {p.returncode}; nothing further is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"arms": rows}, f, indent=1)


if __name__ == "__main__":
    main()
