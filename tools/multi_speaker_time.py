"""Time of K enrolled speakers out of the same mixtures, two ways, alternated inside one process per arithmetic:

  (a) plain  K calls ``model(x, emb_k)`` -- the conv stack and the LSTM input GEMM K times over;
  (b) multi  one ``model.forward_multi(x, emb[B, K, E])`` -- conv stack and input GEMM once, recurrence and head over B*K sequences.

    python tools/multi_speaker_time.py [--reps 9] [--out profiles/multi_speaker_time.json]

Full-width model, T = 301, B in {1, 64}, K in {2, 4, 8}.  Each arithmetic (f16x3, bf16) runs in a child process of its own under a time
limit; the first failure ends the run.  Inside a child every (B, K) is warmed up first (both arms, twice), then each repetition times
(a) and (b) in turn with device events around the whole arm; medians with the spread over repetitions of the SAME arm, so a difference
between arms can be judged against it.  Per (B, K) also the library's own stage timers for one multi call and one plain call
(``vs_profile_begin``: ms per call of conv stack, input GEMM, recurrence, head), taken outside the timed repetitions.  One JSON line
per arithmetic on stdout.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, F, E = 301, 601, 256
BATCHES = (1, 64)
SPEAKERS = (2, 4, 8)


def _stage_ms(lib, _lib, fn, calls):
    """ms per call of fn by the library's stage timers: conv (cnn1..cnn8), lstm_gemm, lstm_rec, head."""
    import torch
    _lib.check(lib.vs_profile_begin(calls), "vs_profile_begin")
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    ms = (ctypes.c_float * _lib.PROF_SLOTS)()
    n = (ctypes.c_int * _lib.PROF_SLOTS)()
    _lib.check(lib.vs_profile_end(ms, n), "vs_profile_end")
    slot = dict(zip(_lib.PROF_NAMES, ms))
    out = {"conv": sum(slot[f"cnn{i}"] for i in range(1, 9))}
    out.update({k: slot[k] for k in ("lstm_gemm", "lstm_rec", "head")})
    return {k: round(v / calls, 4) for k, v in out.items()}


def _child(args):
    import numpy as np
    import torch
    import voicesplit_amd as V
    from voicesplit_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("multi_speaker_time.py measures the GPU: no device here")
    ops.set_conv_math(args.child)
    lib = _lib.load()
    torch.manual_seed(args.seed)
    g = torch.Generator().manual_seed(args.seed)
    m = V.VoiceSplit(V.default_config()).cuda().eval()
    rows = []
    with torch.no_grad():
        for B in BATCHES:
            x = torch.rand(B, T, F, generator=g).cuda()
            for K in SPEAKERS:
                emb = torch.randn(B, K, E, generator=g)
                emb = (emb / emb.norm(dim=2, keepdim=True)).cuda()
                each = [emb[:, k].contiguous() for k in range(K)]

                def plain():
                    return [m(x, e) for e in each]

                def multi():
                    return m.forward_multi(x, emb)

                arms = {"plain": plain, "multi": multi}
                ms = {k: [] for k in arms}
                for fn in arms.values():
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
                # what was timed is what is right: the two arms' masks side by side
                check = float(max((multi()[:, k] - p).abs().max() for k, p in enumerate(plain())))
                row = {"B": B, "K": K, "T": T, "max_abs_multi_vs_plain_mask": check,
                       "stage_ms_multi": _stage_ms(lib, _lib, multi, 3), "stage_ms_one_plain_call": _stage_ms(lib, _lib, lambda: m(x, each[0]), 3)}
                for k, v in ms.items():
                    row[k + "_ms_median"], row[k + "_ms_min"], row[k + "_ms_max"] = float(np.median(v)), float(np.min(v)), float(np.max(v))
                row["plain_over_multi"] = row["plain_ms_median"] / row["multi_ms_median"]
                row["ms_per_extra_speaker"] = (row["multi_ms_median"] - row["plain_ms_median"] / K) / (K - 1)
                rows.append(row)
            ops.release_workspaces()
    print(json.dumps({"math": args.child, "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one arithmetic's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return _child(args)
    arms = []
    for math in ("f16x3", "bf16"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", math, "--reps", str(args.reps), "--seed", str(args.seed)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"multi_speaker_time.py: the {math} step ran into its time limit of {args.step_timeout} s; nothing further is started")
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"multi_speaker_time.py: the {math} step failed with status {p.returncode}; nothing further is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        arms.append(json.loads(line))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"arms": arms}, f, indent=1)


if __name__ == "__main__":
    main()
