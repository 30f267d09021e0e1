"""Time of metrics.stoi (vs_stoi) on the GPU, from device events after warm-up: STOI and ESTOI of B = 64 clips of 3 s, given at
16 kHz (both signals through the cached resampler first) and given at 10 kHz (no resampling), next to metrics.bss_sdr on the same
16 kHz batch for scale and to the fp64 host restatement (tests/stoi_ref.py, form 1) on ONE clip.

    python tools/stoi_time.py [--reps 20] [--out profiles/stoi_time.json]     (one JSON line per arm on stdout)

The five GPU arms alternate inside one process, rep by rep; the median of the reps with its minimum and maximum is reported.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _spread(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def main():
    import stoi_ref as SR
    from voicesplit_amd import metrics
    from voicesplit_amd.resample import Resampler
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=48000, help="samples per clip at 16 kHz")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stoi_time.py measures the GPU: no device here")
    B, N = args.B, args.N
    base = [SR.speech(N, (N // 3, N // 2), s) for s in range(4)]            # four synthetic utterances with a silent gap, cycled
    x = np.stack([np.roll(base[b % 4], 997 * (b // 4)) for b in range(B)])
    y = np.stack([SR.noisy(x[b], 5.0, b) for b in range(B)])
    x16, y16 = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    rs = Resampler(16000, 10000, x16.device)
    x10, y10 = rs(x16), rs(y16)
    arms = {
        "stoi_16k": lambda: metrics.stoi(x16, y16, 16000),
        "estoi_16k": lambda: metrics.stoi(x16, y16, 16000, extended=True),
        "stoi_10k": lambda: metrics.stoi(x10, y10, 10000),
        "estoi_10k": lambda: metrics.stoi(x10, y10, 10000, extended=True),
        "bss_sdr_16k": lambda: metrics.bss_sdr(x16, y16),
    }
    for _ in range(3):
        out = {name: fn() for name, fn in arms.items()}
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(args.reps):
        for name, fn in arms.items():
            ms[name].append(_timed(fn))
    # the host restatement on one clip, fed the device's own 10 kHz signals so that the numbers can be compared
    x0, y0 = x10[0].cpu().numpy(), y10[0].cpu().numpy()
    host = {}
    for name, extended in (("stoi", False), ("estoi", True)):
        want = SR.score(x0, y0, extended, 1)                                 # once unmeasured, then the median of five
        host_ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            SR.score(x0, y0, extended, 1)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        host[name] = {"ms_one_clip": float(np.median(host_ms)), "d": want["d"], "Mk": want["Mk"],
                      "abs_diff_device": abs(want["d"] - float(out[f"{name}_10k"][0][0]))}
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N_16k": N, "N_10k": int(x10.shape[1]), "reps": args.reps, "warmup": 3,
           "arms_ms": {name: _spread(v) for name, v in ms.items()},
           "status_ok": int((out["stoi_10k"][1] == 0).sum()),
           "host_restatement_one_clip": host}
    for name, v in res["arms_ms"].items():
        print(json.dumps({"arm": name, **v}), flush=True)
    print(json.dumps({"host_restatement_one_clip": host}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
