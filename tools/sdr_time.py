"""Time of metrics.bss_sdr (vs_sdr) on the GPU, from device events after warm-up, next to the fp64 CPU restatement
(tests/bss_eval_ref.py, mir_eval's algorithm: FFT correlations, LU solve, FFT convolution) on the same data.

    python tools/sdr_time.py [--reps 20] [--out FILE.json]      (one JSON line per shape on stdout; --out: also a file)

Shapes: B = 64 x 48 000 (a test batch of 3 s clips) and B = 1 x 2^22 (one long recording).  The fp64 work per call is
2 * 512 * N FMAs per row for the correlations plus 512 * (N + 511) for the projection (reported as GFLOP, 2 per FMA).
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


def _data(B, N, seed):
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    ref = lfilter([1.0], [1.0, -1.2, 0.5], rng.standard_normal((B, N)), axis=1).astype(np.float32)
    est = (0.8 * ref + 0.1 * rng.standard_normal((B, N))).astype(np.float32)
    return ref, est


def main():
    import bss_eval_ref as R
    from voicesplit_amd import metrics
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-rows", type=int, default=8, help="rows of the B=64 batch the CPU restatement is timed on")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdr_time.py measures the GPU: no device here")
    res = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for B, N in ((64, 48000), (1, 1 << 22)):
        ref, est = _data(B, N, 1)
        r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
        for _ in range(3):
            sdr, st = metrics.bss_sdr(r, e)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            metrics.bss_sdr(r, e)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        rows = min(B, args.cpu_rows)
        t0 = time.perf_counter()
        want, _ = R.sdr_rows(ref[:rows], est[:rows])
        cpu_ms_row = 1e3 * (time.perf_counter() - t0) / rows
        got = sdr.cpu().numpy()[:rows]
        gflop = 2.0 * B * (2 * 512 * N + 512 * (N + 511)) / 1e9
        row = {"B": B, "N": N, "gpu_ms_median": float(np.median(ms)), "gpu_ms_min": float(np.min(ms)),
               "gpu_ms_max": float(np.max(ms)), "reps": args.reps, "gflop_fp64": gflop,
               "tflops_at_median": gflop / np.median(ms) if np.median(ms) > 0 else None,
               "cpu_restatement_ms_per_row": cpu_ms_row, "cpu_restatement_ms_for_B": cpu_ms_row * B,
               "max_abs_diff_db_vs_restatement": float(np.max(np.abs(got - want))), "status_ok": int((st == 0).sum())}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
