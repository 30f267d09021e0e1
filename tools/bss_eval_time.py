"""Time of metrics.bss_eval (vs_bss_eval) on the GPU, from device events after warm-up, next to K^2 calls' worth of
metrics.bss_sdr (vs_sdr on [B * K^2, N] rows: the SDR matrix alone, no SIR, SAR or permutation) and to the fp64 host
restatement (tests/bss_eval_multi_ref.py, mir_eval's algorithm) on one item.

    python tools/bss_eval_time.py [--reps 20] [--out profiles/bss_eval_time.json]     (one JSON line per case on stdout)

B = 64 items of N = 48 000 samples; K = 1, 2, 4 with the permutation, K = 2, 4 without.  The two GPU arms alternate inside
one process: rep by rep, first vs_bss_eval, then vs_sdr on the same data.
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


def _data(B, K, N, seed):
    """K independent coloured sources per item; estimate q = 0.8 s_q + 0.15 * (the other sources) + noise."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    poles = [(-1.2, 0.5), (-0.6, 0.3), (0.4, 0.2), (-1.5, 0.7), (0.9, 0.4), (-0.2, 0.6)]
    ref = np.stack([lfilter([1.0], [1.0, *poles[k]], rng.standard_normal((B, N)), axis=1) for k in range(K)], axis=1)
    ref = (ref / ref.std(axis=2, keepdims=True)).astype(np.float32)
    total = ref.sum(axis=1, keepdims=True)
    est = (0.8 * ref + 0.15 * (total - ref) + 0.1 * rng.standard_normal((B, K, N))).astype(np.float32)
    return ref, est


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
    import bss_eval_multi_ref as M
    from voicesplit_amd import metrics
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=48000)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bss_eval_time.py measures the GPU: no device here")
    B, N = args.B, args.N
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "reps": args.reps, "warmup": 3, "cases": []}
    for K, perm in ((1, True), (2, True), (4, True), (2, False), (4, False)):
        ref, est = _data(B, K, N, 10 + K)
        r, e = torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()
        # the comparison arm's rows: every (estimate q, reference j) pair of every item, as K^2 vs_sdr calls would see them
        rr = r[:, None, :, :].expand(B, K, K, N).reshape(B * K * K, N).contiguous()
        ee = e[:, :, None, :].expand(B, K, K, N).reshape(B * K * K, N).contiguous()
        multi = lambda: metrics.bss_eval(r, e, compute_permutation=perm, return_pairs=True)
        single = lambda: metrics.bss_sdr(rr, ee)
        for _ in range(3):
            out = multi()
            sdr_rows, _ = single()
        torch.cuda.synchronize()
        ms_multi, ms_single = [], []
        for _ in range(args.reps):
            ms_multi.append(_timed(multi))
            ms_single.append(_timed(single))
        pairs = out[5].cpu().numpy()
        t0 = time.perf_counter()
        want = M.bss_eval_item(ref[0], est[0], perm)
        host_ms = 1e3 * (time.perf_counter() - t0)
        mask = np.isfinite(want[4])
        row = {"K": K, "compute_permutation": perm, "bss_eval_ms": _spread(ms_multi),
               "sdr_rows_ms": _spread(ms_single), "sdr_rows": B * K * K,
               "host_restatement_ms_one_item": host_ms, "host_restatement_ms_for_B": host_ms * B,
               "max_abs_diff_db_vs_restatement_item0": float(np.max(np.abs(pairs[0][mask] - want[4][mask]))),
               "sdr_matrix_equals_sdr_rows_bitwise": bool(np.array_equal(pairs[:, 0].reshape(-1), sdr_rows.cpu().numpy()))
               if perm else None,
               "status_ok": int((out[4] == 0).sum())}
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
