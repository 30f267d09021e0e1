"""Cost of the loudness leg on the device (voicesplit_amd/loudness.py, csrc/loudness.hip), one process, the arms of every comparison
alternating:

  (a) ``vs_loudness`` over a pool of synthetic clips of 3-15 s at 16 kHz (default 10^4 clips) against ``vs_clip_range`` over the same
      pool: ``vs_clip_range`` is one HBM-bound read of the pool and the yardstick -- the meter reads the pool twice;
  (b) ``vs_scale_clips`` over the pool against ``torch.mul_`` over the flat buffer;
  (c) the fp64 scipy restatement (tests/loudness_ref.py, ``serial``) of ONE 9 s clip on the host, for scale.

    python tools/loudness_time.py [--reps 20] [--clips 10000] [--out profiles/loudness_time.json]

Device events around the bare library calls (outputs and workspace allocated once, the clip table uploaded once); every arm is warmed
up first; medians with the min / max over the repetitions of the SAME arm.  A machine without a GPU fails: nothing here falls back.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from mix_time import _event_ms, _stats
    from voicesplit_amd import _lib, loudness
    from voicesplit_amd._call import ptr as _p, stream as _stream
    if not torch.cuda.is_available():
        raise SystemExit("loudness_time.py measures the GPU: no device here")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(args.seed)
    n = torch.randint(3 * SR, 15 * SR, (args.clips,), generator=g, dtype=torch.int64)
    offsets = torch.zeros(args.clips + 1, dtype=torch.int64)
    offsets[1:] = n.cumsum(0)
    total = int(offsets[-1])
    flat = torch.empty(total, dtype=torch.float32, device=dev)
    gd = torch.Generator(device=dev).manual_seed(args.seed)
    for lo in range(0, total, 1 << 26):                            # speech-like level, made on the device piece by piece
        flat[lo:lo + (1 << 26)].normal_(0.0, 0.05, generator=gd)
    table = torch.stack((offsets[:-1], n), dim=1).contiguous()
    table_dev, offsets_dev = table.to(dev), offsets.to(dev)
    N = args.clips
    meter = loudness.LoudnessMeter(SR, dev)
    nbytes = lib.vs_loudness_workspace_bytes(ctypes.byref(meter.dims), total, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lufs = torch.empty(N, dtype=torch.float64, device=dev)
    peak = torch.empty(N, dtype=torch.float32, device=dev)
    counts = torch.empty(N, 3, dtype=torch.int32, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev)
    rng = torch.empty(N, 2, dtype=torch.float32, device=dev)
    gain = torch.full((N,), 1.0009765625, dtype=torch.float32, device=dev)
    stream = _stream()

    def arm_loudness():
        _lib.check(lib.vs_loudness(ctypes.byref(meter.dims), _p(flat), total, _p(table), _p(table_dev), N, _p(lufs), _p(peak), _p(counts),
                                   _p(valid), None, None, _p(ws), ws.numel(), stream), "vs_loudness")

    def arm_range():
        _lib.check(lib.vs_clip_range(_p(flat), total, _p(offsets), _p(offsets_dev), None, N, _p(rng), stream), "vs_clip_range")

    def arm_scale():
        _lib.check(lib.vs_scale_clips(_p(flat), total, _p(table), _p(table_dev), _p(gain), N, stream), "vs_scale_clips")

    def arm_mul():
        flat.mul_(1.0009765625)

    arms = {"loudness": arm_loudness, "clip_range": arm_range, "scale_clips": arm_scale, "torch_mul_": arm_mul}
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in arms.items():
            ms[name].append(_event_ms(fn))
    out = {"device": torch.cuda.get_device_name(0), "sample_rate": SR, "clips": N, "samples": total, "bytes": 4 * total, "reps": args.reps,
           "workspace_bytes": int(nbytes)}
    for k, v in ms.items():
        out[k + "_ms"] = _stats(v)
    out["loudness_over_clip_range"] = round(out["loudness_ms"]["median"] / out["clip_range_ms"]["median"], 3)
    out["scale_over_mul_"] = round(out["scale_clips_ms"]["median"] / out["torch_mul__ms"]["median"], 3)
    out["loudness_GBps_of_two_reads"] = round(2 * 4 * total / out["loudness_ms"]["median"] / 1e6, 1)
    out["clip_range_GBps"] = round(4 * total / out["clip_range_ms"]["median"] / 1e6, 1)
    out["scale_clips_GBps_read_and_write"] = round(2 * 4 * total / out["scale_clips_ms"]["median"] / 1e6, 1)
    out["hours_of_audio_per_s"] = round(total / SR / 3600 / (out["loudness_ms"]["median"] / 1e3), 1)

    # ---- (c) the host restatement of one 9 s clip ------------------------------------------------------------------------------------
    import loudness_ref as LR
    x = (0.05 * np.random.default_rng(args.seed).standard_normal(9 * SR)).astype(np.float32)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        r = LR.serial(x, SR)
        host.append(1e3 * (time.perf_counter() - t0))
    one = float(loudness.integrated_loudness(torch.from_numpy(x).to(dev), SR))
    out["scipy_one_9s_clip_ms"] = _stats(host)
    out["scipy_one_9s_clip_lufs"] = r["lufs"]
    out["device_one_9s_clip_lufs"] = one
    out["device_ms_per_clip_in_the_pool"] = round(out["loudness_ms"]["median"] / N, 6)

    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
