"""Cost of building training mixtures on the device (voicesplit_amd/mixing.py), B = 64 items of L = 48000 samples, one process,
the arms of every comparison alternating:

  (a) one batch of ``MixtureBatches`` (vs_mix_clips, both front ends, the embedding gather; the host plan of the epoch is timed on
      its own and given per batch) against the front end of ``BatchFeeder._finish`` alone on a resident wav batch
      (``audio.wav_to_spec(wav, want_phase=True)``): the difference is what mixing costs;
  (b) the bf16 training step fed by ``MixtureBatches.epoch`` against the same step on ONE resident batch;
  (c) ``vs_trim_bounds`` (``ClipPool``'s one launch) over a pool of about 10^4 synthetic clips of 3-15 s: clips/s and bytes/s of
      samples read.

    python tools/mix_time.py [--reps 7] [--out profiles/mix_time.json]

Device events around whole arms (a, c) and a host clock around steps that end in a synchronise (b); every shape is warmed up first;
medians with the min / max over the repetitions of the SAME arm.  A machine without a GPU fails: nothing here falls back.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, SR = 64, 48000, 16000


def _stats(v, digits=4):
    import numpy as np
    return {"median": round(float(np.median(v)), digits), "min": round(float(np.min(v)), digits), "max": round(float(np.max(v)), digits)}


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _synthetic_clips(n, seed, device, lo_s=3.0, hi_s=15.0):
    """speech-like levels, made on the device: noise under a slow envelope, quiet ends of random length"""
    import torch
    g = torch.Generator().manual_seed(seed)
    gd = torch.Generator(device=device).manual_seed(seed)
    sizes = torch.randint(int(lo_s * SR), int(hi_s * SR), (n,), generator=g).tolist()
    ends = torch.randint(0, SR // 2, (n, 2), generator=g).tolist()
    clips = []
    for m, (lead, tail) in zip(sizes, ends):
        y = torch.randn(m, generator=gd, device=device) * 0.1
        y *= 0.55 + 0.45 * torch.sin(torch.arange(m, device=device) * (6.283 / SR * 3.1))
        y[:lead] *= 1e-3
        y[m - tail:] *= 1e-3
        clips.append(y)
    return clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=16, help="training steps / batches per arm and repetition")
    ap.add_argument("--pool-clips", type=int, default=384, help="clips of the pool of (a) and (b)")
    ap.add_argument("--trim-clips", type=int, default=10000, help="clips of the pool of (c)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import voicesplit_amd as V
    from voicesplit_amd import _lib, audio, mixing, ops
    from voicesplit_amd.trainer import EpochShard, Trainer
    if not torch.cuda.is_available():
        raise SystemExit("mix_time.py measures the GPU: no device here")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    c = V.default_config()
    acfg = c.audio[c.audio["backend"]]
    out = {"device": torch.cuda.get_device_name(0), "B": B, "L": L, "reps": args.reps, "steps_per_rep": args.steps}

    # ---- the pool of (a) and (b) --------------------------------------------------------------------------------------------------
    pool = mixing.ClipPool(_synthetic_clips(args.pool_clips, args.seed, dev), dev)
    g = torch.Generator().manual_seed(args.seed)
    n_tri = B * args.steps
    tri = [tuple(int(v) for v in torch.randint(0, len(pool), (3,), generator=g)) for _ in range(2 * n_tri)]
    kept, _ = mixing.plan_triplets(pool, tri, L)
    kept = kept[:n_tri]
    assert len(kept) == n_tri, "the synthetic pool lost too many triplets to the length rule"
    table = torch.randn(len(pool), c.model["emb_dim"], generator=g)
    table = (table / table.norm(dim=1, keepdim=True)).to(dev)
    shard = EpochShard(n_tri, B, seed=args.seed)
    mb = mixing.MixtureBatches(pool, kept, table, acfg, L / SR, shard, crop="random", seed=args.seed)
    out["pool"] = {"clips": len(pool), "samples": pool.total, "triplets": n_tri}

    # ---- (a) one batch: mixing + both front ends against the feeder's front end alone ------------------------------------------
    wav = next(mb.items(list(shard.epoch(0))[:1], 0))["mixed_wav"]
    order = list(shard.epoch(0))
    _, at, _ = mb.plan(order, 0)
    at_dev = at.to(dev)

    def arm_mix():
        for _ in mb.epoch(0):
            pass

    def arm_front():
        for _ in range(args.steps):
            audio.wav_to_spec(wav, acfg, want_phase=True)

    def arm_kernels():                                            # vs_mix_clips alone
        for k in range(args.steps):
            mixing.mix_clips(pool.flat, at_dev[0, k * B:(k + 1) * B], at_dev[1, k * B:(k + 1) * B], L)

    arms = {"mixture_batch": arm_mix, "feeder_front_end": arm_front, "mix_clips_only": arm_kernels}
    ms = {k: [] for k in arms}
    for fn in arms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in arms.items():
            ms[name].append(_event_ms(fn) / args.steps)
    plan_ms = []
    for e in range(args.reps):
        t0 = time.perf_counter()
        mb.plan(list(shard.epoch(e)), e)
        plan_ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    a = {k + "_ms_per_batch": _stats(v) for k, v in ms.items()}
    a["host_plan_ms_per_batch"] = _stats(plan_ms)
    a["mixing_cost_ms_per_batch"] = round(a["mixture_batch_ms_per_batch"]["median"] - a["feeder_front_end_ms_per_batch"]["median"], 4)
    # bytes vs_mix_clips moves: reads c and i twice (the second pass out of cache at this size), writes two rows
    a["mix_clips_bytes"] = 6 * B * L * 4
    a["mix_clips_GBps_over_all_four_launches"] = round(a["mix_clips_bytes"] / a["mix_clips_only_ms_per_batch"]["median"] / 1e6, 1)
    out["a_batch"] = a

    # ---- (b) the bf16 training step: fed from the pool against one resident batch ------------------------------------------------
    ops.set_conv_math("bf16")
    c.train_config["learning_rate"] = 1e-4                        # noise has nothing to learn: keep the loss finite, the time is the same
    torch.manual_seed(args.seed)
    tr = Trainer(V.VoiceSplit(c).to(dev), c)
    resident = next(iter(mb.epoch(0)))

    def step_resident():
        for _ in range(args.steps):
            tr.train_step(resident)

    def step_mixed(e=[0]):
        e[0] += 1
        for batch in mb.epoch(e[0]):
            tr.train_step(batch)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    steps = {"resident_batch": step_resident, "mixture_batches": step_mixed}
    sms = {k: [] for k in steps}
    for fn in steps.values():
        fn()
    for _ in range(args.reps):
        for name, fn in steps.items():
            sms[name].append(wall_ms(fn))
    b = {k + "_ms_per_step": _stats(v, 3) for k, v in sms.items()}
    r, m = b["resident_batch_ms_per_step"]["median"], b["mixture_batches_ms_per_step"]["median"]
    b["fed_over_resident_percent"] = round(100.0 * (m / r - 1.0), 2)
    b["per_rep_percent"] = [round(100.0 * (y / x - 1.0), 2) for x, y in zip(sms["resident_batch"], sms["mixture_batches"])]
    b["utterances_per_s_fed"] = round(B / m * 1e3, 1)
    b["invalid_items"] = mb.invalid_items
    out["b_train_step_bf16"] = b
    del tr
    ops.release_workspaces()
    torch.cuda.empty_cache()

    # ---- (c) vs_trim_bounds over a large pool ----------------------------------------------------------------------------------------
    del pool, mb
    big = mixing.ClipPool(_synthetic_clips(args.trim_clips, args.seed + 1, dev), dev)
    n = len(big)
    ws = torch.empty(lib.vs_trim_workspace_bytes(big.total, n), dtype=torch.uint8, device=dev)
    bounds = torch.empty(n, 2, dtype=torch.int32, device=dev)
    peak = torch.empty(n, dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def trim(with_peak):
        _lib.check(lib.vs_trim_bounds(big.flat.data_ptr(), big.total, big.offsets.data_ptr(), big.offsets_dev.data_ptr(), n,
                                      bounds.data_ptr(), peak.data_ptr() if with_peak else None, ws.data_ptr(), ws.numel(), stream),
                   "vs_trim_bounds")

    tms = {"bounds_and_peak": [], "bounds_only": []}
    trim(True)
    trim(False)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        tms["bounds_and_peak"].append(_event_ms(lambda: trim(True)))
        tms["bounds_only"].append(_event_ms(lambda: trim(False)))
    assert torch.equal(bounds.cpu(), big.bounds)
    cc = {"clips": n, "samples": big.total, "bytes": big.total * 4,
          "trimmed_fraction_kept": round(float(big.trimmed_lengths.sum()) / big.total, 4)}
    for k, v in tms.items():
        s = _stats(v)
        cc[k + "_ms"] = s
        cc[k + "_clips_per_s"] = round(n / s["median"] * 1e3)
        cc[k + "_GBps_of_samples"] = round(big.total * 4 / s["median"] / 1e6, 1)
    out["c_trim_bounds"] = cc

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
