"""Cost of building the training items without voice overlay on the device (voicesplit_amd/mixing.py, csrc/mix_seq.hip), B = 64 items
of L = 64000 samples (2 s + 2 s), one process, the arms of every comparison alternating:

  (a) the batches of one ``OverlayBatches`` epoch (kind 1 only, both voices 2 s: every item has L samples) against the batches of one
      ``MixtureBatches`` epoch of the same B and length; the overlay epoch's work in front of its first batch (host plan,
      vs_split_point, descriptor assembly) is inside its arm and is also timed on its own;
  (b) ``vs_mix_sequence`` alone against ``vs_mix_clips`` alone on the same B and L;
  (c) ``vs_split_point`` over the trimmed clips of a pool of synthetic clips of 3-15 s: regions/s and bytes/s of samples read.

    python tools/overlay_time.py [--reps 7] [--out profiles/overlay_time.json]

Device events around whole arms; every shape is warmed up first; medians with the min / max over the repetitions of the SAME arm.
A machine without a GPU fails: nothing here falls back.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, SR, SECONDS = 64, 16000, 2
L = 2 * SECONDS * SR


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=16, help="batches per arm and repetition")
    ap.add_argument("--pool-clips", type=int, default=384, help="clips of the pool of (a) and (b)")
    ap.add_argument("--split-clips", type=int, default=4000, help="clips of the pool of (c)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import voicesplit_amd as V
    from mix_time import _event_ms, _stats, _synthetic_clips
    from voicesplit_amd import mixing
    from voicesplit_amd.trainer import EpochShard
    if not torch.cuda.is_available():
        raise SystemExit("overlay_time.py measures the GPU: no device here")
    dev = torch.device("cuda:0")
    c = V.default_config()
    acfg = c.audio[c.audio["backend"]]
    out = {"device": torch.cuda.get_device_name(0), "B": B, "L": L, "reps": args.reps, "steps_per_rep": args.steps}

    pool = mixing.ClipPool(_synthetic_clips(args.pool_clips, args.seed, dev, lo_s=5.5), dev)
    gd = torch.Generator(device=dev).manual_seed(args.seed)
    noise_pool = mixing.ClipPool([torch.randn(30 * SR + 17 * k, generator=gd, device=dev) * 0.05 for k in range(8)], dev, trim=False)
    g = torch.Generator().manual_seed(args.seed)
    n_tri = B * args.steps
    tri = [tuple(int(v) for v in torch.randint(0, len(pool), (3,), generator=g)) for _ in range(n_tri)]
    kept, dropped = mixing.plan_triplets(pool, tri, L)
    assert dropped == 0, "the synthetic pool lost triplets to the length rule"
    table = torch.randn(len(pool), c.model["emb_dim"], generator=g)
    table = (table / table.norm(dim=1, keepdim=True)).to(dev)
    shard = EpochShard(n_tri, B, seed=args.seed)
    mb = mixing.MixtureBatches(pool, kept, table, acfg, L / SR, shard, crop="head")
    ob = mixing.OverlayBatches(pool, noise_pool, kept, table, acfg, shard, seed=args.seed, kinds=(1,), seconds=(SECONDS,))
    out["pool"] = {"clips": len(pool), "samples": pool.total, "noise_samples": noise_pool.total, "triplets": n_tri}

    # ---- (a) whole epochs of batches ---------------------------------------------------------------------------------------------
    positions = [p for b in shard.epoch(0) for p in b]
    plan = ob.plan(positions, 0)
    assert sum(plan.dropped.values()) == 0 and len(plan.item_kind) == n_tri
    count, split, _ = mixing.split_points(pool.flat, plan.split_regions, plan.split_ratio)
    desc = mixing.overlay_items(plan, split, count)
    _, at, _ = mb.plan(list(shard.epoch(0)), 0)
    at_dev = at.to(dev)

    def arm_overlay():
        n = sum(1 for _ in ob.epoch(0))
        assert n == args.steps

    def arm_mixture():
        n = sum(1 for _ in mb.epoch(0))
        assert n == args.steps

    def arm_prepare():                                            # what an overlay epoch does in front of its first batch, device half
        cnt, spl, _ = mixing.split_points(pool.flat, plan.split_regions, plan.split_ratio)
        mixing.overlay_items(plan, spl, cnt)

    def arm_sequence():                                           # vs_mix_sequence alone
        for k in range(args.steps):
            mixing.mix_sequence(pool.flat, noise_pool.flat, desc[k * B:(k + 1) * B], L, L)

    def arm_clips():                                              # vs_mix_clips alone
        for k in range(args.steps):
            mixing.mix_clips(pool.flat, at_dev[0, k * B:(k + 1) * B], at_dev[1, k * B:(k + 1) * B], L)

    arms = {"overlay_batch": arm_overlay, "mixture_batch": arm_mixture, "mix_sequence_only": arm_sequence, "mix_clips_only": arm_clips}
    ms = {k: [] for k in arms}
    prep = []
    for fn in list(arms.values()) + [arm_prepare]:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in arms.items():
            ms[name].append(_event_ms(fn) / args.steps)
        prep.append(_event_ms(arm_prepare) / args.steps)
    plan_ms = []
    for e in range(args.reps):
        t0 = time.perf_counter()
        ob.plan(positions, e)
        plan_ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    a = {k + "_ms_per_batch": _stats(v) for k, v in ms.items() if k.endswith("_batch")}
    a["overlay_epoch_prepare_ms_per_batch"] = _stats(prep)
    a["overlay_host_plan_ms_per_batch"] = _stats(plan_ms)
    a["overlay_over_mixture"] = round(a["overlay_batch_ms_per_batch"]["median"] / a["mixture_batch_ms_per_batch"]["median"], 3)
    out["a_batch"] = a
    b = {k + "_ms_per_batch": _stats(v) for k, v in ms.items() if k.endswith("_only")}
    # bytes: vs_mix_sequence reads the voice and both noises twice (maximum and scale) and the noise slice once, writes two rows;
    # vs_mix_clips reads two voices twice and writes two rows
    b["mix_sequence_bytes"] = (2 * 3 + 2 + 2) * B * L * 4
    b["mix_clips_bytes"] = 6 * B * L * 4
    b["mix_sequence_GBps_over_all_launches"] = round(b["mix_sequence_bytes"] / b["mix_sequence_only_ms_per_batch"]["median"] / 1e6, 1)
    b["mix_clips_GBps_over_all_launches"] = round(b["mix_clips_bytes"] / b["mix_clips_only_ms_per_batch"]["median"] / 1e6, 1)
    b["sequence_over_clips"] = round(b["mix_sequence_only_ms_per_batch"]["median"] / b["mix_clips_only_ms_per_batch"]["median"], 3)
    out["b_kernels"] = b
    del mb, ob, pool, desc

    # ---- (c) vs_split_point over a pool ----------------------------------------------------------------------------------------------
    big = mixing.ClipPool(_synthetic_clips(args.split_clips, args.seed + 1, dev), dev)
    regions = torch.stack((big.trimmed_starts, big.trimmed_lengths), dim=1)
    ok = regions[:, 1] >= mixing.MIN_CLIP
    regions = regions[ok].contiguous()
    ratio = torch.full((len(regions),), mixing.RATIO_CLEAN, dtype=torch.float64)
    sms = []
    mixing.split_points(big.flat, regions, ratio)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        sms.append(_event_ms(lambda: mixing.split_points(big.flat, regions, ratio)))
    cnt, _, _ = mixing.split_points(big.flat, regions, ratio)
    s = _stats(sms)
    nbytes = int(regions[:, 1].sum()) * 4
    out["c_split_point"] = {"regions": len(regions), "samples": int(regions[:, 1].sum()), "bytes": nbytes, "ms": s,
                            "regions_per_s": round(len(regions) / s["median"] * 1e3), "GBps_of_samples": round(nbytes / s["median"] / 1e6, 1),
                            "mean_intervals": round(float(cnt.float().mean()), 3),
                            "note": "the time includes the wrapper's allocations and the upload of the region table"}

    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
