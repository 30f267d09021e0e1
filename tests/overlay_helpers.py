"""Helpers shared by tests/test_overlay_cpu.py and tests/test_gpu_overlay.py (a helper module, not a test): synthetic clips, pools
without audio for the host planner, a plain numpy interpreter of the ``vs_seq_item`` descriptors that ``overlay_items`` writes
(independent of the kernel and of the restatement: it knows segments, affines and a noise bed, nothing of the recipe), and the
restatement of tests/overlay_ref.py run over the kept triplets of a plan."""
import numpy as np
import torch

import mixing_ref as MR
import overlay_ref as OR


def bursts(rng, n, spans, amp=0.3, floor=1e-3):
    """quiet noise with loud stretches"""
    y = (rng.uniform(-1.0, 1.0, n) * floor).astype(np.float32)
    for lo, hi in spans:
        y[lo:hi] += (amp * np.sin(np.arange(hi - lo) * 0.21) * rng.uniform(0.5, 1.0, hi - lo)).astype(np.float32)
    return y


def host_pool(clips):
    """ClipPool.planned from numpy clips, with the numbers the device would compute (restated here)"""
    from voicesplit_amd.mixing import ClipPool
    bounds = [MR.trim_bounds(c) for c in clips]
    peak = [float(np.abs(c[s:e]).max()) if e > s else 0.0 for c, (s, e) in zip(clips, bounds)]
    rng = [(float(c[s:e].min()), float(c[s:e].max())) if e > s else (0.0, 0.0) for c, (s, e) in zip(clips, bounds)]
    return ClipPool.planned([len(c) for c in clips], bounds, peak, value_range=rng), bounds


def whole_pool(clips):
    from voicesplit_amd.mixing import ClipPool
    return ClipPool.planned([len(c) for c in clips], [(0, len(c)) for c in clips], None,
                            value_range=[(float(c.min()), float(c.max())) for c in clips])


def gen(seed, epoch=0, rank=0):
    from voicesplit_amd.mixing import crop_seed
    return torch.Generator().manual_seed(crop_seed(seed, epoch, rank))


def parse_items(desc):
    raw = desc.cpu().numpy()
    assert raw.dtype == np.uint8 and raw.shape[1] == 136
    i64 = np.ascontiguousarray(raw[:, :56]).view(np.int64)
    i32 = np.ascontiguousarray(raw[:, 56:96]).view(np.int32)
    f32 = np.ascontiguousarray(raw[:, 96:]).view(np.float32)
    return [dict(src_at=a[:3], noise1_at=a[3], noise2_at=a[4], range_at1=a[5], range_at2=a[6], len=b[:3], in_target=b[3:6],
                 noise_sel=b[6:9], range_len=b[9], gain=c[:3], bias=c[3:6], lo=c[6:8], hi=c[8:10]) for a, b, c in zip(i64, i32, f32)]


def interpret(it, flat, noise, norm_in=None):
    """vs_seq_item -> (mixed, target, norm) in fp64 from the fp32 numbers of the descriptor"""
    n = int(it["len"].sum())
    s = (noise[it["range_at1"]:it["range_at1"] + it["range_len"]] + noise[it["range_at2"]:it["range_at2"] + it["range_len"]]).astype(np.float64)
    aff = [OR.minmax_affine(float(it["lo"][k]), float(it["hi"][k]), s.min(), s.max()) for k in range(2)]
    mixed, target, t = np.zeros(n), np.zeros(n), 0
    for k in range(3):
        ln = int(it["len"][k])
        x = flat[it["src_at"][k]:it["src_at"][k] + ln].astype(np.float64)
        v = float(it["gain"][k]) * x + float(it["bias"][k])
        sel = int(it["noise_sel"][k])
        if sel >= 0:
            bed = (noise[it["noise1_at"] + t:it["noise1_at"] + t + ln] + noise[it["noise2_at"] + t:it["noise2_at"] + t + ln]).astype(np.float64)
            v = v + aff[sel][0] * bed + aff[sel][1]
        mixed[t:t + ln] = v
        if it["in_target"][k]:
            target[t:t + ln] = v
        t += ln
    norm = 1.1 * np.abs(mixed).max() if norm_in is None else norm_in
    return mixed / norm, target / norm, norm


def reference_items(plan, clips, bounds, noises):
    """the restatement for every kept triplet of a plan: [(pairs, norm, info)]"""
    out = []
    trimmed = [c[s:e] for c, (s, e) in zip(clips, bounds)]
    for k in range(len(plan.tri)):
        c, r, i = plan.tri[k].tolist()
        draws = {"two_clean": bool(plan.two_clean[k]),
                 "seconds_clean": int(plan.Lc[k]) / plan.sample_rate, "seconds_interf": int(plan.Li[k]) / plan.sample_rate,
                 "noise_start": int(plan.noise_start[k])}
        # the plan keeps the feature ranges, the restatement takes the underlying u: invert a + (b - a) u
        lo, hi = plan.amp[k, :, 0], plan.amp[k, :, 1]
        draws["amp"] = [((float(lo[j]) + 1.0) / 0.7, (float(hi[j]) + float(lo[j])) / 0.02) for j in range(3)]
        a = min(float(lo[1]), float(lo[2]))
        lr, hr = plan.range_random[k].tolist()
        draws["noise_random"] = ((lr - a) / (-0.1 - a), (-lr - hr) / 0.02)
        a = float(min(trimmed[c].min(), trimmed[i].min()))
        lp, hp = plan.range_plain[k].tolist()
        draws["noise"] = ((lp - a) / (-0.1 - a), (-lp - hp) / 0.02)
        info = {}
        n1, n2 = (noises[j] for j in plan.noise_ids[k].tolist())
        pairs, norm = OR.mix_without_overlay(trimmed[r], trimmed[c], trimmed[i], n1, n2, draws, plan.sample_rate, info)
        out.append((pairs, norm, info))
    return out
