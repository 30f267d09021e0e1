"""CPU: the restatement of mix_wavfiles_without_voice_overlay (tests/overlay_ref.py) and the host half of the overlay path of
voicesplit_amd/mixing.py -- the planner's draws and drop rules, the packing by length, and the descriptors of ``overlay_items``,
which a plain numpy interpreter (tests/overlay_helpers.py) turns back into audio and compares with the restatement for all 16 branch x kind cases."""
import os

import numpy as np
import pytest
import torch

import mixing_ref as MR
import overlay_ref as OR
from conftest import GOLDEN_DIR
from overlay_helpers import bursts, gen, host_pool, interpret, parse_items, reference_items, whole_pool

SR = 1000                              # 2 .. 4 "seconds" are 2000 .. 4000 samples: every rule of the recipe at a small size


def demo_clips():
    z = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    return [z[k][i].astype(np.float32) / 32768.0 for k in ("target", "mixed") for i in range(4)]


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_minmax_affine_is_sklearns_minmax_scale():
    sk = pytest.importorskip("sklearn.preprocessing")
    rng = np.random.default_rng(0)
    x = rng.standard_normal(500) * 0.3
    for xs, (lo, hi) in ((x, (-0.7, 0.71)), (x, (0.4, -0.35)), (np.full(17, 0.25), (-0.5, 0.5)), (np.zeros(9), (-0.9, 0.9)),
                         (x[:1], (-1.0, 1.0))):
        a, b = OR.minmax_affine(lo, hi, xs.min(), xs.max())
        want = sk.minmax_scale(xs.astype(np.float64), feature_range=(lo, hi)) if lo < hi else None
        if want is None:
            # sklearn refuses a reversed range outright; the reference only ever reaches it through uniform(a, b) with a > b, which
            # still gives lo < hi.  The affine itself is the formula of MinMaxScaler.fit, checked with the ends swapped
            fwd = sk.minmax_scale(xs.astype(np.float64), feature_range=(hi, lo))
            assert np.abs((xs * a + b) - (lo + hi - fwd)).max() <= 1e-12
            continue
        assert np.abs((xs * a + b) - want).max() <= 1e-12, (lo, hi)


def test_uniform_with_a_greater_than_b():
    assert OR.uniform(-0.05, -0.1, 0.0) == -0.05 and np.isclose(OR.uniform(-0.05, -0.1, 0.5), -0.075)
    lo, hi = OR.noise_range(-0.05, 0.999, 0.5)
    assert -0.1 < lo < -0.05 and np.isclose(hi, -lo - 0.01)


def test_split_spans_what_trim_keeps_on_the_demo_clips():
    for y in demo_clips():
        parts = OR.split_intervals(y, 1e-2)
        assert (parts[0][0], parts[-1][1]) == MR.trim_bounds(y)
        assert all(a < b for a, b in parts) and all(parts[k][1] < parts[k + 1][0] for k in range(len(parts) - 1))


def test_split_interval_shapes():
    rng = np.random.default_rng(1)
    n = 30000
    one = OR.split_intervals(bursts(rng, n, [(8000, 12000)]), 1e-2)
    assert len(one) == 1 and one[0][0] % 512 == 0 and 0 < one[0][0] <= 8000 and 12000 <= one[0][1] < n
    two = OR.split_intervals(bursts(rng, n, [(3000, 7000), (15000, 20000)]), 1e-2)
    assert len(two) == 2 and two[0][1] < 15000 and two[1][0] > 7000
    spans = [(2000 + 5500 * k, 4500 + 5500 * k) for k in range(5)]
    y5 = bursts(rng, n, spans)
    five = OR.split_intervals(y5, 1e-2)
    assert len(five) == 5
    assert OR.split_point(y5, 1e-2) == (five[2][1], 5) and spans[2][1] <= five[2][1] < spans[3][0]
    # an interval that runs into the last frame ends at n, not at a multiple of 512
    m = 30001
    tail = OR.split_intervals(bursts(rng, m, [(5000, 9000), (26000, m)]), 1e-2)
    assert len(tail) == 2 and tail[1][1] == m and m % 512 != 0
    assert OR.split_point(bursts(rng, m, [(5000, 9000), (26000, m)]), 1e-2)[0] == m
    # an all-zero signal: every frame at the clamp, one interval
    assert OR.split_intervals(np.zeros(5000, dtype=np.float32), 1e-2) == [(0, 5000)]
    assert OR.split_intervals(np.zeros(5000, dtype=np.float32), OR.RATIO_INTERF) == [(0, 5000)]
    # the interferer's threshold is the lower one: what 1e-2 calls loud, 10^-1.5 calls loud too
    assert OR.RATIO_INTERF > OR.RATIO_CLEAN


# ---- the planner --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """ids 0-3: voices of two bursts with a pause of more than a frame between them (two intervals in a 3 or 4 s crop, one in a
    2 s crop: a 2048-sample frame is silent only when all of it is), 4-7: one long burst (one interval),
    8-9: quiet voices (minimum above -0.1: uniform(a, b) with a > b), 10: a long reference clip, 11: a short reference clip,
    12: a voice of 2.5 s, 13: an all-zero clip."""
    rng = np.random.default_rng(7)
    clips = []
    for k in range(4):
        n = 4600 + 37 * k
        clips.append(bursts(rng, n, [(30 + 5 * k, 450), (2600 + 7 * k, n - 60)], amp=0.3 + 0.1 * k))
    for k in range(4):
        n = 4500 + 53 * k
        clips.append(bursts(rng, n, [(100, n - 100)], amp=0.25 + 0.1 * k))
    clips.append(bursts(rng, 4444, [(100, 4300)], amp=0.05))
    clips.append(bursts(rng, 4555, [(120 + 1100 * j, 700 + 1100 * j) for j in range(4)], amp=0.06))
    clips.append(bursts(rng, 15500, [(200, 15300)], amp=0.4))
    clips.append(bursts(rng, 9000, [(200, 8800)], amp=0.4))
    clips.append(bursts(rng, 2700, [(60, 2650)], amp=0.3))
    clips.append(np.zeros(4200, dtype=np.float32))
    noises = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((9000, 0.05), (8600, 0.2), (8300, 0.01))]
    pool, bounds = host_pool(clips)
    return clips, bounds, pool, noises, whole_pool(noises)


def voice_triplets():
    return [(c, 10, i) for c in range(10) for i in range(10) if c != i]


def test_planner_is_a_function_of_seed_epoch_rank(corpus):
    from voicesplit_amd.mixing import plan_overlay
    _, _, pool, _, npool = corpus
    tri = voice_triplets()
    fields = ("tri", "noise_ids", "Lc", "Li", "two_clean", "noise_start", "amp", "range_random", "range_plain", "gain", "bias",
              "item_trip", "item_kind", "item_len")
    a, b = plan_overlay(pool, npool, tri, SR, gen(3, 1, 0)), plan_overlay(pool, npool, tri, SR, gen(3, 1, 0))
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields) and a.dropped == b.dropped
    for other in (gen(4, 1, 0), gen(3, 2, 0), gen(3, 1, 1)):
        c = plan_overlay(pool, npool, tri, SR, other)
        assert not all(torch.equal(getattr(a, f), getattr(c, f)) for f in ("Lc", "two_clean", "noise_start", "amp"))


def test_planner_draws_stay_inside_the_references_ranges(corpus):
    from voicesplit_amd.mixing import plan_overlay
    clips, bounds, pool, noises, npool = corpus
    p = plan_overlay(pool, npool, voice_triplets() * 4, SR, gen(11))
    n = len(p.tri)
    assert n == 360 and sum(p.dropped.values()) == 0
    assert set(p.Lc.tolist()) == {2000, 3000, 4000} == set(p.Li.tolist())
    assert set(p.two_clean.tolist()) == {True, False} and set(p.noise_ids.flatten().tolist()) == {0, 1, 2}
    lo, hi = p.amp[:, :, 0], p.amp[:, :, 1]
    assert (lo >= -1).all() and (lo < -0.3).all() and (hi >= -lo).all() and (hi < -lo + 0.02).all()
    a = torch.minimum(lo[:, 1], lo[:, 2])
    lr, hr = p.range_random[:, 0], p.range_random[:, 1]
    assert (lr >= a).all() and (lr < -0.1).all() and (hr <= -lr).all() and (hr > -lr - 0.02).all()
    vmin = torch.tensor([float(c[s:e].min()) if e > s else 0.0 for c, (s, e) in zip(clips, bounds)], dtype=torch.float64)
    a = torch.minimum(vmin[p.tri[:, 0]], vmin[p.tri[:, 2]])
    lp, hp = p.range_plain[:, 0], p.range_plain[:, 1]
    assert (lp >= torch.minimum(a, torch.tensor(-0.1, dtype=torch.float64))).all() and (lp <= torch.clamp(a, min=-0.1)).all()
    assert (a > -0.1).any() and (a < -0.1).any()                            # uniform(a, b) with a > b is among them
    assert (hp <= -lp).all() and (hp > -lp - 0.02).all()
    nlen = torch.tensor([len(x) for x in noises])
    room = nlen[p.noise_ids].min(dim=1).values - (p.Lc + p.Li + 1)
    assert (p.noise_start >= 0).all() and (p.noise_start <= room).all() and (p.noise_start > 0).any()
    assert torch.equal(p.noise_at, npool.offsets[:-1][p.noise_ids] + p.noise_start[:, None])
    # the items: every triplet in the order of the kinds, with the length of its kind
    assert p.item_kind.tolist() == [1, 2, 3, 4] * n and p.item_trip.tolist() == [k for k in range(n) for _ in range(4)]
    want = torch.stack((p.Lc + p.Li, p.Lc, p.Li, p.Lc + p.Li), dim=1).flatten()
    assert torch.equal(p.item_len, want)
    p2 = plan_overlay(pool, npool, voice_triplets(), SR, gen(11), kinds=(4, 1), seconds=(2,))
    assert p2.item_kind.tolist() == [4, 1] * len(p2.tri) and set(p2.item_len.tolist()) == {4000}


def test_planner_drops_what_the_reference_drops_and_counts_it(corpus):
    from voicesplit_amd.mixing import plan_overlay
    _, _, pool, noises, npool = corpus
    tri = [(0, 10, 4), (0, 11, 4), (1, 11, 13), (12, 10, 4), (4, 10, 12), (13, 10, 4), (4, 10, 13), (5, 10, 1), (12, 11, 13)]
    p = plan_overlay(pool, npool, tri, SR, gen(0), seconds=(3,))
    # 11 is too short a reference (checked first, :77); 12 has 2.5 s for the 3 s drawn (:99); 13 is all zero
    assert p.dropped == {"emb_short": 3, "noise_short": 0, "voice_short": 2, "silent": 2}
    assert p.positions.tolist() == [0, 7] and p.tri.tolist() == [[0, 10, 4], [5, 10, 1]] and p.n_input == 9
    # 4 + 4 s need 8001 noise samples: only recording 0 of these three has them
    cut = [noises[0], noises[1][:8000], noises[2][:7000]]
    p = plan_overlay(pool, whole_pool(cut), [(0, 10, 4)] * 40, SR, gen(5), seconds=(4,))
    assert p.dropped["noise_short"] > 0 and p.dropped["noise_short"] + len(p.tri) == 40
    assert (p.noise_ids == 0).all() and sum(p.dropped.values()) == p.dropped["noise_short"]
    only_short = whole_pool(cut[1:])
    p = plan_overlay(pool, only_short, [(0, 10, 4)] * 5, SR, gen(5), seconds=(4,))
    assert p.dropped["noise_short"] == 5 and len(p.tri) == 0 and len(p.item_kind) == 0
    with pytest.raises(ValueError):
        plan_overlay(pool, npool, tri, SR, gen(0), kinds=(1, 5))
    with pytest.raises(ValueError):
        plan_overlay(pool, npool, tri, SR, gen(0), seconds=(1,))          # 1000 samples: below the 1025 a split needs


def test_every_batch_holds_one_length(corpus):
    from voicesplit_amd.mixing import pack_by_length, plan_overlay
    _, _, pool, _, npool = corpus
    p = plan_overlay(pool, npool, voice_triplets(), SR, gen(2))
    lens, groups = p.item_len.tolist(), ((p.item_kind == 2) | (p.item_kind == 3)).tolist()
    batches = pack_by_length(lens, groups, 3)
    assert batches and all(len(b) == 3 for b in batches)
    assert all(len({(lens[k], groups[k]) for k in b}) == 1 for b in batches)
    used = [k for b in batches for k in b]
    assert len(set(used)) == len(used)
    left = {}
    for k in set(range(len(lens))) - set(used):
        left[(lens[k], groups[k])] = left.get((lens[k], groups[k]), 0) + 1
    assert all(v < 3 for v in left.values())                               # drop_last per length
    assert all(b == sorted(b) for b in batches) and [b[-1] for b in batches] == sorted(b[-1] for b in batches)   # item order


# ---- the descriptors ----------------------------------------------------------------------------------------------------------
def test_descriptors_reproduce_the_restatement_in_all_16_cases(corpus):
    from voicesplit_amd.mixing import overlay_items, plan_overlay
    clips, bounds, pool, noises, npool = corpus
    flat, nflat = np.concatenate(clips), np.concatenate(noises)
    multi_ids, single_ids, quiet = [0, 1, 2, 3], [4, 5, 6, 7], [8, 9]
    tri = [(c, 10, i) for c in multi_ids for i in single_ids] + [(c, 10, i) for c in single_ids for i in multi_ids] + \
          [(c, 10, i) for c in single_ids for i in single_ids if c != i] + [(c, 10, i) for c in multi_ids for i in multi_ids if c != i] + \
          [(8, 10, 9), (9, 10, 8), (8, 10, 9), (9, 10, 8)]
    plan = plan_overlay(pool, npool, tri, SR, gen(21))
    assert sum(plan.dropped.values()) == 0
    ref = reference_items(plan, clips, bounds, noises)
    split = torch.tensor([r[2]["clip_idx"] for r in ref], dtype=torch.int32)
    count = torch.tensor([r[2]["count"] for r in ref], dtype=torch.int32)
    items = parse_items(overlay_items(plan, split, count))
    assert len(items) == 4 * len(ref)
    seen, worst, a_gt_b = set(), 0.0, 0
    for j, it in enumerate(items):
        k, kind = int(plan.item_trip[j]), int(plan.item_kind[j])
        pairs, norm1, info = ref[k]
        want_m, want_t = pairs[kind - 1]
        got_m, got_t, norm = interpret(it, flat, nflat, None if kind in (1, 4) else norm1)
        assert len(got_m) == len(want_m) == int(plan.item_len[j])
        assert abs(norm - (norm1 if kind != 4 else info["norm_random"])) <= 1e-6 * norm
        for got, want in ((got_m, want_m), (got_t, want_t)):
            err = float(np.abs(got - want).max())
            worst = max(worst, err / max(float(np.abs(want_m).max()), 1e-30))
            assert err <= 1e-6 * np.abs(want_m).max(), (j, kind, err)
        zero_t = want_t == 0
        assert (got_t[zero_t] == 0).all() and zero_t.any() == (kind != 2)      # silent target stretches are exact zeros
        seen.add((bool(plan.two_clean[k]), info["count"] > 1, kind))
        a_gt_b += min(clips[plan.tri[k, 0]].min(), clips[plan.tri[k, 2]].min()) > -0.1
    print("descriptors vs restatement: worst error %.3e of the row maximum" % worst)
    assert seen == {(tc, multi, kind) for tc in (True, False) for multi in (True, False) for kind in (1, 2, 3, 4)}, sorted(seen)
    assert a_gt_b >= 4                                                         # uniform(a, b) with a > b went through
    # the line-212 case reads the PLAIN affine for its clean half and the random one for the interferer half
    odd = [it for j, it in enumerate(items) if int(plan.item_kind[j]) == 4 and not plan.two_clean[plan.item_trip[j]]
           and ref[int(plan.item_trip[j])][2]["count"] == 1]
    assert odd and all(it["noise_sel"].tolist() == [1, 0, 1] and it["len"][2] == 0 for it in odd)


def test_command_lines_refuse_half_of_the_flag_pair(tmp_path):
    """--no-overlay and --noise-csv go together, in both tools, before anything touches a device or a file"""
    from voicesplit_amd import mixing, trainer
    for argv in (["-c", "none.json", "-r", ".", "-o", str(tmp_path), "--no-overlay"],
                 ["-c", "none.json", "-r", ".", "-o", str(tmp_path), "--noise-csv", "noise.csv"]):
        with pytest.raises(SystemExit):
            mixing.main(argv)
    for argv in (["-c", "none.json", "--mix-csv", "t.csv", "--no-overlay"], ["-c", "none.json", "--mix-csv", "t.csv", "--noise-csv", "n.csv"],
                 ["-c", "none.json", "--no-overlay", "--noise-csv", "n.csv"]):
        with pytest.raises(SystemExit):
            trainer.main(argv)
    names = tmp_path / "noise.csv"
    (tmp_path / "a.wav").write_bytes(b"")
    names.write_text("a.wav\n\n")
    assert mixing.read_noise_csv(str(names), str(tmp_path)) == [str(tmp_path / "a.wav")]
    names.write_text("a.wav\nmissing.wav\n")
    with pytest.raises(FileNotFoundError):
        mixing.read_noise_csv(str(names), str(tmp_path))
    assert mixing.output_name_sub("d", "*-mixed.wav", 12, 3) == os.path.join("d", "000012_3-mixed.wav")


def test_every_rank_sees_the_same_number_of_batches_and_their_union_is_the_global_batch(corpus):
    """Ranks that planned for themselves would each get their own number of batches (the lengths are drawn), and the training step
    ends in a collective.  Every rank plans the whole epoch alike and takes its share of each global batch."""
    from voicesplit_amd.mixing import OverlayBatches, pack_by_length
    from voicesplit_amd.trainer import EpochShard
    _, _, pool, _, npool = corpus
    tri = voice_triplets()
    acfg = {"sample_rate": SR, "hop_length": 10}
    table = torch.zeros(len(pool), 4)
    world, b = 3, 2
    obs = [OverlayBatches(pool, npool, tri, table, acfg, EpochShard(len(tri), b, r, world, seed=5), seed=8) for r in range(world)]
    for epoch in (0, 1):
        pos = [o.global_positions(epoch) for o in obs]
        assert pos[0] == pos[1] == pos[2] and len(pos[0]) == len(tri) // (b * world) * (b * world)
        # rank r's k-th list of the shard is its share of the k-th global batch
        for r, o in enumerate(obs):
            own = [p for lst in o.shard.epoch(epoch) for p in lst]
            assert own == [p for k in range(0, len(pos[0]), b * world) for p in pos[0][k + r * b:k + (r + 1) * b]]
        plans = [o.plan(pos[0], epoch) for o in obs]
        assert all(torch.equal(plans[0].item_len, p.item_len) and torch.equal(plans[0].noise_start, p.noise_start) for p in plans[1:])
        per_rank = [o.rank_batches(p) for o, p in zip(obs, plans)]
        assert len({len(x) for x in per_rank}) == 1 and len(per_rank[0]) > 4          # the same number of steps on every rank
        lens, groups = plans[0].item_len.tolist(), ((plans[0].item_kind == 2) | (plans[0].item_kind == 3)).tolist()
        whole = pack_by_length(lens, groups, b * world)
        for k, gb in enumerate(whole):
            parts = [per_rank[r][k] for r in range(world)]
            assert all(len(x) == b for x in parts) and [i for x in parts for i in x] == gb
            assert len({(lens[i], groups[i]) for i in gb}) == 1                       # one length on every rank, the same one
    assert len(obs[0].plan(pos[0], 0).tri) and not torch.equal(obs[0].plan(pos[0], 0).Lc, obs[0].plan(pos[0], 1).Lc)
    with pytest.raises(ValueError, match="one rank only"):
        OverlayBatches(pool, npool, tri, table, acfg, EpochShard(len(tri), b, 1, world), drop_last=False)
    from voicesplit_amd._lib import VoiceSplitHipError
    with pytest.raises(VoiceSplitHipError):
        next(obs[0].items(pos[0], 0))                                                 # pools without audio: no batches off the device
