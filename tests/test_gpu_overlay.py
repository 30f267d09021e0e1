"""GPU: the items without voice overlay (voicesplit_amd/mixing.py, csrc/mix_seq.hip) through the C ABI, against the fp64 restatement
of tests/overlay_ref.py.

vs_clip_range: exact.  vs_split_point: EXACT count, split point and interval list for every region whose closest frame is at least
1e-3 (relative) away from the silence threshold -- asserted on the inputs, as tests/test_gpu_mixing.py does for the trim.

vs_mix_sequence, the bound on a sample (u = 2^-24, the unit roundoff of fp32; the operation order is the header's):
  the voice   v1 = fmaf(g', x, b') with g' = fl(g), b' = fl(b): |v1 - (g x + b)| <= u (|g x| + |b|) + u |g x + b| <= 2 u V,  V = |g x| + |b|
  the noise   s = fl(n1 + n2) is the restatement's own float32 sum.  lo' = fl(lo), hi' = fl(hi); hi is close to -lo, so hi' - lo' has
              relative error <= u and scale' too; ngain = fl(scale'): 2 u; nbias = fl(lo' - nmin scale'): <= u |lo| + u |nmin scale| +
              u |nbias| <= 2 u Bn, Bn = |lo| + |nmin scale|; the fmaf rounds once more: the noise term is off by <= 3 u (A + Bn), A = |scale s|
  the add     one rounding of the sum: <= u (V + A + Bn)
so |v_gpu - v| <= 3 u V + 4 u (A + Bn) <= 4 u M with M = V + A + Bn taken over the MAGNITUDES of the terms (voice and noise can
cancel in v).  The maximum is off by at most 4 u M_max, norm = fl(1.1 m) by one more rounding: e_n = 4 u M_max / m + u relative.
The IEEE division adds one rounding:
  |out_gpu - out| <= (4 u M + |v| (e_n + u)) / norm,   times 1 + 2^-10 for the second-order terms.
With norm_in the same holds with e_n = u (the fp32 norm is given; the restatement's differs from it by what the kind-1 check
allows, which the test adds).  The measured maxima are printed; DESIGN.md 6.8h records them (on an MI355X over the 16 cases: worst
sample error 0.20 of its bound, 0.23 with norm_in; worst norm error 1.02e-7 relative against the asserted 2^-22 = 2.38e-7)."""
import json
import os

import numpy as np
import pytest
import torch

import mixing_ref as MR
import overlay_ref as OR
from overlay_helpers import bursts, gen, interpret, parse_items, reference_items

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MARGIN = 1e-3
U = 2.0 ** -24
RATIOS = (OR.RATIO_CLEAN, OR.RATIO_INTERF)


# ---- vs_clip_range ------------------------------------------------------------------------------------------------------------
def test_clip_range_is_exact_at_every_alignment_and_blind_to_its_neighbours():
    from voicesplit_amd import _lib
    from voicesplit_amd.mixing import ClipPool
    rng = np.random.default_rng(31)
    probe = bursts(rng, 7003, [(2500, 4200)], amp=0.05)
    loud = (rng.uniform(-1.0, 1.0, 4099) * 0.9).astype(np.float32)
    silent = np.zeros(4099, dtype=np.float32)
    clips = [bursts(rng, n, [(n // 3, n // 3 + 300 + 7 * k)], amp=0.1 + 0.05 * k) for k, n in enumerate((1025, 2047, 2049, 5119, 5121, 6000, 3001))]
    at = len(clips) + 1
    clips += [loud, probe, loud.copy(), silent, probe.copy(), silent.copy()]
    pool = ClipPool([torch.from_numpy(c) for c in clips], DEV)
    assert set((pool.offsets[:-1] % 4).tolist()) == {0, 1, 2, 3}
    got = pool.range
    assert got.dtype == torch.float32 and got.shape == (len(clips), 2) and pool.range is got
    bounds = pool.bounds.tolist()
    assert any(s > 0 and e < len(c) for (s, e), c in zip(bounds, clips))
    for k, (c, (s, e)) in enumerate(zip(clips, bounds)):
        assert got[k].tolist() == [float(c[s:e].min()), float(c[s:e].max())], k
    assert got[at].tolist() == got[at + 3].tolist() and bounds[at] == bounds[at + 3] and 0 < bounds[at][0]
    # bounds = NULL: the whole clip
    lib = _lib.load()
    out = torch.empty(len(clips), 2, device=DEV)
    rc = lib.vs_clip_range(pool.flat.data_ptr(), pool.total, pool.offsets.data_ptr(), pool.offsets_dev.data_ptr(), None, len(clips),
                           out.data_ptr(), None)
    assert rc == 0, lib.vs_last_error()
    assert out.cpu().tolist() == [[float(c.min()), float(c.max())] for c in clips]
    assert lib.vs_clip_range(pool.flat.data_ptr(), pool.total, None, pool.offsets_dev.data_ptr(), None, 3, out.data_ptr(), None) == -1


# ---- vs_split_point -----------------------------------------------------------------------------------------------------------
SPLIT_N = (1025, 2047, 2048, 2049, 5119, 5121, 32000)
GUARD = 1100                           # samples around a region: more than the 1024 a wrong reflection could reach


def split_signals():
    rng = np.random.default_rng(41)
    out = {}
    for n in SPLIT_N:
        if n < 5000:
            spans = [(n // 3, n // 3 + 300)]
        elif n < 6000:
            spans = [(0, 420), (3100, n)]                                  # two intervals, the second runs into the last frame
        else:
            spans = [(1000, 3000), (7000, 9500), (13000, 16000), (20000, 23000), (27000, n)]
        out[n] = bursts(rng, n, spans)
    return out


@pytest.fixture(scope="module")
def split_case():
    """Every signal at every alignment, once with loud and once with silent samples around it, at both ratios: (flat, regions,
    ratios, the signal of every region)."""
    rng = np.random.default_rng(42)
    sig = split_signals()
    parts, regions, ratios, which = [], [], [], []
    pos = 0
    for n in SPLIT_N:
        for r in range(4):
            for loud in (True, False):
                guard = lambda m: (rng.uniform(-1.0, 1.0, m) * 0.9).astype(np.float32) if loud else np.zeros(m, dtype=np.float32)
                lead = GUARD + (r - (pos + GUARD)) % 4                     # the region starts at residue r
                parts += [guard(lead), sig[n], guard(GUARD)]
                for ratio in RATIOS:
                    regions.append((pos + lead, n))
                    ratios.append(ratio)
                    which.append(n)
                pos += lead + n + GUARD
    flat = np.concatenate(parts)
    return flat, regions, ratios, which, sig


def test_split_inputs_are_off_the_threshold_and_cover_the_cases(split_case):
    flat, regions, ratios, which, sig = split_case
    margins = {(n, ratio): OR.split_margin(sig[n], ratio) for n in SPLIT_N for ratio in RATIOS}
    print("split margins: min %.3e" % min(margins.values()))
    assert min(margins.values()) >= MARGIN, margins
    assert {at % 4 for at, _ in regions} == {0, 1, 2, 3} and len(regions) == len(SPLIT_N) * 4 * 2 * 2
    for (at, n), w in zip(regions, which):
        assert np.array_equal(flat[at:at + n], sig[w])
    counts = {n: len(OR.split_intervals(sig[n], OR.RATIO_CLEAN)) for n in SPLIT_N}
    assert counts[32000] == 5 and counts[5119] == counts[5121] == 2 and counts[1025] == 1
    assert OR.split_intervals(sig[5121], OR.RATIO_CLEAN)[-1][1] == 5121      # ends at n, not at a multiple of 512


def test_split_points_equal_the_restatement_exactly(split_case):
    from voicesplit_amd.mixing import split_points
    flat, regions, ratios, which, sig = split_case
    cap = 8
    count, split, intervals = split_points(torch.from_numpy(flat).to(DEV), torch.tensor(regions), torch.tensor(ratios, dtype=torch.float64), cap)
    torch.cuda.synchronize()
    count, split, intervals = count.cpu().tolist(), split.cpu().tolist(), intervals.cpu().tolist()
    ref = {(n, ratio): OR.split_intervals(sig[n], ratio) for n in SPLIT_N for ratio in RATIOS}
    for b, (w, ratio) in enumerate(zip(which, ratios)):
        want = ref[(w, ratio)]
        assert count[b] == len(want), (b, w, ratio)
        assert split[b] == want[len(want) // 2][1] == OR.split_point(sig[w], ratio)[0], (b, w, ratio)
        assert [tuple(x) for x in intervals[b][:len(want)]] == want, (b, w, ratio)
        assert all(x == [-1, -1] for x in intervals[b][len(want):])        # the rest of the row is not written
    # a cap below the count: the first intervals only, count and split unchanged; and no interval buffer at all
    c2, s2, i2 = split_points(torch.from_numpy(flat).to(DEV), torch.tensor(regions), torch.tensor(ratios, dtype=torch.float64), 2)
    c3, s3, i3 = split_points(torch.from_numpy(flat).to(DEV), torch.tensor(regions), torch.tensor(ratios, dtype=torch.float64), 0)
    assert c2.cpu().tolist() == count == c3.cpu().tolist() and s2.cpu().tolist() == split == s3.cpu().tolist() and i3 is None
    assert all(row[:2] == full[:2] for row, full in zip(i2.cpu().tolist(), intervals))
    # an all-zero region: every frame at the clamp, one interval (0, n)
    z = torch.zeros(9000, device=DEV)
    c, s, i = split_points(z, torch.tensor([[3, 5000]]), torch.tensor([1e-2], dtype=torch.float64), 2)
    assert c.tolist() == [1] and s.tolist() == [5000] and i.tolist() == [[[0, 5000], [-1, -1]]]
    # outside the header's 0 < ratio < 1 no frame is non-silent: count 0, split n, no interval
    sig1 = torch.from_numpy(sig[5121]).to(DEV)
    c, s, i = split_points(sig1, torch.tensor([[0, 5121], [0, 5121]]), torch.tensor([1.0, 0.3], dtype=torch.float64), 2)
    assert OR.split_margin(sig[5121], 0.3) >= MARGIN
    want = OR.split_intervals(sig[5121], 0.3)
    assert c.tolist() == [0, len(want)] and s.tolist() == [5121, want[len(want) // 2][1]]
    assert i[0].tolist() == [[-1, -1], [-1, -1]] and [tuple(x) for x in i[1].tolist()[:len(want)]] == want[:2]


def test_split_refuses_a_region_of_1024_samples():
    from voicesplit_amd import _lib
    lib = _lib.load()
    flat = torch.zeros(8000, device=DEV)
    regions = torch.tensor([[0, 3000], [3001, 1024]], dtype=torch.int64)
    regions_dev, ratio = regions.to(DEV), torch.full((2,), 1e-2, dtype=torch.float64, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    split = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.vs_split_workspace_bytes(3000, 2), dtype=torch.uint8, device=DEV)
    args = lambda rh: (flat.data_ptr(), 8000, rh.data_ptr(), regions_dev.data_ptr(), ratio.data_ptr(), 2, count.data_ptr(),
                       split.data_ptr(), None, 0, ws.data_ptr(), ws.numel(), None)
    assert lib.vs_split_point(*args(regions)) == -1 and b"region 1 has 1024 samples" in lib.vs_last_error()
    outside = torch.tensor([[0, 3000], [6000, 2001]], dtype=torch.int64)
    assert lib.vs_split_point(*args(outside)) == -1 and b"leaves the buffer" in lib.vs_last_error()
    assert lib.vs_split_workspace_bytes(1024, 2) == 0
    torch.cuda.synchronize()
    assert (count == -7).all() and (split == -7).all()                     # nothing was launched


# ---- vs_mix_sequence ----------------------------------------------------------------------------------------------------------
SR = 1001                              # 2 and 3 "seconds" are 2002 and 3003 samples: lengths of 2 and 3 mod 4


def overlay_corpus():
    """The clips of tests/test_overlay_cpu.py's corpus that the 16 cases need, at odd lengths: ids 0-3 two bursts with a pause of more
    than a frame (two intervals in a 3 s crop), 4-7 one burst, 8-9 quiet (minimum above -0.1), 10 the reference clip."""
    rng = np.random.default_rng(7)
    clips = []
    for k in range(4):
        n = 4601 + 37 * k
        clips.append(bursts(rng, n, [(30 + 5 * k, 450), (2600 + 7 * k, n - 60)], amp=0.3 + 0.1 * k))
    for k in range(4):
        n = 4502 + 53 * k
        clips.append(bursts(rng, n, [(100, n - 100)], amp=0.25 + 0.1 * k))
    clips.append(bursts(rng, 4443, [(100, 4300)], amp=0.05))
    clips.append(bursts(rng, 4555, [(120 + 1100 * j, 700 + 1100 * j) for j in range(4)], amp=0.06))
    clips.append(bursts(rng, 15501, [(200, 15300)], amp=0.4))
    noises = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((9001, 0.05), (8602, 0.2), (8303, 0.01))]
    return clips, noises


def sixteen(plan, ref):
    """the first item of every (two_clean, more than one interval, kind) case: {case: item index}"""
    first = {}
    for j in range(len(plan.item_kind)):
        k = int(plan.item_trip[j])
        first.setdefault((bool(plan.two_clean[k]), ref[k][2]["count"] > 1, int(plan.item_kind[j])), j)
    return first


@pytest.fixture(scope="module")
def seq_case():
    """Pools on the device, a plan whose items cover the 16 branch x kind cases, the restatement of every kept triplet (computed once)
    and the device's split points."""
    from voicesplit_amd.mixing import ClipPool, overlay_items, plan_overlay, split_points
    clips, noises = overlay_corpus()
    pool = ClipPool([torch.from_numpy(c) for c in clips], DEV)
    npool = ClipPool([torch.from_numpy(c) for c in noises], DEV, trim=False)
    multi_ids, single_ids = [0, 1, 2, 3], [4, 5, 6, 7]
    tri = [(c, 10, i) for c in multi_ids for i in single_ids] + [(c, 10, i) for c in single_ids for i in multi_ids] + \
          [(8, 10, 9), (9, 10, 8), (4, 10, 5), (6, 10, 7), (0, 10, 1), (2, 10, 3)]
    plan = plan_overlay(pool, npool, tri, SR, gen(21), seconds=(2, 3))
    bounds = [tuple(b) for b in pool.bounds.tolist()]
    ref = reference_items(plan, clips, bounds, noises)
    count, split, _ = split_points(pool.flat, plan.split_regions, plan.split_ratio)
    desc = overlay_items(plan, split, count)
    torch.cuda.synchronize()
    return dict(clips=clips, noises=noises, pool=pool, npool=npool, plan=plan, bounds=bounds, ref=ref, count=count, split=split,
                desc=desc, cases=sixteen(plan, ref))


def test_seq_inputs_cover_the_cases_and_sit_off_the_thresholds(seq_case):
    s = seq_case
    plan, clips, ref = s["plan"], s["clips"], s["ref"]
    assert sum(plan.dropped.values()) == 0
    assert [tuple(b) for b in s["bounds"]] == [MR.trim_bounds(c) for c in clips] and min(MR.margin(c) for c in clips) >= MARGIN
    trimmed = [c[a:b] for c, (a, b) in zip(clips, s["bounds"])]
    for k in range(len(plan.tri)):
        c, _, i = plan.tri[k].tolist()
        crop = trimmed[c][:int(plan.Lc[k])] if plan.two_clean[k] else trimmed[i][:int(plan.Li[k])]
        assert OR.split_margin(crop, float(plan.split_ratio[k])) >= MARGIN, k
    # the device's split points are the restatement's
    assert s["split"].cpu().tolist() == [r[2]["clip_idx"] for r in ref] and s["count"].cpu().tolist() == [r[2]["count"] for r in ref]
    assert set(s["cases"]) == {(tc, multi, kind) for tc in (True, False) for multi in (True, False) for kind in (1, 2, 3, 4)}
    items = parse_items(s["desc"])
    batch = [items[j] for j in s["cases"].values()]
    # lengths of 2 and 3 mod 4 (a split point itself is a multiple of 512 or the crop's length), every residue of the indices
    lens = {int(x) % 4 for it in batch for x in it["len"] if x > 0}
    assert lens >= {2, 3} and len({int(it["len"].sum()) % 4 for it in batch}) >= 3
    assert {int(x) % 4 for it in batch for x, n in zip(it["src_at"], it["len"]) if n > 0} == {0, 1, 2, 3}
    assert {int(it["noise1_at"]) % 4 for it in batch} == {0, 1, 2, 3} == {int(it["noise2_at"]) % 4 for it in batch}
    assert any(min(clips[a].min(), clips[b].min()) > -0.1 for a, _, b in plan.tri.tolist())    # uniform(a, b) with a > b


def magnitudes(it, flat, noise):
    """(v, M) per output sample of a descriptor in fp64: the value and the sum of the magnitudes of its terms (the docstring's M)"""
    n = int(it["len"].sum())
    s = (noise[it["range_at1"]:it["range_at1"] + it["range_len"]] + noise[it["range_at2"]:it["range_at2"] + it["range_len"]]).astype(np.float64)
    v, M, t = np.zeros(n), np.zeros(n), 0
    for k in range(3):
        ln = int(it["len"][k])
        x = flat[it["src_at"][k]:it["src_at"][k] + ln].astype(np.float64)
        g, b = float(it["gain"][k]), float(it["bias"][k])
        v[t:t + ln] = g * x + b
        M[t:t + ln] = np.abs(g * x) + abs(b)
        sel = int(it["noise_sel"][k])
        if sel >= 0:
            sc, nb = OR.minmax_affine(float(it["lo"][sel]), float(it["hi"][sel]), s.min(), s.max())
            bed = (noise[it["noise1_at"] + t:it["noise1_at"] + t + ln] + noise[it["noise2_at"] + t:it["noise2_at"] + t + ln]).astype(np.float64)
            v[t:t + ln] += sc * bed + nb
            M[t:t + ln] += np.abs(sc * bed) + abs(float(it["lo"][sel])) + abs(s.min() * sc)
        t += ln
    return v, M


def check_rows(got_m, got_t, norm, want_m, want_t, want_norm, it, flat, noise, L, given_norm=False, norm_slack=0.0):
    """one item against the restatement; returns (relative norm error, worst sample error / its bound)"""
    n = len(want_m)
    v, M = magnitudes(it, flat, noise)
    m = np.abs(v).max()
    e_n = U if given_norm else 4 * U * M.max() / m + U
    bound = (4 * U * M + np.abs(v) * (e_n + U + norm_slack)) / want_norm * (1 + 2.0 ** -10)
    norm_err = abs(float(norm) - want_norm) / want_norm
    assert given_norm or norm_err <= e_n * (1 + 2.0 ** -10), (norm_err, e_n)
    worst = 0.0
    for got, want in ((got_m, want_m), (got_t, want_t)):
        assert got.shape == (L,) and got.dtype == np.float32
        err = np.abs(got[:n].astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (float((err / bound).max()), int((err / bound).argmax()))
        assert (got[n:] == 0.0).all()                                      # the row's tail
    assert (got_t[:n][want_t == 0] == 0.0).all()                           # zero target segments are exact zeros
    return norm_err, worst


@pytest.mark.parametrize("pad", [2, 5])
def test_mix_sequence_all_16_cases_against_the_restatement(seq_case, pad):
    from voicesplit_amd.mixing import mix_sequence
    s = seq_case
    plan, ref, pool, npool = s["plan"], s["ref"], s["pool"], s["npool"]
    flat, nflat = np.concatenate(s["clips"]), np.concatenate(s["noises"])
    cases = sorted(s["cases"].items())
    idx = torch.tensor([j for _, j in cases])
    desc = s["desc"].index_select(0, idx.to(DEV))
    items = parse_items(desc)
    L = 6006 + pad                                                         # 6008 = 0 mod 4, 6011 = 3 mod 4; the longest item has 6006
    assert max(int(it["len"].sum()) for it in items) <= 6006 < L and L % 4 == (0 if pad == 2 else 3)
    R = 6006
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    runs = [mix_sequence(pool.flat, npool.flat, desc, L, R, invalid_count=count) for _ in range(2)]
    only_max = mix_sequence(pool.flat, npool.flat, desc, L, R, rows=False)
    torch.cuda.synchronize()
    for x, y in zip(*runs):
        assert torch.equal(x, y)                                           # bit-identical reruns
    assert only_max[0] is None and only_max[1] is None
    assert torch.equal(only_max[2], runs[0][2]) and torch.equal(only_max[3], runs[0][3]) and torch.equal(only_max[4], runs[0][4])
    mixed, target, norm, aux, valid = (t.cpu().numpy() for t in runs[0])
    assert valid.tolist() == [1] * 16 and int(count) == 0
    worst_norm = worst = 0.0
    norm1 = {}
    for row, ((tc, multi, kind), j) in enumerate(cases):
        it, k = items[row], int(plan.item_trip[j])
        pairs, n1, info = ref[k]
        # the noise range and both affines: exactly the header's fp64 formula on the fp32 range and feature ranges
        if (it["noise_sel"][it["len"] > 0] >= 0).any():
            rs = nflat[it["range_at1"]:it["range_at1"] + it["range_len"]] + nflat[it["range_at2"]:it["range_at2"] + it["range_len"]]
            assert rs.dtype == np.float32 and aux[row, 0] == rs.min() == np.float32(info["nmin"]) and aux[row, 1] == rs.max()
            for sel in range(2):
                sc, nb = OR.minmax_affine(float(it["lo"][sel]), float(it["hi"][sel]), float(rs.min()), float(rs.max()))
                assert aux[row, 3 + 2 * sel] == np.float32(sc) and aux[row, 4 + 2 * sel] == np.float32(nb), (row, sel)
            # and the restatement's own affines (fp64 feature ranges) to the roundings of lo', hi', the scale and the bias
            for sel, (sc, nb) in enumerate((info["affine_plain"], info["affine_random"])):
                assert abs(aux[row, 3 + 2 * sel] - sc) <= 2 * U * abs(sc)
                assert abs(aux[row, 4 + 2 * sel] - nb) <= 2 * U * (abs(float(it["lo"][sel])) + abs(info["nmin"] * sc))
        else:
            assert (tc, multi) in ((True, True), (False, True)) and kind in (2, 3) and not aux[row, [0, 1, 3, 4, 5, 6]].any()
        want_m, want_t = pairs[kind - 1]
        want_norm = {1: n1, 4: info["norm_random"]}.get(kind)
        if kind in (2, 3):                                                 # without norm_in the item is divided by its own maximum
            own = 1.1 * np.abs(want_m * n1).max()
            want_m, want_t, want_norm = want_m * n1 / own, want_t * n1 / own, own
        assert norm[row] == np.float32(1.1 * np.float64(aux[row, 2]))
        e, w = check_rows(mixed[row], target[row], norm[row], want_m, want_t, want_norm, it, flat, nflat, L)
        worst_norm, worst = max(worst_norm, e), max(worst, w)
        if kind == 1:
            norm1[k] = (norm[row], n1)
    print("mix_sequence L=%d: worst norm error %.3e (bound 2^-22 = %.3e), worst sample error %.3f of its bound" % (L, worst_norm, 2.0 ** -22, worst))
    assert worst_norm <= 2.0 ** -22
    # kinds 2 and 3 as the recipe has them: divided by their triplet's kind-1 norm, given as norm_in
    rows23 = [(row, j) for row, ((_, _, kind), j) in enumerate(cases) if kind in (2, 3)]
    sub = desc.index_select(0, torch.tensor([r for r, _ in rows23], device=DEV))
    # the kind-1 norm of every triplet from a maximum-only call over kind-1 descriptors, as OverlayBatches gets them
    from voicesplit_amd.mixing import overlay_items
    trips = torch.tensor([int(plan.item_trip[j]) for _, j in rows23])
    kind1 = overlay_items(plan, s["split"], s["count"], trips, torch.ones(len(trips), dtype=torch.int64))
    n_in = mix_sequence(pool.flat, npool.flat, kind1, L, R, rows=False)[2]
    m2, t2, norm2, aux2, valid2 = (t.cpu().numpy() for t in mix_sequence(pool.flat, npool.flat, sub, L, R, norm_in=n_in))
    assert valid2.tolist() == [1] * 8 and np.array_equal(norm2, n_in.cpu().numpy()) and not aux2[:, 2].any()
    worst23 = 0.0
    for r2, (row, j) in enumerate(rows23):
        k, kind = int(plan.item_trip[j]), int(plan.item_kind[j])
        pairs, n1, _ = ref[k]
        slack = abs(float(norm2[r2]) - n1) / n1
        assert slack <= 2.0 ** -22
        if k in norm1:
            assert norm1[k][0] == norm2[r2]                                # the same bits as the full kind-1 item gave
        _, w = check_rows(m2[r2], t2[r2], norm2[r2], pairs[kind - 1][0], pairs[kind - 1][1], n1, items[row], flat, nflat, L,
                          given_norm=True, norm_slack=slack)
        worst23 = max(worst23, w)
        assert kind != 3 or not t2[r2].any()
    print("mix_sequence with norm_in: worst sample error %.3f of its bound" % worst23)


def hand_item(src_at, lens, noise_at=(0, 0), rng_at=(0, 0), range_len=1, sel=(-1, -1, -1), in_target=(1, 0, 1), gain=(1, 1, 1),
              bias=(0, 0, 0), lo=(-0.3, -0.5), hi=(0.29, 0.51)):
    i64 = np.array(list(src_at) + list(noise_at) + list(rng_at), dtype=np.int64)
    i32 = np.array(list(lens) + list(in_target) + list(sel) + [range_len], dtype=np.int32)
    f32 = np.array(list(gain) + list(bias) + list(lo) + list(hi), dtype=np.float32)
    row = np.concatenate([i64.view(np.uint8), i32.view(np.uint8), f32.view(np.uint8)])
    assert row.shape == (136,)
    return row


def test_mix_sequence_hand_built_segments_of_every_length_mod_4():
    """Descriptors the recipe cannot produce -- a first segment of 1 mod 4, three segments with three affines, absent segments in
    front -- against the numpy interpreter of the descriptor (tests/overlay_helpers.py)."""
    from voicesplit_amd.mixing import mix_sequence
    rng = np.random.default_rng(9)
    flat = (rng.standard_normal(30000) * 0.2).astype(np.float32)
    noise = (rng.standard_normal(20000) * 0.05).astype(np.float32)
    rows = [hand_item((3, 5002, 9001), (2049, 1023, 2050), (1, 6), (1, 6), 5122, sel=(0, 1, 0), gain=(0.9, -1.3, 0.5), bias=(0.01, -0.02, 0.0)),
            hand_item((10, 20, 30), (1, 2, 3), (7, 2), (7, 2), 6, sel=(1, -1, 1)),
            hand_item((0, 0, 4097), (0, 0, 4099), (3, 0), (0, 3), 4099, sel=(0, 0, 0), in_target=(0, 0, 1)),
            hand_item((6, 0, 0), (2047, 0, 0), sel=(-1, 0, 0)),
            hand_item((0, 12001, 0), (0, 2047, 0), (5, 5), (4, 4), 3001, sel=(-1, 1, -1), in_target=(0, 1, 0), gain=(1, 0.25, 1), bias=(0, 0.125, 0))]
    desc = torch.from_numpy(np.stack(rows)).to(DEV)
    items = parse_items(desc)
    assert {int(x) % 4 for it in items for x in it["len"] if x > 0} == {1, 2, 3}
    for L in (5124, 5123 + 4):
        mixed, target, norm, aux, valid = (t.cpu().numpy() for t in mix_sequence(torch.from_numpy(flat).to(DEV), torch.from_numpy(noise).to(DEV), desc, L, 5122))
        assert valid.tolist() == [1] * 5
        for row, it in enumerate(items):
            want_m, want_t, want_norm = interpret(it, flat, noise)
            e, w = check_rows(mixed[row], target[row], norm[row], want_m, want_t, want_norm, it, flat, noise, L)
            print("hand-built row %d, L=%d: norm error %.3e, worst sample error %.3f of its bound" % (row, L, e, w))


def test_mix_sequence_refuses_indices_outside_either_buffer_and_counts():
    from voicesplit_amd import _lib
    lib = _lib.load()
    total, ntotal, L, R = 4000, 3000, 1603, 1700
    flat = torch.ones(total, device=DEV)
    flat[2000:3700] = 0.0
    noise = torch.full((ntotal,), 0.5, device=DEV)
    rows = [hand_item((0, 0, 0), (1600, 0, 0)),                                                         # fine
            hand_item((2401, 0, 0), (1600, 0, 0)),                                                      # a segment past the voices
            hand_item((-1, 0, 0), (1600, 0, 0)),
            hand_item((0, 3999, 0), (800, 2, 0)),
            hand_item((0, 0, 0), (1600, 0, 0), (1401, 0), (0, 0), 10, sel=(0, -1, -1)),                 # the noise bed past the noise
            hand_item((0, 0, 0), (1600, 0, 0), (0, -2), (0, 0), 10, sel=(0, -1, -1)),
            hand_item((0, 0, 0), (1600, 0, 0), (0, 0), (0, 1301), 1700, sel=(0, -1, -1)),               # the range slice past the noise
            hand_item((0, 0, 0), (1600, 0, 0), (0, 0), (0, 0), 1701, sel=(0, -1, -1)),                  # range_len above R
            hand_item((0, 0, 0), (1600, 0, 0), (0, 0), (0, 0), 10, sel=(2, -1, -1)),                    # noise_sel outside -1 .. 1
            hand_item((0, 0, 0), (1000, 604, 0)),                                                       # longer than L
            hand_item((0, 0, 0), (-4, 0, 0)),
            hand_item((2000, 0, 0), (1600, 0, 0)),                                                      # all zero: valid 0
            hand_item((0, 0, 0), (0, 0, 0)),                                                            # no segment at all: valid 0
            hand_item((2000, 0, 0), (1600, 0, 0), (1400, 1400), (0, 0), 3000, sel=(0, -1, -1), lo=(-0.2, -0.2), hi=(0.2, 0.2))]  # to the last sample
    B = len(rows)
    desc = torch.from_numpy(np.stack(rows)).to(DEV)
    want_valid = [1] + [-1] * 10 + [0, 0, 1]
    guard = 64
    bufs = [torch.full((B * L + 2 * guard,), 7.0, device=DEV) for _ in range(2)]
    norm, aux = torch.full((B,), 7.0, device=DEV), torch.full((B, 8), 7.0, device=DEV)
    valid = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        rc = lib.vs_mix_sequence(flat.data_ptr(), total, noise.data_ptr(), ntotal, desc.data_ptr(), B, L, 3000, None,
                                 bufs[0].data_ptr() + 4 * guard, bufs[1].data_ptr() + 4 * guard, norm.data_ptr(), aux.data_ptr(),
                                 valid.data_ptr(), count.data_ptr(), None)
        assert rc == 0, lib.vs_last_error()
    torch.cuda.synchronize()
    # R = 3000 here so that item 13's range is allowed; item 7 (range_len 1701) is then inside R too and fine as a range -- it is
    # refused in the second call below, with R = 1700
    want_first = list(want_valid)
    want_first[7] = 1
    assert valid.tolist() == want_first and int(count) == 2 * sum(v != 1 for v in want_first)           # invalid_count accumulates
    for buf in bufs:
        assert (buf[:guard] == 7.0).all() and (buf[-guard:] == 7.0).all()                               # the canary around the rows
        rows_out = buf[guard:-guard].view(B, L)
        for b, v in enumerate(want_first):
            if v != 1:
                assert not rows_out[b].any(), b
    mixed = bufs[0][guard:-guard].view(B, L)
    assert torch.equal(mixed[0, :1600], torch.full((1600,), 1.0 / float(np.float32(1.1)), device=DEV)) and not mixed[0, 1600:].any()
    # the constant noise bed: den = 1, scale 0.4, bias lo - 0.4: v = 0 + fmaf(0.4, 1.0, -0.6) everywhere
    assert float(aux[13, 0]) == 1.0 == float(aux[13, 1]) and valid[13] == 1 and (mixed[13, :1600] != 0).all()
    valid2 = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    rc = lib.vs_mix_sequence(flat.data_ptr(), total, noise.data_ptr(), ntotal, desc.data_ptr(), B, L, R, None, None, None,
                             norm.data_ptr(), aux.data_ptr(), valid2.data_ptr(), None, None)
    assert rc == 0
    want_second = list(want_valid)
    want_second[13] = -1                                                                                # its range_len is above R = 1700
    assert valid2.tolist() == want_second
    # argument errors: no exception across the ABI, nothing launched
    assert lib.vs_mix_sequence(flat.data_ptr(), total, noise.data_ptr(), ntotal, desc.data_ptr(), B, L, R, None, bufs[0].data_ptr(), None,
                               norm.data_ptr(), aux.data_ptr(), valid.data_ptr(), None, None) == -1 and b"together" in lib.vs_last_error()
    assert lib.vs_mix_sequence(flat.data_ptr(), total, noise.data_ptr(), ntotal, desc.data_ptr(), 0, L, R, None, None, None,
                               norm.data_ptr(), aux.data_ptr(), valid.data_ptr(), None, None) == -1


# ---- batch level --------------------------------------------------------------------------------------------------------------
def _small_cfg():
    """the small configuration of tests/test_gpu_trainer.py"""
    import voicesplit_amd as V
    dims = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
    c = V.default_config(**dims)
    c.audio["voicefilter"].update({"hop_length": 16, "win_length": 40})
    c.train_config["learning_rate"] = 1e-3
    return c, dims


@pytest.fixture(scope="module")
def batch_case():
    """A dozen synthetic voices of a bit more than 3 s at 16 kHz (half of them with a pause: two intervals) and two noise clips."""
    from voicesplit_amd.mixing import ClipPool
    rng = np.random.default_rng(17)
    clips = []
    for k in range(12):
        n = 49000 + 1237 * k
        spans = [(300 + 11 * k, 9000), (30000 + 13 * k, n - 200)] if k % 2 == 0 else [(400, n - 300)]
        clips.append(bursts(rng, n, spans, amp=0.15 + 0.03 * k))
    noises = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((100001, 0.05), (97003, 0.1))]
    pool = ClipPool([torch.from_numpy(c) for c in clips], DEV)
    npool = ClipPool([torch.from_numpy(c) for c in noises], DEV, trim=False)
    assert npool.peak is None and npool.bounds.tolist() == [[0, len(c)] for c in noises]     # used whole: no trim pass
    tri = [(a, (a + 5) % 12, (a + 1 + 2 * (a % 3)) % 12) for a in range(12)]
    return clips, noises, pool, npool, tri


def test_overlay_batches_first_batch_is_the_restatement_and_trains(batch_case):
    import voicesplit_amd as V
    from voicesplit_amd import audio, mixing
    from voicesplit_amd.trainer import EpochShard, Trainer
    clips, noises, pool, npool, tri = batch_case
    c, dims = _small_cfg()
    acfg = c.audio["voicefilter"]
    B = 2
    table = torch.randn(len(pool), dims["emb_dim"], generator=torch.Generator().manual_seed(2)).to(DEV)
    shard = EpochShard(len(tri), B, seed=4)
    ob = mixing.OverlayBatches(pool, npool, tri, table, acfg, shard, seed=6, seconds=(2, 3))
    positions = [p for b in shard.epoch(0) for p in b]
    items = list(ob.items(positions, 0))
    batches = list(ob.epoch(0))
    assert len(items) == len(batches) >= 6 and ob.invalid_items == 0 == ob.refused_items and sum(ob.dropped.values()) == 0
    assert positions == ob.global_positions(0)                             # one rank: its own triplets are the global list
    plan = items[0]["plan"]
    assert len(plan.tri) == 12 and plan.tri.tolist() == [list(tri[p]) for p in positions]
    F, sr = dims["num_freq"], acfg["sample_rate"]
    seen_len = set()
    for it, (emb, target, mixed, seq_len, target_wav, phase) in zip(items, batches):
        L = int(seq_len[0])
        seen_len.add(L)
        T = L // acfg["hop_length"] + 1
        assert L in (2 * sr, 3 * sr, 4 * sr, 5 * sr, 6 * sr) and seq_len.tolist() == [L] * B and seq_len.dtype == torch.int64
        assert emb.shape == (B, dims["emb_dim"]) and target.shape == mixed.shape == phase.shape == (B, T, F) and target_wav.shape == (B, L)
        assert all(t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() for t in (emb, target, mixed, target_wav, phase))
        assert it["valid"].tolist() == [1] * B and plan.item_len[it["item_trip"] * 4 + it["item_kind"] - 1].tolist() == [L] * B
        assert torch.equal(emb, table[plan.tri[it["item_trip"], 1]]) and torch.equal(it["target_wav"], target_wav)
        spec, ph = audio.wav_to_spec(it["mixed_wav"], acfg, want_phase=True)
        assert torch.equal(mixed, spec) and torch.equal(phase, ph)
        assert torch.equal(target, audio.wav_to_spec(target_wav, acfg, want_phase=False)[0])
        kinds = set(it["item_kind"].tolist())
        assert kinds <= {1, 4} or kinds <= {2, 3}                          # the two groups are packed apart
    assert len(seen_len) >= 3
    # the same tuple as MixtureBatches yields for this B and length (3 s: what every voice of this pool has)
    same = next(b for b in batches if int(b[3][0]) == 3 * sr)
    kept, dropped = mixing.plan_triplets(pool, tri, 3 * sr)
    assert dropped == 0
    mb = mixing.MixtureBatches(pool, kept, table, acfg, 3, EpochShard(len(kept), B, seed=4), crop="head")
    other = next(iter(mb.epoch(0)))
    for a, b in zip(same, other):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
    it0 = items[0]
    L0 = int(batches[0][3][0])
    # the first batch against the restatement
    bounds = [tuple(b) for b in pool.bounds.tolist()]
    assert bounds == [MR.trim_bounds(x) for x in clips]
    flat, nflat = np.concatenate(clips), np.concatenate(noises)
    trips = sorted(set(it0["item_trip"].tolist()))
    sub = mixing.OverlayPlan()
    sub.__dict__.update({k: (v[trips] if torch.is_tensor(v) and len(v) == len(plan.tri) else v) for k, v in plan.__dict__.items()})
    ref = dict(zip(trips, reference_items(sub, clips, bounds, noises)))
    descs = parse_items(it0["desc"])
    mixed_wav, target_wav, norm = (it0[k].cpu().numpy() for k in ("mixed_wav", "target_wav", "norm"))
    for row, (t, kind) in enumerate(zip(it0["item_trip"].tolist(), it0["item_kind"].tolist())):
        pairs, n1, info = ref[t]
        cl, _, itf = plan.tri[t].tolist()
        crop = clips[cl][bounds[cl][0]:][:int(plan.Lc[t])] if plan.two_clean[t] else clips[itf][bounds[itf][0]:][:int(plan.Li[t])]
        assert OR.split_margin(crop, float(plan.split_ratio[t])) >= MARGIN and min(MR.margin(clips[x]) for x in (cl, itf)) >= MARGIN
        want_norm = info["norm_random"] if kind == 4 else n1
        slack = abs(float(norm[row]) - want_norm) / want_norm
        assert slack <= 2.0 ** -22
        e, w = check_rows(mixed_wav[row], target_wav[row], norm[row], pairs[kind - 1][0], pairs[kind - 1][1], want_norm, descs[row], flat,
                          nflat, L0, given_norm=kind in (2, 3), norm_slack=slack if kind in (2, 3) else 0.0)
        print("batch 0 row %d kind %d: norm error %.3e, worst sample error %.3f of its bound" % (row, kind, e, w))
    # the same (seed, epoch, rank): the same bits; another epoch: other draws
    again = list(ob.epoch(0))
    assert all(torch.equal(x, y) for a, b in zip(batches, again) for x, y in zip(a, b))
    nxt = list(ob.epoch(1))
    assert len(nxt) >= 4 and not all(a[4].shape == b[4].shape and torch.equal(a[4], b[4]) for a, b in zip(batches, nxt))
    # an epoch that is abandoned early still reports what the kernel marked (nothing here)
    early = ob.epoch(2)
    next(early)
    early.close()
    assert ob.invalid_items == 0 == ob.refused_items
    # one training step of the small configuration on an overlay batch
    torch.manual_seed(0)
    model = V.VoiceSplit(c).cuda()
    tr = Trainer(model, c)
    short = min(batches, key=lambda b: int(b[3][0]))
    loss = tr.train_step(short)
    assert np.isfinite(loss), loss
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_overlay_writer_round_trip_through_the_dataset(tmp_path):
    from scipy.io import wavfile
    import voicesplit_amd as V
    from voicesplit_amd import mixing
    from voicesplit_amd.trainer import SpecWavDataset
    # voices of a bit more than 4 s and noise of more than 8 s: the command line draws from the reference's 2, 3 and 4 s
    rng = np.random.default_rng(23)
    clips = [bursts(rng, 65000 + 1237 * k, [(300 + 11 * k, 9000), (30000 + 13 * k, 64800 + 1237 * k)] if k % 2 == 0 else [(400, 64700 + 1237 * k)],
                    amp=0.15 + 0.03 * k) for k in range(4)]
    noises = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((130001, 0.05), (129003, 0.1))]
    root = tmp_path / "corpus"
    root.mkdir()
    for k in range(4):
        wavfile.write(str(root / f"v{k}.wav"), 16000, clips[k])            # float32 files
    for k in range(2):
        wavfile.write(str(root / f"n{k}.wav"), 16000, noises[k])
    csv_path = tmp_path / "train.csv"
    csv_path.write_text("clean_utterance,embedding_utterance,interference_utterance\nv0.wav,v2.wav,v1.wav\nv1.wav,v3.wav,gone.wav\nv3.wav,v0.wav,v2.wav\n")
    noise_csv = tmp_path / "noise.csv"
    noise_csv.write_text("n0.wav\nn1.wav\n")
    c = V.default_config()
    out = tmp_path / "out"
    c.dataset = {"train_dir": str(out / "train"), "test_dir": str(out / "train"), "format": dict(mixing.DEFAULT_FORMAT)}
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps({k: (dict(v) if isinstance(v, dict) else v) for k, v in c.items()}, indent=1))
    with pytest.raises(SystemExit):
        mixing.main(["-c", str(cfg_path), "-r", str(root), "-d", str(csv_path), "-o", str(out), "--no-overlay"])
    mixing.main(["-c", str(cfg_path), "-r", str(root), "-d", str(csv_path), "-o", str(out), "--no-overlay", "--noise-csv", str(noise_csv),
                 "--seed", "3"])
    want = sorted(f"{n:06d}_{k}-{s}" for n in (0, 2) for k in (1, 2, 3, 4) for s in ("mixed.wav", "target.wav", "emb.wav", "mixed.pt", "target.pt"))
    assert sorted(os.listdir(out / "train")) == want
    for n in (0, 2):
        for k in (1, 2, 3, 4):
            torch.save(torch.randn(256), str(out / "train" / f"{n:06d}_{k}-emb.pt"))       # the speaker-encoder step of the reference's pipeline
    ds = SpecWavDataset(c)
    assert len(ds) == 8
    acfg = c.audio["voicefilter"]
    for i in range(8):
        emb, target, mixed_wav, seq_len, target_wav = ds[i]
        k = i % 4 + 1
        L = int(seq_len)
        assert mixed_wav.shape == target_wav.shape == (L,) and L in range(32000, 128001, 16000) and target.shape == (L // 160 + 1, 601)
        peak = float(mixed_wav.abs().max())                                # kinds 2 and 3 are parts of kind 1's mixture over ITS norm
        assert np.isclose(peak, 1 / 1.1, rtol=1e-6) if k in (1, 4) else 0 < peak <= (1 + 1e-6) / 1.1
        assert (k == 2) == bool(torch.equal(mixed_wav, target_wav)) and (k == 3) == (not target_wav.any())
    # the emb wav: the trimmed reference clip over the item's norm; for sub 4 min-max scaled first (its extremes are the drawn range)
    paths, triplets, numbers, skipped = mixing.read_triplet_csv(str(csv_path), str(root))
    assert numbers == [0, 2] and skipped == 1
    e1, e2, e4 = (wavfile.read(str(out / "train" / f"000000_{k}-emb.wav"))[1] for k in (1, 2, 4))
    s, e = MR.trim_bounds(clips[2])
    assert e1.dtype == np.float32 and np.array_equal(e1, e2) and e1.shape == e4.shape == (e - s,)
    ratio = clips[2][s:e].astype(np.float64) / e1
    assert np.allclose(ratio[np.abs(e1) > 1e-3], np.median(ratio), rtol=1e-5)
    assert -1.0 / 1.1 <= e4.min() < 0 < e4.max() and abs(e4.max() + e4.min()) < 0.03 * e4.max() + 0.03
    # the files are what OverlayBatches makes from the same pools under the same seed
    pool = mixing.ClipPool.from_files(paths, 16000, DEV)
    npool = mixing.ClipPool.from_files(mixing.read_noise_csv(str(noise_csv), str(root)), 16000, DEV, trim=False)
    ob = mixing.OverlayBatches(pool, npool, triplets, torch.zeros(len(pool), 1, device=DEV), acfg, None, seed=3, batch=16, drop_last=False)
    made = {}
    for it in ob.items(range(2)):
        for row, (t, k) in enumerate(zip(it["item_trip"].tolist(), it["item_kind"].tolist())):
            made[(numbers[int(it["plan"].positions[t])], k)] = (it["mixed_wav"][row].cpu().numpy(), it["target_wav"][row].cpu().numpy())
    assert sorted(made) == [(n, k) for n in (0, 2) for k in (1, 2, 3, 4)]
    for (n, k), (m, t) in made.items():
        assert np.array_equal(wavfile.read(str(out / "train" / f"{n:06d}_{k}-mixed.wav"))[1], m)
        assert np.array_equal(wavfile.read(str(out / "train" / f"{n:06d}_{k}-target.wav"))[1], t)
