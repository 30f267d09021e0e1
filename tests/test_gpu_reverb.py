"""GPU: csrc/reverb.hip against the fp64 restatements of tests/reverb_ref.py -- the image-method responses (vs_rir_shoebox), the
per-row FIR in both arithmetics (vs_fir_rows), the row energies, and the reverberant batches of mixing.MixtureBatches.  Every
maximum is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

import reverb_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- room responses ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rir_case():
    rooms = RR.gpu_test_rooms()
    d_abs, d_rel, href = RR.d_ref(rooms)
    return rooms, d_abs, d_rel, href


def test_rir_equals_the_restatement(rir_case):
    """Per tap: |h - h_ref| <= 64 d_ref + 2^-24 |h_ref| (d_ref: the distance of the two fp64 forms; 2^-24: the one rounding to fp32)."""
    from voicesplit_amd import reverb
    rooms, d_abs, d_rel, href = rir_case
    assert d_rel < 1e-12
    h = reverb.shoebox_rir(torch.from_numpy(rooms), DEV).cpu().numpy().astype(np.float64)
    assert h.shape == (5, 512)
    worst = 0.0
    for r, ref in enumerate(href):
        nh = len(ref)
        tol = 64.0 * d_abs + 2.0 ** -24 * np.abs(ref)
        err = np.abs(h[r, :nh] - ref)
        worst = max(worst, float((err / tol).max()))
        print(f"room {r}: nh {nh}, max |h| {np.abs(ref).max():.3e}, max err {err.max():.3e}, worst fraction of the bound {(err / tol).max():.3f}")
        assert np.all(err <= tol), (r, int(np.argmax(err / tol)))
        assert not h[r, nh:].any()                                                   # the row behind nh is zero
    print(f"d_ref {d_abs:.3e} ({d_rel:.3e} of max |h|); worst fraction of the bound {worst:.3f}")


def test_rir_bits_depend_on_the_descriptor_alone(rir_case):
    from voicesplit_amd import reverb
    rooms = torch.from_numpy(rir_case[0])
    h = reverb.shoebox_rir(rooms, DEV)
    assert torch.equal(h, reverb.shoebox_rir(rooms, DEV))                            # the call
    back = reverb.shoebox_rir(rooms.flip(0).contiguous(), DEV)                       # the row
    assert torch.equal(back.flip(0), h)
    for r in (0, 2, 4):                                                              # R, and a wider row of taps
        alone = reverb.shoebox_rir(rooms[r:r + 1].contiguous(), DEV, H=600)
        nh = int(rooms[r, 17])
        assert torch.equal(alone[0, :nh], h[r, :nh]) and not alone[0, nh:].any()


# ---- the FIR ---------------------------------------------------------------------------------------------------------------------------
TOTAL = 9000
FILTERS = (1, 31, 32, 33, 200, 2049)


@pytest.fixture(scope="module")
def fir_case():
    rng = np.random.default_rng(5)
    flat = (0.1 * rng.standard_normal(TOTAL)).astype(np.float32)
    h = np.zeros((len(FILTERS), 2049), dtype=np.float32)
    for r, n in enumerate(FILTERS):
        h[r, :n] = (rng.standard_normal(n) * np.exp(-np.arange(n) / 300.0)).astype(np.float32)
    return flat, h, torch.from_numpy(flat).to(DEV), torch.from_numpy(h).to(DEV)


def _rows(L, group):
    """three rows: an odd start with history back to sample 7; no history (lo = at, odd); the row that ends with the buffer, with
    100 samples of history"""
    at = [2051, 4403, TOTAL - L]
    lo = [7, 4403, TOTAL - L - 100]
    hrow = [0, 3, 5] if group == 0 else [1, 2, 4]
    return at, lo, hrow, [FILTERS[r] for r in hrow]


def _run(case, at, lo, hrow, nh, L, math_name, flat_dev=None):
    from voicesplit_amd import reverb
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    return reverb.fir_rows(case[2] if flat_dev is None else flat_dev, dev(at, torch.int64), dev(lo, torch.int64), dev(nh, torch.int32),
                           dev(hrow, torch.int32), case[3], L, math_name)


@pytest.mark.parametrize("math_name", ["f16x3", "fp32"])
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("L", [32, 1000, 1600])
def test_fir_is_within_the_contracts_bound(fir_case, L, group, math_name):
    """f16x3: |y - y64| <= (2^-20 + (nh + 32) 2^-23) sum_k |h_k| |x_{n-k}| + u, u = nh 2^-38 max|x| max|h| (the header's formula),
    and u <= nh 2^-30 max|h| max|x|; fp32: nh 2^-24 sum |h| |x|."""
    flat, h = fir_case[0], fir_case[1]
    at, lo, hrow, nh = _rows(L, group)
    y, valid, scale = _run(fir_case, at, lo, hrow, nh, L, math_name)
    assert valid.tolist() == [1, 1, 1] and y.shape == (3, L)
    y = y.cpu().numpy().astype(np.float64)
    for b in range(3):
        ref, mag, mx, mh = RR.fir(flat, at[b], lo[b], L, h[hrow[b]], nh[b])
        bound, u = RR.fir_bound(mag, nh[b], mx, mh, math_name)
        err = np.abs(y[b] - ref)
        frac = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{math_name} L {L} nh {nh[b]} at {at[b]} lo {lo[b]}: max err {err.max():.3e}, max |y| {np.abs(ref).max():.3e}, "
              f"u {u:.3e}, worst fraction of the bound {frac:.3f}")
        assert u <= nh[b] * 2.0 ** -30 * mh * mx
        assert np.all(err <= bound), (b, int(np.argmax(err - bound)))
        if math_name == "f16x3":                                                     # the scales the header states
            sx, isx, sh, ish = scale[b].tolist()
            assert 2.0 ** 14 <= mx * sx < 2.0 ** 15 and 2.0 ** 14 <= mh * sh < 2.0 ** 15 and sx * isx == 1.0 and sh * ish == 1.0


def test_fir_keeps_the_lo_plane():
    """x = 1 + 2^-13 everywhere, h = {1}: the hi plane alone holds 1 (an error of 1.2e-4); the bound is
    (2^-20 + 33 2^-23) |x| + u, about 5e-6."""
    from voicesplit_amd import reverb
    x = torch.full((2, 700), 1.0 + 2.0 ** -13, dtype=torch.float32, device=DEV)
    y = reverb.apply(x, torch.ones(2, 1, device=DEV), math="f16x3")
    err = float((y.double() - x.double()).abs().max())
    xv = 1.0 + 2.0 ** -13
    bound = (2.0 ** -20 + 33 * 2.0 ** -23) * xv + 2.0 ** -38 * xv
    print(f"lo plane: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound < 6e-6


@pytest.mark.parametrize("L", [32, 1000, 1600])
def test_fp32_arm_with_one_tap_returns_x_bit_for_bit(fir_case, L):
    at, lo = [2051, 4403, TOTAL - L], [7, 4403, TOTAL - L - 100]
    one = (None, None, fir_case[2], torch.ones(1, 1, device=DEV))                     # h = {1.0f}
    y, valid, _ = _run(one, at, lo, [0, 0, 0], [1, 1, 1], L, "fp32")
    want = torch.stack([fir_case[2][a:a + L] for a in at])
    assert valid.tolist() == [1, 1, 1] and torch.equal(y, want)


@pytest.mark.parametrize("math_name", ["f16x3", "fp32"])
def test_fir_bits_do_not_depend_on_row_batch_alignment_or_call(fir_case, math_name):
    L = 1000
    at, lo, hrow, nh = _rows(L, 0)
    at[2], lo[2] = 6001, 5901                                                        # room behind it for the shifted copy
    y, _, _ = _run(fir_case, at, lo, hrow, nh, L, math_name)
    again, _, _ = _run(fir_case, at, lo, hrow, nh, L, math_name)
    assert torch.equal(y, again)                                                     # the call
    order = [2, 0, 1]
    perm, _, _ = _run(fir_case, *[[v[k] for k in order] for v in (at, lo, hrow, nh)], L, math_name)
    assert torch.equal(perm, y[order])                                               # the row
    for b in range(3):                                                               # the batch size
        alone, _, _ = _run(fir_case, [at[b]], [lo[b]], [hrow[b]], [nh[b]], L, math_name)
        assert torch.equal(alone[0], y[b])
    # the same samples three samples further on in another buffer: another at mod 8, and other neighbours
    moved = torch.cat((torch.full((3,), 9.0, device=DEV), fir_case[2])).contiguous()
    shifted, _, _ = _run(fir_case, [a + 3 for a in at], [v + 3 for v in lo], hrow, nh, L, math_name, flat_dev=moved)
    assert torch.equal(shifted, y)
    # the samples below lo do not show: poison them
    dirty = fir_case[2].clone()
    dirty[:lo[0]] = 1e6
    dirty[at[0] + L:at[1]] = -1e6                                                    # and those behind the row
    clean_rows, _, _ = _run(fir_case, at[:2], lo[:2], hrow[:2], nh[:2], L, math_name, flat_dev=dirty)
    assert torch.equal(clean_rows, y[:2])


@pytest.mark.parametrize("math_name", ["f16x3", "fp32"])
@pytest.mark.parametrize("loud", [1e3, 1e6])
def test_fir_ignores_loud_samples_between_lo_and_its_window(fir_case, loud, math_name):
    """lo < at - nh + 1: the samples in [lo, at - nh + 1) belong to the clip but to no product of the row.  The split-f16 scale is
    taken over the window alone, so samples there that are 1e3 .. 1e6 times the window's maximum must neither overflow an f16 plane
    (the last tap block runs up to 61 zero taps past nh) nor show in a bit; the contract's bound holds for both arms."""
    L = 700
    hrow = [1, 3, 4, 0, 5]
    nh = [FILTERS[r] for r in hrow]                                                  # 31, 33, 200, 1, 2049
    at = [501, 2051, 4000, 4803, 7999]                                               # no window holds another row's loud samples
    lo = [7, 1500, 3500, 4403, 5700]
    flat = fir_case[0].copy()
    for a, n in zip(at, nh):
        first = a - (n - 1)
        peak = float(np.abs(flat[first:a + L]).max())
        flat[first - 70:first] = loud * peak * np.where(np.arange(70) % 2, -1.0, 1.0)  # the 70 samples in front of every window
    dirty = torch.from_numpy(flat).to(DEV)
    y, valid, _ = _run(fir_case, at, lo, hrow, nh, L, math_name, flat_dev=dirty)
    assert valid.tolist() == [1] * 5 and bool(torch.isfinite(y).all())
    clean, _, _ = _run(fir_case, at, lo, hrow, nh, L, math_name)
    assert torch.equal(y, clean)
    yn = y.cpu().numpy().astype(np.float64)
    for b in range(5):
        ref, mag, mx, mh = RR.fir(flat, at[b], lo[b], L, fir_case[1][hrow[b]], nh[b])
        bound, _ = RR.fir_bound(mag, nh[b], mx, mh, math_name)
        err = np.abs(yn[b] - ref)
        print(f"{math_name} loud {loud:g} nh {nh[b]}: max err {err.max():.3e}, worst fraction of the bound {(err / bound).max():.3f}")
        assert np.all(err <= bound), (b, int(np.argmax(err - bound)))


@pytest.mark.parametrize("math_name", ["f16x3", "fp32"])
def test_fir_marks_rows_that_leave_the_buffer_and_reads_nothing_of_them(fir_case, math_name):
    L = 1000
    at = [2051, TOTAL - L + 1, 3000, 3000, 3000, -5]
    lo = [7, 0, 3001, 3000, 3000, -5]
    hrow = [0, 0, 0, 6, 0, 0]
    nh = [1, 1, 1, 1, 2050, 1]
    y, valid, _ = _run(fir_case, at, lo, hrow, nh, L, math_name)
    assert valid.tolist() == [1, -1, -1, -1, -1, -1]
    assert not y[1:].any() and y[0].abs().max() > 0
    ok, _, _ = _run(fir_case, at[:1], lo[:1], hrow[:1], nh[:1], L, math_name)
    assert torch.equal(ok[0], y[0])


def test_row_energy_is_the_fp64_sum_and_repeats():
    from voicesplit_amd import reverb
    rng = np.random.default_rng(2)
    y = rng.standard_normal((5, 1601)).astype(np.float32)
    y[3] = 0.0
    yd = torch.from_numpy(y).to(DEV)
    e = reverb.row_energy(yd)
    want = (y.astype(np.float64) ** 2).sum(axis=1)
    rel = np.abs(e.cpu().numpy() - want) / np.maximum(want, 1e-300)
    print(f"row energy: max relative distance from numpy's fp64 sum {rel.max():.3e} (bound 1601 * 2^-53)")
    assert e.dtype == torch.float64 and np.all(rel <= 1601 * 2.0 ** -53) and float(e[3]) == 0.0
    assert torch.equal(e, reverb.row_energy(yd)) and torch.equal(reverb.row_energy(yd[1:3].contiguous()), e[1:3])


# ---- batches ---------------------------------------------------------------------------------------------------------------------------
def _small_cfg():
    import voicesplit_amd as V
    dims = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
    c = V.default_config(**dims)
    c.audio["voicefilter"].update({"hop_length": 16, "win_length": 40})
    return c, dims


@pytest.fixture(scope="module")
def batch_case():
    from voicesplit_amd import mixing
    from voicesplit_amd.trainer import EpochShard
    c, dims = _small_cfg()
    acfg = c.audio["voicefilter"]
    rng = np.random.default_rng(3)
    clips = []
    for k in range(7):
        m = 1500 + 211 * k
        y = (1e-4 * rng.standard_normal(m)).astype(np.float32)
        y[200 + 37 * k:m - 150] += (0.2 * rng.standard_normal(m - 350 - 37 * k)).astype(np.float32)
        clips.append(torch.from_numpy(y))
    pool = mixing.ClipPool(clips, DEV)
    T, B = 11, 3
    L = acfg["hop_length"] * (T - 1)
    triplets = [(a, (a + 1) % 7, (a + 3) % 7) for a in range(7)] + [(a, a, (a + 2) % 7) for a in range(7)]
    kept, dropped = mixing.plan_triplets(pool, triplets, L)
    assert dropped == 0
    table = torch.randn(len(pool), dims["emb_dim"], generator=torch.Generator().manual_seed(2)).to(DEV)
    shard = EpochShard(len(kept), B, seed=4)
    return dict(pool=pool, kept=kept, table=table, acfg=acfg, audio_len=L / acfg["sample_rate"], shard=shard, L=L, B=B)


def _batches(case, **kw):
    from voicesplit_amd import mixing
    return mixing.MixtureBatches(case["pool"], case["kept"], case["table"], case["acfg"], case["audio_len"], case["shard"], **kw)


ITEM_KEYS = ("emb", "target", "mixed", "seq_len", "target_wav", "phase", "mixed_wav", "norm", "valid", "positions")


def test_unit_impulses_in_fp32_give_the_present_batches_bit_for_bit(batch_case):
    from voicesplit_amd import reverb
    order = list(batch_case["shard"].epoch(1))
    for history in ("clip", "zero"):
        plain = list(_batches(batch_case, crop="random", seed=9).items(order, 1))
        room = list(_batches(batch_case, crop="random", seed=9, rir_pool=reverb.RirPool.impulses(DEV), math="fp32",
                             history=history).items(order, 1))
        assert len(plain) == len(room) == 4
        for a, b in zip(plain, room):
            assert "rows" in b and "rows" not in a
            for k in ITEM_KEYS:
                assert torch.equal(a[k], b[k]), k


def test_crops_are_the_same_with_and_without_the_pool(batch_case):
    from voicesplit_amd import reverb
    order = list(batch_case["shard"].epoch(2))
    pool = reverb.RirPool(3, DEV, seed=9, nh=120)
    a = _batches(batch_case, crop="random", seed=9)
    b = _batches(batch_case, crop="random", seed=9, rir_pool=pool, sir_db=(0.0, 10.0))
    for x, y in zip(a.plan(order, 2), b.plan(order, 2)):
        assert torch.equal(x, y)
    assert not torch.equal(a.plan(order, 2)[1], a.plan(order, 3)[1])                 # and they are random crops
    # the draws beside them repeat, and the pool of another epoch holds other rooms
    i1, i2 = list(b.items(order, 2)), list(_batches(batch_case, crop="random", seed=9, rir_pool=pool, sir_db=(0.0, 10.0)).items(order, 2))
    assert all(torch.equal(p[k], q[k]) for p, q in zip(i1, i2) for k in ITEM_KEYS)
    assert b.rir_pool.epoch == 2 and not torch.equal(b.rir_pool.rooms, pool.rooms) and torch.equal(pool.redraw(0).h, pool.h)


@pytest.mark.parametrize("history,target,sir_db", [("clip", "reverberant", (2.0, 9.0)), ("zero", "early", None), ("clip", "early", (-3.0, 3.0))])
def test_reverberant_batches_equal_the_restatement(batch_case, history, target, sir_db):
    """Every wav of the batch against reverb_ref.batch under the FIR bound carried through gain, sum, maximum and division; the
    spectrograms are those of the wavs (the STFT has tests of its own)."""
    from voicesplit_amd import audio, reverb
    rooms, _ = reverb.draw_rooms(3, torch.Generator().manual_seed(11), nh=300)
    rooms[1::2, 17] = 171                                                            # the interferers' responses are shorter
    pool = reverb.RirPool.from_rooms(rooms, DEV)
    mb = _batches(batch_case, crop="random", seed=5, rir_pool=pool, sir_db=sir_db, history=history, target=target)
    order = list(batch_case["shard"].epoch(0))
    pos, at, _ = mb.plan(order, 0)
    room, sir = reverb.item_draws(5, 0, 0, pos.numel(), 3, sir_db)
    assert len(set(room.tolist())) > 1
    hrow = torch.stack((2 * room, 2 * room + 1))
    nh = pool.nh_host[hrow]
    lo = mb.start[pos].t() if history == "clip" else at
    flat, h, L, B = batch_case["pool"].flat.cpu().numpy(), pool.h.cpu().numpy(), batch_case["L"], batch_case["B"]
    worst = {"mixed": 0.0, "target": 0.0, "norm": 0.0}
    for k, it in enumerate(mb.items(order, 0)):
        s = slice(k * B, (k + 1) * B)
        ref = RR.batch(flat, at[:, s].tolist(), lo[:, s].tolist(), hrow[:, s].tolist(), nh[:, s].tolist(), h, L,
                       None if sir_db is None else sir[s].tolist(), pool.nh_early_host[hrow[0, s]].tolist() if target == "early" else None)
        assert it["valid"].tolist() == [1] * B and it["positions"].tolist() == order[k]
        for b, r in enumerate(ref):
            for key, got in (("mixed", it["mixed_wav"][b]), ("target", it["target_wav"][b])):
                err = np.abs(got.cpu().numpy().astype(np.float64) - r[key])
                worst[key] = max(worst[key], float((err / r["err_" + key]).max()))
                assert np.all(err <= r["err_" + key]), (k, b, key, float(err.max()))
            worst["norm"] = max(worst["norm"], abs(float(it["norm"][b]) - r["norm"]) / r["err_norm"])
            assert abs(float(it["norm"][b]) - r["norm"]) <= r["err_norm"]
            if sir_db is not None:
                rows = it["rows"].double()
                ratio = 10.0 * math.log10(float(rows[b].pow(2).sum()) / float(rows[B + b].pow(2).sum()))
                assert abs(ratio - float(sir[s][b])) < 1e-5
        spec, ph = audio.wav_to_spec(it["mixed_wav"], batch_case["acfg"], want_phase=True)
        assert torch.equal(it["mixed"], spec) and torch.equal(it["phase"], ph)
        assert torch.equal(it["target"], audio.wav_to_spec(it["target_wav"], batch_case["acfg"], want_phase=False)[0])
        assert torch.equal(it["emb"], batch_case["table"][[batch_case["kept"][p][1] for p in order[k]]])
    print(f"{history} {target} sir {sir_db}: worst fraction of the carried bound {worst}")
    assert mb.invalid_items == 0


def test_a_fixed_ratio_is_met_within_1e_5_db(batch_case):
    """sir_db = (5, 5): the fp64 energy ratio of the clean row and the scaled interferer row is 5 dB within 1e-5 dB, with a real pool
    and with none (unit impulses)."""
    from voicesplit_amd import reverb
    order = list(batch_case["shard"].epoch(0))
    B = batch_case["B"]
    for pool in (None, reverb.RirPool(2, DEV, seed=1, nh=200)):
        worst = 0.0
        for it in _batches(batch_case, rir_pool=pool, sir_db=(5.0, 5.0)).items(order, 0):
            rows = it["rows"].double()
            ratio = 10.0 * torch.log10(rows[:B].pow(2).sum(dim=1) / rows[B:].pow(2).sum(dim=1))
            worst = max(worst, float((ratio - 5.0).abs().max()))
            assert it["valid"].tolist() == [1] * B
        print(f"sir 5 dB, pool {'drawn' if pool is not None else 'of unit impulses'}: worst distance {worst:.3e} dB (bound 1e-5)")
        assert worst < 1e-5
