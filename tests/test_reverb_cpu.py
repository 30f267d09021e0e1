"""CPU: the reverberation contract of include/voicesplit_hip.h without a device -- the two fp64 restatements of the image sum
(tests/reverb_ref.py) against each other and against the closed forms of one and two arrivals, the room draw, the FIR restatement
against its GEMM form, what the entries refuse before any launch, the ABI, and the signature of MixtureBatches."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import reverb_ref as RR
from conftest import ROOT


def _room(src, mic, beta, nh=400, order=-1, size=(4.0, 3.0, 2.5)):
    beta = [beta] * 6 if isinstance(beta, float) else list(beta)
    return np.array([*size, *src, *mic, *beta, 343.0, 16000.0, nh, order], dtype=np.float64)


# ---- the image sum ---------------------------------------------------------------------------------------------------------------------
def test_the_two_image_forms_agree_on_the_gpu_test_rooms():
    """d_ref: the distance of the two differently ordered, differently evaluated fp64 sums; the yardstick of tests/test_gpu_reverb.py."""
    worst, worst_rel, hs = RR.d_ref(RR.gpu_test_rooms())
    print(f"d_ref = {worst:.3e} absolute, {worst_rel:.3e} of max |h| (bound 1e-12)")
    assert worst_rel < 1e-12
    assert all(np.abs(h).max() > 1e-4 for h in hs)                                   # every response has something in it
    counts = [RR.rir_loop(r, count=True)[1] for r in RR.gpu_test_rooms()]
    print("images that reach a tap:", counts)
    assert counts[0] > 200 and counts[3] == 1


def test_window_is_the_contracts():
    assert RR.window(0.0) == 1.0 and RR.window(40.0) == 0.0 and RR.window(-40.0) == 0.0 and RR.window(39.999) != 0.0
    u = np.array([0.5, -0.5, 1.0, 7.25])
    want = np.sin(np.pi * u) / (np.pi * u) * 0.5 * (1.0 + np.cos(np.pi * u / 40.0))
    assert np.allclose(RR.window(u), want, rtol=1e-15, atol=1e-17)


def test_anechoic_room_is_one_image():
    src, mic = (1.0, 2.0, 1.5), (3.1, 0.9, 1.1)
    room = _room(src, mic, 0.0)
    h, used = RR.rir_loop(room, count=True)
    assert used == 1
    d = math.dist(src, mic)
    want = RR.window(np.arange(400.0) - d * 16000.0 / 343.0) / (4.0 * math.pi * d)
    assert np.abs(h - want).max() <= 1e-16 and np.abs(RR.rir_by_delay(room) - want).max() <= 1e-15


@pytest.mark.parametrize("wall", [0, 1])
def test_one_reflective_wall_gives_two_arrivals(wall):
    """Only x0 (wall 0) or x1 (wall 1) reflects: the direct path and the source mirrored at -s_x or at 2 L_x - s_x, each with its own
    delay and amplitude (the mirrored one times beta)."""
    src, mic, size = (1.0, 2.0, 1.5), (3.1, 0.9, 1.1), (4.0, 3.0, 2.5)
    beta = [0.0] * 6
    beta[wall] = 0.7
    room = _room(src, mic, beta, size=size)
    h, used = RR.rir_loop(room, count=True)
    assert used == 2
    mirrored = (-src[0] if wall == 0 else 2.0 * size[0] - src[0], src[1], src[2])
    t = np.arange(400.0)
    want = np.zeros(400)
    for pos, gain in ((src, 1.0), (mirrored, 0.7)):
        d = math.dist(pos, mic)
        want += gain * RR.window(t - d * 16000.0 / 343.0) / (4.0 * math.pi * d)
    assert np.abs(h - want).max() <= 1e-16 and np.abs(RR.rir_by_delay(room) - want).max() <= 1e-15
    peaks = sorted(int(round(math.dist(p, mic) * 16000.0 / 343.0)) for p in (src, mirrored))
    assert abs(h[peaks[0]]) > 0.01 and abs(h[peaks[1]]) > 0.005


def test_max_order_drops_images():
    room = RR.gpu_test_rooms()[0]
    full = RR.rir_loop(room)
    for order in (0, 2):
        cut = room.copy()
        cut[18] = order
        h, used = RR.rir_loop(cut, count=True)
        assert used == (1 if order == 0 else 25) and np.abs(h - full).max() > 1e-4
    # up to the first reflection every order holds the direct path alone
    first = int(math.dist(room[3:6], room[6:9]) * 16000.0 / 343.0) + 41
    cut = room.copy()
    cut[18] = 0
    assert np.abs(RR.rir_loop(cut)[:first] - full[:first]).max() < 0.02 * np.abs(full).max()


# ---- the FIR restatement ---------------------------------------------------------------------------------------------------------------
def test_fir_restatement_equals_the_gemm_form_and_honours_lo():
    """Out[a][i] = sum_c sum_j X[a - c][j] G_c[j][i], G_c[j][i] = h[32 c + i - j]: the form the matrix-core kernel computes."""
    rng = np.random.default_rng(0)
    flat = rng.standard_normal(900).astype(np.float32)
    h = rng.standard_normal(70).astype(np.float32)
    at, lo, L, nh, P = 301, 250, 96, 67, 32
    y, mag, mx, mh = RR.fir(flat, at, lo, L, h, nh)
    x = lambda p: float(flat[p]) if p >= lo else 0.0
    direct = np.array([sum(float(h[k]) * x(at + i - k) for k in range(nh)) for i in range(L)])
    assert np.abs(y - direct).max() < 1e-13
    out = np.zeros((L // P, P))
    hz = lambda k: float(h[k]) if 0 <= k < nh else 0.0
    for a in range(L // P):
        for c in range((nh + P - 2) // P + 1):
            X = np.array([x(at + (a - c) * P + j) for j in range(P)])
            G = np.array([[hz(c * P + i - j) for i in range(P)] for j in range(P)])
            out[a] += X @ G
    assert np.abs(out.reshape(-1) - direct).max() < 1e-13
    assert mx == np.abs(flat[lo:at + L]).max() and mh == np.abs(h[:nh]).max() and np.all(mag >= np.abs(y) - 1e-12)
    bound, u = RR.fir_bound(mag, nh, mx, mh, "f16x3")
    assert u == nh * 2.0 ** -38 * mx * mh <= nh * 2.0 ** -30 * mx * mh


# ---- the room draw ---------------------------------------------------------------------------------------------------------------------
def test_draw_rooms_is_reproducible_inside_its_margins_and_leaves_the_crop_stream_alone():
    from voicesplit_amd import mixing, reverb
    seed = mixing.crop_seed(3, 1, 0)
    rooms, rt60 = reverb.draw_rooms(40, torch.Generator().manual_seed(seed ^ reverb.POOL_SALT))
    again, _ = reverb.draw_rooms(40, torch.Generator().manual_seed(seed ^ reverb.POOL_SALT))
    assert torch.equal(rooms, again) and rooms.shape == (80, 19) and rooms.dtype == torch.float64
    U = torch.rand(40, reverb.DRAWS_PER_ROOM, dtype=torch.float64, generator=torch.Generator().manual_seed(seed ^ reverb.POOL_SALT))
    want, want_rt = RR.draw_rooms(U.numpy())
    assert np.abs(rooms.numpy() - want).max() <= 1e-12 and np.abs(rt60.numpy() - want_rt).max() <= 1e-15
    r = rooms.numpy()
    size, src, mic = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    assert np.all(size >= [3.0, 3.0, 2.4]) and np.all(size <= [8.0, 6.0, 3.5])
    assert np.all(mic >= 0.5) and np.all(mic <= size - 0.5) and np.all(src >= 0.5 - 1e-12) and np.all(src <= size - 0.5 + 1e-12)
    assert np.array_equal(r[0::2, 0:3], r[1::2, 0:3]) and np.array_equal(r[0::2, 6:9], r[1::2, 6:9])      # one receiver, two sources
    assert not np.array_equal(r[0::2, 3:6], r[1::2, 3:6])
    dist = np.linalg.norm(src - mic, axis=1)
    assert np.all(dist > 0) and np.all(dist <= 3.0 + 1e-12)
    assert np.all((rt60.numpy() >= 0.15) & (rt60.numpy() <= 0.5))
    nh = np.minimum(8192, np.ceil(np.repeat(rt60.numpy(), 2) * 16000)).astype(int)
    assert np.array_equal(r[:, 17].astype(int), nh) and np.all(r[:, 18] == -1)
    for k in (0, 17, 39):
        beta = reverb.sabine_beta(size[2 * k], float(rt60[k]))
        assert np.all(r[2 * k, 9:15] == beta) and beta == RR.sabine_beta(size[2 * k], float(rt60[k])) and 0.1 <= beta < 1.0
    # Sabine by hand: 5 x 4 x 3 m, rt60 0.4 s: alpha = 0.161 * 60 / (94 * 0.4)
    assert abs(reverb.sabine_beta((5.0, 4.0, 3.0), 0.4) - math.sqrt(1.0 - 0.161 * 60.0 / 37.6)) < 1e-15
    assert reverb.sabine_beta((5.0, 4.0, 3.0), 1e-3) == math.sqrt(1.0 - 0.99) and reverb.sabine_beta((5.0, 4.0, 3.0), 1e3) == math.sqrt(0.99)
    # the crop generator: the same crops whether or not rooms, responses and levels are drawn beside them
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([[100, 7], [0, 900], [33, 33]], dtype=torch.int64)
    crops = mixing.crop_offsets(room, "random", g)
    g2 = torch.Generator().manual_seed(seed)
    picks, sir = reverb.item_draws(3, 1, 0, 3, 40, (0.0, 10.0))
    assert torch.equal(mixing.crop_offsets(room, "random", g2), crops)
    assert picks.shape == (3,) and int(picks.min()) >= 0 and int(picks.max()) < 40 and float(sir.min()) >= 0.0 and float(sir.max()) <= 10.0
    p2, s2 = reverb.item_draws(3, 1, 0, 3, 40, (0.0, 10.0))
    assert torch.equal(picks, p2) and torch.equal(sir, s2)
    assert float(reverb.item_draws(3, 1, 0, 3, 40, None)[1].abs().max()) == 0.0
    for bad in (dict(size=((0.9, 3, 3), (4, 4, 4))), dict(rt60=(0.0, 0.3)), dict(distance=(2.0, 1.0)), dict(nh=8193)):
        with pytest.raises(ValueError):
            reverb.draw_rooms(2, torch.Generator().manual_seed(0), **bad)


def test_early_taps_follow_the_direct_path():
    from voicesplit_amd import reverb
    rooms = torch.from_numpy(RR.gpu_test_rooms())
    delay = reverb.direct_delay(rooms)
    want = [math.dist(r[3:6], r[6:9]) * 16000.0 / 343.0 for r in RR.gpu_test_rooms()]
    assert np.allclose(delay.numpy(), want, rtol=1e-15)
    assert reverb.early_taps(rooms).tolist() == [min(int(r[17]), int(w) + 1 + 800) for r, w in zip(RR.gpu_test_rooms(), want)]


# ---- header, ctypes, ABI ---------------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_abi_11():
    from voicesplit_amd import _lib
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    assert re.search(r"#define VS_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11 and _lib.load().vs_abi_version() == 11
    for name in ("vs_rir_shoebox", "vs_fir_rows", "vs_row_energy"):
        assert re.search(r"\bint " + name + r"\(", text) and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    said = re.sub(r"\s*\n \*\s*", " ", text).lower()
    assert "restated (allen & berkley 1979), not compared with a pyroomacoustics or rir-generator run" in said
    # the record: 17 doubles and two ints, no padding
    assert ctypes.sizeof(_lib.VsRoom) == 17 * 8 + 8
    assert [f[0] for f in _lib.VsRoom._fields_] == ["size", "src", "mic", "beta", "c", "fs", "nh", "max_order"]
    body = re.search(r"typedef struct vs_room \{(.*?)\} vs_room;", text, flags=re.S).group(1)
    assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).split() == \
        "double size[3], src[3], mic[3]; double beta[6]; double c, fs; int nh, max_order;".split()


# ---- refusals, with no device ----------------------------------------------------------------------------------------------------------
def _shoebox_rc(row, H=8192):
    from voicesplit_amd import _lib, reverb
    lib = _lib.load()
    arr = reverb.room_structs(torch.from_numpy(np.asarray(row, dtype=np.float64)[None]))
    dummy = ctypes.c_void_p(4096)                         # never dereferenced: every call below is refused on the host
    return lib.vs_rir_shoebox(arr, dummy, 1, H, dummy, None), lib.vs_last_error()


def test_shoebox_refuses_bad_descriptors_before_any_launch():
    good = RR.gpu_test_rooms()[0]
    cases = []
    for idx, value, text in ((0, 0.0, b"must be positive"), (1, -2.5, b"must be positive"), (3, 3.0, b"source is outside"),
                             (4, -0.1, b"source is outside"), (8, 2.2, b"receiver is outside"), (9, 1.5, b"beta[0]"),
                             (14, float("nan"), b"beta[5]"), (15, 0.0, b"c = 0"), (16, -16000.0, b"fs = -16000"),
                             (17, 0, b"nh = 0"), (17, 8193, b"nh = 8193"), (18, -2, b"max_order = -2")):
        row = good.copy()
        row[idx] = value
        cases.append((row, text))
    same = good.copy()
    same[3:6] = same[6:9]
    cases.append((same, b"d = 0"))
    tiny = good.copy()
    tiny[0:3], tiny[3:6], tiny[6:9], tiny[17] = 0.05, 0.02, 0.03, 8192
    cases.append((tiny, b"too small for 8192 taps"))
    for row, text in cases:
        rc, msg = _shoebox_rc(row)
        assert rc == -1 and text in msg, (text, msg)
    rc, msg = _shoebox_rc(good, H=256)                     # nh = 512 does not fit the rows
    assert rc == -1 and b"nh = 512" in msg
    from voicesplit_amd import _lib
    lib, p = _lib.load(), ctypes.c_void_p(4096)
    assert lib.vs_rir_shoebox(None, p, 1, 64, p, None) == -1 and b"NULL" in lib.vs_last_error()
    assert lib.vs_rir_shoebox(p, p, 0, 64, p, None) == -1 and b"R=0" in lib.vs_last_error()
    assert lib.vs_rir_shoebox(p, p, 1, 8193, p, None) == -1 and b"H=8193" in lib.vs_last_error()


def test_fir_rows_and_row_energy_refuse_bad_arguments_before_any_launch():
    from voicesplit_amd import _lib
    lib, p = _lib.load(), ctypes.c_void_p(4096)

    def fir(total=1000, B=2, L=100, R=1, H=64, math=1, samples=p, y=p):
        return lib.vs_fir_rows(samples, total, p, p, p, p, B, L, p, R, H, math, y, p, p, None), lib.vs_last_error()

    for kw, text in ((dict(math=2), b"math=2"), (dict(math=7), b"math=7"), (dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"),
                     (dict(L=0), b"L=0"), (dict(L=(1 << 24) + 1), b"L=16777217"), (dict(H=0), b"H=0"), (dict(H=8193), b"H=8193"),
                     (dict(R=0), b"R=0"), (dict(total=99), b"buffer of 99 samples"), (dict(samples=None), b"NULL"), (dict(y=None), b"NULL")):
        rc, msg = fir(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert lib.vs_row_energy(None, 1, 8, p, None) == -1 and b"NULL" in lib.vs_last_error()
    assert lib.vs_row_energy(p, 0, 8, p, None) == -1 and b"B=0" in lib.vs_last_error()
    assert lib.vs_row_energy(p, 1, 0, p, None) == -1 and b"L=0" in lib.vs_last_error()


def test_python_wrappers_refuse_the_host_and_bad_tables():
    from voicesplit_amd import _lib, reverb
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        reverb.shoebox_rir(torch.from_numpy(RR.gpu_test_rooms()), device="cpu")
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        reverb.apply(torch.zeros(2, 64), torch.ones(2, 1))
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        reverb.row_energy(torch.zeros(2, 64))
    with pytest.raises(ValueError, match=r"float64 \[R, 19\]"):
        reverb.room_structs(torch.zeros(2, 18, dtype=torch.float64))
    with pytest.raises(ValueError, match="integers"):
        bad = torch.from_numpy(RR.gpu_test_rooms()[:1].copy())
        bad[0, 17] = 10.5
        reverb.room_structs(bad)
    with pytest.raises(ValueError, match="math must be"):
        reverb.fir_rows(torch.zeros(8), *([torch.zeros(1, dtype=torch.int64)] * 4), torch.ones(1, 1), 4, math="bf16")
    row = reverb.room_row((4, 3, 2.5), (1, 1, 1), (2, 2, 1.5), 0.8, nh=100)
    assert row.shape == (19,) and row[9:15].tolist() == [0.8] * 6 and row[17] == 100 and row[18] == -1 and row[15] == 343.0


# ---- MixtureBatches ---------------------------------------------------------------------------------------------------------------------
def test_mixture_batches_signature_defaults_and_argument_checks():
    from voicesplit_amd import mixing
    sig = inspect.signature(mixing.MixtureBatches.__init__)
    names = list(sig.parameters)
    assert names[:10] == ["self", "pool", "triplets", "emb_table", "audio_cfg", "audio_len", "shard", "crop", "seed", "emb_rows"]
    want = {"crop": "head", "seed": 0, "emb_rows": "clip", "rir_pool": None, "sir_db": None, "history": "clip", "target": "reverberant",
            "math": "f16x3"}
    assert {k: sig.parameters[k].default for k in want} == want
    pool = mixing.ClipPool.planned([3000, 3000], [(0, 3000), (0, 3000)])
    acfg = {"sample_rate": 16000, "hop_length": 16, "win_length": 40, "n_fft": 104, "num_freq": 53}
    args = (pool, [(0, 1, 1)], torch.zeros(2, 4), acfg, 160 / 16000, None)
    mb = mixing.MixtureBatches(*args)
    assert mb.rir_pool is None and mb.sir_db is None and mb.history == "clip" and mb.target == "reverberant"
    assert mixing.MixtureBatches(*args, sir_db=[3, 6]).sir_db == (3.0, 6.0)
    for kw in (dict(history="none"), dict(target="dry"), dict(math="bf16"), dict(sir_db=(6.0, 3.0))):
        with pytest.raises(ValueError):
            mixing.MixtureBatches(*args, **kw)


def test_command_line_flags_parse_and_default_to_no_reverberation():
    import argparse
    from voicesplit_amd import mixing
    ap = argparse.ArgumentParser()
    mixing.add_reverb_arguments(ap)
    none = ap.parse_args([])
    assert none.reverb_rooms == 0 and none.sir_db is None and tuple(none.rt60) == (0.15, 0.5)
    assert mixing.reverb_arguments(none, 16000, "cuda:0", 0) is None
    some = ap.parse_args(["--sir-db", "0", "5"])
    assert mixing.reverb_arguments(some, 16000, "cuda:0", 7) == {"sir_db": (0.0, 5.0), "seed": 7}
    full = ap.parse_args(["--reverb-rooms", "12", "--rt60", "0.2", "0.3"])
    assert full.reverb_rooms == 12 and full.rt60 == [0.2, 0.3]
