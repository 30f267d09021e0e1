"""CPU: the FFT form of the per-row FIR without a device -- the four entries in the header, the ctypes table and the library, the
ABI, what the entries and the wrappers refuse before any launch, the float32 restatement of tests/fir_fft_ref.py against the fp64
sum at a small block, the early taps of a measured response, and the new arguments of MixtureBatches and the command line."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fir_fft_ref as FR
from conftest import ROOT

ENTRIES = ("vs_fir_spectra_bytes", "vs_fir_spectra", "vs_fir_fft_workspace_bytes", "vs_fir_rows_fft")


def test_header_ctypes_library_and_abi_11():
    from voicesplit_amd import _lib, reverb
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    lib = _lib.load()
    assert re.search(r"#define VS_ABI_VERSION 11\b", text) and _lib.ABI_VERSION == 11 and lib.vs_abi_version() == 11
    for name in ENTRIES:
        assert re.search(r"\b(int|size_t) " + name + r"\(", text) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define VS_FIR_FFT_BLOCK 2048\b", text) and reverb.FFT_BLOCK == FR.BK == 2048 and reverb.MAX_TAPS_FFT == 32768
    said = re.sub(r"\s*\n \*\s*", " ", text).lower()
    for phrase in ("the bound is global to a block", "a row of zero samples gives exact zeros", "rounded once to fp32",
                   "the bytes the workspace held before", "the library keeps no lazily initialised state"):
        assert phrase in said, phrase
    assert "fir_fft.hip" in open(os.path.join(ROOT, "voicesplit_amd", "csrc", "Makefile")).read()


def test_sizes():
    from voicesplit_amd import _lib
    lib = _lib.load()
    spec = 2048 * 8
    # the twiddle table (4096 complex), the counts (a 256-byte piece), R ceil(H / Bk) packed spectra
    assert lib.vs_fir_spectra_bytes(5, 6149) == 4096 * 8 + 256 + 5 * 4 * spec
    assert lib.vs_fir_spectra_bytes(1, 1) == 4096 * 8 + 256 + spec
    assert lib.vs_fir_spectra_bytes(256, 32768) == 4096 * 8 + 1024 + 256 * 16 * spec
    # ceil(L / Bk) + ceil(H / Bk) - 1 window spectra per row
    assert lib.vs_fir_fft_workspace_bytes(3, 4113, 6149) == 3 * (3 + 4 - 1) * spec
    assert lib.vs_fir_fft_workspace_bytes(128, 48000, 32768) == 128 * (24 + 16 - 1) * spec
    for args, text in (((0, 64), b"R=0"), ((1, 0), b"H=0"), ((1, 32769), b"H=32769")):
        assert lib.vs_fir_spectra_bytes(*args) == 0 and text in lib.vs_last_error()
    for args, text in (((0, 10, 10), b"B=0"), ((65536, 10, 10), b"B=65536"), ((1, 0, 10), b"L=0"), ((1, (1 << 24) + 1, 10), b"L=16777217"),
                       ((1, 10, 0), b"H=0"), ((1, 10, 32769), b"H=32769")):
        assert lib.vs_fir_fft_workspace_bytes(*args) == 0 and text in lib.vs_last_error()


def test_entries_refuse_bad_arguments_before_any_launch():
    from voicesplit_amd import _lib
    lib, p = _lib.load(), ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on the host
    big = 1 << 40

    def rows(total=100000, B=2, L=5000, R=3, H=4000, samples=p, y=p, blob=big, ws=big, workspace=p):
        return lib.vs_fir_rows_fft(samples, total, p, p, p, B, L, p, blob, R, H, workspace, ws, y, p, None), lib.vs_last_error()

    need_blob, need_ws = lib.vs_fir_spectra_bytes(3, 4000), lib.vs_fir_fft_workspace_bytes(2, 5000, 4000)
    for kw, text in ((dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"), (dict(L=0), b"L=0"), (dict(L=(1 << 24) + 1), b"L=16777217"),
                     (dict(H=0), b"H=0"), (dict(H=32769), b"H=32769"), (dict(R=0), b"R=0"), (dict(total=4999), b"buffer of 4999 samples"),
                     (dict(samples=None), b"NULL"), (dict(y=None), b"NULL"), (dict(workspace=None), b"NULL"),
                     (dict(blob=need_blob - 1), b"blob holds %d bytes" % (need_blob - 1)),
                     (dict(ws=need_ws - 1), b"workspace holds %d bytes" % (need_ws - 1))):
        rc, msg = rows(**kw)
        assert rc == -1 and text in msg, (kw, msg)

    nh_ok = (ctypes.c_int * 3)(1, 4000, 17)

    def spectra(R=3, H=4000, h=p, nh_host=nh_ok, blob=big):
        return lib.vs_fir_spectra(h, nh_host, p, R, H, p, blob, None), lib.vs_last_error()

    for kw, text in ((dict(R=0), b"R=0"), (dict(H=0), b"H=0"), (dict(H=32769), b"H=32769"), (dict(h=None), b"NULL"), (dict(nh_host=None), b"NULL"),
                     (dict(blob=need_blob - 1), b"blob holds %d bytes" % (need_blob - 1)),
                     (dict(nh_host=(ctypes.c_int * 3)(1, 4001, 17)), b"response 1 has nh = 4001"),
                     (dict(nh_host=(ctypes.c_int * 3)(1, 4000, 0)), b"response 2 has nh = 0")):
        rc, msg = spectra(**kw)
        assert rc == -1 and text in msg, (kw, msg)


def test_python_wrappers_refuse_the_host_and_bad_tables():
    from voicesplit_amd import _lib, reverb
    z64, z32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        reverb.fir_spectra(torch.ones(2, 8), [8, 8])
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        reverb.apply(torch.zeros(2, 64), torch.ones(2, 1), math="fft")
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        reverb.RirPool.from_responses(torch.ones(2, 8), device="cpu")
    with pytest.raises(TypeError, match="fir_spectra"):
        reverb.fir_rows_fft(torch.zeros(8), z64, z64, z32, torch.ones(1, 1), 4)
    with pytest.raises(ValueError, match="math must be"):
        reverb.fir_rows(torch.zeros(8), z64, z64, z64, z64, torch.ones(1, 1), 4, math="fft")      # the direct form has no such arm
    for bad in (torch.ones(3, 8), torch.ones(2, 32769), torch.ones(2, 8, dtype=torch.float64), torch.ones(8)):
        with pytest.raises(ValueError, match="from_responses"):
            reverb.RirPool.from_responses(bad)
    for nh in ([8], [8, 9], [0, 8]):
        with pytest.raises(ValueError, match="nh is 2 integers"):
            reverb.RirPool.from_responses(torch.ones(2, 8), nh)
    with pytest.raises(ValueError, match="max_taps"):
        reverb.draw_rooms(2, torch.Generator().manual_seed(0), max_taps=8193)


def test_max_taps_cuts_the_drawn_responses_and_the_default_keeps_every_number():
    from voicesplit_amd import reverb
    g = lambda: torch.Generator().manual_seed(5)
    rooms, rt60 = reverb.draw_rooms(6, g())
    same, _ = reverb.draw_rooms(6, g(), max_taps=reverb.MAX_TAPS)
    cut, _ = reverb.draw_rooms(6, g(), max_taps=3000)
    assert torch.equal(rooms, same) and torch.equal(cut[:, :17], rooms[:, :17])
    want = np.minimum(3000, np.ceil(np.repeat(rt60.numpy(), 2) * 16000))
    assert np.array_equal(cut[:, 17].numpy(), want) and (rooms[:, 17] > 3000).any()


@pytest.mark.parametrize("nh", [1, 63, 64, 65, 197])
def test_float32_restatement_equals_the_fp64_sum_at_a_block_of_64(nh):
    """The partitioned form is the FIR: three rows (history, none, the end of the buffer) at Bk = 64, within 0.5 2^-24 log2(128) E_j
    (a CPU run of this form gave up to 0.13 at this block)."""
    rng = np.random.default_rng(nh)
    flat = (0.1 * rng.standard_normal(900)).astype(np.float32)
    h = (rng.standard_normal(200) * np.exp(-np.arange(200) / 40.0)).astype(np.float32)
    L, worst = 150, 0.0
    for at, lo in ((301, 7), (433, 433), (900 - L, 900 - L - 30)):
        y64 = FR.fir64(flat, at, lo, L, h, nh)
        y32 = FR.partitioned32(flat, at, lo, L, h, nh, Bk=64)
        E = FR.block_energy(flat, at, lo, L, h, nh, Bk=64)
        assert y32.dtype == np.float32 and y32.shape == (L,) and E.shape == (3,) and np.abs(y64).max() > 1e-3
        worst = max(worst, FR.ratio(y32, y64, E, L, 64))
    print(f"nh {nh}, Bk 64: worst |y32 - y64| / (2^-24 log2(N) E_j) = {worst:.4f}")
    assert worst <= 0.5
    # a dropped last partition is far outside
    if nh > 64:
        short = FR.partitioned32(flat, 301, 7, L, h, (nh - 1) // 64 * 64, Bk=64)
        assert FR.ratio(short, FR.fir64(flat, 301, 7, L, h, nh), FR.block_energy(flat, 301, 7, L, h, nh, Bk=64), L, 64) > 100.0


def test_kappa_ref_comes_from_the_reference_alone():
    k = FR.kappa_ref()
    print(f"kappa_ref = {k:.5f} over {sum(len(g) for g in FR.cases().values())} rows at Bk = 2048; the kernel is held to {FR.KAPPA_MARGIN * k:.5f}")
    assert 0.0 < k < 0.1 and FR.KAPPA_MARGIN == 8.0
    assert set(FR.cases()) == {(r, L) for r in range(5) for L in FR.LENGTHS} | {("long", FR.LONG_L)}
    assert FR.FILTERS == (1, 2047, 2048, 2049, 6149) and FR.LENGTHS == (1027, 4113) and (FR.LONG_NH, FR.LONG_L) == (32768, 2053)


def test_from_responses_computes_nh_early_from_a_planted_peak():
    from voicesplit_amd import reverb
    h = 0.01 * torch.randn(4, 3000, generator=torch.Generator().manual_seed(1))
    for r, peak in enumerate((0, 123, 2500, 2999)):
        h[r, peak] = -2.0 if r % 2 else 2.0
    nh = torch.tensor([3000, 3000, 2600, 2000], dtype=torch.int32)
    got = reverb.RirPool.measured_early_taps(h, nh, fs=16000)
    # argmax |h| + 1 + 800, at most nh; row 3's planted peak lies behind its nh and does not count
    assert got.dtype == torch.int32 and got[:3].tolist() == [801, 924, 2600]
    assert int(got[3]) == min(2000, int(h[3, :2000].abs().argmax()) + 801)
    assert reverb.RirPool.measured_early_taps(h, nh, fs=8000)[:2].tolist() == [401, 524]


def test_mixture_batches_takes_fft_and_still_refuses_bf16():
    from voicesplit_amd import mixing
    pool = mixing.ClipPool.planned([3000, 3000], [(0, 3000), (0, 3000)])
    acfg = {"sample_rate": 16000, "hop_length": 16, "win_length": 40, "n_fft": 104, "num_freq": 53}
    args = (pool, [(0, 1, 1)], torch.zeros(2, 4), acfg, 160 / 16000, None)
    assert mixing.MixtureBatches(*args, math="fft").math == "fft" and mixing.MixtureBatches(*args).math == "f16x3"
    with pytest.raises(ValueError, match="math must be"):
        mixing.MixtureBatches(*args, math="bf16")


def test_new_flags_parse_and_without_them_nothing_changes(tmp_path):
    from voicesplit_amd import mixing
    ap = argparse.ArgumentParser()
    mixing.add_reverb_arguments(ap)
    none = ap.parse_args([])
    assert none.reverb_csv is None and none.reverb_math is None and none.reverb_rooms == 0
    assert mixing.reverb_arguments(none, 16000, "cuda:0", 0) is None
    assert mixing.reverb_arguments(ap.parse_args(["--sir-db", "0", "5"]), 16000, "cuda:0", 7) == {"sir_db": (0.0, 5.0), "seed": 7}
    some = ap.parse_args(["--sir-db", "0", "5", "--reverb-math", "fft"])
    assert mixing.reverb_arguments(some, 16000, "cuda:0", 7) == {"sir_db": (0.0, 5.0), "seed": 7, "math": "fft"}
    with pytest.raises(SystemExit):
        ap.parse_args(["--reverb-math", "bf16"])
    listing = tmp_path / "rooms.csv"
    listing.write_text("a/t.wav, a/i.wav\n\n/abs/t.wav,b/i.wav\n")
    assert ap.parse_args(["--reverb-csv", str(listing)]).reverb_csv == str(listing)
    root = str(tmp_path)
    assert mixing.read_reverb_csv(str(listing)) == [(os.path.join(root, "a/t.wav"), os.path.join(root, "a/i.wav")),
                                                     ("/abs/t.wav", os.path.join(root, "b/i.wav"))]
    listing.write_text("only_one.wav\n")
    with pytest.raises(ValueError, match="two columns"):
        mixing.read_reverb_csv(str(listing))
    both = ap.parse_args(["--reverb-csv", str(listing), "--reverb-rooms", "3"])
    with pytest.raises(ValueError, match="give one"):
        mixing.reverb_arguments(both, 16000, "cuda:0", 0)
