"""CPU: the host half of voicesplit_amd/mixing.py -- which triplets are kept, where the crops start, the CSV's path rules, the
output file names, the C-ABI signatures of the two device operations -- and the fp64 restatement the GPU tests compare against."""
import os

import numpy as np
import pytest
import torch

import mixing_ref as MR
from voicesplit_amd import mixing
from voicesplit_amd.trainer import EpochShard

L = 1600


def _pool():
    """Seven clips; trimmed lengths 1599, 1600, 1601, 48000, 1600 (all zero), 3000, 800."""
    lengths = [4000, 4000, 4000, 60000, 4000, 5000, 4000]
    bounds = [(512, 2111), (1024, 2624), (0, 1601), (2048, 50048), (0, 1600), (1000, 4000), (0, 800)]
    peak = [0.5, 0.5, 0.5, 0.5, 0.0, 0.5, 0.5]
    return mixing.ClipPool.planned(lengths, bounds, peak)


def test_planned_pool_numbers():
    pool = _pool()
    assert len(pool) == 7 and pool.total == 85000
    assert pool.trimmed_lengths.tolist() == [1599, 1600, 1601, 48000, 1600, 3000, 800]
    assert pool.trimmed_length(3) == 48000
    assert pool.trimmed_starts.tolist() == [512, 4000 + 1024, 8000, 12000 + 2048, 72000, 76000 + 1000, 81000]


def test_plan_triplets_drops_exactly_the_too_short_ones():
    pool = _pool()
    #            clean 1599     interferer 800   reference length is free   exactly L       all-zero clean   all-zero interferer
    triplets = [(0, 3, 1), (1, 3, 6), (1, 6, 2), (2, 0, 3), (3, 3, 1), (5, 5, 5), (4, 3, 1), (1, 3, 4)]
    kept, dropped = mixing.plan_triplets(pool, triplets, L)
    assert kept == [(1, 6, 2), (2, 0, 3), (3, 3, 1), (5, 5, 5)] and dropped == 4
    assert mixing.keep_mask(pool, triplets, L) == [False, False, True, True, True, True, False, False]
    # a reference clip without an embedding drops its triplets too (the [0] items of the reference's collate)
    emb_ok = [True] * 7
    emb_ok[6] = False
    kept, dropped = mixing.plan_triplets(pool, triplets, L, emb_ok=emb_ok)
    assert kept == [(2, 0, 3), (3, 3, 1), (5, 5, 5)] and dropped == 5
    assert mixing.plan_triplets(pool, triplets, 1601)[0] == [(2, 0, 3), (5, 5, 5)]
    assert mixing.plan_triplets(pool, [], L) == ([], 0)


def _batches(pool, triplets, crop, seed=0, rank=0, world=1, b=2):
    acfg = {"sample_rate": 16000, "hop_length": 160, "n_fft": 1200}
    shard = EpochShard(len(triplets), b, rank, world, seed=3)
    return mixing.MixtureBatches(pool, triplets, torch.zeros(len(pool), 4), acfg, L / 16000, shard, crop=crop, seed=seed)


def test_crop_offsets_head_and_random():
    pool = _pool()
    triplets = [(1, 0, 2), (2, 0, 3), (3, 0, 1), (5, 0, 3), (3, 0, 5), (2, 0, 1)]          # room 0, 1, 1400 and 46400
    mb = _batches(pool, triplets, "head")
    assert mb.L == L and mb.room.tolist() == [[0, 1], [1, 46400], [46400, 0], [1400, 46400], [46400, 1400], [1, 0]]
    order = list(mb.shard.epoch(0))
    pos, at, emb_row = mb.plan(order, 0)
    assert pos.tolist() == [p for b in order for p in b] and emb_row.tolist() == [0] * 6
    assert torch.equal(at.t(), mb.start[pos])                                              # crop="head": offsets are zero
    starts = pool.trimmed_starts
    assert at[0].tolist() == [int(starts[triplets[p][0]]) for p in pos.tolist()]
    # random: inside the trimmed clip for room 0 (length L), 1 (L + 1) and much more; every value of a small range is drawn
    mr = _batches(pool, triplets, "random", seed=5)
    seen = set()
    for e in range(40):
        pos, at, _ = mr.plan(list(mr.shard.epoch(e)), e)
        off = at.t() - mr.start[pos]
        assert (off >= 0).all() and (off <= mr.room[pos]).all()
        seen.update(off[mr.room[pos] == 1].tolist())
    assert seen == {0, 1}
    room = torch.tensor([0, 1, 46400] * 2000)
    off = mixing.crop_offsets(room, "random", torch.Generator().manual_seed(1))
    assert (off >= 0).all() and (off <= room).all() and int(off[2::3].max()) > 46000 and int(off[2::3].min()) < 400
    assert mixing.crop_offsets(room, "head").abs().sum() == 0
    with pytest.raises(ValueError):
        mixing.crop_offsets(torch.tensor([-1]), "random")
    with pytest.raises(ValueError):
        mixing.crop_offsets(room, "tail")


def test_random_crops_repeat_for_equal_seed_epoch_rank_and_differ_otherwise():
    pool = _pool()
    triplets = [(3, 0, 5), (5, 0, 3), (3, 0, 3), (5, 0, 5)] * 4

    def plan(seed, epoch, rank, world=2):
        mb = _batches(pool, triplets, "random", seed=seed, rank=rank, world=world)
        return mb.plan(list(mb.shard.epoch(epoch)), epoch)

    a, b = plan(7, 2, 1), plan(7, 2, 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(plan(7, 3, 1)[1] - _at0(pool, triplets, plan(7, 3, 1)[0]), a[1] - _at0(pool, triplets, a[0]))    # epoch
    assert not torch.equal(plan(7, 2, 0)[1] - _at0(pool, triplets, plan(7, 2, 0)[0]), a[1] - _at0(pool, triplets, a[0]))    # rank
    assert not torch.equal(plan(8, 2, 1)[1], a[1])                                                                          # seed
    assert len({mixing.crop_seed(s, e, r) for s in range(3) for e in range(50) for r in range(8)}) == 1200


def _at0(pool, triplets, pos):
    """the head-crop start indices of the same positions: what is left after subtracting them is the crop offset"""
    s = pool.trimmed_starts
    return torch.tensor([[int(s[triplets[p][0]]) for p in pos.tolist()], [int(s[triplets[p][2]]) for p in pos.tolist()]])


def test_mixture_batches_refuses_what_the_planner_would_have_dropped():
    pool = _pool()
    with pytest.raises(ValueError, match="plan_triplets"):
        _batches(pool, [(0, 3, 1), (1, 3, 2)], "head")
    with pytest.raises(ValueError, match="triplets"):
        acfg = {"sample_rate": 16000, "hop_length": 160, "n_fft": 1200}
        mixing.MixtureBatches(pool, [(1, 3, 2)], torch.zeros(7, 4), acfg, 0.1, EpochShard(5, 1), crop="head")
    with pytest.raises(ValueError, match="hop_length"):
        acfg = {"sample_rate": 16000, "hop_length": 160, "n_fft": 1200}
        mixing.MixtureBatches(pool, [(3, 3, 3)], torch.zeros(7, 4), acfg, 1601 / 16000, EpochShard(1, 1), crop="head")
    mb = _batches(pool, [(1, 3, 2), (2, 3, 1)], "head")
    with pytest.raises(Exception, match="no audio"):
        next(mb.epoch(0))


def test_csv_path_rules_and_missing_files(tmp_path):
    root = tmp_path / "corpus"
    names = ["19-198-0001", "19-198-0002", "26-495-0003", "26-496-0004"]
    for n in names[:3]:                                      # the fourth file does not exist
        s = n.split("-")
        (root / s[0] / s[1]).mkdir(parents=True, exist_ok=True)
        (root / s[0] / s[1] / (n + "-norm.wav")).write_bytes(b"")
        (root / (n + ".wav")).write_bytes(b"")
    rows = [(0, 1, 2), (1, 0, 3), (2, 2, 0), (3, 1, 0), (1, 2, 0)]
    libri = tmp_path / "libri.csv"
    libri.write_text("clean_utterance,embedding_utterance,interference_utterance\n" +
                     "".join(",".join(names[k] for k in r) + "\n" for r in rows))
    paths, triplets, numbers, skipped = mixing.read_triplet_csv(str(libri), str(root), librispeech=True)
    assert paths == [os.path.join(str(root), n.split("-")[0], n.split("-")[1], n + "-norm.wav") for n in names[:3]]
    assert triplets == [(0, 1, 2), (2, 2, 0), (1, 2, 0)] and numbers == [0, 2, 4] and skipped == 2
    plain = tmp_path / "plain.csv"
    plain.write_text("clean_utterance,embedding_utterance,interference_utterance\n" +
                     "".join(",".join(names[k] + ".wav" for k in r) + "\n" for r in rows))
    paths, triplets, numbers, skipped = mixing.read_triplet_csv(str(plain), str(root))
    assert paths == [os.path.join(str(root), n + ".wav") for n in names[:3]]
    assert triplets == [(0, 1, 2), (2, 2, 0), (1, 2, 0)] and numbers == [0, 2, 4] and skipped == 2
    bad = tmp_path / "bad.csv"
    bad.write_text("a,b,c\nx,y\n")
    with pytest.raises(ValueError, match="fields"):
        mixing.read_triplet_csv(str(bad), str(root))


def test_output_file_names():
    f = mixing.DEFAULT_FORMAT
    assert mixing.output_name("out", f["mixed_wav"], 0) == os.path.join("out", "000000-mixed.wav")
    assert mixing.output_name("out", f["target_wav"], 12) == os.path.join("out", "000012-target.wav")
    assert mixing.output_name("out", f["emb_wav"], 123456) == os.path.join("out", "123456-emb.wav")
    assert [os.path.basename(mixing.output_name("o", f[k], 7)) for k in ("mixed", "target", "emb")] == \
        ["000007-mixed.pt", "000007-target.pt", "000007-emb.pt"]
    assert mixing.samples_for({"sample_rate": 16000}, 3) == 48000 and mixing.samples_for({"sample_rate": 16000}, 0.01) == 160


def test_lib_signatures_and_refusals_without_a_device():
    import ctypes
    from voicesplit_amd import _lib
    for name, nargs in (("vs_trim_workspace_bytes", 2), ("vs_trim_bounds", 10), ("vs_mix_clips", 12)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    lib = _lib.load()
    assert lib.vs_trim_workspace_bytes(10 ** 6, 10) == ((10 ** 6 // 512 + 44) * 8 + 255) // 256 * 256
    assert lib.vs_trim_workspace_bytes(0, 10) == 0 and lib.vs_trim_workspace_bytes(100, 0) == 0
    one = ctypes.c_void_p(256)
    offs = (ctypes.c_longlong * 3)(0, 2000, 3024)                       # the second clip has 1024 samples: refused before any launch
    p_offs = ctypes.cast(offs, ctypes.c_void_p)
    assert lib.vs_trim_bounds(one, 4000, p_offs, one, 2, one, None, one, 1 << 20, None) == -1
    msg = lib.vs_last_error()
    assert b"clip 1" in msg and b"1024 samples" in msg and b"1025" in msg
    offs = (ctypes.c_longlong * 2)(0, 5000)
    assert lib.vs_trim_bounds(one, 4000, ctypes.cast(offs, ctypes.c_void_p), one, 1, one, None, one, 1 << 20, None) == -1
    assert b"leave the buffer" in lib.vs_last_error()
    assert lib.vs_mix_clips(None, 4000, one, one, 2, 1600, one, one, one, one, None, None) == -1 and b"NULL" in lib.vs_last_error()
    assert lib.vs_mix_clips(one, 1000, one, one, 2, 1600, one, one, one, one, None, None) == -1 and b"1600 samples" in lib.vs_last_error()
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        mixing.ClipPool([torch.zeros(2000)], "cpu")
    with pytest.raises(ValueError, match="fewer than 1025"):
        mixing.ClipPool([torch.zeros(1024)], "cuda:0")


def test_restatement_on_hand_made_clips():
    """tests/mixing_ref.py against cases whose answer is known without it."""
    n = 6000
    assert MR.trim_bounds(np.zeros(n)) == (0, n)                       # every frame at the clamp: ratio 1
    y = np.zeros(n)
    y[3000:3100] = 0.5                                                 # frame 4 = y[1024:3072) holds 72 of them, 5..7 all, 8 = y[3072:5120) 28
    assert MR.frame_mse(y).shape == (n // 512 + 1,)
    assert MR.trim_bounds(y) == (512 * 4, 512 * 9) and MR.margin(y) > 0.9
    y = np.zeros(n)
    y[:100] = 0.5                                                      # reflected: frames 0 and 1 hold y[1..99] twice and y[0] once
    mse = MR.frame_mse(y)
    assert np.allclose(mse[:3] * 2048, [0.25 * 199, 0.25 * 199, 0.25 * 100]) and mse[3] == 0
    assert MR.trim_bounds(y) == (0, 1536)
    y = np.zeros(n)
    y[-100:] = 0.5
    assert MR.trim_bounds(y) == (512 * 10, n)                          # frame 9 = y[3584:5632) ends in front of them
    c = np.array([0.5, -0.25, 0.125], dtype=np.float32)
    mixed, target, norm, valid = MR.mix(c, -c)
    assert valid == 0 and not mixed.any() and not target.any()
    mixed, target, norm, valid = MR.mix(c, c)
    assert valid == 1 and norm == np.float32(1.1) and np.allclose(mixed, c * 2 / np.float64(np.float32(1.1)))
