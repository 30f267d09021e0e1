"""GPU: training mixtures from a resident pool of clean utterances (voicesplit_amd/mixing.py, csrc/mix.hip) through the C ABI.

vs_trim_bounds against the fp64 restatement of tests/mixing_ref.py: EXACT bounds for every clip whose closest frame is at least
1e-3 (relative) away from the silence threshold -- asserted on the inputs -- since the kernel's fp64 sums differ from numpy's by
1e-15 at most.  vs_mix_clips against fp64: ``norm`` exactly, every sample within 2^-22 relative (four fp32 roundings at most: the
sum, the norm and a division done as reciprocal and multiply; the kernel divides, which is one).  Then the batch contract of
``MixtureBatches`` against ``BatchFeeder``'s, the embeddings, and the writer's files read back by ``SpecWavDataset``."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mixing_ref as MR
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MARGIN = 1e-3


def demo_clips():
    z = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    return [z[k][i].astype(np.float32) / 32768.0 for k in ("target", "mixed") for i in range(4)]


def _noise(rng, n):
    return (rng.uniform(-1.0, 1.0, n) * 1e-3).astype(np.float32)


def _burst(rng, n, lo, hi, amp=0.3):
    """quiet noise with a loud stretch [lo, hi)"""
    y = _noise(rng, n)
    y[lo:hi] += (amp * np.sin(np.arange(hi - lo) * 0.21) * rng.uniform(0.5, 1.0, hi - lo)).astype(np.float32)
    return y


@pytest.fixture(scope="module")
def trim_case():
    """(clips, pool, reference bounds): the clips in pool order.  A spacer cannot be a clip of its own (a clip below 1025 samples is
    refused), so the clips of odd length -- 1025, 2047, 2049, 5119, 5121 and the demo clips with 700 + 1 samples around them -- are
    spread between the others: the clip offsets take every residue mod 4 (asserted)."""
    from voicesplit_amd.mixing import ClipPool
    rng = np.random.default_rng(20)
    demo = demo_clips()
    plain = list(demo)
    wide = [np.concatenate([_noise(rng, 3000), y, _noise(rng, 5000)]) for y in demo]
    odd = [np.concatenate([_noise(rng, 700), y, _noise(rng, 1)]) for y in demo]
    synth = [_burst(rng, n, n // 3, n // 3 + 300) for n in (1025, 2047, 2048, 2049, 5119, 5120, 5121)]
    zero = np.zeros(6000, dtype=np.float32)
    first = np.zeros(6000, dtype=np.float32)
    first[:100] = 0.5
    last = np.zeros(6001, dtype=np.float32)
    last[-100:] = -0.5
    loud = (rng.uniform(-1.0, 1.0, 4099) * 0.9).astype(np.float32)
    silent = np.zeros(4099, dtype=np.float32)
    probe = _burst(rng, 7003, 2500, 4200, amp=0.05)
    clips = []
    for k in range(8):
        clips += [plain[k], synth[k % 7], odd[k], wide[k]]
    clips += [synth[6 - k] for k in range(7)]
    clips += [zero, synth[0], first, synth[1], last, synth[3]]
    leak_at = (len(clips) + 1, len(clips) + 4)
    clips += [loud, probe, loud.copy(), silent, probe.copy(), silent.copy()]
    pool = ClipPool([torch.from_numpy(c) for c in clips], DEV)
    torch.cuda.synchronize()
    ref = [MR.trim_bounds(c) for c in clips]
    return clips, pool, ref, leak_at


def test_trim_inputs_are_off_the_threshold_and_cover_the_cases(trim_case):
    clips, pool, ref, _ = trim_case
    margins = [MR.margin(c) for c in clips]
    print("margins: min %.3e max %.3e" % (min(margins), max(margins)))
    assert min(margins) >= MARGIN, [(k, m) for k, m in enumerate(margins) if m < MARGIN]
    assert set((pool.offsets[:-1] % 4).tolist()) == {0, 1, 2, 3}
    assert {len(c) % 512 for c in clips} >= {0, 1, 511} and min(len(c) for c in clips) == 1025
    nontrivial = [(s, e) for (s, e), c in zip(ref, clips) if s > 0 and e < len(c)]
    assert len(nontrivial) >= 16, ref
    assert pool.total == sum(len(c) for c in clips) and torch.equal(pool.flat.cpu(), torch.from_numpy(np.concatenate(clips)))


def test_trim_bounds_equal_the_restatement_exactly(trim_case):
    clips, pool, ref, _ = trim_case
    got = [tuple(b) for b in pool.bounds.tolist()]
    print("bounds:", got)
    assert got == [tuple(r) for r in ref]
    # the peaks of the trimmed regions, and the views
    for k, (c, (s, e)) in enumerate(zip(clips, ref)):
        assert float(pool.peak[k]) == (float(np.abs(c[s:e]).max()) if e > s else 0.0), k
        assert pool.trimmed_length(k) == e - s
    k = 3
    assert torch.equal(pool.trimmed(k).cpu(), torch.from_numpy(clips[k][ref[k][0]:ref[k][1]]))


def test_trim_special_clips(trim_case):
    clips, pool, ref, leak_at = trim_case
    got = [tuple(b) for b in pool.bounds.tolist()]
    by_len = {len(c): k for k, c in enumerate(clips)}
    assert got[by_len[6000] - 2] == (0, 6000) and not clips[by_len[6000] - 2].any()          # the all-zero clip: (0, n)
    assert got[by_len[6000]] == (0, 1536)                                                    # loud only in its first 100 samples
    assert got[by_len[6001]] == (512 * 10, 6001)                                             # loud only in its last 100 samples
    # the same clip between two very loud neighbours and between two silent ones
    a, b = leak_at
    assert np.array_equal(clips[a], clips[b]) and got[a] == got[b] == tuple(ref[a]) and 0 < got[a][0] < got[a][1] < len(clips[a])


def test_trim_refuses_a_clip_of_1024_samples():
    from voicesplit_amd import _lib
    lib = _lib.load()
    flat = torch.zeros(5000, device=DEV)
    offs = torch.tensor([0, 3000, 4024], dtype=torch.int64)
    offs_dev = offs.to(DEV)
    bounds = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.vs_trim_workspace_bytes(5000, 2), dtype=torch.uint8, device=DEV)
    rc = lib.vs_trim_bounds(flat.data_ptr(), 5000, offs.data_ptr(), offs_dev.data_ptr(), 2, bounds.data_ptr(), None, ws.data_ptr(),
                            ws.numel(), None)
    assert rc == -1 and b"clip 1 has 1024 samples" in lib.vs_last_error()
    torch.cuda.synchronize()
    assert (bounds == -7).all()                                            # nothing was launched


# ---- vs_mix_clips -----------------------------------------------------------------------------------------------------------------
def _check_mix(flat_np, clean_at, interf_at, L, expect_valid):
    from voicesplit_amd.mixing import mix_clips
    flat = torch.from_numpy(flat_np).to(DEV)
    ca, ia = torch.tensor(clean_at, dtype=torch.int64, device=DEV), torch.tensor(interf_at, dtype=torch.int64, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    runs = [mix_clips(flat, ca, ia, L, count) for _ in range(2)]
    torch.cuda.synchronize()
    for x, y in zip(*runs):
        assert torch.equal(x, y)                                           # bit-identical reruns
    mixed, target, norm, valid = (t.cpu().numpy() for t in runs[0])
    assert valid.tolist() == expect_valid and int(count) == 2 * expect_valid.count(0)
    worst = 0.0
    for b in range(len(clean_at)):
        c, i = flat_np[clean_at[b]:clean_at[b] + L], flat_np[interf_at[b]:interf_at[b] + L]
        rm, rt, rnorm, rvalid = MR.mix(c, i)
        assert rvalid == expect_valid[b]
        assert norm[b] == rnorm and norm[b].dtype == np.float32, (b, norm[b], rnorm)
        if not rvalid:
            assert not mixed[b].any() and not target[b].any()
            continue
        for got, want in ((mixed[b], rm), (target[b], rt)):
            err = np.abs(got.astype(np.float64) - want)
            nz = want != 0
            assert (got[~nz] == 0).all()
            worst = max(worst, float((err[nz] / np.abs(want[nz])).max()))
    print("mix: worst relative error %.3e (bound 2^-22 = %.3e)" % (worst, 2.0 ** -22))
    assert worst <= 2.0 ** -22
    return mixed, target


def test_mix_small_every_alignment_edges_and_a_silent_sum():
    L, B = 1600, 5
    rng = np.random.default_rng(5)
    flat = (rng.standard_normal(2 * B * (L + 8)) * 0.1).astype(np.float32)
    clean_at = [b * (L + 8) + r for b, r in enumerate((0, 1, 2, 3, 1))]                     # residues mod 4: 0 1 2 3 1
    interf_at = [(B + b) * (L + 8) + r for b, r in enumerate((3, 0, 1, 2, 2))]              #                 3 0 1 2 2
    assert {a % 4 for a in clean_at} == {0, 1, 2, 3} and {a % 4 for a in interf_at} == {0, 1, 2, 3}
    flat[clean_at[1]] = 3.0                                                # the maximum at sample 0 ...
    flat[interf_at[1]] = 0.5
    flat[clean_at[2] + L - 1] = -2.5                                       # ... and at sample L - 1
    flat[interf_at[2] + L - 1] = -0.25
    flat[interf_at[4]:interf_at[4] + L] = -flat[clean_at[4]:clean_at[4] + L]          # c = -i: every sum is zero
    mixed, _ = _check_mix(flat, clean_at, interf_at, L, [1, 1, 1, 1, 0])
    assert np.abs(mixed[1]).argmax() == 0 and np.abs(mixed[2]).argmax() == L - 1
    assert np.isclose(np.abs(mixed[:4]).max(axis=1), 1 / 1.1, rtol=1e-6).all()
    # lengths that are no multiple of four (unaligned output rows) and of the 2048-sample chunk
    _check_mix(flat, [a + 1 for a in clean_at[:3]], interf_at[:3], 1597, [1, 1, 1])
    _check_mix(flat, [5, 2], [9001, 6003], 4099, [1, 1])


def test_mix_refuses_an_index_outside_the_buffer_without_reading_it():
    from voicesplit_amd.mixing import mix_clips
    flat = torch.ones(4000, device=DEV)
    ca = torch.tensor([0, 2401, -1], dtype=torch.int64, device=DEV)
    ia = torch.tensor([100, 100, 100], dtype=torch.int64, device=DEV)
    mixed, target, norm, valid = mix_clips(flat, ca, ia, 1600)
    assert valid.tolist() == [1, -1, -1] and not mixed[1:].any() and not target[1:].any()
    assert torch.equal(mixed[0], torch.full((1600,), 2.0 / float(np.float32(2.2)), device=DEV))


def test_mix_three_seconds_from_the_demo_clips(trim_case):
    clips, pool, _, _ = trim_case
    offs = pool.offsets.tolist()
    flat = np.concatenate(clips)
    # target 0 + mixed 1 and target 2 + mixed 3: the plain demo clips sit at pool ids 0, 4, 8, ... (target) and 16, 20, ... (mixed)
    clean_at, interf_at = [offs[0], offs[8]], [offs[20], offs[28]]
    assert all(len(clips[k]) == 48000 for k in (0, 8, 20, 28))
    _check_mix(flat, clean_at, interf_at, 48000, [1, 1])


# ---- MixtureBatches ---------------------------------------------------------------------------------------------------------------
def _small_cfg():
    """the small configuration of tests/test_gpu_trainer.py"""
    import voicesplit_amd as V
    dims = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
    c = V.default_config(**dims)
    c.audio["voicefilter"].update({"hop_length": 16, "win_length": 40})
    c.train_config["learning_rate"] = 1e-3
    return c, dims


def _small_pool(seed=3, n=7):
    from voicesplit_amd.mixing import ClipPool
    rng = np.random.default_rng(seed)
    clips = []
    for k in range(n):
        m = 1500 + 211 * k
        clips.append(_burst(rng, m, 200 + 37 * k, m - 150, amp=0.2))
    return ClipPool([torch.from_numpy(c) for c in clips], DEV)


def test_mixture_batches_yield_the_feeders_tuples_and_train():
    import voicesplit_amd as V
    from voicesplit_amd import audio, mixing
    from voicesplit_amd.trainer import EpochShard, Trainer
    c, dims = _small_cfg()
    acfg = c.audio["voicefilter"]
    T, B = 11, 3
    L = acfg["hop_length"] * (T - 1)
    audio_len = L / acfg["sample_rate"]
    pool = _small_pool()
    triplets = [(a, (a + 1) % 7, (a + 3) % 7) for a in range(7)] + [(a, a, (a + 2) % 7) for a in range(7)]
    kept, dropped = mixing.plan_triplets(pool, triplets, L)
    assert dropped == 0 and int(pool.trimmed_lengths.min()) > L
    table = torch.randn(len(pool), dims["emb_dim"], generator=torch.Generator().manual_seed(2)).to(DEV)
    shard = EpochShard(len(kept), B, seed=4)
    mb = mixing.MixtureBatches(pool, kept, table, acfg, audio_len, shard, crop="head")
    order = list(shard.epoch(0))
    items = list(mb.items(order, 0))
    batches = list(mb.epoch(0))
    assert len(batches) == len(items) == len(kept) // B == 4
    F = dims["num_freq"]
    for idx, it, (emb, target, mixed, seq_len, target_wav, phase) in zip(order, items, batches):
        assert emb.shape == (B, dims["emb_dim"]) and target.shape == mixed.shape == phase.shape == (B, T, F)
        assert target_wav.shape == (B, L) and seq_len.tolist() == [L] * B and seq_len.dtype == torch.int64
        assert all(t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() for t in (emb, target, mixed, target_wav, phase))
        assert it["valid"].tolist() == [1] * B and it["positions"].tolist() == idx
        assert torch.equal(emb, table[[kept[p][1] for p in idx]])
        spec, ph = audio.wav_to_spec(it["mixed_wav"], acfg, want_phase=True)
        assert torch.equal(mixed, spec) and torch.equal(phase, ph) and torch.equal(it["mixed"], mixed)
        assert torch.equal(target, audio.wav_to_spec(target_wav, acfg, want_phase=False)[0]) and torch.equal(it["target_wav"], target_wav)
        # crop="head": the item is the head of its two trimmed clips
        for row, p in enumerate(idx):
            cl, _, itf = kept[p]
            rm, rt, rnorm, _ = MR.mix(pool.trimmed(cl)[:L].cpu().numpy(), pool.trimmed(itf)[:L].cpu().numpy())
            assert float(it["norm"][row]) == float(rnorm)
            assert np.allclose(it["mixed_wav"][row].cpu().numpy(), rm, rtol=2.0 ** -22, atol=0)
    assert mb.invalid_items == 0
    # random crops: the same (seed, epoch, rank) gives the same bits, another epoch other crops
    r1 = mixing.MixtureBatches(pool, kept, table, acfg, audio_len, shard, crop="random", seed=9)
    r2 = mixing.MixtureBatches(pool, kept, table, acfg, audio_len, shard, crop="random", seed=9)
    e1, e2, e1b = list(r1.epoch(1)), list(r2.epoch(1)), list(r1.epoch(2))
    assert all(torch.equal(x, y) for a, b in zip(e1, e2) for x, y in zip(a, b))
    assert not all(torch.equal(a[4], b[4]) for a, b in zip(e1, list(mb.epoch(1))))          # not the head crops
    assert len(e1b) == 4
    # one training step on a yielded batch
    torch.manual_seed(0)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    loss = tr.train_step(e1[0])
    assert np.isfinite(loss), loss


def test_pool_embed_equals_one_clip_at_a_time(trim_case):
    from voicesplit_amd import SpeakerEncoder, logmel
    clips, pool, _, _ = trim_case
    z = np.load(os.path.join(GOLDEN_DIR, "speaker_small.npz"))
    m, l, h, e, w, s = (int(v) for v in z["dims"])
    enc = SpeakerEncoder(m, l, h, e, w, s).eval()
    enc.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    enc = enc.to(DEV)
    acfg = {"n_fft": 1200, "num_freq": 601, "sample_rate": 16000, "hop_length": 160, "win_length": 400,
            "min_level_db": -100.0, "ref_level_db": 20.0}
    short = min(range(len(pool)), key=pool.trimmed_length)                                  # too short for one window: a zero row
    assert 1 + pool.trimmed_length(short) // 160 < w
    ids = [0, 2, short, 3, 17, 6]
    got = pool.embed(enc, acfg, ids, batch=4)
    assert got.shape == (len(ids), e)
    for row, i in enumerate(ids):
        if i == short:
            assert not got[row].any()
            continue
        # as tests/test_gpu_speaker.py holds the batched call to the single one: the same bits
        assert torch.equal(got[row], enc(logmel(pool.trimmed(i), acfg, m))), i


def test_writer_round_trip_through_the_dataset(tmp_path):
    from scipy.io import wavfile
    import voicesplit_amd as V
    from voicesplit_amd import mixing
    from voicesplit_amd.trainer import EpochShard, SpecWavDataset
    z = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    root = tmp_path / "corpus"
    root.mkdir()
    names = []
    for k in ("target", "mixed"):
        for i in range(3):
            names.append(f"{k}{i}.wav")
            wavfile.write(str(root / names[-1]), 16000, z[k][i])           # int16 files
    rows = [(0, 3, 1), (1, 4, "missing.wav"), (2, 5, 3), (4, 0, 5)]
    csv_path = tmp_path / "train.csv"
    csv_path.write_text("clean_utterance,embedding_utterance,interference_utterance\n" +
                        "".join(",".join(names[k] if isinstance(k, int) else k for k in r) + "\n" for r in rows))
    c = V.default_config()
    c.audio["audio_len"] = 1
    out = tmp_path / "out"
    c.dataset = {"train_dir": str(out / "train"), "test_dir": str(out / "train"),
                 "format": {"emb": "*-emb.pt", "mixed": "*-mixed.pt", "target": "*-target.pt", "target_wav": "*-target.wav",
                            "mixed_wav": "*-mixed.wav", "emb_wav": "*-emb.wav"}}
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps({k: (dict(v) if isinstance(v, dict) else v) for k, v in c.items()}, indent=1))
    mixing.main(["-c", str(cfg_path), "-r", str(root), "-d", str(csv_path), "-o", str(out)])
    want_files = sorted(f"{n:06d}-{s}" for n in (0, 2, 3) for s in ("mixed.wav", "target.wav", "emb.wav", "mixed.pt", "target.pt"))
    assert sorted(os.listdir(out / "train")) == want_files
    sr, w = wavfile.read(str(out / "train" / "000002-mixed.wav"))
    assert sr == 16000 and w.dtype == np.float32 and w.shape == (16000,)
    g = torch.Generator().manual_seed(1)
    embs = [torch.randn(256, generator=g) for _ in range(3)]
    for n, e in zip((0, 2, 3), embs):                                      # the speaker-encoder step of the reference's pipeline
        torch.save(e, str(out / "train" / f"{n:06d}-emb.pt"))
    ds = SpecWavDataset(c)
    assert len(ds) == 3
    read = ds.collate([ds[i] for i in range(3)], DEV)
    # the same triplets straight from the pool
    acfg = c.audio["voicefilter"]
    paths, triplets, numbers, skipped = mixing.read_triplet_csv(str(csv_path), str(root))
    assert numbers == [0, 2, 3] and skipped == 1
    pool = mixing.ClipPool.from_files(paths, 16000, DEV)
    kept, dropped = mixing.plan_triplets(pool, triplets, 16000)
    assert dropped == 0
    mb = mixing.MixtureBatches(pool, kept, torch.stack(embs).to(DEV), acfg, 1, EpochShard(3, 3, shuffle=False), crop="head",
                               emb_rows="triplet")
    (made,) = list(mb.epoch(0))
    for name, a, b in zip(("emb", "target", "mixed", "seq_len", "target_wav", "phase"), read, made):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.equal(a.cpu(), b.cpu()), name                         # float32 wavs are lossless: the same bits
    emb_wav = wavfile.read(str(out / "train" / "000003-emb.wav"))[1]
    assert np.array_equal(emb_wav, pool.trimmed(kept[2][1]).cpu().numpy())
