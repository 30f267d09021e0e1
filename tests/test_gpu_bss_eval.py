"""GPU: metrics.bss_eval (vs_bss_eval: fp64 correlations between all pairs, the block Levinson solve of the K-source Gram
matrix, the single-source solves, fp64 projections, the permutation search) against the fp64 restatement of mir_eval's
bss_eval_sources (tests/bss_eval_multi_ref.py); compute_permutation=False, K = 1 against metrics.bss_sdr, silent and
degenerate items, exact reconstruction, bitwise repeatability; Trainer.evaluate_speakers and the --speakers-csv CLI mode."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import bss_eval_multi_ref as M
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

TOL_DB = 1e-6                                     # test_gpu_sdr.py's tolerance against its restatement


def _gpu(ref, est, **kw):
    from voicesplit_amd import metrics
    out = metrics.bss_eval(torch.from_numpy(np.array(ref, np.float32)).cuda(),            # a copy: the shared cases are read-only
                           torch.from_numpy(np.array(est, np.float32)).cuda(), **kw)
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _case(K, N):
    """(ref, est, the restatement's results) of the B = 3 batch for (K, N): computed once, never written to."""
    ref, est = M.make_batch(K, N)
    want = M.bss_eval_batch(ref, est)
    for a in (ref, est) + want:
        a.setflags(write=False)
    return ref, est, want


@pytest.mark.parametrize("K,N", [(2, 16000), (3, 16000), (4, 16000), (6, 16000), (2, 6001), (3, 6001), (5, 6001)])
def test_all_pairs_and_the_permutation_match_the_restatement(K, N):
    ref, est, want = _case(K, N)
    M.guards(*want)                               # status 0, every criterion <= 40 dB, the best permutation >= 1 dB ahead
    assert want[3][0].tolist() == [(j + 1) % K for j in range(K)]
    sdr, sir, sar, perm, status, pairs = _gpu(ref, est, return_pairs=True)
    assert status.tolist() == [0, 0, 0]
    diff = np.abs(pairs - want[5]).max(axis=(0, 2, 3))
    print(f"K = {K}, N = {N}: max |GPU - restatement| (dB) sdr {diff[0]:.3e} sir {diff[1]:.3e} sar {diff[2]:.3e}")
    assert np.array_equal(perm, want[3]), (perm, want[3])
    assert (np.abs(pairs - want[5]) <= TOL_DB).all(), diff
    for got, w in zip((sdr, sir, sar), want[:3]):
        assert (np.abs(got - w) <= TOL_DB).all(), (got, w)
    idx = np.arange(K)
    for b in range(3):                            # the returned values are the pairs the permutation picks
        for c, got in enumerate((sdr, sir, sar)):
            assert np.array_equal(got[b], pairs[b, c][perm[b], idx])


def test_without_permutation_is_the_diagonal_of_the_pairs_bitwise():
    ref, est, _ = _case(3, 6001)
    full = _gpu(ref, est, return_pairs=True)
    sdr, sir, sar, perm, status, pairs = _gpu(ref, est, compute_permutation=False, return_pairs=True)
    assert status.tolist() == [0, 0, 0] and (perm == np.arange(3)).all()
    for c, got in enumerate((sdr, sir, sar)):
        assert np.array_equal(got, np.diagonal(full[5][:, c], axis1=1, axis2=2))
        assert np.array_equal(np.diagonal(pairs[:, c], axis1=1, axis2=2), got)
    off = ~np.eye(3, dtype=bool)
    assert np.isnan(pairs[:, :, off]).all()
    assert len(_gpu(ref, est, compute_permutation=False)) == 5


def test_one_source_is_bss_sdr_bit_for_bit():
    from voicesplit_amd import metrics
    for N in (16000, 6001):
        ref, est = M.make_batch(1, N)
        sdr, sir, sar, perm, status = _gpu(ref, est)
        one, st1 = metrics.bss_sdr(torch.from_numpy(ref[:, 0].copy()).cuda(), torch.from_numpy(est[:, 0].copy()).cuda())
        assert status.tolist() == [0, 0, 0] and st1.tolist() == [0, 0, 0]
        assert np.array_equal(sdr[:, 0], one.cpu().numpy())
        assert np.array_equal(sar, sdr) and (sir == np.inf).all() and (perm == 0).all()
    # [K, N] input is one item
    out = _gpu(ref[0], est[0], return_pairs=True)
    assert out[0].shape == (1, 1) and out[5].shape == (1, 3, 1, 1) and out[0][0, 0] == sdr[0, 0]


def test_silent_rows_get_status_1_and_leave_the_other_items_alone():
    ref, est, _ = _case(3, 6001)
    base = _gpu(ref, est, return_pairs=True)
    ref2, est2 = ref.copy(), est.copy()
    ref2[1, 2] = 0.0
    est2[2, 0] = 0.0
    for cp in (True, False):
        got = _gpu(ref2, est2, compute_permutation=cp, return_pairs=True)
        assert got[4].tolist() == [0, 1, 1]
        for a in got[:3] + (got[5],):
            assert np.isnan(a[1:]).all()
        assert (got[3][1:] == -1).all()
    got = _gpu(ref2, est2, return_pairs=True)
    for a, b in zip(got, base):
        assert np.array_equal(a[0], b[0])                                  # bitwise


def test_identical_references_get_status_2():
    ref, est, _ = _case(3, 6001)
    base = _gpu(ref, est, return_pairs=True)
    ref2 = ref.copy()
    ref2[1, 2] = ref2[1, 0]                                               # R[0] of item 1 is exactly singular
    got = _gpu(ref2, est, return_pairs=True)
    assert got[4].tolist() == [0, 2, 0]
    for a in got[:3] + (got[5],):
        assert np.isnan(a[1]).all()
    assert (got[3][1] == -1).all()
    for a, b in zip(got, base):
        assert np.array_equal(a[[0, 2]], b[[0, 2]])                        # bitwise


@pytest.mark.parametrize("K", [2, 3, 4])
def test_identical_references_are_always_caught(K):
    """16 items whose first and last reference rows are the same bits, at 16 different levels and lengths of signal: the
    detection must not depend on how the pivot of R[0] happens to round (1 / p times p is not 1 for about one p in eight)."""
    rng = np.random.default_rng(40 + K)
    N = 3000
    refs, ests = [], []
    for b in range(16):
        r, e = M.make_item(K, N + 64 * b, seed=500 + b)
        r = (r[:, 32 * b:32 * b + N] * rng.uniform(0.3, 3.0, (K, 1))).astype(np.float32)
        r[K - 1] = r[0]
        refs.append(r)
        ests.append(e[:, 32 * b:32 * b + N])
    for cp in (True, False):
        got = _gpu(np.stack(refs), np.stack(ests), compute_permutation=cp, return_pairs=True)
        assert got[4].tolist() == [2] * 16, got[4]
        assert all(np.isnan(a).all() for a in got[:3] + (got[5],)) and (got[3] == -1).all()


def test_exact_reconstruction():
    ref, _, _ = _case(2, 6001)
    sdr, sir, sar, perm, status = _gpu(ref, ref)
    assert status.tolist() == [0, 0, 0] and (perm == np.arange(2)).all()
    assert (sdr >= 100).all() and (sar >= 100).all(), (sdr, sar)            # roundoff-limited, or +inf


def test_repeatable_bitwise_and_independent_of_the_batch():
    ref, est, _ = _case(3, 6001)
    a = _gpu(ref, est, return_pairs=True)
    b = _gpu(ref, est, return_pairs=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for i in range(3):
        one = _gpu(ref[i], est[i], return_pairs=True)
        for x, y in zip(a, one):
            assert np.array_equal(x[i], y[0])


# ---------------------------------------------------------------------------------------------------------------------
def _small_cfg():
    import voicesplit_amd as V
    c = V.default_config(lstm_dim=32, fc1_dim=48, model_name="voicesplit")
    c.loss["loss_name"] = "si_snr"
    return c


def _speaker_waves(n):
    """mixture [2, n] and its two speakers [2, 2, n] (the target and the interferer of two demo clips), fp32."""
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    tgt = clips["target"][:2, 8000:8000 + n].astype(np.float32) / 32767.0
    mix = clips["mixed"][:2, 8000:8000 + n].astype(np.float32) / 32767.0
    return mix, np.stack([tgt, mix - tgt], axis=1)


def _by_hand(tr, acfg, batch):
    """forward_multi -> spec_to_wav -> the restatement: the quantities evaluate_speakers reports."""
    from voicesplit_amd import audio
    emb, mixed, phase, tw = batch
    B, K = emb.shape[:2]
    tr.model.eval()
    with torch.no_grad():
        masks = tr.model.forward_multi(mixed, emb)
        rep = lambda t: t[:, None].expand(B, K, *t.shape[1:]).reshape(B * K, *t.shape[1:]).contiguous()
        est = audio.spec_to_wav(rep(mixed), rep(phase), acfg, mask=masks.reshape(B * K, *mixed.shape[1:]).contiguous())
    tr.model.train()
    want = M.bss_eval_batch(tw.numpy(), est.view(B, K, -1).cpu().numpy())
    ok = want[4] == 0                                                       # items the restatement can score
    if not ok.any():
        return dict.fromkeys(("sdr", "sir", "sar", "confusion"), float("nan"))
    diag = np.diagonal(want[5], axis1=2, axis2=3)[ok]                       # [items, 3, K]
    out = {name: float(diag[:, c].mean()) for c, name in enumerate(("sdr", "sir", "sar"))}
    out["confusion"] = float(np.mean([(p != np.arange(K)).any() for p in want[3][ok]]))
    return out


def test_evaluate_speakers_equals_the_restatement_by_hand():
    import voicesplit_amd as V
    from voicesplit_amd import audio
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg()
    acfg = c.audio[c.audio["backend"]]
    torch.manual_seed(3)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    hop = int(acfg["hop_length"])
    mix, spk = _speaker_waves(hop * 60)                                     # T = 61 frames
    mixed, phase = audio.wav_to_spec(torch.from_numpy(mix).cuda(), acfg, want_phase=True)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(2, 2, 256, generator=g)
    emb = (emb / emb.norm(dim=2, keepdim=True)).cuda()
    batch = (emb, mixed, phase, torch.from_numpy(spk))
    got = tr.evaluate_speakers([batch])
    assert tr.model.training and sorted(got) == ["confusion", "sar", "sdr", "sir"]
    want = _by_hand(tr, acfg, batch)
    print("evaluate_speakers:", got, "by hand:", want)
    for k in ("sdr", "sir", "sar"):
        assert abs(got[k] - want[k]) <= TOL_DB, (k, got[k], want[k])
    assert got["confusion"] in (0.0, 0.5, 1.0) and got["confusion"] == want["confusion"]
    # an unscorable item (a silent speaker) is skipped; nothing left: NaN
    spk2 = spk.copy()
    spk2[1, 1] = 0.0
    silent = (emb, mixed, phase, torch.from_numpy(spk2.copy()))
    one, first = tr.evaluate_speakers([silent]), _by_hand(tr, acfg, silent)
    assert all(abs(one[k] - first[k]) <= TOL_DB for k in ("sdr", "sir", "sar")) and one["confusion"] == first["confusion"]
    assert one["confusion"] in (0.0, 1.0)
    spk2[0, 0] = 0.0
    none = tr.evaluate_speakers([(emb, mixed, phase, torch.from_numpy(spk2))])
    assert all(np.isnan(v) for v in none.values())


def test_evaluate_cli_speakers_csv(tmp_path, capsys):
    import voicesplit_amd as V
    from scipy.io import wavfile
    from voicesplit_amd import evaluate
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg()
    hop = int(c.audio[c.audio["backend"]]["hop_length"])
    data = tmp_path / "test"
    data.mkdir()
    mix, spk = _speaker_waves(hop * 60)
    g = torch.Generator().manual_seed(8)
    rows = []
    for i in range(2):
        wavfile.write(str(data / f"{i}-mixed.wav"), 16000, mix[i])
        row = [f"{i}-mixed.wav"]
        for k in range(2):
            e = torch.randn(256, generator=g)
            torch.save(e / e.norm(), str(data / f"{i}-{k}-emb.pt"))
            wavfile.write(str(data / f"{i}-{k}-target.wav"), 16000, spk[i, k])
            row += [f"{i}-{k}-emb.pt", f"{i}-{k}-target.wav"]
        rows.append(",".join(row))
    csv = tmp_path / "speakers.csv"
    csv.write_text("\n".join(rows) + "\n")
    c["test_config"] = {"batch_size": 2, "num_workers": 1}
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({k: (dict(v) if isinstance(v, dict) else v) for k, v in c.items()}, indent=1))
    ck = tmp_path / "ckpts"
    ck.mkdir()
    torch.manual_seed(1)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    tr.save_checkpoint(str(ck / "checkpoint_1.pt"))
    m = evaluate.main(["-c", str(cfg), "-d", str(data), "--checkpoint_path", str(ck / "checkpoint_1.pt"), "--speakers-csv", str(csv)])
    out = capsys.readouterr().out
    for name, key in (("Mean Test SDR", "sdr"), ("Mean Test SIR", "sir"), ("Mean Test SAR", "sar"), ("Speaker confusion", "confusion")):
        assert f"{name}: {m[key]}" in out
        assert np.isfinite(m[key])
    direct = tr.evaluate_speakers(evaluate.speaker_batches(c, evaluate.read_speakers_csv(str(csv)), str(data), torch.device("cuda", 0)))
    assert direct == m
    table = evaluate.main(["-c", str(cfg), "-d", str(data), "--checkpoints_path", str(ck), "--speakers-csv", str(csv)])
    assert len(table) == 1 and all(table[0][k] == m[k] for k in m)
    saved = json.loads((ck / "speakers_per_checkpoint.json").read_text())
    assert saved["best_sdr"]["checkpoint"] == table[0]["checkpoint"]
