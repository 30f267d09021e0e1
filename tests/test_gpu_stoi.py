"""GPU: vs_stoi / metrics.stoi (STOI and ESTOI at 10 kHz, csrc/stoi.hip) against the fp64 restatement tests/stoi_ref.py.

Counts (F, Mk) and status are exact.  The tolerances are not chosen: they are 64 times the distance between the restatement's own two
forms (rfft with natural sums against an explicit matrix DFT with reversed sums) measured on the very inputs of this file, the margin
tests/test_gpu_loudness.py uses against its own two forms; one for the scores d (absolute; d lies in [-1, 1]) and one for the envelopes
(relative, element by element).  The keep mask is a threshold: the CPU test asserts that no frame of these inputs sits within 1e-6 dB
of it.  Independence of position, batch and call is bit-exact (torch.equal), with NaN around every clip."""
import json
import os

import numpy as np
import pytest
import torch

import stoi_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    """The restatement on every input of this file, computed once and never written to; the two tolerances."""
    pairs, edge = SR.gpu_test_pairs() + SR.long_pairs(), SR.edge_pairs()
    dist_d, dist_env, margin = SR.form_distance(pairs + edge)
    assert margin >= 1e-6 and dist_d > 0.0 and dist_env > 0.0
    want = {ext: [SR.score(x, y, ext, 1) for _, x, y in pairs] for ext in (False, True)}
    assert want[False][-1]["F"] == 311 and want[False][-1]["Mk"] > 93          # two compaction steps, a fold over more than 64 segments
    want_edge = {ext: [SR.score(x, y, ext, 1) for _, x, y in edge] for ext in (False, True)}
    print(f"form distance: d {dist_d:.3e}, envelopes {dist_env:.3e} (relative); gate margin {margin:.3f} dB")
    return {"pairs": pairs, "edge": edge, "want": want, "want_edge": want_edge, "tol_d": 64 * dist_d, "tol_env": 64 * dist_env}


def _device(pairs, extended, lead=5, gap=3, envelopes=True):
    """One ragged vs_stoi call over [(name, x, y)]: the clips `gap` samples apart from sample `lead` on in buffers full of NaN."""
    from voicesplit_amd import metrics
    at, rows = lead, []
    for _, x, _ in pairs:
        rows.append((at, len(x)))
        at += len(x) + gap
    flat_x = torch.full((at + 7,), float("nan"), dtype=torch.float32)
    flat_y = flat_x.clone()
    for (a, n), (_, x, y) in zip(rows, pairs):
        flat_x[a:a + n] = torch.from_numpy(np.asarray(x))
        flat_y[a:a + n] = torch.from_numpy(np.asarray(y))
    table = torch.tensor(rows, dtype=torch.int64)
    out = metrics.stoi_clips(flat_x.cuda(), flat_y.cuda(), table, extended=extended, envelopes=envelopes)
    d, frames, status = (t.cpu() for t in out[:3])
    envs = None
    if envelopes:
        tob, tob_at = out[3].cpu(), out[4].tolist()
        envs = [tob[o:o + 30 * int(mk)].reshape(2, 15, int(mk)) for o, mk in zip(tob_at, frames[:, 1].tolist())]
    return d, frames, status, envs


@pytest.mark.parametrize("extended", [False, True])
def test_counts_status_envelopes_and_scores(ref, extended):
    d, frames, status, envs = _device(ref["pairs"], extended)
    want = ref["want"][extended]
    for i, ((name, _, _), w) in enumerate(zip(ref["pairs"], want)):
        got_f, got_mk = frames[i].tolist()
        err_env = 0.0
        for k, key in enumerate(("X", "Y")):
            err_env = max(err_env, float((np.abs(envs[i][k].numpy() - w[key]) / np.abs(w[key])).max()))
        print(f"{name} extended={extended}: F {got_f} Mk {got_mk} status {int(status[i])} d {float(d[i]):.15f} "
              f"|d - ref| {abs(float(d[i]) - w['d']):.2e} (bound {ref['tol_d']:.2e}) envelopes rel {err_env:.2e} (bound {ref['tol_env']:.2e})")
        assert (got_f, got_mk, int(status[i])) == (w["F"], w["Mk"], w["status"]), name
        assert err_env <= ref["tol_env"], name
        if w["status"] == 1:
            assert float(d[i]) == 1e-5, name
        else:
            assert abs(float(d[i]) - w["d"]) <= ref["tol_d"], name
    assert sorted({(int(f), int(m)) for f, m in frames[:12].tolist()}) == sorted({(c[2], c[3]) for c in SR.CLIPS})
    assert len(want) == 13 and frames[12].tolist() == [311, want[12]["Mk"]]


@pytest.mark.parametrize("extended", [False, True])
def test_frame_count_edges(ref, extended):
    d, frames, status, _ = _device(ref["edge"], extended)
    want = ref["want_edge"][extended]
    assert [len(x) for _, x, _ in ref["edge"]] == [255, 256, 383, 384, 3967, 3968]
    assert frames[:, 0].tolist() == [0, 1, 1, 2, 29, 30] == frames[:, 1].tolist()
    assert status.tolist() == [1, 1, 1, 1, 1, 0] == [w["status"] for w in want]
    assert d[:5].tolist() == [1e-5] * 5
    print(f"n = 3968 extended={extended}: d {float(d[5]):.15f} |d - ref| {abs(float(d[5]) - want[5]['d']):.2e} (bound {ref['tol_d']:.2e})")
    assert abs(float(d[5]) - want[5]["d"]) <= ref["tol_d"]


@pytest.mark.parametrize("extended", [False, True])
def test_position_batch_and_call_independence(ref, extended):
    """The 8000-sample clip with its 5 dB estimate: alone at offset 0; fifth of a batch of 7 with other neighbours at an offset that
    is no multiple of 4; in a second call.  Bit for bit the same score and envelopes, with NaN around every clip."""
    pairs = ref["pairs"]
    mine = pairs[4]
    assert len(mine[1]) == 8000
    d0, f0, s0, e0 = _device([mine], extended, lead=0, gap=0)
    batch = [pairs[0], pairs[9], pairs[7], pairs[2], mine, pairs[11], pairs[3]]
    d1, f1, s1, e1 = _device(batch, extended, lead=5, gap=3)
    assert (5 + sum(len(p[1]) + 3 for p in batch[:4])) % 4 != 0
    d2, f2, s2, e2 = _device(batch[::-1], extended, lead=2, gap=1)
    assert not torch.isnan(d1).any() and not torch.isnan(d2).any() and not any(torch.isnan(e).any() for e in e1 + e2)
    assert torch.equal(d0[0], d1[4]) and torch.equal(d0[0], d2[2])
    assert torch.equal(f0[0], f1[4]) and torch.equal(f0[0], f2[2]) and int(s0[0]) == int(s1[4]) == int(s2[2]) == 0
    assert torch.equal(e0[0], e1[4]) and torch.equal(e0[0], e2[2])
    d3, _, _, e3 = _device(batch, extended, lead=5, gap=3)                              # the same call again
    assert torch.equal(d1, d3) and all(torch.equal(a, b) for a, b in zip(e1, e3))
    # every other clip of the batch too, against the reversed batch
    for i in range(7):
        assert torch.equal(d1[i], d2[6 - i]) and torch.equal(e1[i], e2[6 - i]), i


def _speech16(n, seeds):
    x = np.stack([SR.speech(n, (n // 3, n // 2), s) for s in seeds])
    y = np.stack([SR.noisy(r, 5.0, 30 + s) for r, s in zip(x, seeds)])
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def test_metrics_stoi_resamples_and_keeps_shapes():
    from voicesplit_amd import _lib, metrics
    from voicesplit_amd.resample import Resampler
    N = 14000
    x, y = _speech16(N, (1, 2, 3, 4, 5, 6))
    rs = Resampler(16000, 10000, x.device)
    x10, y10 = rs(x), rs(y)
    n10 = x10.shape[1]
    table = torch.stack((torch.arange(6) * n10, torch.full((6,), n10)), dim=1).to(torch.int64)
    for extended in (False, True):
        want_d, _, want_s = metrics.stoi_clips(x10.reshape(-1), y10.reshape(-1), table, extended=extended)
        d, s = metrics.stoi(x, y, 16000, extended=extended)
        assert d.shape == (6,) and d.dtype == torch.float64 and s.dtype == torch.int32 and d.device == x.device
        assert torch.equal(d, want_d) and torch.equal(s, want_s) and int(s.sum()) == 0
        assert float(d.min()) > 0.05 and float(d.max()) < 1.0
        d3, s3 = metrics.stoi(x.view(2, 3, N), y.view(2, 3, N), extended=extended)      # 16000 is the default
        assert d3.shape == (2, 3) and torch.equal(d3.reshape(-1), d) and torch.equal(s3.reshape(-1), s)
        d1, s1 = metrics.stoi(x[2], y[2], 16000, extended=extended)
        assert d1.shape == () and torch.equal(d1, d[2]) and int(s1) == 0
        # at 10 kHz nothing is resampled
        dd, ss = metrics.stoi(x10, y10, 10000, extended=extended)
        assert torch.equal(dd, want_d) and torch.equal(ss, want_s)
        # a padded ragged batch: NaN behind every row's own length, each row as the unpadded clip
        lengths = [N, 9000, 12345]
        xp = torch.full((3, N), float("nan"), device=x.device)
        yp = xp.clone()
        for b, n in enumerate(lengths):
            xp[b, :n], yp[b, :n] = x[b, :n], y[b, :n]
        dl, sl = metrics.stoi(xp, yp, 16000, extended=extended, lengths=lengths)
        for b, n in enumerate(lengths):
            alone = metrics.stoi(x[b, :n].contiguous(), y[b, :n].contiguous(), 16000, extended=extended)
            assert torch.equal(dl[b], alone[0]) and torch.equal(sl[b], alone[1]), (b, n)
        dk, _ = metrics.stoi(xp[:2, None].expand(2, 2, N).contiguous(), yp[:2, None].expand(2, 2, N).contiguous(), 16000,
                             extended=extended, lengths=torch.tensor(lengths[:2]))
        assert dk.shape == (2, 2) and torch.equal(dk[:, 0], dl[:2]) and torch.equal(dk[:, 1], dl[:2])
        both = metrics.stoi_pair(x, y, 16000)
        assert torch.equal(both[1 if extended else 0], d) and torch.equal(both[2], s)
    # refusals
    with pytest.raises(TypeError, match="float32"):
        metrics.stoi(x.double(), y.double())
    with pytest.raises(TypeError, match="float32"):
        metrics.stoi(x, y.half())
    with pytest.raises(ValueError, match="shape"):
        metrics.stoi(x, y[:, :-1])
    with pytest.raises(ValueError, match="expected"):
        metrics.stoi(x[None, None], y[None, None])
    with pytest.raises(ValueError, match="lengths"):
        metrics.stoi(x, y, lengths=[N] * 5)
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        metrics.stoi(x.cpu(), y.cpu())


def _mean(values):
    return float(np.sum(values) / len(values)) if len(values) else float("nan")


def test_evaluate_intelligibility_equals_per_item_calls():
    import voicesplit_amd as V
    from test_gpu_evaluate import _demo_batches, _small_cfg
    from voicesplit_amd import audio, metrics
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg("voicesplit", "si_snr")
    torch.manual_seed(3)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    batches = _demo_batches(c)
    before = tr.evaluate(batches)
    got = tr.evaluate_intelligibility(batches)
    assert tr.model.training and sorted(got) == ["estoi", "scored", "skipped", "stoi"]
    assert tr.evaluate(batches) == before                                               # evaluate is untouched by it
    acfg = c.audio[c.audio["backend"]]
    tr.model.eval()
    vals = {False: [], True: []}
    skipped = 0
    with torch.no_grad():
        for emb, _t, mixed, _s, tw, phase in batches:
            est = audio.spec_to_wav(mixed, phase, acfg, mask=tr.model(mixed, emb))
            for b in range(est.shape[0]):
                for extended in (False, True):
                    d, s = metrics.stoi(tw[b].cuda(), est[b].contiguous(), 16000, extended=extended)
                    if int(s) == 0:
                        vals[extended].append(float(d))
                skipped += int(s)
    tr.model.train()
    print("evaluate_intelligibility:", got, "per item:", vals)
    assert got["scored"] == len(vals[False]) == 4 and got["skipped"] == skipped == 0
    # the same fp64 values summed in another order: a few units of 2^-53 per term
    assert abs(got["stoi"] - _mean(vals[False])) <= 1e-14 and abs(got["estoi"] - _mean(vals[True])) <= 1e-14
    assert 0.0 < got["estoi"] < 1.0 and 0.0 < got["stoi"] < 1.0
    # a batch whose targets are too short to score: skipped and counted, NaN when nothing is left
    emb, target, mixed, seq_len, tw, phase = batches[0]
    quiet = tw.clone()
    quiet[:, 3000:] = 0.0                                                               # under 0.2 s of signal: fewer than 30 frames
    none = tr.evaluate_intelligibility([(emb, target, mixed, seq_len, quiet, phase)])
    assert none["scored"] == 0 and none["skipped"] == 2 and np.isnan(none["stoi"]) and np.isnan(none["estoi"])


def test_evaluate_speakers_with_stoi():
    import voicesplit_amd as V
    from test_gpu_bss_eval import _small_cfg, _speaker_waves
    from voicesplit_amd import audio, metrics
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg()
    acfg = c.audio[c.audio["backend"]]
    torch.manual_seed(3)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    mix, spk = _speaker_waves(int(acfg["hop_length"]) * 150)
    mixed, phase = audio.wav_to_spec(torch.from_numpy(mix).cuda(), acfg, want_phase=True)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(2, 2, 256, generator=g)
    emb = (emb / emb.norm(dim=2, keepdim=True)).cuda()
    batch = (emb, mixed, phase, torch.from_numpy(spk))
    plain = tr.evaluate_speakers([batch])
    got = tr.evaluate_speakers([batch], stoi=True)
    assert sorted(plain) == ["confusion", "sar", "sdr", "sir"] and sorted(got) == ["confusion", "estoi", "sar", "sdr", "sir", "stoi"]
    assert all(got[k] == plain[k] for k in plain)
    tr.model.eval()
    with torch.no_grad():
        masks = tr.model.forward_multi(mixed, emb)
        B, K, T, F = emb.shape[0], emb.shape[1], mixed.shape[1], mixed.shape[2]
        rep = lambda t: t[:, None].expand(B, K, T, F).reshape(B * K, T, F).contiguous()
        est = audio.spec_to_wav(rep(mixed), rep(phase), acfg, mask=masks.reshape(B * K, T, F).contiguous())
    tr.model.train()
    refs = torch.from_numpy(spk).cuda().reshape(B * K, -1)
    for key, extended in (("stoi", False), ("estoi", True)):
        vals = []
        for r in range(B * K):
            d, s = metrics.stoi(refs[r].contiguous(), est[r].contiguous(), 16000, extended=extended)
            if int(s) == 0:
                vals.append(float(d))
        print(key, got[key], vals)
        assert len(vals) > 0 and abs(got[key] - _mean(vals)) <= 1e-14


def test_evaluate_cli_speakers_csv_with_stoi(tmp_path, capsys):
    import voicesplit_amd as V
    from scipy.io import wavfile
    from test_gpu_bss_eval import _small_cfg, _speaker_waves
    from voicesplit_amd import evaluate
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg()
    data = tmp_path / "test"
    data.mkdir()
    mix, spk = _speaker_waves(int(c.audio[c.audio["backend"]]["hop_length"]) * 150)
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
    torch.manual_seed(1)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    tr.save_checkpoint(str(tmp_path / "checkpoint_1.pt"))
    args = ["-c", str(cfg), "-d", str(data), "--checkpoint_path", str(tmp_path / "checkpoint_1.pt"), "--speakers-csv", str(csv)]
    plain = evaluate.main(args)
    before = capsys.readouterr().out
    assert "STOI" not in before and sorted(plain) == ["confusion", "sar", "sdr", "sir"]
    m = evaluate.main(args + ["--stoi"])
    out = capsys.readouterr().out
    assert out == before + f"Mean Test STOI: {m['stoi']}\nMean Test ESTOI: {m['estoi']}\n"
    assert all(m[k] == plain[k] for k in plain) and 0.0 < m["estoi"] < 1.0 and 0.0 < m["stoi"] < 1.0


def test_evaluate_cli_stoi(tmp_path, capsys):
    import voicesplit_amd as V
    from test_gpu_evaluate import _small_cfg, _write_dataset
    from voicesplit_amd import evaluate
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg("voicesplit", "si_snr")
    data = tmp_path / "test"
    data.mkdir()
    _write_dataset(str(data), [48000] * 2)
    c.dataset = {"train_dir": str(data), "test_dir": str(data),
                 "format": {"emb": "*-emb.pt", "mixed": "*-mixed.pt", "target": "*-target.pt",
                            "target_wav": "*-target.wav", "mixed_wav": "*-mixed.wav"}}
    c["test_config"] = {"batch_size": 2, "num_workers": 1}
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({k: (dict(v) if isinstance(v, dict) else v) for k, v in c.items()}, indent=1))
    ck = tmp_path / "ckpts"
    ck.mkdir()
    torch.manual_seed(1)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    tr.save_checkpoint(str(ck / "checkpoint_1.pt"))
    common = ["-c", str(cfg), "-d", str(data)]
    one = ["--checkpoint_path", str(ck / "checkpoint_1.pt")]
    # without the flag: the two lines of before and nothing else
    loss, sdr = evaluate.main(common + one)
    assert capsys.readouterr().out == f"Mean Test Loss: {loss}\nMean Test SDR: {sdr}\n"
    # with it: the same two lines, then the two new ones
    res = evaluate.main(common + one + ["--stoi"])
    out = capsys.readouterr().out
    assert res[:2] == (loss, sdr) and len(res) == 4
    assert out == f"Mean Test Loss: {loss}\nMean Test SDR: {sdr}\nMean Test STOI: {res[2]}\nMean Test ESTOI: {res[3]}\n"
    assert 0.0 < res[3] < 1.0 and 0.0 < res[2] < 1.0
    direct = tr.evaluate_intelligibility(evaluate.eval_batches(c, evaluate.EvalDataset(c, str(data)), torch.device("cuda", 0)))
    assert (direct["stoi"], direct["estoi"], direct["scored"]) == (res[2], res[3], 2)
    # every checkpoint of a directory: the fields of the table, with and without the flag
    table = evaluate.main(common + ["--checkpoints_path", str(ck), "--stoi", "--json", str(tmp_path / "with.json")])
    assert "Mean Test STOI:" in capsys.readouterr().out
    assert table[0]["mean_stoi"] == res[2] and table[0]["mean_estoi"] == res[3] and table[0]["mean_sdr"] == sdr
    assert json.loads((tmp_path / "with.json").read_text())["checkpoints"][0]["mean_estoi"] == res[3]
    table = evaluate.main(common + ["--checkpoints_path", str(ck), "--json", str(tmp_path / "without.json")])
    assert "STOI" not in capsys.readouterr().out and sorted(table[0]) == ["checkpoint", "mean_loss", "mean_sdr"]
    # ragged: items of unequal length, each at its own length
    rag = tmp_path / "ragged"
    rag.mkdir()
    _write_dataset(str(rag), [48000, 32000])
    res = evaluate.main(["-c", str(cfg), "-d", str(rag)] + one + ["--ragged", "--stoi"])
    out = capsys.readouterr().out
    assert out.splitlines()[2:] == [f"Mean Test STOI: {res[2]}", f"Mean Test ESTOI: {res[3]}"] and np.isfinite(res[2:]).all()
    ds = evaluate.EvalDataset(c, str(rag))
    by_item = tr.evaluate_intelligibility(evaluate.eval_batches(c, ds, torch.device("cuda", 0), ragged=True), ragged=True)
    assert (by_item["stoi"], by_item["estoi"], by_item["scored"]) == (res[2], res[3], 2)
