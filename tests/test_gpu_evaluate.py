"""GPU: Trainer.evaluate (mean test loss + mean BSS-eval SDR, the test=True branch of the reference's validation) and the
checkpoint evaluation CLI voicesplit_amd.evaluate (test.py / test_all_checkpoints.py), in-process."""
import json
import os

import numpy as np
import pytest
import torch

import bss_eval_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def _small_cfg(model_name, loss_name):
    import voicesplit_amd as V
    c = V.default_config(lstm_dim=32, fc1_dim=48, model_name=model_name)
    c.loss["loss_name"] = loss_name
    return c


def _demo_batches(c):
    from voicesplit_amd import audio
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    acfg = c.audio[c.audio["backend"]]
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(4, 256, generator=g)
    emb = emb / emb.norm(dim=1, keepdim=True)
    out = []
    for lo in (0, 2):                                             # two batches of two clips
        tw = torch.from_numpy(clips["target"][lo:lo + 2].astype(np.float32) / 32767.0)
        mw = torch.from_numpy(clips["mixed"][lo:lo + 2].astype(np.float32) / 32767.0).cuda()
        mixed, phase = audio.wav_to_spec(mw, acfg, want_phase=True)
        target, _ = audio.wav_to_spec(tw.cuda(), acfg, want_phase=False)
        seq_len = torch.full((2,), mw.shape[1], dtype=torch.int32, device="cuda")
        out.append((emb[lo:lo + 2].cuda(), target, mixed, seq_len, tw, phase))
    return out


@pytest.mark.parametrize("loss_name", ["si_snr", "power_law_compression"])
def test_evaluate_equals_validate_and_the_restated_sdr(loss_name):
    import voicesplit_amd as V
    from voicesplit_amd import audio
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg("voicesplit", loss_name)
    torch.manual_seed(3)
    tr = Trainer(V.VoiceSplit(c).cuda(), c)
    batches = _demo_batches(c)
    tr.train_step(batches[0])                                      # BatchNorm running statistics away from their init
    mean_loss, mean_sdr = tr.evaluate(batches)
    assert tr.model.training
    assert mean_loss == tr.validate(batches)
    # the restatement applied to the GPU's own estimate
    tr.model.eval()
    acfg = c.audio[c.audio["backend"]]
    sdrs = []
    with torch.no_grad():
        for emb, _t, mixed, _s, tw, phase in batches:
            est = audio.spec_to_wav(mixed, phase, acfg, mask=tr.model(mixed, emb)).cpu().numpy()
            sdrs += list(R.sdr_rows(tw.numpy(), est)[0])
    assert np.isfinite(sdrs).all() and abs(mean_sdr - float(np.mean(sdrs))) <= 1e-6, (mean_sdr, sdrs)


def _write_dataset(d, lengths):
    from scipy.io import wavfile
    clips = np.load(os.path.join(GOLDEN_DIR, "demo_clips.npz"))
    g = torch.Generator().manual_seed(8)
    for i, n in enumerate(lengths):
        stem = os.path.join(d, "%06d" % i)
        e = torch.randn(256, generator=g)
        torch.save(e / e.norm(), stem + "-emb.pt")
        wavfile.write(stem + "-target.wav", 16000, clips["target"][i % 4][:n].astype(np.float32) / 32767.0)
        wavfile.write(stem + "-mixed.wav", 16000, clips["mixed"][i % 4][:n].astype(np.float32) / 32767.0)


def test_evaluate_cli_single_and_all_checkpoints(tmp_path, capsys):
    import voicesplit_amd as V
    from voicesplit_amd import evaluate
    from voicesplit_amd.trainer import Trainer
    c = _small_cfg("voicesplit", "si_snr")
    data = tmp_path / "test"
    data.mkdir()
    _write_dataset(str(data), [48000] * 4)
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
    torch.manual_seed(2)
    tr2 = Trainer(V.VoiceSplit(c).cuda(), c)
    tr2.save_checkpoint(str(ck / "checkpoint_2.pt"))
    # one checkpoint: test.py's two lines
    loss1, sdr1 = evaluate.main(["-c", str(cfg), "-d", str(data), "--checkpoint_path", str(ck / "checkpoint_1.pt")])
    out = capsys.readouterr().out
    assert f"Mean Test Loss: {loss1}" in out and f"Mean Test SDR: {sdr1}" in out
    assert np.isfinite(loss1) and np.isfinite(sdr1)
    # every checkpoint of the directory: best by SDR copied, the table as JSON
    table = evaluate.main(["-c", str(cfg), "-d", str(data), "--checkpoints_path", str(ck)])
    assert [os.path.basename(t["checkpoint"]) for t in table] == ["checkpoint_1.pt", "checkpoint_2.pt"]
    assert table[0]["mean_loss"] == loss1 and table[0]["mean_sdr"] == sdr1
    best = max(table, key=lambda t: t["mean_sdr"])
    assert "Best SDR checkpoint is: " in capsys.readouterr().out
    with open(best["checkpoint"], "rb") as f1, open(ck / "best_checkpoint.pt", "rb") as f2:
        assert f1.read() == f2.read()
    saved = json.loads((ck / "sdr_loss_per_checkpoint.json").read_text())
    assert saved["best_sdr"]["checkpoint"] == best["checkpoint"] and len(saved["checkpoints"]) == 2
    # a second pass skips best_checkpoint.pt
    again = evaluate.main(["-c", str(cfg), "-d", str(data), "--checkpoints_path", str(ck)])
    assert len(again) == 2
    # items of one batch with different lengths: refused, naming the files
    bad = tmp_path / "bad"
    bad.mkdir()
    _write_dataset(str(bad), [48000, 32000])
    with pytest.raises(ValueError, match="000001-target.wav"):
        evaluate.main(["-c", str(cfg), "-d", str(bad), "--checkpoint_path", str(ck / "checkpoint_1.pt")])
