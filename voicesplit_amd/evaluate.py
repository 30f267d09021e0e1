"""Checkpoint evaluation on the GPU: the reference's test.py and test_all_checkpoints.py.

    python -m voicesplit_amd.evaluate -c config.json -d TEST_DIR --checkpoint_path checkpoint_1000.pt
        Mean Test Loss: ...
        Mean Test SDR: ...
    python -m voicesplit_amd.evaluate -c config.json -d TEST_DIR --checkpoints_path LOG_DIR [--json FILE]
        every *.pt of LOG_DIR but best_checkpoint.pt, in sorted order; prints the best checkpoint by SDR and by loss,
        copies the best by SDR to LOG_DIR/best_checkpoint.pt and writes the per-checkpoint table as JSON
        (default LOG_DIR/sdr_loss_per_checkpoint.json; the reference writes a .np array)

Items are read as the reference's evaluation dataset reads them (utils/dataset.py:43-56): the embedding (``*-emb.pt``),
the target and mixed waveforms (``c.dataset['format']``); the mixture's spectrogram and phase and the target spectrogram
come from the GPU front end (``audio.wav_to_spec``), the estimate from ``audio.spec_to_wav`` and the SDR from
``metrics.bss_sdr`` -- the whole of ``validation(test=True)`` (utils/generic_utils.py:476-530) on the device, in batches of
``c.test_config['batch_size']`` items (which must share a length).  Scores are ``Trainer.evaluate``'s.

``--ragged``: the items may differ in length (the reference's own test sets do, which is why it scores them one by one).
Batches of at most ``batch_size`` items are planned over the whole set by length (``streaming.plan_ragged_batches``), the
network runs each padded batch with every item computed as if alone (``model.forward_ragged``), and loss and SDR are taken
per item at its own length and averaged over items (``Trainer.evaluate_ragged``).

``--speakers-csv FILE``: several enrolled speakers per mixture.  Every row of FILE is
``mixed_wav,emb_1,target_wav_1,...,emb_K,target_wav_K`` (paths relative to ``-d``, the same K in every row); the K speakers
are extracted in one pass (``model.forward_multi``) and scored with the multi-source BSS-eval (``metrics.bss_eval``) by
``Trainer.evaluate_speakers``:

        Mean Test SDR: ...  Mean Test SIR: ...  Mean Test SAR: ...      (output k against speaker k)
        Speaker confusion: ...                                            (share of items whose best permutation is not the identity)

Under ``--checkpoints_path`` the four numbers are printed and written per checkpoint; the best checkpoint is the one with
the largest mean SDR.

``--stoi``: the intelligibility scores beside the distortion ones (``Trainer.evaluate_intelligibility``, or
``Trainer.evaluate_speakers(stoi=True)`` with ``--speakers-csv``; ``metrics.stoi`` -- restated, not compared with a pystoi run):

        Mean Test STOI: ...
        Mean Test ESTOI: ...

after the lines above, and the fields ``mean_stoi`` / ``mean_estoi`` (``stoi`` / ``estoi`` with ``--speakers-csv``) in the ``--json``
table.  Without the flag nothing changes.
"""
import argparse
import csv
import json
import os
import shutil
from glob import glob

import torch

from .config import resolve_audio
from .trainer import Trainer, load_wav


class EvalDataset:
    """(emb, target_wav, mixed_wav, names) per item of ``test_dir``, sorted by the ``c.dataset['format']`` globs."""

    def __init__(self, c, test_dir: str):
        if not os.path.isdir(test_dir):
            raise FileNotFoundError("Test or Train dataset dir is incorrect! Fix it in config.json: " + str(test_dir))
        fmt = c.dataset["format"]
        find = lambda g: sorted(glob(os.path.join(test_dir, g)))
        self.emb, self.target_wav, self.mixed_wav = (find(fmt[k]) for k in ("emb", "target_wav", "mixed_wav"))
        if not (len(self.emb) == len(self.target_wav) == len(self.mixed_wav)):
            raise ValueError(" The number of target and mixed Specs and Embs not Match! Check its")
        if not self.emb:
            raise ValueError(f" Test files not found in {test_dir}!")
        self.sr = int(resolve_audio(c.audio)["sample_rate"])

    def __len__(self):
        return len(self.emb)

    def __getitem__(self, i):
        return (torch.load(self.emb[i]), load_wav(self.target_wav[i], self.sr), load_wav(self.mixed_wav[i], self.sr),
                (self.emb[i], self.target_wav[i], self.mixed_wav[i]))


def _ragged_batches(c, ds: EvalDataset, device, bs: int):
    """``Trainer.evaluate_ragged``'s batches over the whole set: at most ``bs`` items each, grouped by length."""
    from . import audio
    from .streaming import plan_ragged_batches
    acfg = resolve_audio(c.audio)
    if acfg.get("mel_spec"):
        raise ValueError("ragged evaluation: forward_ragged takes linear spectrograms; config.audio['mel_spec'] is set")
    hop = int(acfg["hop_length"])
    items = [it for it in (ds[i] for i in range(len(ds))) if it[0].tolist() != [0]]
    for it in items:
        if it[1].shape[0] != it[2].shape[0]:
            raise ValueError(f"target and mixture differ in length: {os.path.basename(it[3][1])} ({it[1].shape[0]}) / "
                             f"{os.path.basename(it[3][2])} ({it[2].shape[0]})")
    if not items:
        return
    frames = [audio.frames_for(it[2].shape[0], hop) for it in items]
    for batch in plan_ragged_batches(frames, bs, bs * max(frames)):
        specs = []
        for i in batch:                                   # the STFT reflects at the clip's own ends: front end per item
            mixed, phase = audio.wav_to_spec(items[i][2].to(device).reshape(1, -1), acfg, want_phase=True)
            target, _ = audio.wav_to_spec(items[i][1].to(device).reshape(1, -1), acfg, want_phase=False)
            specs.append((mixed[0], phase[0], target[0]))
        mixed, lens = audio.pad_specs([s[0] for s in specs])
        phase, _ = audio.pad_specs([s[1] for s in specs])
        target, _ = audio.pad_specs([s[2] for s in specs])
        emb = torch.stack([items[i][0].float().reshape(-1) for i in batch]).to(device)
        seq_len = torch.tensor([items[i][2].shape[0] for i in batch], dtype=torch.int32, device=device)
        yield emb, target, mixed, seq_len, [items[i][1] for i in batch], phase, lens


def eval_batches(c, ds: EvalDataset, device, ragged: bool = False):
    """``Trainer.evaluate``'s batches: (emb, target_spec, mixed_spec, seq_len, target_wav (host), mixed_phase), in dataset
    order, ``c.test_config['batch_size']`` items each; items whose embedding is [0] are dropped (utils/dataset.py:93-95).
    ragged: ``Trainer.evaluate_ragged``'s batches instead -- items of any length, planned over the whole set."""
    from . import audio
    acfg = resolve_audio(c.audio)
    bs = int(c["test_config"]["batch_size"]) if "test_config" in c else 1          # config.json:33-36 (1 when absent)
    if ragged:
        yield from _ragged_batches(c, ds, device, bs)
        return
    for lo in range(0, len(ds), bs):
        items = [ds[i] for i in range(lo, min(lo + bs, len(ds)))]
        items = [it for it in items if it[0].tolist() != [0]]
        if not items:
            continue
        lengths = {(it[1].shape[0], it[2].shape[0]) for it in items}
        if len(lengths) != 1 or items[0][1].shape[0] != items[0][2].shape[0]:
            desc = ", ".join(f"{os.path.basename(it[3][1])} ({it[1].shape[0]}) / {os.path.basename(it[3][2])} ({it[2].shape[0]})"
                             for it in items)
            raise ValueError(f"items of one test batch must share a length (test_config.batch_size = {bs}): {desc}")
        emb = torch.stack([it[0].float().reshape(-1) for it in items]).to(device)
        target_wav = torch.stack([it[1] for it in items])
        mixed_wav = torch.stack([it[2] for it in items]).to(device)
        seq_len = torch.full((len(items),), mixed_wav.shape[1], dtype=torch.int32, device=device)
        mixed, phase = audio.wav_to_spec(mixed_wav, acfg, want_phase=True)
        target, _ = audio.wav_to_spec(target_wav.to(device), acfg, want_phase=False)
        yield emb, target, mixed, seq_len, target_wav, phase


def read_speakers_csv(path: str):
    """The rows of a ``--speakers-csv`` file: ``[(mixed_wav, [(emb_1, target_wav_1), .., (emb_K, target_wav_K)]), ..]``.
    Empty lines and lines starting with '#' are skipped; every row must have 1 + 2 K fields with the same K >= 1."""
    rows = []
    with open(path, newline="") as f:
        for ln, rec in enumerate(csv.reader(f), 1):
            rec = [x.strip() for x in rec]
            if not rec or not any(rec) or rec[0].startswith("#"):
                continue
            if len(rec) < 3 or len(rec) % 2 != 1 or not all(rec):
                raise ValueError(f"{path}:{ln}: expected mixed_wav,emb_1,target_wav_1,...,emb_K,target_wav_K, got {len(rec)} fields")
            rows.append((rec[0], [(rec[i], rec[i + 1]) for i in range(1, len(rec), 2)]))
            if len(rows[-1][1]) != len(rows[0][1]):
                raise ValueError(f"{path}:{ln}: {len(rows[-1][1])} speakers, the rows before have {len(rows[0][1])}")
    if not rows:
        raise ValueError(f"{path}: no rows")
    return rows


def speaker_items(rows, root: str, sample_rate: int, load_emb=torch.load, load=load_wav):
    """(emb [K, E], target_wavs [K, S], mixed_wav [S], names) per row of ``read_speakers_csv``, paths taken relative to root."""
    for mixed, speakers in rows:
        emb = torch.stack([load_emb(os.path.join(root, e)).float().reshape(-1) for e, _ in speakers])
        targets = [load(os.path.join(root, t), sample_rate) for _, t in speakers]
        yield emb, targets, load(os.path.join(root, mixed), sample_rate), [mixed] + [t for _, t in speakers]


def group_speaker_items(items, bs: int):
    """Host batches of at most ``bs`` items in order: (emb [B, K, E], target_wavs [B, K, S], mixed_wav [B, S]); every waveform
    of one batch must have the same length."""
    items = list(items)
    for lo in range(0, len(items), bs):
        group = items[lo:lo + bs]
        lengths = {int(w.shape[0]) for it in group for w in it[1] + [it[2]]}
        if len(lengths) != 1:
            desc = ", ".join(f"{os.path.basename(n)} ({w.shape[0]})" for it in group for n, w in zip(it[3], [it[2]] + it[1]))
            raise ValueError(f"items of one test batch must share a length (test_config.batch_size = {bs}): {desc}")
        yield (torch.stack([it[0] for it in group]), torch.stack([torch.stack(it[1]) for it in group]),
               torch.stack([it[2] for it in group]))


def speaker_batches(c, rows, root: str, device):
    """``Trainer.evaluate_speakers``'s batches from the rows of a speakers CSV: (emb, mixed_spec, mixed_phase, target_wavs)."""
    from . import audio
    acfg = resolve_audio(c.audio)
    bs = int(c["test_config"]["batch_size"]) if "test_config" in c else 1
    for emb, target_wavs, mixed_wav in group_speaker_items(speaker_items(rows, root, int(acfg["sample_rate"])), bs):
        mixed, phase = audio.wav_to_spec(mixed_wav.to(device), acfg, want_phase=True)
        yield emb.to(device), mixed, phase, target_wavs


def _speakers_main(args, c, tr: Trainer, dev):
    rows = read_speakers_csv(args.speakers_csv)

    def score(path):
        tr.load_checkpoint(path)
        if args.stoi:
            return tr.evaluate_speakers(speaker_batches(c, rows, args.dataset_dir, dev), stoi=True)
        return tr.evaluate_speakers(speaker_batches(c, rows, args.dataset_dir, dev))

    def line(m):
        text = (f"Mean Test SDR: {m['sdr']} Mean Test SIR: {m['sir']} Mean Test SAR: {m['sar']} "
                f"Speaker confusion: {m['confusion']}")
        return text + (f" Mean Test STOI: {m['stoi']} Mean Test ESTOI: {m['estoi']}" if args.stoi else "")

    if args.checkpoint_path:
        m = score(args.checkpoint_path)
        for name, key in (("Mean Test SDR", "sdr"), ("Mean Test SIR", "sir"), ("Mean Test SAR", "sar"), ("Speaker confusion", "confusion")):
            print(f"{name}:", m[key])
        if args.stoi:
            print("Mean Test STOI:", m["stoi"])
            print("Mean Test ESTOI:", m["estoi"])
        return m
    paths = [p for p in sorted(glob(os.path.join(args.checkpoints_path, "*.pt"))) if os.path.basename(p) != "best_checkpoint.pt"]
    if not paths:
        raise FileNotFoundError(f"no *.pt checkpoints in {args.checkpoints_path}")
    table = []
    for p in paths:
        m = score(p)
        print(f"{p}: {line(m)}", flush=True)
        table.append({"checkpoint": p, **m})
    scored = [t for t in table if t["sdr"] == t["sdr"]]
    if not scored:
        raise RuntimeError("no checkpoint has a mean SDR: every test item was skipped")
    best = max(scored, key=lambda t: t["sdr"])
    print("Best SDR checkpoint is: ", best["checkpoint"], line(best))
    out = args.json or os.path.join(args.checkpoints_path, "speakers_per_checkpoint.json")
    with open(out, "w") as f:
        json.dump({"checkpoints": table, "best_sdr": best}, f, indent=1)
    return table


def build_trainer(c, device) -> Trainer:
    from . import VoiceFilter, VoiceSplit
    if c.model_name == "voicefilter":
        model = VoiceFilter(c)
    elif c.model_name == "voicesplit":
        model = VoiceSplit(c)
    else:
        raise Exception(" The model '" + c.model_name + "' is not suported")
    return Trainer(model.to(device), c)


def score_checkpoint(tr: Trainer, path: str, ds: EvalDataset, device, ragged: bool = False):
    """(mean_loss, mean_sdr) of one checkpoint (test.py:test + validation(test=True))."""
    tr.load_checkpoint(path)
    if ragged:
        return tr.evaluate_ragged(eval_batches(tr.c, ds, device, ragged=True))
    return tr.evaluate(eval_batches(tr.c, ds, device))


def score_intelligibility(tr: Trainer, ds: EvalDataset, device, ragged: bool = False):
    """``Trainer.evaluate_intelligibility`` of the checkpoint ``tr`` holds, over the batches ``score_checkpoint`` scores."""
    return tr.evaluate_intelligibility(eval_batches(tr.c, ds, device, ragged=ragged), ragged=ragged)


def main(argv=None):
    from . import load_config
    ap = argparse.ArgumentParser(description="Mean test loss and SDR of VoiceSplit checkpoints (test.py / test_all_checkpoints.py)")
    ap.add_argument("-c", "--config_path", required=True, help="json file with configurations")
    ap.add_argument("-d", "--dataset_dir", default="./", help="directory of the test items")
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--checkpoint_path", help="one checkpoint (test.py)")
    which.add_argument("--checkpoints_path", help="a directory of checkpoints (test_all_checkpoints.py)")
    ap.add_argument("--json", default=None, help="--checkpoints_path: where the per-checkpoint table goes")
    ap.add_argument("--ragged", action="store_true",
                    help="test items may differ in length: ragged batches, loss and SDR per item at its own length")
    ap.add_argument("--speakers-csv", default=None,
                    help="several enrolled speakers per mixture: rows mixed_wav,emb_1,target_wav_1,...,emb_K,target_wav_K "
                         "relative to -d; prints mean SDR / SIR / SAR and the speaker confusion")
    ap.add_argument("--stoi", action="store_true",
                    help="also print the mean STOI and ESTOI (intelligibility at 10 kHz) and add them to the --json table")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("voicesplit_amd.evaluate needs a GPU: the evaluation path has no CPU implementation")
    c = load_config(args.config_path)
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.speakers_csv:                                   # the CSV names the files: no c.dataset globs
        if args.ragged:
            raise ValueError("--speakers-csv scores batches of one length: group the rows by length instead of --ragged")
        return _speakers_main(args, c, build_trainer(c, dev), dev)
    c.dataset["test_dir"] = args.dataset_dir
    ds = EvalDataset(c, args.dataset_dir)
    tr = build_trainer(c, dev)
    if args.checkpoint_path:
        mean_loss, mean_sdr = score_checkpoint(tr, args.checkpoint_path, ds, dev, ragged=args.ragged)
        print("Mean Test Loss:", mean_loss)
        print("Mean Test SDR:", mean_sdr)
        if args.stoi:
            m = score_intelligibility(tr, ds, dev, ragged=args.ragged)
            print("Mean Test STOI:", m["stoi"])
            print("Mean Test ESTOI:", m["estoi"])
            return mean_loss, mean_sdr, m["stoi"], m["estoi"]
        return mean_loss, mean_sdr
    paths = [p for p in sorted(glob(os.path.join(args.checkpoints_path, "*.pt"))) if os.path.basename(p) != "best_checkpoint.pt"]
    if not paths:
        raise FileNotFoundError(f"no *.pt checkpoints in {args.checkpoints_path}")
    table = []
    for p in paths:
        mean_loss, mean_sdr = score_checkpoint(tr, p, ds, dev, ragged=args.ragged)
        row = {"checkpoint": p, "mean_sdr": mean_sdr, "mean_loss": mean_loss}
        more = ""
        if args.stoi:
            m = score_intelligibility(tr, ds, dev, ragged=args.ragged)
            row.update(mean_stoi=m["stoi"], mean_estoi=m["estoi"])
            more = f" Mean Test STOI: {m['stoi']} Mean Test ESTOI: {m['estoi']}"
        print(f"{p}: Mean Test Loss: {mean_loss} Mean Test SDR: {mean_sdr}{more}", flush=True)
        table.append(row)
    scored = [t for t in table if t["mean_sdr"] == t["mean_sdr"]]          # NaN: no item of the set could be scored
    if not scored:
        raise RuntimeError("no checkpoint has a mean SDR: every test item was skipped")
    best_sdr = max(scored, key=lambda t: t["mean_sdr"])
    best_loss = min(table, key=lambda t: t["mean_loss"])
    print("Best SDR checkpoint is: ", best_sdr["checkpoint"], "Best Loss checkpoint is: ", best_loss["checkpoint"],
          "Best SDR:", best_sdr["mean_sdr"], "Best Loss:", best_loss["mean_loss"])
    shutil.copyfile(best_sdr["checkpoint"], os.path.join(args.checkpoints_path, "best_checkpoint.pt"))
    out = args.json or os.path.join(args.checkpoints_path, "sdr_loss_per_checkpoint.json")
    with open(out, "w") as f:
        json.dump({"checkpoints": table, "best_sdr": best_sdr, "best_loss": best_loss}, f, indent=1)
    return table


if __name__ == "__main__":
    main()
