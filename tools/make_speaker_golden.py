#!/usr/bin/env python3
"""Writes tests/golden/speaker_small.npz: a reduced-size GE2E speaker encoder evaluated by the REFERENCE notebook's own class
(CPU, fp64).  The notebook cannot be imported (it moves its model to a GPU and walks a dataset at import), so this reads its
text, takes the LinearNorm and SpeakerEncoder class definitions out of it with `ast` and executes only those; none of that
text is stored here or in the fixture.

    python tools/make_speaker_golden.py /path/to/reference

Fixture: mels 8, hidden 24, 3 layers, emb 16, window 10, stride 5; T in {10, 23, 57}; LSTM weights of torch's default init
scaled x3 (gates leave their linear range); log-mel-like inputs in [-6, 2]."""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTEBOOK = "notebooks/GE2E-Seungwonpark-ExtractSpeakerEmbedding-adaptado-para-openvoicefilter.py"
DIMS = dict(num_mels=8, lstm_layers=3, lstm_hidden=24, emb_dim=16, window=10, stride=5)
FRAMES = (10, 23, 57)


def reference_classes(ref_root, emb_dim):
    tree = ast.parse(open(os.path.join(ref_root, NOTEBOOK)).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("LinearNorm", "SpeakerEncoder")]
    assert [n.name for n in keep] == ["LinearNorm", "SpeakerEncoder"]
    ns = {"torch": torch, "nn": torch.nn, "emb_dim": emb_dim}
    exec(compile(ast.Module(body=keep, type_ignores=[]), NOTEBOOK, "exec"), ns)
    return ns["SpeakerEncoder"]


def main():
    ref_root = sys.argv[1]
    cls = reference_classes(ref_root, DIMS["emb_dim"])
    torch.manual_seed(20)
    m = cls(DIMS["num_mels"], DIMS["lstm_layers"], DIMS["lstm_hidden"], DIMS["window"], DIMS["stride"]).double().eval()
    with torch.no_grad():
        for k, p in m.lstm.named_parameters():
            if k.startswith("weight"):
                p.mul_(3.0)
    out = {f"sd.{k}": v.numpy().astype(np.float32) for k, v in m.state_dict().items()}
    # the fp64 run uses the fp32-rounded weights, which is what the module under test is given
    m.load_state_dict({k[3:]: torch.from_numpy(v).double() for k, v in out.items()})
    g = torch.Generator().manual_seed(21)
    for T in FRAMES:
        mel = (torch.rand(DIMS["num_mels"], T, generator=g) * 8.0 - 6.0).float()
        with torch.no_grad():
            x = mel.double()
            dvec = m(x)
            # the per-window stages of the same forward (notebook :78-82), through the reference module's own members
            h, _ = m.lstm(x.unfold(1, DIMS["window"], DIMS["stride"]).permute(1, 2, 0))
            h_last = h[:, -1, :]
            proj = m.proj(h_last)
            again = (proj / torch.norm(proj, p=2, dim=1, keepdim=True)).sum(0) / proj.size(0)
            assert torch.equal(again, dvec)
        out[f"mel.{T}"] = mel.numpy()
        out[f"h_last.{T}"] = h_last.numpy()
        out[f"proj.{T}"] = proj.numpy()
        out[f"dvec.{T}"] = dvec.numpy()
    out["dims"] = np.array([DIMS[k] for k in ("num_mels", "lstm_layers", "lstm_hidden", "emb_dim", "window", "stride")], dtype=np.int64)
    out["frames"] = np.array(FRAMES, dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "speaker_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
