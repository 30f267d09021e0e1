"""CPU: the fp64 multi-source BSS-eval restatement (tests/bss_eval_multi_ref.py) against the single-source one and, when it is
installed, against mir_eval itself; the permutation tie rule; argument checks of vs_bss_eval and of metrics.bss_eval that
run without a GPU; the speakers-CSV reader and batch grouping of voicesplit_amd.evaluate."""
import ctypes

import numpy as np
import pytest
import torch

import bss_eval_multi_ref as M
import bss_eval_ref as R


def test_restatement_at_one_source_is_the_single_source_one():
    ref, est = M.make_item(1, 3000)
    sdr, sir, sar, perm, pairs = M.bss_eval_item(ref, est)
    want = R.sdr(ref[0], est[0])
    assert sdr[0] == want and sar[0] == want and np.isinf(sir[0]) and sir[0] > 0 and perm.tolist() == [0]
    assert pairs.shape == (3, 1, 1) and pairs[0, 0, 0] == want


def test_restatement_recipe_and_conventions():
    ref, est = M.make_item(3, 3000)
    assert ref.dtype == est.dtype == np.float32 and ref.shape == est.shape == (3, 3000)
    assert np.allclose(np.sqrt(np.mean(ref.astype(np.float64) ** 2, axis=1)), 0.05, rtol=1e-6)
    sdr, sir, sar, perm, pairs = M.bss_eval_item(ref, est)
    assert perm.tolist() == [1, 2, 0]                                          # the estimates are rolled by one
    assert np.array_equal(sdr, pairs[0][perm, np.arange(3)]) and np.array_equal(sir, pairs[1][perm, np.arange(3)])
    assert sir.sum() > pairs[1][np.arange(3), np.arange(3)].sum()             # output k holds speaker k - 1, not k
    d = M.bss_eval_item(ref, est, compute_permutation=False)
    assert d[3].tolist() == [0, 1, 2]
    assert np.array_equal(np.diagonal(d[4], axis1=1, axis2=2), np.diagonal(pairs, axis1=1, axis2=2))
    assert np.isnan(d[4][:, 0, 1]).all()
    # a silent row of an item: status 1, NaN, perm -1; the other item is scored
    r2, e2 = np.stack([ref, ref]), np.stack([est, est])
    r2[1, 2] = 0.0
    out = M.bss_eval_batch(r2, e2)
    assert out[4].tolist() == [0, 1] and np.isnan(out[0][1]).all() and out[3][1].tolist() == [-1, -1, -1]
    assert np.array_equal(out[0][0], sdr)


def test_restatement_matches_mir_eval_when_installed():
    sep = pytest.importorskip("mir_eval.separation")
    for K, N in ((2, 6001), (3, 6001)):
        ref, est = M.make_item(K, N)
        for cp in (True, False):
            want = sep.bss_eval_sources(ref.astype(np.float64), est.astype(np.float64), cp)
            got = M.bss_eval_item(ref, est, cp)
            for g, w in zip(got[:3], want[:3]):
                assert np.abs(g - w).max() <= 1e-6, (K, cp, g, w)
            assert got[3].tolist() == list(want[3])


def test_permutation_tie_rule():
    # (0, 1, 2) and (1, 0, 2) both sum to 12: the first in itertools.permutations order wins, as np.argmax picks it
    sir = np.array([[5.0, 4.0, 0.0], [6.0, 5.0, 0.0], [0.0, 0.0, 2.0]])
    perm, sums = M.best_permutation(sir)
    assert sums[0] == sums[2] == 12.0 and sums.max() == 12.0
    assert perm.tolist() == [0, 1, 2]
    perm, _ = M.best_permutation(np.array([[1.0, 3.0], [3.0, 1.0]]))
    assert perm.tolist() == [1, 0]
    perm, _ = M.best_permutation(np.array([[2.0, 2.0], [2.0, 2.0]]))
    assert perm.tolist() == [0, 1]


def test_vs_bss_eval_argument_errors_without_a_gpu():
    from voicesplit_amd import _lib
    lib = _lib.load()
    assert lib.vs_abi_version() == 11
    wsb = lib.vs_bss_eval_workspace_bytes
    assert wsb(0, 2, 100) == 0 and wsb(4, 0, 100) == 0 and wsb(4, 7, 100) == 0 and wsb(4, 2, 0) == 0 and wsb(-1, 2, 100) == 0
    assert wsb(1, 1, 1) > 0 and wsb(2, 6, 1000) > wsb(2, 2, 1000) > wsb(2, 1, 1000)
    p = ctypes.c_void_p(256)                      # never dereferenced: every call below fails its argument checks first
    need = wsb(2, 3, 1000)

    def args(ref=p, est=p, B=2, K=3, N=1000, cp=1, sdr=p, sir=p, sar=p, perm=p, status=p, pairs=None, ws=p, nbytes=need):
        return (ref, est, B, K, N, cp, sdr, sir, sar, perm, status, pairs, ws, nbytes, None)

    cases = [(args(B=0), "B="), (args(K=0), "K="), (args(K=7), "K="), (args(N=0), "N="), (args(ref=None), "NULL"),
             (args(est=None), "NULL"), (args(sdr=None), "NULL"), (args(sir=None), "NULL"), (args(sar=None), "NULL"),
             (args(perm=None), "NULL"), (args(status=None), "NULL"), (args(ws=None), "NULL"),
             (args(nbytes=need - 1), "workspace too small"), (args(ws=ctypes.c_void_p(264)), "misaligned")]
    for a, msg in cases:
        assert lib.vs_bss_eval(*a) == -1, a
        assert msg in lib.vs_last_error().decode(), (a, lib.vs_last_error())


def test_bss_eval_rejects_bad_dtype_and_shape():
    from voicesplit_amd import metrics
    x = torch.zeros(2, 3, 100)
    with pytest.raises(TypeError):
        metrics.bss_eval(x.double(), x)
    with pytest.raises(TypeError):
        metrics.bss_eval(x, x.half())
    with pytest.raises(TypeError):
        metrics.bss_eval(x.numpy(), x)
    with pytest.raises(ValueError):
        metrics.bss_eval(x, torch.zeros(2, 3, 99))
    with pytest.raises(ValueError):
        metrics.bss_eval(x, torch.zeros(2, 2, 100))
    with pytest.raises(ValueError):
        metrics.bss_eval(torch.zeros(100), torch.zeros(100))
    with pytest.raises(ValueError):
        metrics.bss_eval(torch.zeros(1, 7, 100), torch.zeros(1, 7, 100))
    with pytest.raises(ValueError):
        metrics.bss_eval(torch.zeros(2, 0, 100), torch.zeros(2, 0, 100))
    with pytest.raises(ValueError):
        metrics.bss_eval(torch.zeros(2, 3, 0), torch.zeros(2, 3, 0))


def test_speakers_csv_reader_and_batch_grouping(tmp_path):
    from voicesplit_amd import evaluate
    f = tmp_path / "speakers.csv"
    f.write_text("# mixed, then (emb, target) per speaker\n"
                 "m0.wav, a0-emb.pt, a0.wav, b0-emb.pt, b0.wav\n\n"
                 "m1.wav,a1-emb.pt,a1.wav,b1-emb.pt,b1.wav\n")
    rows = evaluate.read_speakers_csv(str(f))
    assert rows == [("m0.wav", [("a0-emb.pt", "a0.wav"), ("b0-emb.pt", "b0.wav")]),
                    ("m1.wav", [("a1-emb.pt", "a1.wav"), ("b1-emb.pt", "b1.wav")])]
    f.write_text("m0.wav,a-emb.pt,a.wav,b-emb.pt,b.wav\nm1.wav,a-emb.pt,a.wav\n")
    with pytest.raises(ValueError, match="speakers"):
        evaluate.read_speakers_csv(str(f))
    f.write_text("m0.wav,a-emb.pt,a.wav,b-emb.pt\n")
    with pytest.raises(ValueError, match="fields"):
        evaluate.read_speakers_csv(str(f))
    f.write_text("\n")
    with pytest.raises(ValueError, match="no rows"):
        evaluate.read_speakers_csv(str(f))

    lengths = {"m0.wav": 800, "a0.wav": 800, "b0.wav": 800, "m1.wav": 800, "a1.wav": 800, "b1.wav": 640}
    load = lambda path, sr: torch.full((lengths[path.split("/")[-1]],), float(sr))
    load_emb = lambda path: torch.arange(4.0) + (1.0 if "b" in path.split("/")[-1] else 0.0)
    items = list(evaluate.speaker_items(rows, "root", 16000, load_emb=load_emb, load=load))
    assert items[0][0].shape == (2, 4) and items[0][0][1, 0] == 1.0 and len(items[0][1]) == 2 and items[0][2].shape == (800,)
    (emb, tw, mw), = list(evaluate.group_speaker_items(items[:1], 4))
    assert emb.shape == (1, 2, 4) and tw.shape == (1, 2, 800) and mw.shape == (1, 800)
    with pytest.raises(ValueError, match="items of one test batch must share a length"):
        list(evaluate.group_speaker_items(items, 4))
