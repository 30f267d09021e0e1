"""GPU: csrc/fir_fft.hip (vs_fir_spectra, vs_fir_rows_fft) against the restatements of tests/fir_fft_ref.py -- the error bound of
include/voicesplit_hip.h at kappa = 8 kappa_ref, the cross-check with the direct form, what the bits of a row depend on, invalid and
silent rows, the caller's stream, a whole MixtureBatches batch with math="fft", and the pool's kept spectra.  One flat buffer of 20000
samples and a table of five responses; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import fir_fft_ref as FR
import reverb_ref as RR
from stream_helpers import probe

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BK = FR.BK


def _dev(v, dt):
    return torch.tensor(v, dtype=dt, device=DEV)


@pytest.fixture(scope="module")
def case():
    from voicesplit_amd import reverb
    flat, h, long_h = FR.data()
    d = dict(flat=flat, h=h, long_h=long_h, flat_dev=torch.from_numpy(flat).to(DEV), h_dev=torch.from_numpy(h).to(DEV),
             long_dev=torch.from_numpy(long_h).to(DEV), kappa=FR.KAPPA_MARGIN * FR.kappa_ref(), worst=[0.0])
    d["spectra"] = reverb.fir_spectra(d["h_dev"], list(FR.FILTERS))
    print(f"kappa_ref = {FR.kappa_ref():.5f}; the kernel is held to kappa = {d['kappa']:.5f}")
    return d


def _run(case, at, lo, hrow, L, spectra=None, flat_dev=None, **kw):
    from voicesplit_amd import reverb
    return reverb.fir_rows_fft(case["flat_dev"] if flat_dev is None else flat_dev, _dev(at, torch.int64), _dev(lo, torch.int64),
                               _dev(hrow, torch.int32), case["spectra"] if spectra is None else spectra, L, **kw)


def _judge(case, label, y, rows):
    y = y.cpu().numpy()
    for b, c in enumerate(rows):
        frac = FR.ratio(y[b], c["y64"], c["E"], c["L"], BK) / case["kappa"]
        ref = FR.ratio(c["y32"], c["y64"], c["E"], c["L"], BK)
        case["worst"][0] = max(case["worst"][0], frac)
        print(f"{label} at {c['at']} lo {c['lo']}: max |y| {np.abs(c['y64']).max():.3e}, max err {np.abs(y[b] - c['y64']).max():.3e}, "
              f"kernel {frac * case['kappa']:.5f}, pocketfft {ref:.5f}, fraction of the bound {frac:.3f} "
              f"(worst so far {case['worst'][0]:.3f})")
        assert np.all(np.abs(y[b].astype(np.float64) - c["y64"]) <= FR.bound(c["E"], c["L"], BK, case["kappa"])), (label, b)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", FR.LENGTHS)
@pytest.mark.parametrize("r", range(len(FR.FILTERS)))
def test_every_output_is_within_the_bound(case, r, L):
    """|y - y64| <= 8 kappa_ref 2^-24 log2(N) E_j for nh in {1, Bk - 1, Bk, Bk + 1, 3 Bk + 5} and L in {Bk / 2 + 3, 2 Bk + 17}: an
    odd start with history, no history, the end of the buffer."""
    rows = FR.cases()[(r, L)]
    y, valid = _run(case, [c["at"] for c in rows], [c["lo"] for c in rows], [r] * 3, L)
    assert valid.tolist() == [1, 1, 1] and y.shape == (3, L) and y.dtype == torch.float32
    _judge(case, f"nh {FR.FILTERS[r]} L {L}", y, rows)


def test_long_response(case):
    """nh = 32768 (P = 16), L = Bk + 5: the row ends with the buffer and its history starts at sample 0, so windows wholly below lo
    are skipped beside windows that are not."""
    from voicesplit_amd import reverb
    rows = FR.cases()[("long", FR.LONG_L)]
    sp = reverb.fir_spectra(case["long_dev"], [FR.LONG_NH])
    y, valid = _run(case, [rows[0]["at"]], [rows[0]["lo"]], [0], FR.LONG_L, spectra=sp)
    assert valid.tolist() == [1]
    _judge(case, f"nh {FR.LONG_NH} L {FR.LONG_L}", y, rows)


@pytest.mark.parametrize("L", FR.LENGTHS)
def test_the_direct_form_agrees_within_the_sum_of_both_bounds(case, L):
    """The same rows through vs_fir_rows f16x3: two independent kernels, |y_fft - y_f16x3| <= bound_fft + bound_f16x3."""
    from voicesplit_amd import reverb
    worst = 0.0
    for r, nh in enumerate(FR.FILTERS):
        rows = FR.cases()[(r, L)]
        at, lo = [c["at"] for c in rows], [c["lo"] for c in rows]
        y, _ = _run(case, at, lo, [r] * 3, L)
        d, valid, _ = reverb.fir_rows(case["flat_dev"], _dev(at, torch.int64), _dev(lo, torch.int64), _dev([nh] * 3, torch.int32),
                                      _dev([r] * 3, torch.int32), case["h_dev"], L, "f16x3")
        assert valid.tolist() == [1, 1, 1]
        diff = (y.double() - d.double()).abs().cpu().numpy()
        for b, c in enumerate(rows):
            both = FR.bound(c["E"], L, BK, case["kappa"]) + RR.fir_bound(c["mag"], nh, c["mx"], c["mh"], "f16x3")[0]
            worst = max(worst, float((diff[b] / both).max()))
            assert np.all(diff[b] <= both), (r, b)
    print(f"L {L}: worst |y_fft - y_f16x3| as a fraction of the sum of both bounds {worst:.3f}")


# ---- bits --------------------------------------------------------------------------------------------------------------------------------
L_BITS = BK + 77
BATCH = dict(at=[7001, 9403, 20000 - L_BITS, 5000, 12345], lo=[13, 9403, 20000 - L_BITS - 100, 2953, 12000], hrow=[4, 1, 3, 0, 2])


@pytest.fixture(scope="module")
def batch_bits(case):
    y, valid = _run(case, BATCH["at"], BATCH["lo"], BATCH["hrow"], L_BITS)
    assert valid.tolist() == [1] * 5 and torch.isfinite(y).all() and float(y.abs().max()) > 0.01
    return y.clone()


def test_bits_repeat_and_do_not_depend_on_the_batch(case, batch_bits):
    y, _ = _run(case, BATCH["at"], BATCH["lo"], BATCH["hrow"], L_BITS)
    assert torch.equal(y, batch_bits)                                                # the call
    for b in range(5):                                                               # B and the row's index
        alone, _ = _run(case, BATCH["at"][b:b + 1], BATCH["lo"][b:b + 1], BATCH["hrow"][b:b + 1], L_BITS)
        assert torch.equal(alone[0], batch_bits[b]), b
    back, _ = _run(case, BATCH["at"][::-1], BATCH["lo"][::-1], BATCH["hrow"][::-1], L_BITS)
    assert torch.equal(back.flip(0), batch_bits)


def test_bits_do_not_depend_on_the_table(case, batch_bits):
    """A permuted table with hrow permuted to match; a response alone in a table of its own width (another R, H and partition
    count of the table)."""
    from voicesplit_amd import reverb
    perm = [3, 0, 4, 2, 1]                                                           # new row k holds old response perm[k]
    sp = reverb.fir_spectra(case["h_dev"][perm].contiguous(), [FR.FILTERS[k] for k in perm])
    y, _ = _run(case, BATCH["at"], BATCH["lo"], [perm.index(r) for r in BATCH["hrow"]], L_BITS, spectra=sp)
    assert torch.equal(y, batch_bits)
    for b, r in enumerate(BATCH["hrow"]):
        nh = FR.FILTERS[r]
        own = reverb.fir_spectra(case["h_dev"][r:r + 1, :nh].contiguous(), [nh])
        y, _ = _run(case, BATCH["at"][b:b + 1], BATCH["lo"][b:b + 1], [0], L_BITS, spectra=own)
        assert torch.equal(y[0], batch_bits[b]), b


def test_bits_do_not_depend_on_the_alignment_of_the_buffer(case, batch_bits):
    for shift in (1, 3):
        moved = torch.cat((torch.full((shift,), float("nan"), device=DEV), case["flat_dev"]))
        y, valid = _run(case, [a + shift for a in BATCH["at"]], [l + shift for l in BATCH["lo"]], BATCH["hrow"], L_BITS, flat_dev=moved)
        assert valid.tolist() == [1] * 5 and torch.equal(y, batch_bits), shift


def test_bits_do_not_depend_on_what_the_workspace_held(case, batch_bits):
    from voicesplit_amd import _call
    need = _call.sized("fir_fft_workspace_bytes", 5, L_BITS, case["spectra"].H)
    for fill in (0xFF, 0x00):
        ws = torch.full((need + 64,), fill, dtype=torch.uint8, device=DEV)
        y, _ = _run(case, BATCH["at"], BATCH["lo"], BATCH["hrow"], L_BITS, workspace=ws)
        assert torch.equal(y, batch_bits), fill
    with pytest.raises(ValueError, match="workspace"):
        _run(case, BATCH["at"], BATCH["lo"], BATCH["hrow"], L_BITS, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


def test_nan_outside_what_a_row_reads_changes_nothing(case, batch_bits):
    """NaN in h behind nh; NaN in the samples below lo and at or behind at + L (row by row: the rows of the batch overlap)."""
    from voicesplit_amd import reverb
    h = case["h_dev"].clone()
    for r, nh in enumerate(FR.FILTERS):
        h[r, nh:] = float("nan")
    y, _ = _run(case, BATCH["at"], BATCH["lo"], BATCH["hrow"], L_BITS, spectra=reverb.fir_spectra(h, list(FR.FILTERS)))
    assert torch.equal(y, batch_bits)
    for b in range(5):
        at, lo = BATCH["at"][b], BATCH["lo"][b]
        flat = case["flat_dev"].clone()
        flat[:lo] = float("nan")
        flat[at + L_BITS:] = float("nan")
        y, valid = _run(case, [at], [lo], BATCH["hrow"][b:b + 1], L_BITS, flat_dev=flat)
        assert valid.tolist() == [1] and torch.equal(y[0], batch_bits[b]), b


# ---- invalid and silent rows ---------------------------------------------------------------------------------------------------------------
def test_invalid_rows_give_zeros_and_leave_their_neighbours_alone(case, batch_bits):
    total, L = FR.TOTAL, L_BITS
    at = [BATCH["at"][0], 3000, 3000, total - L + 1, BATCH["at"][1], 3000, 3000, BATCH["at"][4]]
    lo = [BATCH["lo"][0], -1, 3001, 3000, BATCH["lo"][1], 3000, 3000, BATCH["lo"][4]]
    hrow = [BATCH["hrow"][0], 0, 0, 0, BATCH["hrow"][1], 5, -1, BATCH["hrow"][4]]
    out = torch.full((8, L), float("nan"), device=DEV)
    y, valid = _run(case, at, lo, hrow, L, out=out)
    assert y is out and valid.tolist() == [1, -1, -1, -1, 1, -1, -1, 1]
    assert not y[[1, 2, 3, 5, 6]].any()
    for k, b in ((0, 0), (4, 1), (7, 4)):
        assert torch.equal(y[k], batch_bits[b]), k


def test_a_silent_row_gives_exact_zeros(case):
    flat = case["flat_dev"].clone()
    at, lo = 9001, 2000
    flat[lo:at + L_BITS] = 0.0
    y, valid = _run(case, [at, BATCH["at"][4]], [lo, BATCH["lo"][4]], [4, 4], L_BITS, flat_dev=flat)
    assert valid.tolist() == [1, 1] and bool((y[0] == 0).all()) and float(y[1].abs().max()) > 0.01


# ---- the caller's stream -------------------------------------------------------------------------------------------------------------------
def test_spectra_and_rows_run_on_the_callers_stream(case):
    """Both calls under a stream that is still busy with a delay, their float inputs NaN until a copy behind the delay brings them
    (tests/stream_helpers.py): bit equality with the null-stream run.  The tap counts are given on both sides, so nothing is
    uploaded and the host does not block."""
    from voicesplit_amd import reverb
    flat, h = case["flat_dev"].clone(), case["h_dev"].clone()
    nh_host = torch.tensor(FR.FILTERS, dtype=torch.int32)
    nh_dev = nh_host.to(DEV)
    at, lo, hrow = _dev(BATCH["at"], torch.int64), _dev(BATCH["lo"], torch.int64), _dev(BATCH["hrow"], torch.int32)
    torch.cuda.synchronize()
    want = probe("fir_spectra + fir_rows_fft", lambda: reverb.fir_rows_fft(flat, at, lo, hrow, reverb.fir_spectra(h, nh_host, nh_dev), L_BITS),
                 [flat, h])
    sp = reverb.fir_spectra(h, nh_host, nh_dev)
    torch.cuda.synchronize()
    probe("fir_rows_fft with kept spectra", lambda: reverb.fir_rows_fft(flat, at, lo, hrow, sp, L_BITS), [flat])
    assert torch.equal(want[0][1], _run(case, BATCH["at"], BATCH["lo"], BATCH["hrow"], L_BITS)[0])


# ---- batches -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mix_case():
    """The small geometry of tests/test_gpu_reverb.py: seven clips, batches of three, 160 samples a crop; six measured responses of
    up to 2300 taps (two partitions), their peaks planted."""
    import voicesplit_amd as V
    from voicesplit_amd import mixing, reverb
    from voicesplit_amd.trainer import EpochShard
    dims = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
    c = V.default_config(**dims)
    c.audio["voicefilter"].update({"hop_length": 16, "win_length": 40})
    acfg = c.audio["voicefilter"]
    rng = np.random.default_rng(3)
    clips = []
    for k in range(7):
        m = 1500 + 211 * k
        y = (1e-4 * rng.standard_normal(m)).astype(np.float32)
        y[200 + 37 * k:m - 150] += (0.2 * rng.standard_normal(m - 350 - 37 * k)).astype(np.float32)
        clips.append(torch.from_numpy(y))
    pool = mixing.ClipPool(clips, DEV)
    L, B = acfg["hop_length"] * 10, 3
    triplets = [(a, (a + 1) % 7, (a + 3) % 7) for a in range(7)] + [(a, a, (a + 2) % 7) for a in range(7)]
    kept, dropped = mixing.plan_triplets(pool, triplets, L)
    assert dropped == 0
    table = torch.randn(len(pool), dims["emb_dim"], generator=torch.Generator().manual_seed(2)).to(DEV)
    nh = [2300, 2100, 2049, 171, 900, 2048]
    h = np.zeros((6, 2300), dtype=np.float32)
    for r, n in enumerate(nh):
        h[r, :n] = (0.05 * rng.standard_normal(n) * np.exp(-np.arange(n) / 400.0)).astype(np.float32)
        h[r, 20 + 7 * r] = 1.0
    rirs = reverb.RirPool.from_responses(torch.from_numpy(h), nh, 16000, DEV)
    return dict(pool=pool, kept=kept, table=table, acfg=acfg, audio_len=L / acfg["sample_rate"], shard=EpochShard(len(kept), B, seed=4),
                L=L, B=B, rirs=rirs, h=h, nh=nh)


def _batches(mc, **kw):
    from voicesplit_amd import mixing
    return mixing.MixtureBatches(mc["pool"], mc["kept"], mc["table"], mc["acfg"], mc["audio_len"], mc["shard"], rir_pool=mc["rirs"],
                                 crop="random", seed=5, **kw)


def test_fft_batches_equal_the_restatement(case, mix_case):
    """Every wav of the batches against reverb_ref.batch with the FFT form's bound (kappa 2^-24 log2(N) E_j) carried through the gain,
    the sum, the maximum and the division."""
    from voicesplit_amd import reverb
    mc = mix_case
    assert mc["rirs"].nh_early_host.tolist() == [min(n, 21 + 7 * r + 800) for r, n in enumerate(mc["nh"])]
    sir_db = (2.0, 9.0)
    mb = _batches(mc, sir_db=sir_db, math="fft")
    order = list(mc["shard"].epoch(0))
    pos, at, _ = mb.plan(order, 0)
    room, sir = reverb.item_draws(5, 0, 0, pos.numel(), 3, sir_db)
    assert len(set(room.tolist())) > 1
    hrow = torch.stack((2 * room, 2 * room + 1))
    nh = mc["rirs"].nh_host[hrow]
    lo = mb.start[pos].t()
    flat, L, B = mc["pool"].flat.cpu().numpy(), mc["L"], mc["B"]
    worst = {"mixed": 0.0, "target": 0.0, "norm": 0.0}
    for k, it in enumerate(mb.items(order, 0)):
        s = slice(k * B, (k + 1) * B)
        ref = FR.batch(flat, at[:, s].tolist(), lo[:, s].tolist(), hrow[:, s].tolist(), nh[:, s].tolist(), mc["h"], L, sir[s].tolist(),
                       case["kappa"])
        assert it["valid"].tolist() == [1] * B
        for b, r in enumerate(ref):
            for key, got in (("mixed", it["mixed_wav"][b]), ("target", it["target_wav"][b])):
                err = np.abs(got.cpu().numpy().astype(np.float64) - r[key])
                worst[key] = max(worst[key], float((err / r["err_" + key]).max()))
                assert np.all(err <= r["err_" + key]), (k, b, key, float(err.max()))
            worst["norm"] = max(worst["norm"], abs(float(it["norm"][b]) - r["norm"]) / r["err_norm"])
            assert abs(float(it["norm"][b]) - r["norm"]) <= r["err_norm"]
    print(f"math fft, sir {sir_db}: worst fraction of the carried bound {worst}")
    assert mb.invalid_items == 0


def test_the_default_batches_do_not_change_and_early_targets_stay_on_the_direct_form(mix_case):
    """Without math the batches are those of math="f16x3" bit for bit; with math="fft" and target="early" the target rows, which stay
    on the f16x3 direct form, times the norm are the f16x3 batch's target rows times its norm within three fp32 roundings."""
    mc = mix_case
    order = list(mc["shard"].epoch(0))[:2]
    plain = list(_batches(mc, target="early").items(order, 0))
    named = list(_batches(mc, target="early", math="f16x3").items(order, 0))
    fft = list(_batches(mc, target="early", math="fft").items(order, 0))
    for a, b, f in zip(plain, named, fft):
        for k in ("mixed_wav", "target_wav", "norm", "mixed", "target", "phase"):
            assert torch.equal(a[k], b[k]), k
        ta, tf = a["target_wav"].double() * a["norm"].double()[:, None], f["target_wav"].double() * f["norm"].double()[:, None]
        assert float(ta.abs().max()) > 0.01 and bool(((ta - tf).abs() <= 3 * 2.0 ** -24 * ta.abs()).all())
        assert not torch.equal(a["mixed_wav"], f["mixed_wav"]) and float((a["mixed_wav"] - f["mixed_wav"]).abs().max()) < 1e-4


# ---- the pool's spectra --------------------------------------------------------------------------------------------------------------------
def test_the_pools_spectra_are_made_once_and_again_after_redraw(mix_case, monkeypatch):
    from voicesplit_amd import reverb
    made = []
    real = reverb.fir_spectra
    monkeypatch.setattr(reverb, "fir_spectra", lambda *a, **k: made.append(1) or real(*a, **k))
    pool = reverb.RirPool(2, DEV, seed=3, nh=256)
    assert made == []                                                                # lazily
    sp = pool.spectra
    assert pool.spectra is sp and made == [1] and (sp.R, sp.H) == (4, 256) and sp.nh_host.tolist() == [256] * 4
    fresh = pool.redraw(1)
    assert fresh is not pool and made == [1]
    assert fresh.spectra is not sp and fresh.spectra is fresh.spectra and made == [1, 1] and pool.spectra is sp
    # the pool's spectra are those of its table: the kept ones and ones made on the fly give the same rows
    wav = torch.from_numpy(FR.data()[0][:4 * 3000].reshape(4, 3000)).to(DEV)
    at = torch.arange(4, dtype=torch.int64, device=DEV) * 3000
    y, _ = reverb.fir_rows_fft(wav.reshape(-1), at, at, torch.arange(4, dtype=torch.int32, device=DEV), sp, 3000)
    assert torch.equal(y, reverb.apply(wav, pool.h, math="fft")) and made == [1, 1, 1]
    # a fixed pool returns itself from redraw and keeps its spectra; an epoch of batches makes them once
    rirs = mix_case["rirs"]
    rirs._spectra = None
    made.clear()
    assert rirs.redraw(3) is rirs
    mb = _batches(mix_case, math="fft")
    assert len(list(mb.items(list(mix_case["shard"].epoch(0)), 0))) > 1 and made == [1] and mb.rir_pool is rirs


# ---- measured responses from files ---------------------------------------------------------------------------------------------------------
def test_from_files_reads_pairs_resamples_and_serves_long_pools(tmp_path):
    """Two rooms from four wav files, one of them at half the rate (converted on the device); the table is as wide as the longest
    response, 9000 taps -- more than the direct form takes --, every response keeps its own length, and the early table is a cut copy."""
    from scipy.io import wavfile
    from voicesplit_amd import _lib, audio, reverb
    from voicesplit_amd.trainer import load_wav
    rng = np.random.default_rng(8)
    lengths, rates = [9000, 2500, 700, 3000], [16000, 16000, 8000, 16000]
    paths = []
    for k, (n, sr) in enumerate(zip(lengths, rates)):
        w = 0.02 * rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 5.0))
        w[30 + k] = 0.9
        paths.append(str(tmp_path / f"rir{k}.wav"))
        wavfile.write(paths[-1], sr, np.round(w * 32767).astype(np.int16))
    pairs = [(paths[0], paths[1]), (paths[2], paths[3])]
    pool = reverb.RirPool.from_files(pairs, 16000, DEV)
    low = audio.resample(load_wav(paths[2], 8000).to(DEV), 8000, 16000)
    want = [load_wav(paths[0], 16000).to(DEV), load_wav(paths[1], 16000).to(DEV), low, load_wav(paths[3], 16000).to(DEV)]
    assert len(pool) == 2 and pool.h.shape == (4, 9000) and pool.nh_host.tolist() == [9000, 2500, low.numel(), 3000] and low.numel() == 1400
    for r, w in enumerate(want):
        assert torch.equal(pool.h[r, :w.numel()], w) and not pool.h[r, w.numel():].any()
    assert pool.nh_early_host[[0, 1, 3]].tolist() == [831, 832, 834] and pool.redraw(5) is pool
    assert pool.h_early.shape == (4, int(pool.nh_early_host.max())) and torch.equal(pool.h_early, pool.h[:, :pool.h_early.shape[1]])
    with pytest.raises(ValueError, match="sample rate 8000"):
        reverb.RirPool.from_files(pairs, 16000, DEV, resample=False)
    # the long pool serves the FFT form, and the direct form refuses its 9000 taps by name
    x = torch.from_numpy(FR.data()[0][:12000].reshape(4, 3000)).to(DEV)
    y = reverb.apply(x, pool.h, nh=pool.nh_host, math="fft")
    h0 = pool.h[0].cpu().numpy()
    ref, E = FR.fir64(FR.data()[0], 0, 0, 3000, h0, 9000), FR.block_energy(FR.data()[0], 0, 0, 3000, h0, 9000)
    assert np.all(np.abs(y[0].cpu().numpy() - ref) <= FR.bound(E, 3000, BK, FR.KAPPA_MARGIN * FR.kappa_ref())) and np.abs(ref).max() > 0.05
    with pytest.raises(_lib.VoiceSplitHipError, match="H=9000"):
        reverb.apply(x, pool.h)
