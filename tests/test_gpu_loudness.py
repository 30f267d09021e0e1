"""GPU: programme loudness on the device (csrc/loudness.hip, voicesplit_amd/loudness.py) against the fp64 restatement of its contract
(tests/loudness_ref.py), its independence of position, neighbours, batch and call, the gain pass, ``normalize`` and the hooks built
on them (ClipPool(normalize=), audio.separate(loudness=)).

The tolerance on lufs is not measured on the device: it is max(64 d_ref, 1e-12 dB), d_ref being how far the restatement's own two
forms (serial filter, segmented evaluation) are apart on these very signals, and the tests first assert that it is below 1e-10 dB.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import loudness_ref as LR
import resample_ref as RR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
AUDIO = {"n_fft": 1200, "hop_length": 160, "win_length": 400, "min_level_db": -100.0, "ref_level_db": 20.0}
_METERS, _REF = {}, {}


def _meter(fs):
    from voicesplit_amd.loudness import LoudnessMeter
    if fs not in _METERS:
        _METERS[fs] = LoudnessMeter(fs, DEV)
    return _METERS[fs]


@pytest.fixture(scope="module")
def reference():
    """name -> (fs, x, serial result) for every signal of the length and gate tests, and tol = max(64 d_ref, 1e-12 dB); computed
    once and never modified."""
    if not _REF:
        d_ref = 0.0
        for name, fs, x in LR.gpu_test_signals():
            a = LR.serial(x, fs)
            _REF[name] = (fs, x, a)
            if a["valid"]:
                d_ref = max(d_ref, abs(a["lufs"] - LR.segmented(x, fs)["lufs"]))
        _REF["tol"] = max(64.0 * d_ref, 1e-12)
        print(f"d_ref = {d_ref:.3e} dB, tol = {_REF['tol']:.3e} dB")
    assert _REF["tol"] <= 1e-10, "the tolerance must not hide a failure"
    return _REF


def _lay(clips, fill=1e3):
    """The clips in one flat device buffer at ODD offsets, `fill` in front, between and behind them -> (flat, table [N, 2] host)."""
    at, pos = [], 1
    for k, c in enumerate(clips):
        pos += (pos + 1) % 2                                               # make it odd
        at.append(pos)
        pos += len(c) + 2 * k + 1
    flat = torch.full((pos + 8,), float(fill), dtype=torch.float32)
    for a, c in zip(at, clips):
        flat[a:a + len(c)] = torch.from_numpy(np.asarray(c, dtype=np.float32))
    table = torch.tensor([[a, len(c)] for a, c in zip(at, clips)], dtype=torch.int64)
    assert all(a % 2 == 1 for a in at)
    return flat.to(DEV), table


def _judge(tag, got, ref, tol, S, per_block=True):
    """one clip: (lufs, peak, counts, valid, energy) of the device against the serial restatement.  Energies within 1e-12 relative,
    per sub-block; per_block=False: relative to the clip's largest (a sub-block of digital silence behind a DC offset holds nothing
    but the rounding noise of the high-pass, 30 orders of magnitude down, in any evaluation)."""
    lufs, peak, counts, valid, energy = got
    print(f"  {tag}: lufs {lufs!r} (ref {ref['lufs']!r}), counts {counts} (ref {ref['counts']}), peak {peak!r}, valid {valid}")
    assert valid == ref["valid"] and tuple(counts) == tuple(ref["counts"]), tag
    assert peak == float(ref["peak"]), tag
    assert energy.shape == ref["energy"].shape, tag
    if len(energy):
        rel = np.abs(energy - ref["energy"]) / (ref["energy"] if per_block else ref["energy"].max())
        print(f"    energy: {len(energy)} sub-blocks, worst relative error {rel.max():.3e} (bound 1e-12, {'per sub-block' if per_block else 'of the largest'})")
        assert np.all(rel <= 1e-12), tag
    if ref["valid"]:
        print(f"    |lufs - ref| = {abs(lufs - ref['lufs']):.3e} dB (tol {tol:.3e})")
        assert abs(lufs - ref["lufs"]) <= tol, tag
    else:
        assert lufs == -np.inf, tag


def _run(fs, clips, fill=1e3):
    """-> per clip (lufs, peak, counts, valid, energy) on the host, and the raw device tensors"""
    flat, table = _lay(clips, fill)
    before = flat.clone()
    lufs, peak, counts, valid, energy = _meter(fs).clips(flat, table, energy=True)
    torch.cuda.synchronize()
    assert torch.equal(flat, before)                                       # the meter reads
    rows = [(float(lufs[i]), float(peak[i]), tuple(counts[i].tolist()), int(valid[i]), energy[i].cpu().numpy()) for i in range(len(clips))]
    return rows, (lufs, peak, counts, valid, energy)


# ---- lengths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,S", [(16000, 1600), (48000, 4800)])
def test_lengths(reference, fs, S):
    """n = 0, 1, 4 S - 1 (no block: -inf, valid 0), 4 S, 4 S + 1, 5 S - 1, 5 S, 64 S, 65 S + 7 and, at S = 1600, 257 S + 3: the ends of
    the block rule, one tile of 64 sub-blocks exactly, one more, and five tiles; clips at odd offsets between neighbours of 1e3."""
    assert _meter(fs).sub == S
    names = [k for k in reference if k.startswith("len") and k.endswith(f"@{fs}")]
    assert len(names) == (10 if S == 1600 else 9)
    rows, _ = _run(fs, [reference[k][1] for k in names])
    for k, got in zip(names, rows):
        _judge(k, got, reference[k][2], reference["tol"], S)
    short = [r for k, r in zip(names, rows) if len(reference[k][1]) < 4 * S]
    assert len(short) == 3 and all(r[0] == -np.inf and r[3] == 0 and r[2] == (0, 0, 0) for r in short)
    assert rows[0][1] == 0.0                                               # n = 0: no sample, peak 0


# ---- gates --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", LR.GATE_RATES)
def test_gates(reference, fs):
    """Loud, silent, quieter, below the absolute gate, loud again, and a tail that is never counted -- as it is and with DC + 0.05
    and + 0.5 (the high-pass removes it; the fp64 state carries it).  34 blocks, 26-27 past the absolute gate, 15 past both."""
    names = [f"gate@{fs}+{dc}" for dc in LR.GATE_DC]
    rows, _ = _run(fs, [reference[k][1] for k in names])
    for k, got in zip(names, rows):
        _judge(k, got, reference[k][2], reference["tol"], LR.sub_block(fs), per_block=False)
        assert got[2][0] == 34 and got[2][1] in (26, 27) and got[2][2] == 15


# ---- calibration --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [16000, 48000])
def test_calibration_on_the_device(fs):
    """A 997 Hz sine at -23 dBFS reads -26.01 LUFS; +- 0.1 LU is EBU Tech 3341's tolerance."""
    from voicesplit_amd.loudness import integrated_loudness
    x = torch.from_numpy(LR.sine(fs, 3.0, amplitude=10.0 ** (-23.0 / 20.0)))
    got = float(integrated_loudness(x.to(DEV), fs))
    also = float(integrated_loudness([x, x[: fs]], fs)[0])                 # the list form, from the host
    print(f"{fs}: {got:.4f} LUFS")
    assert abs(got - (-26.01)) <= 0.1 and also == got


# ---- independence -------------------------------------------------------------------------------------------------------------------
def _bits(dev, i):
    lufs, peak, counts, valid, energy = dev
    return (lufs[i:i + 1].cpu().view(torch.int64).item(), peak[i:i + 1].cpu().view(torch.int32).item(), tuple(counts[i].tolist()),
            int(valid[i]), energy[i].cpu().view(torch.int64).tolist())


def test_results_do_not_depend_on_position_neighbours_batch_or_call():
    fs, S = 16000, 1600
    g = np.random.default_rng(5)
    five = [(a * g.standard_normal(n)).astype(np.float32) for a, n in ((0.1, 4 * S), (0.02, 7 * S + 11), (0.3, 64 * S + 1), (0.05, 66 * S - 1), (1e-5, 9 * S))]
    _, loud = _run(fs, five, fill=1e3)
    base = [_bits(loud, i) for i in range(5)]
    assert base[4][3] == 0 and all(b[3] == 1 for b in base[:4])            # the last one is below the absolute gate
    _, quiet = _run(fs, five, fill=0.0)                                     # other neighbours (and other offsets are tried below)
    assert [_bits(quiet, i) for i in range(5)] == base
    _, again = _run(fs, five, fill=1e3)                                     # a second call
    assert [_bits(again, i) for i in range(5)] == base
    for i, c in enumerate(five):                                           # alone, at another offset
        _, alone = _run(fs, [c], fill=-7.0)
        assert _bits(alone, 0) == base[i], i
    # among 300 short clips, in other places of the table
    short = [(0.1 * g.standard_normal(n)).astype(np.float32) for n in g.integers(0, 6 * S, size=295)]
    where = [3, 77, 150, 151, 299]
    many = list(short)
    for w, c in zip(where, five):
        many.insert(w, c)
    assert len(many) == 300
    _, big = _run(fs, many, fill=1e3)
    assert [_bits(big, w) for w in where] == base


# ---- vs_scale_clips -----------------------------------------------------------------------------------------------------------------
def test_scale_clips():
    from voicesplit_amd.loudness import scale_clips_
    g = np.random.default_rng(6)
    lengths = [5000, 0, 2049, 1, 4099]                                      # more than one tile of 2048, one tile + 1, one sample, none
    clips = [g.standard_normal(n).astype(np.float32) for n in lengths]
    flat, table = _lay(clips, fill=0.37)
    assert sorted({int(a) % 4 for a in table[:, 0]}) == [1, 3]              # unaligned starts
    before = flat.clone()
    gain = torch.tensor([0.3, 2.0, 1.7, -0.5, 1e-3], dtype=torch.float32, device=DEV)
    scale_clips_(flat, table, gain)
    torch.cuda.synchronize()
    want = before.clone()
    for i, (a, n) in enumerate(table.tolist()):
        want[a:a + n] = before[a:a + n] * gain[i]
    assert torch.equal(flat, want)                                         # x * gain per clip, gaps untouched
    # a table naming clips 0, 2 and 4 leaves clips 1 and 3 and the gaps bit-identical
    flat = before.clone()
    scale_clips_(flat, table[[0, 2, 4]].contiguous(), gain[[0, 2, 4]].contiguous())
    torch.cuda.synchronize()
    want = before.clone()
    for i in (0, 2, 4):
        a, n = table[i].tolist()
        want[a:a + n] = before[a:a + n] * gain[i]
    assert torch.equal(flat, want)
    a, n = table[3].tolist()
    assert torch.equal(flat[a:a + n], before[a:a + n])
    # aligned and every misalignment of one clip; a table of empty clips only
    for shift in range(4):
        buf = torch.full((4 + 6000 + 4,), 9.0, device=DEV)
        x = torch.from_numpy(g.standard_normal(6000).astype(np.float32)).to(DEV)
        buf[shift:shift + 6000] = x
        scale_clips_(buf, torch.tensor([[shift, 6000]]), gain[2:3].contiguous())
        assert torch.equal(buf[shift:shift + 6000], x * gain[2]) and bool((buf[:shift] == 9.0).all()) and bool((buf[shift + 6000:] == 9.0).all())
    flat = before.clone()
    scale_clips_(flat, torch.tensor([[5, 0], [9, 0]]), gain[:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(flat, before)


# ---- normalize ----------------------------------------------------------------------------------------------------------------------
def _steady(fs, seconds, seed):
    """Noise whose blocks are all far above both gates before and after any gain of these tests (a gain moves blocks across the
    ABSOLUTE gate, which would change the measure itself): amplitude 0.02 with a stretch at 0.05."""
    g = np.random.default_rng(seed)
    x = 0.02 * g.standard_normal(int(fs * seconds))
    x[len(x) // 3: len(x) // 2] *= 2.5
    return torch.from_numpy(x.astype(np.float32))


def test_normalize_lands_on_the_target():
    """Bound 1e-3 LU, derived: the gain is 10^((target - lufs) / 20) in fp64 rounded once to fp32 (relative 2^-24: 5.2e-7 dB) and
    every product is rounded once (relative 2^-24 per sample, at most 2^-23 on any energy: 1.0e-6 dB); the gates are scale-invariant
    for this signal.  1.6e-6 dB in all, far inside the 1e-3 LU asked for."""
    from voicesplit_amd.loudness import integrated_loudness, normalize
    fs = 16000
    x = torch.stack((_steady(fs, 3.0, 1), 3.0 * _steady(fs, 3.0, 2))).to(DEV)
    for target in (-23.0, -30.0):
        y = normalize(x, fs, target=target)
        got = integrated_loudness(y, fs)
        print(f"target {target}: re-measured {got.tolist()}, peaks {y.abs().amax(dim=1).tolist()}")
        assert y.shape == x.shape and y.data_ptr() != x.data_ptr()
        assert float((got - target).abs().max()) <= 1e-3
    one = normalize(x[0], fs)
    assert one.shape == x[0].shape and torch.equal(one, normalize(x, fs)[0])


def test_normalize_peaky_clip_lands_at_the_cap():
    from voicesplit_amd.loudness import integrated_loudness, normalize
    fs = 16000
    x = 0.5 * _steady(fs, 3.0, 3)
    x[20000] = 0.9                                                         # about -40 LUFS with a peak of -0.9 dBFS
    x = x.to(DEV)
    y = normalize(x, fs)
    cap = 10.0 ** (-2.0 / 20.0)
    peak, lufs = float(y.abs().max()), float(integrated_loudness(y, fs))
    print(f"peak {peak!r} (cap {cap!r}), lufs {lufs:.3f}")
    assert abs(peak - cap) <= 2.0 ** -22 * cap                             # the gain and the product: two fp32 roundings
    assert lufs < -23.0 - 1.0
    free = normalize(x, fs, peak_db=None)                                  # without the cap: on the target, above full scale
    assert abs(float(integrated_loudness(free, fs)) + 23.0) <= 1e-3 and float(free.abs().max()) > 1.0


def test_true_peak_of_a_sine_at_a_quarter_of_the_rate():
    """A sin(pi n / 2 + pi / 4) has the sample peak 0.7071 A and the true peak A.  The device's 4x peak against the restatement of the
    resampler within the resampler's own bound, (T + 2) 2^-24 A[n]."""
    from voicesplit_amd.loudness import normalize, true_peaks
    fs, A, n = 16000, 0.8, 8000
    x = LR.sine(fs, n / fs, amplitude=A, freq=fs / 4.0, phase=np.pi / 4.0)
    assert abs(np.abs(x).max() - A * np.sqrt(0.5)) <= 1e-6
    y, Asum = RR.resample(x.astype(np.float64), fs, 4 * fs, with_A=True)
    T = RR.plan(fs, 4 * fs)[4]
    bound = float(((T + 2) * 2.0 ** -24 * Asum).max())
    ref_peak = float(np.abs(y).max())
    xd = torch.from_numpy(x).to(DEV)
    got = float(true_peaks(xd, torch.tensor([[0, n]]), fs)[0])
    print(f"sample peak {np.abs(x).max():.6f}, true peak: device {got:.7f}, restatement {ref_peak:.7f}, bound {bound:.2e}")
    assert abs(got - ref_peak) <= bound
    # fs / 4 is deep inside the pass band of the 4x filter: away from the clip's abrupt ends (whose overshoot is part of the clip's
    # true peak, and of ref_peak) the converted sine reaches A, not 0.7071 A
    inner = float(np.abs(y[1024:-1024]).max())
    assert abs(inner - A) <= 1e-3 * A and ref_peak >= inner and got > 0.99 * A
    # normalize to a target far above: the cap decides, on the true peak with true_peak=True, on the sample peak without
    cap = 10.0 ** (-2.0 / 20.0)
    # (this sine reads about -1.5 LUFS: + 10 LUFS asks for a gain near 3.8, which lifts either peak above the cap)
    by_sample, by_true = normalize(xd, fs, target=10.0), normalize(xd, fs, target=10.0, true_peak=True)
    assert abs(float(by_sample.abs().max()) - cap) <= 2.0 ** -22
    assert abs(float(by_true.abs().max()) - cap * float(np.abs(x).max()) / got) <= 2.0 ** -22


# ---- hooks --------------------------------------------------------------------------------------------------------------------------
def test_clip_pool_normalize():
    from voicesplit_amd.loudness import normalize
    from voicesplit_amd.mixing import ClipPool
    fs = 16000
    clips = [_steady(fs, 1.0 + 0.37 * k, 10 + k) * (0.2 + k) for k in range(4)] + [torch.zeros(2000)]
    clips[1][:3000] *= 1e-3                                                # something for the trim
    plain = ClipPool(clips, DEV)
    assert plain.lufs is None and plain.gain is None
    for o, c in zip(plain.offsets.tolist(), clips):                        # normalize=None: the waveforms as they are, as before
        assert torch.equal(plain.flat[o:o + c.numel()].cpu(), c)
    also = ClipPool(clips, DEV, normalize=None)
    assert torch.equal(also.flat, plain.flat) and torch.equal(also.bounds, plain.bounds) and torch.equal(also.peak, plain.peak)
    pool = ClipPool(clips, DEV, normalize=-23.0, sample_rate=fs)
    each = [normalize(c.to(DEV), fs) for c in clips]
    for k, (o, e) in enumerate(zip(pool.offsets.tolist(), each)):
        assert torch.equal(pool.flat[o:o + e.numel()], e), k
    by_hand = ClipPool([e.cpu() for e in each], DEV)                       # peak, bounds and range are those of the normalised clips
    assert torch.equal(pool.bounds, by_hand.bounds) and torch.equal(pool.peak, by_hand.peak) and torch.equal(pool.range, by_hand.range)
    assert pool.lufs.shape == (5,) and pool.lufs.dtype == torch.float64 and not pool.lufs.is_cuda
    assert pool.gain.shape == (5,) and pool.gain.dtype == torch.float32 and not pool.gain.is_cuda
    assert float(pool.gain[4]) == 1.0 and pool.lufs[4] == float("-inf")    # the all-zero clip keeps gain 1
    assert torch.isfinite(pool.lufs[:4]).all() and bool((pool.gain[:4] != 1.0).all())


def test_norm_wav_writer(tmp_path):
    """python -m voicesplit_amd.loudness --root ROOT --resample: <name>-norm.wav beside every .wav, at 16 kHz, at -23 LUFS; a second
    run does not take its own outputs for inputs."""
    from scipy.io import wavfile
    from voicesplit_amd import loudness
    (tmp_path / "spk" / "chap").mkdir(parents=True)
    a, b = tmp_path / "spk" / "chap" / "a.wav", tmp_path / "b.wav"
    wavfile.write(str(a), 48000, _steady(48000, 1.5, 31).numpy())
    wavfile.write(str(b), 16000, np.round(_steady(16000, 1.0, 32).numpy() * 3.0 * 32767).astype(np.int16))
    for _ in range(2):
        loudness.main(["--root", str(tmp_path), "--resample", "--sample-rate", "16000"])
        outs = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*-norm.wav"))
        assert outs == ["b-norm.wav", "spk/chap/a-norm.wav"] and len(list(tmp_path.rglob("*.wav"))) == 4
    for p, n in ((tmp_path / "spk" / "chap" / "a-norm.wav", 24000), (tmp_path / "b-norm.wav", 16000)):
        sr, y = wavfile.read(str(p))
        assert sr == 16000 and y.dtype == np.float32 and y.shape == (n,)
        got = float(loudness.integrated_loudness(torch.from_numpy(y.copy()).to(DEV), 16000))
        print(f"{p.name}: {got:.6f} LUFS")
        assert abs(got + 23.0) <= 1e-3


_MODEL = {}


def _model():
    if not _MODEL:
        import voicesplit_amd as V
        from oracle import reference_forward as R
        dims = R.default_dims()
        m = V.VoiceSplit(V.default_config()).eval()
        m.load_state_dict(R.spread_logits(R.build_state_dict(dims, 3), 8.0))
        _MODEL["m"] = m.cuda()
        _MODEL["dvec"] = R.synthetic_inputs(2, 8, dims, 13)[1].cuda()
    return _MODEL["m"], _MODEL["dvec"]


def test_separate_with_loudness():
    """loudness=None is the plain path.  With loudness=-23 the call is the composition: normalise (gain g), separate, multiply by
    fp32(1 / g).  For a clip scaled by 0.05 the output is that of the unscaled clip scaled by 0.05, within fp32 rounding of the two
    gains; derived: with g1, g2 the two gains, r = fp32(1 / g), x1 = fl(x g1) and x2 = fl(fl(0.05 x) g2) the two inputs of the network,
      out2 - 0.05 out1 = (sep(x2) - sep(x1)) r2 + sep(x1) (r2 - 0.05 r1)  up to one rounding of each product (2^-24 each),
    |r2 - 0.05 r1| <= 8 * 2^-24 r2 (seven roundings: the samples of fl(0.05 x), the two gains, the two reciprocals, fp32(0.05) and
    its product with r1), and sep(x2) - sep(x1) is the network's own answer to inputs 3 * 2^-24 apart, taken from the
    plain path."""
    from voicesplit_amd import audio
    from voicesplit_amd.loudness import _rows_table, normalize_clips_
    m, dvec = _model()
    fs, n = 16000, 8000
    x = torch.stack((_steady(fs, n / fs, 21), 2.0 * _steady(fs, n / fs, 22))).to(DEV)
    assert torch.equal(audio.separate(m, x, dvec, AUDIO, loudness=None), audio.separate(m, x, dvec, AUDIO))
    outs, seps, recips = [], [], []
    for scale in (1.0, 0.05):
        xin = (x * scale).contiguous()
        outs.append(audio.separate(m, xin, dvec, AUDIO, loudness=-23.0))
        xn = xin.clone()
        g = normalize_clips_(*_rows_table(xn), fs, -23.0)[1]
        seps.append(audio.separate(m, xn, dvec, AUDIO))
        recips.append(1.0 / g)
        assert torch.equal(outs[-1], seps[-1] * recips[-1][:, None])       # the composition, bit for bit
    (out1, out2), (sep1, sep2), (r1, r2) = outs, seps, recips
    eps = 2.0 ** -24
    print(f"gains {(1 / r1).tolist()} and {(1 / r2).tolist()}; network's answer to the input rounding {float((sep2 - sep1).abs().max()):.3e}")
    assert float(((r2 - 0.05 * r1).abs() / r2).max()) <= 8 * eps
    bound = (sep2 - sep1).abs() * r2[:, None] + 8 * eps * sep1.abs() * r2[:, None] + eps * (out2.abs() + 0.05 * out1.abs())
    err = (out2 - 0.05 * out1).abs()
    print(f"max |out(0.05 x) - 0.05 out(x)| = {float(err.max()):.3e}, max |out| = {float(out2.abs().max()):.3e}")
    assert bool((err <= bound * (1 + 1e-6)).all()) and float(out2.abs().max()) > 1e-5
