"""GPU: the device resampler (csrc/resample.hip) against the fp64 restatement of its contract (tests/resample_ref.py), its position
independence (windows, chunks, clips, neighbours), and the hooks built on it (ClipPool.from_files(resample=True),
audio.separate(sample_rate=...), audio.StreamingSeparatorAtRate).

The accuracy bound is derived, not measured: every tap is rounded once to fp32 (error <= 2^-24 |tap x| each, 2^-24 A[n] in all with
A[n] = sum |tap x|) and the fmaf chain rounds once per step, each partial sum being at most A[n] in magnitude (T 2^-24 A[n]):
|y - ref| <= (T + 2) 2^-24 A[n], checked on EVERY output.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import resample_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AUDIO = {"n_fft": 1200, "hop_length": 160, "win_length": 400, "min_level_db": -100.0, "ref_level_db": 20.0}
# beside the issue's seven: the direct kernel (T = 20481: no tile fits LDS), M = 2 (the smallest skewed stride) and the copy
EXTRA_PAIRS = [(16000, 100), (32000, 16000), (16000, 16000)]
_R = {}


def _resampler(sr_in, sr_out):
    from voicesplit_amd.resample import Resampler
    if (sr_in, sr_out) not in _R:
        _R[(sr_in, sr_out)] = Resampler(sr_in, sr_out, DEV)
    return _R[(sr_in, sr_out)]


def _signal(rows, n, seed):
    """Noise plus a tone, a different one per row, fp32."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    x = 0.3 * torch.randn(rows, n, generator=g, dtype=torch.float64) + 0.5 * torch.sin(0.05 * t)[None] * torch.arange(1, rows + 1)[:, None]
    return x.float()


def _judge(tag, got, x, sr_in, sr_out, ref=None):
    """got [B, n_out] (device) against the restatement of x [B, n_in] (host fp32), every output, bound (T + 2) 2^-24 A[n]."""
    T = RR.plan(sr_in, sr_out)[4]
    y, A = ref if ref is not None else RR.resample(x.double().numpy(), sr_in, sr_out, with_A=True)
    got = got.detach().cpu().double().numpy()
    assert got.shape == y.shape, (got.shape, y.shape)
    assert np.isfinite(got).all()
    bound = (T + 2) * 2.0 ** -24 * A
    err = np.abs(got - y)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"  {tag}: {got.size} outputs, max |err| {err.max() if err.size else 0.0:.3e}, worst err / bound {worst:.3f} (T = {T})")
    assert np.all(err <= bound), (tag, worst)
    return y, A


def _lengths(d):
    tile = d.tile_periods * d.M if d.tile_periods else 256 * d.M          # inputs of one workgroup's outputs (direct kernel: 256 outputs)
    return [1, 50, tile, tile + 1, 3 * tile + 17]


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RR.PAIRS + EXTRA_PAIRS)
def test_every_output_is_within_the_rounding_bound(sr_in, sr_out):
    """n_in = 1, 50 (shorter than H), exactly one workgroup tile, one tile + 1, three tiles + 17; B = 3 rows that are views with a row
    stride larger than the row, on both sides; the floats behind the output rows stay untouched."""
    rs = _resampler(sr_in, sr_out)
    d = rs.dims
    print(f"{sr_in} -> {sr_out}: L={d.L} M={d.M} H={d.H} T={d.T} tile_periods={d.tile_periods} lds_bytes={d.lds_bytes}")
    for n_in in _lengths(d):
        if (sr_in, sr_out) == (16000, 100) and n_in > 50000:
            n_in = 2 * 256 * d.M + 17                                      # (the fp64 restatement of 20481 taps per output is slow)
        x = _signal(3, n_in, n_in + sr_in)
        wide = torch.full((3, n_in + 5), 1e3)
        wide[:, :n_in] = x
        n_out = rs.out_len(n_in)
        assert n_out == RR.out_len(sr_in, sr_out, n_in)
        out_wide = torch.full((3, n_out + 3), -7.0, device=DEV)
        got = rs.window(wide.to(DEV)[:, :n_in], 0, n_in, 0, n_out, out=out_wide[:, :n_out])
        assert torch.all(out_wide[:, n_out:] == -7.0)
        ref = _judge(f"n_in={n_in} strided B=3", got, x, sr_in, sr_out)
        # the plain calls: contiguous batch, and one row alone -- the same bits
        assert torch.equal(rs(x.to(DEV)), got) and torch.equal(rs(x[1].to(DEV)), got[1])
        if sr_in == sr_out:
            assert torch.equal(got.cpu(), x)


# ---- clips --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 44100), (48000, 44100)])
def test_clips_ignore_their_neighbours(sr_in, sr_out):
    """Five clips of 1025, 3001, 50, 4096 and 777 samples at odd offsets of one flat buffer, once with neighbours of amplitude 1e3
    between them and once with zeros: identical outputs, within the bound, and the floats between the output regions untouched."""
    rs = _resampler(sr_in, sr_out)
    sizes = [1025, 3001, 50, 4096, 777]
    gaps = [3, 7, 1, 13, 5, 9]                                             # in front of clip 0, between the clips, behind the last
    clips = [_signal(1, n, 100 + n)[0] for n in sizes]
    n_out = [rs.out_len(n) for n in sizes]
    starts_in = np.cumsum([gaps[0]] + [sizes[i] + gaps[i + 1] for i in range(4)]).tolist()
    starts_out = np.cumsum([gaps[0]] + [n_out[i] + gaps[i + 1] for i in range(4)]).tolist()
    assert any(s % 4 for s in starts_in) and any(s % 4 for s in starts_out)
    total_in, total_out = starts_in[-1] + sizes[-1] + gaps[-1], starts_out[-1] + n_out[-1] + gaps[-1]
    table = torch.tensor([[starts_in[i], sizes[i], starts_out[i]] for i in range(5)], dtype=torch.int64)
    outs = []
    for fill in (1e3, 0.0):
        flat = torch.full((total_in,), fill)
        for s, c in zip(starts_in, clips):
            flat[s:s + c.numel()] = c
        out = torch.full((total_out,), 123.0, device=DEV)
        rs.clips_into(flat.to(DEV), out, table)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    between = torch.ones(total_out, dtype=torch.bool)
    for i in range(5):
        between[starts_out[i]:starts_out[i] + n_out[i]] = False
        _judge(f"{sr_in} -> {sr_out} clip {i} ({sizes[i]} samples)", outs[0][None, starts_out[i]:starts_out[i] + n_out[i]], clips[i][None],
               sr_in, sr_out)
    assert int(between.sum()) == sum(gaps) and torch.all(outs[0][between] == 123.0)
    # Resampler.clips (its own flat layout) and the row call give the same bits
    listed = rs.clips(clips)
    for i in range(5):
        assert torch.equal(listed[i].cpu(), outs[0][starts_out[i]:starts_out[i] + n_out[i]])
        assert torch.equal(rs(clips[i].to(DEV)).cpu(), listed[i].cpu())


# ---- position independence and streaming ----------------------------------------------------------------------------------------
STREAM_PAIRS = [(48000, 16000), (44100, 16000), (16000, 48000)]


@pytest.mark.parametrize("sr_in,sr_out", STREAM_PAIRS + [(48000, 44100)])
def test_windows_of_one_stream_agree_bit_for_bit(sr_in, sr_out):
    rs = _resampler(sr_in, sr_out)
    d = rs.dims
    n_in = 5000
    x = _signal(2, n_in, 5).to(DEV)
    whole = rs(x)
    n_out = whole.shape[1]
    for y_first, y_count in ((0, n_out), (1, n_out - 1), (n_out // 3 + 1, n_out // 2), (n_out - 7, 7), (n_out // 2, 1)):
        assert torch.equal(rs.window(x, 0, n_in, y_first, y_count), whole[:, y_first:y_first + y_count]), (y_first, y_count)
        # the same outputs from a buffer that holds only the samples they read, at another place in memory
        lo = max(0, y_first * d.M // d.L - d.H)
        hi = min(n_in, (y_first + y_count - 1) * d.M // d.L + d.H + 1)
        part = x[:, lo:hi].clone()
        assert torch.equal(rs.window(part, lo, n_in, y_first, y_count), whole[:, y_first:y_first + y_count]), (y_first, y_count, lo, hi)
    # a far position in a long stream: the same samples give the same bits wherever L and M allow the same phase
    far = 3 * (1 << 31) // d.M * d.M                                        # input position, a multiple of M: output far / M * L, phase 0
    y_far = far // d.M * d.L
    first = -(-d.H * d.L // d.M) + 1                                        # outputs that read no sample in front of the buffer
    count = min(300, (n_in - d.H) * d.L // d.M - 2 - first)                  # nor behind it (the end of this stream is not known)
    assert count > 100
    got = rs.window(x, far, -1, y_far + first, count)
    assert torch.equal(got, whole[:, first:first + count])


@pytest.mark.parametrize("chunking", ["1", "7", "160", "1023", "random"])
@pytest.mark.parametrize("sr_in,sr_out", STREAM_PAIRS)
def test_streaming_equals_the_one_shot_call(sr_in, sr_out, chunking):
    from voicesplit_amd.resample import StreamingResampler
    rs = _resampler(sr_in, sr_out)
    n_in = 5000
    x = _signal(2, n_in, 6).to(DEV)
    whole = rs(x)
    g = torch.Generator().manual_seed(9)
    st = StreamingResampler(sr_in, sr_out, DEV, resampler=rs)
    outs, pos = [], 0
    while pos < n_in:
        k = int(torch.randint(1, 700, (1,), generator=g)) if chunking == "random" else int(chunking)
        k = min(k, n_in - pos)
        outs.append(st.push(x[:, pos:pos + k]))
        pos += k
    outs.append(st.finish())
    got = torch.cat(outs, dim=1)
    assert got.shape == whole.shape and torch.equal(got, whole)


def test_calls_that_would_read_outside_the_buffer_are_refused():
    from voicesplit_amd import _lib
    rs = _resampler(48000, 16000)
    x = torch.zeros(1, 1000, device=DEV)
    with pytest.raises(_lib.VoiceSplitHipError, match="the buffer holds"):
        rs.window(x, 0, -1, 0, 334)                                        # the end is not known: output 333 reads up to sample 1191
    with pytest.raises(_lib.VoiceSplitHipError, match="the buffer holds"):
        rs.window(x, 500, 2000, 0, 10)                                     # sample 0 is inside the stream and not in the buffer
    assert rs.window(x, 0, 1000, 0, 334).shape == (1, 334)


# ---- hooks ----------------------------------------------------------------------------------------------------------------------
def test_pool_from_files_of_mixed_rates(tmp_path):
    from scipy.io import wavfile
    from voicesplit_amd import mixing
    from voicesplit_amd.trainer import load_wav_native
    spec = [("a48.wav", 48000, 9000, np.int16), ("b44.wav", 44100, 6001, np.float32), ("c16.wav", 16000, 2500, np.int16),
            ("d48.wav", 48000, 4000, np.float32)]
    paths = []
    for k, (name, sr, n, dtype) in enumerate(spec):
        x = _signal(1, n, 40 + k)[0].numpy() * 0.5
        x[: n // 5] *= 1e-4                                                 # a quiet lead-in for the trim
        wavfile.write(str(tmp_path / name), sr, x.astype(np.float32) if dtype == np.float32 else np.round(x * 20000).astype(np.int16))
        paths.append(str(tmp_path / name))
    with pytest.raises(ValueError, match="resample the dataset first"):
        mixing.ClipPool.from_files(paths, 16000, DEV)
    pool = mixing.ClipPool.from_files(paths, 16000, DEV, resample=True)
    assert len(pool) == 4
    expect = []
    for p in paths:
        w, sr = load_wav_native(p)
        expect.append(w.to(DEV) if sr == 16000 else _resampler(sr, 16000)(w.to(DEV)))
    sizes = [e.numel() for e in expect]
    assert sizes == [3000, -(-6001 * 160 // 441), 2500, -(-4000 // 3)]
    assert pool.offsets.tolist() == [0] + np.cumsum(sizes).tolist() and pool.total == sum(sizes) == pool.flat.numel()
    assert torch.equal(pool.offsets_dev.cpu(), pool.offsets)
    for k, e in enumerate(expect):
        o = int(pool.offsets[k])
        assert torch.equal(pool.flat[o:o + sizes[k]], e), spec[k][0]
    # the trim ran on the converted clips: the same bounds as a pool built from them
    again = mixing.ClipPool([e.cpu() for e in expect], DEV)
    assert pool.bounds.shape == (4, 2) and torch.equal(pool.bounds, again.bounds) and torch.equal(pool.peak, again.peak)
    assert all(0 <= int(b[0]) < int(b[1]) <= n for b, n in zip(pool.bounds, sizes))


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


def _speechlike(B, n, sr, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / float(sr)
    tones = sum(a * torch.sin(2 * np.pi * fr * t + p) for a, fr, p in [(0.05, 220.0, 0.1), (0.03, 1750.0, 1.0), (0.01, 5300.0, 2.0)])
    return (tones[None] + 0.004 * torch.randn(B, n, generator=g)).float()


def test_separate_at_another_rate_is_the_composition():
    from voicesplit_amd import audio
    m, dvec = _model()
    n = 24007                                                               # 0.5 s at 48 kHz; 8003 samples at 16 kHz, not a multiple of hop
    wav = _speechlike(2, n, 48000, 3).cuda()
    got = audio.separate(m, wav, dvec, AUDIO, sample_rate=48000)
    down, up = _resampler(48000, 16000), _resampler(16000, 48000)
    x = down(wav)
    assert x.shape[1] == 8003
    x = torch.nn.functional.pad(x, (0, 8160 - 8003))
    by_hand = up(audio.separate(m, x, dvec, AUDIO))
    assert by_hand.shape[1] >= n
    assert got.shape == wav.shape and torch.isfinite(got).all() and torch.equal(got, by_hand[:, :n])
    assert float(got.abs().max()) > 1e-4
    # the configured rate, named or not, is the plain path
    w16 = _speechlike(2, 8000, 16000, 4).cuda()
    assert torch.equal(audio.separate(m, w16, dvec, AUDIO, sample_rate=16000), audio.separate(m, w16, dvec, AUDIO))


def test_streaming_separator_at_48k():
    """Pushes of a sound card's 10 ms and of uneven sizes.  The concatenation has the input's length and equals, bit for bit, the
    composition by hand: the stream converted in ONE call (padded with zeros to whole hops), fed to StreamingSeparator in the blocks
    the class is documented to hand over (after each push, the whole hops of the outputs whose last input has arrived), converted
    back in ONE call and cut.  No sample stays withheld for as long as the reported latency."""
    from voicesplit_amd import audio
    from voicesplit_amd.resample import ready_outputs
    m, dvec = _model()
    C, Rl, hop = 16, 8, 160
    n = 72011                                                               # 1.5 s at 48 kHz
    wav = _speechlike(2, n, 48000, 5).cuda()
    down, up = _resampler(48000, 16000), _resampler(16000, 48000)
    x = down(wav)
    x = torch.nn.functional.pad(x, (0, -x.shape[1] % hop))
    for tag, sizes in (("10 ms pushes", (480,)), ("uneven pushes", (4801, 37, 12000, 1))):
        st = audio.StreamingSeparatorAtRate(m, dvec, AUDIO, C, Rl, 48000)
        sep = audio.StreamingSeparator(m, dvec, AUDIO, C, Rl)
        lat = st.latency_samples
        assert lat == 192 + 3 * (hop + (C + Rl + 65 + 2 * 4) * hop + 64)
        outs, ref16, pos, i, returned, worst, fed = [], [], 0, 0, 0, 0, 0
        while pos < n:
            k = min(sizes[i % len(sizes)], n - pos)
            out = st.push(wav[:, pos:pos + k])
            pos, i, returned = pos + k, i + 1, returned + out.shape[1]
            outs.append(out)
            worst = max(worst, pos - returned)                               # withheld when the push returns
            upto = ready_outputs(down.dims, pos) // hop * hop
            if upto > fed:
                ref16.append(sep.push(x[:, fed:upto].contiguous()))
                fed = upto
        outs.append(st.finish())
        if x.shape[1] > fed:
            ref16.append(sep.push(x[:, fed:].contiguous()))
        ref16.append(sep.finish())
        ref16 = torch.cat(ref16, dim=1)
        assert ref16.shape == x.shape
        ref = up(ref16.contiguous())[:, :n]
        got = torch.cat(outs, dim=1)
        err = (got - ref).abs().max().item() if got.shape == ref.shape else float("nan")
        print(f"{tag}: {got.shape[1]} samples, max |streamed - by hand| {err:.3e} (range {ref.abs().max().item():.3e}); "
              f"at most {worst} samples withheld behind a push, reported latency {lat}")
        assert got.shape == wav.shape and torch.isfinite(got).all() and float(got.abs().max()) > 1e-4
        assert worst < lat
        assert torch.equal(got, ref)
