"""CPU: the resampling contract of include/voicesplit_hip.h -- its fp64 restatement (tests/resample_ref.py) against an independent
polyphase implementation (scipy.signal.resample_poly with the same filter as one FIR), the host planner inside the library
(vs_resample_plan, the code every device call checks its dims against), the definition's own sanity (DC gain, a tone), the
bookkeeping of StreamingResampler with the restatement injected as the compute function, and load_wav_native."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as RR

CHUNKINGS = {"1": [1], "7": [7], "160": [160], "1023": [1023], "mixed": [3, 500, 1, 64, 1023, 2, 161]}


def _noise(n, seed, rows=None):
    g = np.random.default_rng(seed)
    return g.standard_normal(n if rows is None else (rows, n))


# ---- the restatement against scipy's polyphase resampler ------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RR.PAIRS)
def test_restatement_matches_resample_poly(sr_in, sr_out):
    """Independent check of the indexing (b, r, the tap's sign convention, n_out).  scipy multiplies a supplied filter by `up`."""
    from scipy.signal import resample_poly
    L, M, s, H, T = RR.plan(sr_in, sr_out)
    lengths = {1000, 10 * M + 3, 1 if (sr_in, sr_out) == (44100, 16000) else 2, 777 if (sr_in, sr_out) == (22050, 16000) else 300}
    for n_in in sorted(lengths):
        x = _noise(n_in, n_in + sr_in)
        ours = RR.resample(x, sr_in, sr_out)
        theirs = resample_poly(x, L, M, window=RR.fir(sr_in, sr_out)) / L
        assert ours.shape == theirs.shape == (-(-n_in * L // M),)
        err = np.abs(ours - theirs).max()
        print(f"{sr_in} -> {sr_out} n_in={n_in}: max |restatement - resample_poly| = {err:.2e} (bound 1e-12)")
        assert err <= 1e-12


# ---- the planner -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RR.PAIRS)
def test_plan_table(sr_in, sr_out):
    from voicesplit_amd import resample
    d = resample.plan(sr_in, sr_out)
    L, M, T = RR.PLAN_TABLE[(sr_in, sr_out)]
    assert (d.L, d.M, d.T, d.H) == (L, M, T, (T - 1) // 2)
    assert (d.L, d.M, d.H, d.T) == tuple(np.array(RR.plan(sr_in, sr_out))[[0, 1, 3, 4]].astype(int))
    assert d.bank_bytes == L * T * 4 <= 230 * 1024
    for n_in in (1, 2, M, M + 1, 10 * M - 1):
        assert resample.out_len(d, n_in) == -(-n_in * L // M) == RR.out_len(sr_in, sr_out, n_in)
    # the launch the plan describes: whole periods in at most 72 KiB, so two workgroups share a CU's 160 KiB
    assert d.tile_periods >= 8 and 0 < d.lds_bytes <= 72 * 1024
    assert d.lds_bytes >= (d.tile_periods * (M + L) + T - 1) * 4


def test_plan_special_and_refused_pairs():
    from voicesplit_amd import _lib, resample
    d = resample.plan(16000, 16000)                       # a copy
    assert (d.L, d.M, d.H, d.T, d.bank_bytes) == (1, 1, 0, 1, 4) and resample.out_len(d, 12345) == 12345
    d = resample.plan(44100, 16000)
    assert d.bank_bytes == 160 * 355 * 4                  # "222 KB"
    d = resample.plan(16000, 100)                         # T = 20481 taps: no tile fits, the direct kernel
    assert (d.L, d.M, d.H, d.T, d.tile_periods, d.lds_bytes) == (1, 160, 10240, 20481, 0, 0)
    for a, b in ((16000, 44101), (44101, 16000)):
        with pytest.raises(_lib.VoiceSplitHipError, match="refused"):
            resample.plan(a, b)
    for a, b in ((0, 16000), (16000, -1)):
        with pytest.raises(_lib.VoiceSplitHipError, match="positive"):
            resample.plan(a, b)
    with pytest.raises(ValueError, match="integers"):
        resample.plan(44100.5, 16000)
    lib = _lib.load()
    assert lib.vs_resample_out_len(ctypes.byref(d), -1) == -1
    # every device call checks the dims it is given against a plan of its own, before it touches the device
    d = resample.plan(48000, 16000)
    d.T = 999
    assert lib.vs_resample_bank(ctypes.byref(d), None, None) != 0 and b"vs_resample_plan" in lib.vs_last_error()
    d = resample.plan(48000, 16000)
    one = ctypes.c_void_p(256)
    assert lib.vs_resample(ctypes.byref(d), one, one, 0, 10, 10, 30, one, 0, 11, 11, 1, None) != 0 and b"which has 10" in lib.vs_last_error()
    # output 9 of an unfinished stream reads sample 27 + 192: not in a buffer of 100 samples
    assert lib.vs_resample(ctypes.byref(d), one, one, 0, 100, 100, -1, one, 0, 10, 10, 1, None) != 0 and b"the buffer holds" in lib.vs_last_error()
    assert lib.vs_resample(ctypes.byref(d), one, one, 0, 100, 100, -1, one, 0, 10, 10, 0, None) != 0 and b"B=0" in lib.vs_last_error()
    table = (ctypes.c_longlong * 3)(0, 50, 0)
    assert lib.vs_resample_clips(ctypes.byref(d), one, one, 49, one, 100, table, one, 1, None) != 0 and b"leaves the input" in lib.vs_last_error()
    assert lib.vs_resample_clips(ctypes.byref(d), one, one, 50, one, 16, table, one, 1, None) != 0 and b"leave the output" in lib.vs_last_error()


# ---- the definition's own sanity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RR.PAIRS)
def test_dc_gain_and_a_tone_mid_signal(sr_in, sr_out):
    L, M, s, H, T = RR.plan(sr_in, sr_out)
    n_in = 2 * H + 40 * max(M, 1) + 400
    n_out = RR.out_len(sr_in, sr_out, n_in)
    mid = np.arange(n_out)
    mid = mid[((mid * M) // L >= H) & ((mid * M) // L + H < n_in)]          # outputs that read no sample outside the signal
    assert len(mid) > 50
    dc = RR.resample(np.ones(n_in), sr_in, sr_out)[mid]
    tone = RR.resample(np.sin(2 * np.pi * 1000.0 * np.arange(n_in) / sr_in), sr_in, sr_out)[mid]
    e_dc, e_tone = np.abs(dc - 1.0).max(), np.abs(tone - np.sin(2 * np.pi * 1000.0 * mid / sr_out)).max()
    print(f"{sr_in} -> {sr_out}: DC gain off by {e_dc:.2e}, 1 kHz tone off by {e_tone:.2e} (bounds 1e-6)")
    assert e_dc <= 1e-6 and e_tone <= 1e-6


# ---- StreamingResampler's bookkeeping ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 48000), (16000, 16000)])
def test_streaming_bookkeeping(sr_in, sr_out, chunking):
    """With the restatement as the compute function (it raises when an output needs a sample the kept tail no longer holds): a push
    releases exactly the outputs whose last input b + H has arrived, the tail kept is no longer than the next output needs, finish()
    completes the stream, and the concatenation is the one-shot result."""
    from voicesplit_amd.resample import StreamingResampler
    L, M, s, H, T = RR.plan(sr_in, sr_out)
    n_in = 5000 if chunking != "1" else 1200
    x = _noise(n_in, 11, rows=2)
    whole = RR.resample(x, sr_in, sr_out)
    calls = []

    def compute(buf, x_first, stream_len, y_first, y_count):
        calls.append((x_first, buf.shape[1], stream_len, y_first, y_count))
        return torch.from_numpy(RR.window(buf.numpy(), x_first, None if stream_len < 0 else stream_len, y_first, y_count, sr_in, sr_out))

    st = StreamingResampler(sr_in, sr_out, "cpu", compute=compute)
    assert st.latency_inputs == H
    outs, pos, i, sizes = [], 0, 0, CHUNKINGS[chunking]
    all_n = np.arange(RR.out_len(sr_in, sr_out, n_in) + 5)
    while pos < n_in:
        k = min(sizes[i % len(sizes)], n_in - pos)
        out = st.push(torch.from_numpy(x[:, pos:pos + k]))
        pos, i = pos + k, i + 1
        outs.append(out)
        released = int(np.sum((all_n * M) // L + H <= pos - 1))                 # outputs whose last needed input has arrived
        assert st.emitted == released == sum(o.shape[1] for o in outs), (pos, st.emitted, released)
        assert st.received == pos and st._first == max(0, (st.emitted * M) // L - H) and st._tail.shape[1] == pos - st._first
        assert st._tail.shape[1] <= 2 * H + M + k                                # the state does not grow with the stream
    outs.append(st.finish())
    got = torch.cat(outs, dim=1).numpy()
    assert got.shape == whole.shape and st.emitted == whole.shape[1]
    assert np.array_equal(got, whole)
    # only finish() knows the stream's length (a copy, H = 0, has nothing left to flush)
    assert [c[2] for c in calls if c[2] != -1] == ([n_in] if H else []) and (H == 0 or calls[-1][2] == n_in)
    with pytest.raises(RuntimeError, match="finished"):
        st.push(torch.zeros(2, 1, dtype=torch.float64))


def test_resampler_has_no_cpu_fallback():
    from voicesplit_amd import _lib, audio
    from voicesplit_amd.resample import Resampler, StreamingResampler
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        Resampler(48000, 16000, "cpu")
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        StreamingResampler(48000, 16000, "cpu")
    with pytest.raises(_lib.VoiceSplitHipError, match="no CPU fallback"):
        audio.resample(torch.zeros(100), 48000, 16000)


# ---- load_wav_native -------------------------------------------------------------------------------------------------------------
def test_load_wav_native(tmp_path):
    from scipy.io import wavfile
    from voicesplit_amd.trainer import load_wav, load_wav_native
    x = (0.5 * np.sin(np.arange(4800) * 0.01)).astype(np.float32)
    wavfile.write(str(tmp_path / "f32.wav"), 48000, x)
    wavfile.write(str(tmp_path / "i16.wav"), 48000, np.round(x * 32767).astype(np.int16))
    wavfile.write(str(tmp_path / "stereo.wav"), 44100, np.stack((x, -x / 2), axis=1))
    w, sr = load_wav_native(str(tmp_path / "f32.wav"))
    assert sr == 48000 and w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(x))
    w, sr = load_wav_native(str(tmp_path / "i16.wav"))
    assert sr == 48000 and w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(np.round(x * 32767).astype(np.int16)).float() / 32768.0)
    w, sr = load_wav_native(str(tmp_path / "stereo.wav"))
    assert sr == 44100 and w.shape == (4800,) and torch.allclose(w, torch.from_numpy(x / 4), atol=1e-7)
    # the same decoding as load_wav, which still refuses another rate
    assert torch.equal(load_wav(str(tmp_path / "i16.wav"), 48000), load_wav_native(str(tmp_path / "i16.wav"))[0])
    with pytest.raises(ValueError, match="resample the dataset first"):
        load_wav(str(tmp_path / "i16.wav"), 16000)
