"""CPU: the wavernn / waveglow audio back ends without a device: the fp64 restatement (tests/audio_backend_ref.py) against
itself where it must agree with itself, the inputs of the device tests against the assumptions those tests make, and the Python
surface (``config.resolve_audio``, the named refusals, ``speaker.mel_filterbank``'s new keywords, the ABI table)."""
import ctypes

import numpy as np
import pytest
import torch

import audio_backend_ref as A
import griffin_lim_ref as G


# ---- the restatement ------------------------------------------------------------------------------------------------------------
CODECS = dict(A.DBNORM_VARIANTS, log=A.log_codec(), db01=A.db01_codec())


@pytest.mark.parametrize("name", sorted(CODECS))
def test_every_codec_round_trips_down_to_its_floor(name):
    """decode(encode(m)) == max(floor, m) to 1e-12 relative, floor = the magnitude of the codec's smallest stored value
    (``effective_floor``: the encoder's own floor, or the bottom clip of the normalisation where that lies above it)."""
    c = CODECS[name]
    m = np.concatenate(([0.0, 1e-7, c["floor"], 9.9e-5, 1e-4, 1.01e-4], np.logspace(-6, np.log10(9.9), 400)))
    back = A.decode(A.encode(m, c), c)
    want = np.maximum(A.effective_floor(c), m)
    assert np.abs(back - want).max() <= 1e-12 * want.max() and (np.abs(back - want) <= 1e-12 * want).all()
    if A.top(c) is not None:                                       # the top clip: 0 dB above ref_level_db is magnitude 10
        assert A.encode(10.0, c) == pytest.approx(A.top(c), abs=1e-12) and A.encode(30.0, c) == A.top(c)


def test_the_dbnorm_floor_is_the_fp64_expression_not_1e_5():
    assert A.dbnorm_codec()["floor"] == 9.99999999999998e-06 != 1e-5


@pytest.mark.parametrize("case", A.FRONT_CASES, ids=[f"{c[0]}-B{c[1]}-T{c[2]}-{c[4]}-a{c[5]}" for c in A.FRONT_CASES])
def test_no_front_end_input_reaches_the_top_clip(case):
    """The device tests compare decoded magnitudes, which says nothing above a top clip: no DBNORM value of their clips reaches
    max_norm (pre-emphasis only lowers the level; LOG has none)."""
    tag, B, T, gain, name, a = case
    c = A.front_codec(name, a)
    x = A.clips(tag, B, T, gain)
    assert x.shape == (B, G.GEOMETRIES[tag][1] * (T - 1)) and x.shape[1] > G.GEOMETRIES[tag][0] // 2
    if A.top(c) is None:
        return
    for b in range(B):
        mag, _ = A.analysis(x[b], G.GEOMETRIES[tag], a)
        assert A.encode(mag, c).max() < A.top(c)


def test_preemphasis_and_its_inverse_are_lfilter_and_the_segmented_form_agrees():
    x = G._clips()[0][0]
    for a in (0.97, 0.98):
        p = A.preemphasis(x, a)
        assert p[0] == x[0] and np.array_equal(p[1:], x[1:] - a * x[:-1])
        assert np.abs(A.deemphasis(p, a) - x).max() < 1e-13
        for L in (128, 256, 1024, 1600):
            assert A.segment_distance(x, a, L) < 5e-15                  # measured 0.9e-15 .. 1.4e-15 at max|y| = 1.77
    for n in (1, 127, 128, 129, 259):
        assert A.segment_distance(x[:n], 0.98, 128) < 5e-15


def test_zero_padded_transform_differs_from_the_reflected_one_only_at_the_ends():
    n_fft, hop, win = G.GEOMETRIES["G4"]
    y = G._clips()[0][0][16000:16000 + hop * 8]
    r, z = A.stft(y, n_fft, hop, win, "reflect"), A.stft(y, n_fft, hop, win, "zero")
    assert r.shape == z.shape == (n_fft // 2 + 1, 9)
    edge = -(-(n_fft // 2) // hop)
    assert np.array_equal(r[:, edge:-edge], z[:, edge:-edge]) and not np.allclose(r[:, 0], z[:, 0])


@pytest.mark.parametrize("case,init,power,n_iter", A.gl_cases()[0], ids=A.gl_cases()[1])
def test_griffin_lim_cases_stay_below_the_cap(case, init, power, n_iter):
    tw, tr = A.tolerances(case, init, power, n_iter)
    assert (tw < A.MAX_TOLERANCE).all() and (tw > 0).all() and (tr < A.MAX_TOLERANCE).all()
    wav, res = A.reference(case, init, power, n_iter)
    assert wav.shape == (case[1], G.GEOMETRIES[case[0]][1] * (case[2] - 1)) and res.shape == (n_iter, case[1])


def test_reflect_griffin_lim_restatement_is_griffin_lim_refs():
    x = A.gl_inputs("G5", 2, 11, 0.25, 0.98)
    S, ph = x["mag"][0].astype(np.float64) ** 1.5, x["random"][0].astype(np.float64)
    n_fft, hop, win = G.GEOMETRIES["G5"]
    ys, res = A.griffin_lim(S, ph, 2, G.GEOMETRIES["G5"], "reflect")
    ys0, res0 = G.griffin_lim(S, ph, 2, n_fft, hop, win)
    assert np.array_equal(ys, ys0) and np.array_equal(res, res0)


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_geometry_of_both_reference_blocks():
    from voicesplit_amd import config
    blocks = config.reference_audio_blocks()
    assert blocks["wavernn"] == A.WAVERNN and blocks["waveglow"] == A.WAVEGLOW
    r = config.resolve_audio(blocks["wavernn"])
    assert (r["n_fft"], r["hop_length"], r["win_length"]) == (2048, 200, 800) == A.wavernn_geometry(A.WAVERNN)
    assert r["backend"] == "wavernn" and r["sample_rate"] == 16000 and r["power"] == 1.5 and r["griffin_lim_iters"] == 60
    assert r["codec"] == A.dbnorm_codec(preemphasis=0.98) and r["num_mels"] == 80 and r["mel_spec"] is False
    g = config.resolve_audio(blocks["waveglow"])
    assert (g["n_fft"], g["hop_length"], g["win_length"]) == (1024, 256, 1024)
    assert g["backend"] == "waveglow" and g["codec"] == A.log_codec() and g["num_mels"] == 80 and g["mel_fmax"] == 8000.0
    assert blocks["wavernn"] == A.WAVERNN                                # the input is not written to


def test_resolve_is_idempotent_recognises_blocks_and_leaves_voicefilter_alone():
    import voicesplit_amd as V
    from voicesplit_amd import audio, config
    c = V.default_config()
    vf = c.audio["voicefilter"]
    before = dict(vf)
    assert audio.resolve(vf) is vf and audio.resolve(c.audio) is vf and vf == before
    assert audio.resolve is config.resolve_audio
    c.audio.update(config.reference_audio_blocks())
    for name in ("wavernn", "waveglow"):
        c.audio["backend"] = name
        c.audio["mel_spec"] = name == "waveglow"
        whole, block = audio.resolve(c.audio), audio.resolve(c.audio[name])
        assert whole["backend"] == block["backend"] == name and audio.resolve(whole) is whole and audio.resolve(block) == block
        assert whole["mel_spec"] is (name == "waveglow") and block["mel_spec"] is False
        assert {k: v for k, v in whole.items() if k != "mel_spec"} == {k: v for k, v in block.items() if k != "mel_spec"}
    c.audio["backend"] = "tacotron"
    with pytest.raises(ValueError, match="Invalid AudioProcessor Backend"):
        audio.resolve(c.audio)
    c.audio["backend"], c.audio["wavernn"] = "wavernn", dict(A.WAVEGLOW)
    with pytest.raises(ValueError, match="keys of 'waveglow'"):
        audio.resolve(c.audio)
    assert V.default_config() == V.default_config() and "wavernn" not in V.default_config().audio


def test_loss_dims_take_a_foreign_block():
    from voicesplit_amd import losses
    d = losses.loss_dims(2, 11, 1025, A.WAVERNN)
    assert (d.n_fft, d.hop, d.win, d.min_level_db, d.ref_level_db) == (2048, 200, 800, -100.0, 20.0)
    d = losses.loss_dims(2, 9, 513, A.WAVEGLOW)
    assert (d.n_fft, d.hop, d.win) == (1024, 256, 1024)


def test_named_refusals():
    from voicesplit_amd import audio, losses
    z = torch.zeros(1, 4, 33)
    for block in (A.wavernn_block(64, 11, 64), A.waveglow_block(64, 11, 64)):
        with pytest.raises(ValueError, match="torch_inv_spectrogram"):
            losses.sisnr_loss(z, z, z, z, None, block)
        with pytest.raises(ValueError, match="StreamingSeparator: the w.* audio back end is not streamed"):
            audio.StreamingSeparator(None, torch.zeros(1, 16), block, 8, 2)
        with pytest.raises(ValueError, match="StreamingSeparatorAtRate: the w.* audio back end is not streamed"):
            audio.StreamingSeparatorAtRate(None, torch.zeros(1, 16), block, 8, 2, 48000)
        with pytest.raises(ValueError, match="forward_ragged takes linear spectrograms"):
            audio.separate_many(None, [torch.zeros(33)], torch.zeros(1, 16), dict(block, mel_spec=True))
    with pytest.raises(ValueError, match="mel_fmax 8000.0 is above"):
        audio.resolve(dict(A.WAVERNN, sample_rate=8000))
    with pytest.raises(ValueError, match="no mel form"):
        audio.AudioProcessor(G.AUDIO).mag_to_mel(z)


def test_mel_filterbank_defaults_are_todays_bits_and_the_keywords_move_the_edges():
    from voicesplit_amd import speaker
    w = speaker.mel_filterbank(16000, 1200, 40)
    # the parent's function, restated: edges from 0 to sr / 2
    fft_f = np.linspace(0.0, 8000.0, 601)
    edges = speaker.mel_to_hz(np.linspace(speaker.hz_to_mel(0.0), speaker.hz_to_mel(8000.0), 42))
    fdiff, ramps = np.diff(edges), edges[:, None] - fft_f[None, :]
    old = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None])) * (2.0 / (edges[2:] - edges[:-2]))[:, None]
    assert np.array_equal(w.numpy(), old)
    assert torch.equal(w, speaker.mel_filterbank(16000, 1200, 40, 0.0, None)) and torch.equal(w, speaker.mel_filterbank(16000, 1200, 40, fmax=8000.0))
    g = speaker.mel_filterbank(22050, 1024, 80, 0.0, 8000.0)
    assert g.shape == (80, 513) and (g[:, int(8000.0 / (22050 / 2) * 512) + 2:] == 0).all() and (g.sum(1) > 0).all()
    lo = speaker.mel_filterbank(16000, 2048, 80, 95.0, 8000.0)
    assert (lo[:, :int(95.0 / 8000.0 * 1024)] == 0).all()


def test_abi_table_carries_the_codec_entry_points():
    from voicesplit_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 11 == lib.vs_abi_version()          # additive entries under the unchanged version
    for name in ("vs_codec_wav_to_spec", "vs_codec_decode", "vs_codec_encode", "vs_project_floor", "vs_mag_to_wav", "vs_griffin_lim_mag",
                 "vs_deemphasis_block", "vs_deemphasis_workspace_bytes", "vs_deemphasis", "vs_preemphasis"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert ctypes.sizeof(_lib.VsAudioCodec) == 6 * 4 + 5 * 8 and ctypes.sizeof(_lib.VsLossDims) == 32      # vs_loss_dims keeps its layout
    L = lib.vs_deemphasis_block()
    assert L == 128 and lib.vs_deemphasis_workspace_bytes(3, 2 * L + 3) == 2 * 256 and lib.vs_deemphasis_workspace_bytes(0, 5) == 0
    # refused before any device work
    p, ws = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    codec = _lib.VsAudioCodec(7, 0, 0, 0, 0, 0, 1e-5, -100.0, 20.0, 1.0, 0.0)
    d = _lib.VsLossDims(2, 9, 33, 64, 16, 64, -100.0, 20.0)
    assert lib.vs_codec_wav_to_spec(ctypes.byref(d), ctypes.byref(codec), p, None, 0, p, p, ws, 1 << 40, None) != 0
    assert b"unknown codec kind" in lib.vs_last_error()
    assert lib.vs_codec_decode(None, p, None, 8, p, None) != 0 and b"codec is NULL" in lib.vs_last_error()
    assert lib.vs_griffin_lim_mag(ctypes.byref(d), p, p, 1.0, 1, 2, p, None, ws, 1 << 40, None) != 0 and b"pad=2" in lib.vs_last_error()
    assert lib.vs_deemphasis(p, p, 1, 8, 0.97, ws, 1 << 20, None) != 0 and b"x == y" in lib.vs_last_error()
    assert lib.vs_deemphasis(p, ws, 1, 8, 1.0, ws, 1 << 20, None) != 0 and b"inside (-1, 1)" in lib.vs_last_error()
    assert lib.vs_project_floor(p, p, p, 0, 4, 4, 0.0, None) != 0 and b"bad dims" in lib.vs_last_error()
