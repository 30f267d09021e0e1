"""CPU: the speaker encoder's module surface, window plan, mel filterbank, ABI argument checks and the host logic of the
preprocessing tool (no compute calls here -- no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch


def test_module_surface_matches_torch_lstm_and_linear():
    from voicesplit_amd import SpeakerEncoder
    from voicesplit_amd._lib import VoiceSplitHipError
    torch.manual_seed(5)
    enc = SpeakerEncoder()
    torch.manual_seed(5)
    lstm = torch.nn.LSTM(40, 768, 3, batch_first=True)
    lin = torch.nn.Linear(768, 256)
    ref = {f"lstm.{k}": v for k, v in lstm.state_dict().items()}
    ref.update({"proj.linear_layer.weight": lin.weight.detach(), "proj.linear_layer.bias": lin.bias.detach()})
    sd = enc.state_dict()
    assert list(sd) == list(ref)
    assert list(sd)[:4] == ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"] and len(sd) == 14
    for k in sd:
        assert sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype, k
        assert torch.equal(sd[k], ref[k]), k                      # the default init under a seed is torch's
    other = SpeakerEncoder()
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), sd.values()))
    with pytest.raises(VoiceSplitHipError, match="no CPU fallback"):
        enc(torch.zeros(40, 100))
    with pytest.raises(VoiceSplitHipError, match="no CPU fallback"):
        enc.embed_many([torch.zeros(40, 100)])
    import voicesplit_amd
    assert voicesplit_amd.SpeakerEncoder is SpeakerEncoder and callable(voicesplit_amd.logmel) and callable(voicesplit_amd.mel_filterbank)
    # the packed-weight cache does not travel with copies
    import copy
    import pickle
    enc.__dict__["_prepared"] = ("key", object())
    for c in (copy.deepcopy(enc), pickle.loads(pickle.dumps(enc))):
        assert "_prepared" not in c.__dict__ and list(c.state_dict()) == list(sd)


@pytest.mark.parametrize("T,n", [(80, 1), (119, 1), (120, 2), (301, 6), (1001, 24)])
def test_window_count(T, n):
    from voicesplit_amd.speaker import window_count
    assert window_count(T) == n == (T - 80) // 40 + 1
    assert torch.zeros(40, T).unfold(1, 80, 40).shape[1] == n


def test_short_clip_and_ragged_offsets():
    from voicesplit_amd.speaker import window_count, window_plan
    assert window_count(79) == 0
    frames, wins = window_plan([301, 79, 80, 1001, 119])
    assert frames == [0, 301, 380, 460, 1461, 1580]
    assert wins == [0, 6, 6, 7, 31, 32]
    assert window_plan([10, 23, 57], 10, 5)[1] == [0, 1, 4, 14]


def test_forward_refuses_a_clip_shorter_than_one_window(monkeypatch):
    from voicesplit_amd import SpeakerEncoder, _call
    monkeypatch.setattr(_call, "dev_check", lambda *a, **k: None)         # no device here: only the length check is exercised
    with pytest.raises(ValueError, match="fewer than one window"):
        SpeakerEncoder()(torch.zeros(40, 79))


def test_mel_filterbank_is_the_slaney_bank():
    from voicesplit_amd.speaker import hz_to_mel, mel_band_edges, mel_filterbank, mel_to_hz
    fb = mel_filterbank(16000, 1200, 40)
    assert tuple(fb.shape) == (40, 601) and fb.dtype == torch.float64 and (fb >= 0).all()
    w = fb.numpy()
    assert float(hz_to_mel(1000.0)) == 15.0
    assert abs(float(hz_to_mel(500.0)) - 7.5) < 1e-12
    assert abs(float(hz_to_mel(6400.0)) - 42.0) < 1e-9            # 15 + ln(6.4) / (ln(6.4) / 27)
    edges = mel_band_edges(16000, 40)
    assert len(edges) == 42 and edges[0] == 0.0 and abs(edges[-1] - 8000.0) < 1e-9
    m = hz_to_mel(edges)
    assert np.allclose(np.diff(m), float(hz_to_mel(8000.0)) / 41, rtol=0, atol=1e-10)
    assert np.allclose(mel_to_hz(m), edges, rtol=1e-13)
    freqs = np.linspace(0.0, 8000.0, 601)
    for i in range(40):
        nz = np.nonzero(w[i])[0]
        assert len(nz) >= 1 and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))           # one run of bins
        assert edges[i] < freqs[nz[0]] and freqs[nz[-1]] < edges[i + 2]                    # inside its band
        k = int(np.argmax(w[i]))
        assert (np.diff(w[i][nz[0]:k + 1]) > 0).all() and (np.diff(w[i][k:nz[-1] + 1]) < 0).all()   # rising, then falling
        if i:
            assert nz[0] <= np.nonzero(w[i - 1])[0][-1]                                    # consecutive rows overlap
        # the row is the continuous triangle over (f_lo, f_c, f_hi) of unit peak, times 2 / (f_hi - f_lo), sampled at the bin centres
        lo, c, hi = edges[i], edges[i + 1], edges[i + 2]
        tri = np.maximum(0.0, np.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c)))
        assert np.allclose(w[i] * (hi - lo) / 2.0, tri, rtol=0, atol=1e-12)
        # whose integral (peak 1, base hi - lo) times the norm is 1
        assert abs((0.5 * (hi - lo)) * (2.0 / (hi - lo)) - 1.0) < 1e-15
        assert abs(w[i].max() * (hi - lo) / 2.0 - tri.max()) < 1e-12


def test_abi_argument_checks_run_without_a_device():
    from voicesplit_amd import _lib
    lib = _lib.load()
    assert lib.vs_abi_version() == 11

    def dims(n_mels=40, hidden=768, layers=3, emb=256, window=80, stride=40, math=_lib.MATH_F16X3):
        return _lib.VsSpeakerDims(n_mels, hidden, layers, emb, window, stride, math)

    good = dims()
    pb = lib.vs_speaker_prepared_bytes(ctypes.byref(good))
    assert pb % 256 == 0 and pb > 2 * 2 * (768 + 2 * 1536) * 3072           # the hi + lo f16 planes of [W_ih | W_hh] dominate
    assert lib.vs_speaker_prepared_bytes(ctypes.byref(dims(math=_lib.MATH_FP32))) % 256 == 0
    for bad, msg in ((dims(hidden=770), b"multiple of 8"), (dims(layers=0), b"layers"), (dims(layers=5), b"layers"),
                     (dims(window=0), b"window"), (dims(stride=0), b"stride"), (dims(math=7), b"unknown math"),
                     (dims(math=_lib.MATH_BF16), b"not built")):
        assert lib.vs_speaker_prepared_bytes(ctypes.byref(bad)) == 0 and msg in lib.vs_last_error(), msg
        assert lib.vs_speaker_workspace_bytes(ctypes.byref(bad), 6, 301) == 0 and msg in lib.vs_last_error()
        assert lib.vs_speaker_prepare(ctypes.byref(bad), None, None, 0, None) != 0 and msg in lib.vs_last_error()
        assert lib.vs_speaker_embed(ctypes.byref(bad), None, 0, None, 301, None, None, 1, 6, None, None, None, None, 0, None) != 0
        assert msg in lib.vs_last_error()
    # size queries: 256-byte multiples, monotone in N and in the frame count
    sizes = [lib.vs_speaker_workspace_bytes(ctypes.byref(good), n, 1001) for n in (1, 6, 24, 64, 1024)]
    assert all(s % 256 == 0 and s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.vs_speaker_workspace_bytes(ctypes.byref(good), 6, 301) < lib.vs_speaker_workspace_bytes(ctypes.byref(good), 6, 1001)
    assert lib.vs_speaker_workspace_bytes(ctypes.byref(good), 0, 301) == 0 and b"windows" in lib.vs_last_error()
    assert lib.vs_speaker_workspace_bytes(ctypes.byref(good), 1, 79) == 0 and b"total_frames" in lib.vs_last_error()
    # NULL buffers, small or misaligned buffers: refused before any launch
    one = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(264)
    sp = _lib.VsSpeakerParams()
    assert lib.vs_speaker_prepare(ctypes.byref(good), None, one, pb, None) != 0 and b"NULL" in lib.vs_last_error()
    assert lib.vs_speaker_prepare(ctypes.byref(good), ctypes.byref(sp), one, pb, None) != 0 and b"NULL parameter" in lib.vs_last_error()
    for k in range(4):
        sp.w_ih[k] = sp.w_hh[k] = sp.b_ih[k] = sp.b_hh[k] = 256
    sp.proj_w = sp.proj_b = 256
    assert lib.vs_speaker_prepare(ctypes.byref(good), ctypes.byref(sp), one, pb - 1, None) != 0 and b"too small" in lib.vs_last_error()
    assert lib.vs_speaker_prepare(ctypes.byref(good), ctypes.byref(sp), odd, pb, None) != 0 and b"misaligned" in lib.vs_last_error()
    wb = lib.vs_speaker_workspace_bytes(ctypes.byref(good), 6, 301)
    assert lib.vs_speaker_embed(ctypes.byref(good), None, pb, None, 301, None, None, 1, 6, None, None, None, None, wb, None) != 0
    assert b"NULL" in lib.vs_last_error()
    assert lib.vs_speaker_embed(ctypes.byref(good), one, pb, one, 301, one, one, 1, 6, None, None, one, one, wb - 1, None) != 0
    assert b"workspace too small" in lib.vs_last_error()
    assert lib.vs_speaker_embed(ctypes.byref(good), one, pb, one, 301, one, one, 1, 6, None, None, one, odd, wb, None) != 0
    assert b"misaligned" in lib.vs_last_error()
    assert lib.vs_speaker_embed(ctypes.byref(good), one, pb - 1, one, 301, one, one, 1, 6, None, None, one, one, wb, None) != 0
    assert b"prepared buffer too small" in lib.vs_last_error()
    assert lib.vs_speaker_embed(ctypes.byref(good), one, pb, one, 301, one, one, 0, 6, None, None, one, one, wb, None) != 0
    assert lib.vs_speaker_embed(ctypes.byref(good), one, pb, one, 79, one, one, 1, 1, None, None, one, one, wb, None) != 0
    # log-mel front end
    ld = _lib.VsLossDims(1, 301, 601, 1200, 160, 400, -100.0, 20.0)
    mb = lib.vs_logmel_workspace_bytes(ctypes.byref(ld), 48000, 40)
    assert mb % 256 == 0 and mb > 0 and mb < lib.vs_logmel_workspace_bytes(ctypes.byref(ld), 160000, 40)
    assert lib.vs_logmel_workspace_bytes(ctypes.byref(ld), 47917, 40) > 0            # any length above n_fft / 2
    assert lib.vs_logmel_workspace_bytes(ctypes.byref(ld), 600, 40) == 0 and b"reflect padding" in lib.vs_last_error()
    assert lib.vs_wav_to_logmel(ctypes.byref(ld), one, 600, one, 40, one, one, mb, None) != 0 and b"reflect padding" in lib.vs_last_error()
    assert lib.vs_wav_to_logmel(ctypes.byref(ld), None, 48000, one, 40, one, one, mb, None) != 0 and b"NULL" in lib.vs_last_error()
    assert lib.vs_wav_to_logmel(ctypes.byref(ld), one, 48000, one, 40, one, one, mb - 1, None) != 0 and b"too small" in lib.vs_last_error()
    assert lib.vs_wav_to_logmel(ctypes.byref(ld), one, 48000, one, 40, one, odd, mb, None) != 0 and b"misaligned" in lib.vs_last_error()
    assert lib.vs_wav_to_logmel(ctypes.byref(ld), one, 48000, one, 0, one, one, mb, None) != 0 and b"n_mels" in lib.vs_last_error()
    bad_ld = _lib.VsLossDims(1, 301, 600, 1200, 160, 400, -100.0, 20.0)
    assert lib.vs_wav_to_logmel(ctypes.byref(bad_ld), one, 48000, one, 40, one, one, mb, None) != 0 and b"n_fft/2+1" in lib.vs_last_error()


class _FakeEncoder:
    num_mels, window = 40, 80

    def __init__(self):
        self.batches = []

    def embed_many(self, mels):
        self.batches.append(len(mels))
        valid = torch.tensor([m.shape[1] >= self.window for m in mels])
        dvec = torch.stack([torch.full((256,), float(m.shape[1])) * float(v) for m, v in zip(mels, valid)])
        return dvec, valid


def test_cli_host_logic_names_marker_and_batches(tmp_path):
    """Against a temporary directory and a fake encoder: X-ref_emb.wav names an utterance, X-emb.pt receives a 1-D float
    tensor, or the [0] marker for a clip too short; the items go through the encoder in batches."""
    from voicesplit_amd import speaker
    data = tmp_path / "data"
    data.mkdir()
    frames = {"a": 301, "b": 79, "c": 120, "d": 1001, "e": 2}
    for name in frames:
        (data / f"{name}-ref_emb.wav").write_text(f"wavs/{name}.wav\n")
    (data / "a-mixed.wav").write_text("not a reference")
    seen = []

    def load_wav(path, sr):
        seen.append(path)
        assert sr == 16000
        name = os.path.basename(path)[0]
        return torch.zeros(160 * (frames[name] - 1) + 1)

    cfg = {"n_fft": 1200, "hop_length": 160, "win_length": 400, "sample_rate": 16000}
    enc = _FakeEncoder()
    good = speaker.embed_directory(enc, str(data), cfg, batch=2, device="cpu", root=str(tmp_path),
                                   load_wav=load_wav, mel_fn=lambda w: torch.zeros(40, 1 + w.numel() // 160))
    assert good == 3
    assert seen == [str(tmp_path / "wavs" / f"{n}.wav") for n in "abcde"]
    assert enc.batches == [2, 2]                       # (a, b), (c, d); e is shorter than the STFT padding and never reaches the encoder
    for name, T in frames.items():
        out = torch.load(str(data / f"{name}-emb.pt"))
        if T >= 80:
            assert out.dtype == torch.float32 and tuple(out.shape) == (256,) and out[0].item() == float(T)
        else:
            assert out.tolist() == [0]                 # what evaluate.eval_batches and BatchFeeder drop
    assert sorted(p.name for p in data.glob("*-emb.pt")) == [f"{n}-emb.pt" for n in "abcde"]
    assert speaker.emb_path("/x/y/spk-ref_emb.wav") == "/x/y/spk-emb.pt"
