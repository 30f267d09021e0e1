"""GPU: the GE2E speaker encoder (csrc/speaker.hip, voicesplit_amd/speaker.py) against torch.nn.LSTM / Linear in fp64 on the
CPU with the same weights.  Bound: the project's fp32-class bar, max|got - ref| / max|ref| <= 1e-4.

A d-vector alone is a weak oracle (with torch's default init all windows of a clip embed to almost the same direction), so every
case also compares the un-normalised per-window projections [N][emb] and layer-3's h_last [N][hidden], with the LSTM weights
scaled x3 so that gates leave their linear range, on log-mel-like inputs (real clips through logmel, or seeded values in [-6, 2])."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND = 1e-4
GOLD = os.path.join(ROOT, "tests", "golden")
AUDIO = {"n_fft": 1200, "num_freq": 601, "sample_rate": 16000, "hop_length": 160, "win_length": 400,
         "min_level_db": -100.0, "ref_level_db": 20.0}


def rel(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def build(num_mels=40, layers=3, hidden=768, emb=256, window=80, stride=40, seed=0, scale=3.0):
    from voicesplit_amd import SpeakerEncoder
    torch.manual_seed(seed)
    enc = SpeakerEncoder(num_mels, layers, hidden, emb, window, stride).eval()
    with torch.no_grad():
        for k, p in enc.lstm.named_parameters():
            if k.startswith("weight"):
                p.mul_(scale)
    return enc


def reference(enc, mel):
    """fp64 on the CPU from torch.nn.LSTM / Linear built directly: (h_last [n, H], proj [n, E], dvec [E])."""
    lstm = torch.nn.LSTM(enc.num_mels, enc.lstm_hidden, num_layers=enc.lstm_layers, batch_first=True).double()
    lin = torch.nn.Linear(enc.lstm_hidden, enc.emb_dim).double()
    sd = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
    lstm.load_state_dict({k[len("lstm."):]: v for k, v in sd.items() if k.startswith("lstm.")})
    lin.load_state_dict({"weight": sd["proj.linear_layer.weight"], "bias": sd["proj.linear_layer.bias"]})
    with torch.no_grad():
        x = mel.detach().cpu().double().unfold(1, enc.window, enc.stride).permute(1, 2, 0)
        h = lstm(x)[0][:, -1, :]
        p = lin(h)
        d = (p / torch.norm(p, p=2, dim=1, keepdim=True)).sum(0) / p.size(0)
    return h, p, d


def seeded_mel(num_mels, T, seed):
    return torch.rand(num_mels, T, generator=torch.Generator().manual_seed(seed)) * 8.0 - 6.0


def demo_wavs():
    z = np.load(os.path.join(GOLD, "demo_clips.npz"))
    return [torch.from_numpy(z[k][i].astype(np.float32) / 32768.0) for k in ("mixed", "target") for i in range(4)]


def check_stages(enc, mels, label):
    """embed_many on the device vs fp64 for every utterance long enough; prints each figure before it asserts."""
    dvec, valid, h_last, proj, wins = enc.embed_many([m.to(DEV) for m in mels], return_stages=True)
    torch.cuda.synchronize()
    worst = 0.0
    for u, m in enumerate(mels):
        if m.shape[1] < enc.window:
            assert not valid[u] and wins[u + 1] == wins[u] and dvec[u].abs().max().item() == 0.0
            continue
        assert valid[u]
        h, p, d = reference(enc, m)
        figs = (rel(h_last[wins[u]:wins[u + 1]], h), rel(proj[wins[u]:wins[u + 1]], p), rel(dvec[u], d))
        print(f"{label} utt {u} T={m.shape[1]} windows={wins[u + 1] - wins[u]}: h_last {figs[0]:.2e} proj {figs[1]:.2e} dvec {figs[2]:.2e}")
        worst = max(worst, *figs)
    assert worst <= BOUND, f"{label}: {worst:.3e}"
    return worst


def test_reduced_sizes_against_the_reference_notebooks_class():
    """tests/golden/speaker_small.npz was written by the reference notebook's own SpeakerEncoder (tools/make_speaker_golden.py)."""
    from voicesplit_amd import SpeakerEncoder
    z = np.load(os.path.join(GOLD, "speaker_small.npz"))
    m, l, h, e, w, s = (int(v) for v in z["dims"])
    enc = SpeakerEncoder(m, l, h, e, w, s).eval()
    enc.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    enc = enc.to(DEV)
    for math in ("f16x3", "fp32"):
        enc.math = math
        mels = [torch.from_numpy(z[f"mel.{T}"]).to(DEV) for T in z["frames"]]
        dvec, valid, h_last, proj, wins = enc.embed_many(mels, return_stages=True)
        assert valid.all() and wins == [0, 1, 4, 14]
        for u, T in enumerate(int(t) for t in z["frames"]):
            figs = (rel(h_last[wins[u]:wins[u + 1]], torch.from_numpy(z[f"h_last.{T}"])),
                    rel(proj[wins[u]:wins[u + 1]], torch.from_numpy(z[f"proj.{T}"])),
                    rel(dvec[u], torch.from_numpy(z[f"dvec.{T}"])))
            print(f"small {math} T={T}: h_last {figs[0]:.2e} proj {figs[1]:.2e} dvec {figs[2]:.2e}")
            assert max(figs) <= BOUND, (math, T, figs)
            # forward() is the one-utterance form of the same call
            assert torch.equal(enc(mels[u]), dvec[u])


def test_full_size_one_window_six_windows_and_a_ragged_batch():
    from voicesplit_amd import logmel
    enc = build().to(DEV)
    wavs = demo_wavs()
    check_stages(enc, [seeded_mel(40, 80, 1)], "N=1")
    check_stages(enc, [logmel(wavs[0].to(DEV), AUDIO).cpu()], "N=6 (demo clip)")
    # five clips, one too short: 6 + 3 + 0 + 1 + 24 windows
    mels = [logmel(wavs[5].to(DEV), AUDIO).cpu(), seeded_mel(40, 161, 2), seeded_mel(40, 79, 3), seeded_mel(40, 119, 4), seeded_mel(40, 1001, 5)]
    check_stages(enc, mels, "ragged")
    with pytest.raises(ValueError):
        enc(mels[2].to(DEV))
    out = enc(mels[1].to(DEV))
    assert not out.requires_grad and out.grad_fn is None


def test_fp32_arm_and_default_arithmetic_agree_with_fp64():
    from voicesplit_amd import logmel
    enc = build().to(DEV)
    mel = logmel(demo_wavs()[0].to(DEV), AUDIO).cpu()
    worst = {}
    for math in ("f16x3", "fp32"):
        enc.math = math
        worst[math] = check_stages(enc, [mel], math)
    print("fp32 arm vs default:", worst)
    enc.math = "bf16"
    from voicesplit_amd._lib import VoiceSplitHipError
    with pytest.raises(VoiceSplitHipError, match="not built"):
        enc.embed_many([mel.to(DEV)])


@pytest.mark.parametrize("layers", [1, 2])
def test_one_and_two_layers_at_reduced_size(layers):
    enc = build(8, layers, 24, 16, 10, 5, seed=layers).to(DEV)
    for math in ("f16x3", "fp32"):
        enc.math = math
        check_stages(enc, [seeded_mel(8, T, 10 + T) for T in (10, 23, 57, 9)], f"layers={layers} {math}")


def test_large_batch_every_row_equals_its_batch_of_32_and_a_rerun():
    """N = 1032 windows (43 clips of 1001 frames).  Every row: bitwise equal to the same window computed in a batch of at most 32
    (the K order of the step kernel does not depend on N); a seeded sample of 32 rows against fp64; a rerun is bit-identical."""
    enc = build().to(DEV)
    U, T = 43, 1001
    mels = [seeded_mel(40, T, 100 + u).to(DEV) for u in range(U)]
    _, valid, h_big, p_big, wins = enc.embed_many(mels, return_stages=True)
    N = wins[-1]
    assert N == 1032 and valid.all()
    _, _, h_again, p_again, _ = enc.embed_many(mels, return_stages=True)
    assert torch.equal(h_big, h_again) and torch.equal(p_big, p_again)
    # batches of 24 windows (one clip) and of 32 (a clip and a third of the next, as separate utterances)
    for u in range(U):
        _, _, h1, p1, _ = enc.embed_many([mels[u]], return_stages=True)
        assert torch.equal(h1, h_big[wins[u]:wins[u + 1]]) and torch.equal(p1, p_big[wins[u]:wins[u + 1]]), u
    _, _, h32, p32, w32 = enc.embed_many([mels[7], mels[8][:, :80 + 7 * 40].contiguous()], return_stages=True)
    assert w32[-1] == 32
    assert torch.equal(h32, h_big[wins[7]:wins[7] + 32]) and torch.equal(p32, p_big[wins[7]:wins[7] + 32])
    # a seeded sample of 32 rows against fp64
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:32].tolist()
    worst = 0.0
    for n in rows:
        u, k = divmod(n, 24)
        h, p, _ = reference(enc, mels[u][:, k * 40:k * 40 + 80].cpu())
        worst = max(worst, rel(h_big[n:n + 1], h), rel(p_big[n:n + 1], p))
    print(f"N=1032 sample of 32 rows vs fp64: {worst:.2e}")
    assert worst <= BOUND


def _stft_power(wav, dtype, n_fft=1200, hop=160, win=400):
    """|librosa.stft(n_fft, hop, win, hann, center, reflect)|^2 restated with torch.stft on the reflect-padded signal:
    periodic Hann of ``win`` zero-padded to n_fft at offset (n_fft - win) // 2 (1200 / 160 / 400: 400 centred in 1200)."""
    x = wav.to(dtype)
    pad = torch.nn.functional.pad(x[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    lo = (n_fft - win) // 2
    window = torch.zeros(n_fft, dtype=dtype)
    window[lo:lo + win] = torch.hann_window(win, periodic=True, dtype=dtype)
    D = torch.stft(pad, n_fft, hop_length=hop, win_length=n_fft, window=window, center=False, return_complex=True)
    return D.real ** 2 + D.imag ** 2          # [n_fft / 2 + 1, T]


def test_logmel_against_fp64_restatement():
    """All eight demo clips at 48000 and 47917 samples (T = 301 and 300).  Linear power within 1e-4 of the clip's largest mel power;
    log value on the bins with P_ref > 1e-5 (asserted to be >= 70 % of the bins) within 4x the error of the same restatement run
    in fp32 on the CPU (split-f16 products carry 2^-22 of the operand scale where fp32 carries 2^-24).
    Measured on an MI355X: largest log error per clip 5.0e-6 .. 1.5e-5 for the kernel, 1.9e-6 .. 7.3e-6 for
    the fp32 CPU arm, ratio 1.86 .. 3.01; linear 6.0e-7 .. 1.0e-6; share 0.749 .. 0.949."""
    from voicesplit_amd import logmel, mel_filterbank
    fb = mel_filterbank(16000, 1200, 40)
    for ci, wav in enumerate(demo_wavs()):
        for n in (48000, 47917):
            w = wav[:n].contiguous()
            got = logmel(w.to(DEV), AUDIO).double().cpu()
            P_ref = fb @ _stft_power(w, torch.float64)
            assert got.shape == P_ref.shape == (40, 1 + n // 160)
            lin = ((10.0 ** got - 1e-6) - P_ref).abs().max().item() / P_ref.max().item()
            mask = P_ref > 1e-5
            share = mask.double().mean().item()
            L_ref = torch.log10(P_ref + 1e-6)
            L_32 = torch.log10(fb.float() @ _stft_power(w, torch.float32) + 1e-6).double()
            e_gpu = (got - L_ref)[mask].abs().max().item()
            e_32 = (L_32 - L_ref)[mask].abs().max().item()
            print(f"logmel clip {ci} n={n}: linear {lin:.2e}  share {share:.3f}  log err gpu {e_gpu:.3e} vs cpu fp32 {e_32:.3e} (x{e_gpu / e_32:.2f})")
            assert lin <= BOUND
            assert share >= 0.7
            assert e_gpu <= 4.0 * e_32


@pytest.mark.parametrize("n", [601, 800, 1237])
def test_logmel_short_clips_against_fp64_restatement(n):
    """The shortest legal clip (n_fft / 2 + 1 samples; the 400-sample window reaches only 200 samples past a clip edge, so neither
    reflection is at its limit here: test_logmel_other_geometries_against_fp64_restatement has that case), a multiple of the hop
    and a non-multiple, cut from demo clip 0 at sample 16000 (largest mel power of the three slices 6.5 .. 9.4: speech, not a pause).
    The linear criterion of test_logmel_against_fp64_restatement, same bound."""
    from voicesplit_amd import logmel, mel_filterbank
    w = demo_wavs()[0][16000:16000 + n].contiguous()
    got = logmel(w.to(DEV), AUDIO).double().cpu()
    P_ref = mel_filterbank(16000, 1200, 40) @ _stft_power(w, torch.float64)
    assert got.shape == P_ref.shape == (40, 1 + n // 160)
    assert P_ref.max().item() > 1e-3
    lin = ((10.0 ** got - 1e-6) - P_ref).abs().max().item() / P_ref.max().item()
    print(f"logmel n={n}: linear {lin:.2e}")
    assert lin <= BOUND


@pytest.mark.parametrize("n_fft,hop,win,sr,mels,n", [
    (1024, 256, 1024, 22050, 80, 513),       # win == n_fft at the shortest legal clip: both reflections reach across the whole clip
    (1024, 256, 1024, 22050, 80, 1237),      # no multiple of the hop
    (256, 64, 255, 16000, 20, 129),          # odd window one short of the frame (lead 128), the shortest legal clip
    (256, 64, 255, 16000, 20, 300),
])
def test_logmel_other_geometries_against_fp64_restatement(n_fft, hop, win, sr, mels, n):
    """The linear criterion of test_logmel_short_clips_against_fp64_restatement, same bound, at the reference's waveglow block
    (1024 / 256 / 1024, 80 mels at 22050 Hz) and at 256 / 64 / 255 with 20 mels: the shortest legal clip n = n_fft / 2 + 1, where,
    once the window is as wide as the frame, the first frame's reflection lands exactly on sample n - 1 and the last frame's
    (centred on sample n - 1 here) on sample 1, and a length that is no multiple of the hop.  Neither filter bank has an empty row
    (asserted)."""
    from voicesplit_amd import logmel, mel_filterbank
    cfg = dict(AUDIO, n_fft=n_fft, num_freq=n_fft // 2 + 1, hop_length=hop, win_length=win, sample_rate=sr)
    fb = mel_filterbank(sr, n_fft, mels)
    assert fb.shape == (mels, n_fft // 2 + 1) and (fb.sum(dim=1) > 0).all()
    w = demo_wavs()[0][16000:16000 + n].contiguous()
    got = logmel(w.to(DEV), cfg, mels).double().cpu()
    P_ref = fb.double() @ _stft_power(w, torch.float64, n_fft, hop, win)
    assert got.shape == P_ref.shape == (mels, 1 + n // hop)
    assert P_ref.max().item() > 1e-3
    lin = ((10.0 ** got - 1e-6) - P_ref).abs().max().item() / P_ref.max().item()
    print(f"logmel {n_fft}/{hop}/{win} mels={mels} n={n}: linear {lin:.2e}")
    assert lin <= BOUND


def test_separate_with_reference_equals_separate_with_the_embedding():
    import voicesplit_amd as V
    from voicesplit_amd import audio
    torch.manual_seed(3)
    model = V.VoiceSplit(V.default_config()).eval().to(DEV)
    enc = build(scale=1.0, seed=4).to(DEV)
    wavs = demo_wavs()
    wav = torch.stack(wavs[:2]).to(DEV)
    refs = [wavs[4].to(DEV), wavs[5][:40000].contiguous().to(DEV)]
    got = audio.separate_with_reference(model, enc, wav, refs, AUDIO)
    dvec, valid = enc.embed_many([V.logmel(r, AUDIO) for r in refs])
    assert valid.all()
    assert torch.equal(got, audio.separate(model, wav, dvec, AUDIO))
    assert torch.isfinite(got).all()
