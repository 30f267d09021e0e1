"""GPU: the audio legs (vs_wav_to_spec, vs_spec_to_wav) at STFT geometries other than the reference's 1200 / 160 / 400, each clip
against the fp64 oracle (oracle/reference_audio.py) with the bounds of tests/test_gpu_audio.py unchanged: linear magnitude within
2e-5 ref + 3e-6 of the frame's maximum, median dB error below 1e-6, phase within 1e-3 on the bins above 1e-2 of the maximum, waveform
within 2e-5 (tests/test_gpu_loss_b64._audio_legs_per_clip).  The loss head, Griffin-Lim, the log-mel front end and the streaming
separator meet the same geometries in tests/test_gpu_loss.py, test_gpu_griffin_lim.py, test_gpu_speaker.py and test_gpu_stream.py.

What the geometry decides in csrc/stft.hip and its callers, and which one reaches it (griffin_lim_ref.GEOMETRIES):

  G1  64 / 11 / 64     win == n_fft; an odd hop that does not divide the window, so a sample lies under ceil(64 / 11) = 6 frames (the
                       gather loops have walked 3); with T = 4 the clip has S = 33 = n_fft / 2 + 1 samples, the shortest one the
                       library takes: the reflected index of stft_frames_kernel lands exactly on S - 1 and on 0; M = B T is below
                       one GEMM tile
  G2  402 / 100 / 200  n_fft = 2 (mod 4): F = 202 and K = 2 F = 404 = ldk, so spec_to_reim_kernel writes no row padding and the
                       split-f16 contraction over the whole row has nothing zeroed behind it; hop = win / 2
  G3  256 / 64 / 255   an odd window one short of the frame (lead = 128), win % 4 != 0 (the GEMM's scalar-load instance)
  G4  1024 / 256 / 1024  the waveglow block of the reference's config.json: a contraction over 1024 window samples
  G5  2048 / 200 / 800   its wavernn block (50 ms frames, 12.5 ms hops at 16 kHz): K = 2050, the longest iSTFT contraction

Clip 0 of a case is the tone recipe of tests/test_gpu_audio.py, the others are demo speech from sample 16000.  A window of 800
samples or more collects enough energy for that recipe (and for speech at 1024) to reach the 0 dB clip of the spectrogram, so at G4
and G5 the clips are scaled by 0.25, and by 0.125 in the T = 63 case, whose second of speech still reaches the clip at 0.25 (fp64
oracle: spec max 1.000 in demo clip 1); the helper asserts that nothing is clipped at the top."""
import pytest
import torch

import griffin_lim_ref as G
from test_gpu_backward import _dump
from test_gpu_loss_b64 import _audio_legs_per_clip, _clips

pytestmark = pytest.mark.gpu

#        tag, B, T, gain
CASES = [("G1", 3, 4, 1.0), ("G1", 2, 9, 1.0), ("G2", 3, 12, 1.0), ("G3", 2, 7, 1.0), ("G4", 3, 9, 0.25), ("G5", 2, 11, 0.25),
         ("G4", 3, 63, 0.125)]          # M = 189: more than one row tile of the contraction and no multiple of it


def clips(tag, B, T, gain):
    """[B, hop (T - 1)] float32: the tone recipe, then demo speech (the target clips 0 .. B - 2 from sample 16000)."""
    hop = G.GEOMETRIES[tag][1]
    S = hop * (T - 1)
    speech = torch.from_numpy(G._clips()[0][:B - 1, 16000:16000 + S]).float()
    return (torch.cat((_clips(1, S, 41, spread=False), speech)) * gain).contiguous()


@pytest.mark.parametrize("tag,B,T,gain", CASES, ids=[f"{t}-B{B}-T{T}" for t, B, T, _ in CASES])
def test_audio_legs_per_clip_at_other_geometries(tag, B, T, gain):
    n_fft, hop, win = G.GEOMETRIES[tag]
    cfg = {"n_fft": n_fft, "hop_length": hop, "win_length": win, "min_level_db": -100.0, "ref_level_db": 20.0}
    wav = clips(tag, B, T, gain)
    assert wav.shape == (B, hop * (T - 1)) and wav.shape[1] > n_fft // 2
    table, bad = _audio_legs_per_clip(wav, cfg, 35)
    _dump(f"stft_geometry_{tag}_B{B}_T{T}", table)
    for row in table:
        print(f"{tag} B{B} T{T}: " + "  ".join(f"{k} {v:.3g}" for k, v in row.items()))
    assert not bad, bad


def test_the_shortest_legal_clip_is_taken_and_one_sample_less_is_refused():
    """G1 at T = 4 has S = 33 = n_fft / 2 + 1 samples (the case above compares it); a clip of n_fft / 2 samples, which needs a
    second reflection, is refused by name."""
    from voicesplit_amd import _lib, audio
    cfg = {"n_fft": 64, "hop_length": 16, "win_length": 64, "min_level_db": -100.0, "ref_level_db": 20.0}
    with pytest.raises(_lib.VoiceSplitHipError, match="reflect padding"):
        audio.wav_to_spec(torch.rand(2, 32).cuda(), cfg)
    spec, phase = audio.wav_to_spec(torch.rand(2, 48).cuda(), cfg)
    assert spec.shape == phase.shape == (2, 4, 33) and torch.isfinite(spec).all() and torch.isfinite(phase).all()
