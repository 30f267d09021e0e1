"""GPU: the scratch registry of voicesplit_amd/_call.py behind the real calls.  One small call of every family fills its slot;
``ops.release_workspaces()`` empties all of them and torch's allocator gets the bytes back; the same calls then run again on
fresh buffers and still meet the bound their own tests hold them to (no bit equality is asked across the reallocation).

The shapes and the judges are the existing tests' own: the smoke dims for ``ops.forward`` (REL_TOL of tests/test_gpu_forward.py), G1
at B = 2, T = 4 -- the smallest STFT geometry -- for the audio legs (``_audio_legs_per_clip`` against the fp64 oracle, as
tests/test_gpu_stft_geometry.py runs it) and for ``losses.sisnr_loss`` (that case of tests/test_gpu_loss.py, called as it stands),
4 x 20000 demo rows for ``metrics.bss_sdr`` (``_agree`` of tests/test_gpu_sdr.py) and the 601-sample clip of
tests/test_gpu_speaker.py for ``speaker.logmel`` (its linear criterion and BOUND)."""
import pytest
import torch

import griffin_lim_ref as G
from oracle import reference_forward as R
from test_gpu_forward import REL_TOL, _rel
from test_gpu_loss import test_sisnr_loss_and_mask_gradient as sisnr_case
from test_gpu_loss_b64 import _audio_legs_per_clip
from test_gpu_sdr import _agree, _demo_batch
from test_gpu_speaker import AUDIO, BOUND, demo_wavs
from test_gpu_stft_geometry import clips

pytestmark = pytest.mark.gpu

DIMS = dict(num_freq=37, emb_dim=16, lstm_dim=24, fc1_dim=40, fc2_dim=37)


def _forward():
    from voicesplit_amd import ops
    sd = {k: v.cuda().contiguous() for k, v in R.build_state_dict(DIMS, 2).items()}
    x, dvec = (t.cuda() for t in R.synthetic_inputs(2, 40, DIMS, 2))
    dims = ops.make_dims(2, 40, *(DIMS[k] for k in ("num_freq", "emb_dim", "lstm_dim", "fc1_dim", "fc2_dim")))
    return lambda: ops.forward(sd, x, dvec, dims, "mish").cpu().numpy()


def _audio_legs():
    n_fft, hop, win = G.GEOMETRIES["G1"]
    cfg = {"n_fft": n_fft, "hop_length": hop, "win_length": win, "min_level_db": -100.0, "ref_level_db": 20.0}
    wav = clips("G1", 2, 4, 1.0)
    return lambda: _audio_legs_per_clip(wav, cfg, 35)[1]           # the rows that break the bounds: none


def _sdr():
    from voicesplit_amd import metrics
    ref, est = (torch.from_numpy(a).cuda() for a in _demo_batch(B=4, N=20000))      # scaled mixtures: SDR -2 .. 8 dB, _agree's absolute arm
    return lambda: metrics.bss_sdr(ref, est)[0].cpu().numpy()


def _logmel():
    from voicesplit_amd import speaker
    wav = demo_wavs()[0][16000:16000 + 601].contiguous().cuda()
    return lambda: 10.0 ** speaker.logmel(wav, AUDIO).double().cpu()


def test_release_returns_every_slot_and_the_calls_run_again():
    from voicesplit_amd import _call, ops
    ops.release_workspaces()
    forward, legs, sdr, logmel = _forward(), _audio_legs(), _sdr(), _logmel()
    sisnr = lambda: sisnr_case(2, 4, 64, 11, 64, None, 1.0)
    first = {"forward": forward(), "sdr": sdr(), "logmel": logmel()}
    assert legs() == []
    sisnr()
    held = {slot: t.numel() for (slot, _), t in _call._SCRATCH.items()}
    print("scratch held:", held)
    assert set(held) == {"model", "audio", "loss", "metric", "logmel"} and all(n > 0 for n in held.values())
    reported = _call.scratch_bytes()
    assert reported == sum(held.values()) == _call.scratch_bytes("cuda:0")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ops.release_workspaces()
    assert _call.scratch_bytes() == 0 and ops.tape_pool_bytes() == 0
    assert before - torch.cuda.memory_allocated() >= reported
    # again, on fresh buffers
    assert _rel(forward(), first["forward"]) < REL_TOL
    _agree(sdr(), first["sdr"], "sdr after release")
    again = logmel()
    assert ((again - first["logmel"]).abs().max() / first["logmel"].max()).item() <= BOUND
    assert legs() == []
    sisnr()
    assert _call.scratch_bytes() == reported
