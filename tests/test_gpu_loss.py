"""GPU: the training-loop side of the mask (vs_sisnr_loss: mixed*mask -> iSTFT -> SI-SNR and its
gradient w.r.t. the mask) against the CPU oracle (oracle/reference_loss.py) in fp64."""
import numpy as np
import pytest
import torch

from oracle import reference_loss as RL

pytestmark = pytest.mark.gpu


def _case(B, T, n_fft, hop, win, seed, lens=None, mixed_gain=1.0):
    F = n_fft // 2 + 1
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(B, T, F, generator=g)
    mixed = torch.rand(B, T, F, generator=g) * mixed_gain
    target = torch.rand(B, T, F, generator=g)
    phase = (torch.rand(B, T, F, generator=g) - 0.5) * 6.2
    S = hop * (T - 1)
    lens = torch.tensor(lens) if lens is not None else torch.full((B,), S)
    return mask, mixed, target, phase, lens, dict(n_fft=n_fft, hop_length=hop, win_length=win)


@pytest.mark.parametrize("B,T,n_fft,hop,win,lens,gain", [
    (2, 9, 40, 8, 16, None, 1.0),
    (3, 12, 40, 8, 16, [88, 50, 70], 1.3),        # ragged lengths, some mixed*mask above the clamp
    (1, 5, 64, 16, 64, None, 1.0),                # window as wide as the frame
    (2, 21, 1200, 160, 400, [3200, 2500], 1.0),   # the reference's STFT geometry, short clip
    (2, 4, 64, 11, 64, None, 1.0),                # odd hop that does not divide the window (6 frames per sample); w[0] = w[63] = 0 under the envelope
    (2, 12, 402, 100, 200, [1100, 700], 1.3),     # n_fft = 2 (mod 4): K = 2 F = 404, no row padding; hop = win / 2
    (1, 7, 256, 64, 255, None, 1.0),              # odd window one short of the frame; win % 4 != 0
])
def test_sisnr_loss_and_mask_gradient(B, T, n_fft, hop, win, lens, gain):
    from voicesplit_amd import losses
    mask, mixed, target, phase, lens_t, audio = _case(B, T, n_fft, hop, win, 3, lens, gain)
    md = mask.double().requires_grad_(True)
    ref, ref_wav = RL.training_loss(md, mixed.double(), target.double(), phase.double(), lens_t, **audio)
    ref.backward()
    mc = mask.cuda().requires_grad_(True)
    loss, wav = losses.sisnr_loss(mc, mixed.cuda(), target.cuda(), phase.cuda(), lens_t.cuda(), audio, return_wav=True)
    loss.backward()
    assert abs(loss.item() - ref.item()) < 2e-4 * max(1.0, abs(ref.item()))
    assert (wav.cpu().double() - ref_wav.detach()).abs().max() <= 2e-5 * ref_wav.detach().abs().max()
    err = (mc.grad.cpu().double() - md.grad).abs().max() / md.grad.abs().max()
    assert err < 1e-4, err


def test_sisnr_loss_full_size_through_the_model():
    """One training step exactly as train.py:94-111 runs it (model -> mask -> loss -> backward ->
    Adam) at the reference's geometry (301 frames, n_fft 1200): finite, and the loss matches the
    oracle evaluated on the mask the model produced."""
    import voicesplit_amd as V
    from oracle import reference_forward as R
    from voicesplit_amd import losses
    B, T = 2, 301
    mask0, mixed, target, phase, lens_t, audio = _case(B, T, 1200, 160, 400, 5)
    m = V.VoiceSplit(V.default_config()).cuda().train()
    dvec = R.synthetic_inputs(B, T, R.default_dims(), 5)[1].cuda()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    mask = m(mixed.cuda(), dvec)
    loss = losses.sisnr_loss(mask, mixed.cuda(), target.cuda(), phase.cuda(), lens_t.cuda(), audio)
    ref, _ = RL.training_loss(mask.detach().cpu().double(), mixed.double(), target.double(), phase.double(), lens_t, **audio)
    assert abs(loss.item() - ref.item()) < 2e-4 * abs(ref.item())
    opt.zero_grad()
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    opt.step()


# ---------------------------------------------------------------------------------------------
# PowerLaw_Compressed_Loss (loss_name 'power_law_compression', the voicefilter configuration)
# ---------------------------------------------------------------------------------------------
def _rel(a, b):
    return (a.double().cpu() - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("power,ratio", [(0.3, 0.113), (0.5, 1.0)])
def test_powerlaw_loss_matches_upstream_golden(power, ratio):
    """Inputs, loss and d(loss)/d(mask) written by the upstream class (make_golden.py --powerlaw),
    exact-zero bins included.  fp32 kernel vs fp64 truth: 1e-5 on the loss, 2e-5 of the largest
    gradient entry (pow of fp32 operands; the oracle's own fp32 run sits at the same distance)."""
    import os
    from conftest import GOLDEN_DIR
    from voicesplit_amd import losses
    z = np.load(os.path.join(GOLDEN_DIR, "powerlaw_loss.npz"))
    tag = f"p{power}_r{ratio}"
    mixed, target = (torch.from_numpy(z[k]).float().cuda() for k in ("mixed", "target"))
    m = torch.from_numpy(z["mask"]).float().cuda().requires_grad_(True)
    loss = losses.power_law_loss(m, mixed, target, power, ratio)
    loss.backward()
    assert abs(loss.item() - float(z["loss/" + tag])) < 1e-5 * float(z["loss/" + tag])
    assert _rel(m.grad, torch.from_numpy(z["dmask/" + tag])) < 2e-5
    assert torch.isfinite(m.grad).all()


def test_powerlaw_loss_full_size_vs_oracle_and_through_the_model():
    """B=64 x 301 x 601 (BASELINE size): loss and gradient against the fp64 oracle on the CPU, then
    the voicefilter training graph end to end (model -> loss -> backward) once."""
    import voicesplit_amd as V
    from voicesplit_amd import losses
    g = torch.Generator().manual_seed(11)
    B, T, F = 64, 301, 601
    mixed = torch.rand(B, T, F, generator=g)
    target = mixed * torch.rand(B, T, F, generator=g)
    mask = torch.sigmoid(torch.randn(B, T, F, generator=g))
    md = mask.double().requires_grad_(True)
    ref = RL.training_loss_power_law(md, mixed.double(), target.double())
    ref.backward()
    mc = mask.cuda().requires_grad_(True)
    loss = losses.power_law_loss(mc, mixed.cuda(), target.cuda())
    loss.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * ref.item()
    assert _rel(mc.grad, md.grad) < 2e-5
    # scaling the upstream gradient scales dmask (autograd.Function.backward)
    mc2 = mask.cuda().requires_grad_(True)
    (3.0 * losses.power_law_loss(mc2, mixed.cuda(), target.cuda())).backward()
    assert torch.allclose(mc2.grad, 3.0 * mc.grad, rtol=1e-6, atol=0)
    del mc, mc2, md
    torch.manual_seed(0)
    model = V.VoiceFilter(V.default_config()).cuda().train()
    d = torch.randn(B, 256, generator=g)
    d = (d / d.norm(dim=1, keepdim=True)).cuda()
    out = model(mixed.cuda(), d)
    l2 = losses.power_law_loss(out, mixed.cuda(), target.cuda())
    l2.backward()
    assert torch.isfinite(l2).item()
    assert all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in model.parameters())
