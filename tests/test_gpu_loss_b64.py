"""GPU: the SI-SNR loss head (vs_sisnr_loss) and the audio legs (vs_wav_to_spec, vs_spec_to_wav) at the batches bench.py and
evaluation run, against the fp64 oracles on the CPU (oracle/reference_loss.py with autograd, oracle/reference_audio.py), PER
UTTERANCE.  tests/test_gpu_loss.py and tests/test_gpu_audio.py stop at B <= 3: there every producer of a split-f16 operand
(spec_to_reim_kernel, overlap_add_bwd_kernel, stft_frames_kernel: one resident round of <= 2048 workgroups walking the tensor with a
grid-stride loop, each folding its |max| into the operand scale with vs_absmax_commit) makes exactly one pass, and the bounds are
relative to the batch's maximum, so a quiet utterance can be wrong by far more than its own size.  Here:

  1. the metric batch (B = 64 x 301 x 601, about 22 passes of spec_to_reim_kernel) with ragged seq_len and mixed*mask across the
     clamp at 1: loss, est_wav and d(loss)/d(mask) of every utterance against its own maximum;
  2. the same geometry with utterance levels spread over 2^0 .. 2^12 plus a near-silent one beside a saturated one, loudest first
     and quietest first (the batch-wide operand scale);
  3. smaller shapes whose producers take 2 .. 4 passes with a partial last one, rows M = B*T off the GEMM tile, a window with
     win % 4 != 0 (the GEMM's scalar-load instance) and an odd one;
  4. the audio legs at an evaluation batch (16 clips of 3 s) with the same level spread.

Bounds.  Where every utterance's operands sit near the batch's maximum, the bounds of test_gpu_loss.py hold per utterance: est_wav
to 2e-5 and dmask to 1e-4 of that utterance's own maximum.  Below that the batch-wide scale sets a floor, derived as follows.  A
split-f16 contraction (gemm_f16x3.hip, scheme in conv_f16x3.hip) multiplies each operand by s = 2^(10 - e), max|x| = f 2^e with
f in [0.5, 1), so max|x| s lies in [2^9, 2^10), and splits x s = hi + lo with both halves rounded toward zero to f16.  While lo is
a normal f16 number the split is exact to 2^-20 of |x s|; once it is subnormal the error is below the f16 subnormal spacing 2^-24,
which is 2^-24 / s <= 2^-33 max|x| in the operand's own units.  An utterance whose own operand maximum is rho times the batch's
therefore carries an absolute floor of 2^-33 / rho of its own maximum.  For rho >= 2^-10 that is at most 2^-23, one fp32 rounding
of the operand: the regime the bounds of test_gpu_loss.py were set in, so they apply unchanged.  Below 2^-10 the floor exceeds an
fp32 rounding by the factor 2^-10 / rho, and the contraction's output error, linear in its operands' errors, grows by at most that
factor:

    bound(rho) = bound_fp32 * max(1, 2^-10 / rho)

est_wav comes from one contraction (the estimate's iSTFT), so rho is that operand's.  dmask passes through all three (the two
iSTFTs feed the SI-SNR coefficients, then the transposed iSTFT of d(frames)), so rho is the smallest of the three; note that the
SI-SNR gradient scales as 1 / level, so in the backward contraction the QUIETEST estimate owns the batch's maximum.  rho is
computed from the fp64 oracle's own operands: mag * exp(cos / sin phase) of mixed*mask and of the target, and d(wav) / envelope.
Every loss-head test asserts this bound.  In sections 1 and 3 the estimate and target operands of every utterance lie within
2^-10 of their maxima (asserted), so est_wav is held to 2e-5 throughout; d(frames) does not: the few-sample utterances' gradients
are 2^7 .. 2^17 larger than the others', and dmask of the utterances they push below 2^-10 gets the floor-derived bound.

Conditioning.  The reference divides the sum of the UNMASKED target over the whole clip by seq_len, so for a few-sample seq_len
the gradient follows that sum.  Where it nearly cancels (0.39 from 48000 samples of about +-0.1), a systematic offset of one
fp32 rounding per sample moves d(loss)/d(mask) by more than 1e-4, and the split-f16 iSTFT's waveform carries a systematic
offset of that order (measured at B = 64: about 2^-25 of the target's maximum per sample, where an fp32 iSTFT's rounding errors
average out), which moved such an utterance's dmask by 2e-3.  _assert_loss_head therefore first asserts that the inputs are
well conditioned: an offset of 2^-24 of the target's maximum moves no utterance's gradient by more than DMASK_TOL / 4.
"""
import math

import numpy as np
import pytest
import torch

from oracle import reference_audio as RA
from oracle import reference_loss as RL
from test_gpu_backward import _dump

pytestmark = pytest.mark.gpu
GEOM = dict(n_fft=1200, hop_length=160, win_length=400)
AUDIO = {"n_fft": 1200, "hop_length": 160, "win_length": 400, "min_level_db": -100.0, "ref_level_db": 20.0}
WAV_TOL, DMASK_TOL = 2e-5, 1e-4              # test_gpu_loss.py's bounds, here per utterance
FLOOR_RHO = 2.0 ** -10                        # below this fraction of the batch's operand maximum the split's floor dominates
OCTAVE_V = math.log10(2.0) / 5.0              # mag = 10^(5 (v - 1) + 1): one octave of magnitude is 0.0602 of v = mixed*mask


def _off_the_kink(mixed, mask):
    """Keep mixed*mask out of (1 - 2e-6, 1 + 2e-6): the kernel forms the product in fp32, the oracle in fp64 (exactly), and the
    clamp's gradient jumps from its full value to 0 at 1, so a product within an fp32 rounding of 1 has no agreed gradient."""
    v = mixed.double() * mask.double()
    near = (v - 1.0).abs() < 2e-6
    mixed[near] = (mixed[near].double() * (1.0 - 4e-6) / v[near]).float()
    return mixed


def _ragged_lens(B, S, hop, few=True):
    """seq_len cycling through: = S, a multiple of hop, not a multiple of hop, a few samples, larger than S (the reference then
    divides by the given length but masks nothing).  few=False: no seq_len below S/2 (the few-sample kind becomes S - 1 - 13 b)."""
    nh = S // hop
    lo = 0 if few else nh // 2
    lens = []
    for b in range(B):
        r = b % 5
        if r == 0:
            lens.append(S)
        elif r == 1:
            lens.append(hop * (lo + 1 + (37 * b) % (nh - 1 - lo)))
        elif r == 2:
            lens.append(hop * (lo + (53 * b) % (nh - 1 - lo)) + 1 + (7 * b) % (hop - 1))
        elif r == 3:
            lens.append(5 + b % 7 if few else S - 1 - 13 * b)
        else:
            lens.append(S + 1 + 97 * b)
    return torch.tensor(lens)


def _random_case(B, T, F, seed, est_gain=1.0, tgt_gain=1.0, hot_every=4):
    """sigmoid(randn) masks; every `hot_every`-th utterance's mixed is scaled by 1.5, so mixed*mask crosses the clamp at 1."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.sigmoid(torch.randn(B, T, F, generator=g))
    gain = torch.full((B, 1, 1), est_gain)
    gain[::hot_every] *= 1.5
    mixed = _off_the_kink(torch.rand(B, T, F, generator=g) * gain, mask)
    target = torch.rand(B, T, F, generator=g) * tgt_gain
    phase = (torch.rand(B, T, F, generator=g) - 0.5) * 6.2
    return mask, mixed, target, phase


def _env(S, T, n_fft, hop, win):
    """sum over frames of the squared (non-periodic Hann) window at each output sample, fp64: frame t holds sample
    hop*t - n_fft/2 + (n_fft - win)//2 + j at window index j (istft, center=True, window centred in the frame)."""
    w = torch.hamming_window(win, periodic=False, alpha=0.5, beta=0.5, dtype=torch.float64)
    lead = n_fft // 2 - (n_fft - win) // 2
    env = torch.zeros(S + 2 * win, dtype=torch.float64)
    for t in range(T):
        a = hop * t - lead + win
        env[a:a + win] += w * w
    return env[win:win + S]


def _reim_max(v, phase):
    """per-utterance max of the iSTFT operand: mag * exp(cos phase), mag * exp(sin phase), mag from the clamped v (fp64)"""
    mag = torch.pow(10.0, ((v.double().clamp(0.0, 1.0) - 1.0) * 100.0 + 20.0) * 0.05)
    return (mag * torch.maximum(phase.double().cos(), phase.double().sin()).exp()).flatten(1).amax(1)


def _rho(x):
    return x / x.max()


def _bound(tol, rho):
    return tol * torch.clamp(FLOOR_RHO / rho, min=1.0)


def _offset_sensitivity(est_wav, tgt_wav, lens):
    """per utterance: how far d(loss)/d(est_wav) moves, relative to its maximum, when the target waveform is shifted by a
    constant 2^-24 of its own maximum (fp64).  The reference divides the UNMASKED target's sum by seq_len, so for a short
    seq_len the gradient follows the target's whole-clip sum; where that sum nearly cancels, a systematic offset of the
    order of one fp32 rounding per sample moves the gradient by more than DMASK_TOL."""
    def grad(s):
        e = est_wav.detach().clone().requires_grad_(True)
        RL.sisnr_with_pit(e.unsqueeze(1), s.unsqueeze(1), lens).backward()
        return e.grad
    g0 = grad(tgt_wav)
    g1 = grad(tgt_wav + 2.0 ** -24 * tgt_wav.abs().amax(1, keepdim=True))
    return (g1 - g0).abs().amax(1) / g0.abs().amax(1)


def _loss_head(mask, mixed, target, phase, lens, geom):
    """the kernel and the fp64 oracle on the same inputs -> per-utterance errors, bounds and the operand ratios"""
    from voicesplit_amd import losses
    B, T, F = mask.shape
    hop, win, n_fft = geom["hop_length"], geom["win_length"], geom["n_fft"]
    S = hop * (T - 1)
    md = mask.double().requires_grad_(True)
    ref_wav = RL.torch_spec2wav(mixed.double() * md, phase.double(), **geom)       # RL.training_loss, its target wav kept
    tgt_wav = RL.torch_spec2wav(target.double(), phase.double(), **geom)
    ref = RL.sisnr_with_pit(ref_wav.unsqueeze(1), tgt_wav.unsqueeze(1), lens)
    ref_wav.retain_grad()
    ref.backward()
    mc = mask.cuda().requires_grad_(True)
    loss, wav = losses.sisnr_loss(mc, mixed.cuda(), target.cuda(), phase.cuda(), lens.cuda(), geom, return_wav=True)
    loss.backward()
    torch.cuda.synchronize()
    wav, dmask = wav.detach().cpu().double(), mc.grad.cpu().double()
    ref_dwav, ref_wav, ref_dmask = ref_wav.grad, ref_wav.detach(), md.grad
    own_wav, own_dm = ref_wav.abs().amax(1), ref_dmask.flatten(1).abs().amax(1)
    assert (own_wav > 0).all() and (own_dm > 0).all()
    wav_err = (wav - ref_wav).abs().amax(1) / own_wav
    dm_err = (dmask - ref_dmask).flatten(1).abs().amax(1) / own_dm
    rho_e = _rho(_reim_max(mixed.double() * mask.double(), phase))
    rho_t = _rho(_reim_max(target, phase))
    rho_d = _rho((ref_dwav.abs() / _env(S, T, n_fft, hop, win)).amax(1))
    rho_g = torch.minimum(rho_e, torch.minimum(rho_t, rho_d))
    r = dict(loss=loss.item(), ref=ref.item(), wav_err=wav_err, wav_tol=_bound(WAV_TOL, rho_e), dm_err=dm_err,
             dm_tol=_bound(DMASK_TOL, rho_g), rho_e=rho_e, rho_t=rho_t, rho_d=rho_d, sens=_offset_sensitivity(ref_wav, tgt_wav, lens))
    keys = ("wav_err", "wav_tol", "dm_err", "dm_tol", "rho_e", "rho_t", "rho_d", "sens")
    r["table"] = {"loss": r["loss"], "loss_ref": r["ref"],
                  "per_utterance": [{k: float(r[k][b]) for k in keys} for b in range(B)],
                  "worst_wav_err": float(wav_err.max()), "worst_dm_err": float(dm_err.max()),
                  "worst_wav_ratio": float((wav_err / r["wav_tol"]).max()), "worst_dm_ratio": float((dm_err / r["dm_tol"]).max())}
    return r


def _assert_loss_head(r, lens=None):
    """the loss, and est_wav / dmask of every utterance within the bounds of the module docstring"""
    wav_tol, dm_tol = r["wav_tol"], r["dm_tol"]
    assert (r["sens"] <= DMASK_TOL / 4).all(), ("inputs not well conditioned", r["sens"].max().item(), int(r["sens"].argmax()))
    assert abs(r["loss"] - r["ref"]) < 2e-4 * max(1.0, abs(r["ref"])), (r["loss"], r["ref"])
    bad = (r["wav_err"] > wav_tol).nonzero().flatten().tolist()
    assert not bad, [(b, float(r["wav_err"][b]), float(wav_tol[b]), float(r["rho_e"][b])) for b in bad]
    bad = (r["dm_err"] > dm_tol).nonzero().flatten().tolist()
    assert not bad, [(b, None if lens is None else int(lens[b]), float(r["dm_err"][b]), float(dm_tol[b]),
                      float(r["rho_e"][b]), float(r["rho_t"][b]), float(r["rho_d"][b])) for b in bad]


# ---------------------------------------------------------------------------------------------
# 1. the metric batch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("few", [True, False])
def test_sisnr_loss_head_b64_ragged_per_utterance(few):
    """bench.py's loss head at B = 64 x 301 x 601: masks sigmoid(randn), every fourth utterance's mixed*mask across the clamp at 1,
    seq_len ragged over the batch.  Bounds per utterance, against its own maximum: test_gpu_loss.py's for est_wav (every
    estimate operand is within 2^-10 of the batch's maximum, asserted).  few: some seq_len are a few samples long; those
    utterances' gradients are 2^7 .. 2^17 larger than the others', so dmask of the rest gets the floor-derived bound.  Without
    them every operand of every contraction is within 2^-10 of its maximum (asserted) and all bounds are test_gpu_loss.py's:
    here the d(frames) operand is about 1e-5 .. 1e-4 in absolute terms, so it needs its power-of-two scale to stay in the f16
    normal range."""
    B, T, F = 64, 301, 601
    S = GEOM["hop_length"] * (T - 1)
    mask, mixed, target, phase = _random_case(B, T, F, 23 if few else 24)
    lens = _ragged_lens(B, S, GEOM["hop_length"], few)
    assert (mixed.double() * mask.double() > 1.0).any(dim=2).any(dim=1)[::4].all()
    r = _loss_head(mask, mixed, target, phase, lens, GEOM)
    _dump("loss_b64_ragged" + ("" if few else "_no_short"), dict(r["table"], seq_len=lens.tolist()))
    assert min(r["rho_e"].min(), r["rho_t"].min()) >= FLOOR_RHO
    if not few:
        assert r["rho_d"].min() >= FLOOR_RHO
    _assert_loss_head(r, lens)


# ---------------------------------------------------------------------------------------------
# 2. level spread inside one batch: the batch-wide operand scale
# ---------------------------------------------------------------------------------------------
def _level_case(B, T, F, seed):
    """mixed*mask of utterance b spans 2^4 below its top, the tops falling from the saturated utterance 0 (v up to 1.05: part of
    it above the clamp, mag 10) over 2^12 (utterance B - 2) to the near-silent utterance B - 1 (v in (0, 0.02]: mag 1e-4 ..
    1.26e-4, 2^-16.3 of the loudest).  The target's tops run over 2^0 .. 2^8 in a scrambled order (a different pattern)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.linspace(0.0, 12.0, B - 1)
    top = torch.cat([1.0 - OCTAVE_V * k, torch.tensor([0.02])])
    top[0] = 1.05
    span = torch.full((B,), 4 * OCTAVE_V)
    span[-1] = 0.02
    v = top[:, None, None] - span[:, None, None] * torch.rand(B, T, F, generator=g, dtype=torch.float64)
    mask = 0.5 + 0.5 * torch.rand(B, T, F, generator=g)
    mixed = _off_the_kink((v / mask.double()).float(), mask)
    kt = torch.tensor([8.0 * ((29 * b) % B) / (B - 1) for b in range(B)])
    vt = (0.95 - OCTAVE_V * kt)[:, None, None] - 4 * OCTAVE_V * torch.rand(B, T, F, generator=g, dtype=torch.float64)
    target = vt.float()
    phase = (torch.rand(B, T, F, generator=g) - 0.5) * 6.2
    return mask, mixed, target, phase


@pytest.mark.parametrize("order", ["loud_first", "quiet_first"])
def test_sisnr_loss_head_b64_level_spread(order):
    """B = 64 x 301 x 601 with levels 2^0 .. 2^12 apart and a near-silent utterance beside a saturated one (_level_case), loudest
    first, then quietest first (the order in which spec_to_reim_kernel's grid-stride passes meet them).  Bounds as derived in
    the module docstring: the per-utterance bounds of test_gpu_loss.py wherever rho >= 2^-10, scaled by 2^-10 / rho below."""
    B, T, F = 64, 301, 601
    S = GEOM["hop_length"] * (T - 1)
    mask, mixed, target, phase = _level_case(B, T, F, 22)
    if order == "quiet_first":
        mask, mixed, target, phase = (x.flip(0).contiguous() for x in (mask, mixed, target, phase))
    lens = torch.full((B,), S)
    r = _loss_head(mask, mixed, target, phase, lens, GEOM)
    _dump(f"loss_b64_levels_{order}", r["table"])
    loud, silent = (0, B - 1) if order == "loud_first" else (B - 1, 0)
    assert r["rho_e"][loud] == 1.0 and r["rho_e"][silent] < 2.0 ** -16
    assert (mixed[loud].double() * mask[loud].double() > 1.0).any()
    assert (r["rho_e"] >= FLOOR_RHO).sum() >= 3 * B // 4          # most of the batch is held to the fp32-class bounds
    _assert_loss_head(r)


# ---------------------------------------------------------------------------------------------
# 3. producer passes, ragged GEMM tiles, windows off the vector width
# ---------------------------------------------------------------------------------------------
def _passes(n):
    return -(-n // (2048 * 256))


@pytest.mark.parametrize("B,T,win,est_gain,seed", [
    (5, 301, 400, 0.25, 29),     # spec_to_reim 2 passes, overlap_add_bwd 2; M = 1505; the target 2^10 louder than the estimate
    (3, 1001, 400, 1.0, 26),     # spec_to_reim 4 passes, overlap_add_bwd 3; M = 3003
    (4, 401, 398, 1.0, 27),      # win % 4 != 0: the d(frames) contraction takes the GEMM's scalar-load instance; M = 1604
    (4, 401, 399, 1.0, 27),      # odd window: it starts at (n_fft - win) // 2 in the frame, so its centre is not win // 2
])
def test_sisnr_loss_head_multi_pass_shapes(B, T, win, est_gain, seed):
    """Checked like the metric batch."""
    F = GEOM["n_fft"] // 2 + 1
    geom = dict(GEOM, win_length=win)
    S = geom["hop_length"] * (T - 1)
    assert _passes(B * T * F) >= 2 and _passes(B * T * win) >= 2 and (B * T) % 128
    mask, mixed, target, phase = _random_case(B, T, F, seed, est_gain=est_gain)
    lens = _ragged_lens(B, S, geom["hop_length"])
    r = _loss_head(mask, mixed, target, phase, lens, geom)
    _dump(f"loss_b64_passes_{B}x{T}_win{win}", dict(r["table"], seq_len=lens.tolist()))
    assert min(r["rho_e"].min(), r["rho_t"].min()) >= FLOOR_RHO
    _assert_loss_head(r, lens)


# ---------------------------------------------------------------------------------------------
# 4. the audio legs at an evaluation batch
# ---------------------------------------------------------------------------------------------
def _clips(B, S, seed, spread=True):
    """B clips of tones + noise (test_gpu_audio.py's recipe, frequencies varied per clip).  spread: attenuated by 2^-k, k = 0 ..
    12 over the first B - 1 and 13.5 for the last: clip 0 peaks just below the 0 dB clip of the spectrogram (|STFT| = 10), the
    last sits near silence (|STFT| below 1e-3, its noise under the -100 dB floor)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(S, dtype=torch.float64) / 16000.0
    k = torch.cat([torch.linspace(0.0, 12.0, B - 1), torch.tensor([13.5])]) if spread else torch.zeros(B)
    out = []
    for b in range(B):
        x = sum(a * torch.sin(2 * np.pi * (f + 37.0 * b) * t + p + b)
                for a, f, p in [(0.08, 190.0, 0.1), (0.03, 1750.0, 1.0), (0.01, 5300.0, 2.0)])
        out.append((x + 0.004 * torch.randn(S, generator=g, dtype=torch.float64)) * 2.0 ** -float(k[b]))
    return torch.stack(out).float()


def _audio_legs_per_clip(wav, cfg, mask_seed):
    """vs_wav_to_spec, then vs_spec_to_wav with and without a mask, each clip against reference_audio: a table row per clip
    and the rows that break test_gpu_audio.py's bounds.  The phase is compared where the clip's own |STFT| is within 1e-2 of
    its maximum (a phase is only defined up to its bin's magnitude; test_gpu_audio.py's clips have no bins that weak at that
    threshold)."""
    from voicesplit_amd import audio
    B, S = wav.shape
    hop, win = cfg["hop_length"], cfg["win_length"]
    spec, phase = audio.wav_to_spec(wav.cuda(), cfg)
    mask = torch.rand(B, S // hop + 1, cfg["n_fft"] // 2 + 1, generator=torch.Generator().manual_seed(mask_seed)).cuda()
    out_m = audio.spec_to_wav(spec, phase, cfg, mask=mask).cpu().double().numpy()
    out_1 = audio.spec_to_wav(spec, phase, cfg).cpu().double().numpy()
    spec_c, phase_c, mask_c = spec.cpu(), phase.cpu(), mask.cpu()
    min_db, ref_db = float(cfg["min_level_db"]), float(cfg["ref_level_db"])
    lin = lambda s_: np.power(10.0, ((s_ - 1.0) * -min_db + ref_db) / 20.0)
    table, bad = [], []
    for b in range(B):
        x = wav[b].double().numpy()
        rs, rp = RA.wav2spec(x, cfg["n_fft"], hop, win, min_db, ref_db)
        mag = np.abs(RA.stft(x, cfg["n_fft"], hop, win)).T
        got_s, ph_b = spec_c[b].double().numpy(), phase_c[b].double().numpy()
        got, ref = lin(got_s), lin(rs)
        lin_ratio = (np.abs(got - ref) / (2e-5 * ref + 3e-6 * ref.max(axis=1, keepdims=True))).max()
        med = np.median(np.abs(got_s - rs))
        strong = mag > 1e-2 * mag.max()
        ph = np.abs(np.angle(np.exp(1j * (ph_b - rp))))[strong].max()
        ref_m = RA.spec2wav((spec_c[b] * mask_c[b]).double().numpy(), ph_b, hop, win, min_db, ref_db)
        ref_1 = RA.spec2wav(got_s, ph_b, hop, win, min_db, ref_db)
        em = np.abs(out_m[b] - ref_m).max() / np.abs(ref_m).max()
        e1 = np.abs(out_1[b] - ref_1).max() / np.abs(ref_1).max()
        row = dict(clip=b, spec_max=float(rs.max()), lin_ratio=float(lin_ratio), median=float(med), phase=float(ph),
                   spec2wav_mask=float(em), spec2wav=float(e1))
        table.append(row)
        if not (rs.max() < 1.0 and lin_ratio <= 1.0 and med < 1e-6 and ph < 1e-3 and em <= 2e-5 and e1 <= 2e-5):
            bad.append(row)
    return table, bad


@pytest.mark.parametrize("order", ["loud_first", "quiet_first"])
def test_audio_legs_b16_level_spread_per_clip(order):
    """vs_wav_to_spec and vs_spec_to_wav (with and without a mask) at B = 16 x 48000 (stft_frames_kernel 4 passes,
    spec_to_reim_kernel 6), each clip against reference_audio with test_gpu_audio.py's bounds applied to that clip alone."""
    B, S = 16, 48000
    wav = _clips(B, S, 31)
    if order == "quiet_first":
        wav = wav.flip(0).contiguous()
    loud, silent = (0, B - 1) if order == "loud_first" else (B - 1, 0)
    table, bad = _audio_legs_per_clip(wav, AUDIO, 32)
    _dump(f"loss_b64_audio_b16_{order}", table)
    assert table[loud]["spec_max"] > 0.97 and table[silent]["spec_max"] < 0.2
    assert not bad, bad


def test_audio_legs_odd_window_per_clip():
    """An odd window (win 399 starts at (n_fft - win) // 2 = 400 in the 1200-sample frame, so frame t spans samples
    hop*t - 200 .. hop*t + 198, not hop*t - 199 ..): both legs per clip against reference_audio, as above."""
    table, bad = _audio_legs_per_clip(_clips(3, 16000, 33, spread=False), dict(AUDIO, win_length=399), 34)
    _dump("loss_b64_audio_odd_window", table)
    assert not bad, bad
