"""One SHA-256 per case over what the host entry points around the short-time transform return (csrc/stft.hip and its callers
csrc/loss.hip, csrc/audio.hip, csrc/griffin_lim.hip and the log-mel front end of csrc/speaker.hip), at the smallest shapes that reach
every branch: ld padding columns (K = 18), an odd window (win % 4 != 0: the scalar-load GEMM instance), a window as wide as the frame,
the reference's geometry, and hop == win, which the envelope check refuses.  T = 2 is refused by the reflect-padding rule for most
geometries.  A refusal by the library is that case's line (the error text is hashed), so two builds must refuse the same cases with
the same words.  Every tensor goes into the hash with its name, dtype and shape.  The SI-SNR moments run in deterministic mode; the
only sums left to arrival order are Griffin-Lim's fp64 residuals where T * F > 256 (several workgroups per item), which is why
`wav` and `residual` are separate lines.  All inputs come from seeded CPU generators.

    python tools/audio_digest.py [--lib path/to/libvoicesplit_hip.so] [--dump DIR] > digests.txt

--dump DIR keeps every case's tensors as DIR/<case>.npz."""
import argparse
import hashlib
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRIES = ((16, 2, 8), (16, 2, 7), (64, 16, 64), (1200, 160, 400), (16, 8, 8))      # (n_fft, hop, win)
BATCHES = (1, 3)
FRAMES = (2, 9, 21)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--dump")
    args = ap.parse_args()
    from voicesplit_amd import _lib, audio, losses, speaker
    lib = _lib.load(args.lib)

    def emit(case, fn, split=False):
        """fn() -> dict of tensors; a refusal of the library is hashed in their place.  split: one line per tensor."""
        try:
            arrays = {k: v.detach().cpu().numpy() for k, v in fn().items()}
        except _lib.VoiceSplitHipError as err:
            arrays = {"refused": np.frombuffer(str(err).encode(), dtype=np.uint8)}
        groups = {f"{case}/{k}": {k: v} for k, v in arrays.items()} if split and "refused" not in arrays else {case: arrays}
        for name, group in groups.items():
            h = hashlib.sha256()
            for k in sorted(group):
                h.update(f"{k}:{group[k].dtype}:{group[k].shape}:".encode())
                h.update(group[k].tobytes())
            print(f"{h.hexdigest()}  {name}{'  (refused)' if 'refused' in group else ''}", flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            np.savez(os.path.join(args.dump, case.replace("/", "_") + ".npz"), **arrays)

    def sisnr(cfg, mask, mixed, target, phase, seq_len):
        m = mask.clone().requires_grad_(True)
        prev = _lib.set_option("DETERMINISTIC", 1)
        try:
            loss, wav = losses.sisnr_loss(m, mixed, target, phase, seq_len, cfg, return_wav=True)
            loss.backward()
        finally:
            _lib.set_option("DETERMINISTIC", prev)
        return dict(loss=loss, dmask=m.grad, wav=wav)

    def griffin_lim(cfg, spec, phase, n_iter, mode):
        _lib.check(lib.vs_set_griffin_lim_reframe(mode), "vs_set_griffin_lim_reframe")
        try:
            wav, res = audio.griffin_lim(spec, cfg, n_iter=n_iter, power=1.5, init_phase=phase, return_residual=True)
        finally:
            lib.vs_set_griffin_lim_reframe(0)
        return dict(wav=wav, residual=res)

    for n_fft, hop, win in GEOMETRIES:
        cfg = dict(n_fft=n_fft, hop_length=hop, win_length=win, min_level_db=-100.0, ref_level_db=20.0, sample_rate=16000)
        F = n_fft // 2 + 1
        geo = f"fft{n_fft}hop{hop}win{win}"
        for B in BATCHES:
            for T in FRAMES:
                g = torch.Generator().manual_seed(100000 * n_fft + 1000 * win + 100 * hop + 10 * T + B)
                wav = (0.1 * torch.randn(B, hop * (T - 1), generator=g)).cuda()
                spec, mask, target = (torch.rand(B, T, F, generator=g).cuda() for _ in range(3))
                phase = ((2.0 * torch.rand(B, T, F, generator=g) - 1.0) * math.pi).cuda()
                ragged = torch.tensor([max(1, hop * (T - 1) - 3 * b - 1) for b in range(B)], dtype=torch.int32)
                tag = f"{geo}/B{B}T{T}"
                emit(f"{tag}/wav_to_spec", lambda: dict(zip(("spec", "phase"), audio.wav_to_spec(wav, cfg))))
                emit(f"{tag}/spec_to_wav", lambda: dict(wav=audio.spec_to_wav(spec, phase, cfg)))
                emit(f"{tag}/spec_to_wav/mask", lambda: dict(wav=audio.spec_to_wav(spec, phase, cfg, mask=mask)))
                emit(f"{tag}/sisnr/full", lambda: sisnr(cfg, mask, spec, target, phase, None))
                emit(f"{tag}/sisnr/ragged", lambda: sisnr(cfg, mask, spec, target, phase, ragged))
                for n_iter in (0, 3):
                    for mode in (1, 2):
                        emit(f"{tag}/griffin_lim/iter{n_iter}/reframe{mode}", lambda: griffin_lim(cfg, spec, phase, n_iter, mode), split=True)
        # log-mel: the shortest legal clip, a multiple of hop, a non-multiple; the reference's geometry also at its odd length
        clips = [(n_fft // 2 + 1, 5), (hop * (n_fft // hop + 2), 5), (hop * (n_fft // hop + 2) + max(1, hop // 2), 5)]
        if (n_fft, hop, win) == (1200, 160, 400):
            clips.append((47917, 40))
        for n, rows in clips:
            g = torch.Generator().manual_seed(7 * n + rows + win)
            clip = (0.1 * torch.randn(n, generator=g)).cuda()
            emit(f"{geo}/logmel/n{n}mels{rows}", lambda: dict(mel=speaker.logmel(clip, cfg, rows)))

    g = torch.Generator().manual_seed(200)
    pm, px, pt = (torch.rand(200, generator=g).cuda() for _ in range(3))      # one workgroup

    def power_law():
        m = pm.clone().requires_grad_(True)
        loss = losses.power_law_loss(m, px, pt)
        loss.backward()
        return dict(loss=loss, dmask=m.grad)
    emit("powerlaw/n200", power_law)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
