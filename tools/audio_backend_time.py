"""Cost of the wavernn / waveglow audio back ends on the device (csrc/audio_codec.hip, voicesplit_amd/audio.py) at B = 64 clips of
3 s, one process, the arms of a group alternating, median of 20 with min and max:

  front end      the wavernn block (DBNORM codec, pre-emphasis 0.98; 2048 / 200 / 800 at 16 kHz) and the waveglow block (LOG codec;
                 1024 / 256 / 1024 at 22.05 kHz), each with and without its 80-band mel projection, against ``vs_wav_to_spec``
                 (the DB01 front end) at the same geometry: what codec, pre-emphasis and mel add
  de-emphasis    ``audio.deemphasis`` against ``torch.mul_`` over the same buffer (one HBM-bound read and write), and against
                 ``scipy.signal.lfilter`` in fp64 on ONE clip on the host
  Griffin-Lim    ``audio.griffin_lim_mag`` at 60 rounds, power 1.5, in both pad modes (waveglow geometry)

    python tools/audio_backend_time.py [--reps 20] [--out profiles/audio_backend_time.json]

Device events around whole calls; every arm is warmed up first.  A machine without a GPU fails: nothing here falls back.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SECONDS, N_ITER, POWER = 64, 3, 60, 1.5


def _stats(v, digits=4):
    import numpy as np
    return {"median": round(float(np.median(v)), digits), "min": round(float(np.min(v)), digits), "max": round(float(np.max(v)), digits)}


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(arms, reps):
    import torch
    for fn in arms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            ms[name].append(_event_ms(fn))
    return {k + "_ms": _stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.signal import lfilter
    from voicesplit_amd import audio, config
    if not torch.cuda.is_available():
        raise SystemExit("audio_backend_time.py measures the GPU: no device here")
    blocks = config.reference_audio_blocks()
    z = np.load(os.path.join(ROOT, "tests", "golden", "demo_clips.npz"))
    clips = torch.from_numpy(z["mixed"].astype(np.float32) / 32768.0)
    out = {"device": torch.cuda.get_device_name(0), "B": B, "seconds": SECONDS, "reps": args.reps}

    # ---- front ends
    for name in ("wavernn", "waveglow"):
        cfg = audio.resolve(blocks[name])
        hop = cfg["hop_length"]
        n = SECONDS * cfg["sample_rate"] // hop * hop
        wav = (0.25 * clips.repeat(B // 4, 2)[:, :n]).contiguous().cuda()          # the samples only fill the buffer: 3 s at either rate
        db01 = {k: cfg[k] for k in ("n_fft", "hop_length", "win_length", "sample_rate")}
        db01.update(min_level_db=-100.0, ref_level_db=20.0)
        arms = {"db01": lambda: audio.wav_to_spec(wav, db01), "codec": lambda: audio.wav_to_spec(wav, cfg),
                "codec_mel": lambda: audio.wav_to_spec(wav, dict(cfg, mel_spec=True))}
        r = _alternate(arms, args.reps)
        r.update(samples=n, frames=n // hop + 1, n_fft=cfg["n_fft"], hop=hop, win=cfg["win_length"],
                 codec_over_db01=round(r["codec_ms"]["median"] / r["db01_ms"]["median"], 3),
                 codec_mel_over_db01=round(r["codec_mel_ms"]["median"] / r["db01_ms"]["median"], 3))
        out["front_end_" + name] = r

    # ---- de-emphasis
    n = SECONDS * 16000
    x = (0.25 * clips.repeat(B // 4, 1)[:, :n]).contiguous().cuda()
    scratch = x.clone()
    r = _alternate({"deemphasis": lambda: audio.deemphasis(x, 0.98), "torch_mul_": lambda: scratch.mul_(1.0)}, args.reps)
    r["deemphasis_over_mul_"] = round(r["deemphasis_ms"]["median"] / r["torch_mul__ms"]["median"], 2)
    one = x[0].cpu().double().numpy()
    host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        lfilter([1], [1, -0.98], one)
        host.append((time.perf_counter() - t0) * 1e3)
    r["scipy_lfilter_one_clip_ms"] = _stats(host)
    r["samples"] = n
    out["deemphasis"] = r

    # ---- Griffin-Lim on a linear target, both pad modes
    cfg = audio.resolve(blocks["waveglow"])
    hop = cfg["hop_length"]
    n = SECONDS * cfg["sample_rate"] // hop * hop
    wav = (0.25 * clips.repeat(B // 4, 2)[:, :n]).contiguous().cuda()
    mag = audio.decode(audio.wav_to_spec(wav, cfg, want_phase=False)[0], cfg)
    angles = 2.0 * np.pi * torch.rand(mag.shape, generator=torch.Generator().manual_seed(B)).cuda()
    arms = {pad: (lambda pad=pad: audio.griffin_lim_mag(mag, cfg, n_iter=N_ITER, power=POWER, init_phase=angles, pad=pad))
            for pad in ("reflect", "zero")}
    r = _alternate(arms, args.reps)
    r.update(n_iter=N_ITER, power=POWER, frames=n // hop + 1, zero_over_reflect=round(r["zero_ms"]["median"] / r["reflect_ms"]["median"], 3))
    out["griffin_lim_mag"] = r

    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
