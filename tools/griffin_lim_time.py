"""Cost of Griffin-Lim on the device (vs_griffin_lim, voicesplit_amd/audio.py): 3 s clips (T = 301 frames), 60 iterations,
power 1, at B = 1 and B = 64, one process, the arms alternating:

  resident        ``audio.griffin_lim`` = one vs_griffin_lim call, in the library's default re-framing form;
  two_kernel      the same with vs_set_griffin_lim_reframe(1): overlap-add, then framing, through the waveform (6 launches a round);
  gather          the same with vs_set_griffin_lim_reframe(2): one gather launch from frames to frames (5 launches a round);
  composed        the loop a caller could already write from the public calls, ``spec_to_wav(S, phase)`` ->
                  ``wav_to_spec(wav)`` -> take its phase -> repeat: the baseline (it needs nothing of vs_griffin_lim);
  resident_0_iter vs_griffin_lim with n_iter = 0: what a call costs outside its loop.

    python tools/griffin_lim_time.py [--reps 9] [--out profiles/griffin_lim_time.json]

Device events around whole calls; every arm is warmed up first; medians with the min / max over the repetitions of the SAME arm.
The spectrograms are those of the four demo mixtures of tests/golden/demo_clips.npz (repeated to fill the batch), the starting
angles uniform.  A machine without a GPU fails: nothing here falls back.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N_ITER, POWER = 301, 60, 1.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import voicesplit_amd as V
    from voicesplit_amd import _lib, audio
    if not torch.cuda.is_available():
        raise SystemExit("griffin_lim_time.py measures the GPU: no device here")
    lib = _lib.load()
    c = V.default_config()
    acfg = c.audio[c.audio["backend"]]
    z = np.load(os.path.join(ROOT, "tests", "golden", "demo_clips.npz"))
    clips = torch.from_numpy(z["mixed"].astype(np.float32) / 32768.0)
    out = {"device": torch.cuda.get_device_name(0), "T": T, "n_iter": N_ITER, "power": POWER, "reps": args.reps, "batches": {}}

    for B in args.batches:
        wav = clips.repeat((B + 3) // 4, 1)[:B, :160 * (T - 1)].contiguous().cuda()
        spec, _ = audio.wav_to_spec(wav, acfg)
        angles = 2.0 * np.pi * torch.rand(spec.shape, generator=torch.Generator().manual_seed(B)).cuda()

        def resident(mode, n_iter=N_ITER):
            def run():
                _lib.check(lib.vs_set_griffin_lim_reframe(mode), "vs_set_griffin_lim_reframe")
                return audio.griffin_lim(spec, acfg, n_iter=n_iter, power=POWER, init_phase=angles)
            return run

        def composed():
            y = audio.spec_to_wav(spec, angles, acfg)
            for _ in range(N_ITER):
                _, phase = audio.wav_to_spec(y, acfg)
                y = audio.spec_to_wav(spec, phase, acfg)
            return y

        arms = {"resident": resident(0), "two_kernel": resident(1), "gather": resident(2), "composed": composed,
                "resident_0_iter": resident(0, 0)}
        ms = {k: [] for k in arms}
        ys = {}
        for name, fn in arms.items():
            fn()
            ys[name] = fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in arms.items():
                ms[name].append(_event_ms(fn))
        lib.vs_set_griffin_lim_reframe(0)
        r = {k + "_ms": _stats(v) for k, v in ms.items()}
        base = r["resident_0_iter_ms"]["median"]
        for k in ("resident", "two_kernel", "gather"):
            r[k + "_ms_per_iteration"] = round((r[k + "_ms"]["median"] - base) / N_ITER, 5)
        r["composed_ms_per_iteration"] = round(r["composed_ms"]["median"] / (N_ITER + 1), 5)
        r["composed_over_resident"] = round(r["composed_ms"]["median"] / r["resident_ms"]["median"], 2)
        r["two_kernel_over_gather"] = round(r["two_kernel_ms"]["median"] / r["gather_ms"]["median"], 3)
        r["launches_per_iteration"] = {"two_kernel": 6, "gather": 5}
        # the arms compute the same thing: both resident forms to the bit, the composed loop up to its phase round trip
        r["resident_forms_bit_identical"] = bool(torch.equal(ys["two_kernel"], ys["gather"]) and torch.equal(ys["resident"], ys["gather"]))
        r["composed_vs_resident_max_rel"] = float((ys["composed"] - ys["resident"]).abs().max() / ys["resident"].abs().max())
        out["batches"][str(B)] = r

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
