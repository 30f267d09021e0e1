"""Writes tests/golden/sdr_bss_eval.npz: inputs and expected SDRs (dB) of single-source BSS-eval, the expected values from
the fp64 restatement tests/bss_eval_ref.py.

    python tools/make_sdr_golden.py          (needs the reference checkout: $VOICESPLIT_REFERENCE, see oracle/_refimport.py)

Contents (every row is a (reference, estimate) pair; rows of one group share a length):
  demo_clips_sdr [4]           the four (target, mixed) pairs of tests/golden/demo_clips.npz (data stays in that file);
  demo_ref / demo_est [4, L]   the reference's demo (clean = enhanced/, estimate = predict/ -- the output of the reference's
                               own trained model) pairs, samples 16000 .. 16000 + L, fp32; demo_sdr [4];
  syn{N}_ref / _est [R, N]     seeded synthetic rows for N in 1, 100, 511, 512, 513, 4000: white and band-limited noise
                               references, estimates that are filtered + noisy copies, a gain, and est = ref; syn{N}_sdr [R].
"""
import os
import sys

import numpy as np
from scipy.io import wavfile
from scipy.signal import lfilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bss_eval_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DEMO_NAMES = ["1701-141760-0023.251-136532-0023.wav", "2078-142845-0028.4153-186222-0000.wav",
              "3081-166546-0036.3170-137482-0042.wav", "6841-88291-0003.1585-157660-0013.wav"]
DEMO_LEN = 24000
SYN_LENGTHS = (1, 100, 511, 512, 513, 4000)


def synthetic_rows(n, rng):
    """Rows of length n: (white ref, filtered + noisy est), (band-limited ref, noisy est), (band-limited ref,
    heavily filtered est), (white ref, 0.3 * ref + small noise), (band-limited ref, est = ref)."""
    f32 = lambda x: x.astype(np.float32)
    white = rng.standard_normal(n)
    band = lfilter([1.0], [1.0, -1.6, 0.9], rng.standard_normal(n))          # resonant AR(2): strongly coloured spectrum
    fir = rng.standard_normal(24) * np.exp(-np.arange(24) / 6.0)
    rows = [(white, lfilter(fir, [1.0], white) + 0.1 * rng.standard_normal(n)),
            (band, band + 0.05 * np.std(band) * rng.standard_normal(n)),
            (band, lfilter([0.5, 0.3, -0.2], [1.0, -0.5], band) + 0.3 * np.std(band) * rng.standard_normal(n)),
            (white, 0.3 * white + 0.003 * rng.standard_normal(n)),
            (band, band)]
    ref = np.stack([f32(r) for r, _ in rows])
    est = np.stack([f32(e) for _, e in rows])
    est[4] = ref[4]                                                            # est = ref bit for bit
    return ref, est


def main():
    from oracle._refimport import REFERENCE_ROOT
    out = {}
    clips = np.load(os.path.join(GOLDEN, "demo_clips.npz"))
    tgt = clips["target"].astype(np.float32) / 32767.0
    mix = clips["mixed"].astype(np.float32) / 32767.0
    out["demo_clips_sdr"], st = R.sdr_rows(tgt, mix)
    assert not st.any()
    root = os.path.join(REFERENCE_ROOT, "datasets/LibriSpeech/audios_demo/2_speakers")
    refs, ests = [], []
    for n in DEMO_NAMES:
        sr, clean = wavfile.read(os.path.join(root, "enhanced", n))
        sr2, pred = wavfile.read(os.path.join(root, "predict", n))
        assert sr == sr2 == 16000 and clean.dtype == pred.dtype == np.float32
        refs.append(clean[16000:16000 + DEMO_LEN])
        ests.append(pred[16000:16000 + DEMO_LEN])
    out["demo_ref"], out["demo_est"] = np.stack(refs), np.stack(ests)
    out["demo_sdr"], st = R.sdr_rows(out["demo_ref"], out["demo_est"])
    assert not st.any()
    out["demo_source"] = np.array([f"datasets/LibriSpeech/audios_demo/2_speakers/{{enhanced,predict}}/{n}[16000:{16000 + DEMO_LEN}]"
                                   for n in DEMO_NAMES])
    rng = np.random.default_rng(20261015)
    for n in SYN_LENGTHS:
        ref, est = synthetic_rows(n, rng)
        out[f"syn{n}_ref"], out[f"syn{n}_est"] = ref, est
        out[f"syn{n}_sdr"], st = R.sdr_rows(ref, est)
        assert not st.any()
    out["syn_lengths"] = np.array(SYN_LENGTHS)
    p = os.path.join(GOLDEN, "sdr_bss_eval.npz")
    np.savez_compressed(p, **out)
    print(f"{p}: {os.path.getsize(p) / 1e3:.0f} kB")
    for k in sorted(out):
        if k.endswith("_sdr"):
            print(k, np.array2string(out[k], precision=4))


if __name__ == "__main__":
    main()
