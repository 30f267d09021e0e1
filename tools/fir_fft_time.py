"""Cost of the FFT form of the per-row FIR (voicesplit_amd/csrc/fir_fft.hip) against the direct form and against torch.fft, one
process, the arms alternating (the method of tools/reverb_time.py):

  B = 128 rows of 48000 samples, every row its own response, nh in {1024, 4096, 8192, 16384, 32768}:
    fir_fft_nh*              ``vs_fir_rows_fft`` with the spectra made beforehand (what a resident pool keeps)
    fir_f16x3_nh*            ``vs_fir_rows`` in VS_MATH_F16X3, up to its 8192 taps
    torch_fft_nh*            ``irfft(rfft(x) * rfft(h))`` in one transform of the next power of two
    torch_fft_cached_nh*     the same with rfft(h) kept
    fir_spectra_256_nh*      ``vs_fir_spectra`` for 256 responses of that length (once per pool and epoch)
  and the crossover between the two library arms: the smallest measured nh at which the FFT form is the faster one.

    python tools/fir_fft_time.py [--reps 20] [--out profiles/fir_fft_time.json]

Device events around the calls; 3 warm-ups per arm, then medians of --reps with [min, max] of the SAME arm.  The library arms are
the BARE calls (outputs, workspace and blob allocated once); the torch arms allocate their results.  Accuracy on the way: two rows
of every length against the fp64 sum, as a fraction of the header's bound at kappa = 1.  A machine without a GPU fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAPS = (1024, 4096, 8192, 16384, 32768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import fir_fft_ref as FR
    from mix_time import _event_ms, _stats
    from voicesplit_amd import _lib, reverb
    from voicesplit_amd._call import ptr as _p, stream as _stream
    if not torch.cuda.is_available():
        raise SystemExit("fir_fft_time.py measures the GPU: no device here")
    dev = torch.device("cuda:0")
    B, L = args.rows, args.samples
    gd = torch.Generator(device=dev).manual_seed(args.seed)
    x = torch.empty(B, L, device=dev).normal_(0.0, 0.05, generator=gd)
    at = torch.arange(B, dtype=torch.int64, device=dev) * L
    hrow = torch.arange(B, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    scale = torch.empty(B, 4, device=dev)
    out = torch.empty(B, L, device=dev)
    lib, stream = _lib.load(), _stream()
    arms, meta = {}, {}
    for nh in TAPS:
        decay = torch.exp(-torch.arange(nh, device=dev) / (nh / 6.0))
        h = (torch.empty(B, nh, device=dev).normal_(0.0, 1.0, generator=gd) * decay).contiguous()
        taps = torch.full((B,), nh, dtype=torch.int32, device=dev)
        sp = reverb.fir_spectra(h, taps.cpu(), taps)
        ws = torch.empty(lib.vs_fir_fft_workspace_bytes(B, L, nh), dtype=torch.uint8, device=dev)
        n_fft = 1 << (L + nh - 1).bit_length()

        def fft_form(sp=sp, ws=ws, nh=nh):
            return lambda: _lib.check(lib.vs_fir_rows_fft(_p(x), B * L, _p(at), _p(at), _p(hrow), B, L, _p(sp.blob), sp.blob.numel(), B, nh,
                                                          _p(ws), ws.numel(), _p(out), _p(valid), stream), "vs_fir_rows_fft")

        def direct(h=h, taps=taps, nh=nh):
            return lambda: _lib.check(lib.vs_fir_rows(_p(x), B * L, _p(at), _p(at), _p(taps), _p(hrow), B, L, _p(h), B, nh,
                                                      reverb.MATH["f16x3"], _p(out), _p(valid), _p(scale), stream), "vs_fir_rows")

        def torch_fft(h=h, n_fft=n_fft):
            return torch.fft.irfft(torch.fft.rfft(x, n_fft) * torch.fft.rfft(h, n_fft), n_fft)[:, :L]

        Hf = torch.fft.rfft(h, n_fft)

        def torch_fft_cached(Hf=Hf, n_fft=n_fft):
            return torch.fft.irfft(torch.fft.rfft(x, n_fft) * Hf, n_fft)[:, :L]

        # vs_fir_spectra for 256 responses: the table twice over
        h256 = h.repeat(-(-256 // B), 1)[:256].contiguous()
        taps256 = torch.full((256,), nh, dtype=torch.int32, device=dev)
        taps256_host = taps256.cpu()
        blob = torch.empty(lib.vs_fir_spectra_bytes(256, nh), dtype=torch.uint8, device=dev)

        def spectra(h256=h256, taps256=taps256, taps256_host=taps256_host, blob=blob, nh=nh):
            return lambda: _lib.check(lib.vs_fir_spectra(_p(h256), _p(taps256_host), _p(taps256), 256, nh, _p(blob), blob.numel(), stream),
                                      "vs_fir_spectra")

        arms[f"fir_fft_nh{nh}"] = fft_form()
        if nh <= reverb.MAX_TAPS:
            arms[f"fir_f16x3_nh{nh}"] = direct()
        arms[f"torch_fft_nh{nh}"], arms[f"torch_fft_cached_nh{nh}"] = torch_fft, torch_fft_cached
        arms[f"fir_spectra_256_nh{nh}"] = spectra()
        # accuracy: two rows against the fp64 sum
        y, _ = reverb.fir_rows_fft(x.reshape(-1), at[:2].contiguous(), at[:2].contiguous(), hrow[:2].contiguous(), sp, L)
        xs, hs, y = x[:2].cpu().numpy().reshape(-1), h[:2].cpu().numpy(), y.cpu().numpy()
        meta[f"fir_fft_nh{nh}_error_over_unit_bound"] = round(max(
            FR.ratio(y[b], FR.fir64(xs, b * L, b * L, L, hs[b], nh), FR.block_energy(xs, b * L, b * L, L, hs[b], nh), L, FR.BK) for b in range(2)), 5)

    ms = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in arms.items():
            ms[name].append(_event_ms(fn))
    res = {"device": torch.cuda.get_device_name(0), "rows": B, "samples_per_row": L, "reps": args.reps, "warmups": 3}
    for k, v in ms.items():
        res[k + "_ms"] = _stats(v)
    med = lambda k: res[k + "_ms"]["median"]
    crossover = None
    for nh in TAPS:
        res[f"fir_fft_over_torch_fft_cached_nh{nh}"] = round(med(f"fir_fft_nh{nh}") / med(f"torch_fft_cached_nh{nh}"), 3)
        res[f"fir_fft_over_torch_fft_nh{nh}"] = round(med(f"fir_fft_nh{nh}") / med(f"torch_fft_nh{nh}"), 3)
        if nh <= 8192:
            res[f"fir_fft_over_f16x3_nh{nh}"] = round(med(f"fir_fft_nh{nh}") / med(f"fir_f16x3_nh{nh}"), 3)
            if crossover is None and med(f"fir_fft_nh{nh}") < med(f"fir_f16x3_nh{nh}"):
                crossover = nh
    res["crossover_nh"] = crossover                      # None: the direct form wins at every length it takes
    res["kappa_ref"] = round(FR.kappa_ref(), 5)
    res.update(meta)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
