"""Cost of the reverberation leg on the device (voicesplit_amd/reverb.py, csrc/reverb.hip), one process, the arms alternating:

  (a) ``vs_fir_rows`` in VS_MATH_F16X3 (matrix cores) and in VS_MATH_FP32 (the cross-check arm) against
      ``torch.fft.irfft(rfft(x) * rfft(h))`` at B = 128 rows, L = 48000 samples, nh in {1024, 4096}: every row its own filter;
  (b) ``vs_rir_shoebox`` for 256 responses (128 drawn rooms) of 4096 taps;
  (c) one ``MixtureBatches`` batch of 64 three-second items from a synthetic pool, without and with a pool of drawn rooms
      (responses of 4096 taps, a drawn level), the front end included;
  (d) accuracy on the way: d_ref of the two fp64 image sums on the test rooms, the device's worst fraction of the response bound,
      and the worst fraction of each FIR bound on a slice of (a).

    python tools/reverb_time.py [--reps 20] [--out profiles/reverb_time.json]

Device events around the calls; 3 warm-ups per arm, then medians of --reps with [min, max] of the SAME arm.  The FIR and response
arms are the BARE library calls (outputs allocated once); the FFT arms are torch calls and allocate their results, and an arm of
a few tenths of a millisecond still holds the host's dispatch of its launches.  ``fft_cached_spectra`` keeps rfft(h), as a pool could.
A machine without a GPU fails: nothing here falls back.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000


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
    import reverb_ref as RR
    from mix_time import _event_ms, _stats
    import voicesplit_amd as V
    from voicesplit_amd import _lib, mixing, reverb
    from voicesplit_amd._call import ptr as _p, stream as _stream
    from voicesplit_amd.trainer import EpochShard
    if not torch.cuda.is_available():
        raise SystemExit("reverb_time.py measures the GPU: no device here")
    dev = torch.device("cuda:0")
    B, L = args.rows, args.samples
    gd = torch.Generator(device=dev).manual_seed(args.seed)
    x = torch.empty(B, L, device=dev).normal_(0.0, 0.05, generator=gd)
    at = torch.arange(B, dtype=torch.int64, device=dev) * L
    hrow = torch.arange(B, dtype=torch.int32, device=dev)
    arms, meta = {}, {}
    lib, stream = _lib.load(), _stream()
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    scale = torch.empty(B, 4, device=dev)
    for nh in (1024, 4096):
        decay = torch.exp(-torch.arange(nh, device=dev) / (nh / 6.0))
        h = (torch.empty(B, nh, device=dev).normal_(0.0, 1.0, generator=gd) * decay).contiguous()
        taps = torch.full((B,), nh, dtype=torch.int32, device=dev)
        out = torch.empty(B, L, device=dev)
        n_fft = 1 << (L + nh - 1).bit_length()

        def fir(math_name, h=h, taps=taps, out=out, nh=nh):                        # the bare library call: nothing allocated inside
            code = reverb.MATH[math_name]
            return lambda: _lib.check(lib.vs_fir_rows(_p(x), B * L, _p(at), _p(at), _p(taps), _p(hrow), B, L, _p(h), B, nh, code, _p(out),
                                                      _p(valid), _p(scale), stream), "vs_fir_rows")

        def fft(h=h, n_fft=n_fft):
            return torch.fft.irfft(torch.fft.rfft(x, n_fft) * torch.fft.rfft(h, n_fft), n_fft)[:, :L]

        Hf = torch.fft.rfft(h, n_fft)                                              # what a pool could keep: the filters' spectra

        def fft_cached(Hf=Hf, n_fft=n_fft):
            return torch.fft.irfft(torch.fft.rfft(x, n_fft) * Hf, n_fft)[:, :L]

        arms[f"fir_f16x3_nh{nh}"], arms[f"fir_fp32_nh{nh}"], arms[f"fft_nh{nh}"] = fir("f16x3"), fir("fp32"), fft
        arms[f"fft_cached_spectra_nh{nh}"] = fft_cached
        # accuracy of both arms on two rows of this shape, against np.convolve in fp64
        xs, hs = x[:2].cpu().numpy(), h[:2].cpu().numpy()
        for math_name in ("f16x3", "fp32"):
            y = reverb.fir_rows(x.reshape(-1), at[:2].contiguous(), at[:2].contiguous(), taps[:2].contiguous(), hrow[:2].contiguous(), h, L,
                                math_name)[0].cpu().numpy().astype(np.float64)
            worst = 0.0
            for b in range(2):
                ref, mag, mx, mh = RR.fir(xs.reshape(-1), b * L, b * L, L, hs[b], nh)
                bound, _ = RR.fir_bound(mag, nh, mx, mh, math_name)
                worst = max(worst, float((np.abs(y[b] - ref) / bound).max()))
            meta[f"fir_{math_name}_nh{nh}_worst_fraction_of_bound"] = round(worst, 4)
        yf = fft()[:2].cpu().numpy().astype(np.float64)
        ref = np.stack([RR.fir(xs.reshape(-1), b * L, b * L, L, hs[b], nh)[0] for b in range(2)])
        meta[f"fft_nh{nh}_max_abs_error"] = float(np.abs(yf - ref).max())
        meta[f"fft_nh{nh}_max_abs_output"] = float(np.abs(ref).max())

    # (b) 256 responses of 4096 taps
    rooms, _ = reverb.draw_rooms(128, torch.Generator().manual_seed(args.seed), nh=4096)
    structs = reverb.room_structs(rooms)
    room_table = torch.frombuffer(bytearray(ctypes.string_at(structs, ctypes.sizeof(structs))), dtype=torch.uint8).to(dev)
    hpool = torch.empty(256, 4096, device=dev)
    arms["rir_shoebox_256x4096"] = lambda: _lib.check(lib.vs_rir_shoebox(structs, _p(room_table), 256, 4096, _p(hpool), stream), "vs_rir_shoebox")
    arms["shoebox_rir_python_256x4096"] = lambda: reverb.shoebox_rir(rooms, dev)   # with the host loop over the table and its upload
    test_rooms = RR.gpu_test_rooms()
    d_abs, d_rel, href = RR.d_ref(test_rooms)
    got = reverb.shoebox_rir(torch.from_numpy(test_rooms), dev).cpu().numpy().astype(np.float64)
    meta["d_ref_abs"], meta["d_ref_rel_to_max_h"] = d_abs, d_rel
    meta["rir_worst_fraction_of_bound"] = round(max(float((np.abs(got[r, :len(ref)] - ref) / (64.0 * d_abs + 2.0 ** -24 * np.abs(ref))).max())
                                                    for r, ref in enumerate(href)), 4)

    # (c) one batch of 64 three-second mixtures, with and without rooms
    c = V.default_config()
    acfg = c.audio["voicefilter"] if "voicefilter" in c.audio else c.audio
    g = torch.Generator().manual_seed(args.seed)
    clips = [0.05 * torch.randn(int(n), generator=g) for n in torch.randint(4 * SR, 8 * SR, (96,), generator=g)]
    pool = mixing.ClipPool(clips, dev)
    triplets = [(k, (k + 1) % 96, (k + 7) % 96) for k in range(64)]
    audio_len = 3
    kept, _ = mixing.plan_triplets(pool, triplets, mixing.samples_for(acfg, audio_len))
    emb_table = torch.zeros(len(pool), 8, device=dev)
    shard = EpochShard(len(kept), len(kept), seed=0)
    rir = reverb.RirPool(32, dev, seed=args.seed, nh=4096)
    plain = mixing.MixtureBatches(pool, kept, emb_table, acfg, audio_len, shard, crop="random")
    roomy = mixing.MixtureBatches(pool, kept, emb_table, acfg, audio_len, shard, crop="random", rir_pool=rir, sir_db=(0.0, 10.0))
    order = [list(range(len(kept)))]
    arms["batch64_plain"] = lambda: list(plain.items(order, 0))
    arms["batch64_rooms_nh4096"] = lambda: list(roomy.items(order, 0))
    meta["batch_items"] = len(kept)

    ms = {k: [] for k in arms}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in arms.items():
            ms[name].append(_event_ms(fn))
    out = {"device": torch.cuda.get_device_name(0), "rows": B, "samples_per_row": L, "reps": args.reps, "warmups": 3}
    for k, v in ms.items():
        out[k + "_ms"] = _stats(v)
    for nh in (1024, 4096):
        med = lambda k: out[k + "_ms"]["median"]
        out[f"f16x3_over_fft_nh{nh}"] = round(med(f"fir_f16x3_nh{nh}") / med(f"fft_nh{nh}"), 3)
        out[f"f16x3_over_fft_cached_spectra_nh{nh}"] = round(med(f"fir_f16x3_nh{nh}") / med(f"fft_cached_spectra_nh{nh}"), 3)
        out[f"fp32_over_f16x3_nh{nh}"] = round(med(f"fir_fp32_nh{nh}") / med(f"fir_f16x3_nh{nh}"), 3)
        out[f"f16x3_nh{nh}_useful_TFLOPs"] = round(2.0 * B * L * nh / med(f"fir_f16x3_nh{nh}") / 1e9, 2)
    out["rooms_over_plain_batch"] = round(out["batch64_rooms_nh4096_ms"]["median"] / out["batch64_plain_ms"]["median"], 3)
    out.update(meta)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
