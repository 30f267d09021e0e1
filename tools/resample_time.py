"""Cost of sample-rate conversion on the device (csrc/resample.hip, voicesplit_amd/resample.py), one process, the arms of every
comparison alternating:

  (a) ``vs_resample_clips`` over a synthetic pool of about 10^4 clips of 3-15 s at 48000 -> 16000 and at 44100 -> 16000: clips/s and
      bytes/s of samples read plus written, beside the one-sweep figure of tools/stream_probe.hip (6.35 TB/s);
  (b) one chunk of ``audio.StreamingSeparatorAtRate`` at 48000 against the chunk of ``audio.StreamingSeparator`` at 16000 with the
      same C and R (profiles/stream_time.json holds the latter as measured before the resampler existed);
  (c) ``scipy.signal.resample_poly`` with the same taps on the host for ONE clip of 9 s, the only CPU yardstick at hand.

    python tools/resample_time.py [--reps 7] [--out profiles/resample_time.json]

Device events around whole arms (a), a host clock around arms that end in a synchronise (b) and around (c); every shape is warmed up
first; medians with the min / max over the repetitions of the SAME arm.  A machine without a GPU fails: nothing here falls back.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ONE_SWEEP_TBPS = 6.35                 # tools/stream_probe.hip: one sweep of short-lived workgroups, read + write


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--stream-seconds", type=float, default=8.0)
    ap.add_argument("--C", type=int, default=16)
    ap.add_argument("--R", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import voicesplit_amd as V
    from voicesplit_amd import audio
    from voicesplit_amd.resample import Resampler
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py measures the GPU: no device here")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "one_sweep_TBps_of_stream_probe": ONE_SWEEP_TBPS}

    # ---- (a) a pool of clips ---------------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(args.seed)
    seconds = 3.0 + 12.0 * torch.rand(args.clips, generator=g, dtype=torch.float64)
    pools = {}
    for sr in (48000, 44100):
        rs = Resampler(sr, 16000, dev)
        n_in = (seconds * sr).to(torch.int64)
        n_out = torch.tensor([rs.out_len(int(n)) for n in n_in], dtype=torch.int64)
        table = torch.stack((n_in.cumsum(0) - n_in, n_in, n_out.cumsum(0) - n_out), dim=1).contiguous()
        pools[sr] = dict(rs=rs, table=table, n_in=int(n_in.sum()), n_out=int(n_out.sum()))
    flat = torch.randn(max(p["n_in"] for p in pools.values()), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seed)) * 0.1
    dst = torch.empty(max(p["n_out"] for p in pools.values()), device=dev)
    arms = {sr: (lambda p=p: p["rs"].clips_into(flat[:p["n_in"]], dst[:p["n_out"]], p["table"])) for sr, p in pools.items()}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {sr: [] for sr in arms}
    for _ in range(args.reps):
        for sr, fn in arms.items():
            ms[sr].append(_event_ms(fn))
    a = {}
    for sr, p in pools.items():
        s = _stats(ms[sr])
        moved = 4 * (p["n_in"] + p["n_out"])
        d = p["rs"].dims
        a[f"{sr}_to_16000"] = {"clips": args.clips, "samples_in": p["n_in"], "samples_out": p["n_out"], "taps": d.T, "tile_periods": d.tile_periods,
                               "lds_bytes": d.lds_bytes, "ms": s, "clips_per_s": round(args.clips / s["median"] * 1e3),
                               "audio_hours_per_s": round(p["n_in"] / sr / 3600.0 / s["median"] * 1e3, 2),
                               "GBps_read_plus_written": round(moved / s["median"] / 1e6, 1),
                               "fraction_of_one_sweep": round(moved / s["median"] / 1e6 / (ONE_SWEEP_TBPS * 1e3), 4),
                               "Gtaps_per_s": round(p["n_out"] * d.T / s["median"] / 1e6, 1)}
    out["a_resample_clips"] = a
    del flat, dst, pools, arms
    torch.cuda.empty_cache()

    # ---- (b) one streamed chunk at 48000 against one at 16000 --------------------------------------------------------------------
    c = V.default_config()
    acfg = c.audio[c.audio["backend"]]
    hop = int(acfg["hop_length"])
    torch.manual_seed(args.seed)
    model = V.VoiceSplit(c).eval().to(dev)
    dvec = torch.randn(1, c.model["emb_dim"], device=dev)
    chunks = int(args.stream_seconds * 16000) // (args.C * hop)
    wav16 = torch.randn(1, chunks * args.C * hop, device=dev) * 0.05
    wav48 = torch.randn(1, 3 * chunks * args.C * hop, device=dev) * 0.05

    def stream(make, wav, step):
        def run():
            st = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(chunks):
                st.push(wav[:, k * step:(k + 1) * step])
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / chunks
        return run

    runs = {"separator_16000": stream(lambda: audio.StreamingSeparator(model, dvec, acfg, args.C, args.R), wav16, args.C * hop),
            "separator_at_48000": stream(lambda: audio.StreamingSeparatorAtRate(model, dvec, acfg, args.C, args.R, 48000), wav48,
                                         3 * args.C * hop)}
    for fn in runs.values():
        fn()
    bms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            bms[k].append(fn())
    b = {"C": args.C, "R": args.R, "chunk_audio_ms": 1e3 * args.C * hop / 16000, "chunks": chunks}
    b.update({k + "_ms_per_chunk": _stats(v) for k, v in bms.items()})
    b["resampling_cost_ms_per_chunk"] = round(b["separator_at_48000_ms_per_chunk"]["median"] - b["separator_16000_ms_per_chunk"]["median"], 4)
    b["per_rep_ms"] = [round(y - x, 4) for x, y in zip(bms["separator_16000"], bms["separator_at_48000"])]
    out["b_streamed_chunk"] = b

    # ---- (c) the host yardstick ------------------------------------------------------------------------------------------------------
    import resample_ref as RR
    from scipy.signal import resample_poly
    x = np.random.default_rng(args.seed).standard_normal(9 * 48000).astype(np.float32)
    fir = RR.fir(48000, 16000).astype(np.float32)
    resample_poly(x, 1, 3, window=fir)
    cms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        resample_poly(x, 1, 3, window=fir)
        cms.append(1e3 * (time.perf_counter() - t0))
    s = _stats(cms)
    out["c_scipy_resample_poly_one_9s_clip_48000_to_16000"] = {"ms": s, "clips_per_s": round(1e3 / s["median"], 1)}

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
