#!/usr/bin/env python3
"""Times the GE2E speaker encoder at full size (40 / 768 / 3 / 256 / 80 / 40) for N in {6, 64, 1024} windows, one process.

Arm A (this library): "rec" = vs_speaker_embed up to h_last (layer-0 input projection + the stacked recurrence);
"e2e" = logmel of every clip + recurrence + projection + pooling (SpeakerEncoder.embed_many).
Arm B (what the reference notebook runs on its GPU): torch.nn.LSTM(40, 768, 3) in fp32 on the unfolded windows + Linear,
under no_grad.  The arms alternate inside the call; every timed block is device events around warmed-up repetitions.

    python tools/speaker_time.py [--out profiles/speaker_encoder_timing.json] [--rounds 5]"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AUDIO = {"n_fft": 1200, "num_freq": 601, "sample_rate": 16000, "hop_length": 160, "win_length": 400,
         "min_level_db": -100.0, "ref_level_db": 20.0}
CASES = {6: (1, 301), 64: (8, 361), 1024: (64, 681)}        # N windows: (clips, frames per clip)
FLOP_PER_WINDOW = 80 * 2 * (808 + 1536 + 1536) * 3072 + 2 * 768 * 256


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speaker_encoder_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-ms", type=float, default=300.0)
    args = ap.parse_args()
    import voicesplit_amd as V
    from voicesplit_amd import _call
    dev = "cuda:0"
    torch.manual_seed(0)
    enc = V.SpeakerEncoder().eval().to(dev)
    ref_lstm = torch.nn.LSTM(40, 768, num_layers=3, batch_first=True).to(dev).eval()
    ref_lin = torch.nn.Linear(768, 256).to(dev).eval()
    ref_lstm.load_state_dict({k[5:]: v for k, v in enc.state_dict().items() if k.startswith("lstm.")})
    result = {"device": torch.cuda.get_device_name(0), "flop_per_window": FLOP_PER_WINDOW, "cases": {}}
    arm_b_error = None
    for N, (U, T) in CASES.items():
        g = torch.Generator().manual_seed(N)
        wavs = [(torch.rand(160 * (T - 1), generator=g) * 0.2 - 0.1).to(dev) for _ in range(U)]
        mels = [V.logmel(w, AUDIO) for w in wavs]
        mel = torch.cat(mels, dim=1).contiguous()
        d = enc._dims()
        prepared = enc._prepare(torch.device(dev))
        frames = [u * T for u in range(U + 1)]
        wins = [u * (N // U) for u in range(U + 1)]
        offs = torch.tensor([frames, wins], dtype=torch.int32, device=dev)
        ws = _call.scratch("embed", _call.sized("speaker_workspace_bytes", ctypes.byref(d), N, U * T), dev)
        h_last = torch.empty(N, 768, device=dev)

        def rec():
            _call.call("speaker_embed", dev, ctypes.byref(d), prepared, prepared.numel(), mel, U * T, offs[0], offs[1], U, N,
                       h_last, None, None, ws, ws.numel())

        def e2e():
            enc.embed_many([V.logmel(w, AUDIO) for w in wavs])

        def arm_b():
            with torch.no_grad():
                x = mel.view(40, U, T).permute(1, 0, 2).unfold(2, 80, 40)            # [U, 40, n, 80]
                x = x.permute(0, 2, 3, 1).reshape(N, 80, 40)
                ref_lin(ref_lstm(x)[0][:, -1, :])

        arms = {"A_rec": rec, "A_e2e": e2e}
        if arm_b_error is None:
            try:
                arm_b()
                torch.cuda.synchronize()
                arms["B_torch_lstm"] = arm_b
            except Exception as err:          # MIOpen's RNN path missing or failing: said once, not retried
                arm_b_error = f"{type(err).__name__}: {err}"
        reps = {}
        for name, fn in arms.items():
            fn(); fn()
            torch.cuda.synchronize()
            ms = timed(fn, 3)
            reps[name] = max(3, min(400, math.ceil(args.block_ms / max(ms, 1e-3))))
        samples = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                samples[name].append(timed(fn, reps[name]))
        case = {"clips": U, "frames_per_clip": T, "reps": reps}
        for name, s in samples.items():
            s = sorted(s)
            case[name] = {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1]}
        med = case["A_rec"]["median_ms"]
        case["A_rec_tflops"] = N * FLOP_PER_WINDOW / med / 1e9
        case["A_rec_us_per_tick"] = med * 1e3 / 82
        result["cases"][str(N)] = case
        print(json.dumps({str(N): case}))
    result["arm_b_error"] = arm_b_error
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
