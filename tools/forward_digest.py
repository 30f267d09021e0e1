"""One SHA-256 per case over every entry point of the tape-less forward (whole path and stages, every arithmetic that serves the
entry, both activations, FEAT_ROWS on and off where cnn8 may write the GEMM operand): two builds of the library that print the same
lines launch the same kernels on the same operands.  Train-mode cases also digest the running statistics they leave behind.

    python tools/forward_digest.py [--lib path/to/libvoicesplit_hip.so] [--dump DIR] > digests.txt

--dump DIR keeps every case's tensors as DIR/<case>.npz (for cases whose digest differs between two runs of ONE build: the
double-precision atomics of the batch statistics are unordered)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import reference_forward as R  # noqa: E402

SMALL = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
KPAD = dict(num_freq=16, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=16)       # 8 F = 128 rows of K, padded to the GEMM's block
# (dims, B, T): a clip too short for the unprepared operand copies, several blocks, K padding, the config.json sizes
SHAPES = (("small", SMALL, 1, 5), ("small", SMALL, 3, 45), ("kpad", KPAD, 2, 40), ("full", R.default_dims(), 1, 20))
LENGTHS = [45, 17, 1]      # for the (3, 45) shape
K_SPEAKERS = 3
CHANNELS_LAST = ("f16x3", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--dump")
    args = ap.parse_args()
    from voicesplit_amd import _lib, ops
    _lib.load(args.lib)

    def emit(case, tensors):
        h = hashlib.sha256()
        arrays = {k: v.detach().cpu().numpy() for k, v in tensors.items()}
        for k in sorted(arrays):
            h.update(arrays[k].tobytes())
        print(f"{h.hexdigest()}  {case}", flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            np.savez(os.path.join(args.dump, case.replace("/", "_") + ".npz"), **arrays)

    def with_stats(out, sd):
        return dict(out=out, **{k: v for k, v in sd.items() if "running_" in k})

    for tag, dd, B, T in SHAPES:
        sd0 = R.spread_logits(R.build_state_dict(dd, 21), 6.0)
        x, dvec = (t.cuda() for t in R.synthetic_inputs(B, T, dd, 21))
        g = torch.Generator().manual_seed(5)
        dvecs = torch.randn(B, K_SPEAKERS, dd["emb_dim"], generator=g).cuda()
        feat = torch.randn(B, T, 8 * dd["num_freq"], generator=g).cuda()
        lstm_out = torch.randn(B, T, 2 * dd["lstm_dim"], generator=g).cuda()
        lengths = (None, LENGTHS) if (B, T) == (3, 45) else (None,)
        for math in ("fp32", "f16x3", "bf16"):
            dims = ops.make_dims(B, T, dd["num_freq"], dd["emb_dim"], dd["lstm_dim"], dd["fc1_dim"], dd["fc2_dim"], math=math)
            ragged = tuple(le for le in lengths if le is None or math in CHANNELS_LAST)
            fresh = lambda: {k: v.clone().cuda() for k, v in sd0.items()}       # noqa: E731  (train mode moves the running statistics)
            sd = fresh()
            name = f"{tag}/B{B}T{T}/{math}"
            for act in ("mish", "relu"):
                for rows in ((1, 0) if math in CHANNELS_LAST else (1,)):
                    _lib.set_option("FEAT_ROWS", rows)
                    emit(f"{name}/{act}/rows{rows}/forward", dict(out=ops.forward(sd, x, dvec, dims, act)))
                    prep = ops.PreparedWeights(sd, dims)
                    for le in ragged:
                        emit(f"{name}/{act}/rows{rows}/forward_prepared/len{int(le is not None)}",
                             dict(out=ops.forward_prepared(sd, prep, x, dvec, dims, act, lengths=le)))
                        if math in CHANNELS_LAST:
                            emit(f"{name}/{act}/rows{rows}/forward_prepared_multi/len{int(le is not None)}",
                                 dict(out=ops.forward_prepared_multi(sd, prep, x, dvecs, dims, act, lengths=le)))
                _lib.set_option("FEAT_ROWS", 1)
                for le in ragged:
                    emit(f"{name}/{act}/conv_stack/len{int(le is not None)}", dict(out=ops.conv_stack(sd, x, dims, act, lengths=le)))
                t = fresh()
                emit(f"{name}/{act}/forward_train", with_stats(ops.forward(t, x, dvec, dims, act, training=True), t))
                t = fresh()
                emit(f"{name}/{act}/conv_stack_train", with_stats(ops.conv_stack(t, x, dims, act, training=True), t))
            for le in ragged:
                emit(f"{name}/bilstm/len{int(le is not None)}", dict(out=ops.bilstm(sd, feat, dvec, dims, lengths=le)))
                if math in CHANNELS_LAST:
                    emit(f"{name}/bilstm_multi/len{int(le is not None)}", dict(out=ops.bilstm_multi(sd, feat, dvecs, dims, lengths=le)))
            mask, logits = ops.head(sd, lstm_out, dims, want_logits=True)
            emit(f"{name}/head", dict(mask=mask, logits=logits))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
