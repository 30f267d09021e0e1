"""One SHA-256 per case over the raw BiLSTM recurrences (csrc/lstm_fwd.hip, csrc/lstm_bwd.hip) where tools/forward_digest.py and
tools/backward_digest.py do not reach: every vs_set_lstm_kernel mode that launches kernels of its own (0, 1, 3, 4; mode 2 launches
what mode 0 does), the tape-writing forward, the BPTT and the carry form, in fp32, f16x3 and bf16, at the smallest shapes that reach
every branch of the kernels.  The recurrences have no atomics: two builds of the library that launch the same kernels print the same
lines, and so do two runs of one build.  Every tensor goes into the hash with its name, dtype and shape.  A refusal by the library is
that case's line (the error text, which carries the entry point, its return code and the library's message, is hashed), so two builds must
also refuse the same (mode, arithmetic, shape) combinations with the same words.

    python tools/lstm_digest.py [--lib path/to/libvoicesplit_hip.so] [--dump DIR] > digests.txt

--dump DIR keeps every case's tensors as DIR/<case>.npz."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (B, T, H): one chunk with an unowned upper half-chunk, no recurrent step | H % 16 == 8, fewer chunks than waves, T wraps the four
# exchange buffers | two batch tiles with 31 padding columns, wave 0 holds two chunks | past every resident limit (416 fp32 forward, 448 f16
# forward: the flag kernel serves it, 400 fp32 BPTT, 416 bf16 BPTT): every streaming tail loop runs
SHAPES = ((1, 1, 8), (2, 9, 40), (33, 6, 72), (3, 7, 456))
MODES = (0, 1, 3, 4)
MATHS = ("fp32", "f16x3", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--dump")
    args = ap.parse_args()
    from voicesplit_amd import _lib, ops
    lib = _lib.load(args.lib)

    def emit(case, fn):
        """fn() -> dict of tensors; a refusal of the library is hashed in their place"""
        try:
            arrays = {k: v.detach().cpu().numpy() for k, v in fn().items()}
        except _lib.VoiceSplitHipError as err:
            arrays = {"refused": np.frombuffer(str(err).encode(), dtype=np.uint8)}
        h = hashlib.sha256()
        for k in sorted(arrays):
            h.update(f"{k}:{arrays[k].dtype}:{arrays[k].shape}:".encode())
            h.update(arrays[k].tobytes())
        print(f"{h.hexdigest()}  {case}{'  (refused)' if 'refused' in arrays else ''}", flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            np.savez(os.path.join(args.dump, case.replace("/", "_") + ".npz"), **arrays)

    for B, T, H in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + 10 * T + H)
        xg = torch.randn(B, T, 8 * H, generator=g).cuda()
        w_f, w_b = ((torch.randn(4 * H, H, generator=g) * H ** -0.5).cuda() for _ in range(2))
        dout = torch.randn(B, T, 2 * H, generator=g).cuda()
        state = (torch.randn(B, 2, H, generator=g) * 0.5).cuda()
        name = f"B{B}T{T}H{H}"
        for math in MATHS:
            code = ops.MATH_CODES[math]
            for mode in MODES:
                assert lib.vs_set_lstm_kernel(mode) == 0
                tag = f"{name}/{math}/mode{mode}"
                emit(f"{tag}/recurrent", lambda: dict(out=ops.bilstm_recurrent(xg, w_f, w_b, math=code)))
                tape = {}

                def train():
                    tape.update(zip(("out", "gates", "c"), ops.bilstm_recurrent_train(xg, w_f, w_b, math=code)))
                    return tape
                emit(f"{tag}/recurrent_train", train)
                if tape:
                    emit(f"{tag}/recurrent_bwd", lambda: dict(dxg=ops.bilstm_recurrent_bwd(tape["gates"], tape["c"], dout, w_f, w_b, math=code)))
            lib.vs_set_lstm_kernel(0)
            for keep in sorted({1, (T + 1) // 2, T}):
                for start, st in (("zero", None), ("state", state)):
                    emit(f"{name}/{math}/carry/keep{keep}/{start}",
                         lambda: dict(zip(("out", "state"), ops.bilstm_recurrent_carry(xg, w_f, w_b, code, state=st, keep=keep))))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
