"""One SHA-256 per case over the backward kernels of the NCHW fp32 layouts (csrc/conv_bwd.hip, csrc/wgrad_f16x3.hip) at the
shapes of tests/test_gpu_backward.py, and over every gradient of one small training step: two builds of the library that print
the same lines launch the same kernels on the same operands.  The 64->64 weight gradient runs in fp32 and in split-f16
arithmetic under every vs_set_wgrad_kernel mode (0 auto, 1 eight-wave ring, 2 kt-split, 3 four-wave ring).

    python tools/backward_digest.py [--lib path/to/libvoicesplit_hip.so] [--dump DIR] > digests.txt

--dump DIR keeps every case's tensors as DIR/<case>.npz (for cases whose digest differs between two runs of ONE build: the
double-precision atomics of the BatchNorm backward sums and of cnn1's weight gradient are unordered)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import reference_forward as R  # noqa: E402

SMALL = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)
# (KT, KF, dil, B, T, F): CONV_BWD_CASES of tests/test_gpu_backward.py
CONV_BWD_CASES = [(7, 1, 1, 2, 19, 37), (5, 5, 1, 2, 19, 37), (5, 5, 2, 1, 23, 70), (5, 5, 4, 2, 21, 133), (5, 5, 8, 1, 50, 64),
                  (5, 5, 16, 2, 40, 31), (5, 5, 16, 1, 20, 37), (5, 5, 1, 1, 1, 5), (7, 1, 1, 1, 8, 601), (5, 5, 2, 3, 9, 601),
                  (5, 5, 1, 1, 70, 37), (7, 1, 1, 2, 100, 64)]
BN_SHAPES = [(3, 11, 37, 0), (2, 33, 301, 0), (2, 33, 301, 1)]       # (B, T, F, skew) of test_bn_act_backward
BN_FIRST_SHAPES = [(3, 11, 37), (2, 33, 301), (1, 2, 5)]


def bn_consts(z, g, training):
    """scale, shift, mean, invstd of a BatchNorm over z [B, C, T, F] (batch or made-up running statistics), as the tests form them"""
    C = z.shape[1]
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rmean, rvar = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    if training:
        mean, var = z.double().mean(dim=(0, 2, 3)), z.double().var(dim=(0, 2, 3), unbiased=False)
    else:
        mean, var = rmean.double(), rvar.double()
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = gamma.double() * invstd
    return [t.float().cuda() for t in (scale, beta.double() - mean * scale, mean, invstd)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--dump")
    args = ap.parse_args()
    from voicesplit_amd import _lib, ops
    lib = _lib.load(args.lib)

    def emit(case, tensors):
        h = hashlib.sha256()
        arrays = {k: v.detach().cpu().numpy() for k, v in tensors.items()}
        for k in sorted(arrays):
            h.update(arrays[k].tobytes())
        print(f"{h.hexdigest()}  {case}", flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            np.savez(os.path.join(args.dump, case.replace("/", "_") + ".npz"), **arrays)

    for KT, KF, dil, B, T, Fq in CONV_BWD_CASES:
        g = torch.Generator().manual_seed(KT * 1000 + dil * 10 + B)
        x = torch.randn(B, 64, T, Fq, generator=g).cuda()
        w = (torch.randn(64, 64, KT, KF, generator=g) * (1.0 / (64 * KT * KF) ** 0.5)).cuda()
        dz = torch.randn(B, 64, T, Fq, generator=g).cuda()
        name = f"conv64/{KT}x{KF}d{dil}/B{B}T{T}F{Fq}"
        for math in ("fp32", "f16x3"):
            emit(f"{name}/dgrad/{math}", dict(dx=ops.conv64_dgrad(dz, w, dil, math=math)))
        emit(f"{name}/wgrad/fp32", dict(dw=ops.conv64_wgrad(dz, x, KT, KF, dil, math="fp32")))
        for mode in (0, 1, 2, 3):
            assert lib.vs_set_wgrad_kernel(mode) == 0
            emit(f"{name}/wgrad/f16x3/mode{mode}", dict(dw=ops.conv64_wgrad(dz, x, KT, KF, dil, math="f16x3")))
        lib.vs_set_wgrad_kernel(0)

    for B, T, Fq, skew in BN_SHAPES:
        for layout, C in (("nchw", 64), ("feat", 8)):
            for act in ("mish", "relu"):
                for training in (True, False):
                    g = torch.Generator().manual_seed(7)
                    z = torch.randn(B, C, T, Fq, generator=g) * 1.5 + 0.3
                    da = torch.randn(B, C, T, Fq, generator=g)
                    consts = bn_consts(z, g, training)
                    if layout == "feat":      # [B][T][8][F]
                        z, da = z.permute(0, 2, 1, 3).contiguous(), da.permute(0, 2, 1, 3).contiguous()
                    L = Fq if layout == "feat" else T * Fq
                    buf = torch.empty(da.numel() + skew).cuda()       # skew = 1: dA one float off z's 16-byte phase
                    buf[skew:].copy_(da.reshape(-1))
                    out = ops.bn_act_bwd(buf[skew:].view(-1, L), z.cuda().reshape(-1, L), C, act, training, *consts)
                    emit(f"bn_act_bwd/B{B}T{T}F{Fq}s{skew}/{layout}/{act}/train{int(training)}",
                         dict(zip(("dz", "dgamma", "dbeta", "dbias"), out)))

    for B, T, Fq in BN_FIRST_SHAPES:
        for act in ("mish", "relu"):
            for training in (True, False):
                g = torch.Generator().manual_seed(17)
                z = torch.randn(B, 64, T, Fq, generator=g) * 1.5 + 0.3
                da = torch.randn(B, 64, T, Fq, generator=g)
                x = torch.rand(B, T, Fq, generator=g)
                out = ops.bn_act_bwd_first(da.cuda(), z.cuda(), x.cuda(), act, training, *bn_consts(z, g, training))
                emit(f"bn_act_bwd_first/B{B}T{T}F{Fq}/{act}/train{int(training)}", dict(zip(("dgamma", "dbeta", "dbias", "dw"), out)))

    g = torch.Generator().manual_seed(9)      # test_conv_edge_layers_backward
    B, T, Fq = 2, 7, 83
    a7 = torch.randn(B, 64, T, Fq, generator=g).cuda()
    w8 = (torch.randn(8, 64, 1, 1, generator=g) * 0.2).cuda()
    dz8 = torch.randn(B, T, 8, Fq, generator=g).cuda()
    x = torch.rand(B, T, Fq, generator=g).cuda()
    torch.randn(64, 1, 1, 7, generator=g)
    dz1 = torch.randn(B, 64, T, Fq, generator=g).cuda()
    emit("conv_last_dgrad", dict(din=ops.conv_last_dgrad(dz8, w8, B, T, Fq)))
    emit("conv_last_wgrad", dict(dw=ops.conv_last_wgrad(dz8, a7)))
    emit("conv_first_wgrad", dict(dw=ops.conv_first_wgrad(dz1, x)))

    B, T = 2, 45
    sd = {k: v.cuda() for k, v in R.spread_logits(R.build_state_dict(SMALL, 21), 6.0).items()}
    x, dvec = (t.cuda() for t in R.synthetic_inputs(B, T, SMALL, 21))
    dmask = torch.randn(B, T, SMALL["fc2_dim"], generator=torch.Generator().manual_seed(5)).cuda()
    for math in ("fp32", "f16x3"):
        dims = ops.make_dims(B, T, SMALL["num_freq"], SMALL["emb_dim"], SMALL["lstm_dim"], SMALL["fc1_dim"], SMALL["fc2_dim"], math=math)
        tape = ops.new_tape(dims, x.device)
        t = {k: v.clone() for k, v in sd.items()}       # train mode moves the running statistics
        mask = ops.forward_train(t, x, dvec, dims, "mish", True, tape)
        grads = ops.backward(t, x, dvec, dims, "mish", True, tape, mask, dmask, want_dvec=True)
        emit(f"small/B{B}T{T}/{math}/mish/forward_train+backward", dict(mask=mask, **grads))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
