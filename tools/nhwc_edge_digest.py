"""One SHA-256 per case over the HBM-bound kernels of the channels-last path (csrc/nhwc_first.hip, nhwc_bn.hip, nhwc_last.hip): what
tools/forward_digest.py and tools/backward_digest.py do not reach.  Every layer-level op of ops.py that lands in those files, with
every activation and BatchNorm mode it takes, at four shapes (B, T, F):
    (1, 2, 5)      a row shorter than the 7 taps
    (3, 11, 37)    npix no multiple of 32, F no multiple of 16
    (2, 16, 64)    cnn8's grid is 32 workgroups: the round-robin over the XCDs runs (at the other shapes the grid is no multiple of 8)
    (2, 33, 301)   several sweeps' worth of blocks per statistics slot
then one small bf16 training step (forward_train + backward) with VS_OPT_DETERMINISTIC 1 and 0, and the refusals (unsupported
activation, NULL arguments: the return code and the library's message are what is hashed).  Every tensor goes into the hash with
its name, dtype and shape.  Two builds of the library that launch the same kernels on the same operands print the same lines
wherever one build does so twice: the fp64 atomics of the statistics arrive in any order outside the deterministic mode, so the
lines that depend on them may differ in the last bits between two runs of ONE build (--dump DIR keeps every case's tensors as
DIR/<case>.npz to measure by how much).

    python tools/nhwc_edge_digest.py [--lib path/to/libvoicesplit_hip.so] [--dump DIR] > digests.txt"""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import reference_forward as R  # noqa: E402

SMALL = dict(num_freq=53, emb_dim=24, lstm_dim=32, fc1_dim=44, fc2_dim=53)      # tools/backward_digest.py
SHAPES = [(1, 2, 5), (3, 11, 37), (2, 16, 64), (2, 33, 301)]
ACTS = ("mish", "relu", "none")
# entry points of the three files that take pointers: called with every pointer NULL
NULL_CALLS = ["vs_nhwc_conv_first", "vs_nhwc_first_moments", "vs_nhwc_first_stats", "vs_nhwc_first_bwd", "vs_nhwc_bn_apply", "vs_nhwc_conv_last",
              "vs_nhwc_conv_last_pre", "vs_nhwc_bn_act_bwd", "vs_nhwc_bn_act_bwd_first", "vs_nhwc_conv_last_bwd", "vs_nhwc_conv_last_bwd_dy",
              "vs_nhwc_bn_bwd_from_dy", "vs_nhwc_bn_bwd_first_from_dy"]


def as_numpy(t):
    t = t.detach().cpu()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.numpy()       # numpy has no bf16: the bits, named so below


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
            tensors = fn()
            arrays = {k: as_numpy(v) for k, v in tensors.items()}
            dtypes = {k: str(v.dtype) for k, v in tensors.items()}
        except _lib.VoiceSplitHipError as err:
            arrays = {"refused": np.frombuffer(str(err).encode(), dtype=np.uint8)}
            dtypes = {"refused": "text"}
        h = hashlib.sha256()
        for k in sorted(arrays):
            h.update(f"{k}:{dtypes[k]}:{arrays[k].shape}:".encode())
            h.update(arrays[k].tobytes())
        print(f"{h.hexdigest()}  {case}{'  (refused)' if 'refused' in arrays else ''}", flush=True)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            np.savez(os.path.join(args.dump, case.replace("/", "_") + ".npz"), **arrays)

    def bn_consts(z, g, training):
        """scale, shift, mean, invstd of a BatchNorm over z [.., C] (batch or made-up running statistics)"""
        C = z.shape[-1]
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
        rmean, rvar = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        zz = z.double().reshape(-1, C)
        mean, var = (zz.mean(0), zz.var(0, unbiased=False)) if training else (rmean.double(), rvar.double())
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        scale = gamma.double() * invstd
        return [t.float().cuda() for t in (scale, beta.double() - mean * scale, mean, invstd)]

    for B, T, Fq in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + 10 * T + Fq)
        sh = f"B{B}T{T}F{Fq}"
        x = torch.rand(B, T, Fq, generator=g).cuda()
        w1 = (torch.randn(64, 1, 1, 7, generator=g) * 0.4).cuda()
        b1 = (torch.randn(64, generator=g) * 0.1).cuda()
        w8 = (torch.randn(8, 64, 1, 1, generator=g) * 0.2).cuda()
        s8, h8 = (torch.rand(8, generator=g) + 0.5).cuda(), (torch.randn(8, generator=g) * 0.1).cuda()
        z = (torch.randn(B, T, Fq, 64, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
        da = torch.randn(B, T, Fq, 64, generator=g).to(torch.bfloat16).cuda()
        dz8 = torch.randn(B, T, 8 * Fq, generator=g).cuda()
        consts = {tr: bn_consts(z.float(), g, tr) for tr in (True, False)}
        z = z.cuda()
        scale, shift = consts[False][:2]

        for act in ACTS:
            emit(f"{sh}/conv_first/{act}", lambda: dict(a=ops.nhwc_conv_first(x, w1, scale, shift, act)))
            emit(f"{sh}/bn_apply/{act}", lambda: dict(a=ops.nhwc_bn_apply(z, scale, shift, act)))
            emit(f"{sh}/conv_last/{act}", lambda: dict(feat=ops.nhwc_conv_last(z, w8, s8, h8, act)))
        emit(f"{sh}/conv_first/none/stats", lambda: dict(zip(("z", "stats"), ops.nhwc_conv_first(x, w1, scale, shift, "none", stats=True))))
        mom = ops.nhwc_first_moments(x)
        emit(f"{sh}/first_moments", lambda: dict(mom=mom))
        emit(f"{sh}/first_stats", lambda: dict(stats=ops.nhwc_first_stats(mom, w1, b1, B * T * Fq)))
        for act in ("mish", "relu"):
            emit(f"{sh}/conv_last_pre/{act}", lambda: dict(feat=ops.nhwc_conv_last_pre(z, scale, shift, act, w8, s8, h8)))
            emit(f"{sh}/conv_last_pre/{act}/stats", lambda: dict(zip(("feat", "stats"), ops.nhwc_conv_last_pre(z, scale, shift, act, w8, s8, h8, stats=True))))
        emit(f"{sh}/conv_last_bwd", lambda: dict(zip(("din", "dw"), ops.nhwc_conv_last_bwd(dz8, w8, z))))

        for training in (True, False):
            c = consts[training]
            tr = f"train{int(training)}"
            for act in ACTS:
                emit(f"{sh}/first_bwd/{act}/{tr}", lambda: dict(zip(("dw", "dgamma", "dbeta", "dbias"), ops.nhwc_first_bwd(da, x, w1, b1, act, training, *c))))
                emit(f"{sh}/bn_act_bwd/{act}/{tr}", lambda: dict(zip(("dz", "dgamma", "dbeta", "dbias"), ops.nhwc_bn_act_bwd(da, z, act, training, *c))))
                emit(f"{sh}/bn_act_bwd_first/{act}/{tr}",
                     lambda: dict(zip(("dw", "dgamma", "dbeta", "dbias"), ops.nhwc_bn_act_bwd_first(da, z, x, act, training, *c))))
            for act in ("mish", "relu"):
                a7 = ops.nhwc_bn_apply(z, c[0], c[1], act)
                for recomputed in (False, True):
                    name = f"{sh}/conv_last_bwd_dy/{act}/{tr}/{'recomputed' if recomputed else 'a7'}"
                    dy, dw, st = ops.nhwc_conv_last_bwd_dy(dz8, w8, None if recomputed else a7, z, act, *c)
                    emit(name, lambda: dict(dy=dy, dw=dw, stats=st))
                # the statistics are folded (and zeroed) by the consumer: each gets its own copy
                emit(f"{sh}/bn_bwd_from_dy/{act}/{tr}",
                     lambda: dict(zip(("dz", "dgamma", "dbeta", "dbias"), ops.nhwc_bn_bwd_from_dy(dy, z, st.clone(), training, c[0], c[2], c[3]))))
                emit(f"{sh}/bn_bwd_first_from_dy/{act}/{tr}",
                     lambda: dict(zip(("dw", "dgamma", "dbeta", "dbias"), ops.nhwc_bn_bwd_first_from_dy(dy, z, x, st.clone(), training, c[0], c[2], c[3]))))

        if (B, T, Fq) == SHAPES[1]:       # refusals: an activation these kernels do not have
            c = consts[True]
            emit("refuse/act/conv_first", lambda: dict(a=ops.nhwc_conv_first(x, w1, scale, shift, "sigmoid")))
            emit("refuse/act/conv_first_stats", lambda: dict(a=ops.nhwc_conv_first(x, w1, scale, shift, "mish", stats=True)[0]))
            emit("refuse/act/bn_apply", lambda: dict(a=ops.nhwc_bn_apply(z, scale, shift, "sigmoid")))
            emit("refuse/act/conv_last", lambda: dict(a=ops.nhwc_conv_last(z, w8, s8, h8, "sigmoid")))
            emit("refuse/act/conv_last_pre", lambda: dict(a=ops.nhwc_conv_last_pre(z, scale, shift, "none", w8, s8, h8)))
            emit("refuse/act/first_bwd", lambda: dict(a=ops.nhwc_first_bwd(da, x, w1, b1, "sigmoid", True, *c)[0]))
            emit("refuse/act/bn_act_bwd", lambda: dict(a=ops.nhwc_bn_act_bwd(da, z, "sigmoid", True, *c)[0]))
            emit("refuse/act/bn_act_bwd_first", lambda: dict(a=ops.nhwc_bn_act_bwd_first(da, z, x, "sigmoid", True, *c)[0]))
            emit("refuse/act/conv_last_bwd_dy", lambda: dict(a=ops.nhwc_conv_last_bwd_dy(dz8, w8, None, z, "none", *c)[0]))

    def null_call(name):
        """every pointer NULL (the stream too: the default one), every number 1"""
        _, argtypes = _lib.SIGNATURES[name]
        argv = [1.0 if t in (ctypes.c_double, ctypes.c_float) else 1 if t in (ctypes.c_int, ctypes.c_longlong) else None for t in argtypes]
        _lib.check(getattr(lib, name)(*argv), name)
        return {}

    for name in NULL_CALLS:
        emit(f"refuse/null/{name}", lambda: null_call(name))

    B, T = 2, 45
    sd = {k: v.cuda() for k, v in R.spread_logits(R.build_state_dict(SMALL, 21), 6.0).items()}
    x, dvec = (t.cuda() for t in R.synthetic_inputs(B, T, SMALL, 21))
    dmask = torch.randn(B, T, SMALL["fc2_dim"], generator=torch.Generator().manual_seed(5)).cuda()
    dims = ops.make_dims(B, T, SMALL["num_freq"], SMALL["emb_dim"], SMALL["lstm_dim"], SMALL["fc1_dim"], SMALL["fc2_dim"], math="bf16")
    prev = _lib.get_option("DETERMINISTIC")
    try:
        for det in (1, 0):
            _lib.set_option("DETERMINISTIC", det)

            def step():
                tape = ops.new_tape(dims, x.device)
                t = {k: v.clone() for k, v in sd.items()}       # train mode moves the running statistics
                mask = ops.forward_train(t, x, dvec, dims, "mish", True, tape)
                grads = ops.backward(t, x, dvec, dims, "mish", True, tape, mask, dmask, want_dvec=True)
                moved = {"state/" + k: v for k, v in t.items() if "running" in k}
                return dict(mask=mask, **{"grad/" + k: v for k, v in grads.items()}, **moved)

            emit(f"small/B{B}T{T}/bf16/mish/forward_train+backward/deterministic{det}", step)
    finally:
        _lib.set_option("DETERMINISTIC", prev)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
