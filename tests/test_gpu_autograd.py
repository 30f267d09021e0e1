"""GPU: the autograd contract of the module (model._MaskForward) beyond "forward, then backward at once".

What users of an nn.Module do besides that, and what torch promises for it:
(1) several graphs in flight: F(A), F(B), then the backward calls in any order, or one backward through L_A + L_B, or a
    recycled tape reused by a third forward while another tape is still alive -- every gradient, every mask and the BatchNorm
    running statistics must be the bits of the sequential run (deterministic mode, so that bits are comparable), and the sum
    must agree with the fp64 oracle;
(2) the BatchNorm mode of the FORWARD decides the backward, whatever the module's mode when backward runs;
(3) an in-place edit of anything the backward depends on -- every parameter, x, the speaker embedding and, behind an eval-mode
    BatchNorm forward, the running statistics -- between forward and backward raises, as torch's own layers raise;
    edits after the backward, or of tensors the backward does not depend on, do not;
(4) frozen subsets (requires_grad_(False)) leave the remaining gradients bit-identical and the frozen ones None.
Small dims as in test_gpu_backward.py's training-step test, in all three arithmetics; one full-size bf16 case."""
import contextlib

import pytest
import torch

from oracle import reference_backward as RB
from oracle import reference_forward as R
from test_gpu_backward import MTOL, _branch_consistent_oracle, _dump, _module, _zero_bias_keys, rel_err

pytestmark = pytest.mark.gpu

DIMS = dict(num_freq=37, emb_dim=16, lstm_dim=24, fc1_dim=40, fc2_dim=37)
# A and B differ in shape (their tapes differ in size); C has A's shape and new data: it reuses A's recycled tape
SHAPES = {"A": (3, 21), "B": (2, 33), "C": (3, 21)}
SEEDS = {"A": 11, "B": 12, "C": 13}
MATHS = ["fp32", "f16x3", "bf16"]
MODELS = [("VoiceSplit", "mish"), ("VoiceFilter", "relu")]
# bf16 keeps 8 significant bits: against the fp64 oracle it is held to pooled bounds (tests/test_gpu_bf16.py states the
# per-tensor ones).  Measured on MI355X: 0.05 .. 0.26 relative L2, cosine >= 0.966 (VoiceFilter with batch statistics the
# worst).  A gradient that misses or doubles one of the two batches is ~0.7 off on both measures.
BF16_POOLED_L2 = 0.4
BF16_POOLED_COS = 0.92


def _sd():
    return R.spread_logits(R.build_state_dict(DIMS, 7), 6.0)


def _data(name, dims=DIMS, shapes=SHAPES, seeds=SEEDS):
    B, T = shapes[name]
    x, dvec = R.synthetic_inputs(B, T, dims, seeds[name])
    return x, dvec, RB.loss_weights(B, T, dims["fc2_dim"], seeds[name])


@contextlib.contextmanager
def _mode(math):
    """conv math + deterministic mode (bitwise comparisons), both restored."""
    from voicesplit_amd import _lib, ops
    prev_math = ops.get_conv_math()
    prev_det = _lib.set_option("DETERMINISTIC", 1)
    ops.set_conv_math(math)
    try:
        yield
    finally:
        ops.set_conv_math(prev_math)
        _lib.set_option("DETERMINISTIC", prev_det)


def _fwd(m, data):
    """-> (mask, speaker embedding leaf, weighted loss)"""
    x, dvec, w = data
    emb = dvec.cuda().requires_grad_(True)
    mask = m(x.cuda(), emb)
    return mask, emb, (mask * w.cuda()).sum()


def _grads(m):
    return {k: None if p.grad is None else p.grad.detach().clone() for k, p in m.named_parameters()}


def _buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}


def _sequential(cls_name, sd, training, names, dims=DIMS, data=None):
    """The reference: forward + backward per batch, in order, .grad captured (and cleared) per batch.
    -> {name: (mask, parameter gradients, speaker-embedding gradient)}, {name: buffers after that batch}"""
    m = _module(cls_name, dims, sd).train(training)
    out, bufs = {}, {}
    for n in names:
        m.zero_grad(set_to_none=True)
        mask, emb, loss = _fwd(m, data[n] if data else _data(n))
        loss.backward()
        out[n] = (mask.detach().clone(), _grads(m), emb.grad.detach().clone())
        bufs[n] = _buffers(m)
    return out, bufs


def _assert_equal(got, ref, what):
    bad = [k for k in ref if not torch.equal(got[k], ref[k])]
    assert not bad, f"{what}: not bit-identical: {bad}"


def _pooled(got, ref, keys):
    g = torch.cat([got[k].detach().double().cpu().reshape(-1) for k in keys])
    r = torch.cat([ref[k].detach().double().cpu().reshape(-1) for k in keys])
    return float((g - r).norm() / r.norm().clamp_min(1e-300)), float((g @ r) / (g.norm() * r.norm()).clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------
# (1) several tapes in flight
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cls_name,act", MODELS)
@pytest.mark.parametrize("training", [True, False])
def test_interleaved_tapes_are_bit_identical_to_the_sequential_run(math, cls_name, act, training):
    sd = _sd()
    with _mode(math):
        ref, ref_bufs = _sequential(cls_name, sd, training, "ABC")
        gA, gB = ref["A"][1], ref["B"][1]
        summed = {k: gA[k] + gB[k] for k in gA}

        # order 1: F(A), F(B), backward B, backward A -- .grad accumulates
        m = _module(cls_name, DIMS, sd).train(training)
        mA, eA, lA = _fwd(m, _data("A"))
        mB, eB, lB = _fwd(m, _data("B"))
        lB.backward()
        lA.backward()
        _assert_equal(_grads(m), summed, "order 1")
        assert torch.equal(mA, ref["A"][0]) and torch.equal(mB, ref["B"][0])
        assert torch.equal(eA.grad, ref["A"][2]) and torch.equal(eB.grad, ref["B"][2])
        _assert_equal(_buffers(m), ref_bufs["B"], "order 1, running statistics")

        # order 2: F(A), F(B), one backward through L_A + L_B
        m = _module(cls_name, DIMS, sd).train(training)
        mA, eA, lA = _fwd(m, _data("A"))
        mB, eB, lB = _fwd(m, _data("B"))
        (lA + lB).backward()
        _assert_equal(_grads(m), summed, "order 2")
        assert torch.equal(mA, ref["A"][0]) and torch.equal(mB, ref["B"][0])
        assert torch.equal(eA.grad, ref["A"][2]) and torch.equal(eB.grad, ref["B"][2])
        _assert_equal(_buffers(m), ref_bufs["B"], "order 2, running statistics")

        # order 3: F(A), F(B), backward A, F(C) on A's recycled tape while B's is live, backward C, backward B
        m = _module(cls_name, DIMS, sd).train(training)
        mA, eA, lA = _fwd(m, _data("A"))
        tape_a = mA.grad_fn.tape.data_ptr()
        mB, eB, lB = _fwd(m, _data("B"))
        lA.backward()
        got_a = _grads(m)
        m.zero_grad(set_to_none=True)
        mC, eC, lC = _fwd(m, _data("C"))
        assert mC.grad_fn.tape.data_ptr() == tape_a, "C did not take A's recycled tape: the case is not exercised"
        lC.backward()
        got_c = _grads(m)
        m.zero_grad(set_to_none=True)
        lB.backward()
        for n, got, mask, emb in (("A", got_a, mA, eA), ("C", got_c, mC, eC), ("B", _grads(m), mB, eB)):
            _assert_equal(got, ref[n][1], f"order 3, batch {n}")
            assert torch.equal(mask, ref[n][0]), n
            assert torch.equal(emb.grad, ref[n][2]), n
        _assert_equal(_buffers(m), ref_bufs["C"], "order 3, running statistics")


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cls_name,act", MODELS)
@pytest.mark.parametrize("training", [True, False])
def test_interleaved_gradient_sum_matches_fp64_oracle(math, cls_name, act, training):
    """Order 1 against the sum of the fp64 oracle's per-batch gradients: a consistent but wrong answer does not pass."""
    from voicesplit_amd import ops
    sd = _sd()
    data = {n: _data(n) for n in "AB"}
    with _mode(math):
        m = _module(cls_name, DIMS, sd).train(training)
        mA, eA, lA = _fwd(m, data["A"])
        mB, eB, lB = _fwd(m, data["B"])
        tapes = {"A": mA.grad_fn.tape, "B": mB.grad_fn.tape}
        lB.backward()
        lA.backward()
        torch.cuda.synchronize()
        got = _grads(m)
        refs = {}
        for n in "AB":
            x, dvec, w = data[n]
            if math == "bf16":       # (the tape holds bf16 channels-last activations: no fp32 ReLU signs to read back)
                refs[n] = RB.gradients(sd, x, dvec, w, act=act, training=training, dtype=torch.float64, lstm_impl="loop",
                                       want_dvec=True)
            else:
                dims = ops.make_dims(x.shape[0], x.shape[1], *DIMS.values())
                refs[n] = _branch_consistent_oracle(sd, x, dvec, w, act, training, tapes[n], dims, lstm_impl="loop",
                                                    want_dvec=True)
    zero = _zero_bias_keys(training)
    for k in zero:
        assert got[k].abs().max().item() == 0.0, k
    keys = [k for k in got if k not in zero]
    ref = {k: refs["A"][k] + refs["B"][k] for k in keys}
    ref["dvec/A"], ref["dvec/B"] = refs["A"]["speaker_embedding"], refs["B"]["speaker_embedding"]
    got["dvec/A"], got["dvec/B"] = eA.grad, eB.grad
    keys += ["dvec/A", "dvec/B"]
    if math == "bf16":
        l2, cos = _pooled(got, ref, keys)
        _dump(f"autograd_bf16_{cls_name}_{training}", {"pooled_rel_l2": l2, "pooled_cos": cos})
        assert l2 < BF16_POOLED_L2 and cos >= BF16_POOLED_COS, (l2, cos)
    else:
        worst = {k: rel_err(got[k], ref[k]) for k in keys}
        bad = {k: v for k, v in worst.items() if not v < MTOL}
        assert not bad, bad


def test_interleaved_tapes_full_size_bf16():
    """The metric dims in bf16 at B = 4, T = 301 (the side-stream prologue and the backward-overlap stream at the real widths):
    order 1 bit-identical to the sequential run."""
    dims = R.default_dims()
    sd = R.spread_logits(R.build_state_dict(dims, 3), 8.0)
    shapes, seeds = {"A": (4, 301), "B": (4, 301)}, {"A": 31, "B": 32}
    data = {n: _data(n, dims, shapes, seeds) for n in "AB"}
    with _mode("bf16"):
        ref, ref_bufs = _sequential("VoiceSplit", sd, True, "AB", dims=dims, data=data)
        m = _module("VoiceSplit", dims, sd).train()
        mA, eA, lA = _fwd(m, data["A"])
        mB, eB, lB = _fwd(m, data["B"])
        lB.backward()
        lA.backward()
        torch.cuda.synchronize()
        assert m.lstm_status() == 0
    gA, gB = ref["A"][1], ref["B"][1]
    _assert_equal(_grads(m), {k: gA[k] + gB[k] for k in gA}, "full size, order 1")
    assert torch.equal(mA, ref["A"][0]) and torch.equal(mB, ref["B"][0])
    assert torch.equal(eA.grad, ref["A"][2]) and torch.equal(eB.grad, ref["B"][2])
    _assert_equal(_buffers(m), ref_bufs["B"], "full size, running statistics")


# ---------------------------------------------------------------------------------------------
# (2) the forward's BatchNorm mode decides the backward
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("training", [True, False])
def test_mode_switch_between_forward_and_backward(math, training):
    sd = _sd()
    with _mode(math):
        ref, _ = _sequential("VoiceSplit", sd, training, "A")
        m = _module("VoiceSplit", DIMS, sd).train(training)
        mask, emb, loss = _fwd(m, _data("A"))
        m.train(not training)
        loss.backward()
    _assert_equal(_grads(m), ref["A"][1], "mode switched before backward")
    assert torch.equal(emb.grad, ref["A"][2])


# ---------------------------------------------------------------------------------------------
# (3) in-place edits between forward and backward
# ---------------------------------------------------------------------------------------------

# one parameter of each kind: cnn3 (a 64->64 layer: its backward image sits in the bf16 tape), cnn1, cnn8, a conv bias,
# BatchNorm gamma / beta, the LSTM input / recurrent weights and a bias, the head
EDITED = ["conv.9.weight", "conv.1.weight", "conv.28.weight", "conv.13.bias", "conv.14.weight", "conv.14.bias",
          "lstm.weight_ih_l0", "lstm.weight_hh_l0_reverse", "lstm.bias_ih_l0", "fc1.weight", "fc2.bias"]


def _raises_inplace(loss):
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("training", [True, False])
def test_inplace_edit_between_forward_and_backward_raises(math, training):
    sd = _sd()
    with _mode(math):
        m = _module("VoiceSplit", DIMS, sd).train(training)
        params = dict(m.named_parameters())
        for key in EDITED:
            _, _, loss = _fwd(m, _data("A"))
            with torch.no_grad():
                params[key].add_(1e-3)
            _raises_inplace(loss)

        # an optimizer step (it needs gradients: one full step first)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        _fwd(m, _data("A"))[2].backward()
        _, _, loss = _fwd(m, _data("A"))
        opt.step()
        _raises_inplace(loss)

        # load_state_dict copies into the same tensors
        _, _, loss = _fwd(m, _data("A"))
        m.load_state_dict(sd)
        _raises_inplace(loss)

        # the inputs
        x, dvec, w = _data("A")
        xc = x.cuda()
        loss = (m(xc, dvec.cuda()) * w.cuda()).sum()
        xc.mul_(0.5)
        _raises_inplace(loss)
        mask, emb, loss = _fwd(m, _data("A"))
        with torch.no_grad():
            emb.add_(1e-3)
        _raises_inplace(loss)

        if not training:
            # eval-mode forward, then a train-mode forward moves the running statistics the first one used
            _, _, loss_a = _fwd(m, _data("A"))
            m.train()
            _, _, loss_b = _fwd(m, _data("B"))
            _raises_inplace(loss_a)
            loss_b.backward()          # its own forward ran with batch statistics: unaffected


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("training", [True, False])
def test_edits_the_backward_does_not_depend_on_do_not_raise(math, training):
    sd = _sd()
    with _mode(math):
        ref, _ = _sequential("VoiceSplit", sd, training, "A")
        m = _module("VoiceSplit", DIMS, sd).train(training)
        other = torch.zeros(64, device="cuda")
        _, _, loss = _fwd(m, _data("A"))
        other.add_(1.0)                                       # an unrelated tensor
        if training:
            # batch-statistics BatchNorm: the running statistics are outputs of the forward, not inputs of the backward
            with torch.no_grad():
                m.conv[14].running_mean.add_(1e-3)
                m.conv[14].running_var.mul_(1.01)
                m.conv[14].num_batches_tracked.add_(1)
        loss.backward()
        _assert_equal(_grads(m), ref["A"][1], "backward after unrelated edits")
        # edits after the backward: nothing is pending
        with torch.no_grad():
            m.fc1.weight.add_(1e-3)
            m.conv[9].weight.add_(1e-3)
        # the forward -> backward -> optimizer step loop of train.py:109-112
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        for _ in range(3):
            opt.zero_grad()
            _fwd(m, _data("A"))[2].backward()
            opt.step()
        assert all(torch.isfinite(p).all() for p in m.parameters())


# ---------------------------------------------------------------------------------------------
# (4) frozen subsets
# ---------------------------------------------------------------------------------------------

FROZEN = {"conv": lambda k: k.startswith("conv."), "lstm": lambda k: k.startswith("lstm."), "all": lambda k: True}


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("cls_name,act", MODELS)
@pytest.mark.parametrize("training", [True, False])
def test_frozen_subsets_leave_the_other_gradients_bit_identical(math, cls_name, act, training):
    from voicesplit_amd import ops
    sd = _sd()
    x, dvec, w = _data("A")
    with _mode(math):
        ref, _ = _sequential(cls_name, sd, training, "A")
        for name, frozen in FROZEN.items():
            m = _module(cls_name, DIMS, sd).train(training)
            for k, p in m.named_parameters():
                p.requires_grad_(not frozen(k))
            mask, emb, loss = _fwd(m, (x, dvec, w))
            tape = mask.grad_fn.tape
            loss.backward()
            torch.cuda.synchronize()
            got = _grads(m)
            assert torch.equal(mask, ref["A"][0]), name
            assert all(got[k] is None for k in got if frozen(k)), name
            _assert_equal({k: v for k, v in got.items() if not frozen(k)},
                          {k: v for k, v in ref["A"][1].items() if not frozen(k)}, f"frozen {name}")
            assert torch.equal(emb.grad, ref["A"][2]), name
        # every parameter frozen, only the speaker embedding's gradient asked for: against the oracle
        if math == "bf16":
            oracle = RB.gradients(sd, x, dvec, w, act=act, training=training, dtype=torch.float64, lstm_impl="loop",
                                  want_dvec=True)
        else:
            dims = ops.make_dims(x.shape[0], x.shape[1], *DIMS.values())
            oracle = _branch_consistent_oracle(sd, x, dvec, w, act, training, tape, dims, lstm_impl="loop", want_dvec=True)
    if math == "bf16":
        l2, cos = _pooled({"d": emb.grad}, {"d": oracle["speaker_embedding"]}, ["d"])
        _dump(f"autograd_bf16_dvec_{cls_name}_{training}", {"rel_l2": l2, "cos": cos})
        assert l2 < BF16_POOLED_L2 and cos >= BF16_POOLED_COS, (l2, cos)
    else:
        assert rel_err(emb.grad, oracle["speaker_embedding"]) < MTOL
