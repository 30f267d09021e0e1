"""CPU: the host side of the ragged eval forward (clips of unequal length in one batch, each as if alone): the batch
planner's properties, the new C-ABI prototypes in header, library and ctypes table, and the module surface."""
import inspect
import os
import random
import re

import pytest

from conftest import ROOT


def _random_lengths(seed, n):
    rng = random.Random(seed)
    return [rng.randint(531, 1142) for _ in range(n)]          # the demo clips' range of frames


@pytest.mark.parametrize("seed,n,max_items,max_frames", [(0, 64, 16, 16 * 1142), (1, 37, 8, 6000), (2, 5, 64, 64 * 301), (3, 1, 1, 1)])
def test_plan_is_a_partition_within_its_bounds(seed, n, max_items, max_frames):
    from voicesplit_amd.streaming import padded_frame_share, plan_ragged_batches
    lens = _random_lengths(seed, n)
    plan = plan_ragged_batches(lens, max_items, max_frames)
    assert sorted(i for b in plan for i in b) == list(range(n))               # every item exactly once
    for b in plan:
        assert 1 <= len(b) <= max_items
        assert len(b) == 1 or len(b) * max(lens[i] for i in b) <= max_frames
    assert plan == plan_ragged_batches(list(lens), max_items, max_frames)      # deterministic
    assert 0.0 <= padded_frame_share(lens, plan) < 1.0
    # sorted by length: no clip of a later batch is longer than one of an earlier batch
    for a, b in zip(plan, plan[1:]):
        assert min(lens[i] for i in a) >= max(lens[i] for i in b)


def test_plan_edge_cases():
    from voicesplit_amd.streaming import padded_frame_share, plan_ragged_batches
    # one item longer than max_frames still gets a batch of its own; the others pack behind it
    assert plan_ragged_batches([5000, 100, 100, 100], 8, 1000) == [[0], [1, 2, 3]]
    assert plan_ragged_batches([], 4, 100) == []
    # ties keep index order; equal lengths pad nothing
    plan = plan_ragged_batches([301] * 5, 2, 10 ** 6)
    assert plan == [[0, 1], [2, 3], [4]] and padded_frame_share([301] * 5, plan) == 0.0
    # tensors of lengths are accepted as well as lists
    import torch
    assert plan_ragged_batches(torch.tensor([3, 9, 4]), 2, 100) == [[1, 2], [0]]
    for bad in ((0, 10), (4, 0)):
        with pytest.raises(ValueError, match="positive"):
            plan_ragged_batches([10], *bad)
    with pytest.raises(ValueError, match="at least 1"):
        plan_ragged_batches([10, 0], 4, 100)


RAGGED_EXPORTS = {
    "vs_forward_prepared_ragged": 12, "vs_conv_stack_fwd_ragged": 9, "vs_bilstm_fwd_ragged": 9, "vs_zero_tail_rows": 6,
}


def test_header_library_and_ctypes_table_agree_on_the_ragged_entry_points():
    from voicesplit_amd import _lib
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, nargs in RAGGED_EXPORTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == nargs and restype is _lib.c_int, name
        assert any(re.fullmatch(r"const int\s*\*\s*lengths", a) for a in args), f"{name}: lengths is a device const int*"
        assert hasattr(lib, name)
    assert lib.vs_abi_version() == 11                       # additive entries under the same ABI number
    # argument errors come back as codes with a message, before any launch
    assert lib.vs_zero_tail_rows(None, 1, 1, 4, None, None) != 0 and b"NULL" in lib.vs_last_error()
    assert lib.vs_zero_tail_rows(256, 1, 4, 6, 256, None) != 0 and b"row_bytes" in lib.vs_last_error()
    from voicesplit_amd import ops
    import ctypes
    for math in ("fp32",):
        d = ops.make_dims(2, 10, 37, 16, 24, 40, 37, math=math)
        rc = lib.vs_forward_prepared_ragged(ctypes.byref(d), None, None, 0, None, None, 256, 1, None, 0, 256, None)
        assert rc != 0 and b"VS_MATH_FP32" in lib.vs_last_error()
    d = ops.make_dims(2, 10, 37, 16, 24, 40, 37, math="f16x3")
    assert lib.vs_conv_stack_fwd_ragged(ctypes.byref(d), None, None, None, 1, None, 0, None, None) != 0
    assert b"lengths is NULL" in lib.vs_last_error()


def test_module_surface():
    import voicesplit_amd as V
    for cls in (V.VoiceSplit, V.VoiceFilter):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "x", "speaker_embedding"]       # the reference's
        assert list(inspect.signature(cls.forward_ragged).parameters) == ["self", "x", "speaker_embedding", "lengths"]
    from voicesplit_amd import audio, evaluate, ops
    from voicesplit_amd.trainer import Trainer
    assert inspect.signature(ops.forward_prepared).parameters["lengths"].default is None
    assert inspect.signature(evaluate.eval_batches).parameters["ragged"].default is False
    assert callable(audio.separate_many) and callable(Trainer.evaluate_ragged)
    assert inspect.signature(ops.conv_stack).parameters["lengths"].default is None
    assert inspect.signature(ops.bilstm).parameters["lengths"].default is None


def test_lengths_are_range_checked_on_the_host():
    import torch
    from voicesplit_amd import ops
    assert ops.device_lengths([3, 1, 5], 3, 5, "cpu").tolist() == [3, 1, 5]
    assert ops.device_lengths(torch.tensor([5, 5]), 2, 5, "cpu").dtype == torch.int32
    for bad in ([0, 3], [6, 3]):
        with pytest.raises(ValueError, match="1 <= length <= T = 5"):
            ops.device_lengths(bad, 2, 5, "cpu")
    with pytest.raises(ValueError, match="3 values for a batch of 2"):
        ops.device_lengths([1, 2, 3], 2, 5, "cpu")
