"""CPU: the one place a call crosses into the library (voicesplit_amd/_call.py) -- device guard, stream last, pointer conversion,
error text, sizers, the scratch registry -- with a fake library and a recording stand-in for ``torch.cuda.device``, and one wrapper of
each family of ``ops`` that used to run without the guard."""
import ctypes

import pytest
import torch

STREAM = ctypes.c_void_p(0x5ead)


class _FakeLib:
    """Records (symbol, args); every entry point returns ``rc`` (default 0), every ``*_floats`` / ``*_bytes`` query 128."""

    def __init__(self):
        self.calls, self.rc, self.error, self.effects = [], {}, b"the reason", {}

    def vs_last_error(self):
        return self.error

    def __getattr__(self, name):
        if not name.startswith("vs_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name in self.effects:
                self.effects[name](*args)
            return self.rc.get(name, 128 if name.endswith(("_floats", "_bytes")) else 0)
        return fn


class _Guard:
    def __init__(self, log, device):
        self.log, self.device = log, device

    def __enter__(self):
        self.log.append(("enter", self.device))

    def __exit__(self, *exc):
        self.log.append(("exit", self.device))


@pytest.fixture
def fake(monkeypatch):
    from voicesplit_amd import _call
    lib = _FakeLib()
    lib.guards = []
    monkeypatch.setattr(_call._lib, "load", lambda path=None: lib)
    monkeypatch.setattr(_call, "dev_check", lambda t, name, dtype=torch.float32: None)
    monkeypatch.setattr(_call, "stream", lambda: STREAM)
    monkeypatch.setattr(_call, "_SCRATCH", {})
    monkeypatch.setattr(torch.cuda, "device", lambda dev: _Guard(lib.guards, dev))
    return lib


def test_call_guards_converts_and_passes_the_stream_last(fake):
    from voicesplit_amd import _call, _lib
    t, d = torch.zeros(4), _lib.VsDims(1, 2, 3, 4, 5, 6, 7, 0)
    ref = ctypes.byref(d)
    inside = []
    fake.effects["vs_thing"] = lambda *a: inside.append(list(fake.guards))
    assert _call.call("thing", "cuda:1", ref, t, None, 7, 2.5, d) is None
    (name, args), = fake.calls
    assert name == "vs_thing" and len(args) == 7
    assert args[0] is ref and args[5] is d                                       # structures: as they are
    assert isinstance(args[1], ctypes.c_void_p) and args[1].value == t.data_ptr()
    assert isinstance(args[2], ctypes.c_void_p) and args[2].value is None        # NULL
    assert args[3] == 7 and type(args[3]) is int and args[4] == 2.5 and type(args[4]) is float
    assert args[6] is STREAM                                                     # the stream, last
    assert inside == [[("enter", "cuda:1")]]                                     # the library ran inside the guard
    assert fake.guards == [("enter", "cuda:1"), ("exit", "cuda:1")]


def test_call_raises_with_the_last_error_and_the_label(fake):
    from voicesplit_amd import _call
    from voicesplit_amd._lib import VoiceSplitHipError
    fake.rc["vs_thing"] = -3
    with pytest.raises(VoiceSplitHipError) as e:
        _call.call("thing", "cuda:0", 1)
    assert str(e.value) == "vs_thing failed (rc=-3): the reason"
    with pytest.raises(VoiceSplitHipError) as e:
        _call.call("thing", "cuda:0", 1, what="vs_thing(dgrad)")
    assert str(e.value) == "vs_thing(dgrad) failed (rc=-3): the reason"
    assert fake.guards[-1] == ("exit", "cuda:0")                                 # the guard is left before the error is raised


def test_sized_returns_the_size_and_raises_on_zero(fake):
    from voicesplit_amd import _call
    from voicesplit_amd._lib import VoiceSplitHipError
    assert _call.sized("thing_bytes", 3, 4) == 128
    assert fake.calls == [("vs_thing_bytes", (3, 4))] and fake.guards == []      # a sizer takes no stream and needs no guard
    fake.rc["vs_thing_bytes"] = 0
    with pytest.raises(VoiceSplitHipError) as e:
        _call.sized("thing_bytes", 3, 4)
    assert str(e.value) == "vs_thing_bytes failed (rc=-1): the reason"
    with pytest.raises(VoiceSplitHipError, match=r"vs_thing_bytes\(B=3\) failed \(rc=-1\): the reason"):
        _call.sized("thing_bytes", 3, 4, what="vs_thing_bytes(B=3)")


def test_scratch_grows_only_and_keeps_slots_and_devices_apart(fake, monkeypatch):
    from voicesplit_amd import _call
    made = []

    def empty(n, dtype, device):             # no second device here: the registry's bookkeeping is what is under test
        made.append((n, str(device)))
        return torch.zeros(n, dtype=dtype)

    monkeypatch.setattr(torch, "empty", empty)
    a = _call.scratch("model", 100, "cuda:0")
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert _call.scratch("model", 100, "cuda:0") is a and _call.scratch("model", 7, torch.device("cuda:0")) is a
    b = _call.scratch("model", 101, "cuda:0")
    assert b is not a and b.numel() == 101 and _call.scratch("model", 100, "cuda:0") is b
    c, d = _call.scratch("loss", 5, "cuda:0"), _call.scratch("model", 9, "cuda:1")
    assert c is not b and d is not b and _call.scratch("model", 1, "cuda:0") is b
    assert made == [(100, "cuda:0"), (101, "cuda:0"), (5, "cuda:0"), (9, "cuda:1")]
    assert _call.scratch_bytes() == 101 + 5 + 9 and _call.scratch_bytes("cuda:0") == 106 and _call.scratch_bytes("cuda:1") == 9
    with pytest.raises(KeyError):
        _call.scratch("nobody", 1, "cuda:0")
    assert set(_call.SLOTS) >= {"model", "multi", "loss", "audio", "deemph", "metric", "logmel", "embed"}
    _call.release_scratch()
    assert _call.scratch_bytes() == 0


def test_release_workspaces_empties_every_slot_and_the_tape_pool(fake):
    from voicesplit_amd import _call, ops
    for slot in _call.SLOTS:
        _call.scratch(slot, 64, "cpu")
    ops.recycle_tape(torch.zeros(32, dtype=torch.uint8))
    assert _call.scratch_bytes() == 64 * len(_call.SLOTS) and ops.tape_pool_bytes() == 32
    ops.release_workspaces()
    assert _call.scratch_bytes() == 0 and ops.tape_pool_bytes() == 0


def _bf16(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def _zero_state(xg, packed, state, *rest):
    ctypes.memset(state.value, 0, 128 * 4)       # the word _lstm_check_err reads: the kernels leave it 0


@pytest.mark.parametrize("family", ["gemm_bf16", "sigmoid_bwd", "nhwc_bn_apply", "bilstm_recurrent"])
def test_kernel_level_wrappers_enter_the_guard_with_their_tensors_device(fake, family):
    from voicesplit_amd import ops
    fake.effects["vs_bilstm_recurrent"] = _zero_state
    first = {"gemm_bf16": _bf16(64, 64), "sigmoid_bwd": torch.zeros(2, 5), "nhwc_bn_apply": _bf16(3, 64), "bilstm_recurrent": torch.zeros(1, 2, 16)}[family]
    if family == "gemm_bf16":
        ops.gemm_bf16(first, _bf16(64, 64), 64, 64, 64)
    elif family == "sigmoid_bwd":
        ops.sigmoid_bwd(first, torch.zeros(2, 5))
    elif family == "nhwc_bn_apply":
        ops.nhwc_bn_apply(first, torch.zeros(64), torch.zeros(64), "mish")
    else:
        ops.bilstm_recurrent(first, torch.zeros(8, 2), torch.zeros(8, 2))
    streamed = [(n, a) for n, a in fake.calls if not n.endswith(("_floats", "_bytes"))]
    assert [n for n, _ in streamed] == {"bilstm_recurrent": ["vs_lstm_pack", "vs_bilstm_recurrent"]}.get(family, ["vs_" + family])
    assert all(a[-1] is STREAM for _, a in streamed)
    assert first.data_ptr() in [a.value for a in streamed[-1][1] if isinstance(a, ctypes.c_void_p)]
    assert fake.guards == [(k, first.device) for _ in streamed for k in ("enter", "exit")]
