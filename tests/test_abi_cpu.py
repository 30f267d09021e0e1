"""CPU: the C-ABI library loads and exports every symbol include/voicesplit_hip.h declares; the
host-side mirror of the reference interface behaves (no compute calls here -- no GPU)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from oracle import reference_forward as R


def _header_functions():
    text = open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from voicesplit_amd import _lib
    lib = _lib.load()
    names = _header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(_lib.SIGNATURES) == names
    assert lib.vs_abi_version() == _lib.ABI_VERSION


def test_library_exports_nothing_but_the_header():
    """-fvisibility=hidden: the dynamic symbol table holds the header's functions and the compiler's own
    __hip_cuid_* / fatbin bookkeeping, no internal launcher, kernel stub or helper."""
    import subprocess
    from voicesplit_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = [l.split()[-1] for l in out.splitlines() if l.strip()]
    extra = [s for s in syms if s not in set(_header_functions()) and not s.startswith("__hip_")]
    assert not extra, f"unexpected exports: {extra[:10]}"


def test_workspace_layout_and_argument_errors():
    from voicesplit_amd import _lib, ops
    lib = _lib.load()
    d = ops.make_dims(64, 301, 601, 256, 400, 600, 601)
    lay = ops.workspace_layout(d)
    assert lay.total_bytes == lib.vs_workspace_bytes(ctypes.byref(d))
    act = 64 * 64 * 301 * 601 * 4
    assert lay.act1 - lay.act0 >= act and lay.total_bytes > 2 * act
    offs = [lay.act0, lay.act1, lay.feat, lay.dvbias, lay.xg, lay.lstm_out, lay.fc1_out, *lay.conv_packed,
            lay.bn_scale, lay.bn_shift, lay.bn_stats, lay.lstm_packed, lay.lstm_state]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    # bad arguments: error code + message, no exception across the ABI
    bad = ops.make_dims(1, 10, 37, 16, 30, 40, 37)          # H not a multiple of 8
    assert lib.vs_workspace_bytes(ctypes.byref(bad)) == 0
    assert b"multiple of 8" in lib.vs_last_error()
    with pytest.raises(_lib.VoiceSplitHipError):
        ops.workspace_layout(bad)
    # prepared eval-mode weights: a function of the model dimensions and the arithmetic, not of B or T
    pb = lib.vs_prepared_bytes(ctypes.byref(d))
    assert pb == lib.vs_prepared_bytes(ctypes.byref(ops.make_dims(1, 17, 601, 256, 400, 600, 601))) and pb % 256 == 0
    kp = (8 * 601 + 63) // 64 * 64          # VS_GEMM_KPAD
    assert 2 * 8 * 400 * kp * 2 < pb < 2 * 8 * 400 * kp * 2 + 16 * 2 ** 20        # the split W_ih halves dominate (62 MB)
    assert lib.vs_prepared_bytes(ctypes.byref(bad)) == 0
    assert lib.vs_prepare_weights(ctypes.byref(d), None, None, 0, None) != 0 and b"NULL" in lib.vs_last_error()
    assert lib.vs_set_backward_overlap(2) == -1 and lib.vs_set_backward_overlap(1) == 0
    assert lib.vs_conv64_packed_floats(5, 5) == (8 * 25 + 4) * 512   # + 4 dummy taps for the prefetch overrun
    # fp32 fragment form + room for the two f16 planes of the math-selected recurrence + a 64-float header
    assert lib.vs_lstm_packed_floats(400) == 2 * 1600 * 400 + 2 * 1600 * 400 + 64
    assert lib.vs_lstm_packed_t_floats(400) == 2 * 13 * 200 * 256 + 2 * 13 * 100 * 256 + 64
    # the *_math entry points of the recurrence refuse an unknown arithmetic and NULL buffers before touching the device
    assert lib.vs_lstm_pack_math(None, None, None, 400, 7, None) != 0 and b"unknown math" in lib.vs_last_error()
    assert lib.vs_lstm_pack_math(None, None, None, 400, 2, None) != 0 and b"NULL" in lib.vs_last_error()
    assert lib.vs_bilstm_recurrent_math(None, None, None, None, None, None, 1, 1, 8, 1, None) != 0 and b"NULL" in lib.vs_last_error()
    assert lib.vs_bilstm_recurrent_bwd_math(None, None, None, None, None, 1, 1, 8, 9, None) != 0 and b"unknown math" in lib.vs_last_error()
    assert lib.vs_nhwc_conv_last_pre(None, None, None, 2, None, None, None, None, None, 1, 1, 8, None) != 0 and b"NULL" in lib.vs_last_error()
    # the exported BatchNorm finalize refuses NULL statistics / constants and half a pair of running buffers before any launch
    assert lib.vs_bn_finalize(None, 64, 1000.0, 64, None, None, None, None, 1e-5, 0.1, None, None, None, None, None) != 0
    assert b"bn_finalize" in lib.vs_last_error()
    one = ctypes.c_void_p(256)
    assert lib.vs_bn_finalize(one, 64, 1000.0, 64, one, one, one, None, 1e-5, 0.1, one, one, None, None, None) != 0 and b"both running" in lib.vs_last_error()
    assert lib.vs_bn_finalize(one, 64, 1000.0, 64, one, one, None, None, 1e-5, 1.5, one, one, None, None, None) != 0 and b"momentum" in lib.vs_last_error()
    # the channels-last split-f16 layer (round 4): scratch = two packed f16 planes + 1 KiB of row norms / scale / plan, which every
    # mid-layer region of the workspace has room for; NULL, in-place and foreign kernel shapes are refused before any launch
    assert lib.vs_nhwc_conv_f16x3_scratch_bytes(5, 5) == 2 * 64 * 64 * 25 * 2 + 1024
    assert all(lay.conv_packed[i + 1] - lay.conv_packed[i] >= lib.vs_nhwc_conv_f16x3_scratch_bytes(5, 5) for i in range(1, 5))
    assert lay.conv_packed[1] - lay.conv_packed[0] >= lib.vs_nhwc_conv_f16x3_scratch_bytes(7, 1)
    assert lib.vs_nhwc_conv_f16x3_layer(None, None, None, None, 1, None, None, None, None, 0, None, None, None, None,
                                        1, 4, 4, 5, 5, 1, 1, None) != 0 and b"NULL" in lib.vs_last_error()
    two = ctypes.c_void_p(512)
    assert lib.vs_nhwc_conv_f16x3_layer(one, two, one, one, 1, one, one, one, one, 0, one, two, one, None,
                                        1, 4, 4, 5, 5, 1, 1, None) != 0 and b"in-place" in lib.vs_last_error()
    three, four = ctypes.c_void_p(768), ctypes.c_void_p(1024)
    assert lib.vs_nhwc_conv_f16x3_layer(one, two, one, one, 1, one, one, one, one, 0, three, four, one, None,
                                        1, 4, 4, 3, 3, 1, 1, None) != 0 and b"7x1, 5x5" in lib.vs_last_error()
    assert lib.vs_f16x3_split(None, None, None, None, 8, None) != 0 and lib.vs_f16x3_merge(None, None, None, None, 8, None) != 0
    assert lib.vs_set_lstm_kernel(3) == 0 and lib.vs_set_lstm_kernel(4) == 0 and lib.vs_set_lstm_kernel(5) != 0 and lib.vs_set_lstm_kernel(0) == 0
    # four exchange regions (the tagged hand-off of round 5), sized for the 16-wide K chunks of the f16 form (H = 24 -> 32)
    assert lib.vs_lstm_state_floats(3, 24) == 4 * 2 * 32 * 32 + 64 and lib.vs_lstm_state_floats(64, 400) == 4 * 2 * 400 * 64 + 64


def test_gemm_entry_points_refuse_bad_descriptors_before_any_launch():
    """Every refusal of the GEMM checks that the exported calls can reach, one call per condition, over aligned fake pointers:
    each is refused before a launch, with the message of its kernel's prefix (gemm:, gemm_f16x3:, gemm_bf16:)."""
    from voicesplit_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    NONE, MISH = 2, 1

    def refused(rc, fragment):
        assert rc != 0 and fragment in lib.vs_last_error(), (rc, fragment, lib.vs_last_error())

    def gemm(split=False, **kw):
        a = dict(la=0, lw=0, lda=32, ldw=32, ldc=24, M=16, N=24, K=32, bias=None, gate=None, ldg=0, a_relu=0, w_relu=0, act=NONE, acc=0,
                 w_shift=0, w_group=0, splits=1, partials=None)
        a.update(kw)
        head = (a["la"], a["lw"], p, a["lda"], p, a["ldw"], p, a["ldc"], a["M"], a["N"], a["K"], a["bias"], a["gate"], a["ldg"],
                a["a_relu"], a["w_relu"], a["act"], a["acc"])
        if split:
            return lib.vs_gemm_f16x3(*head, p, None)
        return lib.vs_gemm(*head, a["w_shift"], a["w_group"], a["splits"], a["partials"], None)

    # the checks both kernels share, under either prefix.  (vs_gemm_f16x3 with a bad shape: refused before its two scale passes)
    for split, pre in ((False, b"gemm: "), (True, b"gemm_f16x3: ")):
        refused(gemm(split, M=0), pre + b"bad shape")
        refused(gemm(split, N=-1), pre + b"bad shape")
        refused(gemm(split, la=2), pre + b"bad layout")
        refused(gemm(split, lw=-1), pre + b"bad layout")
        refused(gemm(split, lda=31), pre + b"leading dims")                 # K-contiguous A: lda >= K
        refused(gemm(split, la=1, lda=15), pre + b"leading dims")           # K-major A: lda >= M
        refused(gemm(split, ldw=31), pre + b"leading dims")                 # K-contiguous W: ldw >= K
        refused(gemm(split, lw=1, ldw=23), pre + b"leading dims")           # K-major W: ldw >= N
        refused(gemm(split, ldc=23), pre + b"leading dims")
        refused(gemm(split, gate=p, ldg=23), pre + b"gate needs ldg>=N")
        refused(gemm(split, act=MISH), pre + b"unsupported activation 1")
    # the fp32 kernel's own
    refused(gemm(M=65535 * 128 + 1), b"gemm: M=8388481 too large")
    refused(gemm(w_group=4, w_shift=1), b"gemm: w_shift/w_group need the K-major W layout")
    splitk = b"gemm: split-K needs a partial buffer, a dense C and no epilogue terms"
    refused(gemm(splits=2, partials=p, bias=p), splitk)
    refused(gemm(splits=2, partials=p, gate=p, ldg=24), splitk)
    refused(gemm(splits=2, partials=p, acc=1), splitk)
    refused(gemm(splits=2, partials=p, act=0), splitk)
    refused(gemm(splits=2, partials=p, ldc=32), splitk)
    refused(gemm(splits=2), splitk)                                         # NULL partials
    refused(lib.vs_gemm(0, 0, None, 32, p, 32, p, 24, 16, 24, 32, None, None, 0, 0, 0, NONE, 0, 0, 0, 1, None, None), b"gemm: NULL argument")
    # the split kernel's own: 32-bit offsets of its operands, its tile raster
    refused(gemm(True, la=1, lda=1 << 30, K=2, ldw=2), b"gemm_f16x3: K-major A above 4 GiB")
    refused(gemm(True, lw=1, ldw=1 << 30, K=2, lda=2), b"gemm_f16x3: K-major W above 4 GiB")
    refused(gemm(True, lda=1 << 30), b"gemm_f16x3: A above 4 GiB")
    refused(gemm(True, ldw=1 << 30), b"gemm_f16x3: W above 4 GiB")
    refused(gemm(True, M=1 << 22, N=1 << 22, K=1, lda=1, ldw=1, ldc=1 << 22), b"gemm_f16x3: too many tiles")
    refused(lib.vs_gemm_f16x3(0, 0, p, 32, p, 32, p, 24, 16, 24, 32, None, None, 0, 0, 0, NONE, 0, None, None), b"gemm_f16x3: NULL argument")

    # the row bias is reachable through vs_gemm_nt
    def gemm_nt(**kw):
        a = dict(M=16, N=24, K=32, ldrb=24, group=4)
        a.update(kw)
        return lib.vs_gemm_nt(p, 32, p, 32, p, 24, a["M"], a["N"], a["K"], None, None, p, a["ldrb"], a["group"], 0, NONE, None)

    refused(gemm_nt(group=0), b"gemm: rowbias needs group>0 and ldrb>=N")
    refused(gemm_nt(ldrb=23), b"gemm: rowbias needs group>0 and ldrb>=N")
    refused(gemm_nt(K=0), b"gemm: bad shape M=16 N=24 K=0")

    # the bf16-operand kernel: operands [16][64] x [24][64] (row forms padded to 64 in k)
    def gemm_bf16(**kw):
        a = dict(ak=0, bk=0, A=p, lda=64, B=p, ldb=64, M=16, N=24, K=40, rowbias=None, ldrb=0, group=1)
        a.update(kw)
        return lib.vs_gemm_bf16(a["ak"], a["bk"], a["A"], a["lda"], a["B"], a["ldb"], p, 24, a["M"], a["N"], a["K"],
                                a["rowbias"], a["ldrb"], a["group"], 0, None)

    aligned = b"gemm_bf16: operands must be 16-byte aligned with ld a multiple of 8"
    refused(gemm_bf16(M=0), b"gemm_bf16: bad argument")
    refused(gemm_bf16(A=None), b"gemm_bf16: bad argument")
    refused(gemm_bf16(A=ctypes.c_void_p(264)), aligned)
    refused(gemm_bf16(B=ctypes.c_void_p(258)), aligned)
    refused(gemm_bf16(lda=68), aligned)
    refused(gemm_bf16(ldb=68), aligned)
    refused(gemm_bf16(rowbias=p, ldrb=24, group=0), b"gemm_bf16: rowbias needs group > 0 and ldrb >= N")
    refused(gemm_bf16(rowbias=p, ldrb=23, group=4), b"gemm_bf16: rowbias needs group > 0 and ldrb >= N")
    refused(gemm_bf16(K=65), b"gemm_bf16: row-form A must be padded to a multiple of 64 in k")
    refused(gemm_bf16(K=65, lda=128), b"gemm_bf16: row-form B must be padded to a multiple of 64 in k")
    refused(gemm_bf16(ak=1, lda=16), b"gemm_bf16: the col x row form is not used by the path")
    refused(lib.vs_gemm_bf16_gated(0, 0, p, 64, p, 64, p, 24, 16, 24, 40, p, 23, None), b"gemm_bf16: gate needs ldg >= N and a single output")
    refused(lib.vs_gemm_bf16_gated(0, 0, p, 64, p, 68, p, 24, 16, 24, 40, p, 24, None), aligned)
    refused(lib.vs_gemm_bf16_split(0, 0, p, 64, p, 64, p, p, 24, 8, 16, 24, 65, 0, None), b"gemm_bf16: row-form A must be padded")
    refused(lib.vs_gemm_bf16_split(0, 0, p, 64, p, 64, p, p, 24, 8, 16, 0, 40, 0, None), b"gemm_bf16: bad argument")


def test_missing_library_fails_loudly(tmp_path):
    from voicesplit_amd import _lib
    with pytest.raises(_lib.VoiceSplitHipError, match="no PyTorch/CPU fallback"):
        _lib.load(str(tmp_path / "libvoicesplit_hip.so"))


@pytest.mark.parametrize("cls_name", ["VoiceSplit", "VoiceFilter"])
def test_module_surface_matches_reference(cls_name):
    import voicesplit_amd
    from models.voicefilter.model import VoiceFilter   # reference import paths (train.py:21-22)
    from models.voicesplit.model import VoiceSplit
    cls = {"VoiceSplit": VoiceSplit, "VoiceFilter": VoiceFilter}[cls_name]
    assert cls is getattr(voicesplit_amd, cls_name)
    dims = R.default_dims()
    torch.manual_seed(0)
    m = cls(voicesplit_amd.default_config())
    ref = R.build_state_dict(dims, 0, randomize_bn=False)
    sd = m.state_dict()
    assert list(sd) == list(ref)                         # same keys, same order
    for k in sd:
        assert sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype, k
        assert torch.equal(sd[k], ref[k]), k              # same default init under the same seed
    assert sum(p.numel() for p in m.parameters()) == 18876001
    m.load_state_dict(R.build_state_dict(dims, 3), strict=True)
    assert m.training and not m.eval().training
    # CPU tensors are refused, not silently computed some other way
    from voicesplit_amd._lib import VoiceSplitHipError
    with pytest.raises(VoiceSplitHipError, match="no CPU fallback"):
        m(torch.rand(1, 4, 601), torch.rand(1, 256))


REFERENCE_FORMAT_CONFIG = """{
    "model_name":"voicesplit", // or voicefilter
    "loss":{
        "loss_name":"si_snr", // or power_law_compression
        "power": 0.30,
        "complex_loss_ratio":0.113 // weight of the complex term
    },
    "train_config": {
        "learning_rate": 1e-2,
        "optimizer":"adam",
        "batch_size": 2,
        "reinit_layers": null
    },
    "model":{
        "lstm_dim": 400,
        "fc1_dim": 600,
        "fc2_dim": 601, // one mask value per frequency bin
        "emb_dim": 256 // d-vector size
    },
    "audio": {
        "backend":"voicefilter", // the STFT front end
        "audio_len": 3,
        "voicefilter":{
            "n_fft": 1200,
            "num_freq": 601, // n_fft / 2 + 1
            "sample_rate": 16000,
            "hop_length": 160,
            "win_length": 400,
            "min_level_db": -100.0,
            "ref_level_db": 20.0
        }
    }
}
"""


def test_reference_config_json_is_accepted(tmp_path):
    """A config.json in the reference's own format: JSON with // comments after values and after the last value of a block."""
    from voicesplit_amd import VoiceSplit, load_config
    path = tmp_path / "config.json"
    path.write_text(REFERENCE_FORMAT_CONFIG)
    c = load_config(str(path))
    m = VoiceSplit(c)
    assert m.lstm.input_size == 8 * 601 + 256 and m.fc2.out_features == 601


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "voicesplit_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "oracle/" not in text and "reference_forward" not in text, f


def test_tensor_index_follows_the_module_tree_and_transients_stay_out_of_copies():
    """The cached (key, owning dict, name) index behind every C-ABI call is rebuilt when the module tree changes below
    the top level too, and caches / foreign views do not travel with deepcopy or pickling."""
    import copy
    import pickle
    import voicesplit_amd as V
    m = V.VoiceSplit(V.default_config(37, 16, 24, 40, 37))
    t0 = m._tensors()
    assert list(t0) == list(m.state_dict())
    old_w = m.conv[5].weight
    m.conv[5] = torch.nn.Conv2d(64, 64, kernel_size=(7, 1))           # a child of a child replaced: Sequential.__setitem__
    assert m._tensors()["conv.5.weight"] is m.conv[5].weight and m._tensors()["conv.5.weight"] is not old_w
    m.fc1.register_buffer("extra_stat", torch.zeros(3))               # a buffer registered on a child
    assert "fc1.extra_stat" in m._tensors()
    m.fc1.register_buffer("scratch", torch.zeros(3), persistent=False)
    assert "fc1.scratch" not in m._tensors()                          # state_dict() semantics: persistent buffers only
    m.lstm.weight_hh_l0 = torch.nn.Parameter(torch.zeros_like(m.lstm.weight_hh_l0))   # a replaced tensor is read through the dict
    assert m._tensors()["lstm.weight_hh_l0"] is m.lstm.weight_hh_l0
    assert [k for k, _ in m._named_params()] == [k for k, _ in m.named_parameters()]
    m.fc1.add_module("probe", torch.nn.Linear(2, 2))                  # a NEW grandchild: no existing link changes
    assert "fc1.probe.weight" in m._tensors() and list(m._tensors()) == list(m.state_dict())
    del m.fc1._modules["probe"]
    assert "fc1.probe.weight" not in m._tensors() and list(m._tensors()) == list(m.state_dict())
    # the recurrence's error word lives in the tape: with no training forward behind the module (or its tape released) the
    # status is unknown, never "OK"
    assert V.VoiceSplit(V.default_config(37, 16, 24, 40, 37)).lstm_status() is None
    # transients
    m.__dict__["_last_tape"] = ("tape", "dims")
    m.set_gradient_sink({"fc1.weight": torch.zeros_like(m.fc1.weight)})
    m.__dict__["_prepared"] = object()
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert not any(k in c.__dict__ for k in m._TRANSIENT)
        assert list(c._tensors()) == list(m._tensors()) and c._tensors()["fc2.weight"] is c.fc2.weight
    assert "_grad_sink" in m.__dict__
    m.set_gradient_sink(None)
    assert "_grad_sink" not in m.__dict__


# ---- the STFT entry points: geometries the library refuses, and the envelope cache -------------------------------------------
def _loss_dims(n_fft, hop, win, F=None, B=2, T=9):
    from voicesplit_amd import _lib
    return _lib.VsLossDims(B, T, n_fft // 2 + 1 if F is None else F, n_fft, hop, win, -100.0, 20.0)


def _stft_calls():
    """name -> call(dims, ws_bytes) -> (rc, message).  Every pointer is a dummy that is never dereferenced: each call of the tests
    below is refused before any device work."""
    from voicesplit_amd import _lib
    lib = _lib.load()
    p, ws = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    big = 1 << 40

    def answer(rc):
        return rc, lib.vs_last_error()

    return lib, {
        "vs_sisnr_workspace_bytes": lambda d, n=big: answer(0 if lib.vs_sisnr_workspace_bytes(ctypes.byref(d)) else -1),
        "vs_sisnr_loss": lambda d, n=big: answer(lib.vs_sisnr_loss(ctypes.byref(d), p, p, p, p, None, ws, n, p, None, None, None)),
        "vs_spec_to_wav": lambda d, n=big: answer(lib.vs_spec_to_wav(ctypes.byref(d), p, None, p, p, ws, n, None)),
        "vs_wav_to_spec": lambda d, n=big: answer(lib.vs_wav_to_spec(ctypes.byref(d), p, p, p, ws, n, None)),
        "vs_wav_to_logmel": lambda d, n=big: answer(lib.vs_wav_to_logmel(ctypes.byref(d), p, 4000, p, 40, p, ws, n, None)),
    }


@pytest.mark.parametrize("name", ["vs_sisnr_workspace_bytes", "vs_spec_to_wav", "vs_wav_to_spec", "vs_wav_to_logmel"])
def test_stft_entry_points_refuse_a_geometry_they_cannot_serve(name):
    """hop > win, win > n_fft and F != n_fft / 2 + 1: a non-zero return (0 bytes from the size function) and the message that
    names the rule, from every entry point that takes a vs_loss_dims."""
    _lib_, calls = _stft_calls()
    call = calls[name]
    for dims, text in ((_loss_dims(64, 17, 16), b"need hop <= win <= n_fft"),
                       (_loss_dims(64, 16, 65), b"need hop <= win <= n_fft"),
                       (_loss_dims(64, 16, 64, F=32), b"must be n_fft/2+1"),
                       (_loss_dims(64, 16, 64, F=34), b"must be n_fft/2+1")):
        rc, msg = call(dims)
        assert rc != 0 and text in msg, (name, dims.n_fft, dims.hop, dims.win, dims.F, rc, msg)
    # the limits themselves are legal: hop == win == n_fft passes the shape rules (what refuses it next is the envelope, below)
    assert _lib_.vs_sisnr_workspace_bytes(ctypes.byref(_loss_dims(64, 64, 64))) > 0


def test_no_overlap_is_refused_and_the_envelope_cache_follows_the_geometry():
    """hop == win leaves samples under a zero of the Hann window: vs_spec_to_wav (periodic window) and vs_sisnr_loss (symmetric)
    refuse it with "envelope".  vs_stft_check_envelope keeps the last shape's minimum in a thread-local cache keyed on (hop, win, T,
    periodic); three calls in a row that end at the workspace check when the envelope check has passed show that the cache is
    invalidated in both directions."""
    _lib_, calls = _stft_calls()
    bad, good = _loss_dims(64, 64, 64), _loss_dims(64, 16, 64)
    for name in ("vs_spec_to_wav", "vs_sisnr_loss"):
        rc, msg = calls[name](bad)
        assert rc != 0 and b"envelope" in msg and b"hop=64 win=64" in msg, (name, msg)
    for dims, text in ((good, b"workspace too small"), (bad, b"envelope"), (good, b"workspace too small"), (good, b"workspace too small")):
        rc, msg = calls["vs_spec_to_wav"](dims, 256)
        assert rc != 0 and text in msg, (dims.hop, msg)
    # the same T and hop with another window, and the two window forms of one geometry, are different cache entries
    rc, msg = calls["vs_spec_to_wav"](_loss_dims(64, 16, 16), 256)
    assert rc != 0 and b"envelope" in msg and b"periodic" in msg
    rc, msg = calls["vs_sisnr_loss"](_loss_dims(64, 16, 16), 256)
    assert rc != 0 and b"envelope" in msg and b"symmetric" in msg
    rc, msg = calls["vs_sisnr_loss"](good, 256)
    assert rc != 0 and b"workspace too small" in msg
