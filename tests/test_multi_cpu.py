"""CPU: the multi-speaker entry points (vs_multi_workspace_bytes, vs_bilstm_fwd_multi, vs_forward_prepared_multi) are declared,
exported and bound; their argument errors come back as error code + message before anything touches a device; the Python
surface refuses what it must and orders the B*K rows as documented (no compute calls here -- no GPU)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

MULTI = ("vs_multi_workspace_bytes", "vs_bilstm_fwd_multi", "vs_forward_prepared_multi")


def _dims(B=2, T=20, math=None):
    from voicesplit_amd import ops
    return ops.make_dims(B, T, 601, 256, 400, 600, 601, math)


def test_prototypes_in_header_library_and_ctypes_table():
    from voicesplit_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voicesplit_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in MULTI:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert re.search(r"#define\s+VS_ABI_VERSION\s+11\b", text)
    assert lib.vs_abi_version() == 11 and _lib.ABI_VERSION == 11          # additive entries under the unchanged version
    # argument counts of the bindings = those of the declarations
    for name in MULTI:
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_argument_errors_are_codes_and_messages():
    from voicesplit_amd import _lib
    lib = _lib.load()
    d = _dims()
    one = ctypes.c_void_p(256)
    # K = 0
    assert lib.vs_multi_workspace_bytes(ctypes.byref(d), 0) == 0 and b"K=0" in lib.vs_last_error()
    assert lib.vs_forward_prepared_multi(ctypes.byref(d), None, None, 0, one, one, 0, None, 1, None, 0, one, None) != 0
    assert b"K=0" in lib.vs_last_error()
    assert lib.vs_bilstm_fwd_multi(ctypes.byref(d), None, one, one, 0, None, None, 0, one, None) != 0 and b"K=0" in lib.vs_last_error()
    assert lib.vs_bilstm_fwd_multi(ctypes.byref(d), None, one, one, -3, None, None, 0, one, None) != 0 and b"K=-3" in lib.vs_last_error()
    # NULL dvecs
    assert lib.vs_forward_prepared_multi(ctypes.byref(d), None, None, 0, one, None, 2, None, 1, None, 0, one, None) != 0
    assert b"dvecs is NULL" in lib.vs_last_error()
    assert lib.vs_bilstm_fwd_multi(ctypes.byref(d), None, one, None, 2, None, None, 0, one, None) != 0 and b"dvecs is NULL" in lib.vs_last_error()
    # VS_MATH_FP32 has no shared-input recurrence
    f = _dims(math="fp32")
    assert lib.vs_forward_prepared_multi(ctypes.byref(f), None, None, 0, one, one, 2, None, 1, None, 0, one, None) != 0
    assert b"VS_MATH_FP32" in lib.vs_last_error()
    assert lib.vs_bilstm_fwd_multi(ctypes.byref(f), None, one, one, 2, None, None, 0, one, None) != 0 and b"VS_MATH_FP32" in lib.vs_last_error()
    # then the usual ones: NULL outputs, prepared blob, workspace
    assert lib.vs_forward_prepared_multi(ctypes.byref(d), None, None, 0, one, one, 2, None, 1, None, 0, None, None) != 0
    assert b"mask is NULL" in lib.vs_last_error()
    assert lib.vs_forward_prepared_multi(ctypes.byref(d), None, None, 0, one, one, 2, None, 1, None, 0, one, None) != 0
    assert b"prepared weights" in lib.vs_last_error()
    assert lib.vs_bilstm_fwd_multi(ctypes.byref(d), None, one, one, 2, None, None, 0, one, None) != 0 and b"workspace is NULL" in lib.vs_last_error()
    assert lib.vs_bilstm_fwd_multi(ctypes.byref(d), None, one, one, 2, None, one, 1024, one, None) != 0 and b"too small" in lib.vs_last_error()
    bad = _dims()
    bad.H = 30
    assert lib.vs_multi_workspace_bytes(ctypes.byref(bad), 2) == 0 and b"multiple of 8" in lib.vs_last_error()


def test_workspace_grows_with_k_but_not_its_conv_buffers():
    from voicesplit_amd import _lib
    lib = _lib.load()
    for B, T in ((1, 301), (64, 301), (3, 37)):
        d = _dims(B, T)
        base = lib.vs_workspace_bytes(ctypes.byref(d))
        sizes = [lib.vs_multi_workspace_bytes(ctypes.byref(d), K) for K in range(1, 10)]
        assert sizes[0] >= base > 0
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        # per extra speaker: row bias, recurrence state, LSTM output and fc1 scratch of B sequences -- far below a conv buffer for B
        step = sizes[8] - sizes[7]
        per_seq = T * (2 * 400 + 600) * 4
        tiles = B // 32 + 2                              # 32-column batch tiles of recurrence state an extra B sequences can add
        assert B * per_seq <= step <= B * per_seq + B * 8 * 400 * 4 + tiles * 4 * lib.vs_lstm_state_floats(32, 400) + 4096
        assert sizes[8] - base < 2 * B * 64 * T * 601 * 4          # nine speakers add less than the two conv buffers of B mixtures


def _cpu_model():
    import voicesplit_amd as V
    return V.VoiceSplit(V.default_config(37, 16, 24, 40, 37))


def test_forward_multi_refuses_train_mode_grad_and_mismatched_embeddings():
    m = _cpu_model()
    x, e = torch.rand(2, 5, 37), torch.rand(2, 3, 16)
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval mode"):
        m.forward_multi(x, e)
    m.eval()
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_multi(x, e)
    with torch.no_grad():
        with pytest.raises(ValueError, match="speaker_embeddings"):
            m.forward_multi(x, e[:1])                          # leading dimension differs from x's
        with pytest.raises(ValueError, match="speaker_embeddings"):
            m.forward_multi(x, e[:, 0])                        # [B, E]: that is forward()'s argument
        from voicesplit_amd._lib import VoiceSplitHipError
        with pytest.raises(VoiceSplitHipError, match="no CPU fallback"):
            m.forward_multi(x, e)                              # CPU tensors are refused, not computed some other way


class _StubModel:
    """forward_multi -> mask[b, k] = 10 b + k + 1 everywhere; records what it was given."""

    def forward_multi(self, spec, dvecs, lengths=None):
        self.spec_shape, self.dvecs = tuple(spec.shape), dvecs
        B, K = dvecs.shape[0], dvecs.shape[1]
        tag = (10.0 * torch.arange(B)[:, None] + torch.arange(K)[None, :] + 1.0)
        return tag[:, :, None, None].expand(B, K, spec.shape[1], spec.shape[2]).contiguous()


def test_separate_speakers_orders_rows_by_mixture_then_speaker(monkeypatch):
    """The host side of ``audio.separate_speakers`` with the device calls stubbed: one STFT of the B mixtures, one forward_multi,
    one iSTFT over B*K rows in which row b*K + k carries mixture b's spectrogram and phase and speaker k's mask."""
    from voicesplit_amd import audio
    acfg = {"hop_length": 4, "n_fft": 8}
    calls = []

    def wav_to_spec(wav, cfg, want_phase=True):
        B, n = wav.shape
        T, F = n // cfg["hop_length"] + 1, cfg["n_fft"] // 2 + 1
        spec = wav[:, :1, None].expand(B, T, F).contiguous()               # mixture b's spectrogram holds wav[b, 0]
        calls.append(("stft", B))
        return spec, -spec

    def spec_to_wav(spec, phase, cfg, mask=None):
        calls.append(("istft", spec.shape[0]))
        assert spec.is_contiguous() and phase.is_contiguous() and mask.is_contiguous()
        assert torch.equal(phase, -spec)
        n = cfg["hop_length"] * (spec.shape[1] - 1)
        return (spec[:, 0, 0] * 1000.0 + mask[:, 0, 0])[:, None].expand(spec.shape[0], n).contiguous()

    monkeypatch.setattr(audio, "wav_to_spec", wav_to_spec)
    monkeypatch.setattr(audio, "spec_to_wav", spec_to_wav)
    B, K, n = 3, 2, 12
    wav = (torch.arange(B, dtype=torch.float32)[:, None] + 1.0).expand(B, n).contiguous()       # wav[b] = b + 1
    dvecs = torch.rand(B, K, 16)
    stub = _StubModel()
    est = audio.separate_speakers(stub, wav, dvecs, acfg)
    assert calls == [("stft", B), ("istft", B * K)]
    assert stub.spec_shape == (B, 4, 5) and stub.dvecs is dvecs
    assert tuple(est.shape) == (B, K, n)
    for b in range(B):
        for k in range(K):
            assert torch.all(est[b, k] == (b + 1) * 1000.0 + 10.0 * b + k + 1.0), (b, k)
    with pytest.raises(ValueError, match="dvecs must be"):
        audio.separate_speakers(stub, wav, dvecs[:2], acfg)
    with pytest.raises(ValueError, match="dvecs must be"):
        audio.separate_speakers(stub, wav, dvecs[:, 0], acfg)
    with pytest.raises(ValueError, match="wav must be"):
        audio.separate_speakers(stub, wav[0], dvecs, acfg)


def test_separate_speakers_with_reference_embeds_all_references_in_one_call(monkeypatch):
    from voicesplit_amd import audio, speaker
    seen = {}

    class Encoder:
        num_mels, window = 40, 80

        def embed_many(self, mels):
            seen["mels"] = list(mels)
            e = torch.stack([torch.full((16,), float(v)) for v in mels])
            return e, torch.tensor([v >= 0 for v in mels])

    monkeypatch.setattr(speaker, "logmel", lambda r, cfg, n_mels: float(r[0]))
    monkeypatch.setattr(audio, "separate_speakers", lambda model, wav, dvecs, cfg: dvecs)
    wav = torch.zeros(2, 8)
    refs = [[torch.tensor([1.0]), torch.tensor([2.0]), torch.tensor([3.0])], [torch.tensor([4.0]), torch.tensor([5.0]), torch.tensor([6.0])]]
    dvecs = audio.separate_speakers_with_reference(None, Encoder(), wav, refs, {})
    assert seen["mels"] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]                 # one embed_many call, mixture-major
    assert tuple(dvecs.shape) == (2, 3, 16) and dvecs.is_contiguous()
    assert torch.equal(dvecs[:, :, 0], torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]))
    with pytest.raises(ValueError, match="lists of reference"):
        audio.separate_speakers_with_reference(None, Encoder(), wav, refs[:1], {})
    with pytest.raises(ValueError, match="same number"):
        audio.separate_speakers_with_reference(None, Encoder(), wav, [refs[0], refs[1][:2]], {})
    refs[1][2] = torch.tensor([-1.0])
    with pytest.raises(ValueError, match=r"\(1, 2\)"):
        audio.separate_speakers_with_reference(None, Encoder(), wav, refs, {})
