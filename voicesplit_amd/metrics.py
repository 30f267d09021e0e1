"""Evaluation metric of the reference on the GPU: single-source BSS-eval SDR.

The reference scores every test item with ``mir_eval.separation.bss_eval_sources(clean_wav, est_wav, False)[0][0]``
(utils/generic_utils.py:476-530; test.py prints its mean, test_all_checkpoints.py picks the best checkpoint by it).
``bss_sdr`` computes exactly that definition -- one source, the fixed 512-tap distortion filter -- for a batch of rows
in one call into libvoicesplit_hip.so (``vs_sdr``: fp64 correlations, a Toeplitz Levinson solve per row, fp64
projection), on the caller's stream, without a host round trip.
"""
import ctypes

import torch

from . import _lib
from .ops import _dev_check, _p, _stream

_WS = {}


def _workspace(B: int, N: int, device):
    lib = _lib.load()
    n = lib.vs_sdr_workspace_bytes(B, N)
    if n == 0:
        _lib.check(-1, f"vs_sdr_workspace_bytes(B={B}, N={N})")
    key = torch.device(device).index
    ws = _WS.get(key)
    if ws is None or ws.numel() < n:
        _WS.pop(key, None)
        ws = torch.empty(n, dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def bss_sdr(reference: torch.Tensor, estimate: torch.Tensor):
    """SDR (dB) of ``estimate`` against ``reference``, row by row, in mir_eval's argument order.

    reference, estimate: fp32 tensors on an MI355X, same shape, ``[N]`` or ``[B, N]``.
    Returns ``(sdr, status)``: float64 ``[B]`` and int32 ``[B]`` on the same device (``[1]`` for 1-D input).
    status 0 = ok; 1 = the reference or estimate row is all zero (mir_eval raises ValueError for it); 2 = the Toeplitz
    solve failed.  A row with status != 0 has SDR NaN.  +inf when the estimate is reproduced exactly.

    Raises TypeError for any dtype but float32 (an fp64 signal is not rounded silently) and ValueError for a shape
    mismatch, as mir_eval's ``validate`` does."""
    for name, t in (("reference", reference), ("estimate", estimate)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected torch.float32, got {t.dtype} (convert explicitly)")
    if reference.shape != estimate.shape:
        raise ValueError(f"reference shape {tuple(reference.shape)} != estimate shape {tuple(estimate.shape)}")
    if reference.dim() not in (1, 2) or reference.shape[-1] == 0 or reference.numel() == 0:
        raise ValueError(f"expected [N] or [B, N] with N, B >= 1, got {tuple(reference.shape)}")
    ref = reference.reshape(1, -1) if reference.dim() == 1 else reference
    est = estimate.reshape(1, -1) if estimate.dim() == 1 else estimate
    ref, est = ref.contiguous(), est.contiguous()
    _dev_check(ref, "reference")
    _dev_check(est, "estimate")
    if ref.device != est.device:
        raise ValueError(f"reference on {ref.device}, estimate on {est.device}")
    B, N = ref.shape
    lib = _lib.load()
    ws = _workspace(B, N, ref.device)
    sdr = torch.empty(B, dtype=torch.float64, device=ref.device)
    status = torch.empty(B, dtype=torch.int32, device=ref.device)
    with torch.cuda.device(ref.device):
        rc = lib.vs_sdr(_p(ref), _p(est), B, N, _p(sdr), _p(status), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "vs_sdr")
    return sdr, status
