"""Evaluation metric of the reference on the GPU: single-source BSS-eval SDR.

The reference scores every test item with ``mir_eval.separation.bss_eval_sources(clean_wav, est_wav, False)[0][0]``
(utils/generic_utils.py:476-530; test.py prints its mean, test_all_checkpoints.py picks the best checkpoint by it).
``bss_sdr`` computes exactly that definition -- one source, the fixed 512-tap distortion filter -- for a batch of rows
in one call into libvoicesplit_hip.so (``vs_sdr``: fp64 correlations, a Toeplitz Levinson solve per row, fp64
projection), on the caller's stream, without a host round trip.

``bss_eval`` is the full multi-source definition, ``bss_eval_sources(reference, estimate, compute_permutation)`` for K
references and K estimates per item: SDR, SIR, SAR and the best permutation (``vs_bss_eval``: the same correlations between
all pairs, a block Levinson solve of the K-source Gram matrix, the K x K single-source solves, fp64 projections and the
permutation search on the device).
"""
import ctypes

import torch

from . import _lib
from .ops import _dev_check, _p, _stream

_WS = {}


def _buffer(n: int, device):
    """The device's metric workspace, grown to n bytes: one buffer per device, shared by ``bss_sdr`` and ``bss_eval``."""
    key = torch.device(device).index
    ws = _WS.get(key)
    if ws is None or ws.numel() < n:
        _WS.pop(key, None)
        ws = torch.empty(n, dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def _workspace(B: int, N: int, device):
    lib = _lib.load()
    n = lib.vs_sdr_workspace_bytes(B, N)
    if n == 0:
        _lib.check(-1, f"vs_sdr_workspace_bytes(B={B}, N={N})")
    return _buffer(n, device)


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


def _workspace_multi(B: int, K: int, N: int, device):
    lib = _lib.load()
    n = lib.vs_bss_eval_workspace_bytes(B, K, N)
    if n == 0:
        _lib.check(-1, f"vs_bss_eval_workspace_bytes(B={B}, K={K}, N={N})")
    return _buffer(n, device)


MAX_SOURCES = 6


def bss_eval(reference: torch.Tensor, estimate: torch.Tensor, compute_permutation: bool = True, return_pairs: bool = False):
    """SDR, SIR and SAR (dB) of K estimated sources against K reference sources per item, in mir_eval's argument order:
    ``mir_eval.separation.bss_eval_sources(reference, estimate, compute_permutation)`` for every item of a batch.

    reference, estimate: fp32 tensors on an MI355X, same shape, ``[K, N]`` or ``[B, K, N]``, 1 <= K <= 6.
    Returns ``(sdr, sir, sar, perm, status)``: float64 ``[B, K]`` x 3, int32 ``[B, K]`` and int32 ``[B]`` on the same device
    (B = 1 for 2-D input).  With ``compute_permutation`` all K x K (estimate, reference) pairs are scored, ``perm[b, j]`` is
    the estimate assigned to reference j by the permutation with the largest mean SIR (the first one in
    ``itertools.permutations`` order among equals), and ``sdr[b, j]`` etc. are the values of that pair; without it only
    estimate j against reference j is scored and ``perm`` is ``0 .. K-1``.
    ``return_pairs``: a sixth value, float64 ``[B, 3, K, K]`` indexed ``[b, criterion (sdr, sir, sar), estimate, reference]``;
    without ``compute_permutation`` its off-diagonal entries are NaN.
    status 0 = ok; 1 = a reference or estimate row of the item is all zero (mir_eval raises ValueError for the whole call);
    2 = a solve failed (for instance two identical references).  An item with status != 0 has NaN values and ``perm`` -1.
    K = 1: ``sdr`` equals ``bss_sdr`` bit for bit, ``sir`` is +inf and ``sar`` equals ``sdr``.

    Raises TypeError for any dtype but float32 and ValueError for a shape mismatch, K > 6 or an empty input."""
    for name, t in (("reference", reference), ("estimate", estimate)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected torch.float32, got {t.dtype} (convert explicitly)")
    if reference.shape != estimate.shape:
        raise ValueError(f"reference shape {tuple(reference.shape)} != estimate shape {tuple(estimate.shape)}")
    if reference.dim() not in (2, 3) or reference.numel() == 0:
        raise ValueError(f"expected [K, N] or [B, K, N] with B, K, N >= 1, got {tuple(reference.shape)}")
    if reference.shape[-2] > MAX_SOURCES:
        raise ValueError(f"at most {MAX_SOURCES} sources per item, got K = {reference.shape[-2]}")
    ref = reference.unsqueeze(0) if reference.dim() == 2 else reference
    est = estimate.unsqueeze(0) if estimate.dim() == 2 else estimate
    ref, est = ref.contiguous(), est.contiguous()
    _dev_check(ref, "reference")
    _dev_check(est, "estimate")
    if ref.device != est.device:
        raise ValueError(f"reference on {ref.device}, estimate on {est.device}")
    B, K, N = ref.shape
    lib = _lib.load()
    ws = _workspace_multi(B, K, N, ref.device)
    sdr, sir, sar = (torch.empty(B, K, dtype=torch.float64, device=ref.device) for _ in range(3))
    perm = torch.empty(B, K, dtype=torch.int32, device=ref.device)
    status = torch.empty(B, dtype=torch.int32, device=ref.device)
    pairs = torch.empty(B, 3, K, K, dtype=torch.float64, device=ref.device) if return_pairs else None
    with torch.cuda.device(ref.device):
        rc = lib.vs_bss_eval(_p(ref), _p(est), B, K, N, 1 if compute_permutation else 0, _p(sdr), _p(sir), _p(sar), _p(perm),
                             _p(status), _p(pairs), _p(ws), ws.numel(), _stream())
    _lib.check(rc, "vs_bss_eval")
    return (sdr, sir, sar, perm, status, pairs) if return_pairs else (sdr, sir, sar, perm, status)
