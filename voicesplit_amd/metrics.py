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

``stoi`` is the intelligibility score reported beside them: STOI (Taal et al. 2011) and, with ``extended=True``, ESTOI (Jensen & Taal
2016) at 10 kHz (``vs_stoi``: silent-frame removal, one-third-octave band envelopes from a short fp64 DFT, the 30-frame correlation
stage, all fp64 with fixed summation orders).  It is pystoi's algorithm as remembered -- restated, not compared with a pystoi run: the
contract is the text in include/voicesplit_hip.h, and where pystoi resamples with an Octave-style filter this uses ``vs_resample``.
"""
import ctypes

import torch

from . import _call, _lib


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
    _call.dev_check(ref, "reference")
    _call.dev_check(est, "estimate")
    if ref.device != est.device:
        raise ValueError(f"reference on {ref.device}, estimate on {est.device}")
    B, N = ref.shape
    ws = _call.scratch("metric", _call.sized("sdr_workspace_bytes", B, N, what=f"vs_sdr_workspace_bytes(B={B}, N={N})"), ref.device)
    sdr = torch.empty(B, dtype=torch.float64, device=ref.device)
    status = torch.empty(B, dtype=torch.int32, device=ref.device)
    _call.call("sdr", ref.device, ref, est, B, N, sdr, status, ws, ws.numel())
    return sdr, status


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
    _call.dev_check(ref, "reference")
    _call.dev_check(est, "estimate")
    if ref.device != est.device:
        raise ValueError(f"reference on {ref.device}, estimate on {est.device}")
    B, K, N = ref.shape
    ws = _call.scratch("metric", _call.sized("bss_eval_workspace_bytes", B, K, N,
                                             what=f"vs_bss_eval_workspace_bytes(B={B}, K={K}, N={N})"), ref.device)
    sdr, sir, sar = (torch.empty(B, K, dtype=torch.float64, device=ref.device) for _ in range(3))
    perm = torch.empty(B, K, dtype=torch.int32, device=ref.device)
    status = torch.empty(B, dtype=torch.int32, device=ref.device)
    pairs = torch.empty(B, 3, K, K, dtype=torch.float64, device=ref.device) if return_pairs else None
    _call.call("bss_eval", ref.device, ref, est, B, K, N, 1 if compute_permutation else 0, sdr, sir, sar, perm, status, pairs,
               ws, ws.numel())
    return (sdr, sir, sar, perm, status, pairs) if return_pairs else (sdr, sir, sar, perm, status)


STOI_RATE = 10000
_STOI_DIMS = None
_STOI_RESAMPLERS = {}


def stoi_plan() -> _lib.VsStoiDims:
    """``vs_stoi_plan``: the constants and band edges of the contract (host arithmetic inside the library, no device)."""
    global _STOI_DIMS
    if _STOI_DIMS is None:
        d = _lib.VsStoiDims()
        _lib.check(_lib.load().vs_stoi_plan(ctypes.byref(d)), "vs_stoi_plan")
        _STOI_DIMS = d
    return _STOI_DIMS


def _stoi_resampler(sample_rate: int, device):
    from .resample import Resampler
    key = (torch.device(device).index, int(sample_rate))
    rs = _STOI_RESAMPLERS.get(key)
    if rs is None:
        rs = _STOI_RESAMPLERS[key] = Resampler(int(sample_rate), STOI_RATE, device)
    return rs


def stoi_clips(reference: torch.Tensor, estimate: torch.Tensor, table: torch.Tensor, extended: bool = False, envelopes: bool = False):
    """``vs_stoi`` on two flat 10 kHz buffers: reference, estimate 1-D fp32 on an MI355X, same length; table [R, 2] int64 on the
    HOST = (first sample, samples) of pair i in both buffers.  Returns ``(d, frames, status)``: float64 [R], int32 [R, 2] = (frames F,
    kept frames Mk), int32 [R]; status 1 = fewer than 30 kept frames, d = 1e-5.  envelopes: two more values, the band envelopes as
    one flat float64 buffer and their offsets [R] int64 (host): pair i's X then Y as [2, 15, Mk_i] from its offset on."""
    for name, t in (("reference", reference), ("estimate", estimate)):
        _call.dev_check(t, name)
        if t.dim() != 1:
            raise ValueError(f"{name}: expected a flat 1-D buffer, got {tuple(t.shape)}")
    if reference.shape != estimate.shape or reference.device != estimate.device:
        raise ValueError(f"reference {tuple(reference.shape)} on {reference.device}, estimate {tuple(estimate.shape)} on {estimate.device}")
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != 2 or table.dtype != torch.int64 or table.is_cuda \
            or table.shape[0] == 0:
        raise ValueError("table: expected [R, 2] int64 on the host, R >= 1")
    table = table.contiguous()
    dev, R, total = reference.device, table.shape[0], reference.numel()
    dims = stoi_plan()
    ws = _call.scratch("metric", _call.sized("stoi_workspace_bytes", ctypes.byref(dims), total, R,
                                             what=f"vs_stoi_workspace_bytes(total={total}, R={R})"), dev)
    table_dev = table.to(dev)
    d = torch.empty(R, dtype=torch.float64, device=dev)
    frames = torch.empty(R, 2, dtype=torch.int32, device=dev)
    status = torch.empty(R, dtype=torch.int32, device=dev)
    tob = tob_at = tob_at_dev = None
    if envelopes:
        counts = 30 * torch.clamp((table[:, 1] - 256) // 128 + 1, min=0)
        tob_at = counts.cumsum(0) - counts
        tob = torch.zeros(max(1, int(counts.sum())), dtype=torch.float64, device=dev)
        tob_at_dev = tob_at.to(dev)
    _call.call("stoi", dev, ctypes.byref(dims), reference, estimate, total, table, table_dev, R, 1 if extended else 0,
               d, frames, status, tob, tob_at_dev, ws, ws.numel())
    return (d, frames, status, tob, tob_at) if envelopes else (d, frames, status)


def stoi(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, extended: bool = False, lengths=None):
    """STOI (``extended``: ESTOI) of ``estimate`` against ``reference``, row by row.

    reference, estimate: fp32 tensors on an MI355X, same shape, ``[N]``, ``[B, N]`` or ``[B, K, N]`` at ``sample_rate`` Hz.
    lengths: optional ``[B]`` integers for a padded ragged batch: row b (all K rows of item b) is scored over its first
    ``lengths[b]`` samples, exactly as the unpadded clip would be.
    Returns ``(d, status)``: float64 and int32 on the same device, shaped like the leading axes (``[]``, ``[B]`` or ``[B, K]``).
    status 0 = ok; 1 = fewer than 30 frames are left after the silent frames of the reference are removed (under about 0.4 s of
    speech; pystoi warns and returns 1e-5): d is 1e-5 exactly.

    When ``sample_rate`` is not 10000 both signals go through one cached ``resample.Resampler(sample_rate, 10000)`` (pystoi uses an
    Octave-style resampler instead: one reason the numbers are restated, not compared with a pystoi run).
    Raises TypeError for any dtype but float32 and ValueError for a shape mismatch, as ``bss_sdr`` does; there is no CPU fallback."""
    flat_ref, flat_est, table, lead = _stoi_inputs(reference, estimate, sample_rate, lengths)
    d, _, status = stoi_clips(flat_ref, flat_est, table, extended=extended)
    return d.reshape(lead), status.reshape(lead)


def stoi_pair(reference: torch.Tensor, estimate: torch.Tensor, sample_rate: int = 16000, lengths=None):
    """``(stoi, estoi, status)``: both forms of ``stoi`` from one resampling of the two signals (bit-identical to the two calls)."""
    flat_ref, flat_est, table, lead = _stoi_inputs(reference, estimate, sample_rate, lengths)
    d, _, status = stoi_clips(flat_ref, flat_est, table, extended=False)
    e, _, _ = stoi_clips(flat_ref, flat_est, table, extended=True)
    return d.reshape(lead), e.reshape(lead), status.reshape(lead)


def _stoi_inputs(reference, estimate, sample_rate, lengths):
    """The checks of ``stoi`` and its two flat 10 kHz buffers: (reference, estimate, table [rows, 2] on the host, leading shape)."""
    for name, t in (("reference", reference), ("estimate", estimate)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected torch.float32, got {t.dtype} (convert explicitly)")
    if reference.shape != estimate.shape:
        raise ValueError(f"reference shape {tuple(reference.shape)} != estimate shape {tuple(estimate.shape)}")
    if reference.dim() not in (1, 2, 3) or reference.numel() == 0:
        raise ValueError(f"expected [N], [B, N] or [B, K, N] with B, K, N >= 1, got {tuple(reference.shape)}")
    if int(sample_rate) != sample_rate or sample_rate <= 0:
        raise ValueError(f"sample_rate={sample_rate!r}: a positive integer")
    lead, N = tuple(reference.shape[:-1]), reference.shape[-1]
    rows = reference.numel() // N
    if lengths is None:
        n = torch.full((rows,), N, dtype=torch.int64)
    else:
        n = torch.as_tensor(lengths).detach().to("cpu", torch.int64).reshape(-1)
        if reference.dim() == 1 or n.numel() != reference.shape[0]:
            raise ValueError(f"lengths: expected [B] = [{reference.shape[0] if reference.dim() > 1 else '-'}] for input "
                             f"{tuple(reference.shape)}, got {n.numel()} values")
        if int(n.min()) < 0 or int(n.max()) > N:
            raise ValueError(f"lengths: every length must lie in 0 .. {N}")
        n = n.repeat_interleave(rows // n.numel())
    ref = reference.reshape(-1, N).contiguous()
    est = estimate.reshape(-1, N).contiguous()
    _call.dev_check(ref, "reference")
    _call.dev_check(est, "estimate")
    if ref.device != est.device:
        raise ValueError(f"reference on {ref.device}, estimate on {est.device}")
    at = torch.arange(rows, dtype=torch.int64) * N
    if int(sample_rate) == STOI_RATE:
        flat_ref, flat_est, table = ref.reshape(-1), est.reshape(-1), torch.stack((at, n), dim=1)
    else:
        rs = _stoi_resampler(int(sample_rate), ref.device)
        if lengths is None:
            n_out = rs.out_len(N)
            flat_ref, flat_est = rs(ref).reshape(-1), rs(est).reshape(-1)
            table = torch.stack((torch.arange(rows, dtype=torch.int64) * n_out, torch.full((rows,), n_out, dtype=torch.int64)), dim=1)
        else:
            by_len = {v: rs.out_len(v) for v in set(n.tolist())}
            n_out = torch.tensor([by_len[v] for v in n.tolist()], dtype=torch.int64)
            at_out = n_out.cumsum(0) - n_out
            plan3 = torch.stack((at, n, at_out), dim=1)
            flat_ref, flat_est = (torch.empty(max(1, int(n_out.sum())), dtype=torch.float32, device=ref.device) for _ in range(2))
            rs.clips_into(ref.reshape(-1), flat_ref, plan3)
            rs.clips_into(est.reshape(-1), flat_est, plan3)
            table = torch.stack((at_out, n_out), dim=1)
    return flat_ref, flat_est, table, lead
