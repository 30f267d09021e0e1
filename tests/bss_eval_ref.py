"""fp64 numpy / scipy restatement of single-source BSS-eval SDR, the number the reference's validation reports
(utils/generic_utils.py:476-530: ``mir_eval.separation.bss_eval_sources(clean_wav, est_wav, False)[0][0]``).

Written from the published definition (Vincent, Gribonval, Fevotte, "Performance measurement in blind audio source
separation", IEEE TASLP 14(4), 2006) in the form mir_eval implements it, for ONE reference source and no permutation:

* the estimate is projected onto the subspace spanned by the reference delayed by 0 .. flen - 1 samples (flen = 512):
  the Gram matrix G of the zero-padded reference is the symmetric Toeplitz matrix of its autocorrelation, D the
  cross-correlation of reference and estimate, both taken with FFTs of length 2**ceil(log2(N + flen - 1));
  C = solve(G, D); the projection is P = fftconvolve(C, s_padded)[:N + flen - 1];
* with one source the interference term is identically zero, so SDR = SAR = 10 log10(sum P^2 / sum (e_padded - P)^2),
  +inf when the denominator is exactly 0;
* an all-zero reference or estimate is rejected (mir_eval's ``validate`` raises ValueError; the reference's validation
  then skips the item).

Pure numpy / scipy: no GPU, no mir_eval (it is not a dependency; tests/test_sdr_cpu.py compares against it when present).
"""
import numpy as np
from scipy.linalg import toeplitz
from scipy.signal import fftconvolve

FLEN = 512


def validate(reference, estimate):
    """mir_eval.separation.validate for one source: same shape, neither all zero."""
    reference, estimate = np.asarray(reference), np.asarray(estimate)
    if reference.shape != estimate.shape:
        raise ValueError(f"reference shape {reference.shape} != estimate shape {estimate.shape}")
    if not np.any(reference):
        raise ValueError("the reference source is all zero (silent)")
    if not np.any(estimate):
        raise ValueError("the estimated source is all zero (silent)")


def project(s, e, flen=FLEN):
    """Projection of e onto the span of s delayed by 0 .. flen-1: (P [N + flen - 1], e_padded, C [flen])."""
    s = np.asarray(s, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    n = s.shape[0]
    sp = np.concatenate([s, np.zeros(flen - 1)])
    ep = np.concatenate([e, np.zeros(flen - 1)])
    n_fft = int(2 ** np.ceil(np.log2(n + flen - 1.0)))
    sf = np.fft.fft(sp, n=n_fft)
    ef = np.fft.fft(ep, n=n_fft)
    ssf = np.real(np.fft.ifft(sf * np.conj(sf)))
    G = toeplitz(np.concatenate([ssf[:1], ssf[-1:-flen:-1]]), r=ssf[:flen])
    sef = np.real(np.fft.ifft(sf * np.conj(ef)))
    D = np.concatenate([sef[:1], sef[-1:-flen:-1]])
    C = np.linalg.solve(G, D)
    P = fftconvolve(C, sp)[: n + flen - 1]
    return P, ep, C


def safe_db(num, den):
    if den == 0:
        return np.inf
    return 10.0 * np.log10(num / den)


def sdr(reference, estimate, flen=FLEN):
    """SDR in dB of one estimate [N] against one reference [N]; ValueError as mir_eval's validate."""
    validate(reference, estimate)
    P, ep, _ = project(reference, estimate, flen)
    return safe_db(float(np.sum(P ** 2)), float(np.sum((ep - P) ** 2)))


def sdr_rows(reference, estimate, flen=FLEN):
    """Row-wise: (sdr float64 [B], status int32 [B]) with the GPU's conventions: status 1 and NaN for a row that
    validate rejects."""
    reference = np.atleast_2d(np.asarray(reference))
    estimate = np.atleast_2d(np.asarray(estimate))
    if reference.shape != estimate.shape:
        raise ValueError(f"reference shape {reference.shape} != estimate shape {estimate.shape}")
    out = np.full(reference.shape[0], np.nan)
    status = np.zeros(reference.shape[0], dtype=np.int32)
    for i in range(reference.shape[0]):
        try:
            out[i] = sdr(reference[i], estimate[i], flen)
        except ValueError:
            status[i] = 1
    return out, status
