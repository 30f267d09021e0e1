"""fp64 numpy restatements of what voicesplit_amd/csrc/reverb.hip and voicesplit_amd/reverb.py compute (a helper module, not a
test); the contract is the text in include/voicesplit_hip.h.  The image method is restated from Allen & Berkley (1979): NOBODY HAS
COMPARED IT WITH A PYROOMACOUSTICS OR RIR-GENERATOR RUN.

``rir_loop(room)``      the image sum as a plain loop in the contract's enumeration order (q, j, k, n, l, p), w evaluated as
                        np.sinc(u) * (1 + cos(pi u / 40)) / 2 at u = t - tau;
``rir_by_delay(room)``  the same sum in another order and by other arithmetic: all images at once, the squares of the distance
                        summed from the other end, tau = d / (c / fs), ONE sine per image (sin(pi (t - tau)) alternates in sign with
                        t), sorted by delay and added tap by tap with np.add.at.  The distance between the two is ``d_ref``: what
                        fp64 evaluation noise does to a response;
``fir(..)``             the per-row FIR as np.convolve in fp64 on the fp32 inputs, with sum_k |h_k| |x_{n-k}| for the error bounds;
``draw_rooms(U, ..)``   the room draw from its block of uniform numbers;
``batch(..)``           one whole reverberant batch: FIR, energies, level, mix_wavfiles' normalisation.
A room is one row of the table of voicesplit_amd/reverb.py: size 3 | source 3 | receiver 3 | beta 6 | c | fs | nh | max_order."""
import math

import numpy as np

HALF = 40


def _fields(room):
    r = np.asarray(room, dtype=np.float64)
    return r[0:3], r[3:6], r[6:9], r[9:15], float(r[15]), float(r[16]), int(r[17]), int(r[18])


def image_range(room):
    """|n| <= N[0], |l| <= N[1], |p| <= N[2] reaches every image whose window touches a tap (include/voicesplit_hip.h)."""
    L, _, _, _, c, fs, nh, order = _fields(room)
    N = [int(math.floor((nh + HALF) * c / fs / (2.0 * L[d]))) + 1 for d in range(3)]
    if order >= 0:
        N = [min(n, (order + 1) // 2) for n in N]
    return N


def window(u):
    u = np.asarray(u, dtype=np.float64)
    return np.where(np.abs(u) < HALF, np.sinc(u) * 0.5 * (1.0 + np.cos(np.pi * u / HALF)), 0.0)


def _pow(b, e):
    return 1.0 if e == 0 else b ** e


def rir_loop(room, count=False):
    """h [nh] fp64; count=True: (h, number of images whose window touches a tap)."""
    L, s, m, beta, c, fs, nh, order = _fields(room)
    N = image_range(room)
    t = np.arange(nh, dtype=np.float64)
    h = np.zeros(nh)
    used = 0
    for q in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                for n in range(-N[0], N[0] + 1):
                    for l in range(-N[1], N[1] + 1):
                        for p in range(-N[2], N[2] + 1):
                            if order >= 0 and abs(2 * n - q) + abs(2 * l - j) + abs(2 * p - k) > order:
                                continue
                            Rx = (1 - 2 * q) * s[0] - m[0] + 2 * n * L[0]
                            Ry = (1 - 2 * j) * s[1] - m[1] + 2 * l * L[1]
                            Rz = (1 - 2 * k) * s[2] - m[2] + 2 * p * L[2]
                            d = math.sqrt((Rx * Rx + Ry * Ry) + Rz * Rz)
                            tau = d * fs / c
                            if tau - HALF >= nh:
                                continue
                            amp = (_pow(beta[0], abs(n - q)) * _pow(beta[1], abs(n)) * _pow(beta[2], abs(l - j)) * _pow(beta[3], abs(l))
                                   * _pow(beta[4], abs(p - k)) * _pow(beta[5], abs(p))) / (4.0 * math.pi * d)
                            if amp == 0.0:
                                continue
                            used += 1
                            h += amp * window(t - tau)
    return (h, used) if count else h


def rir_by_delay(room):
    L, s, m, beta, c, fs, nh, order = _fields(room)
    N = image_range(room)
    par = np.array([0, 1])
    q, j, k, n, l, p = np.meshgrid(par, par, par, np.arange(-N[0], N[0] + 1), np.arange(-N[1], N[1] + 1), np.arange(-N[2], N[2] + 1),
                                   indexing="ij")
    q, j, k, n, l, p = (a.reshape(-1) for a in (q, j, k, n, l, p))
    keep = np.ones(q.shape, dtype=bool) if order < 0 else (np.abs(2 * n - q) + np.abs(2 * l - j) + np.abs(2 * p - k) <= order)
    q, j, k, n, l, p = (a[keep] for a in (q, j, k, n, l, p))
    Rx = (1 - 2 * q) * s[0] - m[0] + 2 * n * L[0]
    Ry = (1 - 2 * j) * s[1] - m[1] + 2 * l * L[1]
    Rz = (1 - 2 * k) * s[2] - m[2] + 2 * p * L[2]
    d = np.sqrt(Rz * Rz + (Ry * Ry + Rx * Rx))
    tau = d / (c / fs)
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.ones(d.shape)
        for b, e in zip(beta, (np.abs(n - q), np.abs(n), np.abs(l - j), np.abs(l), np.abs(p - k), np.abs(p))):
            amp = amp * np.where(e == 0, 1.0, np.power(b, e.astype(np.float64)))
    amp = amp / (4.0 * np.pi * d)
    order_by_delay = np.argsort(tau, kind="stable")
    tau, amp = tau[order_by_delay], amp[order_by_delay]
    tau, amp = tau[tau - HALF < nh], amp[tau - HALF < nh]
    ti = np.rint(tau)
    frac = tau - ti
    s0 = np.sin(np.pi * frac)                              # sin(pi (t - tau)) = -(-1)^(t - ti) sin(pi frac)
    h = np.zeros(nh)
    for off in range(-HALF, HALF + 1):                     # tap ti + off of every image at once
        t = ti + off
        u = off - frac
        sign = -1.0 if off % 2 == 0 else 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            sinc = np.where(u == 0.0, 1.0, sign * s0 / (np.pi * u))
        w = np.where(np.abs(u) < HALF, sinc * (0.5 + 0.5 * np.cos(np.pi * u / HALF)), 0.0)
        ok = (t >= 0) & (t < nh)
        np.add.at(h, t[ok].astype(np.int64), (amp * w)[ok])
    return h


def d_ref(rooms):
    """(max over the rooms of max_t |rir_loop - rir_by_delay|, the same relative to each room's max |h|, the loop responses)."""
    worst, worst_rel, hs = 0.0, 0.0, []
    for room in rooms:
        a, b = rir_loop(room), rir_by_delay(room)
        dist = float(np.abs(a - b).max())
        worst, worst_rel = max(worst, dist), max(worst_rel, dist / float(np.abs(a).max()))
        hs.append(a)
    return worst, worst_rel, hs


# ---- the FIR ---------------------------------------------------------------------------------------------------------------------------
def fir(flat, at, lo, L, h, nh):
    """(y [L] fp64, sum_k |h_k| |x_{n-k}| [L] fp64, max |x| over the samples the row reads, max |h|) for one row:
    y[i] = sum_{k < nh} h[k] x(at + i - k), x(p) = flat[p] for p >= lo, else 0."""
    flat = np.asarray(flat)
    assert flat.dtype == np.float32 and np.asarray(h).dtype == np.float32
    hk = np.asarray(h[:nh], dtype=np.float64)
    first = max(lo, at - (nh - 1))
    x = np.concatenate([np.zeros(first - (at - (nh - 1))), flat[first:at + L].astype(np.float64)])      # x(at - nh + 1 .. at + L - 1)
    y = np.convolve(x, hk)[nh - 1:nh - 1 + L]
    mag = np.convolve(np.abs(x), np.abs(hk))[nh - 1:nh - 1 + L]
    return y, mag, float(np.abs(flat[first:at + L]).max()), float(np.abs(hk).max())


def fir_bound(mag, nh, mx, mh, math_name):
    """The contract's per-output error bound and, for the split-f16 arm, its underflow term u = nh 2^-38 mx mh."""
    if math_name == "fp32":
        return nh * 2.0 ** -24 * mag, 0.0
    u = nh * 2.0 ** -38 * mx * mh
    return (2.0 ** -20 + (nh + 32) * 2.0 ** -23) * mag + u, u


# ---- the room draw -----------------------------------------------------------------------------------------------------------------------
def sabine_beta(L, rt60):
    V, S = L[0] * L[1] * L[2], 2.0 * (L[0] * L[1] + L[1] * L[2] + L[0] * L[2])
    return math.sqrt(1.0 - min(0.99, max(0.01, 0.161 * V / (S * rt60))))


def draw_rooms(U, size=((3.0, 3.0, 2.4), (8.0, 6.0, 3.5)), rt60=(0.15, 0.5), distance=(0.5, 3.0), margin=0.5, fs=16000, nh=None,
               c=343.0, max_order=-1):
    """U [R, 13] uniform numbers -> ([2 R, 19] table, [R] reverberation times)."""
    U = np.asarray(U, dtype=np.float64)
    lo3, hi3 = np.array(size[0], dtype=np.float64), np.array(size[1], dtype=np.float64)
    rows, times = [], []
    for u in U:
        L = lo3 + u[0:3] * (hi3 - lo3)
        t60 = rt60[0] + u[3] * (rt60[1] - rt60[0])
        mic = margin + u[4:7] * (L - 2.0 * margin)
        beta = sabine_beta(L, t60)
        taps = min(8192, int(math.ceil(t60 * fs))) if nh is None else nh
        for sidx in range(2):
            az, ce = 2.0 * math.pi * u[7 + 3 * sidx], 2.0 * u[8 + 3 * sidx] - 1.0
            dist = distance[0] + u[9 + 3 * sidx] * (distance[1] - distance[0])
            se = math.sqrt(max(0.0, 1.0 - ce * ce))
            direction = np.array([se * math.cos(az), se * math.sin(az), ce])
            with np.errstate(divide="ignore"):
                hi_wall, lo_wall = (L - margin - mic) / np.abs(direction), (mic - margin) / np.abs(direction)
            forward = np.where(direction > 0.0, hi_wall, lo_wall)[direction != 0.0].min()
            backward = np.where(direction > 0.0, lo_wall, hi_wall)[direction != 0.0].min()
            if backward > forward:
                direction, forward = -direction, backward
            dist = min(dist, 0.95 * forward)
            rows.append(np.concatenate([L, mic + dist * direction, mic, [beta] * 6, [c, float(fs), taps, max_order]]))
        times.append(t60)
    return np.array(rows), np.array(times)


# ---- one whole batch ---------------------------------------------------------------------------------------------------------------------
def batch(flat, at, lo, hrow, nh, h, L, sir=None, nh_early=None, math_name="f16x3"):
    """One reverberant batch in fp64.  flat: the pool (fp32); at, lo, hrow, nh: [2][B] (clean, interferer); h [R][H] fp32 (the
    device's responses: vs_rir_shoebox has a test of its own); sir [B] in dB or None; nh_early [B] or None (the early target).
    Returns per item a dict: mixed, target (fp64, divided by ``norm``), norm (fp64, 1.1 max |c + g i|), gain, the measured ratio in dB,
    and err_mixed / err_target / err_norm: the FIR bound of the contract carried through the gain, the sum, the maximum and the
    division (every step's own fp32 rounding of 2^-24 added)."""
    B = len(at[0])
    eps = 2.0 ** -24
    out = []
    for b in range(B):
        c, cmag, cmx, cmh = fir(flat, at[0][b], lo[0][b], L, h[hrow[0][b]], nh[0][b])
        i, imag, imx, imh = fir(flat, at[1][b], lo[1][b], L, h[hrow[1][b]], nh[1][b])
        cb, _ = fir_bound(cmag, nh[0][b], cmx, cmh, math_name)
        ib, _ = fir_bound(imag, nh[1][b], imx, imh, math_name)
        cb, ib = cb + eps * np.abs(c), ib + eps * np.abs(i)                    # the rows are stored as fp32
        g, grel = 1.0, 0.0
        Ec, Ei = float((c * c).sum()), float((i * i).sum())
        if sir is not None:
            g = math.sqrt(Ec / Ei * 10.0 ** (-sir[b] / 10.0))
            # relative error of an energy: (2 sum |y| e + sum e^2) / E; of the gain: half of both, plus its rounding to fp32
            rc = (2.0 * (np.abs(c) * cb).sum() + (cb * cb).sum()) / Ec
            ri = (2.0 * (np.abs(i) * ib).sum() + (ib * ib).sum()) / Ei
            grel = 0.5 * (rc + ri) * (1.0 + rc + ri) + eps
        gi = g * i
        gib = g * ib + np.abs(gi) * (grel + eps)                                 # the scaled row, rounded once more
        s = c + gi
        sb = cb + gib + eps * np.abs(s)                                          # the fp32 sum inside vs_mix_clips
        m = float(np.abs(s).max())
        norm = 1.1 * m
        nrel = float(sb.max()) / m + eps                                         # the maximum moves by at most the largest error
        d = {"norm": norm, "err_norm": norm * nrel, "gain": g, "mixed": s / norm, "target": c / norm,
             "ratio_db": 10.0 * math.log10(Ec / (g * g * Ei)),
             "err_mixed": (sb / norm + np.abs(s / norm) * (nrel + eps)) * (1.0 + 2.0 * nrel),
             "err_target": (cb / norm + np.abs(c / norm) * (nrel + eps)) * (1.0 + 2.0 * nrel)}
        if nh_early is not None:
            e, emag, emx, emh = fir(flat, at[0][b], lo[0][b], L, h[hrow[0][b]], nh_early[b])
            eb, _ = fir_bound(emag, nh_early[b], emx, emh, math_name)
            d["target"] = e / norm
            d["err_target"] = ((eb + eps * np.abs(e)) / norm + np.abs(e / norm) * (nrel + eps)) * (1.0 + 2.0 * nrel)
        out.append(d)
    return out


def gpu_test_rooms():
    """The five responses of tests/test_gpu_reverb.py: a 3 x 2.5 x 2.2 m room with a different beta on every wall, nh in {1, 64, 512},
    max_order in {-1, 0, 2}; a few hundred images reach each of the long ones."""
    size, beta = [3.0, 2.5, 2.2], [0.9, 0.85, 0.8, 0.75, 0.7, 0.6]
    mic = [1.3, 1.1, 1.2]
    cases = [([2.1, 1.7, 1.5], 512, -1), ([0.7, 1.9, 0.9], 64, -1), ([1.5, 1.3, 1.45], 1, -1), ([2.1, 1.7, 1.5], 512, 0),
             ([2.4, 0.6, 1.0], 512, 2)]
    return np.array([size + src + mic + beta + [343.0, 16000.0, nh, order] for src, nh, order in cases], dtype=np.float64)
