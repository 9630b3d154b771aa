"""A numpy restatement of sph_frames (include/summersph.h): the terms of a frame in np.longdouble with F from the header's
formulas, the plain sum and the sum of |term| per node, and the cadence rule replayed on a list of t values in float64."""
import numpy as np

LD = np.longdouble


def _ints(p2, t):
    r = np.sqrt(p2 + t * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.where(p2 > 0, p2 * np.log(t + r), LD(0))
    I1 = (t * r + L) / 2
    I2 = p2 * t + t ** 3 / 3
    I3 = t * r ** 3 / 4 + 3 * p2 * t * r / 8 + 3 * p2 * L / 8
    return I1, I2, I3


def _g_in(p2, t):
    _, I2, I3 = _ints(p2, t)
    return t - LD(1.5) * I2 + LD(0.75) * I3


def _g_out(p2, t):
    I1, I2, I3 = _ints(p2, t)
    return 2 * t - 3 * I1 + LD(1.5) * I2 - LD(0.25) * I3


def spline_column(p):
    """F(p) of the header ("Footprint"), in long double: F(0) = 1.5, 0 for p >= 2"""
    p = np.asarray(p, dtype=LD)
    p2 = p * p
    zero = np.zeros_like(p)
    t2 = np.sqrt(np.maximum(4 - p2, 0))
    t1 = np.sqrt(np.maximum(1 - p2, 0))
    inner = 2 * (_g_in(p2, t1) - _g_in(p2, zero) + _g_out(p2, t2) - _g_out(p2, t1))
    outer = 2 * (_g_out(p2, t2) - _g_out(p2, zero))
    return np.where(p < 1, inner, np.where(p < 2, outer, zero))


def nodes(lo, hi, n):
    """np.linspace; a single node sits on lo"""
    return np.linspace(lo, lo if n == 1 else hi, n)


def project(pos, rot, centre):
    """P = rot (r - centre), every row as ((a0 dx + a1 dy) + a2 dz) in float64"""
    d = np.asarray(pos, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    r = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    return np.stack([(r[a, 0] * d[:, 0] + r[a, 1] * d[:, 1]) + r[a, 2] * d[:, 2] for a in range(3)], axis=1)


def select(pos, clip=None):
    pos = np.asarray(pos)
    if clip is None:
        return np.ones(len(pos), bool)
    c = np.asarray(clip, dtype=np.float64).reshape(2, 3)
    return np.all((pos > c[0]) & (pos < c[1]), axis=1)


def frame(pos, m, h, weights, shape, bounds, rot=None, centre=(0.0, 0.0, 0.0), clip=None):
    """(sums, abs_sums, n_sel): two (1 + nq, n_u, n_v) long double arrays -- per node the sum of the terms y0 A F(p) over
    the selected particles and the sum of their magnitudes -- and the selected count.  weights: nq arrays A (plane 0 has
    A = 1); h: a number or one per particle."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    rot = np.eye(3) if rot is None else rot
    b = np.asarray(bounds, dtype=np.float64).reshape(2, 2)
    gu, gv = nodes(b[0, 0], b[1, 0], shape[0]), nodes(b[0, 1], b[1, 1], shape[1])
    P = project(pos, rot, centre)
    sel = select(pos, clip)
    A = [np.ones(n)] + [np.asarray(w, dtype=np.float64) for w in weights]
    y0 = np.asarray(m, dtype=np.float64) / (np.pi * (hh * hh))
    sums = np.zeros((len(A), shape[0], shape[1]), dtype=LD)
    mags = np.zeros_like(sums)
    for j in np.nonzero(sel)[0]:
        reach = 2.0 * hh[j] * (1 + 1e-6)
        iu = np.nonzero(np.abs(gu - P[j, 0]) <= reach)[0]
        iv = np.nonzero(np.abs(gv - P[j, 1]) <= reach)[0]
        if iu.size == 0 or iv.size == 0:
            continue
        du = (gu[iu] - P[j, 0]).astype(LD)[:, None]
        dv = (gv[iv] - P[j, 1]).astype(LD)[None, :]
        F = spline_column(np.sqrt(du * du + dv * dv) / LD(hh[j]))
        for q, a in enumerate(A):
            t = LD(y0[j]) * LD(a[j]) * F
            sums[q][np.ix_(iu, iv)] += t
            mags[q][np.ix_(iu, iv)] += np.abs(t)
    return sums, mags, int(sel.sum())


def exponent(y0a):
    """e with 1.5 max |y0 A| < 2^e (0 for 0)"""
    b = 1.5 * float(np.max(np.abs(y0a))) if len(y0a) else 0.0
    return int(np.frexp(b)[1])


def cadence(ts, t0, dt_frame):
    """The steps (numbered from 1) that record a frame: step i ends at ts[i - 1]; it records iff t >= t0 + k dt_frame
    (product, then sum, in float64), and afterwards k = floor((t - t0) / dt_frame) + 1"""
    t0, dt = np.float64(t0), np.float64(dt_frame)
    k, out = 1, []
    for i, t in enumerate(np.asarray(ts, dtype=np.float64), start=1):
        if t >= t0 + np.float64(k) * dt:
            out.append(i)
            k = int(np.floor((t - t0) / dt)) + 1
    return out
