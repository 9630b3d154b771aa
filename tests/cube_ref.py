"""numpy / scipy restatement of sph_cube (include/summersph.h, "spectral cubes"): the optically thin position-position-
velocity cube of a particle set seen along any direction.  Every particle is walked over its own footprint only."""
import numpy as np
from scipy.special import erf

XCUT = 8.5


def _ints(p2, t):
    r = np.sqrt(p2 + t * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.where(p2 > 0.0, p2 * np.log(t + r), 0.0)
    I1 = 0.5 * (t * r + L)
    I2 = p2 * t + t ** 3 / 3.0
    I3 = 0.25 * t * r ** 3 + 0.375 * p2 * t * r + 0.375 * p2 * L
    return I1, I2, I3


def _g_in(p2, t):
    _, I2, I3 = _ints(p2, t)
    return t - 1.5 * I2 + 0.75 * I3


def _g_out(p2, t):
    I1, I2, I3 = _ints(p2, t)
    return 2.0 * t - 3.0 * I1 + 1.5 * I2 - 0.25 * I3


def column_kernel(p):
    """F(p): the cubic spline 1 - 1.5 q^2 + 0.75 q^3 (q <= 1), 0.25 (2 - q)^3 (q <= 2) integrated along the line of sight at
    impact parameter p (both in units of h), in closed form"""
    p = np.asarray(p, dtype=np.float64)
    p2 = p * p
    zero = np.zeros_like(p)
    t1 = np.sqrt(np.maximum(1.0 - p2, 0.0))
    t2 = np.sqrt(np.maximum(4.0 - p2, 0.0))
    inner = 2.0 * (_g_in(p2, t1) - _g_in(p2, zero) + _g_out(p2, t2) - _g_out(p2, t1))
    outer = 2.0 * (_g_out(p2, t2) - _g_out(p2, zero))
    return np.where(p < 1.0, inner, np.where(p < 2.0, outer, 0.0))


def _w(q):
    return np.where(q <= 1.0, 1.0 - 1.5 * q * q + 0.75 * q ** 3, np.where(q <= 2.0, 0.25 * (2.0 - q) ** 3, 0.0))


def column_kernel_quad(p, nodes=64):
    """F(p) by piecewise Gauss-Legendre quadrature along the line of sight (pieces [0, t1], [t1, t2] where the spline's
    polynomial changes): the independent form the closed one is tested against"""
    x, w = np.polynomial.legendre.leggauss(nodes)
    out = []
    for pp in np.atleast_1d(np.asarray(p, dtype=np.float64)):
        if pp >= 2.0:
            out.append(0.0)
            continue
        t1 = np.sqrt(max(1.0 - pp * pp, 0.0))
        t2 = np.sqrt(4.0 - pp * pp)
        tot = 0.0
        for a, b in ((0.0, t1), (t1, t2)):
            if b > a:
                t = 0.5 * (b - a) * x + 0.5 * (b + a)
                tot += 0.5 * (b - a) * np.sum(w * _w(np.sqrt(pp * pp + t * t)))
        out.append(2.0 * tot)
    return np.array(out).reshape(np.shape(p))


def linspace_nodes(lo, hi, n):
    return np.linspace(lo, hi, n) if n > 1 else np.array([float(lo)])


def project(rot, pos, vel, centre=(0.0, 0.0, 0.0), v_ref=(0.0, 0.0, 0.0)):
    """P = rot (r - centre) and V = w^ . (v - v_ref), each row in the order ((a0 dx + a1 dy) + a2 dz)"""
    rot = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    d = np.asarray(pos, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    dv = np.asarray(vel, dtype=np.float64) - np.asarray(v_ref, dtype=np.float64)
    P = np.stack([(rot[a, 0] * d[:, 0] + rot[a, 1] * d[:, 1]) + rot[a, 2] * d[:, 2] for a in range(3)], axis=1)
    V = (rot[2, 0] * dv[:, 0] + rot[2, 1] * dv[:, 1]) + rot[2, 2] * dv[:, 2]
    return P, V


def edges(v0, dv, n_chan):
    return (np.arange(n_chan + 1) - 0.5) * dv + v0


def cdf(e, V, sigma):
    """the truncated Gaussian's cdf at the edges e for one particle; sigma == 0: the step that puts the particle into the
    channel with e_k <= V < e_{k+1}"""
    if sigma > 0.0:
        x = (e - V) / sigma
        return np.where(x >= XCUT, 0.5, np.where(x <= -XCUT, -0.5, 0.5 * erf(x / np.sqrt(2.0))))
    return np.where(e > V, 0.5, -0.5)


def selection(pos, n_owned=None, clip=None):
    n = pos.shape[0]
    sel = np.arange(n) < (n if n_owned is None else n_owned)
    if clip is not None:
        lo, hi = np.asarray(clip, dtype=np.float64).reshape(2, 3)
        with np.errstate(invalid="ignore"):
            sel &= np.all((pos > lo) & (pos < hi), axis=1)
    return sel


def sigmas(c, sigma_scale, sigma_floor, n):
    if sigma_scale == 0.0:
        return np.full(n, float(sigma_floor))
    return np.sqrt((sigma_scale * np.asarray(c, dtype=np.float64)) ** 2 + sigma_floor ** 2)


def cube(pos, vel, m, h, shape, bounds, v0, dv, n_chan, rot=None, centre=(0.0, 0.0, 0.0), v_ref=(0.0, 0.0, 0.0), c=None,
         sigma_scale=0.0, sigma_floor=0.0, values=None, clip=None, n_owned=None, per_velocity=False, column=column_kernel):
    """voxel[k][iu][iv] = sum_j m_j A_j F(b / h_j) / (pi h_j^2) (cdf_j(e_{k+1}) - cdf_j(e_k)); h: a number or per particle"""
    rot = np.eye(3) if rot is None else np.asarray(rot, dtype=np.float64).reshape(3, 3)
    n = pos.shape[0]
    n_u, n_v = (shape, shape) if np.isscalar(shape) else shape
    (lo_u, lo_v), (hi_u, hi_v) = bounds
    gu, gv = linspace_nodes(lo_u, hi_u, n_u), linspace_nodes(lo_v, hi_v, n_v)
    P, V = project(rot, pos, vel, centre, v_ref)
    hh = np.full(n, float(h)) if np.isscalar(h) else np.asarray(h, dtype=np.float64)
    A = np.ones(n) if values is None else np.asarray(values, dtype=np.float64)
    sg = sigmas(c, sigma_scale, sigma_floor, n)
    e = edges(v0, dv, n_chan)
    out = np.zeros((n_chan, n_u, n_v))
    for j in np.flatnonzero(selection(pos, n_owned, clip)):
        iu = np.flatnonzero(np.abs(gu - P[j, 0]) <= 2.0 * hh[j])
        iv = np.flatnonzero(np.abs(gv - P[j, 1]) <= 2.0 * hh[j])
        if iu.size == 0 or iv.size == 0:
            continue
        cd = cdf(e, V[j], sg[j])
        w = cd[1:] - cd[:-1]
        ks = np.flatnonzero(w != 0.0)
        if ks.size == 0 and not np.isnan(w).any():
            continue
        b = np.sqrt((gu[iu, None] - P[j, 0]) ** 2 + (gv[None, iv] - P[j, 1]) ** 2)
        Y = m[j] * A[j] * column(b / hh[j]) / (np.pi * hh[j] * hh[j])
        k0, k1 = ks[0], ks[-1] + 1
        out[k0:k1, iu[0]:iu[-1] + 1, iv[0]:iv[-1] + 1] += w[k0:k1, None, None] * Y[None]
    return out / dv if per_velocity else out


def voxels(pos, vel, m, h, gu, gv, pix, v0, dv, n_chan, chans, rot, c=None, sigma_scale=0.0, sigma_floor=0.0):
    """brute force for single voxels: pix an (M, 2) array of node indices, chans the M channels"""
    n = pos.shape[0]
    P, V = project(rot, pos, vel)
    hh = np.full(n, float(h)) if np.isscalar(h) else np.asarray(h, dtype=np.float64)
    sg = sigmas(c, sigma_scale, sigma_floor, n)
    out = np.zeros(len(chans))
    for q, ((iu, iv), k) in enumerate(zip(pix, chans)):
        b = np.hypot(gu[iu] - P[:, 0], gv[iv] - P[:, 1])
        js = np.flatnonzero(b < 2.0 * hh)
        Y = m[js] * column_kernel(b[js] / hh[js]) / (np.pi * hh[js] ** 2)
        e0, e1 = (k - 0.5) * dv + v0, (k + 1 - 0.5) * dv + v0
        w = np.array([cdf(np.array([e0, e1]), V[j], sg[j]) for j in js]).reshape(-1, 2)
        out[q] = np.sum(Y * (w[:, 1] - w[:, 0]))
    return out
