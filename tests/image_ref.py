"""Extended-precision references of the image-forming passes for tests/image_sets.py's cases, with the per-node term
scale the binning tests bound the error by.

Every particle is added, in extended precision, to the nodes of the index box it can reach (2 h_j (1 + 1e-9) per axis:
outside it every term is an exact zero of the definition).  np.longdouble where its eps is <= 2^-63 (x87), else float64
terms summed exactly (math.fsum).

  render(case inputs) -> num, den, S_num, S_den, near          include/summersph.h, sph_render_density / sph_render_field
      num = sum ws_j A_j Wn(q), den = sum ws_j Wn(q), ws_j = w_j / (pi h_j^3) (np.pi: the definition's double-precision pi)
      S_num = sum_{q <= 2} |ws_j A_j|, S_den = sum_{q <= 2} ws_j;  near: some particle within 2 h_j (1 + 1e-12);
      render_terms: the number of terms with q <= 2 per node
  cube(...)   -> vox, S, near                                  include/summersph.h, "spectral cubes"
      S[iu, iv] = sum |y0_j| F(0) over the footprints covering the node.  erf has no extended-precision form here: the
      channel weights are differences of float64 0.5 erf values (absolute error <= 2^-53 each, i.e. <= 2^-52 of a term's
      scale |y0_j| F, which S counts in full)."""
from __future__ import annotations

import math

import numpy as np

import cube_ref

EXTENDED = np.finfo(np.longdouble).eps <= 2.0 ** -63
LD = np.longdouble if EXTENDED else np.float64


class _Acc:
    """a grid that adds terms in extended precision, or exactly where there is none"""

    def __init__(self, shape):
        self.shape = tuple(shape)
        if EXTENDED:
            self.a = np.zeros(self.shape, dtype=np.longdouble)
        else:
            self.terms = {}

    def add(self, index, values):
        """index: a tuple of slices (a box of the grid), values: the box's terms"""
        if EXTENDED:
            self.a[index] += values
        else:
            idx = np.arange(int(np.prod(self.shape))).reshape(self.shape)[index].ravel()
            for i, v in zip(idx, np.asarray(values, dtype=np.float64).ravel()):
                if v != 0.0:
                    self.terms.setdefault(int(i), []).append(float(v))

    def value(self):
        if EXTENDED:
            return self.a
        out = np.zeros(int(np.prod(self.shape)))
        for i, t in self.terms.items():
            out[i] = math.fsum(t)
        return out.reshape(self.shape)


def _range(g, p, r):
    """the slice of the sorted-or-constant node coordinates g within r of p"""
    idx = np.flatnonzero(np.abs(g - p) <= r)
    return None if idx.size == 0 else slice(int(idx[0]), int(idx[-1]) + 1)


def _wn(q):
    """W / sigma in the working precision"""
    one, two = LD(1.0), LD(2.0)
    t = two - q
    return np.where(q <= one, (one - LD(1.5) * q * q) + LD(0.75) * q * q * q, np.where(q <= two, LD(0.25) * t * t * t, LD(0.0)))


def render(pos, w, a, h, g, sel=None):
    """pos (N, 3), weights w (N,), values a (N,), h a number or (N,), g: the three node coordinate arrays, sel: a mask"""
    n = pos.shape[0]
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    shape = tuple(x.size for x in g)
    num, den, s_num, s_den = _Acc(shape), _Acc(shape), _Acc(shape), _Acc(shape)
    near = np.zeros(shape, dtype=bool)
    gl = [x.astype(LD) for x in g]
    for j in (range(n) if sel is None else np.flatnonzero(sel)):
        r = 2.0 * hh[j] * (1.0 + 1e-9)
        box = tuple(_range(g[k], pos[j, k], r) for k in range(3))
        if any(b is None for b in box):
            continue
        d = [gl[k][box[k]] - LD(pos[j, k]) for k in range(3)]
        r2 = (d[0] * d[0])[:, None, None] + (d[1] * d[1])[None, :, None] + (d[2] * d[2])[None, None, :]
        hj = LD(hh[j])
        q = np.sqrt(r2) / hj
        ws = LD(w[j]) / (LD(np.pi) * hj * hj * hj)
        t = ws * _wn(q)
        inside = q <= LD(2.0)
        num.add(box, t * LD(a[j]))
        den.add(box, t)
        s_num.add(box, np.where(inside, abs(ws * LD(a[j])), LD(0.0)))
        s_den.add(box, np.where(inside, abs(ws), LD(0.0)))
        near[box] |= np.asarray(q <= LD(2.0 * (1.0 + 1e-12)))
    return num.value(), den.value(), s_num.value(), s_den.value(), near


def render_terms(pos, h, g, sel=None):
    """the number of particles within 2 h_j of every node"""
    n = pos.shape[0]
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    cnt = np.zeros(tuple(x.size for x in g), dtype=np.int64)
    for j in (range(n) if sel is None else np.flatnonzero(sel)):
        box = tuple(_range(g[k], pos[j, k], 2.0 * hh[j]) for k in range(3))
        if any(b is None for b in box):
            continue
        d = [(g[k][box[k]] - pos[j, k]) ** 2 for k in range(3)]
        cnt[box] += (d[0][:, None, None] + d[1][None, :, None] + d[2][None, None, :]) <= 4.0 * hh[j] ** 2
    return cnt


# ---- the cube ---------------------------------------------------------------------------------------------------------
def _ints(p2, t):
    r = np.sqrt(p2 + t * t)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.where(p2 > 0, p2 * np.log(np.where(p2 > 0, t + r, LD(1.0))), LD(0.0))
    I1 = LD(0.5) * (t * r + L)
    I2 = p2 * t + t * t * t / LD(3.0)
    I3 = LD(0.25) * t * r * r * r + LD(0.375) * p2 * t * r + LD(0.375) * p2 * L
    return I1, I2, I3


def _g_in(p2, t):
    _, I2, I3 = _ints(p2, t)
    return t - LD(1.5) * I2 + LD(0.75) * I3


def _g_out(p2, t):
    I1, I2, I3 = _ints(p2, t)
    return LD(2.0) * t - LD(3.0) * I1 + LD(1.5) * I2 - LD(0.25) * I3


def column_kernel(p):
    """cube_ref.column_kernel's closed form in the working precision"""
    p = np.asarray(p, dtype=LD)
    p2 = p * p
    zero = np.zeros_like(p)
    t1 = np.sqrt(np.maximum(LD(1.0) - p2, LD(0.0)))
    t2 = np.sqrt(np.maximum(LD(4.0) - p2, LD(0.0)))
    inner = LD(2.0) * (_g_in(p2, t1) - _g_in(p2, zero) + _g_out(p2, t2) - _g_out(p2, t1))
    outer = LD(2.0) * (_g_out(p2, t2) - _g_out(p2, zero))
    return np.where(p < LD(1.0), inner, np.where(p < LD(2.0), outer, LD(0.0)))


def cube(pos, vel, m, h, values, gu, gv, v0, dv, n_chan, rot, centre, v_ref, sigma_floor):
    """the cube of every particle (no clip; sigma_scale = 0) on the image nodes gu x gv -> vox (n_chan, n_u, n_v), S, near"""
    n = pos.shape[0]
    P, V = cube_ref.project(rot, pos, vel, centre, v_ref)      # the definition's float64 frame
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    e = cube_ref.edges(v0, dv, n_chan)
    vox = [_Acc((gu.size, gv.size)) for _ in range(n_chan)]
    S = _Acc((gu.size, gv.size))
    near = np.zeros((gu.size, gv.size), dtype=bool)
    gul, gvl = gu.astype(LD), gv.astype(LD)
    for j in range(n):
        r = 2.0 * hh[j] * (1.0 + 1e-9)
        box = (_range(gu, P[j, 0], r), _range(gv, P[j, 1], r))
        if box[0] is None or box[1] is None:
            continue
        du, dvv = gul[box[0]] - LD(P[j, 0]), gvl[box[1]] - LD(P[j, 1])
        b = np.sqrt((du * du)[:, None] + (dvv * dvv)[None, :])
        hj = LD(hh[j])
        p = b / hj
        y0 = (LD(m[j]) * LD(values[j])) / (LD(np.pi) * hj * hj)
        Y = y0 * column_kernel(p)
        S.add(box, np.where(p <= LD(2.0), abs(y0) * LD(1.5), LD(0.0)))
        near[box] |= np.asarray(p <= LD(2.0 * (1.0 + 1e-12)))
        cd = cube_ref.cdf(e, V[j], sigma_floor)
        wk = cd[1:] - cd[:-1]
        for k in np.flatnonzero(wk != 0.0):
            vox[k].add(box, Y * LD(wk[k]))
    return np.stack([v.value() for v in vox]), S.value(), near
