"""sph_modes restated in numpy (include/summersph.h, "mode sums").  modes() forms every term in double in the header's
order, scales it by 2^(62 - e), rounds half-even (np.rint) and accumulates integers (int64 halves that cannot overflow,
joined into Python integers); the doubles are float(int) scaled back, the limbs the integer's two's complement.  The ring
sums use only + - * / sqrt, so they are the library's bit for bit; the spiral sums go through log, cos and sin, where two
libraries differ by ulps.  truth() is the brute-force version in np.longdouble (80-bit here: eps 1.08e-19), the yardstick
of the spiral sums."""
import math

import numpy as np


def frame_axes(normal):
    """(n^, e1, e2) by the header's rule"""
    nin = np.asarray(normal, dtype=np.float64)
    n = nin / np.sqrt((nin[0] * nin[0] + nin[1] * nin[1]) + nin[2] * nin[2])
    a = np.zeros(3)
    a[0 if abs(n[0]) <= 0.9 else 1] = 1.0
    an = (a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]
    t = a - an * n
    e1 = t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    e2 = np.array([n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]])
    return n, e1, e2


def edges_formula(r_min, r_max, n_r, log=False):
    k = np.arange(n_r, dtype=np.float64)
    e = r_min * np.power(r_max / r_min, k / float(n_r)) if log else r_min + (k * (r_max - r_min)) / float(n_r)
    return np.concatenate([e, [r_max]])


def p_formula(p_min, p_max, n_p):
    if n_p == 1:
        return np.array([float(p_min)])
    return p_min + (np.arange(n_p, dtype=np.float64) * (p_max - p_min)) / float(n_p - 1)


def to_limbs(total):
    """a Python integer -> its 128-bit two's complement as (low, high)"""
    t = total & ((1 << 128) - 1)
    return t & ((1 << 64) - 1), t >> 64


def from_limbs(lo, hi):
    t = (int(hi) << 64) | int(lo)
    return t - (1 << 128) if t >> 127 else t


def finish_int(total, e):
    """the correctly rounded double of total 2^(e - 62)"""
    return math.ldexp(float(total), int(e) - 62)


def _dot(r, e, T=np.float64):
    return (r[:, 0] * T(e[0]) + r[:, 1] * T(e[1])) + r[:, 2] * T(e[2])


def place(pos, centre, normal, T=np.float64):
    """(X, Y, Z, R) of every particle in the disc frame, in the type T (the axes are the doubles the library builds)"""
    n, e1, e2 = frame_axes(normal)
    r = np.asarray(pos, dtype=np.float64).astype(T) - np.asarray(centre, dtype=np.float64).astype(T)[None, :]
    X, Y, Z = _dot(r, e1, T), _dot(r, e2, T), _dot(r, n, T)
    return X, Y, Z, np.sqrt(X * X + Y * Y)


def select(pos, base, A, centre, normal, r_range, z_max, n_owned):
    """(usable selected, outside, not usable) bool arrays in the upload order, by the header's rule"""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    owned = np.arange(n) < (n if n_owned is None else int(n_owned))
    okpos = np.all(np.isfinite(pos), axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y, Z, R = place(np.where(okpos[:, None], pos, 0.0), centre, normal)
        inside = (R >= r_range[0]) & (R < r_range[1]) & (np.abs(Z) < z_max)
    okw = np.isfinite(base) & np.isfinite(A)
    sel = owned & okpos & inside & okw
    outside = owned & okpos & ~inside
    bad = owned & (~okpos | (inside & ~okw))
    return sel, outside, bad


def _accumulate(q, where, n_bins):
    """the exact sums of the int64 terms q per bin as Python integers"""
    hi = np.zeros(n_bins, dtype=np.int64)
    lo = np.zeros(n_bins, dtype=np.int64)
    np.add.at(hi, where, q >> 31)
    np.add.at(lo, where, q & 0x7fffffff)
    return [(int(h) << 31) + int(l) for h, l in zip(hi, lo)]


def modes(pos, m, A=None, *, edges, m_max, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), z_max=np.inf, weight_m=True,
          p=None, r_ref=1.0, n_owned=None):
    """sph_modes: pos (n, 3), m (n,), A (n,) or None, all in the upload order; edges the ring table, p the spiral table or
    None.  Returns {"ring" (n_r, m_max + 1, 2), "spiral" (m_max + 1, n_p, 2) or None, "raw_ring", "raw_spiral" (..., 2)
    uint64, "exp", "ring_counts" (n_r,) int64, "counts" (4,), and for the bounds "sel", the selected particles' "w", "u" and
    "ws" (w, 0 where R == 0: the weight in the spiral sums)}."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    edges = np.asarray(edges, dtype=np.float64)
    n_r, m1 = edges.size - 1, m_max + 1
    base = np.asarray(m, dtype=np.float64) if weight_m else np.ones(n)
    Aq = np.ones(n) if A is None else np.asarray(A, dtype=np.float64)
    sel, outside, bad = select(pos, base, Aq, centre, normal, (edges[0], edges[-1]), z_max, n_owned)
    X, Y, Z, R = place(pos[sel], centre, normal)
    w = base[sel] * Aq[sel]
    zero = R == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(zero, 1.0, X / R)
        s = np.where(zero, 0.0, Y / R)
    ring_of = np.searchsorted(edges, R, side="right") - 1
    e = int(np.frexp(np.float64(2.0) * (np.max(np.abs(w)) if w.size else np.float64(0.0)))[1])
    sh = 62 - e
    ring = np.zeros((n_r, m1, 2))
    raw_ring = np.zeros((n_r, m1, 2, 2), dtype=np.uint64)
    spiral = raw_spiral = None
    n_p = 0 if p is None else len(p)
    u = np.zeros(w.size)
    if n_p:
        p = np.asarray(p, dtype=np.float64)
        spiral = np.zeros((m1, n_p, 2))
        raw_spiral = np.zeros((m1, n_p, 2, 2), dtype=np.uint64)
        far = ~zero
        with np.errstate(divide="ignore"):
            u = np.where(far, np.log(np.where(far, R, 1.0) / r_ref), 0.0)
        th = p[None, :] * u[far][:, None]
        cp, sp = np.cos(th), np.sin(th)
        col = np.tile(np.arange(n_p), int(far.sum()))
    cm, sm = np.ones(w.size), np.zeros(w.size)
    for mm in range(m1):
        for t, v in enumerate((cm, sm)):
            q = np.rint(np.ldexp(w * v, sh)).astype(np.int64)
            for k, total in enumerate(_accumulate(q, ring_of, n_r)):
                ring[k, mm, t] = finish_int(total, e)
                raw_ring[k, mm, t] = to_limbs(total)
        if n_p:
            a, b, ww = cm[far][:, None], sm[far][:, None], w[far][:, None]
            for t, v in enumerate((ww * (a * cp - b * sp), ww * (b * cp + a * sp))):
                q = np.rint(np.ldexp(v, sh)).astype(np.int64).reshape(-1)
                for l, total in enumerate(_accumulate(q, col, n_p)):
                    spiral[mm, l, t] = finish_int(total, e)
                    raw_spiral[mm, l, t] = to_limbs(total)
        cm, sm = cm * c - sm * s, sm * c + cm * s
    return {"ring": ring, "spiral": spiral, "raw_ring": raw_ring, "raw_spiral": raw_spiral, "exp": e,
            "ring_counts": np.bincount(ring_of, minlength=n_r).astype(np.int64),
            "counts": (int(sel.sum()), int(outside.sum()), int(bad.sum()), int(zero.sum())), "w": w, "ws": np.where(zero, 0.0, w),
            "u": u, "sel": sel}


def truth(pos, w, sel, ring_of_edges, m_max, p, *, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), r_ref=1.0):
    """The sums of the selected particles (sel, with their double weights w) in np.longdouble, by plain summation: (ring
    (n_r, m_max + 1, 2), spiral (m_max + 1, n_p, 2)) as longdouble arrays.  The rings are decided in double, as the call
    decides them."""
    T = np.longdouble
    pos = np.asarray(pos, dtype=np.float64)[sel]
    edges = np.asarray(ring_of_edges, dtype=np.float64)
    Rd = place(pos, centre, normal)[3]
    ring_of = np.searchsorted(edges, Rd, side="right") - 1
    X, Y, Z, R = place(pos, centre, normal, T)
    zero = Rd == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(zero, T(1), X / R)
        s = np.where(zero, T(0), Y / R)
        u = np.log(np.where(zero, T(1), R) / T(r_ref))
    wl = np.asarray(w, dtype=np.float64).astype(T)
    ws = np.where(zero, T(0), wl)
    n_r, m1 = edges.size - 1, m_max + 1
    p = np.zeros(0) if p is None else np.asarray(p, dtype=np.float64)
    ring = np.zeros((n_r, m1, 2), dtype=T)
    spiral = np.zeros((m1, p.size, 2), dtype=T)
    th = p.astype(T)[None, :] * u[:, None]
    cp, sp = np.cos(th), np.sin(th)
    cm, sm = np.ones(wl.size, dtype=T), np.zeros(wl.size, dtype=T)
    for mm in range(m1):
        for k in range(n_r):
            ring[k, mm, 0] = np.sum((wl * cm)[ring_of == k])
            ring[k, mm, 1] = np.sum((wl * sm)[ring_of == k])
        spiral[mm, :, 0] = np.sum(ws[:, None] * (cm[:, None] * cp - sm[:, None] * sp), axis=0)
        spiral[mm, :, 1] = np.sum(ws[:, None] * (sm[:, None] * cp + cm[:, None] * sp), axis=0)
        cm, sm = cm * c - sm * s, sm * c + cm * s
    return ring, spiral


def spiral_bound(w, u, m_max, p):
    """the spiral sums' error bound per (m, l): sum_j |w_j| (2 |p_l u_j| + 2 m + 8) 2^-53"""
    w, u, p = np.abs(np.asarray(w, dtype=np.float64)), np.asarray(u, dtype=np.float64), np.asarray(p, dtype=np.float64)
    pu = np.sum(w[:, None] * np.abs(p[None, :] * u[:, None]), axis=0)              # (n_p,)
    mm = np.arange(m_max + 1, dtype=np.float64)
    return (2.0 * pu[None, :] + (2.0 * mm[:, None] + 8.0) * np.sum(w)) * 2.0 ** -53
