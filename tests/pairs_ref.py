"""sph_pairs restated in numpy, bit for bit (include/summersph.h, "pair sums"): O(n^2), vectorised by rows of targets.
Every term is formed in the header's order, scaled by 2^(62 - e_s), rounded half-even (np.rint) and accumulated as integers
(int64 halves that cannot overflow, joined into Python integers); the doubles are float(int) scaled back, the limbs the
integer's two's complement.  Bounds, exponents and counts are restated too.  brute_force is the plain double loop."""
import math

import numpy as np

ROWS = 128          # targets per vectorised chunk


def edges_formula(lo, hi, n, log=False):
    """sph_binned's edges: linear lo + (k (hi - lo)) / n, log lo pow(hi / lo, k / n); the last edge is hi exactly"""
    k = np.arange(n, dtype=np.float64)
    e = lo * np.power(hi / lo, k / float(n)) if log else lo + (k * (hi - lo)) / float(n)
    return np.concatenate([e, [hi]])


def nsum_of(n_q, velocity):
    return 2 + 2 * n_q + (4 if velocity else 0)


def classes(pos, vel, m, h, A, n_owned, weight_m, velocity, scale_h, clip, stride, phase):
    """(source, target, not usable) bool arrays in the upload order"""
    n = pos.shape[0]
    idx = np.arange(n)
    owned = idx < n_owned
    ok = np.all(np.isfinite(pos), axis=1)
    if weight_m:
        ok &= np.isfinite(m)
    if scale_h:
        ok &= np.isfinite(h) & (h > 0.0)
    if velocity:
        ok &= np.all(np.isfinite(vel), axis=1)
    for a in A:
        ok &= np.isfinite(a)
    src = owned & ok
    tgt = src & (idx % stride == phase)
    if clip is not None:
        lo, hi = np.asarray(clip[0], dtype=np.float64), np.asarray(clip[1], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            tgt &= np.all((lo < pos) & (pos < hi), axis=1)
    return src, tgt, owned & ~ok


def exponents(w, vel, A, src, velocity):
    """e_s of every sum from the sources' maxima (the header's "Bounds")"""
    def top(a):
        return float(np.max(np.abs(a[src]))) if src.any() else 0.0

    def e_of(b):
        return int(np.frexp(np.float64(b))[1])
    nq = len(A)
    wm = np.float64(top(w))
    w2 = wm * wm
    ex = [62, e_of(w2)]
    D = [np.float64(2.0) * np.float64(top(a)) for a in A]
    ex += [e_of(w2 * d) for d in D]
    ex += [e_of(w2 * (d * d)) for d in D]
    if velocity:
        V = np.float64(4.0) * np.float64(max(top(vel[:, 0]), top(vel[:, 1]), top(vel[:, 2])))
        V2 = V * V
        ex += [e_of(w2 * V), e_of(w2 * V2), e_of(w2 * (V2 * V)), e_of(w2 * V2)]
    assert len(ex) == nsum_of(nq, velocity)
    return np.array(ex, dtype=np.int32)


def pair_terms(pos, vel, w, h, A, i, js, velocity, scale_h):
    """the binned variable and the float terms (one array per sum s >= 1) of the pairs (i, j in js), in the header's order"""
    dx, dy, dz = pos[js, 0] - pos[i, 0], pos[js, 1] - pos[i, 1], pos[js, 2] - pos[i, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    r = np.sqrt(d2)
    var = r / h[i] if scale_h else r
    ww = w[i] * w[js]
    terms = [ww]
    dA = [a[js] - a[i] for a in A]
    terms += [ww * d for d in dA]
    terms += [ww * (d * d) for d in dA]
    if velocity:
        ux, uy, uz = vel[js, 0] - vel[i, 0], vel[js, 1] - vel[i, 1], vel[js, 2] - vel[i, 2]
        dot = (ux * dx + uy * dy) + uz * dz
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(r == 0.0, 0.0, dot / r)
        u2 = u * u
        terms += [ww * u, ww * u2, ww * (u2 * u), ww * ((ux * ux + uy * uy) + uz * uz)]
    return var, terms


def bin_of(var, edge):
    """(selected, bin): edge[b] <= var < edge[b + 1] against the table"""
    sel = (var >= edge[0]) & (var < edge[-1])
    return sel, np.searchsorted(edge, var, side="right") - 1


def to_limbs(total):
    """a Python integer -> its 128-bit two's complement as (low, high) uint64"""
    t = total & ((1 << 128) - 1)
    return t & ((1 << 64) - 1), t >> 64


def from_limbs(lo, hi):
    t = (int(hi) << 64) | int(lo)
    return t - (1 << 128) if t >> 127 else t


def finish_int(total, e):
    """the correctly rounded double of total 2^(e - 62)"""
    return math.ldexp(float(total), int(e) - 62)


def pairs(pos, vel, m, h, A, edge, *, n_owned=None, weight_m=False, velocity=False, scale_h=False, clip=None, stride=1, phase=0):
    """sph_pairs: pos, vel (n, 3); m (n,); h (n,) or a number; A a list of (n,) arrays, all in the upload order; edge the
    table.  Returns {"sums" (n_bins, nsum), "raw" (n_bins, nsum, 2) uint64, "exps" (nsum,) int32, "counts" (3,)}."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    vel = np.zeros((n, 3)) if vel is None else np.asarray(vel, dtype=np.float64)
    h = np.full(n, float(h)) if np.ndim(h) == 0 else np.asarray(h, dtype=np.float64)
    A = [np.asarray(a, dtype=np.float64) for a in A]
    edge = np.asarray(edge, dtype=np.float64)
    n_owned = n if n_owned is None else int(n_owned)
    n_bins, nsum = edge.size - 1, nsum_of(len(A), velocity)
    src, tgt, bad = classes(pos, vel, m, h, A, n_owned, weight_m, velocity, scale_h, clip, stride, phase)
    w = np.asarray(m, dtype=np.float64) if weight_m else np.ones(n)
    ex = exponents(w, vel, A, src, velocity)
    js_all = np.flatnonzero(src)
    hi_acc = np.zeros((n_bins, nsum), dtype=np.int64)       # the terms' upper halves (t >> 31) and lower 31 bits: each sum
    lo_acc = np.zeros((n_bins, nsum), dtype=np.int64)       # of up to 2^32 of them fits an int64
    tl = np.flatnonzero(tgt)
    for c0 in range(0, tl.size, ROWS):
        rows = tl[c0:c0 + ROWS]
        ii = np.repeat(rows, js_all.size)
        jj = np.tile(js_all, rows.size)
        keep = ii != jj
        ii, jj = ii[keep], jj[keep]
        var, terms = pair_terms(pos, vel, w, h, A, ii, jj, velocity, scale_h)
        sel, b = bin_of(var, edge)
        b = b[sel]
        order = np.argsort(b, kind="stable")
        bs = b[order]
        if bs.size == 0:
            continue
        starts = np.flatnonzero(np.concatenate([[True], bs[1:] != bs[:-1]]))
        ub = bs[starts]
        hi_acc[ub, 0] += np.diff(np.concatenate([starts, [bs.size]]))
        for s, t in enumerate(terms, start=1):
            q = np.rint(np.ldexp(t[sel][order], 62 - int(ex[s]))).astype(np.int64)
            hi_acc[ub, s] += np.add.reduceat(q >> 31, starts)
            lo_acc[ub, s] += np.add.reduceat(q & 0x7fffffff, starts)
    sums = np.zeros((n_bins, nsum))
    raw = np.zeros((n_bins, nsum, 2), dtype=np.uint64)
    for b in range(n_bins):
        for s in range(nsum):
            total = int(hi_acc[b, s]) if s == 0 else (int(hi_acc[b, s]) << 31) + int(lo_acc[b, s])
            sums[b, s] = finish_int(total, ex[s])
            raw[b, s] = to_limbs(total)
    return {"sums": sums, "raw": raw, "exps": ex, "counts": (int(tgt.sum()), int(src.sum()), int(bad.sum()))}


def brute_force(pos, vel, m, h, A, edge, *, n_owned=None, weight_m=False, velocity=False, scale_h=False, clip=None, stride=1,
                phase=0):
    """the plain double loop in Python floats: (sums (n_bins, nsum) with every float sum an exactly rounded math.fsum of the
    double terms, counts)"""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    vel = np.zeros((n, 3)) if vel is None else np.asarray(vel, dtype=np.float64)
    h = np.full(n, float(h)) if np.ndim(h) == 0 else np.asarray(h, dtype=np.float64)
    n_owned = n if n_owned is None else int(n_owned)
    n_bins, nq = len(edge) - 1, len(A)
    nsum = nsum_of(nq, velocity)
    src, tgt, bad = classes(pos, vel, m, h, A, n_owned, weight_m, velocity, scale_h, clip, stride, phase)
    lists = [[[] for _ in range(nsum)] for _ in range(n_bins)]
    for i in np.flatnonzero(tgt):
        for j in np.flatnonzero(src):
            if i == j:
                continue
            dx, dy, dz = (float(pos[j, a]) - float(pos[i, a]) for a in range(3))
            r = math.sqrt((dx * dx + dy * dy) + dz * dz)
            var = r / float(h[i]) if scale_h else r
            if not (edge[0] <= var < edge[-1]):
                continue
            b = max(k for k in range(n_bins) if edge[k] <= var)
            w = float(m[i]) * float(m[j]) if weight_m else 1.0
            L = lists[b]
            L[0].append(1.0)
            L[1].append(w)
            for k, a in enumerate(A):
                dA = float(a[j]) - float(a[i])
                L[2 + k].append(w * dA)
                L[2 + nq + k].append(w * (dA * dA))
            if velocity:
                ux, uy, uz = (float(vel[j, a]) - float(vel[i, a]) for a in range(3))
                u = 0.0 if r == 0.0 else ((ux * dx + uy * dy) + uz * dz) / r
                s0 = 2 + 2 * nq
                L[s0].append(w * u)
                L[s0 + 1].append(w * (u * u))
                L[s0 + 2].append(w * ((u * u) * u))
                L[s0 + 3].append(w * ((ux * ux + uy * uy) + uz * uz))
    sums = np.array([[math.fsum(L[s]) for s in range(nsum)] for L in lists]).reshape(n_bins, nsum)
    largest = np.array([[max((abs(t) for t in L[s]), default=0.0) for s in range(nsum)] for L in lists]).reshape(n_bins, nsum)
    return sums, largest, (int(tgt.sum()), int(src.sum()), int(bad.sum()))
