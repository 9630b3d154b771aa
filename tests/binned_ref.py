"""The numpy restatement of sph_binned (include/summersph.h, "binned sums"): bins by np.searchsorted against the library's
own edge tables (capi.binned_edges), the selection rule, and the sums per bin by np.bincount (sequential sums in id order;
the library's differ by rounding only)."""
import numpy as np


def edges_formula(lo, hi, n, log=False):
    """the header's edge formulas, with numpy's pow"""
    k = np.arange(n + 1, dtype=np.float64)
    e = lo * np.power(hi / lo, k / n) if log else lo + (k * (hi - lo)) / n
    e[-1] = hi
    return e


def bin_index(a, edges):
    """(inside, k): edges[k] <= a < edges[k + 1]; a NaN is outside"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (a >= edges[0]) & (a < edges[-1])
    k = np.searchsorted(edges, a, side="right") - 1
    return inside, np.clip(k, 0, edges.size - 2)


def binned_sums(axes, tables, q, w, owned=None, squares=False, skip_nan=True):
    """(sums (n0, n1, nsum), counts (selected, outside, dropped)).  axes: one or two arrays of sph_count values in the upload
    order; tables: their edge tables; q: the quantities' arrays; w: the weights; owned: mask of the owned gas (default: all)."""
    n = np.asarray(axes[0]).size
    owned = np.ones(n, bool) if owned is None else np.asarray(owned, bool)
    inside = owned.copy()
    ks = []
    for a, e in zip(axes, tables):
        ok, k = bin_index(a, np.asarray(e, dtype=np.float64))
        inside &= ok
        ks.append(k)
    n0 = len(tables[0]) - 1
    n1 = len(tables[1]) - 1 if len(tables) == 2 else 1
    b = ks[0] * n1 + (ks[1] if len(tables) == 2 else 0)
    q = [np.asarray(v, dtype=np.float64) for v in q]
    nan = np.zeros(n, bool)
    for v in q:
        nan |= np.isnan(v)
    dropped = inside & nan if skip_nan else np.zeros(n, bool)
    sel = inside & ~dropped
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), (n,))
    cols = [np.ones(n), w] + [w * v for v in q] + ([w * (v * v) for v in q] if squares else [])
    out = np.zeros((n0 * n1, len(cols)))
    for s, c in enumerate(cols):
        out[:, s] = np.bincount(b[sel], weights=c[sel], minlength=n0 * n1)
    counts = (int(sel.sum()), int((owned & ~inside).sum()), int(dropped.sum()))
    return out.reshape(n0, n1, len(cols)), counts


def brute_force(axes, tables, q, w, owned=None, squares=False, skip_nan=True):
    """the same by a plain loop over the particles and linear scans of the tables"""
    n = len(axes[0])
    n0 = len(tables[0]) - 1
    n1 = len(tables[1]) - 1 if len(tables) == 2 else 1
    nq = len(q)
    out = np.zeros((n0, n1, 2 + nq * (2 if squares else 1)))
    counts = [0, 0, 0]
    for i in range(n):
        if owned is not None and not owned[i]:
            continue
        k = []
        for a, e in zip(axes, tables):
            v = a[i]
            kk = -1
            for j in range(len(e) - 1):
                if e[j] <= v < e[j + 1]:
                    kk = j
            k.append(kk)
        if min(k) < 0:
            counts[1] += 1
            continue
        if skip_nan and any(np.isnan(v[i]) for v in q):
            counts[2] += 1
            continue
        counts[0] += 1
        cell = out[k[0], k[1] if len(k) == 2 else 0]
        cell[0] += 1.0
        cell[1] += w[i]
        for j, v in enumerate(q):
            cell[2 + j] += w[i] * v[i]
            if squares:
                cell[2 + nq + j] += w[i] * (v[i] * v[i])
    return out, tuple(counts)
