"""numpy + scipy.spatial.cKDTree restatement of sph_gradients (include/summersph.h, "SPH gradients"): the target and
source sets, the cell edge E and the (cell key, id) order of every target's sources, the sums in that order and without
fused multiply-adds, both forms, the singular rule and the NaN rows.  Tests compare with tolerances; bitwise agreement
with the device is not required."""
import numpy as np
from scipy.spatial import cKDTree

AXIS_MASK = (1 << 21) - 1
AXIS_CELLS = float((1 << 21) - 8)
DBL_MAX = np.finfo(np.float64).max
CHUNK = 1 << 22               # padded (target, neighbour) entries per vectorised step


def _good_h(h):
    with np.errstate(invalid="ignore"):
        return (h > 0.0) & (h <= DBL_MAX)


def cell_edge(pos_src, h_src, h_one=None):
    """E of the sources (pos_src (n, 3) finite, h_src their h): 2 h (1 + 1e-6) for one h, else 2 h_ref (1 + 1e-6) with h_ref
    the upper edge of the quarter octave (bits >> 50) that holds the lower median of the sources' good h; enlarged where an
    axis would need more than 2^21 - 8 cells.  Returns (lo (3,), E)."""
    if h_one is not None:
        h_ref = float(h_one)
    else:
        hs = np.asarray(h_src, dtype=np.float64)
        hs = hs[_good_h(hs)]
        h_ref = 0.0
        if hs.size:
            bins = np.sort(hs.view(np.uint64) >> np.uint64(50))
            b = int(bins[(hs.size - 1) // 2])
            h_ref = float(np.array([(b + 1) << 50], dtype=np.uint64).view(np.float64)[0])
    e = (2.0 * h_ref) * (1.0 + 1e-6)
    if not (e > 0.0 and e <= DBL_MAX):
        e = 1.0
    if len(pos_src) == 0:
        return np.zeros(3), e
    lo = pos_src.min(axis=0)
    ext = pos_src.max(axis=0) - lo
    for a in range(3):
        if ext[a] / e > AXIS_CELLS:
            e = (ext[a] / AXIS_CELLS) * (1.0 + 1e-6)
    return lo, e


def cell_keys(pos, lo, e):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.clip(np.nan_to_num(np.floor((pos - lo) * (1.0 / e)), nan=0.0), 0, AXIS_MASK).astype(np.int64)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def targets_mask(pos, n_owned, clip=None):
    n = len(pos)
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    with np.errstate(invalid="ignore"):
        t = (np.arange(n) < n_owned) & np.all(np.isfinite(pos), axis=1)
        for a in range(3):
            t &= (lo[a] < pos[:, a]) & (pos[:, a] < hi[a])
    return t


def gradients(pos, m, A, h, n_owned=None, clip=None, corrected=True, h_one=None, only=None, info=None):
    """pos (n, 3), m (n,), A (K, n) field values, h (n,) per-particle h (or a scalar), all in download order with ghosts
    (ids >= n_owned).  h_one: desc.h > 0 (one h for every target) -- otherwise each particle's own h.  only: optional
    ids to evaluate (a subset of the targets; other rows stay NaN).  info: an optional dict that receives "ratio", det C /
    (tr C / 3)^3 per particle (NaN for non-targets; the singular test is ratio > 1e-6).  Returns (grad (K, 3, n), rho (n,), n_targets,
    n_singular) with NaN rows for non-targets; n_singular counts the evaluated targets."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    K = A.shape[0]
    m = np.asarray(m, dtype=np.float64)
    hp = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)) if h_one is None else np.full(n, float(h_one))
    n_owned = n if n_owned is None else n_owned
    src = np.nonzero(np.all(np.isfinite(pos), axis=1))[0]
    lo, e = cell_edge(pos[src], hp[src], h_one=h_one)
    key = cell_keys(pos[src], lo, e)
    tmask = targets_mask(pos, n_owned, clip)
    grad = np.full((K, 3, n), np.nan)
    rho = np.full(n, np.nan)
    ratio = np.full(n, np.nan)
    if info is not None:
        info["ratio"] = ratio
    n_t = int(tmask.sum())
    tid = np.nonzero(tmask)[0] if only is None else np.asarray(only, dtype=np.int64)
    assert np.all(tmask[tid])
    if not np.all(_good_h(hp[tid])):
        raise ValueError("a target has h <= 0 or a non-finite h")
    if tid.size == 0 or src.size == 0:
        return grad, rho, n_t, 0
    tree = cKDTree(pos[src])
    nb = tree.query_ball_point(pos[tid], r=(2.0 * hp[tid]) * (1.0 + 1e-9) + 1e-300)
    lens = np.array([len(v) for v in nb], dtype=np.int64)
    order = np.argsort(lens, kind="stable")
    n_sing = 0
    k0 = 0
    while k0 < len(order):
        lmax = lens[order[k0]]
        k1 = k0 + 1
        while k1 < len(order) and (k1 - k0 + 1) * max(lens[order[k1]], 1) <= CHUNK:
            k1 += 1
        rows = order[k0:k1]
        lmax = max(int(lens[rows].max()), 1)
        J = np.zeros((len(rows), lmax), dtype=np.int64)
        valid = np.zeros((len(rows), lmax), dtype=bool)
        for r, t in enumerate(rows):
            js = src[np.asarray(nb[t], dtype=np.int64)]
            kk = key[np.searchsorted(src, js)]
            o = np.lexsort((js, kk))                       # cell key, then id
            J[r, :len(js)] = js[o]
            valid[r, :len(js)] = True
        n_sing += _sums(pos, m, A, hp, tid[rows], J, valid, corrected, grad, rho, ratio)
        k0 = k1
    return grad, rho, n_t, n_sing


def _sums(pos, m, A, hp, ti, J, valid, corrected, grad, rho, ratio):
    K = A.shape[0]
    h = hp[ti]
    xi = pos[ti]
    r2max = 4.0 * (h * h)
    ih = 1.0 / h
    T, L = J.shape
    sw = np.zeros(T)
    c = [np.zeros(T) for _ in range(6)]
    b = np.zeros((K, 3, T))
    ai = A[:, ti]
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(L):
            j = J[:, k]
            dx = xi[:, 0] - pos[j, 0]
            dy = xi[:, 1] - pos[j, 1]
            dz = xi[:, 2] - pos[j, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = valid[:, k] & (d2 <= r2max)
            q = np.sqrt(d2) * ih
            tq = 2.0 - q
            w = np.where(q <= 1.0, (1.0 - 1.5 * (q * q)) + 0.75 * ((q * q) * q), 0.25 * ((tq * tq) * tq))
            mj = m[j]
            sw = np.where(ok, sw + mj * w, sw)
            ok &= d2 != 0.0
            f = np.where(q <= 1.0, 3.0 - 2.25 * q, (0.75 * (tq * tq)) / q)
            mf = mj * f
            if corrected:
                fx = mf * dx
                fy = mf * dy
                terms = (fx * dx, fx * dy, fx * dz, fy * dy, fy * dz, (mf * dz) * dz)
                for s in range(6):
                    c[s] = np.where(ok, c[s] + terms[s], c[s])
            for kk in range(K):
                g = mf * (ai[kk] - A[kk, j])
                b[kk, 0] = np.where(ok, b[kk, 0] + g * dx, b[kk, 0])
                b[kk, 1] = np.where(ok, b[kk, 1] + g * dy, b[kk, 1])
                b[kk, 2] = np.where(ok, b[kk, 2] + g * dz, b[kk, 2])
    sig = 1.0 / (np.pi * ((h * h) * h))
    rr = sig * sw
    rho[ti] = rr
    if corrected:
        cxx, cxy, cxz, cyy, cyz, czz = c
        a00 = cyy * czz - cyz * cyz
        a01 = cxz * cyz - cxy * czz
        a02 = cxy * cyz - cxz * cyy
        a11 = cxx * czz - cxz * cxz
        a12 = cxy * cxz - cxx * cyz
        a22 = cxx * cyy - cxy * cxy
        det = (cxx * a00 + cxy * a01) + cxz * a02
        t3 = ((cxx + cyy) + czz) / 3.0
        sing = ~(det > 1e-6 * ((t3 * t3) * t3))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio[ti] = det / ((t3 * t3) * t3)
        with np.errstate(invalid="ignore", divide="ignore"):
            for kk in range(K):
                bx, by, bz = b[kk]
                g = np.stack([((a00 * bx + a01 * by) + a02 * bz) / det,
                              ((a01 * bx + a11 * by) + a12 * bz) / det,
                              ((a02 * bx + a12 * by) + a22 * bz) / det])
                g[:, sing] = np.nan
                grad[kk][:, ti] = g
        return int(sing.sum())
    sc = sig / (h * h)
    with np.errstate(invalid="ignore", divide="ignore"):
        for kk in range(K):
            for a in range(3):
                grad[kk, a, ti] = (sc * b[kk, a]) / rr
    return 0


def velocity_derivatives(grad):
    """(3, 3, n) gradients of vx, vy, vz -> div v, curl v (3, n)"""
    g = grad
    return (g[0, 0] + g[1, 1]) + g[2, 2], np.stack([g[2, 1] - g[1, 2], g[0, 2] - g[2, 0], g[1, 0] - g[0, 1]])


def naive(pos, m, A, h, corrected=True):
    """O(N^2) double loop of the definitions (every particle a target and a source, each particle's own h), for checking
    the restatement: (grad (K, 3, n), rho (n,), singular mask)"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    K = A.shape[0]
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    grad = np.full((K, 3, n), np.nan)
    rho = np.zeros(n)
    sing = np.zeros(n, dtype=bool)
    for i in range(n):
        C = np.zeros((3, 3))
        b = np.zeros((K, 3))
        s = 0.0
        sig = 1.0 / (np.pi * h[i] ** 3)
        for j in range(n):
            x = pos[i] - pos[j]
            r = float(np.sqrt(x @ x))
            q = r / h[i]
            if q > 2.0:
                continue
            w = 1 - 1.5 * q ** 2 + 0.75 * q ** 3 if q <= 1 else 0.25 * (2 - q) ** 3
            s += m[j] * sig * w
            if r == 0.0:
                continue
            f = 3 - 2.25 * q if q <= 1 else 0.75 * (2 - q) ** 2 / q
            F = sig / h[i] ** 2 * f
            C += m[j] * F * np.outer(x, x)
            b += m[j] * F * (A[:, i] - A[:, j])[:, None] * x[None, :]
        rho[i] = s
        if corrected:
            det = np.linalg.det(C)
            if not det > 1e-6 * (np.trace(C) / 3) ** 3:
                sing[i] = True
                continue
            grad[:, :, i] = np.linalg.solve(C, b.T).T
        else:
            grad[:, :, i] = b / s
    return grad, rho, sing
