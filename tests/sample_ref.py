"""numpy restatement of sph_sample's contract (include/summersph.h, "SPH interpolation at arbitrary points").

den(p) = sum_j ws_j Wn(|p - r_j| / h_j) and num_k(p) = sum_j ws_j A_j^(k) Wn over the sources (the owned particles with a
finite position strictly inside the clip box), ws_j Wn = w_j W(r, h_j) with render_ref.cubic_w (the analytic cubic spline,
sigma = 1 / (np.pi h^3)) and w_j = m_j (mass weight) or m_j / rho_j (volume weight).  The pairs are found per SOURCE: a
scipy cKDTree over the points, one ball query of radius 2 h_j per source (the scatter form: the points have no h)."""
import numpy as np
from scipy.spatial import cKDTree

import render_ref


def sources_mask(pos, n_owned=None, clip=None):
    """the selection: original ids < n_owned, finite, strictly inside clip = (lo xyz, hi xyz)"""
    n = pos.shape[0]
    ok = np.isfinite(pos).all(axis=1) & (np.arange(n) < (n if n_owned is None else n_owned))
    if clip is not None:
        lo, hi = np.asarray(clip[0], dtype=np.float64), np.asarray(clip[1], dtype=np.float64)
        ok &= ((pos > lo) & (pos < hi)).all(axis=1)
    return ok


def sample(points, pos, m, h, A=None, rho=None, n_owned=None, clip=None, normalise=False, chunk=20000):
    """(out (K, M), den (M,), (n_hit, n_nonfinite)) at points (M, 3) from particles pos (N, 3), m (N,), h scalar or (N,),
    values A (K, N) or None, rho (N,) for the volume weight or None for the mass weight"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    M, N = points.shape[0], pos.shape[0]
    A = np.zeros((0, N)) if A is None else np.asarray(A, dtype=np.float64).reshape(-1, N)
    K = A.shape[0]
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (N,))
    w = m if rho is None else m / rho
    src = np.nonzero(sources_mask(pos, n_owned, clip))[0]
    fin = np.isfinite(points).all(axis=1)
    pid = np.nonzero(fin)[0]
    den, num = np.zeros(M), np.zeros((K, M))
    if src.size and pid.size:
        tree = cKDTree(points[pid])
        for s in range(0, src.size, chunk):
            js = src[s:s + chunk]
            hit = tree.query_ball_point(pos[js], 2.0 * h[js] * (1.0 + 1e-9))
            cnt = np.fromiter((len(t) for t in hit), dtype=np.int64, count=js.size)
            if cnt.sum() == 0:
                continue
            j = np.repeat(js, cnt)
            p = pid[np.concatenate([np.asarray(t, dtype=np.int64) for t in hit if len(t)])]
            r = np.sqrt(((points[p] - pos[j]) ** 2).sum(axis=1))
            t = w[j] * render_ref.cubic_w(r, h[j])
            den += np.bincount(p, weights=t, minlength=M)
            for k in range(K):
                num[k] += np.bincount(p, weights=t * A[k, j], minlength=M)
    if normalise:
        out = np.zeros((K, M))
        nz = den != 0
        out[:, nz] = num[:, nz] / den[nz]
    else:
        out = num
    counts = (int(np.count_nonzero(den[fin] != 0)), int(M - fin.sum()))
    den = den.copy()
    den[~fin] = np.nan
    out[:, ~fin] = np.nan
    return out, den, counts
