"""numpy restatement of sph_render_density's semantics (include/summersph.h) for the render tests.

D(g) = sum_j m_j W(|g - r_j|, h_j) with Density_Image.py's analytic cubic spline (sigma = 1 / (np.pi h^3)), nodes from
np.linspace.  Two forms: a brute force over given nodes, and a per-particle scatter over the node boxes each particle
can reach (for grids whose brute force would be too large, e.g. the script's 120^3)."""
import numpy as np


def cubic_w(r, h):
    """the script's cubic_spline_kernel, for arrays r and h (h broadcast)"""
    q = r / h
    sigma = 1.0 / (np.pi * h ** 3)
    w = np.zeros(np.broadcast(r, h).shape)
    s = np.broadcast_to(sigma, w.shape)
    q = np.broadcast_to(q, w.shape)
    m1 = q <= 1
    m2 = (q > 1) & (q <= 2)
    w[m1] = s[m1] * (1 - 1.5 * q[m1] ** 2 + 0.75 * q[m1] ** 3)
    w[m2] = s[m2] * 0.25 * (2 - q[m2]) ** 3
    return w


def axes(lo, hi, n):
    return [np.linspace(lo[a], hi[a], n[a]) if n[a] > 1 else np.array([lo[a]], dtype=np.float64) for a in range(3)]


def brute(nodes, pos, m, h, chunk=2048):
    """D at nodes (M, 3) from particles pos (N, 3), m (N,), h scalar or (N,)"""
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, 3)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), m.shape)
    out = np.zeros(nodes.shape[0])
    for s in range(0, nodes.shape[0], chunk):
        g = nodes[s:s + chunk]
        r = np.sqrt(((g[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2))
        out[s:s + chunk] = (m[None, :] * cubic_w(r, h[None, :])).sum(axis=1)
    return out


def grid_brute(pos, m, h, lo, hi, n):
    ax = axes(lo, hi, n)
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return brute(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), pos, m, h).reshape(n)


def grid_scatter(pos, m, h, lo, hi, n):
    """the same 3-D grid, each particle added to the nodes of its reachable index box (np.add.at)"""
    n = tuple(int(v) for v in n)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), m.shape)
    ax = axes(lo, hi, n)
    base, K = [], []
    for a in range(3):
        if n[a] == 1:
            base.append(np.zeros(m.size, dtype=np.int64)); K.append(0)
            continue
        step = (hi[a] - lo[a]) / (n[a] - 1)
        base.append(np.floor((pos[:, a] - lo[a]) / step).astype(np.int64))
        K.append(int(np.ceil(2.0 * h.max() / step)) + 1)
    grid = np.zeros(n)
    for ox in range(-K[0], K[0] + 2):
        ix = base[0] + ox
        for oy in range(-K[1], K[1] + 2):
            iy = base[1] + oy
            for oz in range(-K[2], K[2] + 2):
                iz = base[2] + oz
                ok = (ix >= 0) & (ix < n[0]) & (iy >= 0) & (iy < n[1]) & (iz >= 0) & (iz < n[2])
                if not ok.any():
                    continue
                i, j, k = ix[ok], iy[ok], iz[ok]
                d = np.stack([ax[0][i], ax[1][j], ax[2][k]], axis=1) - pos[ok]
                r = np.sqrt((d ** 2).sum(axis=1))
                w = m[ok] * cubic_w(r, h[ok])
                np.add.at(grid, (i, j, k), w)
    return grid
