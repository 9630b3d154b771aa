"""numpy restatement of sph_render_field's semantics (include/summersph.h) for the field-render tests.

With the density render's kernel (render_ref.cubic_w: the analytic cubic spline, sigma = 1 / (np.pi h^3)) and nodes
(np.linspace), a node g has num(g) = sum_j w_j A_j W(|g - r_j|, h_j) and den(g) = sum_j w_j W(|g - r_j|, h_j), with
w_j = m_j (mass weight) or m_j / rho_j (volume weight).  Images are num, num / den (0 where den == 0), and their column
forms: sum num times the spacing, or sum num / sum den."""
import numpy as np

import render_ref


def brute(nodes, pos, w, a, h, chunk=2048):
    """(num, den) at nodes (M, 3) from particles pos (N, 3) with weights w (N,), values a (N,), h scalar or (N,)"""
    nodes = np.asarray(nodes, dtype=np.float64).reshape(-1, 3)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), w.shape)
    num, den = np.zeros(nodes.shape[0]), np.zeros(nodes.shape[0])
    for s in range(0, nodes.shape[0], chunk):
        g = nodes[s:s + chunk]
        r = np.sqrt(((g[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2))
        t = w[None, :] * render_ref.cubic_w(r, h[None, :])
        num[s:s + chunk] = (t * a[None, :]).sum(axis=1)
        den[s:s + chunk] = t.sum(axis=1)
    return num, den


def grid_brute(pos, w, a, h, lo, hi, n):
    """(num, den) on the n0 x n1 x n2 np.linspace grid (x slowest)"""
    X, Y, Z = np.meshgrid(*render_ref.axes(lo, hi, n), indexing="ij")
    num, den = brute(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), pos, w, a, h)
    return num.reshape(n), den.reshape(n)


def ratio(num, den):
    """num / den, exactly 0 where den == 0"""
    out = np.zeros(np.shape(num))
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def image(num, den, axis=None, normalise=False, scale=1.0):
    """the render's image (and weight) from the 3-D num / den grids: axis None = the grid, else the column sums"""
    if axis is not None:
        num, den = num.sum(axis=axis), den.sum(axis=axis)
        if not normalise:
            num = num * scale
        return (ratio(num, den) if normalise else num), den * scale
    return (ratio(num, den) if normalise else num), den
