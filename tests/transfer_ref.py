"""numpy restatement of sph_transfer (include/summersph.h, "emission-absorption images"): the selected particles sorted by
(D, id), a loop over the particles, vectorised over the nodes of each particle's footprint.  transfer_nodes is the brute
force for single nodes (every particle tested against the node, the node's own list composited by a scalar loop)."""
import numpy as np

from cube_ref import column_kernel, linspace_nodes, project, selection

NEAR = 1e-9          # the scoring rule's window about tau_surface / tau_max, relative


def inputs(pos, m, h, K, S, rot=None, centre=(0.0, 0.0, 0.0), kappa_scale=1.0, clip=None, n_owned=None):
    """(order, P, h, y0, S): the selected particles' indices in ascending (D, id) and the per-particle arrays.  K, S: None
    (the constant 1) or arrays."""
    rot = np.eye(3) if rot is None else np.asarray(rot, dtype=np.float64).reshape(3, 3)
    n = pos.shape[0]
    P, _ = project(rot, pos, np.zeros_like(pos), centre)
    hh = np.full(n, float(h)) if np.isscalar(h) else np.asarray(h, dtype=np.float64)
    K = np.ones(n) if K is None else np.asarray(K, dtype=np.float64)
    S = np.ones(n) if S is None else np.asarray(S, dtype=np.float64)
    y0 = (m * (kappa_scale * K)) / (np.pi * (hh * hh))
    sel = np.flatnonzero(selection(pos, n_owned, clip))
    D = P[sel, 2] + 0.0                                   # -0.0 and +0.0 compare equal anyway; ties fall to the id
    order = sel[np.lexsort((sel, D))]
    return order, P, hh, y0, S


def transfer(pos, m, h, shape, bounds, rot=None, centre=(0.0, 0.0, 0.0), source=None, kappa=None, kappa_scale=1.0,
             tau_surface=1.0, tau_max=np.inf, background=0.0, clip=None, n_owned=None, info=None):
    """The four planes (4, n_u, n_v).  info: a dict that receives `thin` (sum S dtau over the particles met), `near_surface`
    and `near_stop` (the nodes whose tau just before or after crossing tau_surface / tau_max lies within NEAR of it)."""
    n_u, n_v = (shape, shape) if np.isscalar(shape) else shape
    (lo_u, lo_v), (hi_u, hi_v) = bounds
    gu, gv = linspace_nodes(lo_u, hi_u, n_u), linspace_nodes(lo_v, hi_v, n_v)
    order, P, hh, y0, S = inputs(pos, m, h, kappa, source, rot, centre, kappa_scale, clip, n_owned)
    reach = 2.0 * hh[order]                               # the loop only sees the particles that reach the node box
    order = order[(P[order, 0] >= gu.min() - reach) & (P[order, 0] <= gu.max() + reach) &
                  (P[order, 1] >= gv.min() - reach) & (P[order, 1] <= gv.max() + reach)]
    tau, T, I = np.zeros((n_u, n_v)), np.ones((n_u, n_v)), np.zeros((n_u, n_v))
    surf = np.full((n_u, n_v), np.nan)
    run = np.ones((n_u, n_v), dtype=bool)
    thin = np.zeros((n_u, n_v))
    near_s, near_m = np.zeros((n_u, n_v), dtype=bool), np.zeros((n_u, n_v), dtype=bool)

    def near(t, ref):
        return np.abs(t - ref) <= NEAR * ref if np.isfinite(ref) else np.zeros(t.shape, dtype=bool)
    for j in order:
        iu = np.flatnonzero(np.abs(gu - P[j, 0]) <= 2.0 * hh[j])
        iv = np.flatnonzero(np.abs(gv - P[j, 1]) <= 2.0 * hh[j])
        if iu.size == 0 or iv.size == 0:
            continue
        w = (slice(iu[0], iu[-1] + 1), slice(iv[0], iv[-1] + 1))
        b = np.sqrt((gu[iu, None] - P[j, 0]) ** 2 + (gv[None, iv] - P[j, 1]) ** 2)
        p = b / hh[j]
        act = run[w] & (p < 2.0)
        if not act.any():
            continue
        dtau = y0[j] * column_kernel(p)
        a = -np.expm1(-dtau)
        t0 = tau[w]
        t1 = t0 + dtau
        I[w] = np.where(act, I[w] + (S[j] * T[w]) * a, I[w])
        T[w] = np.where(act, T[w] - T[w] * a, T[w])
        thin[w] = np.where(act, thin[w] + S[j] * dtau, thin[w])
        tau[w] = np.where(act, t1, t0)
        cross = act & np.isnan(surf[w]) & (t1 >= tau_surface)
        surf[w] = np.where(cross, P[j, 2], surf[w])
        near_s[w] |= cross & (near(t0, tau_surface) | near(t1, tau_surface))
        stop = act & (t1 >= tau_max)
        near_m[w] |= stop & (near(t0, tau_max) | near(t1, tau_max))
        run[w] &= ~stop
    if info is not None:
        info.update(thin=thin, near_surface=near_s, near_stop=near_m, stopped=~run)
    return np.stack([I + T * background, tau, T, surf])


def transfer_nodes(pos, m, h, gu, gv, pix, rot=None, centre=(0.0, 0.0, 0.0), source=None, kappa=None, kappa_scale=1.0,
                   tau_surface=1.0, tau_max=np.inf, background=0.0, clip=None, n_owned=None):
    """brute force for single nodes: pix an (M, 2) array of node indices -> (4, M)"""
    order, P, hh, y0, S = inputs(pos, m, h, kappa, source, rot, centre, kappa_scale, clip, n_owned)
    Po, ho = P[order], hh[order]
    out = np.empty((4, len(pix)))
    for q, (iu, iv) in enumerate(pix):
        b = np.sqrt((gu[iu] - Po[:, 0]) ** 2 + (gv[iv] - Po[:, 1]) ** 2)
        p = b / ho
        tau, T, I, surf = 0.0, 1.0, 0.0, np.nan
        for k in np.flatnonzero(p < 2.0):                 # in (D, id) order
            j = order[k]
            dtau = float(y0[j] * column_kernel(p[k]))
            a = -np.expm1(-dtau)
            I = I + (S[j] * T) * a
            T = T - T * a
            tau = tau + dtau
            if np.isnan(surf) and tau >= tau_surface:
                surf = P[j, 2]
            if tau >= tau_max:
                break
        out[:, q] = (I + T * background, tau, T, surf)
    return out
