"""numpy restatement of sph_gravity_at (include/summersph.h, "gravitational potential and acceleration at arbitrary
points"): the chunked direct O(N M) sum of the gas term with the softening potential phi and its pull gamma, the unsoftened
sink term, and per output row and point the sum of the terms' absolute values (the scale for comparisons of sums that
cancel).  The GPU walks a Barnes-Hut tree; with theta -> 0 it opens every node and the walk is this direct sum."""
import numpy as np

from energy_ref import phi_kernel

SOFT2 = 0.001 * 2.5            # the force walk's softening term, 0.001_dp * smoothing ([F]:275)


def gamma_kernel(q):
    """gamma(q) = M(q) / q^3, M the grav_table polynomial ([F]:81-101): the pull that belongs to phi_kernel,
    phi'(q) = q gamma(q); 1 / q^3 for q >= 2, 4/3 at q = 0"""
    q = np.asarray(q, dtype=np.float64)
    out = np.empty_like(q)
    a = q < 1.0
    b = (q >= 1.0) & (q < 2.0)
    c = q >= 2.0
    qa, qb = q[a], q[b]
    out[a] = 4.0 / 3.0 - 1.2 * qa**2 + 0.5 * qa**3
    out[b] = 8.0 / 3.0 - 3.0 * qb + 1.2 * qb**2 - qb**3 / 6.0 - 1.0 / (15.0 * qb**3)
    out[c] = 1.0 / q[c]**3
    return out


def gas_field(points, h, src, G, soft2=SOFT2, support=False, budget=4_000_000):
    """(out, scale), each (4, M): Phi and a of the sources src = (x, y, z, m) at points (M, 3) with the points' softening
    length h (a scalar or (M,)), and the sums of the absolute terms.  support=True: a third (4, M) array, the absolute
    terms of the sources inside the softening support (q < 2) only."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    m_pts = p.shape[0]
    sx, sy, sz, sm = (np.asarray(a, dtype=np.float64).reshape(-1) for a in src)
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (m_pts,))
    out, scale, sup = np.zeros((4, m_pts)), np.zeros((4, m_pts)), np.zeros((4, m_pts))
    if sx.size == 0:
        return (out, scale, sup) if support else (out, scale)
    chunk = max(1, budget // sx.size)
    for i0 in range(0, m_pts, chunk):
        i1 = min(m_pts, i0 + chunk)
        d = [p[i0:i1, k, None] - s[None, :] for k, s in enumerate((sx, sy, sz))]
        s = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + soft2)
        hi = hh[i0:i1, None]
        q = s / hi
        terms = [(G * sm[None, :] / hi) * phi_kernel(q)]
        f = (G * sm[None, :] / hi**3) * gamma_kernel(q)
        terms += [-(f * d[k]) for k in range(3)]
        inside = q < 2.0
        for c in range(4):
            out[c, i0:i1] = terms[c].sum(axis=1)
            scale[c, i0:i1] = np.abs(terms[c]).sum(axis=1)
            if support:
                sup[c, i0:i1] = np.where(inside, np.abs(terms[c]), 0.0).sum(axis=1)
    return (out, scale, sup) if support else (out, scale)


def sink_field(points, sinks, G):
    """(out, scale), each (4, M): the unsoftened field of the sinks (a dict with x y z m, or None) in sink order; massless
    sinks add 0; a point on a massive sink gets -inf and NaN"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    out, scale = np.zeros((4, p.shape[0])), np.zeros((4, p.shape[0]))
    if sinks is None:
        return out, scale
    sm = np.atleast_1d(np.asarray(sinks["m"], dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(sm.size):
            if sm[s] == 0.0:
                continue
            d = [p[:, k] - float(np.atleast_1d(sinks[a])[s]) for k, a in enumerate("xyz")]
            r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            gm = G * sm[s]
            terms = [-(gm / r)] + [-((gm / (r * r * r)) * d[k]) for k in range(3)]
            for c in range(4):
                out[c] += terms[c]
                scale[c] += np.abs(terms[c])
    return out, scale


def src_of(gas):
    return gas["x"], gas["y"], gas["z"], gas["m"]
