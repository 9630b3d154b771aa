"""numpy restatement of sph_energy (include/summersph.h, "conserved totals and gravitational potential"): the softened
direct O(N^2) sum for the gas self-potential (chunked), the unsoftened sink potentials, the 28 sums and the derived
totals.  The GPU walks a Barnes-Hut tree; with theta -> 0 it opens every node and the walk is this direct sum."""
import numpy as np

NSUM = 28
SOFT2 = 0.001 * 2.5            # the reference's softening term, 0.001_dp * smoothing ([F]:275)
SUMS = ["N", "M", "mx", "my", "mz", "px", "py", "pz", "lx", "ly", "lz", "K", "U", "W_self", "W_gs",
        "Ns", "Ms", "Mx_s", "My_s", "Mz_s", "Px_s", "Py_s", "Pz_s", "Lx_s", "Ly_s", "Lz_s", "K_s", "W_ss"]


def phi_kernel(q):
    """phi(q) of the cubic-spline softening: q^2 phi'(q) is the grav_table polynomial ([F]:81-101), phi = -1/q for q >= 2"""
    q = np.asarray(q, dtype=np.float64)
    out = np.empty_like(q)
    a = q < 1.0
    b = (q >= 1.0) & (q < 2.0)
    c = q >= 2.0
    qa, qb = q[a], q[b]
    out[a] = (2.0 / 3.0) * qa**2 - 0.3 * qa**4 + 0.1 * qa**5 - 1.4
    out[b] = (4.0 / 3.0) * qb**2 - qb**3 + 0.3 * qb**4 - qb**5 / 30.0 - 1.6 + 1.0 / (15.0 * qb)
    out[c] = -1.0 / q[c]
    return out


def grav_table_poly(q):
    """the force's mass fraction, [F]:81-101 (1 outside the support)"""
    q = np.asarray(q, dtype=np.float64)
    out = np.ones_like(q)
    a = q <= 1.0
    b = (q > 1.0) & (q <= 2.0)
    qa, qb = q[a], q[b]
    out[a] = (40.0 * qa**3 - 36.0 * qa**5 + 15.0 * qa**6) / 30.0
    out[b] = (80.0 * qb**3 - 90.0 * qb**4 + 36.0 * qb**5 - 5.0 * qb**6 - 2.0) / 30.0
    return out


def self_potential(x, y, z, m, h, G, soft2=SOFT2, chunk=512):
    """Phi_self,i = sum_{j != i} (G m_j / h_i) phi(sqrt(|r_i - r_j|^2 + soft2) / h_i); h scalar or per particle"""
    x, y, z, m = (np.asarray(a, dtype=np.float64) for a in (x, y, z, m))
    n = x.size
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    out = np.zeros(n)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        d2 = ((x[i0:i1, None] - x[None, :])**2 + (y[i0:i1, None] - y[None, :])**2) + (z[i0:i1, None] - z[None, :])**2
        s = np.sqrt(d2 + soft2)
        hi = hh[i0:i1, None]
        t = (G * m[None, :] / hi) * phi_kernel(s / hi)
        t[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0          # the target itself, by identity
        out[i0:i1] = t.sum(axis=1)
    return out


def sink_potential(x, y, z, sinks, G):
    """Phi_sink,i = -sum_s G M_s / |r_i - R_s| (unsoftened; massless sinks add 0)"""
    out = np.zeros(np.asarray(x).size)
    for s in range(np.asarray(sinks["m"]).size):
        if sinks["m"][s] == 0.0:
            continue
        r = np.sqrt((np.asarray(x) - sinks["x"][s])**2 + (np.asarray(y) - sinks["y"][s])**2 + (np.asarray(z) - sinks["z"][s])**2)
        out -= G * sinks["m"][s] / r
    return out


def gas_terms(gas, phi_self, phi_sink):
    """(n, 15) per-particle terms of the gas sums, in the header's order"""
    x, y, z, vx, vy, vz, u, m = (np.asarray(gas[k], dtype=np.float64) for k in "x y z vx vy vz u m".split())
    return np.stack([np.ones_like(m), m, m * x, m * y, m * z, m * vx, m * vy, m * vz,
                     m * (y * vz - z * vy), m * (z * vx - x * vz), m * (x * vy - y * vx),
                     0.5 * m * (vx * vx + vy * vy + vz * vz), m * u, 0.5 * m * phi_self, m * phi_sink], axis=1)


def sink_terms(sinks, G):
    """(ns, 13) per-sink terms of the sink sums (the last: each sink's pair terms with the later sinks)"""
    sx, sy, sz, svx, svy, svz, sm = (np.atleast_1d(np.asarray(sinks[k], dtype=np.float64)) for k in "x y z vx vy vz m".split())
    w = np.zeros(sm.size)
    for a in range(sm.size):
        for b in range(a + 1, sm.size):
            if sm[a] * sm[b] != 0.0:
                w[a] -= G * sm[a] * sm[b] / np.sqrt((sx[a] - sx[b])**2 + (sy[a] - sy[b])**2 + (sz[a] - sz[b])**2)
    return np.stack([np.ones_like(sm), sm, sm * sx, sm * sy, sm * sz, sm * svx, sm * svy, sm * svz,
                     sm * (sy * svz - sz * svy), sm * (sz * svx - sx * svz), sm * (sx * svy - sy * svx),
                     0.5 * sm * (svx * svx + svy * svy + svz * svz), w], axis=1)


def energy_sums(gas, sinks, G, h, self_gravity=True, rank0=True, phi_self=None, scales=False):
    """(sums[28], phi = Phi_self + Phi_sink per gas particle) -- with scales=True also the sums of the terms' absolute
    values (the scale of each sum, for relative comparisons of sums that cancel).  gas: x y z vx vy vz u m; sinks: x y z
    vx vy vz m (may be empty or None); h: params.h or the per-particle h.  phi_self: given (e.g. a Barnes-Hut result)
    instead of the direct sum."""
    x, y, z, m = (np.asarray(gas[k], dtype=np.float64) for k in "x y z m".split())
    if phi_self is None:
        phi_self = self_potential(x, y, z, m, h, G) if self_gravity and x.size else np.zeros(x.size)
    phi_sink = sink_potential(x, y, z, sinks, G) if sinks is not None else np.zeros(x.size)
    t = gas_terms(gas, phi_self, phi_sink)
    s = np.zeros(NSUM)
    sc = np.zeros(NSUM)
    s[:15] = t.sum(axis=0)
    sc[:15] = np.abs(t).sum(axis=0)
    if rank0 and sinks is not None and np.atleast_1d(sinks["m"]).size:
        ts = sink_terms(sinks, G)
        s[15:] = ts.sum(axis=0)
        sc[15:] = np.abs(ts).sum(axis=0)
    return (s, phi_self + phi_sink, sc) if scales else (s, phi_self + phi_sink)


def totals(sums):
    """the derived totals of (summed) sums: E = K + U + W_self + W_gs + K_s + W_ss, total P and L, centre of mass"""
    s = np.asarray(sums, dtype=np.float64)
    d = {k: float(v) for k, v in zip(SUMS, s)}
    d["E"] = s[11] + s[12] + s[13] + s[14] + s[26] + s[27]
    d["P"] = s[5:8] + s[20:23]
    d["L"] = s[8:11] + s[23:26]
    mt = s[1] + s[16]
    d["com"] = (s[2:5] + s[17:20]) / mt if mt > 0 else np.zeros(3)
    return d


def rows_to_dicts(g, prefix, variable=False):
    """the gas and sink dicts of a trajectory fixture's state `prefix` (e.g. 'sph_s5_')"""
    names = "x y z vx vy vz u m alpha".split() + (["h"] if variable else [])
    gas = {k: np.asarray(g[prefix + k], dtype=np.float64) for k in names}
    sinks = {k: np.atleast_1d(np.asarray(g[prefix + "s" + k], dtype=np.float64)) for k in "x y z vx vy vz m".split()}
    return gas, sinks
