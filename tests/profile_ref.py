"""numpy restatement of sph_profile / sph_profile_finish (include/summersph.h, "disc profiles"), written from the header's
definitions: the frame, the edge-table binning, the raw sums as sequential float64 sums in (bin, id) order -- or, with
shape="pieces", in the shape the header's "Order" gives the library's reduction (piece_sum) -- and the finish step.  numpy
evaluates every elementwise expression below without fused multiply-adds."""
import math

import numpy as np

NSUM, NCOL = 20, 29
COLUMNS = ["R_lo", "R_hi", "R_mean", "N", "M", "Sigma", "z_mean", "H", "vR_mean", "vphi_mean", "vz_mean", "sigma_R",
           "sigma_phi", "sigma_z", "u_mean", "c_s", "alpha_mean", "h_mean", "Omega", "kappa", "Q", "Mdot", "j", "tilt",
           "twist", "ecc", "peri", "phi_lo", "phi_hi"]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def axes(normal):
    """n^, e1, e2 of the header's frame rule"""
    nin = np.asarray(normal, dtype=np.float64)
    ln = math.sqrt((nin[0] * nin[0] + nin[1] * nin[1]) + nin[2] * nin[2])
    n = nin / ln
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) <= 0.9 else np.array([0.0, 1.0, 0.0])
    an = _dot(a, n)
    t = a - an * n
    e1 = t / math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    e2 = np.array([n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]])
    return n, e1, e2


def edges(r_min, r_max, n_r, log=False):
    k = np.arange(n_r + 1, dtype=np.float64)
    e = np.array([r_min * (r_max / r_min) ** (kk / n_r) for kk in k]) if log else r_min + (k * (r_max - r_min)) / n_r
    e[n_r] = r_max
    return e


def frame(pos, vel, centre, centre_v, normal):
    """per particle: r', v' (lab), X, Y, z', R, v_R, v_phi, v_z, phi"""
    n, e1, e2 = axes(normal)
    r = [pos[:, a] - centre[a] for a in range(3)]
    v = [vel[:, a] - centre_v[a] for a in range(3)]
    X, Y, Z = _dot(r, e1), _dot(r, e2), _dot(r, n)
    R = np.sqrt(X * X + Y * Y)
    v1, v2, vz = _dot(v, e1), _dot(v, e2), _dot(v, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        vR = np.where(R > 0, (X * v1 + Y * v2) / R, 0.0)
        vphi = np.where(R > 0, (X * v2 - Y * v1) / R, 0.0)
    phi = np.arctan2(Y, X)
    phi = np.where(phi >= math.pi, -math.pi, phi)
    return dict(r=r, v=v, X=X, Y=Y, Z=Z, R=R, vR=vR, vphi=vphi, vz=vz, phi=phi)


def bins(fr, r_min, r_max, n_r, n_phi=1, log=False, z_max=np.inf):
    """bin index per particle, -1 = not selected"""
    e = edges(r_min, r_max, n_r, log)
    R = fr["R"]
    sel = (R >= r_min) & (R < r_max) & (np.abs(fr["Z"]) < z_max)
    k = np.clip(np.searchsorted(e, R, side="right") - 1, 0, n_r - 1)
    pe = np.array([-math.pi + (2.0 * math.pi * j) / n_phi for j in range(n_phi + 1)])
    j = np.clip(np.searchsorted(pe[:n_phi], fr["phi"], side="right") - 1, 0, n_phi - 1)
    return np.where(sel, k * n_phi + j, -1)


def moments(fr, m, u, alpha, h, G, central_mass):
    """(n, 20) per-particle terms m q in the header's order"""
    r, v = fr["r"], fr["v"]
    l = [r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]]
    gm = G * central_mass
    if gm > 0:
        rr = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        w = [v[1] * l[2] - v[2] * l[1], v[2] * l[0] - v[0] * l[2], v[0] * l[1] - v[1] * l[0]]
        with np.errstate(invalid="ignore", divide="ignore"):
            e = [w[a] / gm - np.where(rr > 0, r[a] / rr, 0.0) for a in range(3)]
    else:
        e = [np.zeros_like(m)] * 3
    R, Z, vR, vphi, vz = fr["R"], fr["Z"], fr["vR"], fr["vphi"], fr["vz"]
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), m.shape)
    q = [np.ones_like(m), m, m * R, m * Z, m * (Z * Z), m * vR, m * vphi, m * vz, m * (vR * vR), m * (vphi * vphi),
         m * (vz * vz), m * u, m * alpha, m * h, m * l[0], m * l[1], m * l[2], m * e[0], m * e[1], m * e[2]]
    return np.stack(q, axis=1)


PIECE, WAVE = 1024, 64


def _wave_sum(q):
    """(n, 20) -> (20,): lane l adds rows l, l + 64, ... one after the other from 0.0, then the xor butterfly over the 64
    lanes (o = 32, 16, ..., 1: every lane adds its partner's value), lane 0's result"""
    n = q.shape[0]
    rows = -(-n // WAVE)
    pad = np.zeros((rows * WAVE, q.shape[1]))          # a lane past the end adds nothing; acc + 0.0 is acc (acc is never -0.0)
    pad[:n] = q
    acc = np.zeros((WAVE, q.shape[1]))
    for r in range(rows):
        acc = acc + pad[r * WAVE:(r + 1) * WAVE]
    lane = np.arange(WAVE)
    o = WAVE // 2
    while o > 0:
        acc = acc + acc[lane ^ o]
        o >>= 1
    return acc[0]


def piece_sum(q):
    """One bin's terms (n, 20), in id order, reduced in the shape of the header's "Order": pieces of 1024 positions from the
    run's start, each by _wave_sum; then the pieces, in piece order, by _wave_sum again."""
    q = np.asarray(q, dtype=np.float64)
    if q.shape[0] == 0:
        return np.zeros(q.shape[1])
    parts = np.stack([_wave_sum(q[p:p + PIECE]) for p in range(0, q.shape[0], PIECE)])
    return _wave_sum(parts)


def profile_sums(gas, h, G, r_min, r_max, n_r, n_phi=1, log=False, z_max=np.inf, centre=(0, 0, 0), centre_v=(0, 0, 0),
                 central_mass=0.0, normal=(0, 0, 1), shape="sequential", only_bins=None, n_owned=None):
    """raw sums (n_r n_phi, 20) in (bin, id) order; gas: dict of x y z vx vy vz u m alpha arrays in id order; h: one value or
    per particle.  shape: "sequential" (one term after the other) or "pieces" (piece_sum: the library's own shape).
    only_bins: the bins to evaluate (the others must be empty: asserted); n_owned: ids from there on are ghosts, never
    selected.  Returns (sums, bin per particle)."""
    pos = np.stack([gas[k] for k in "xyz"], axis=1)
    vel = np.stack([gas[k] for k in ("vx", "vy", "vz")], axis=1)
    fr = frame(pos, vel, np.asarray(centre, float), np.asarray(centre_v, float), normal)
    b = bins(fr, r_min, r_max, n_r, n_phi, log, z_max)
    al = gas.get("alpha")
    al = np.zeros_like(gas["m"]) if al is None else al
    q = moments(fr, gas["m"], gas["u"], al, h, G, central_mass)
    if n_owned is not None:
        b = np.where(np.arange(b.size) < n_owned, b, -1)
    nb = n_r * n_phi
    sums = np.zeros((nb, NSUM))
    if only_bins is not None:
        assert np.all(np.isin(b[b >= 0], only_bins)), "a selected particle outside only_bins"
    for bi in (range(nb) if only_bins is None else only_bins):
        idx = np.nonzero(b == bi)[0]                   # ascending id
        if idx.size:
            # sequential: left to right, one term after the other
            sums[bi] = piece_sum(q[idx]) if shape == "pieces" else np.add.accumulate(q[idx], axis=0)[-1]
    return sums, b


def finish(sums, r_min, r_max, n_r, n_phi, log, normal, gamma, gamma_m1, G):
    """the derived table (n_bins, 29), from the header's column definitions"""
    s = np.asarray(sums, dtype=np.float64).reshape(n_r, n_phi, NSUM)
    e = edges(r_min, r_max, n_r, log)
    n, e1, e2 = axes(normal)
    pi = math.pi
    t = np.zeros((n_r, n_phi, NCOL))
    with np.errstate(invalid="ignore", divide="ignore"):
        # ring-combined sums, sectors in j order
        m = np.zeros(n_r); mr = np.zeros(n_r); mvp = np.zeros(n_r)
        for j in range(n_phi):
            m = m + s[:, j, 1]; mr = mr + s[:, j, 2]; mvp = mvp + s[:, j, 6]
        Rk = mr / m
        Wk = (mvp / m) / Rk
        f = ((Rk * Rk) * (Rk * Rk)) * (Wk * Wk)
        k2 = np.full(n_r, np.nan)
        if n_r > 1:
            for k in range(n_r):
                a, b = (0, 1) if k == 0 else ((n_r - 2, n_r - 1) if k == n_r - 1 else (k - 1, k + 1))
                k2[k] = ((f[b] - f[a]) / (Rk[b] - Rk[a])) / ((Rk[k] * Rk[k]) * Rk[k])
        kappa = np.sqrt(np.where(k2 < 0, np.nan, k2))
        M = s[..., 1]

        def mean(q):
            return s[..., q] / M

        def disp(q1, q2):
            var = mean(q2) - mean(q1) * mean(q1)
            return np.sqrt(np.where(var < 0, 0.0, var))

        area = (pi * (e[1:] * e[1:] - e[:-1] * e[:-1])) / n_phi
        sig = M / area[:, None]
        t[..., 0] = e[:-1, None]
        t[..., 1] = e[1:, None]
        t[..., 2] = mean(2)
        t[..., 3] = s[..., 0]
        t[..., 4] = M
        t[..., 5] = sig
        t[..., 6] = mean(3)
        t[..., 7] = disp(3, 4)
        for c, q in ((8, 5), (9, 6), (10, 7)):
            t[..., c] = mean(q)
        t[..., 11] = disp(5, 8); t[..., 12] = disp(6, 9); t[..., 13] = disp(7, 10)
        t[..., 14] = mean(11)
        cs2 = (gamma * gamma_m1) * t[..., 14]
        t[..., 15] = np.sqrt(np.where(cs2 < 0, np.nan, cs2))
        t[..., 16] = mean(12)
        t[..., 17] = mean(13)
        t[..., 18] = t[..., 9] / t[..., 2]
        t[..., 19] = kappa[:, None]
        t[..., 20] = np.where(sig == 0, np.nan, (t[..., 15] * kappa[:, None]) / ((pi * G) * sig))
        t[..., 21] = -(((2.0 * pi * t[..., 2]) * sig) * t[..., 8])
        L = [s[..., 14], s[..., 15], s[..., 16]]
        Ln = np.sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2])
        t[..., 22] = Ln / M
        lh = [L[a] / Ln for a in range(3)]
        a1, a2, a3 = _dot(lh, e1), _dot(lh, e2), _dot(lh, n)
        t[..., 23] = np.arctan2(np.sqrt(a1 * a1 + a2 * a2), a3)
        t[..., 24] = np.arctan2(a2, a1)
        E = [s[..., 17], s[..., 18], s[..., 19]]
        t[..., 25] = np.sqrt((E[0] * E[0] + E[1] * E[1]) + E[2] * E[2]) / M
        t[..., 26] = np.where(M == 0, np.nan, np.arctan2(_dot(E, e2), _dot(E, e1)))
        j = np.arange(n_phi, dtype=np.float64)
        t[..., 27] = (-pi + (2.0 * pi * j) / n_phi)[None, :]
        t[..., 28] = (-pi + (2.0 * pi * (j + 1)) / n_phi)[None, :]
    return t.reshape(n_r * n_phi, NCOL)


def edge_margin(gas, r_min, r_max, n_r, n_phi=1, log=False, centre=(0, 0, 0), normal=(0, 0, 1), eps=1e-10):
    """True for the particles within eps R of a ring edge (or eps of a sector edge): rounding may bin them either way"""
    pos = np.stack([gas[k] for k in "xyz"], axis=1)
    fr = frame(pos, np.zeros_like(pos), np.asarray(centre, float), np.zeros(3), normal)
    e = edges(r_min, r_max, n_r, log)
    R = fr["R"]
    near = np.min(np.abs(R[:, None] - e[None, :]), axis=1) <= eps * np.maximum(R, 1e-300)
    if n_phi > 1:
        pe = np.array([-math.pi + (2.0 * math.pi * j) / n_phi for j in range(n_phi + 1)])
        near |= np.min(np.abs(fr["phi"][:, None] - pe[None, :]), axis=1) <= eps * 10
    return near
