"""Brute-force numpy restatement of the variable-h rule, O(n^2), for n up to a few thousand.  Independent of the
oracle's search (oracle/sph_oracle_v.c finds candidates with a cell grid and recurses in C): here the octree splits are
replayed on index sets, the reach test is a full n x n matrix and every sum runs over explicit pair lists.

The rule, as csrc/varh.hip's and oracle/sph_oracle_v.c's headers state it:
  * leaf boxes: bbox-midpoint root, edge = largest extent, child bit = STRICT '>' against the node centre, child centre =
    centre +- edge/4, one particle per leaf, depth limit 1000; points that never separate stay "unresolved";
  * reach[i, j]: on every axis |x_i - c_j| < 2 h_j + e_j / 2 (strict);
  * density: D_i = {j : reach[i, j], r <= 2 h_i}, rho_i = sum m_j W(r, h_i), Omega_i from the same sum;
  * forces: the pair {i, j} counts iff the HIGHER-numbered partner's walk reaches the other's leaf and
    r <= 2 max(h_i, h_j); each partner gathers the other with both kernels;
  * calc_smoothing: one Newton step, accepted iff h_min < hn < h_max; re-evaluated (rho, Omega with the trial length on
    the tree of the OLD lengths) while the step grew by more than tol and hn < h_iter_cap.

coincident = "reference": unresolved points drop out of every sum, their own included (what the reference's walk does,
and the oracle).  coincident = "kernel": DESIGN section 2's documented deviation -- such a point's leaf is the node it is
stuck in at depth 1000, so it is reached like any other, a coincident partner counts W(0) in the density (and in
calc_smoothing's trial sums) and nothing in the forces.

Sums are accumulated in extended precision from fp64 terms formed in the reference's expression order."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

H_MIN_LENGTH = float(np.float32(0.01))
H_ITER_CAP = 10.0
VISC_EPS = float(np.float32(0.01))
ALPHA_DECAY = float(np.float32(0.15))
KERNEL_PI = float(np.float32(3.1415926535897932))
H_MARGIN = 1.1                     # varh.hip: trial lengths up to 1.1 h0 are served from the list's margin shell

# which clause ended calc_smoothing for a particle
KEPT_MAX, KEPT_MIN, LEFT_TOL, LEFT_CAP = "kept_max", "kept_min", "left_tol", "left_cap"


def leaf_boxes(x, y, z, max_depth=1000):
    """(lc[n, 3], ls[n], unresolved[n], root[4]): leaf centre and edge of every particle; for the members of a node that
    still holds several particles at the depth limit, that node's box, ls negated (the oracle's convention) and the flag"""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    n = x.size
    lc = np.zeros((n, 3)); ls = np.zeros(n); unresolved = np.zeros(n, dtype=bool)
    if n == 0:
        return lc, ls, unresolved, np.zeros(4)
    lo = [float(a.min()) for a in (x, y, z)]
    hi = [float(a.max()) for a in (x, y, z)]
    c0 = [(hi[a] + lo[a]) / 2.0 for a in range(3)]
    size0 = max(hi[a] - lo[a] for a in range(3))
    stack = [(np.arange(n), c0[0], c0[1], c0[2], size0, max_depth)]
    while stack:
        idx, cx, cy, cz, size, depth = stack.pop()
        if idx.size <= 1 or depth == 0:
            lc[idx] = (cx, cy, cz)
            ls[idx] = size if idx.size == 1 else -size
            unresolved[idx] = idx.size > 1
            continue
        ch = (x[idx] > cx).astype(np.int64) | ((y[idx] > cy).astype(np.int64) << 1) | ((z[idx] > cz).astype(np.int64) << 2)
        q = 0.25 * size
        for k in np.unique(ch):
            k = int(k)
            stack.append((idx[ch == k], cx + (q if k & 1 else -q), cy + (q if k & 2 else -q), cz + (q if k & 4 else -q),
                          size * 0.5, depth - 1))
    return lc, ls, unresolved, np.array([c0[0], c0[1], c0[2], size0])


def reach_limit(h, ls):
    """2 h_j + e_j / 2, [V]:380,479"""
    return 2.0 * np.asarray(h, dtype=np.float64) + np.abs(ls) / 2.0


def reach_matrix(pos, lc, ls, unresolved, h, coincident="reference"):
    """reach[i, j]: the walk of a body at x_i reaches particle j's leaf"""
    lim = reach_limit(h, ls)
    ok = np.ones((pos.shape[0], pos.shape[0]), dtype=bool)
    for a in range(3):
        ok &= np.abs(pos[:, a][:, None] - lc[:, a][None, :]) < lim[None, :]
    if coincident == "reference":
        ok[:, unresolved] = False
    else:
        assert coincident == "kernel"
        np.fill_diagonal(ok, True)              # the kernels add the self term unconditionally
    return ok


def lookup_kernel(w, dw, nq, r, hi):
    """lookup_kernel(r, hi) of [V]:119-141: linear interpolation in q = r / hi, normalised with hi and the REAL(4) pi"""
    dq = 2.0 / nq
    qi = r / hi
    inside = (qi >= 0.0) & (qi <= 2.0)
    qs = np.where(inside, qi, 0.0)
    k = np.minimum((qs / dq).astype(np.int64), nq - 1)
    a = (qs - k * dq) / dq
    W = np.where(inside, (1.0 - a) * w[k] + a * w[k + 1], 0.0)
    dW = np.where(inside, (1.0 - a) * dw[k] + a * dw[k + 1], 0.0)
    return W / (KERNEL_PI * (hi * hi * hi)), dW / (KERNEL_PI * ((hi * hi) * (hi * hi)))


def _rowsum(I, vals, n):
    """sum of vals per target I, accumulated in extended precision"""
    out = np.zeros(n, dtype=np.longdouble)
    if I.size:
        order = np.argsort(I, kind="stable")
        Is = I[order]
        starts = np.flatnonzero(np.r_[True, Is[1:] != Is[:-1]])
        out[Is[starts]] = np.add.reduceat(vals[order].astype(np.longdouble), starts)
    return out


class VarhRef:
    """gas: dict with x y z vx vy vz u m alpha h; number: the reference's particle numbers (default: the array index)"""

    def __init__(self, gas, number=None, gamma=1.4, eta=1.2, tol=1e-3, max_length=10.0, nq=2500, coincident="reference",
                 tables=None):
        for k in "x y z vx vy vz u m alpha h".split():
            setattr(self, k, np.ascontiguousarray(gas[k], dtype=np.float64).copy())
        self.n = self.x.size
        assert self.n <= 4000, "O(n^2) restatement"
        self.number = np.arange(self.n) if number is None else np.asarray(number)
        self.gamma, self.eta, self.tol, self.max_length, self.nq = gamma, eta, tol, max_length, nq
        self.mode = coincident
        if tables is None:
            from oracle import orc
            tables = orc.tables(nq)[:2]
        self.w, self.dw = tables
        self.pos = np.stack([self.x, self.y, self.z], axis=1)
        self.lc, self.ls, self.unresolved, self.root = leaf_boxes(self.x, self.y, self.z)
        self.reach = reach_matrix(self.pos, self.lc, self.ls, self.unresolved, self.h, coincident)
        d = self.pos[:, None, :] - self.pos[None, :, :]
        self.r = np.sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])      # [V]:481-482
        del d
        off = ~np.eye(self.n, dtype=bool)
        self.in_D = self.reach & (self.r <= 2.0 * self.h[:, None])              # j in D_i (the body itself included)
        hmax = np.maximum(self.h[:, None], self.h[None, :])
        higher = self.number[:, None] > self.number[None, :]
        decides = np.where(higher, self.reach, self.reach.T)                    # [V]:383
        self.in_F = decides & (self.r <= 2.0 * hmax) & off
        if coincident == "kernel":
            self.in_F_live = self.in_F & (self.r > 0.0)
        else:
            self.in_F_live = self.in_F
        # what a list build holds: ordered (i, j), j != i, j in D_i or {i, j} a force pair
        self.n_list_entries = int(np.count_nonzero((self.in_D | self.in_F) & off))
        self.n_D_entries = int(np.count_nonzero(self.in_D & off))
        self.n_F_pairs = int(np.count_nonzero(self.in_F)) // 2
        in_sup = (self.r <= 2.0 * hmax) & off
        self.asym = in_sup & (self.reach != self.reach.T)                       # pairs whose outcome the numbering decides
        self.n_asym_pairs = int(np.count_nonzero(self.asym)) // 2
        # r <= 2 h_i and yet i's walk does not reach j's (small) leaf
        self.n_support_no_reach = int(np.count_nonzero((self.r <= 2.0 * self.h[:, None]) & ~self.reach & off))

    # ---- density, [V]:440-496 ----------------------------------------------------------------------------------------
    def _density_rows(self, I, J, hi_of_I):
        Wj, dWj = lookup_kernel(self.w, self.dw, self.nq, self.r[I, J], hi_of_I)
        W_h = -(self.r[I, J] * dWj - 3 * Wj) / hi_of_I                          # [V]:487
        return self.m[J] * Wj, self.m[J] * W_h

    def density(self):
        I, J = np.nonzero(self.in_D)
        t_rho, t_om = self._density_rows(I, J, self.h[I])
        rho = _rowsum(I, t_rho, self.n)
        om = _rowsum(I, t_om, self.n)
        self.rho = rho.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.omega = (1.0 + (self.h / (3 * rho)) * om).astype(np.float64)   # [V]:455
            self.P = (self.gamma - 1.0) * self.u * self.rho                     # [V]:509
            self.c = np.sqrt(self.gamma * self.P / self.rho)                    # [V]:510
        return self

    # ---- forces, [V]:324-432 (gather form: every partner of a pair collects the other) -------------------------------
    def forces(self):
        I, J = np.nonzero(self.in_F_live)
        h, rho, om, P, c, al = self.h, self.rho, self.omega, self.P, self.c, self.alpha
        nv = self.pos[I] - self.pos[J]                                          # [V]:385
        dr = self.r[I, J]
        v = np.stack([self.vx[I] - self.vx[J], self.vy[I] - self.vy[J], self.vz[I] - self.vz[J]], axis=1)
        vdotr = v[:, 0] * nv[:, 0] + v[:, 1] * nv[:, 1] + v[:, 2] * nv[:, 2]
        vdotr = np.where(vdotr >= 0, 0.0, vdotr)
        nv = nv / dr[:, None]                                                   # [V]:392
        _, dWo = lookup_kernel(self.w, self.dw, self.nq, dr, h[I])
        _, dWn = lookup_kernel(self.w, self.dw, self.nq, dr, h[J])
        go, gn = nv * dWo[:, None], nv * dWn[:, None]
        vdotgradW = ((go[:, 0] * v[:, 0] + go[:, 1] * v[:, 1] + go[:, 2] * v[:, 2])
                     + (gn[:, 0] * v[:, 0] + gn[:, 1] * v[:, 1] + gn[:, 2] * v[:, 2])) / 2       # [V]:401
        avg_len = (h[I] + h[J]) / 2
        vis_nu = (avg_len * vdotr) / (dr * dr + VISC_EPS * avg_len * avg_len)   # [V]:405
        cbar = 0.5 * (c[I] + c[J]); abar = 0.5 * (al[I] + al[J])
        visc = (-abar * cbar * vis_nu + 2 * abar * vis_nu * vis_nu) / (0.5 * (rho[I] + rho[J]))   # [V]:410
        pri = P[I] / (om[I] * rho[I] * rho[I]); prj = P[J] / (om[J] * rho[J] * rho[J])
        cc = pri[:, None] * go + prj[:, None] * gn + visc[:, None] * (gn + go) / 2               # [V]:413-414
        acc = [-_rowsum(I, self.m[J] * cc[:, a], self.n) for a in range(3)]
        self.ax, self.ay, self.az = (a.astype(np.float64) for a in acc)
        self.du = _rowsum(I, self.m[J] * vdotgradW * (pri + 0.5 * visc), self.n).astype(np.float64)
        dal = _rowsum(I, self.m[J] * vdotgradW, self.n).astype(np.float64)
        # local scales: the sums of the terms' magnitudes (what a rounding error of a sum is relative to)
        self.a_scale = _rowsum(I, np.abs(self.m[J]) * np.sqrt(cc[:, 0] ** 2 + cc[:, 1] ** 2 + cc[:, 2] ** 2), self.n).astype(np.float64)
        self.du_scale = _rowsum(I, np.abs(self.m[J] * vdotgradW * (pri + 0.5 * visc)), self.n).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.dalpha_scale = (_rowsum(I, np.abs(self.m[J] * vdotgradW), self.n).astype(np.float64) / self.rho
                                 + np.abs(ALPHA_DECAY * ((0.1 - al) * c / h)))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = dal / self.rho
            self.dalpha = np.where(t > 0.0, t, 0.0) + ALPHA_DECAY * ((0.1 - al) * c / h)         # [V]:346
        return self

    def evaluate(self):
        return self.density().forces()

    # ---- calc_smoothing, [V]:515-546 ---------------------------------------------------------------------------------
    def _density_one(self, i, hn):
        J = np.flatnonzero(self.reach[i])
        I = np.full(J.size, i)
        t_rho, t_om = self._density_rows(I, J, hn)
        rho = np.sum(t_rho.astype(np.longdouble)); om = np.sum(t_om.astype(np.longdouble))
        return float(rho), float(1.0 + (hn / (3 * rho)) * om)                   # [V]:535

    def update_h(self):
        """one calc_smoothing pass on the tree of the last evaluation.  Returns a record per particle: n_reeval (Newton
        re-evaluations of rho), max_trial (largest trial hn / h0 that was evaluated; 0 if none) and clause."""
        n = self.n
        h_new = self.h.copy(); rho = self.rho.copy(); om = self.omega.copy()
        n_reeval = np.zeros(n, dtype=np.int64); max_trial = np.zeros(n); clause = np.empty(n, dtype=object)
        first = np.zeros(n)
        err = np.seterr(divide="ignore", invalid="ignore")       # an unresolved point has rho = 0 in the reference's mode, as in [V]
        for i in range(n):
            h0 = float(self.h[i]); old = h0
            t = self.eta / h0
            hn = h0 * (1 + ((self.m[i] * (t * t * t) / rho[i]) - 1) / (3 * om[i]))             # [V]:527
            first[i] = hn
            if hn < self.max_length and hn > H_MIN_LENGTH:                                     # [V]:528
                clause[i] = LEFT_TOL
                while True:
                    if not ((hn - old) / old) > self.tol:
                        clause[i] = LEFT_TOL
                        break
                    if not hn < H_ITER_CAP:
                        clause[i] = LEFT_CAP
                        break
                    old = hn
                    rho[i], om[i] = self._density_one(i, hn)
                    n_reeval[i] += 1
                    max_trial[i] = max(max_trial[i], hn / h0)
                    t = self.eta / hn
                    hn = hn * (1 + ((self.m[i] * (t * t * t)) / rho[i] - 1) / (3 * om[i]))     # [V]:538
                h_new[i] = hn
            else:
                clause[i] = KEPT_MAX if not hn < self.max_length else KEPT_MIN                 # [V]:541
        np.seterr(**err)
        rec = SimpleNamespace(n_reeval=n_reeval, max_trial=max_trial, clause=clause, first=first)
        self.h_new, self.rho_new, self.omega_new, self.h_record = h_new, rho, om, rec
        return rec


def route_classes(rec):
    """the six classes of tests/varh_sets.h_routes, as boolean masks over the particles"""
    accepted = (rec.clause == LEFT_TOL) | (rec.clause == LEFT_CAP)
    return {
        "no_reeval": accepted & (rec.n_reeval == 0),
        "list_route": accepted & (rec.n_reeval > 0) & (rec.max_trial <= H_MARGIN),
        "cell_walk_route": accepted & (rec.max_trial > H_MARGIN),
        "kept_max": rec.clause == KEPT_MAX,
        "kept_min": rec.clause == KEPT_MIN,
        "left_cap": rec.clause == LEFT_CAP,
    }


def edge_margins(ref, exclude=()):
    """smallest relative distance of any pair from a support edge (r vs 2 h_i, 2 h_j) and of any particle from a reach
    boundary (|x_i - c_j| vs 2 h_j + e_j / 2 on the axis that decides), pairs in `exclude` (a set of frozensets) left out.
    A count check is meaningful only where both are far above rounding."""
    n = ref.n
    off = ~np.eye(n, dtype=bool)
    for pair in exclude:
        i, j = tuple(pair)
        off[i, j] = off[j, i] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        sup = np.abs(ref.r / (2.0 * ref.h[:, None]) - 1.0)
        sup = np.minimum(sup, sup.T)
    support = float(np.min(sup[off])) if np.any(off) else np.inf
    lim = reach_limit(ref.h, ref.ls)
    # L-infinity distance to the leaf centre against the limit: the reach test flips where they are equal
    dmax = np.zeros((n, n))
    for a in range(3):
        dmax = np.maximum(dmax, np.abs(ref.pos[:, a][:, None] - ref.lc[:, a][None, :]))
    with np.errstate(divide="ignore", invalid="ignore"):
        rb = np.abs(dmax / lim[None, :] - 1.0)
    near = off & (ref.r <= 2.2 * np.maximum(ref.h[:, None], ref.h[None, :]))       # only pairs a list can hold matter
    reach_b = float(np.min(rb[near])) if np.any(near) else np.inf
    return support, reach_b


def rate_excess(d, mag, scale):
    """d_i / (1e-11 mag_i + 1e-13 scale_i) for the error d of an element of magnitude mag whose terms' magnitudes sum to
    scale: <= 1 passes; 0 where the two agree exactly, inf where the bar is 0"""
    bar = 1e-11 * mag + 1e-13 * scale
    ex = np.zeros(d.shape)
    nz = d > 0.0
    ex[nz] = np.where(bar[nz] > 0.0, d[nz] / np.where(bar[nz] > 0.0, bar[nz], 1.0), np.inf)
    return ex


def next_dt(ref, dt, scale=0.25):
    """get_next_timestep, [V]:1035-1065, from an evaluated VarhRef (candidates that are NaN are skipped, as a '<' scan does)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v2 = ref.vx * ref.vx + ref.vy * ref.vy + ref.vz * ref.vz
        a2 = ref.ax * ref.ax + ref.ay * ref.ay + ref.az * ref.az
        cand = np.concatenate([np.sqrt(v2 / a2), ref.u / np.abs(ref.du), ref.h / np.sqrt(v2), ref.h / (ref.c + 1.2 * ref.c)])
    cand = float(np.min(cand[~np.isnan(cand)])) * scale if ref.n else np.inf
    dt_max, dt_min = float(np.float32(0.1)), float(np.float32(0.0001))
    if cand > 2 * dt and 1.5 * dt < dt_max:
        return 1.5 * dt
    if cand < 0.5 * dt and dt * 0.5 > dt_min:
        return 0.5 * dt
    return dt
