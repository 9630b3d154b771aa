"""Brute-force numpy restatement of sph_force_terms (include/summersph.h), O(n^2), for n up to 4000: the rates of one force
evaluation split by physical term, every pair sum over an explicit pair list, accumulated in extended precision from fp64
terms formed in the reference's expression order (as tests/varh_ref.py does for the totals).

  fixed h     all ordered pairs (i, j) with 0 < r <= 2 h; the kernel is the oracle's table (oracle.orc.tables /
              lookup_kernel); rho, P and c are the oracle's density pass.  [F]:356-391 with [F]:381-383 and [F]:387 split.
  variable h  the pair sets and per-pair quantities of tests/varh_ref.VarhRef (reach rule, numbering rule, coincident
              mode), with [V]:413-416 and [V]:419-421 split.

Besides each row (TermRef.rows, (16, n) in capi.TERM_ROWS order) the restatement returns the row's scale sum_j |term_j|
(TermRef.scale): what a rounding error of the sum is relative to.  Rows 9-11 (gas self-gravity) are +0.0 with scale 0: the
tests take that term from oracle.orc_grav.
"""
from __future__ import annotations

import numpy as np

import varh_ref as VR

NROW = 16
H_FIXED = 2.5
A_P, A_V, A_S, A_G, DU_P, DU_V, AL_SRC, AL_DECAY = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), 12, 13, 14, 15
ALPHA_FLOOR = 0.1


class TermRef:
    """rows, scale: (16, n); totals: ax ay az du dalpha of the recomposition (rows summed in extended precision)"""

    def __init__(self, n):
        self.n = n
        self.rows = np.zeros((NROW, n))
        self.scale = np.zeros((NROW, n))
        self.n_pairs = 0
        self.n_approaching = 0
        self.list_len = np.zeros(n, dtype=np.int64)

    def recomposed(self):
        """(ax, ay, az, du, dalpha) and their summed scales"""
        r, s = self.rows.astype(np.longdouble), self.scale
        a = [(r[k] + r[3 + k] + r[6 + k] + r[9 + k]).astype(np.float64) for k in range(3)]
        sa = [s[k] + s[3 + k] + s[6 + k] + s[9 + k] for k in range(3)]
        return (a + [(r[DU_P] + r[DU_V]).astype(np.float64), (r[AL_SRC] + r[AL_DECAY]).astype(np.float64)],
                sa + [s[DU_P] + s[DU_V], s[AL_SRC] + s[AL_DECAY]])


def _sink_rows(out, pos, sinks, G):
    """the gas side of sink_gravforces ([F]:567-576, [V]:691-): a -= m_s (G v / dr^3), in sink order"""
    n = pos.shape[0]
    acc = np.zeros((3, n), dtype=np.longdouble); sc = np.zeros((3, n))
    for s in range(int(np.asarray(sinks["x"]).size)):
        v = pos - np.array([sinks["x"][s], sinks["y"][s], sinks["z"][s]])[None, :]
        dr = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        d3 = dr * dr * dr
        for a in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = sinks["m"][s] * (G * v[:, a] / d3)
            acc[a] -= t
            sc[a] += np.abs(t)
    out.rows[A_S] = acc.astype(np.float64)
    out.scale[A_S] = sc


def _pair_rows(out, I, J, m, g, vdotgradW, pri_term, visc_term, pri, visc):
    """the pair sums from per-pair vectors: pri_term / visc_term (npairs, 3) are the bracket's two parts times the gradient"""
    n = out.n
    mj = m[J]
    for a in range(3):
        out.rows[a] = (-VR._rowsum(I, mj * pri_term[:, a], n)).astype(np.float64)
        out.scale[a] = VR._rowsum(I, np.abs(mj * pri_term[:, a]), n).astype(np.float64)
        out.rows[3 + a] = (-VR._rowsum(I, mj * visc_term[:, a], n)).astype(np.float64)
        out.scale[3 + a] = VR._rowsum(I, np.abs(mj * visc_term[:, a]), n).astype(np.float64)
    tP, tV = mj * vdotgradW * pri, mj * vdotgradW * (0.5 * visc)
    out.rows[DU_P] = VR._rowsum(I, tP, n).astype(np.float64); out.scale[DU_P] = VR._rowsum(I, np.abs(tP), n).astype(np.float64)
    out.rows[DU_V] = VR._rowsum(I, tV, n).astype(np.float64); out.scale[DU_V] = VR._rowsum(I, np.abs(tV), n).astype(np.float64)
    out.min_pair_duV = float(tV.min()) if tV.size else 0.0
    return VR._rowsum(I, mj * vdotgradW, n).astype(np.float64), VR._rowsum(I, np.abs(mj * vdotgradW), n).astype(np.float64)


def _alpha_rows(out, dal, dal_scale, rho, alpha, c, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = dal / rho
        out.rows[AL_SRC] = np.where(t > 0.0, t, 0.0)                                       # [F]:317, [V]:346
        out.scale[AL_SRC] = dal_scale / rho
        out.rows[AL_DECAY] = VR.ALPHA_DECAY * ((ALPHA_FLOOR - alpha) * c / h)
    out.scale[AL_DECAY] = np.abs(out.rows[AL_DECAY])


def fixed_terms(gas, sinks, h=H_FIXED, nq=5000, targets=None):
    """the sixteen rows of a fixed-h evaluation.  Also leaves rho, P, c (the oracle's) on the result.
    targets: an index array -- the rows, scales and list_len of these particles only (the others stay 0): O(len(targets) n),
    for the sets too large for the whole matrix.  With targets, n_pairs, n_coincident, n_approaching and n_receding are NOT
    counts of the set: they count the ordered pairs (i, j) with i a target, halved like the full counts -- use them with the
    whole set only.
    Cost: the distances are formed in blocks of 16e6 elements; len(targets) n (n^2 without targets) may be 1.28e8 at the most,
    which is n = 11300 for a full restatement."""
    from oracle import orc
    o = orc.Oracle(gas, sinks, h=h, nq=nq, nthreads=orc.max_threads())
    n = o.n
    rows = np.arange(n) if targets is None else np.asarray(targets, dtype=np.int64)
    assert rows.size * n <= 4000 * 4000 * 8, "O(len(targets) n) restatement: at most 1.28e8 target-particle pairs"
    o.density()
    out = TermRef(n)
    out.rho, out.P, out.c = o.rho.copy(), o.P.copy(), o.c.copy()
    pos = np.stack([o.x, o.y, o.z], axis=1)
    vel = np.stack([o.vx, o.vy, o.vz], axis=1)
    I, J, dr, zero = [], [], [], 0
    for a in range(0, rows.size, 4000):                 # (the whole matrix of a set of <= 4000 in one block, as before)
        blk = rows[a:a + 4000]
        step = max(1, 16_000_000 // n)
        for b in range(0, blk.size, step):
            d = pos[blk[b:b + step], None, :] - pos[None, :, :]
            r = np.sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2])       # [F]:356-357
            del d
            i, j = np.nonzero((r > 0.0) & (r <= 2.0 * h))
            dr.append(r[i, j]); I.append(blk[b:b + step][i]); J.append(j)
            zero += int(np.count_nonzero(r == 0.0))
            del r
    I, J, dr = np.concatenate(I), np.concatenate(J), np.concatenate(dr)
    out.n_pairs = I.size // 2
    out.list_len = np.bincount(I, minlength=n)
    out.n_coincident = (zero - rows.size) // 2
    nv = pos[I] - pos[J]
    v = vel[I] - vel[J]                                                            # [F]:358
    vdotr = v[:, 0] * nv[:, 0] + v[:, 1] * nv[:, 1] + v[:, 2] * nv[:, 2]
    out.n_approaching = int(np.count_nonzero(vdotr < 0.0)) // 2
    out.n_receding = int(np.count_nonzero(vdotr > 0.0)) // 2
    vdotr = np.where(vdotr >= 0, 0.0, vdotr)                                       # [F]:361
    nv = nv / dr[:, None]                                                          # [F]:363
    _, dW = orc.lookup_kernel(dr, h, nq)                                           # [F]:366
    g = nv * dW[:, None]
    vdotgradW = g[:, 0] * v[:, 0] + g[:, 1] * v[:, 1] + g[:, 2] * v[:, 2]          # [F]:370
    vis_nu = (h * vdotr) / (dr * dr + VR.VISC_EPS * h * h)                         # [F]:373
    cbar = 0.5 * (o.c[I] + o.c[J]); abar = 0.5 * (o.alpha[I] + o.alpha[J])
    visc = (-abar * cbar * vis_nu + 2 * abar * vis_nu * vis_nu) / (0.5 * (o.rho[I] + o.rho[J]))     # [F]:378
    pri = o.P[I] / (o.rho[I] * o.rho[I]); prj = o.P[J] / (o.rho[J] * o.rho[J])
    dal, dal_scale = _pair_rows(out, I, J, o.m, g, vdotgradW, (pri + prj)[:, None] * g, visc[:, None] * g, pri, visc)
    _sink_rows(out, pos, sinks, float(orc.lib().orc_G()))
    _alpha_rows(out, dal, dal_scale, o.rho, o.alpha, o.c, h)
    return out


def varh_terms(ref, sinks=None):
    """the sixteen rows from a VarhRef whose density() has run (its pair set in_F_live, its rho, Omega, P, c)"""
    from oracle import orc_v
    n = ref.n
    out = TermRef(n)
    I, J = np.nonzero(ref.in_F_live)
    out.n_pairs = I.size // 2
    out.list_len = np.bincount(I, minlength=n)
    h, rho, om, P, c, al = ref.h, ref.rho, ref.omega, ref.P, ref.c, ref.alpha
    nv = ref.pos[I] - ref.pos[J]                                                   # [V]:385
    dr = ref.r[I, J]
    v = np.stack([ref.vx[I] - ref.vx[J], ref.vy[I] - ref.vy[J], ref.vz[I] - ref.vz[J]], axis=1)
    vdotr = v[:, 0] * nv[:, 0] + v[:, 1] * nv[:, 1] + v[:, 2] * nv[:, 2]
    out.n_approaching = int(np.count_nonzero(vdotr < 0.0)) // 2
    out.n_receding = int(np.count_nonzero(vdotr > 0.0)) // 2
    vdotr = np.where(vdotr >= 0, 0.0, vdotr)
    nv = nv / dr[:, None]                                                          # [V]:392
    _, dWo = VR.lookup_kernel(ref.w, ref.dw, ref.nq, dr, h[I])
    _, dWn = VR.lookup_kernel(ref.w, ref.dw, ref.nq, dr, h[J])
    go, gn = nv * dWo[:, None], nv * dWn[:, None]
    vdotgradW = ((go[:, 0] * v[:, 0] + go[:, 1] * v[:, 1] + go[:, 2] * v[:, 2])
                 + (gn[:, 0] * v[:, 0] + gn[:, 1] * v[:, 1] + gn[:, 2] * v[:, 2])) / 2            # [V]:401
    avg_len = (h[I] + h[J]) / 2
    vis_nu = (avg_len * vdotr) / (dr * dr + VR.VISC_EPS * avg_len * avg_len)       # [V]:405
    cbar = 0.5 * (c[I] + c[J]); abar = 0.5 * (al[I] + al[J])
    visc = (-abar * cbar * vis_nu + 2 * abar * vis_nu * vis_nu) / (0.5 * (rho[I] + rho[J]))       # [V]:410
    pri = P[I] / (om[I] * rho[I] * rho[I]); prj = P[J] / (om[J] * rho[J] * rho[J])
    dal, dal_scale = _pair_rows(out, I, J, ref.m, None, vdotgradW, pri[:, None] * go + prj[:, None] * gn,
                                visc[:, None] * (gn + go) / 2, pri, visc)          # [V]:413-414, 419-421
    if sinks is not None:
        _sink_rows(out, ref.pos, sinks, float(orc_v.lib().orcv_G()))
    _alpha_rows(out, dal, dal_scale, rho, al, c, h)
    return out


def excess(got, ref, rows=None):
    """per row: the largest share of the bar VR.rate_excess (1e-11 of the element's magnitude + 1e-13 of the row's own
    scale) that |got - ref| uses, over the finite reference elements; <= 1 passes.  got: (16, n)"""
    rows = range(NROW) if rows is None else rows
    out = {}
    for k in rows:
        fin = np.isfinite(ref.rows[k])
        ex = VR.rate_excess(np.abs(got[k][fin] - ref.rows[k][fin]), np.abs(ref.rows[k][fin]), ref.scale[k][fin])
        out[k] = float(np.max(ex)) if ex.size else 0.0
        if not np.all(np.isfinite(got[k][fin])):
            out[k] = np.inf
    return out
