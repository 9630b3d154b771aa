"""A numpy restatement of one advance of the tracer grains (include/summersph.h, sph_dust, "Scheme"): the half kick with
the stored sample, the drift, the fates, the gas and the sinks at the new position, the second half kick.  The gas means
come from sample_ref.sample (gas=dict(pos, m, h, vel, u)) or are given as arrays (gas=dict(rho, vg, u)).  Plain float64
numpy in the documented order of operations; numpy never fuses a multiply with an add."""
import numpy as np

EPSTEIN, FIXED_TS = 0, 1
ALIVE, ACCRETED, CULLED, NONFINITE = 0, 1, 2, 3
C_EPSTEIN = float(np.sqrt(8.0 / np.pi))


def half_kick(v, a, vg, r, tau):
    """v (M, 3) after the exact solution of dv/dt = a - r (v - vg) over tau; r (M,)"""
    v = np.array(v, dtype=np.float64)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), v.shape[:1])
    with np.errstate(all="ignore"):
        k = r * tau
        drag = k > 0.0
        free = ~drag & (r == 0.0)
        ks = np.where(drag, k, 1.0)
        e = -np.expm1(-ks)
        f = tau * (e / ks)
        vd = (v + (vg - v) * e[:, None]) + a * f[:, None]
        vf = v + a * tau
    return np.where(drag[:, None], vd, np.where(free[:, None], vf, v))


def sink_accel(x, sinks, G):
    """the sinks' acceleration at x (M, 3): sink order, sph_gravity_at's arithmetic.  sinks: dict of x y z m arrays"""
    a = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for k in range(len(sinks["m"])):
            sm = float(sinks["m"][k])
            if sm == 0.0:
                continue
            dx, dy, dz = x[:, 0] - sinks["x"][k], x[:, 1] - sinks["y"][k], x[:, 2] - sinks["z"][k]
            rr = np.sqrt((dx * dx + dy * dy) + dz * dz)
            f = (G * sm) / ((rr * rr) * rr)
            a[:, 0] = a[:, 0] - f * dx
            a[:, 1] = a[:, 1] - f * dy
            a[:, 2] = a[:, 2] - f * dz
    return a


def drag_rate(rho, u, par, law, rho_grain, gamma, gamma_m1):
    """r = 1 / t_s where rho != 0, else 0"""
    with np.errstate(all="ignore"):
        if law == EPSTEIN:
            r = ((rho * np.sqrt((gamma * gamma_m1) * u)) * C_EPSTEIN) / (rho_grain * par)
        else:
            r = 1.0 / par
    return np.where(rho != 0.0, r, 0.0)


def gas_at(x, gas):
    """(rho, vg (M, 3), u) at x: the given arrays, or sample_ref's sums of the particle set"""
    if "rho" in gas:
        return np.asarray(gas["rho"], float), np.asarray(gas["vg"], float).reshape(-1, 3), np.asarray(gas["u"], float)
    import sample_ref
    A = np.vstack([gas["vel"].T, gas["u"][None, :]])
    out, den, _ = sample_ref.sample(x, gas["pos"], gas["m"], gas["h"], A=A, normalise=True)
    return den, out[:3].T.copy(), out[3]


def advance(x, v, par, S, delta, gas, sinks, *, G=1.0, law=FIXED_TS, rho_grain=1.0, gamma=1.4, gamma_m1=0.4, remove=False,
            radii=None, bound=np.inf):
    """One advance over delta of M grains.  S = dict(a (M, 3), vg (M, 3), r (M,)), the stored sample.  gas: see gas_at, for
    the NEW positions.  Returns dict(x, v, S, fate (M,), sink (M,), rho, u): a grain with a fate keeps the x and v it had
    when the fate was set."""
    x, v = np.array(x, dtype=np.float64).reshape(-1, 3), np.array(v, dtype=np.float64).reshape(-1, 3)
    M = x.shape[0]
    fate, by = np.zeros(M, np.int32), np.full(M, -1, np.int32)
    move = bool(delta > 0.0 and np.isfinite(delta))
    if move:
        v = half_kick(v, S["a"], S["vg"], S["r"], 0.5 * delta)
        with np.errstate(all="ignore"):
            x = x + v * delta
        if remove:
            for k in range(len(sinks["m"])):
                d = x - np.array([sinks["x"][k], sinks["y"][k], sinks["z"][k]])
                with np.errstate(all="ignore"):
                    hit = (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < radii[k]) & (fate == 0)
                fate[hit], by[hit] = ACCRETED, k
            with np.errstate(all="ignore"):
                out = (np.abs(x) > bound).any(axis=1) & (fate == 0)
            fate[out] = CULLED
    bad = ~(np.isfinite(x).all(axis=1) & np.isfinite(v).all(axis=1))
    fate[bad], by[bad] = NONFINITE, -1
    rho, vg, u = gas_at(x, gas)
    vg = np.where((rho != 0.0)[:, None], vg, 0.0)
    u = np.where(rho != 0.0, u, 0.0)
    r = drag_rate(rho, u, par, law, rho_grain, gamma, gamma_m1)
    a = sink_accel(x, sinks, G)
    v2 = half_kick(v, a, vg, r, 0.5 * delta) if move else v
    late = (fate == 0) & ~(np.isfinite(v2).all(axis=1) & np.isfinite(a).all(axis=1))
    fate[late] = NONFINITE
    keep = (fate == 0) | late
    v = np.where(keep[:, None], v2, v)
    return {"x": x, "v": v, "S": {"a": a, "vg": vg, "r": r}, "fate": fate, "sink": by, "rho": rho, "u": u}
