"""GPU tests of sph_gravity_at (include/summersph.h, "gravitational potential and acceleration at arbitrary points") on
the MI355X: the exact field (theta -> 0 opens every node: the walk is the direct sum) against the numpy restatement with
fixed and variable h, agreement with sph_energy's potential and with the force path's acceleration, the Barnes-Hut error
at theta = 0.5, the order rule, small and odd source sets, bad points, the parts, no side effects on a running simulation,
the command line and one 10^6 x 10^6 run.

Bounds: TOL = 1e-12 of a row's sum of absolute terms (the project's bound for such sums); FORCE_TOL and BH_TOL_* are three
times what was measured on the MI355X."""
import ctypes as C
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, load_golden
import energy_ref
from gpu_support import capi, make_context, over_defaults, var_params, with_variable_h
import gravity_at_ref as ref
import octree_ref
from summersph_amd import ic, txtio
from summersph_amd import gravity as gv
from summersph_amd import sample as smp

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
TINY_THETA = 1e-9
# |a_gravity_at - a_forces| / sum |in-support terms|: the force interpolates its table of the mass fraction M(q) linearly
# (an error of about q dq^2 on M ~ (4/3) q^3, so the closest pairs of a set decide), this call is analytic.  Measured on
# the MI355X: 6.64e-7 (Plummer sphere, 3000) and 2.81e-7 (disc3000); a numpy sum with the interpolated table in place of
# the polynomial gives 6.64e-7 and 2.82e-7.  The bound is three times the larger; beyond 1e-6 it is a bug.
FORCE_TOL = 2.0e-6
FORCE_BUG = 1.0e-6
# theta = 0.5 on the 20 000-particle heavy disc, a 64 x 64 polar map: max |g - g_direct| / rms |g_direct| and the same for
# Phi.  Measured on the MI355X: 3.73e-2 and 4.44e-3; the bounds are three times that.
BH_TOL_ACC = 0.112
BH_TOL_PHI = 1.33e-2


def _ctx(capi, gas, sinks=None, variable=False, flags=0, **kw):
    flags = over_defaults(capi, with_variable_h(capi, flags, variable), variable)
    return make_context(capi, gas, sinks, variable=variable, flags=flags, **kw)


def _rows(phi, acc):
    """(phi (M,), acc (3, M)) -> (4, M); the split form -> (2, 4, M)"""
    return np.concatenate([phi[..., None, :], acc], axis=-2)


def _close(got, want, scale, tol, what=""):
    """every entry within tol of its own sum of absolute terms; non-finite entries must match exactly"""
    got, want, scale = np.asarray(got), np.asarray(want), np.asarray(scale)
    assert got.shape == want.shape == scale.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    err = np.abs(got[fin] - want[fin])
    ratio = float(np.max(err / np.maximum(scale[fin], 1e-300), initial=0.0))
    print(f"    {what}: max |diff| / sum |terms| = {ratio:.3e} (tol {tol:g})")
    assert np.all(err <= tol * scale[fin]), (what, ratio)


def _fixture(capi, case, **kw):
    variable = case.startswith("sinkcv")
    g = load_golden("sinkcv1500_traj" if variable else "disc3000_traj")
    gas, sinks = energy_ref.rows_to_dicts(g, "full_s3_" if variable else "full_s5_", variable)
    ctx = _ctx(capi, gas, sinks, variable, **kw, **(var_params(g) if variable else {}))
    return ctx, gas, sinks, variable


def _probe_points(gas, sinks, seed):
    """1000 points: a 20 x 40 polar lattice through the disc, a 10 x 10 (R, z) cut, 50 points exactly on particles and 50
    far outside the source box.  The far ones lie 4000 .. 10^4 from the centre of mass in random directions: with every
    mass within a of it, |Phi + G M / r| / (G M / r) <= sum_j (m_j / M) (a_j / r)^2 / (1 - a / r) (the Legendre series
    without its dipole), which is 4.9e-7 for disc3000 (sum m a^2 / M = 7.7, a = 38) and 1.2e-7 for sinkcv1500 (1.8, 88)."""
    rng = np.random.default_rng(seed)
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    R = np.hypot(pos[:, 0], pos[:, 1])
    r0, r1 = np.percentile(R, [1, 99])
    polar, _ = smp.polar_points(r0, r1, 20, 40)
    rz, _ = smp.rz_points(r0, r1, 10, -8.0, 8.0, 10, phi=0.7)
    on = rng.choice(pos.shape[0], 50, replace=False)
    m_all = np.concatenate([gas["m"], sinks["m"]])
    p_all = np.concatenate([pos, np.stack([sinks["x"], sinks["y"], sinks["z"]], axis=1)])
    com = (m_all[:, None] * p_all).sum(axis=0) / m_all.sum()
    u = rng.normal(size=(50, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    far = com + np.exp(rng.uniform(np.log(4000.0), np.log(1.0e4), 50))[:, None] * u
    return np.concatenate([polar, rz, pos[on], far]), on, com, float(m_all.sum())


# ---- 1. the exact field ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["disc3000_full_s5", "sinkcv1500_full_s3"])
def test_exact_field_is_the_direct_sum(capi, case):
    ctx, gas, sinks, variable = _fixture(capi, case, theta=TINY_THETA)
    pts, on, com, m_tot = _probe_points(gas, sinks, 5)
    G = ctx.params.G
    if variable:                    # the points' own lengths: over the particles' range, the particles' own where they sit
        ph = np.random.default_rng(6).uniform(gas["h"].min(), gas["h"].max(), pts.shape[0])
        ph[900:950] = gas["h"][on]
    else:
        ph = None
    h = ph if variable else ctx.params.h
    for soft2 in (ref.SOFT2, 0.0):
        phi, acc = ctx.gravity_at(pts, ph=ph, soft2=soft2, split=True)
        got = _rows(phi, acc)
        want_g, scale_g = ref.gas_field(pts, h, ref.src_of(gas), G, soft2)
        want_s, scale_s = ref.sink_field(pts, sinks, G)
        _close(got[0], want_g, scale_g, TOL, f"{case} soft2 {soft2} gas")
        _close(got[1], want_s, scale_s, TOL, f"{case} soft2 {soft2} sinks")
        assert np.all(np.isfinite(got))
        # far away the whole system is a point mass at its centre of mass
        r = np.linalg.norm(pts[950:] - com, axis=1)
        tot = got[0, 0, 950:] + got[1, 0, 950:]
        mono = -G * m_tot / r
        print(f"    far points: max |Phi r / (G M) + 1| = {np.max(np.abs(tot / mono - 1.0)):.3e}")
        assert np.max(np.abs(tot / mono - 1.0)) <= 1e-6
    ctx.close()


# ---- 2. agreement with sph_energy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["disc3000_full_s5", "sinkcv1500_full_s3"])
def test_agrees_with_sph_energy_at_the_particles(capi, case):
    ctx, gas, sinks, variable = _fixture(capi, case, flags=capi.FLAG_SELF_GRAVITY)
    p = ctx.params
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    hi = gas["h"] if variable else np.full(pos.shape[0], p.h)
    phi, _ = ctx.gravity_at(pos, ph=hi, soft2=ref.SOFT2, split=True)
    own = (p.G * gas["m"] / hi) * energy_ref.phi_kernel(np.sqrt(ref.SOFT2) / hi)     # the point's own source: added, removed
    want = ctx.energy(phi=True)["phi"]
    got = (phi[0] - own) + phi[1]
    rel = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"    {case}: max relative difference to sph_energy's phi = {rel:.3e}")
    assert rel <= TOL
    ctx.close()


# ---- 3. agreement with the force path --------------------------------------------------------------------------------------
def _force_sets():
    pl = octree_ref.plummer(n=3000)
    g = load_golden("disc3000_traj")
    d, _ = energy_ref.rows_to_dicts(g, "full_s5_")
    return {"plummer3000": pl, "disc3000": octree_ref._gas(d["x"], d["y"], d["z"], d["m"])}


@pytest.mark.parametrize("name", ["plummer3000", "disc3000"])
def test_agrees_with_the_force_path(capi, name):
    """u = v = alpha = 0 and no sinks: sph_forces leaves the Barnes-Hut term alone in ax..az.  The two differ by the
    force's linearly interpolated table inside the softening support (bounded against the in-support terms) and by
    rounding everywhere (bounded, as everywhere, by TOL of all terms)."""
    gas = _force_sets()[name]
    ctx = _ctx(capi, gas, None, flags=capi.FLAG_SELF_GRAVITY)
    ctx.density(); ctx.forces()
    a_force = np.stack([ctx.field(k) for k in ("ax", "ay", "az")])
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    _, acc = ctx.gravity_at(pos, soft2=ref.SOFT2, sinks=False)
    _, scale, sup = ref.gas_field(pos, ctx.params.h, ref.src_of(gas), ctx.params.G, ref.SOFT2, support=True)
    diff = np.abs(acc - a_force)
    inside = sup[1:] > 0.0
    ratio = float(np.max((diff[inside] - TOL * scale[1:][inside]) / sup[1:][inside]))
    print(f"    {name}: max |a - a_forces| / sum |in-support terms| = {ratio:.3e} (bound {FORCE_TOL:g}); "
          f"max over all terms {float(np.max(diff / scale[1:])):.3e}")
    assert ratio <= FORCE_BUG, "beyond what the table's error explains: a bug, not a tolerance"
    assert np.all(diff <= FORCE_TOL * sup[1:] + TOL * scale[1:]), ratio
    ctx.close()


# ---- 4. the Barnes-Hut error -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def heavy_disc():
    gas, _ = ic.split_rows(ic.keplerian_disc(20000, seed=5, m_disc=0.5))
    pts, shape = smp.polar_points(10.0, float(np.hypot(gas["x"], gas["y"]).max()), 64, 64)
    return gas, pts


def _bh_errors(got, want):
    g, gd = got[1:], want[1:]
    e_acc = np.max(np.linalg.norm(g - gd, axis=0)) / np.sqrt(np.mean(np.sum(gd * gd, axis=0)))
    e_phi = np.max(np.abs(got[0] - want[0])) / np.sqrt(np.mean(want[0] ** 2))
    return float(e_acc), float(e_phi)


def test_barnes_hut_error_at_theta_half(capi, heavy_disc):
    gas, pts = heavy_disc
    ctx = _ctx(capi, gas, None)
    got = _rows(*ctx.gravity_at(pts, sinks=False))
    want, _ = ref.gas_field(pts, ctx.params.h, ref.src_of(gas), ctx.params.G)
    e_acc, e_phi = _bh_errors(got, want)
    print(f"    theta 0.5, 20000 sources, 64 x 64 map: max |g - g_direct| / rms |g_direct| = {e_acc:.3e}, Phi: {e_phi:.3e}")
    assert e_acc <= BH_TOL_ACC and e_phi <= BH_TOL_PHI
    ctx.close()


# ---- 5. the order rule -----------------------------------------------------------------------------------------------------
def test_order_rule_is_bitwise(capi):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc(6000, seed=17, m_disc=0.1))
    rng = np.random.default_rng(8)
    r1 = float(np.hypot(gas["x"], gas["y"]).max())
    pts = np.concatenate([smp.polar_points(5.0, 1.2 * r1, 30, 30)[0], rng.uniform(-2.0 * r1, 2.0 * r1, (100, 3))])
    assert pts.shape[0] == 1000
    ph = rng.uniform(0.5, 4.0, 1000)
    ctx = _ctx(capi, gas, sinks)
    full = _rows(*ctx.gravity_at(pts, ph=ph, split=True))
    assert np.array_equal(_rows(*ctx.gravity_at(pts, ph=ph, split=True)), full)                       # again
    perm = rng.permutation(1000)
    assert np.array_equal(_rows(*ctx.gravity_at(pts[perm], ph=ph[perm], split=True)), full[..., perm])
    for k in (1, 63, 64, 65):
        assert np.array_equal(_rows(*ctx.gravity_at(pts[:k], ph=ph[:k], split=True)), full[..., :k]), k
    one = _rows(*ctx.gravity_at(pts[777:778], ph=ph[777:778], split=True))
    assert np.array_equal(one, full[..., 777:778])
    dp = torch.tensor(pts, dtype=torch.float64, device="cuda:0")
    dh = torch.tensor(ph, dtype=torch.float64, device="cuda:0")
    dphi, dacc = ctx.gravity_at(dp, ph=dh, split=True, device=True)
    assert np.array_equal(_rows(dphi.cpu().numpy(), dacc.cpu().numpy()), full)
    ctx.density()                                                                                     # re-sorted slots
    assert np.array_equal(_rows(*ctx.gravity_at(pts, ph=ph, split=True)), full)
    ctx.close()
    hashed = _ctx(capi, gas, sinks, flags=capi.FLAG_HASHED_GRID)
    hashed.density()
    assert np.array_equal(_rows(*hashed.gravity_at(pts, ph=ph, split=True)), full)
    hashed.close()
    # a second context, holding other particles, fed the first one's records and box
    rec = np.stack([gas["x"], gas["y"], gas["z"], gas["m"]], axis=1)
    box = np.concatenate([rec[:, :3].min(axis=0), rec[:, :3].max(axis=0)])
    d_rec = torch.tensor(rec, dtype=torch.float64, device="cuda:0").contiguous()
    torch.cuda.synchronize()
    other = _ctx(capi, {k: v[:100] for k, v in gas.items()}, sinks, flags=capi.FLAG_SELF_GRAVITY)
    other.set_gravity_sources_dev(rec.shape[0], d_rec.data_ptr(), box)
    assert np.array_equal(_rows(*other.gravity_at(pts, ph=ph, split=True)), full)
    other.density(); other.forces()                                    # the tree sph_forces built, in place
    assert np.array_equal(_rows(*other.gravity_at(pts, ph=ph, split=True)), full)
    other.close()


# ---- 6. small and odd shapes -----------------------------------------------------------------------------------------------
def _small_sets():
    one = octree_ref._gas(np.array([3.0]), np.array([-2.0]), np.array([0.5]), np.array([1e-3]))
    two = octree_ref._gas(np.array([3.0, -1.0]), np.array([-2.0, 4.0]), np.array([0.5, 0.25]), np.array([1e-3, 3e-3]))
    return {"one": one, "two": two, "coincident": octree_ref.coincident(100), "two_clusters": octree_ref.two_clusters()}


@pytest.mark.parametrize("m_pts", [1, 65])
@pytest.mark.parametrize("name", ["one", "two", "coincident", "two_clusters"])
def test_small_source_sets(capi, name, m_pts):
    gas = _small_sets()[name]
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    rng = np.random.default_rng(21)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    t = rng.uniform(0.0, 1.0, (m_pts, 1))
    pts = lo + t * (hi - lo) + rng.normal(0.0, 3.0, (m_pts, 3))       # along the diagonal: between the two clusters
    pts[0] = pos[0]                                                    # on a source
    ctx = _ctx(capi, gas, None, theta=TINY_THETA)
    for soft2 in (ref.SOFT2, 0.0):
        got = _rows(*ctx.gravity_at(pts, soft2=soft2, sinks=False))
        want, scale = ref.gas_field(pts, ctx.params.h, ref.src_of(gas), ctx.params.G, soft2)
        _close(got, want, scale, TOL, f"{name} x {m_pts} soft2 {soft2}")
    ctx.close()


@pytest.mark.parametrize("m_pts", [1, 65])
def test_empty_context_and_sinks(capi, m_pts):
    rng = np.random.default_rng(22)
    pts = rng.uniform(-50.0, 50.0, (m_pts, 3))
    empty = capi.Context(device=0)
    phi, acc = empty.gravity_at(pts)
    assert np.all(phi == 0.0) and np.all(acc == 0.0)
    sinks = {"x": np.array([1.0, -20.0, 7.0]), "y": np.array([2.0, 5.0, 7.0]), "z": np.array([0.5, 0.0, 7.0]),
             "vx": np.zeros(3), "vy": np.zeros(3), "vz": np.zeros(3), "m": np.array([1.0, 0.0, 0.25])}
    empty.set_sinks(sinks)
    G = empty.params.G
    pts[0] = (1.0, 2.0, 0.5)                                           # on the massive sink 0
    if m_pts > 1:
        pts[1] = (-20.0, 5.0, 0.0)                                     # on the massless sink 1: it adds 0, not NaN
    got = _rows(*empty.gravity_at(pts, split=True))
    want, scale = ref.sink_field(pts, sinks, G)
    assert np.all(got[0] == 0.0)
    _close(got[1], want, scale, TOL, f"sinks only x {m_pts}")
    assert got[1, 0, 0] == -np.inf and np.all(np.isnan(got[1, 1:, 0]))
    assert np.all(np.isfinite(got[1, :, 1:]))
    only = _rows(*empty.gravity_at(pts, gas=False))
    assert np.array_equal(only, got[1], equal_nan=True)
    two = {k: v[1:] for k, v in sinks.items()}                         # without the massive sink 0: the massless one first
    empty.set_sinks(two)
    want2, scale2 = ref.sink_field(pts, {k: v[2:] for k, v in sinks.items()}, G)
    _close(_rows(*empty.gravity_at(pts, gas=False)), want2, scale2, TOL, "massless sink adds 0")
    empty.close()


# ---- 7. bad inputs ---------------------------------------------------------------------------------------------------------
def test_bad_points_and_errors(capi):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc(3000, seed=3, m_disc=0.1))
    ctx = _ctx(capi, gas, sinks)
    rng = np.random.default_rng(23)
    m = 200
    pts = rng.uniform(-40.0, 40.0, (m, 3))
    ph = rng.uniform(1.0, 3.0, m)
    good = _rows(*ctx.gravity_at(pts, ph=ph))
    bad_p, bad_h = pts.copy(), ph.copy()
    nonfin = {5: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 199: (0, np.nan)}
    for i, (a, v) in nonfin.items():
        bad_p[i, a] = v
    badh = {7: 0.0, 63: -1.0, 128: np.nan, 150: np.inf, 199: -2.0}     # 199 is bad both ways
    for i, v in badh.items():
        bad_h[i] = v
    dead = sorted(set(nonfin) | set(badh))
    alive = np.setdiff1d(np.arange(m), dead)
    dp = torch.tensor(bad_p, dtype=torch.float64, device="cuda:0")
    dh = torch.tensor(bad_h, dtype=torch.float64, device="cuda:0")
    for split in (False, True):
        phi, acc, cnt = ctx.gravity_at(dp, ph=dh, split=split, counts=True, device=True)
        got = _rows(phi.cpu().numpy(), acc.cpu().numpy())
        assert cnt == (len(nonfin), len(badh))
        assert np.all(np.isnan(got[..., dead]))
        if split:
            assert np.array_equal(got[0][:, alive] + got[1][:, alive], good[:, alive])
        else:
            assert np.array_equal(got[:, alive], good[:, alive])
    with pytest.raises(capi.SphError) as e:
        ctx.gravity_at(pts, ph=bad_h)
    assert e.value.status == SPH_ERR_STATE
    phi, acc, cnt = ctx.gravity_at(bad_p, ph=ph, counts=True)           # non-finite points alone are no error
    assert cnt == (len(nonfin), 0) and np.all(np.isnan(phi[list(nonfin)]))

    # SPH_ERR_ARG: nothing is written
    lib = ctx.lib
    x, y, z = (np.ascontiguousarray(pts[:, a]) for a in range(3))
    out = np.full(8 * m, -7.0)
    cc = (C.c_int64 * 2)(-3, -3)

    def call(d, n=m, px=x, py=y, pz=z, h=ph, o=out, n_out=4 * m, dev=False):
        f = lib.sph_gravity_at_dev if dev else lib.sph_gravity_at
        ptr = lambda a: None if a is None else a.ctypes.data
        return f(ctx._h, None if d is None else C.byref(d), n, ptr(px), ptr(py), ptr(pz), ptr(h), ptr(o), n_out, cc)

    D = capi.gravity_at_desc
    assert call(D()) == 0
    assert not np.any(out[:4 * m] == -7.0) and np.all(out[4 * m:] == -7.0)
    out[:] = -7.0
    cc[0] = cc[1] = -3

    def desc(**kw):
        d = D()
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    cases = {
        "null descriptor": dict(d=None),
        "null px": dict(d=D(), px=None), "null py": dict(d=D(), py=None), "null pz": dict(d=D(), pz=None),
        "n_points < 0": dict(d=D(), n=-1, n_out=-4), "n_points > 2^31 - 1": dict(d=D(), n=2**31, n_out=4 * 2**31),
        "n_out": dict(d=D(), n_out=4 * m - 1), "n_out for split": dict(d=D(split=True), n_out=4 * m),
        "n_out without split": dict(d=D(), n_out=8 * m), "null out": dict(d=D(), o=None),
        "no part": dict(d=D(gas=False, sinks=False)), "split without gas": dict(d=desc(flags=capi.GRAVAT_SPLIT | capi.GRAVAT_SINKS), n_out=8 * m),
        "split without sinks": dict(d=desc(flags=capi.GRAVAT_SPLIT | capi.GRAVAT_GAS), n_out=8 * m),
        "unknown flags": dict(d=desc(flags=8 | 3)), "reserved 0": dict(d=desc(reserved=0)), "reserved 2": dict(d=desc(reserved=2)),
        "h < 0": dict(d=desc(h=-1.0)), "h NaN": dict(d=desc(h=np.nan)), "soft2 < 0": dict(d=desc(soft2=-1e-3)),
        "soft2 NaN": dict(d=desc(soft2=np.nan)),
    }
    for what, kw in cases.items():
        for dev in (False, True):
            assert call(dev=dev, **kw) == SPH_ERR_ARG, (what, dev)
    assert np.all(out == -7.0) and (cc[0], cc[1]) == (-3, -3)
    assert call(D(), n=0, n_out=0, px=None, py=None, pz=None, h=None, o=None) == 0 and (cc[0], cc[1]) == (0, 0)
    ctx.close()
    vctx, _, _, _ = _fixture(capi, "sinkcv1500_full_s3")
    vctx_call = lambda d, h: lib.sph_gravity_at(vctx._h, C.byref(d), m, x.ctypes.data, y.ctypes.data, z.ctypes.data,
                                                None if h is None else h.ctypes.data, out.ctypes.data, 4 * m, cc)
    assert vctx_call(D(), None) == SPH_ERR_ARG and np.all(out == -7.0)      # h == 0 without ph on a variable-h context
    assert vctx_call(D(h=2.0), None) == 0 and vctx_call(D(), ph) == 0
    vctx.close()


# ---- 8. the parts add up ---------------------------------------------------------------------------------------------------
def test_parts_add_up(capi):
    ctx, gas, sinks, _ = _fixture(capi, "disc3000_full_s5", theta=TINY_THETA)
    pts, _, _, _ = _probe_points(gas, sinks, 9)
    split = _rows(*ctx.gravity_at(pts, split=True))
    assert np.array_equal(_rows(*ctx.gravity_at(pts)), split[0] + split[1])
    assert np.array_equal(_rows(*ctx.gravity_at(pts, sinks=False)), split[0])
    assert np.array_equal(_rows(*ctx.gravity_at(pts, gas=False)), split[1])
    G, h = ctx.params.G, ctx.params.h
    ctx.close()
    n = gas["x"].size
    tot = np.zeros((4, pts.shape[0]))
    for sl in (slice(0, n // 2), slice(n // 2, n)):
        half = _ctx(capi, {k: v[sl] for k, v in gas.items()}, None, theta=TINY_THETA)
        tot += _rows(*half.gravity_at(pts, sinks=False))
        half.close()
    _, scale = ref.gas_field(pts, h, ref.src_of(gas), G)
    _close(tot, split[0], scale, TOL, "two halves")


# ---- 9. no side effects ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_gravity", [False, True])
def test_no_side_effects_on_a_run(capi, self_gravity):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29, m_disc=0.2))
    pts, _ = smp.polar_points(12.0, 60.0, 20, 32)
    runs = []
    for with_call in (False, True):
        ctx = _ctx(capi, gas, sinks, flags=capi.FLAG_SELF_GRAVITY if self_gravity else 0)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_call:
                before = {k: ctx.field(k) for k in ("x", "vx", "rho", "ax", "du")}
                ctx.gravity_at(pts, split=True)
                ctx.gravity_at(pts[:65], h=1.0, soft2=0.0, sinks=False)
                for k, v in before.items():
                    assert np.array_equal(ctx.field(k), v), k
            st = ctx.stats()
            statsl.append({f: (list(getattr(st, f)) if f == "grid_dim" else getattr(st, f)) for f, _ in st._fields_
                           if f != "device_bytes"})
        runs.append(({k: ctx.field(k) for k in ("x", "y", "z", "vx", "vy", "vz", "u", "alpha", "rho", "ax", "du")}, dt, t,
                     statsl, ctx.get_sinks()))
        ctx.close()
    (f0, dt0, t0, s0, k0), (f1, dt1, t1, s1, k1) = runs
    assert dt0 == dt1 and t0 == t1 and s0 == s1
    for k in f0:
        assert np.array_equal(f0[k], f1[k]), k
    for k in k0:
        assert np.array_equal(k0[k], k1[k]), k


def test_after_accrete_and_cull(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=12, m_disc=0.2))
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])
    ctx = _ctx(capi, gas, sinks, theta=TINY_THETA)
    ctx.density(); ctx.forces()
    assert ctx.accrete_and_cull() > 0 and ctx.n < 8000
    left = {k: ctx.field(k) for k in "xyzm"}
    pts, _ = smp.polar_points(5.0, 60.0, 10, 13)
    got = _rows(*ctx.gravity_at(pts, split=True))
    want, scale = ref.gas_field(pts, ctx.params.h, ref.src_of(left), ctx.params.G)
    _close(got[0], want, scale, TOL, "after the cull, gas")
    s = ctx.get_sinks()
    want_s, scale_s = ref.sink_field(pts, s, ctx.params.G)
    _close(got[1], want_s, scale_s, TOL, "after the cull, sinks")
    ctx.close()


# ---- 10. the command line --------------------------------------------------------------------------------------------------
def _save(tmp_path, gas, sinks, name="save.txt"):
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m".split()] + [np.zeros(gas["x"].size)], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / name
    txtio.write_save(str(save), rows, srows)
    g2 = {k: rows[:, i] for i, k in enumerate("x y z vx vy vz u m alpha".split())}
    s2 = {k: srows[:, i] for i, k in zip((0, 1, 2, 3, 4, 5, 7), "x y z vx vy vz m".split())}
    return save, g2, s2


def test_cli_matches_the_context(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(4000, seed=31, m_disc=0.05))
    save, g2, s2 = _save(tmp_path, gas, sinks)
    out = tmp_path / "g.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.gravity", str(save), "-o", str(out), "--polar", "10", "40", "12", "16",
                        "--split", "--h", "2.0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    pts, shape = smp.polar_points(10.0, 40.0, 12, 16)
    ctx = _ctx(capi, g2, s2)
    phi, acc = ctx.gravity_at(pts, h=2.0, split=True)
    assert np.array_equal(z["points"], pts) and tuple(z["shape"]) == shape
    assert np.array_equal(z["phi"], phi) and np.array_equal(z["acc"], acc)
    assert z["desc_h"] == 2.0 and z["desc_flags"] == 7 and z["n_nonfinite"] == 0 and z["n_bad_h"] == 0
    ctx.close()


def test_cli_rotation_curve_of_a_massless_disc(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(4000, seed=32))
    gas = dict(gas); gas["m"] = np.zeros_like(gas["m"])
    save, _, s2 = _save(tmp_path, gas, sinks)
    out = tmp_path / "rc.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.gravity", str(save), "-o", str(out), "--rotation-curve", "10", "40",
                        "15", "32"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    G = capi.default_params().G
    want = G * s2["m"][0] / z["R"]
    assert z["R"].shape == (15,) and np.all(z["vc2_gas"] == 0.0)
    for k in ("vc2", "vc2_sinks"):
        assert np.max(np.abs(z[k] / want - 1.0)) <= TOL, k


# ---- 11. one larger run ----------------------------------------------------------------------------------------------------
def test_million_sources_million_points(capi):
    gas, _ = ic.split_rows(ic.keplerian_disc(1_000_000, seed=41, m_disc=0.5))
    r1 = float(np.hypot(gas["x"], gas["y"]).max())
    pts, _ = smp.polar_points(10.0, r1, 1000, 1000)
    ctx = _ctx(capi, gas, None)
    ctx.gravity_at(pts[:64], sinks=False)                              # the scratch and the tree arrays exist
    t0 = time.perf_counter()
    got = _rows(*ctx.gravity_at(pts, sinks=False))
    wall = time.perf_counter() - t0
    print(f"    10^6 sources x 10^6 points, theta 0.5, host form: {wall * 1e3:.1f} ms")
    pick = np.random.default_rng(42).choice(pts.shape[0], 200, replace=False)
    want, _ = ref.gas_field(pts[pick], ctx.params.h, ref.src_of(gas), ctx.params.G)
    # test 4's bounds with test 4's norm: the rms over the map is taken over the checked subset
    e_acc, e_phi = _bh_errors(got[:, pick], want)
    print(f"    200 points against the direct sum: acc {e_acc:.3e}, Phi {e_phi:.3e}")
    assert e_acc <= BH_TOL_ACC and e_phi <= BH_TOL_PHI
    ctx.close()
