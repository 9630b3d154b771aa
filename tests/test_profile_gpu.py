"""GPU tests of sph_profile (include/summersph.h, "disc profiles") on the MI355X: parity of the sums and the table with the
numpy restatement (fixed and variable h, rings and sectors, z cut, 10^6 particles), the order rule (bitwise across sorted
orders, grids and calls), frames (rotated, translated and boosted discs, AUTO_NORMAL), the circumbinary fixture,
additivity over contexts, full coverage after a cull, no side effects on a running simulation, the device form, the
argument errors and the command line."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err
from gpu_support import capi, make_context
import profile_ref
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPH_ERR_ARG = 1


def _disc(n, seed, variable=False):
    rows = ic.keplerian_disc_var(n, seed=seed) if variable else ic.keplerian_disc(n, seed=seed)
    gas, sinks = ic.split_rows(rows)
    gas = dict(gas)
    rng = np.random.default_rng(seed + 1)
    gas["u"] = rng.uniform(0.1, 0.5, gas["x"].size)        # structure in every column
    gas["alpha"] = rng.uniform(0.0, 1.0, gas["x"].size)
    gas["vz"] = rng.normal(0.0, 0.05, gas["x"].size)
    gas["vx"] = gas["vx"] + rng.normal(0.0, 0.02, gas["x"].size)
    return gas, sinks


def _drop_edges(gas, cases, centre=(0, 0, 0), normal=(0, 0, 1)):
    keep = np.ones(gas["x"].size, bool)
    for (r0, r1, nr, nphi, log) in cases:
        keep &= ~profile_ref.edge_margin(gas, r0, r1, nr, nphi, log, centre, normal)
    return {k: (v[keep] if isinstance(v, np.ndarray) and v.shape == keep.shape else v) for k, v in gas.items()}


def _ref(capi, ctx, gas, sinks, r0, r1, nr, nphi=1, log=False, z_max=np.inf, sink=0, normal=(0, 0, 1), h=None):
    p = ctx.params
    c, cv, cm = ((sinks["x"][sink], sinks["y"][sink], sinks["z"][sink]), (sinks["vx"][sink], sinks["vy"][sink], sinks["vz"][sink]),
                 sinks["m"][sink]) if sink is not None else ((0, 0, 0), (0, 0, 0), 0.0)
    hh = p.h if h is None else h
    sums, b = profile_ref.profile_sums(gas, hh, p.G, r0, r1, nr, nphi, log, z_max, c, cv, cm, normal)
    n = np.asarray(normal, float)
    table = profile_ref.finish(sums, r0, r1, nr, nphi, log, n / np.linalg.norm(n), p.gamma, p.gamma_m1, p.G)
    return sums, table


# a dispersion sqrt(<q q> - <q>^2) is as exact as <q q>: compare its square on the scale of <q q> = sigma^2 + <q>^2
DISPERSIONS = {"H": "z_mean", "sigma_R": "vR_mean", "sigma_phi": "vphi_mean", "sigma_z": "vz_mean"}


def _cmp_table(capi, t, ref, tol=TOL):
    cols = {c: i for i, c in enumerate(capi.PROFILE_COLUMNS)}
    for c, i in cols.items():
        got, want = t[c], ref[:, i]
        assert np.array_equal(np.isnan(got), np.isnan(want)), c
        ok = ~np.isnan(want)
        if not ok.any():
            continue
        if c in DISPERSIONS:
            mean = ref[ok, cols[DISPERSIONS[c]]]
            err = np.max(np.abs(got[ok] ** 2 - want[ok] ** 2)) / max(np.max(want[ok] ** 2 + mean ** 2), 1e-300)
            assert err <= tol, (c, err)
        else:
            assert rel_err(got[ok], want[ok]) <= tol, (c, rel_err(got[ok], want[ok]))


def _cmp_sums(sums, ref, tol=TOL):
    assert np.array_equal(sums[:, 0], ref[:, 0])                     # counts exactly
    for s in range(1, sums.shape[1]):
        assert rel_err(sums[:, s], ref[:, s]) <= tol, (s, rel_err(sums[:, s], ref[:, s]))


CASES = [(10.0, 60.0, 12, 1, False, np.inf), (10.0, 60.0, 12, 1, True, np.inf), (10.0, 60.0, 10, 8, False, np.inf),
         (12.0, 55.0, 9, 8, True, 2.5)]


def test_parity_fixed_h(capi):
    gas, sinks = _disc(20000, 5)
    gas = _drop_edges(gas, [c[:5] for c in CASES])
    ctx = make_context(capi, gas, sinks)
    for (r0, r1, nr, nphi, log, zm) in CASES:
        t, s = ctx.profile(r0, r1, nr, nphi, log=log, sink=0, z_max=zm)
        rs, rt = _ref(capi, ctx, gas, sinks, r0, r1, nr, nphi, log, zm)
        assert s[:, 0].sum() > 1000
        _cmp_sums(s, rs)
        _cmp_table(capi, t, rt)
    ctx.close()


def test_parity_variable_h(capi):
    gas, sinks = _disc(6000, 9, variable=True)
    gas = _drop_edges(gas, [(10.0, 40.0, 8, 1, False)])
    ctx = make_context(capi, gas, sinks, variable=True)
    t, s = ctx.profile(10.0, 40.0, 8, sink=0)
    rs, rt = _ref(capi, ctx, gas, sinks, 10.0, 40.0, 8, h=gas["h"])
    _cmp_sums(s, rs)
    _cmp_table(capi, t, rt)
    assert np.all(t["h_mean"] != ctx.params.h)
    ctx.close()


def test_parity_1e6(capi):
    gas, sinks = _disc(1_000_000, 11)
    # the whole disc in 100 linear rings (~10^4 particles each: a sequential sum of many more equal masses drifts by more
    # than the tolerance by itself)
    r1 = 1.001 * float(np.max(np.hypot(gas["x"], gas["y"])))
    gas = _drop_edges(gas, [(10.0, r1, 100, 1, False)])
    ctx = make_context(capi, gas, sinks)
    t, s = ctx.profile(10.0, r1, 100, sink=0)
    rs, rt = _ref(capi, ctx, gas, sinks, 10.0, r1, 100, 1, False)
    _cmp_sums(s, rs)
    _cmp_table(capi, t, rt)
    assert s[:, 0].sum() == ctx.n > 990_000
    ctx.close()


def test_order_rule_bitwise(capi):
    gas, sinks = _disc(20000, 13)
    args = dict(r_min=5.0, r_max=70.0, n_r=16, n_phi=4, sink=0, z_max=3.0)
    a = make_context(capi, gas, sinks)
    s0 = a.profile(**args)[1]                                 # upload order
    a.density()                                               # cell-sorted
    s1 = a.profile(**args)[1]
    s2 = a.profile(**args)[1]
    b = make_context(capi, gas, sinks, flags=capi.FLAG_HASHED_GRID)
    b.density()
    s3 = b.profile(**args)[1]
    for s in (s1, s2, s3):
        assert np.array_equal(s, s0)
    assert a.grid_info().kind == 0 and b.grid_info().kind == 1
    a.close(); b.close()


def _rot_x(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _transform(gas, sinks, rot, shift=(0, 0, 0), boost=(0, 0, 0)):
    g, s = dict(gas), dict(sinks)
    for d, (p, v) in ((g, ("xyz", ("vx", "vy", "vz"))), (s, ("xyz", ("vx", "vy", "vz")))):
        P = rot @ np.stack([d[k] for k in p]); V = rot @ np.stack([d[k] for k in v])
        for a in range(3):
            d[p[a]] = P[a] + shift[a]
            d[v[a]] = V[a] + boost[a]
    return g, s


def test_frames(capi):
    gas, sinks = _disc(20000, 17)
    gas = _drop_edges(gas, [(10.0, 60.0, 10, 1, False)])
    base = make_context(capi, gas, sinks)
    t0, _ = base.profile(10.0, 60.0, 10, sink=0)
    rot = _rot_x(30.0)
    nz = rot @ np.array([0.0, 0.0, 1.0])
    g, s = _transform(gas, sinks, rot)
    ctx = make_context(capi, g, s)
    t1, _ = ctx.profile(10.0, 60.0, 10, sink=0, normal=tuple(nz))
    assert np.array_equal(t1["N"], t0["N"])
    for c in ("Sigma", "R_mean", "H", "vphi_mean", "vR_mean", "sigma_z", "Omega", "kappa", "Q", "Mdot", "j", "ecc", "tilt"):
        assert rel_err(t1[c], t0[c]) <= 1e-12 or np.max(np.abs(t1[c] - t0[c])) <= 1e-12, c
    tz, _ = ctx.profile(0.0, 200.0, 5, sink=0, normal=(0, 0, 1))
    nonempty = tz["M"] > 0
    assert np.all(np.abs(np.degrees(tz["tilt"][nonempty]) - 30.0) < 2.0)
    base.profile(10.0, 60.0, 10, sink=0, normal="auto")
    n0 = np.array(base.profile_desc.normal[:])
    ctx.profile(10.0, 60.0, 10, sink=0, normal="auto")
    n1 = np.array(ctx.profile_desc.normal[:])
    assert np.allclose(n1, rot @ n0, atol=1e-6, rtol=0)      # the disc's own normal, rotated
    assert np.allclose(n1, nz, atol=1e-2, rtol=0)             # which is z^ up to the sampling noise of L
    # translated and boosted, centred on the sink
    g2, s2 = _transform(gas, sinks, np.eye(3), shift=(123.0, -45.0, 7.0), boost=(3.0, -2.0, 0.5))
    ctx2 = make_context(capi, g2, s2)
    t2, _ = ctx2.profile(10.0, 60.0, 10, sink=0)
    assert np.array_equal(t2["N"], t0["N"])
    for c in capi.PROFILE_COLUMNS:
        ok = ~np.isnan(t0[c])
        assert np.max(np.abs(t2[c][ok] - t0[c][ok])) <= 1e-10 * max(1.0, np.max(np.abs(t0[c][ok]))), c
    base.close(); ctx.close(); ctx2.close()


def test_circumbinary_fixture(capi):
    g = load_golden("bin2000_eval")
    gas = {k: g[k] for k in "x y z vx vy vz u m alpha".split()}
    sinks = {"x": g["sx"], "y": g["sy"], "z": g["sz"], "vx": g["svx"], "vy": g["svy"], "vz": g["svz"], "m": g["sm"]}
    mb = float(np.sum(g["sm"]))
    com = tuple(float(np.sum(g["sm"] * g[k]) / mb) for k in ("sx", "sy", "sz"))
    comv = tuple(float(np.sum(g["sm"] * g[k]) / mb) for k in ("svx", "svy", "svz"))
    R = np.hypot(gas["x"] - com[0], gas["y"] - com[1])
    r0, r1 = 0.5 * float(np.min(R)), 1.01 * float(np.max(R))
    gas = _drop_edges(gas, [(r0, r1, 12, 1, False)], centre=com)
    ctx = make_context(capi, gas, sinks)
    t, s = ctx.profile(r0, r1, 12, centre=(com, comv, mb))
    p = ctx.params
    rs, _ = profile_ref.profile_sums(gas, p.h, p.G, r0, r1, 12, 1, False, np.inf, com, comv, mb)
    rt = profile_ref.finish(rs, r0, r1, 12, 1, False, (0, 0, 1), p.gamma, p.gamma_m1, p.G)
    _cmp_sums(s, rs)
    _cmp_table(capi, t, rt)
    filled = t["M"] > 0
    assert filled.sum() >= 6 and np.all(np.isfinite(t["ecc"][filled]))
    ctx.close()


def test_additivity_over_contexts(capi):
    gas, sinks = _disc(20000, 19)
    args = dict(r_min=10.0, r_max=60.0, n_r=10, n_phi=3, sink=0)
    whole = make_context(capi, gas, sinks)
    tw, sw = whole.profile(**args)
    half = gas["x"].size // 2
    parts = [{k: (v[sl] if isinstance(v, np.ndarray) and v.shape == gas["x"].shape else v) for k, v in gas.items()}
             for sl in (slice(0, half), slice(half, None))]
    sp = []
    for p in parts:
        c = make_context(capi, p, sinks)
        sp.append(c.profile(**args)[1])
        c.close()
    tot = sp[0] + sp[1]
    assert np.array_equal(tot[:, 0], sw[:, 0])
    for s in range(1, tot.shape[1]):
        assert rel_err(tot[:, s], sw[:, s]) <= 1e-13, s
    tf = capi.profile_finish(whole.profile_desc, whole.params, tot)
    _cmp_table(capi, tf, np.stack([tw[c] for c in capi.PROFILE_COLUMNS], axis=1), tol=1e-11)
    whole.close()


def test_full_coverage_and_cull(capi):
    gas, sinks = _disc(20000, 23)
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])   # accretes the inner edge
    ctx = make_context(capi, gas, sinks)
    for step in range(2):
        _, s = ctx.profile(0.0, 1e4, 7, n_phi=2, sink=0)
        assert s[:, 0].sum() == ctx.n
        assert rel_err(s[:, 1].sum(), ctx.field("m").sum()) <= 1e-13
        if step == 0:
            ctx.density(); ctx.forces()
            assert ctx.accrete_and_cull() > 0
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = _disc(8000, 29)
    runs = []
    for with_profile in (False, True):
        ctx = make_context(capi, gas, sinks)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            if with_profile:
                ctx.profile(5.0, 80.0, 9, n_phi=2, sink=0, normal="auto")
            dt, t = ctx.step(dt, t)
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


def test_device_form_is_bitwise_the_host_form(capi):
    import torch
    gas, sinks = _disc(20000, 31)
    ctx = make_context(capi, gas, sinks)
    _, s = ctx.profile(10.0, 60.0, 10, n_phi=4, log=True, sink=0, z_max=4.0)
    d = ctx.profile(10.0, 60.0, 10, n_phi=4, log=True, sink=0, z_max=4.0, device=True)
    assert isinstance(d, torch.Tensor) and np.array_equal(d.cpu().numpy(), s)
    ctx.close()


def test_errors(capi):
    gas, sinks = _disc(3000, 37)
    ctx = make_context(capi, gas, sinks)
    lib = ctx.lib
    good = dict(r_min=10.0, r_max=40.0, n_r=4, n_phi=2, sink=0)
    buf = np.zeros((8, capi.PROFILE_NSUM))

    def call(d, nb=8, sums=buf, table=None):
        return lib.sph_profile(ctx._h, C.byref(d), None if sums is None else sums.ctypes.data,
                               None if table is None else table.ctypes.data, nb)

    def desc(**kw):
        a = dict(good); a.update(kw)
        return capi.profile_desc(**a)

    assert call(desc()) == 0
    bad = [desc(n_r=0), desc(n_phi=0), desc(n_r=2048, n_phi=1024), desc(r_min=-1.0), desc(r_min=40.0),
           desc(r_min=0.0, log=True), desc(normal=(0, 0, 0)), desc(normal=(np.nan, 0, 1)), desc(sink=1), desc(sink=-2)]
    for d in bad:                                             # refused before the output is touched
        nb = d.n_r * d.n_phi if d.n_r > 0 and d.n_phi > 0 else 8
        assert call(d, nb=nb) == SPH_ERR_ARG
    d = desc(); d.reserved[1] = 1
    assert call(d) == SPH_ERR_ARG
    assert call(desc(), nb=7) == SPH_ERR_ARG
    assert call(desc(), sums=None) == SPH_ERR_ARG
    assert lib.sph_profile(ctx._h, None, buf.ctypes.data, None, 8) == SPH_ERR_ARG
    assert lib.sph_profile(None, C.byref(desc()), buf.ctypes.data, None, 8) == SPH_ERR_ARG
    assert lib.sph_profile_dev(ctx._h, C.byref(desc()), None, 8) == SPH_ERR_ARG
    t, s = ctx.profile(**good)                                # still usable
    assert s[:, 0].sum() > 0
    ctx.density()
    ctx.close()


def test_cli_matches_context_profile(capi, tmp_path):
    gas, sinks = _disc(5000, 41)
    n = gas["x"].size
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "p.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.profile", str(save), "-o", str(out), "--rmin", "10", "--rmax", "50",
                        "--bins", "8", "--nphi", "2", "--log", "--centre", "sink:0", "--normal", "auto", "--zmax", "5"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = make_context(capi, g2, s2)
    t, s = ctx.profile(10.0, 50.0, 8, n_phi=2, log=True, sink=0, normal="auto", z_max=5.0)
    for c in capi.PROFILE_COLUMNS:
        assert np.array_equal(z[c], t[c], equal_nan=True), c
    assert np.array_equal(z["sums"], s)
    assert np.array_equal(z["desc_normal"], np.array(ctx.profile_desc.normal[:]))
    assert z["edges"].size == 9 and n == 5000
    ctx.close()
