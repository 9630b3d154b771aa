"""GPU tests of sph_groups (include/summersph.h, "friends-of-friends groups") on the MI355X: parity of the labels and the
table with the numpy restatement (embedded clumps, a uniform box, LINK_H with variable h, the fixtures, 10^6 particles),
adversarial sets (a long helix chain, pairs at exactly b and one ulp either side, coincident particles, a link larger than
the box, clumps 10^7 apart, ghosts, a cull, clip / min_members / max_groups, an empty selection), the order rule, no
side effects on a running simulation, the device form, the argument errors and the command line."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gpu_support import capi, clumped_disc, make_context
import groups_ref
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-13
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
EXACT = ("N", "r_max", "rho_max", "x_dense", "y_dense", "z_dense", "id_dense", "id_min")
FIELDS = "x y z vx vy vz u m rho".split()


_ctx = functools.partial(make_context, density=True)      # every call here reads rho unless it says density=False


def _fields(ctx, h=False):
    f = {k: ctx.field(k) for k in FIELDS}
    if h:
        f["h"] = ctx.field("h")
    return f


def _scale(col):
    a = np.abs(col[np.isfinite(col)])
    return float(a.max()) if a.size else 1.0


def _cmp(capi, labels, table, ng, ref, tol=TOL):
    rl, rt, rn = ref
    assert ng == rn
    assert np.array_equal(labels, rl)
    assert len(table) == rn
    for k, c in enumerate(capi.GROUPS_COLUMNS):
        got, want = table[c], rt[:, k]
        if c in EXACT:
            assert np.array_equal(got, want, equal_nan=True), c
        else:
            assert np.max(np.abs(got - want), initial=0.0) <= tol * _scale(want), c


def _check(capi, ctx, link, n_owned=None, h=False, **kw):
    lab, tab, ng = ctx.groups(link, link_h=h, **kw)
    f = _fields(ctx, h=h and ctx.params.flags & capi.FLAG_VARIABLE_H)
    hh = None if not h else (f["h"] if "h" in f else float(ctx.params.h))
    ref = groups_ref.groups(f, ctx.n if n_owned is None else n_owned, link, link_h=h, h=hh, **kw)
    _cmp(capi, lab, tab, ng, ref)
    return lab, tab, ng


def _gas(pos, seed=0, m=1e-6):
    rng = np.random.default_rng(seed)
    n = len(pos)
    return {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": rng.normal(0, 0.1, n),
            "vy": rng.normal(0, 0.1, n), "vz": rng.normal(0, 0.1, n), "u": rng.uniform(0.1, 0.5, n),
            "m": rng.uniform(0.5, 1.5, n) * m, "alpha": np.ones(n)}


# ---- parity ------------------------------------------------------------------------------------------------------------
def test_parity_embedded_clumps(capi):
    gas, sinks, n0, sizes = clumped_disc(20000, 4, 400, 3)
    ctx = _ctx(capi, gas, sinks)
    rho = ctx.field("rho")
    rho_min = 0.5 * float(np.min(rho[n0:]))
    assert np.max(rho[:n0]) < rho_min
    lab, tab, ng = _check(capi, ctx, 1.0, rho_min=rho_min)
    assert ng == 4 and np.all(lab[:n0] == -1) and np.all(lab[n0:] >= 0)
    assert sorted(tab["N"].tolist()) == sorted(float(s) for s in sizes)
    off = n0
    for s in sizes:                                     # each clump is one group
        assert np.unique(lab[off:off + s]).size == 1
        off += s
    ctx.close()


def test_parity_uniform_box(capi):
    gas, _ = ic.split_rows(ic.uniform_box(100000, seed=5))
    ctx = _ctx(capi, gas)
    n = ctx.n
    lo, hi = ctx.bbox()
    sep = float(np.prod(hi - lo) / n) ** (1 / 3)
    _, tab, ng = _check(capi, ctx, 0.7 * sep)
    assert 100 < ng < n and tab["N"][0] > 10
    _check(capi, ctx, 0.7 * sep, min_members=5)
    ctx.close()


def test_parity_link_h_variable(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000, seed=7))
    ctx = _ctx(capi, gas, sinks, variable=True)
    _, _, ng = _check(capi, ctx, 0.45, h=True)
    assert ng > 10
    rho = ctx.field("rho")
    _check(capi, ctx, 0.6, h=True, rho_min=float(np.median(rho)))
    ctx.close()
    fixed = _ctx(capi, ic.split_rows(ic.keplerian_disc(20000, seed=8))[0])
    _check(capi, fixed, 0.7, h=True)                      # params.h for every particle
    fixed.close()


@pytest.mark.parametrize("name", ["disc3000_traj", "bin2000_eval"])
def test_parity_fixtures(capi, name):
    gas, sinks = ic.split_rows(load_golden(name)["ic"])
    ctx = _ctx(capi, gas, sinks)
    _check(capi, ctx, 1.5)
    _check(capi, ctx, 2.5, min_members=3, rho_min=float(np.median(ctx.field("rho"))))
    ctx.close()


def test_parity_1e6(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(1_000_000, seed=11))
    ctx = _ctx(capi, gas, sinks)
    _, tab, ng = _check(capi, ctx, 1.5)
    assert ng > 1000
    ctx.close()


# ---- adversarial -------------------------------------------------------------------------------------------------------
def _helix(n, step):
    R, pitch = 2000.0, 10.0                               # turns 10 apart; a chord of `step` at a fixed angle step
    dth = 2.0 * np.arcsin(step / (2.0 * np.hypot(R, pitch / (2 * np.pi))))
    th = np.arange(n) * dth
    return np.stack([R * np.cos(th), R * np.sin(th), pitch * th / (2 * np.pi)], axis=1)


@pytest.mark.parametrize("frac, expect", [(0.999, 1), (1.001, 100000)])
def test_helix_chain(capi, frac, expect):
    pos = _helix(100000, frac)
    d = np.diff(pos, axis=0)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.all(d2 < 1.0) if frac < 1 else np.all(d2 >= 1.0)
    ctx = _ctx(capi, _gas(pos, 1))
    lab, tab, ng = _check(capi, ctx, 1.0)
    assert ng == expect
    if expect == 1:
        assert tab["N"][0] == 100000 and tab["id_min"][0] == 0
    ctx.close()


def test_pairs_at_exactly_b(capi):
    b = 0.75
    rows = []
    cases = []
    for k in range(60):
        x0 = 10.0 * k + 0.5
        for j, dx in enumerate((np.nextafter(x0 + b, 0.0) - x0, b, np.nextafter(x0 + b, np.inf) - x0)):
            y0 = 10.0 * j
            rows += [(x0, y0, 0.0), (x0 + dx, y0, 0.0)]
            cases.append((x0 + dx) - x0)
    pos = np.array(rows)
    rng = np.random.default_rng(2)                        # and some in random directions at b (1 +- few ulp)
    for k in range(300):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        p0 = np.array([1000.0 + 10 * k, 500.0, 0.0])
        pos = np.vstack([pos, p0, p0 + v * b * (1 + rng.integers(-3, 4) * 2.2e-16)])
    ctx = _ctx(capi, _gas(pos, 2))
    lab, _, ng = _check(capi, ctx, b)
    x = ctx.field("x")
    for k in range(60):
        base = 6 * k
        dxs = [x[base + 2 * j + 1] - x[base + 2 * j] for j in range(3)]
        assert dxs[0] < b and dxs[1] == b and dxs[2] > b
        assert lab[base] == lab[base + 1] and lab[base + 2] != lab[base + 3] and lab[base + 4] != lab[base + 5]
    ctx.close()


def test_coincident_particles(capi):
    rng = np.random.default_rng(4)
    pos = np.vstack([np.tile([[3.0, 4.0, 5.0]], (200, 1)), rng.uniform(-50, 50, (300, 3))])
    ctx = _ctx(capi, _gas(pos, 4))
    lab, tab, ng = _check(capi, ctx, 0.01)
    assert tab["N"][0] == 200 and np.all(lab[:200] == 0) and tab["r_max"][0] == 0.0
    ctx.close()


def test_link_larger_than_the_box(capi):
    rng = np.random.default_rng(6)
    ctx = _ctx(capi, _gas(rng.uniform(0, 1, (8000, 3)), 6))
    lab, tab, ng = _check(capi, ctx, 10.0)                # one cell holds everything: every pair is tested
    assert ng == 1 and tab["N"][0] == 8000
    ctx.close()


def test_clumps_far_apart(capi):
    rng = np.random.default_rng(8)
    a = rng.normal(0, 0.3, (3000, 3))
    pos = np.vstack([a, a[:2000] + [1e7, 0, 0], a[:1000] + [0, -1e7, 3e6]])
    ctx = _ctx(capi, _gas(pos, 8))
    lab, tab, ng = _check(capi, ctx, 0.05, min_members=2)
    assert ng > 3 and tab["N"][0] > 100
    ctx.close()


def test_ghosts_are_excluded(capi):
    gas, _ = ic.split_rows(ic.uniform_box(30000, seed=9))
    ctx = _ctx(capi, gas, density=False)
    ctx.set_owned(25000)
    ctx.density()
    lab, _, ng = _check(capi, ctx, 1.2, n_owned=25000)
    assert np.all(lab[25000:] == -1) and ng > 0
    ctx.close()


def test_after_accrete_and_cull(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=12))
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])
    ctx = _ctx(capi, gas, sinks)
    ctx.forces()
    assert ctx.accrete_and_cull() > 0
    assert ctx.n < 20000
    _check(capi, ctx, 1.5)
    ctx.close()


def test_clip_min_members_max_groups_empty(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=13))
    ctx = _ctx(capi, gas, sinks)
    clip = ((-30.0, -30.0, -2.0), (30.0, 30.0, 2.0))
    lab, _, _ = _check(capi, ctx, 1.5, clip=clip)
    x, y, z = ctx.field("x"), ctx.field("y"), ctx.field("z")
    assert np.all(lab[(np.abs(x) >= 30) | (np.abs(y) >= 30) | (np.abs(z) >= 2)] == -1)
    _check(capi, ctx, 1.5, min_members=4)
    full_l, full_t, full_n = ctx.groups(1.5)
    lab, tab, ng = ctx.groups(1.5, max_groups=7)
    assert ng == full_n > 7 and len(tab) == 7 and np.array_equal(lab, full_l)
    assert np.array_equal(tab.view(np.float64), full_t[:7].view(np.float64))
    lab, tab, ng = ctx.groups(1.5, max_groups=0)
    assert tab is None and ng == full_n
    lab, tab, ng = ctx.groups(1.5, rho_min=np.inf)
    assert ng == 0 and len(tab) == 0 and np.all(lab == -1)
    lab, tab, ng = ctx.groups(1.5, clip=((1e9,) * 3, (2e9,) * 3))
    assert ng == 0 and np.all(lab == -1)
    ctx.close()


# ---- order rule --------------------------------------------------------------------------------------------------------
def _raw(ctx, link, **kw):
    lab, tab, ng = ctx.groups(link, **kw)
    return lab, tab.view(np.float64).reshape(-1, 21).copy(), ng


def test_order_rule_bitwise(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(40000, seed=15))
    a = _ctx(capi, gas, sinks)
    la, ta, na = _raw(a, 1.5)
    lb, tb, nb = _raw(a, 1.5)
    assert na == nb and np.array_equal(la, lb) and np.array_equal(ta, tb, equal_nan=True)
    for flags in (capi.FLAG_HASHED_GRID, capi.FLAG_NO_LDS_TILES):
        c = _ctx(capi, gas, sinks, flags=flags)
        if flags == capi.FLAG_HASHED_GRID:
            assert c.grid_info().kind == 1
        lc, tc, nc = _raw(c, 1.5)
        assert nc == na and np.array_equal(lc, la) and np.array_equal(tc, ta, equal_nan=True)
        c.close()
    a.forces()                                            # another evaluation in place: the same
    lc, tc, nc = _raw(a, 1.5)
    assert nc == na and np.array_equal(lc, la) and np.array_equal(tc, ta, equal_nan=True)
    # a permuted upload: the same partition through the permutation, the same table group for group
    perm = np.random.default_rng(16).permutation(gas["x"].size)
    pg = {k: v[perm] for k, v in gas.items()}
    p = _ctx(capi, pg, sinks)
    lp, tp, npg = _raw(p, 1.5)
    assert npg == na
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    # group g of a <-> the group of p holding the same particles
    mp = np.full(na, -1)
    sel = la >= 0
    mp[la[sel]] = lp[inv[np.nonzero(sel)[0]]]
    assert np.all(mp >= 0) and np.unique(mp).size == na
    for g in range(na):
        assert np.array_equal(np.sort(np.nonzero(la == g)[0]), np.sort(perm[np.nonzero(lp == mp[g])[0]]))
        r0, r1 = ta[g], tp[mp[g]]
        assert r0[0] == r1[0]
        # rho comes from density sums in another neighbour order: rho_max and the densest member to round-off
        for k in list(range(1, 16)):
            assert abs(r0[k] - r1[k]) <= TOL * max(abs(r0[k]), np.max(np.abs(ta[:, k]))), (g, k)
        if perm[int(r1[19])] != int(r0[19]):
            assert abs(r0[15] - r1[15]) <= TOL * abs(r0[15])
        assert int(r0[20]) == np.min(np.nonzero(la == g)[0])
        assert int(r1[20]) == np.min(np.nonzero(lp == mp[g])[0])
    a.close(); p.close()


# ---- side effects, device form, errors, command line --------------------------------------------------------------------
def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    runs = []
    for with_groups in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_groups:
                ctx.groups(1.5, min_members=2)
                ctx.groups(0.5, link_h=True, max_groups=3)
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
    gas, sinks = ic.split_rows(ic.keplerian_disc(30000, seed=31))
    ctx = _ctx(capi, gas, sinks)
    for kw in ({}, {"min_members": 3, "rho_min": float(np.median(ctx.field("rho")))}, {"link_h": True}):
        lab, tab, ng = _raw(ctx, 0.6 if kw.get("link_h") else 1.5, **kw)
        dl, dtab, dn = ctx.groups(0.6 if kw.get("link_h") else 1.5, max_groups=50, device=True, **kw)
        assert isinstance(dl, torch.Tensor) and dn == ng
        assert np.array_equal(dl.cpu().numpy(), lab)
        k = min(ng, 50)
        assert np.array_equal(dtab.cpu().numpy()[:k], tab[:k], equal_nan=True)
    ctx.close()


def test_errors(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(3000, seed=37))
    ctx = _ctx(capi, gas, sinks, density=False)
    lib = ctx.lib
    n = ctx.n
    lab = np.empty(n, dtype=np.int32)
    tab = np.empty((10, capi.GROUPS_NCOL))
    cnt = C.c_int64(0)

    def call(d, labels=lab, nl=n, table=tab, mg=10, count=True):
        return lib.sph_groups(ctx._h, None if d is None else C.byref(d), None if labels is None else labels.ctypes.data, nl,
                              None if table is None else table.ctypes.data, mg, C.byref(cnt) if count else None)

    assert call(capi.groups_desc(1.0)) == SPH_ERR_STATE                  # rho stale
    ctx.density()
    assert call(capi.groups_desc(1.0)) == 0
    assert call(None) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0), count=False) == SPH_ERR_ARG
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(capi.groups_desc(bad)) == SPH_ERR_ARG, bad
    assert call(capi.groups_desc(1.0, rho_min=np.nan)) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0, clip=((np.nan, 0, 0), (1, 1, 1)))) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0, clip=((0, 0, 0), (1, np.nan, 1)))) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0, min_members=0)) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0), nl=n - 1) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0), mg=-1) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0), mg=0) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0), table=None, mg=-1) == SPH_ERR_ARG
    d = capi.groups_desc(1.0); d.flags = 2
    assert call(d) == SPH_ERR_ARG
    d = capi.groups_desc(1.0); d.reserved = 1
    assert call(d) == SPH_ERR_ARG
    assert lib.sph_groups(None, C.byref(capi.groups_desc(1.0)), None, 0, None, 0, C.byref(cnt)) == SPH_ERR_ARG
    assert call(capi.groups_desc(1.0), labels=None, nl=0, table=None, mg=0) == 0 and cnt.value > 0
    # LINK_H with a bad h on a selected particle (variable h), and with params.h <= 0
    gv, sv = ic.split_rows(ic.keplerian_disc_var(3000, seed=38))
    v = _ctx(capi, gv, sv, variable=True)
    h = v.field("h")
    h[17] = -1.0
    v.upload_field("h", h)
    v.density()
    hv = v.field("h")
    if hv[17] <= 0:                                     # the density pass keeps an uploaded h only where it iterates
        with pytest.raises(capi.SphError) as e:
            v.groups(0.5, link_h=True)
        assert e.value.status == SPH_ERR_STATE
        assert v.groups(0.5, link_h=True, clip=((v.field("x")[17] + 1e-9, -np.inf, -np.inf), (np.inf,) * 3))[2] >= 0
    v.close()
    ctx.groups(1.0)                                       # still usable
    ctx.close()


def test_cli_matches_context_groups(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "g.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.groups", str(save), "-o", str(out), "--link", "1.5",
                        "--min-members", "2", "--json", "--top", "3", "--csv", str(tmp_path / "g.csv")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    lab, tab, ng = ctx.groups(1.5, min_members=2)
    assert int(z["n_groups"]) == ng and np.array_equal(z["labels"], lab)
    for c in capi.GROUPS_COLUMNS:
        assert np.array_equal(z[c], tab[c], equal_nan=True), c
    import json
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["n_groups"] == ng and len(j["table"]) == min(3, ng)
    assert (tmp_path / "g.csv").exists()
    ctx.close()
