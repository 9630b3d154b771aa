"""GPU tests of sph_gradients (include/summersph.h, "SPH gradients") on the MI355X: parity with the numpy restatement
(the fixtures, a uniform box, a variable-h disc, both forms, 1 .. 4 fields, context fields and values, 10^6 particles),
linear fields, a planar set, the order rule, ranks with ghosts, a cull, no side effects on a running simulation, the
device form, the argument errors, a target whose h spans the box, and the command line."""
import ctypes as C
import json
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT
from gpu_support import capi, field_positions, golden_gas, make_context, over_defaults, ref_h
import gradients_ref
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5


def _ctx(capi, gas, sinks=None, variable=False, flags=0, density=True):
    return make_context(capi, gas, sinks, variable=variable, flags=over_defaults(capi, flags, variable), density=density)


def _cmp(g, rg, rho=None, rrho=None, tol=1e-12, ratio=None):
    """every component within tol of the field's largest |grad| over the targets.  ratio (the restatement's det C /
    (tr C / 3)^3, corrected form): a target near the singular threshold (ratio < 1e-3) amplifies the last-bit differences
    of the sums by up to the condition number of C, so those are held to 1e-9 of the scale instead"""
    assert np.array_equal(np.isnan(g), np.isnan(rg))
    for k in range(g.shape[0]):
        ok = np.isfinite(rg[k])
        s = np.max(np.abs(rg[k][ok]))
        err = np.abs(g[k] - rg[k])
        if ratio is None:
            assert np.max(err[ok]) <= tol * s, k
        else:
            good = ok & (ratio >= 1e-3)
            assert np.max(err[good]) <= tol * s, k
            assert np.max(err[ok]) <= 1e-9 * s, k
    if rho is not None:
        assert np.array_equal(np.isnan(rho), np.isnan(rrho))
        ok = np.isfinite(rrho)
        assert np.max(np.abs(rho[ok] - rrho[ok]) / np.abs(rrho[ok])) <= 1e-13


SETS = ["disc3000_eval", "discv3000_eval", "bin2000_eval", "box20000", "discvar20000"]


def _set(capi, name):
    if name == "box20000":
        gas, sinks = ic.split_rows(ic.uniform_box(20000))
        return _ctx(capi, gas, sinks)
    if name == "discvar20000":
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000))
        return _ctx(capi, gas, sinks, variable=True)
    gas, sinks = golden_gas(name)
    return _ctx(capi, gas, sinks, variable="discv" in name)


@pytest.mark.parametrize("name", SETS)
def test_parity_with_the_restatement(capi, name):
    ctx = _set(capi, name)
    n = ctx.n
    pos, m = field_positions(ctx), ctx.field("m")
    rng = np.random.default_rng(3)
    vals = np.stack([rng.normal(size=n), pos[:, 0] * pos[:, 1]])
    A = np.stack([ctx.field("vx"), ctx.field("vy"), ctx.field("u"), ctx.field("rho")])
    h = ref_h(ctx, capi)
    for corrected in (True, False):
        inf = {}
        rg, rr, nt, ns = gradients_ref.gradients(pos, m, np.concatenate([A, vals]), h, corrected=corrected, info=inf)
        ratio = inf["ratio"] if corrected else None
        # context fields, 1 .. 4 of them
        for k in range(1, 5):
            g, rho, (t, s) = ctx.gradients(fields=("vx", "vy", "u", "rho")[:k], corrected=corrected, rho=True)
            assert (t, s) == (nt, ns)
            _cmp(g, rg[:k], rho, rr, ratio=ratio)
        # values rows (and a mix with a context field)
        g, _, (t, s) = ctx.gradients(fields=(capi.GRAD_VALUES, capi.GRAD_VALUES), values=vals, corrected=corrected)
        assert (t, s) == (nt, ns)
        _cmp(g, rg[4:6], ratio=ratio)
        g, _, _ = ctx.gradients(fields=("vx", capi.GRAD_VALUES), values=vals, corrected=corrected)
        _cmp(g[1:], rg[5:6], ratio=ratio)
        _cmp(g[:1], rg[:1], ratio=ratio)
    ctx.close()


def test_million_particle_disc(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(1_000_000, seed=5))
    ctx = _ctx(capi, gas, sinks, density=False)
    g, rho, (nt, ns) = ctx.gradients(rho=True)
    assert nt == ctx.n and ns < 0.01 * nt                         # the thin outskirts of the disc
    pos, m = field_positions(ctx), ctx.field("m")
    A = np.stack([ctx.field("vx"), ctx.field("vy"), ctx.field("vz")])
    ids = np.sort(np.random.default_rng(7).choice(ctx.n, 2000, replace=False))
    inf = {}
    rg, rr, _, _ = gradients_ref.gradients(pos, m, A, 2.5, only=ids, info=inf)
    _cmp(g[:, :, ids], rg[:, :, ids], rho[ids], rr[ids], ratio=inf["ratio"][ids])
    f = {k: ctx.field(k) for k in ("x", "y", "z")}
    sel, r = _keplerian_cut(f)
    omega = np.sqrt(ic.G_DP / r ** 3)
    wz = g[1, 0] - g[0, 1]
    err = (np.abs(wz - omega / 2) / (omega / 2))[sel]
    print(f"10^6 disc: omega_z vs Omega/2 median {np.median(err):.4f} p90 {np.percentile(err, 90):.4f}")
    assert np.median(err) <= 0.03
    ctx.close()


def _keplerian_cut(f, r_in=10.0):
    r = np.hypot(f["x"], f["y"])
    return (np.abs(f["z"]) < 2.5) & (r > r_in + 10.0) & (r < r.max() - 10.0), r


@pytest.mark.parametrize("which", ["box", "discvar"])
def test_linear_fields_are_exact(capi, which):
    if which == "box":
        gas, sinks = ic.split_rows(ic.uniform_box(20000, seed=3))
        ctx = _ctx(capi, gas, sinks, density=False)
        hs = [None, 3.0]
    else:
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000, seed=4))
        ctx = _ctx(capi, gas, sinks, variable=True, density=False)
        hs = [None]
    pos = field_positions(ctx)
    G = np.random.default_rng(5).normal(size=(4, 3))
    vals = 1.0 + G @ pos.T
    for h in hs:
        g, _, (nt, ns) = ctx.gradients(fields=(capi.GRAD_VALUES,) * 4, values=vals, h=h)
        ok = np.isfinite(g[0, 0])
        assert ok.sum() == nt - ns and nt == ctx.n
        for k in range(4):
            assert np.max(np.abs(g[k][:, ok] - G[k][:, None])) <= 1e-11 * np.max(np.abs(G[k]))
    ctx.close()


def test_planar_set(capi):
    rng = np.random.default_rng(13)
    n = 4000
    gas = {"x": rng.uniform(0, 40, n), "y": rng.uniform(0, 40, n), "z": np.zeros(n), "vx": rng.normal(size=n),
           "vy": rng.normal(size=n), "vz": np.zeros(n), "u": np.full(n, 0.25), "m": np.full(n, 1e-6), "alpha": np.zeros(n)}
    ctx = _ctx(capi, gas, density=False)
    g, rho, (nt, ns) = ctx.gradients(rho=True)
    assert nt == ns == n and np.all(np.isnan(g)) and np.all(np.isfinite(rho))
    g, _, (nt, ns) = ctx.gradients(corrected=False, fields=("vx", "vy", "x"))
    assert ns == 0 and np.all(np.isfinite(g)) and np.all(g[:, 2] == 0.0)
    ctx.close()


# ---- order rule --------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2]


@pytest.mark.parametrize("variable", [False, True])
def test_order_rule_bitwise(capi, variable):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(40000, seed=15) if variable else ic.keplerian_disc(40000, seed=15))
    a = _ctx(capi, gas, sinks, variable=variable, density=False)
    kw = {"fields": ("vx", "vy", "vz", "u"), "rho": True}
    h0 = a.field("h") if variable else None
    r0 = a.gradients(**kw)
    _same(r0, a.gradients(**kw))                                   # repeated
    a.density()                                                    # re-sorted slots
    if variable:
        a.upload_field("h", h0)                                    # the density pass iterated h: the uploaded one again
    _same(r0, a.gradients(**kw))
    c = _ctx(capi, gas, sinks, variable=variable, flags=capi.FLAG_HASHED_GRID)
    assert c.grid_info().kind == 1
    if variable:
        c.upload_field("h", h0)
    _same(r0, c.gradients(**kw))
    c.close()
    # clip: the common targets bitwise
    clip = ((-40.0, -30.0, -2.0), (35.0, 30.0, 3.0))
    g, rho, (nt, _) = a.gradients(clip=clip, **kw)
    t = gradients_ref.targets_mask(field_positions(a), a.n, clip)
    assert nt == int(t.sum()) > 0
    assert np.all(np.isnan(g[:, :, ~t])) and np.all(np.isnan(rho[~t]))
    assert np.array_equal(g[:, :, t], r0[0][:, :, t], equal_nan=True) and np.array_equal(rho[t], r0[1][t])
    # an owned / ghost split of the same upload
    s = _ctx(capi, gas, sinks, variable=variable, density=False)
    s.set_owned(25000)
    g, rho, (nt, _) = s.gradients(**kw)
    assert nt == 25000 and np.all(np.isnan(g[:, :, 25000:]))
    assert np.array_equal(g[:, :, :25000], r0[0][:, :, :25000], equal_nan=True) and np.array_equal(rho[:25000], r0[1][:25000])
    s.close()
    a.close()


def test_ranks_with_ghosts_agree_with_one_context(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(30000, seed=17))
    one = _ctx(capi, gas, sinks, variable=True, density=False)
    g1, r1, (nt1, _) = one.gradients(fields=("vx", "vy", "vz", "u"), rho=True)
    one.close()
    x, h = gas["x"], gas["h"]
    reach = 2.0 * h.max()
    got = np.full_like(g1, np.nan)
    rho = np.full_like(r1, np.nan)
    total = 0
    for lo, hi in ((-np.inf, 0.0), (0.0, np.inf)):
        own = np.nonzero((x >= lo) & (x < hi))[0]
        ghost = np.nonzero(~((x >= lo) & (x < hi)) & (x >= lo - reach) & (x < hi + reach))[0]
        ids = np.concatenate([own, ghost])
        ctx = _ctx(capi, {k: v[ids] for k, v in gas.items()}, sinks, variable=True, density=False)
        ctx.set_owned(own.size)
        g, r, (nt, _) = ctx.gradients(fields=("vx", "vy", "vz", "u"), rho=True)
        assert np.all(np.isnan(g[:, :, own.size:]))
        got[:, :, own] = g[:, :, :own.size]
        rho[own] = r[:own.size]
        total += nt
        ctx.close()
    assert total == nt1
    assert np.array_equal(np.isnan(got), np.isnan(g1))
    for k in range(4):
        ok = np.isfinite(g1[k])
        assert np.max(np.abs(got[k][ok] - g1[k][ok])) <= 1e-13 * np.max(np.abs(g1[k][ok])), k
    assert np.max(np.abs(rho - r1) / r1) <= 1e-13


def test_after_accrete_and_cull(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=12))
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])
    ctx = _ctx(capi, gas, sinks)
    ctx.forces()
    assert ctx.accrete_and_cull() > 0 and ctx.n < 20000
    g, rho, (nt, ns) = ctx.gradients(fields=("vx", "vy", "rho"), rho=True)
    assert g.shape == (3, 3, ctx.n) and nt == ctx.n
    A = np.stack([ctx.field("vx"), ctx.field("vy"), ctx.field("rho")])
    inf = {}
    rg, rr, rnt, rns = gradients_ref.gradients(field_positions(ctx), ctx.field("m"), A, 2.5, info=inf)
    assert (nt, ns) == (rnt, rns)
    _cmp(g, rg, rho, rr, ratio=inf["ratio"])
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    runs = []
    for with_grad in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_grad:
                before = {k: ctx.field(k) for k in ("x", "vx", "rho", "ax", "du")}
                ctx.gradients(fields=("vx", "vy", "vz", "rho"), rho=True)
                ctx.gradients(fields=("u",), corrected=False, h=1.0, clip=((0, 0, -1), (50, 50, 1)))
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


def test_device_form_is_bitwise_the_host_form(capi):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(30000, seed=31))
    ctx = _ctx(capi, gas, sinks, variable=True)
    vals = np.random.default_rng(2).normal(size=(2, ctx.n))
    dv = torch.from_numpy(vals).to(torch.device("cuda", 0))
    for kw in ({}, {"corrected": False, "h": 2.0}, {"fields": ("rho", capi.GRAD_VALUES), "clip": ((-30, -30, -3), (30, 30, 3))}):
        hv = vals if capi.GRAD_VALUES in kw.get("fields", ()) else None
        g, rho, cnt = ctx.gradients(rho=True, values=hv, **kw)
        dg, drho, dcnt = ctx.gradients(rho=True, device=True, values=None if hv is None else dv, **kw)
        assert isinstance(dg, torch.Tensor) and dcnt == cnt
        assert np.array_equal(dg.cpu().numpy(), g, equal_nan=True) and np.array_equal(drho.cpu().numpy(), rho, equal_nan=True)
    ctx.close()


def test_errors(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(3000, seed=37))
    ctx = _ctx(capi, gas, sinks, density=False)
    lib = ctx.lib
    n = ctx.n
    out = np.empty(3 * 4 * n)
    vals = np.zeros((4, n))
    nt, ns = C.c_int64(0), C.c_int64(0)

    def call(d, values=None, n_out=None, o=out):
        nf = d.n_fields if d is not None else 1
        return lib.sph_gradients(ctx._h, None if d is None else C.byref(d), None if values is None else values.ctypes.data,
                                 None if o is None else o.ctypes.data, 3 * nf * n if n_out is None else n_out, None,
                                 C.byref(nt), C.byref(ns))

    D = capi.gradients_desc
    assert call(D(("rho",))) == SPH_ERR_STATE                       # rho stale
    assert call(D(("ax",))) == SPH_ERR_STATE                        # rates stale
    assert call(D(("h",))) == SPH_ERR_STATE                         # no h field on a fixed-h context
    assert call(D()) == 0 and nt.value == n
    ctx.density()
    assert call(D(("rho", "P", "c"))) == 0
    assert call(None) == SPH_ERR_ARG
    for k in (0, 5):
        d = D(); d.n_fields = k
        assert call(d, n_out=3 * max(k, 1) * n) == SPH_ERR_ARG, k
    for bad in (-2, 19, 100):
        d = D(); d.fields[1] = bad
        assert call(d) == SPH_ERR_ARG, bad
    assert call(D((capi.GRAD_VALUES,))) == SPH_ERR_ARG               # values missing
    assert call(D(("u",)), values=vals) == SPH_ERR_ARG               # values given, none asked for
    assert call(D((capi.GRAD_VALUES,)), values=vals) == 0
    assert call(D(), n_out=3 * 3 * n - 1) == SPH_ERR_ARG
    assert call(D(), o=None) == SPH_ERR_ARG
    for bad in (-1.0, np.nan):
        assert call(D(h=bad)) == SPH_ERR_ARG, bad
    assert call(D(clip=((np.nan, 0, 0), (1, 1, 1)))) == SPH_ERR_ARG
    assert call(D(clip=((0, 0, 0), (1, 1, np.nan)))) == SPH_ERR_ARG
    d = D(); d.flags = 2
    assert call(d) == SPH_ERR_ARG
    d = D(); d.reserved[1] = 1
    assert call(d) == SPH_ERR_ARG
    assert lib.sph_gradients(None, C.byref(D()), None, out.ctypes.data, 9 * n, None, None, None) == SPH_ERR_ARG
    # an empty target set: 0 targets, all NaN
    g, rho, cnt = ctx.gradients(rho=True, clip=((1e9,) * 3, (2e9,) * 3))
    assert cnt == (0, 0) and np.all(np.isnan(g)) and np.all(np.isnan(rho))
    ctx.close()
    # a bad target h (variable h): SPH_ERR_STATE in the host form, d_counts[0] == -1 and NaN rows in the device form
    gv, sv = ic.split_rows(ic.keplerian_disc_var(3000, seed=38))
    v = _ctx(capi, gv, sv, variable=True, density=False)
    h = v.field("h")
    h[17] = -1.0
    v.upload_field("h", h)
    with pytest.raises(capi.SphError) as e:
        v.gradients()
    assert e.value.status == SPH_ERR_STATE
    dg, _, dcnt = v.gradients(device=True)
    assert dcnt[0] == -1 and bool(dg.isnan().all())
    x17 = v.field("x")[17]
    assert v.gradients(clip=((x17 + 1e-9, -np.inf, -np.inf), (np.inf,) * 3))[2][0] > 0     # 17 outside: fine
    assert v.gradients(h=2.0)[2][0] == v.n
    v.close()


def test_a_target_whose_h_spans_the_box(capi):
    gas, sinks = ic.split_rows(ic.uniform_box(20000, seed=21))
    gas["h"] = np.full(gas["x"].size, 2.5)
    gas["h"][123] = 1e3
    ctx = _ctx(capi, gas, sinks, variable=True, density=False)
    assert ctx.field("h")[123] == 1e3
    vals = np.stack([ctx.field("vx"), ctx.field("x") * 2.0 - ctx.field("z")])
    t0 = time.perf_counter()
    g, rho, (nt, ns) = ctx.gradients(fields=("vx", capi.GRAD_VALUES), values=vals, rho=True)
    dt = time.perf_counter() - t0
    print(f"h spanning the box: host form {dt * 1e3:.1f} ms for {nt} targets")
    inf = {}
    rg, rr, rnt, rns = gradients_ref.gradients(field_positions(ctx), ctx.field("m"), vals, ctx.field("h"), info=inf)
    assert (nt, ns) == (rnt, rns)
    _cmp(g, rg, rho, rr, ratio=inf["ratio"])
    assert np.allclose(g[1, :, 123], [2.0, 0.0, -1.0], rtol=0, atol=1e-11)
    assert abs(rho[123] - np.sum(ctx.field("m")) * (1 / (np.pi * 1e9))) <= 0.02 * rho[123]     # q <= 0.1: w ~ 1
    ctx.close()


def test_cli_matches_context_gradients(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "g.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.gradients", str(save), "-o", str(out), "--fields", "vx,vy,vz,rho",
                        "--json"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    g, rho, (nt, ns) = ctx.gradients(fields=("vx", "vy", "vz", "rho"), rho=True)
    for k, f in enumerate(("vx", "vy", "vz", "rho")):
        assert np.array_equal(z[f"grad_{f}"], g[k], equal_nan=True), f
    assert np.array_equal(z["rho_sph"], rho, equal_nan=True)
    v = capi.velocity_derivatives(g[:3])
    assert np.array_equal(z["divv"], v["divv"], equal_nan=True) and np.array_equal(z["curl"], v["curl"], equal_nan=True)
    assert int(z["n_targets"]) == nt and int(z["n_singular"]) == ns and int(z["desc_flags"]) == capi.GRAD_CORRECTED
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["n_targets"] == nt and j["n_singular"] == ns
    ok = np.isfinite(v["divv"])
    assert j["median_omega_z"] == float(np.median(v["curl"][2][ok]))
    ctx.close()
