"""GPU tests of sph_render_field (include/summersph.h) on the MI355X: bitwise identity with the density render, numpy
brute force for both weights with and without normalisation, exact normalisation, bitwise projections, field ids against
value arrays (host and device) across re-sorts, determinism, no side effects on a running simulation, the argument and
state errors, combining the renders of separate contexts, the command line and a 10^6-particle edge-on map."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err
from gpu_support import capi, field_positions, make_context
import render_field_ref
import render_ref
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPH_ERR_ARG, SPH_ERR_STATE = 1, 5


def _ctx(capi, rows, variable=False, u_seed=None):
    gas, sinks = ic.split_rows(rows)
    if u_seed is not None:                                # a non-uniform u, so that a field render has something to show
        gas = dict(gas)
        gas["u"] = np.random.default_rng(u_seed).uniform(0.1, 0.5, gas["x"].size)
    return make_context(capi, gas, sinks, variable=variable), gas


def _seq_sum(grid, axis):
    acc = np.zeros(np.delete(grid.shape, axis))
    for k in range(grid.shape[axis]):
        acc = acc + np.take(grid, k, axis=axis)
    return acc


def _var_ctx(capi, n=2000, seed=17):
    ctx, gas = _ctx(capi, ic.keplerian_disc_var(n, seed=seed), variable=True, u_seed=seed)
    ctx.density(); ctx.update_h(); ctx.density()          # rho of the current h: the volume weight is readable
    return ctx


def test_identity_with_the_density_render(capi):
    fixed, _ = _ctx(capi, ic.keplerian_disc(3000, seed=9), u_seed=1)
    var = _var_ctx(capi)
    for ctx, hs in ((fixed, (1.25, None)), (var, (None, 2.0))):
        ones = np.ones(ctx.n)
        for h in hs:
            for n in [(23, 19, 11), (17, 1, 9)]:
                for axis in (None, 0, 1, 2):
                    for spacing in ((False, True) if axis is not None and n[axis] > 1 else (False,)):
                        kw = dict(axis=axis, h=h, spacing=spacing)
                        dens = ctx.render_density(n, **kw)
                        assert np.array_equal(ctx.render_field(ones, n, weight="mass", **kw), dens), (n, kw)
                        for f, norm in (("u", True), ("vz", False)):
                            img, w = ctx.render_field(f, n, weight="mass", normalise=norm, weight_out=True, **kw)
                            assert np.array_equal(w, dens), (f, n, kw)
                        assert dens.max() > 0
    fixed.close(); var.close()


def _brute_case(capi, variable):
    if variable:
        ctx = _var_ctx(capi, 2500, seed=23)
        h = ctx.field("h")
        assert not np.all(h == h[0])
        lo, hi, n = np.array([-30.0, -25.0, -6.0]), np.array([28.0, 30.0, 5.0]), (25, 27, 9)
        hr = None
    else:
        ctx, _ = _ctx(capi, ic.keplerian_disc(3000, seed=41), u_seed=4)
        ctx.density()
        h, hr = 1.25, 1.25
        lo, hi, n = np.array([-20.0, -15.0, -3.0]), np.array([25.0, 20.0, 3.5]), (29, 23, 11)
    return ctx, h, hr, lo, hi, n


@pytest.mark.parametrize("variable", [False, True])
def test_brute_force(capi, variable):
    ctx, h, hr, lo, hi, n = _brute_case(capi, variable)
    pos, m, rho = field_positions(ctx), ctx.field("m"), ctx.field("rho")
    a = np.random.default_rng(8).normal(0.3, 1.0, ctx.n)
    ref3 = {wt: render_field_ref.grid_brute(pos, w, a, h, lo, hi, n) for wt, w in (("mass", m), ("volume", m / rho))}
    for weight in ("mass", "volume"):
        num, den = ref3[weight]
        assert (den == 0).any() and (den > 0).any()
        for normalise in (False, True):
            for axis in (None, 0, 2):
                spacing = axis is not None and not normalise
                scale = (hi[axis] - lo[axis]) / (n[axis] - 1) if spacing else 1.0
                got, gw = ctx.render_field(a, n, bounds=(lo, hi), axis=axis, h=hr, spacing=spacing, weight=weight,
                                           normalise=normalise, weight_out=True)
                ref, rw = render_field_ref.image(num, den, axis, normalise, scale)
                assert rel_err(got, ref) <= TOL, (weight, normalise, axis)
                assert rel_err(gw, rw) <= TOL, (weight, normalise, axis)
                assert np.all(got[rw == 0] == 0.0) and np.all(gw[rw == 0] == 0.0)
    # a field id reads the same values from the context
    vx = ctx.field("vx")
    num, den = render_field_ref.grid_brute(pos, m / rho, vx, h, lo, hi, n)
    assert rel_err(ctx.render_field("vx", n, bounds=(lo, hi), h=hr, weight="volume"), num) <= TOL
    ctx.close()


def test_exact_normalisation(capi):
    ctx, _ = _ctx(capi, ic.keplerian_disc(3000, seed=12))
    two = np.full(ctx.n, 2.0)
    lo, hi, n = np.array([-50.0, -50.0, -12.0]), np.array([50.0, 50.0, 12.0]), (33, 31, 13)
    for axis in (None, 0, 1, 2):
        img, w = ctx.render_field(two, n, bounds=(lo, hi), axis=axis, normalise=True, weight_out=True)
        assert (w > 0).any() and (w == 0).any(), axis
        assert np.all(img[w > 0] == 2.0) and np.all(img[w == 0] == 0.0), axis
    ctx.close()


@pytest.mark.parametrize("variable", [False, True])
def test_projection_is_the_sequential_sum(capi, variable):
    ctx = _var_ctx(capi, 2500, seed=31) if variable else _ctx(capi, ic.keplerian_disc(3000, seed=9), u_seed=2)[0]
    for weight in (("mass", "volume") if variable else ("mass",)):
        for n in [(37, 29, 19), (33, 1, 13)]:
            num3, den3 = ctx.render_field("u", n, weight=weight, weight_out=True)
            lo, hi = ctx.render_bounds
            for axis in range(3):
                for spacing in ((False, True) if n[axis] > 1 else (False,)):
                    scale = (hi[axis] - lo[axis]) / (n[axis] - 1) if spacing else 1.0
                    p, pw = ctx.render_field("u", n, axis=axis, weight=weight, spacing=spacing, weight_out=True)
                    assert np.array_equal(p, _seq_sum(num3, axis) * scale), (n, axis, spacing)
                    assert np.array_equal(pw, _seq_sum(den3, axis) * scale), (n, axis, spacing)
                q = ctx.render_field("u", n, axis=axis, weight=weight, normalise=True)
                assert np.array_equal(q, render_field_ref.ratio(_seq_sum(num3, axis), _seq_sum(den3, axis))), (n, axis)
            g3 = ctx.render_field("u", n, weight=weight, normalise=True)
            assert np.array_equal(g3, render_field_ref.ratio(num3, den3))
    ctx.close()


def _three_ways(ctx, n, **kw):
    import torch
    a = ctx.render_field("u", n, **kw)
    b = ctx.render_field(ctx.field("u"), n, **kw)
    t = torch.from_numpy(ctx.field("u")).to(torch.device("cuda", 0))
    c = ctx.render_field(t, n, device=True, **kw).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, c), kw
    return a


def test_field_id_equals_values(capi):
    rows = ic.keplerian_disc(4000, seed=55)
    ctx, gas = _ctx(capi, rows, u_seed=6)
    n, kws = (40, 36, 12), [dict(axis=2, normalise=True), dict(axis=None), dict(axis=1, h=1.25, weight_out=False)]
    first = [_three_ways(ctx, n, **kw) for kw in kws]
    ctx.density()                                         # re-sorts the slots
    for kw, f in zip(kws, first):
        assert np.array_equal(_three_ways(ctx, n, **kw), f)
    dt, t = 1e-2, 0.0
    for _ in range(3):
        dt, t = ctx.step(dt, t)
    for kw in kws:
        _three_ways(ctx, n, **kw)
    # a reversed-order upload: values in that upload's order match the field id bitwise; the image matches the forward
    # upload's to rounding (the (cell, id) order follows the upload's ids)
    rev = capi.Context(device=0)
    rev.upload({k: v[::-1].copy() for k, v in gas.items()})
    rev.density()
    for kw, f in zip(kws, first):
        r = _three_ways(rev, n, **kw)
        assert rel_err(r, f) <= 1e-13, kw
    assert np.array_equal(rev.render_field(gas["u"][::-1].copy(), n, **kws[0]), rev.render_field("u", n, **kws[0]))
    ctx.close(); rev.close()


def test_determinism(capi):
    ctx, _ = _ctx(capi, ic.keplerian_disc(5000, seed=77), u_seed=7)
    ctx.density()
    for kw in (dict(axis=2, normalise=True, weight_out=True), dict(axis=None, weight="volume", weight_out=True)):
        a = ctx.render_field("u", (48, 40, 12), **kw)
        b = ctx.render_field("u", (48, 40, 12), **kw)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), kw
    ctx.close()


def _all_fields(ctx, capi):
    out = {}
    for f in capi.FIELDS:
        try:
            out[f] = ctx.field(f)
        except capi.SphError:          # not available in this mode / state (the same in both runs)
            out[f] = None
    return out


def _stats(ctx):
    s = ctx.stats()
    return {k: (tuple(getattr(s, k)) if k == "grid_dim" else getattr(s, k)) for k, _ in s._fields_ if k != "device_bytes"}


@pytest.mark.parametrize("variable,steps", [(False, 10), (True, 5)])
def test_render_field_has_no_side_effects(capi, variable, steps):
    rows = ic.keplerian_disc_var(2500, seed=5) if variable else ic.keplerian_disc(4000, seed=5)
    runs = []
    for with_render in (False, True):
        ctx, gas = _ctx(capi, rows, variable=variable)
        dt, t, dts = 1e-2, 0.0, []
        for k in range(steps):
            if with_render:
                ctx.render_field("u" if k % 2 else np.arange(ctx.n, dtype=np.float64), (40, 40, 8),
                                 axis=k % 3 if k % 2 else None, h=None if k % 3 else 1.25, normalise=k % 2 == 1,
                                 weight_out=k % 4 == 1)
                if k > 0 and not variable:                # after a fixed-h step the rates (and rho) are readable
                    ctx.render_field("vz", (24, 20, 8), axis=1, weight="volume", normalise=True, weight_out=True)
            dt, t = ctx.step(dt, t)
            dts.append(dt)
        if with_render:
            ctx.render_field("alpha", 24, h=None, weight_out=True)
        runs.append((_all_fields(ctx, capi), dts, t, _stats(ctx), ctx.get_sinks()))
        ctx.close()
    (f0, d0, t0, s0, k0), (f1, d1, t1, s1, k1) = runs
    assert d0 == d1 and t0 == t1
    assert [f for f in f0 if f0[f] is None] == [f for f in f1 if f1[f] is None]
    for f in f0:
        if f0[f] is not None:
            assert np.array_equal(f0[f], f1[f]), f
    assert s0 == s1
    for f in k0:
        assert np.array_equal(k0[f], k1[f]), f


def test_errors(capi):
    rows = ic.keplerian_disc(2000, seed=8)
    ctx, gas = _ctx(capi, rows)
    lib = ctx.lib
    vals = np.ones(ctx.n)
    shape = (10, 11, 12)

    def call(field="u", values=None, weight="mass", normalise=0, out_len=None, **over):
        d = ctx.render_field_desc(field, shape, ((-5, -5, -2), (5, 5, 2)), 2, None, None, True, weight, normalise)
        for k, v in over.items():
            if k == "base_reserved":
                d.base.reserved = v
            else:
                setattr(d, k, v)
        size = 10 * 11 if out_len is None else out_len
        out, w = np.full(max(size, 1), 7.0), np.full(max(size, 1), 7.0)
        st = lib.sph_render_field(ctx._h, C.byref(d), None if values is None else values.ctypes.data, out.ctypes.data,
                                  w.ctypes.data, size)
        return st, out, w

    assert call()[0] == 0
    assert call(field=capi.RENDER_FIELD_VALUES, values=vals)[0] == 0
    bad = [dict(field=19), dict(field=-2), dict(field=capi.RENDER_FIELD_VALUES), dict(field="u", values=vals),
           dict(weight=2), dict(weight=-1), dict(normalise=2), dict(normalise=-1), dict(reserved=1), dict(base_reserved=1),
           dict(out_len=10 * 12)]
    for b in bad:
        st, out, w = call(**b)
        assert st == SPH_ERR_ARG, b
        assert np.all(out == 7.0) and np.all(w == 7.0), b
    d = ctx.render_field_desc("u", 10, None, None, 1.25)
    assert lib.sph_render_field(ctx._h, C.byref(d), None, None, None, 1000) == SPH_ERR_ARG
    assert lib.sph_render_field(ctx._h, None, None, np.zeros(1000).ctypes.data, None, 1000) == SPH_ERR_ARG
    assert lib.sph_render_field(None, C.byref(d), None, np.zeros(1000).ctypes.data, None, 1000) == SPH_ERR_ARG
    assert lib.sph_render_field_dev(ctx._h, C.byref(d), None, None, None, 1000) == SPH_ERR_ARG
    # state: rho is stale after the upload, du before the forces; an argument error still wins over a stale field
    for kw in (dict(weight=1), dict(field="rho"), dict(field="du"), dict(field="h")):
        st, out, _ = call(**kw)
        assert st == SPH_ERR_STATE and np.all(out == 7.0), kw
    assert call(field="rho", out_len=3)[0] == SPH_ERR_ARG
    with pytest.raises(capi.SphError):
        ctx.render_field("u", 10, weight="volume")
    ctx.density()
    assert call(weight=1)[0] == 0 and call(field="rho")[0] == 0
    st, out, _ = call(field="du")
    assert st == SPH_ERR_STATE and np.all(out == 7.0)
    # the context steps bitwise as one that saw no errors
    clean, _ = _ctx(capi, rows)
    clean.density()
    for c in (ctx, clean):
        c.step(1e-2)
    for f in ("x", "vz", "u", "rho", "du"):
        assert np.array_equal(ctx.field(f), clean.field(f)), f
    ctx.close(); clean.close()


def test_combining_contexts(capi):
    gas, _ = ic.split_rows(ic.keplerian_disc(6000, seed=63))
    left = gas["x"] < 0.0
    whole = capi.Context(device=0); whole.upload(gas)
    parts = []
    for sel in (left, ~left):
        c = capi.Context(device=0); c.upload({k: v[sel].copy() for k, v in gas.items()}); parts.append(c)
    lo, hi, n = np.array([-30.0, -30.0, -5.0]), np.array([30.0, 30.0, 5.0]), (61, 33, 21)
    for field in ("vz", "vy"):
        for axis in (None, 1):
            img, w = whole.render_field(field, n, bounds=(lo, hi), axis=axis, normalise=True, weight_out=True)
            sums = [c.render_field(field, n, bounds=(lo, hi), axis=axis, weight_out=True) for c in parts]
            num = sums[0][0] + sums[1][0]
            den = sums[0][1] + sums[1][1]
            assert rel_err(den, w) <= 1e-13, (field, axis)
            assert rel_err(render_field_ref.ratio(num, den), img) <= 1e-13, (field, axis)
            assert np.array_equal(den == 0, w == 0) and (w > 0).any()
    for c in [whole] + parts:
        c.close()


def test_cli_matches_the_api(capi, tmp_path):
    g = load_golden("render_script12k")
    save = tmp_path / "save275.txt"
    txtio.write_save(str(save), g["gas"], g["sinks"])
    out, wout = tmp_path / "v.npy", tmp_path / "w.npy"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-m", "summersph_amd.render", str(save), "--field", "vz", "--axis", "y", "-o", str(out),
                    "--weight-out", str(wout)], check=True, cwd=ROOT, env=env, timeout=300)
    from summersph_amd import render
    rows, _, _ = render.read_save(str(save))
    ctx = capi.Context(device=0)
    ctx.upload({k: rows[:, i] for i, k in enumerate("x y z vx vy vz u m alpha".split())})
    img, w = ctx.render_field("vz", 120, axis="y", normalise=True, weight_out=True)
    got = np.load(out)
    assert got.shape == (120, 120)
    assert np.array_equal(got, img) and np.array_equal(np.load(wout), w)
    assert np.array_equal(w, ctx.render_density(120, axis="y"))
    ctx.close()


def test_scale_1e6_edge_on_velocity_map(capi):
    rows = ic.keplerian_disc_var(1_000_000, seed=99)
    ctx, _ = _ctx(capi, rows, variable=True)
    ctx.density(); ctx.update_h()
    n = (512, 512, 64)
    # the initial disc has vz == 0: the edge-on moment-1 map is that of the line-of-sight velocity vy
    img, w = ctx.render_field("vy", n, axis="y", normalise=True, weight_out=True)
    assert img.shape == (512, 64)
    lo, hi = ctx.render_bounds
    pos = field_positions(ctx)
    m, hv, vy = ctx.field("m"), ctx.field("h"), ctx.field("vy")
    ax = render_ref.axes(lo, hi, n)
    rng = np.random.default_rng(2)
    nz = np.argwhere(w > 0)
    cols = np.vstack([nz[rng.choice(nz.shape[0], 180, replace=False)], np.column_stack([rng.integers(0, 512, 20), rng.integers(0, 64, 20)])])
    scale = np.max(np.abs(img))
    assert scale > 0
    for i, k in cols:
        gx, gz = ax[0][i], ax[2][k]
        near = (np.abs(pos[:, 0] - gx) <= 2 * hv * (1 + 1e-9)) & (np.abs(pos[:, 2] - gz) <= 2 * hv * (1 + 1e-9))
        if not near.any():
            assert img[i, k] == 0.0 and w[i, k] == 0.0
            continue
        nodes = np.stack([np.full(n[1], gx), ax[1], np.full(n[1], gz)], axis=1)
        num, den = render_field_ref.brute(nodes, pos[near], m[near], vy[near], hv[near])
        ref = num.sum() / den.sum() if den.sum() > 0 else 0.0
        assert abs(img[i, k] - ref) <= TOL * scale, (i, k)
    ctx.close()
