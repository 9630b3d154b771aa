"""GPU tests of sph_render_density (include/summersph.h) on the MI355X: the reference script's image, numpy brute force
for fixed and per-particle h, bitwise projections and determinism, no side effects on a running simulation, the
selection rules, the argument errors, and a 10^6-particle projection."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gpu_support import capi, make_context, positions
import render_ref
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPH_ERR_ARG = 1


def _ctx(capi, rows, variable=False):
    gas, sinks = ic.split_rows(rows)
    return make_context(capi, gas, sinks, variable=variable), gas, sinks


def _check_field(got, ref, pos, m, h, lo, hi, n):
    scale = np.max(np.abs(ref))
    assert scale > 0
    assert np.max(np.abs(got - ref)) <= TOL * scale
    # exact zeros where no particle lies within 2h (1 + 1e-12) of the node
    X, Y, Z = np.meshgrid(*render_ref.axes(lo, hi, n), indexing="ij")
    nodes = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), m.shape)
    far = np.ones(nodes.shape[0], dtype=bool)
    for s in range(0, nodes.shape[0], 2048):
        d = np.sqrt(((nodes[s:s + 2048, None, :] - pos[None]) ** 2).sum(axis=2))
        far[s:s + 2048] = ~np.any(d <= 2.0 * hh[None] * (1 + 1e-12), axis=1)
    assert np.all(got.ravel()[far] == 0.0)
    assert (~far).any()


def test_script_parity_cli(tmp_path):
    g = load_golden("render_script12k")
    save = tmp_path / "save275.txt"
    txtio.write_save(str(save), g["gas"], g["sinks"])
    out = tmp_path / "img.npy"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-m", "summersph_amd.render", str(save), "-o", str(out), "--script-compat"],
                   check=True, cwd=ROOT, env=env, timeout=300)
    img, ref = np.load(out), g["projected_density"]
    assert img.shape == ref.shape
    assert np.max(np.abs(img - ref)) <= TOL * ref.max()
    assert np.all(img[ref == 0] == 0.0)


def _edge_set(rows, h, lo, hi):
    """particles outside the node box but within 2h, and at exactly 2h / one ulp either side of a node"""
    extra = []
    node = np.array([lo[0], lo[1], lo[2]])
    for r in (2 * h, np.nextafter(2 * h, 0), np.nextafter(2 * h, 4 * h), 1.5 * h):
        p = node.copy(); p[0] -= r                       # outside the box (x < lo), within / at 2h of the corner node
        extra.append(p)
    p = np.array([hi[0], hi[1], hi[2]]); p[2] += 1.9 * h
    extra.append(p)
    e = np.zeros((len(extra), 8)); e[:, :3] = extra; e[:, 6] = 0.3; e[:, 7] = rows[0, 7]
    return np.vstack([e, rows])


def _clustered(n=2500, seed=11):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20, 20, (6, 3))
    pts = c[rng.integers(0, 6, n)] + rng.normal(0, rng.uniform(0.5, 4, n)[:, None], (n, 3))
    rows = np.zeros((n, 8)); rows[:, :3] = pts; rows[:, 6] = 0.2; rows[:, 7] = rng.uniform(1e-7, 3e-6, n)
    return rows


@pytest.mark.parametrize("case", ["sod", "disc3000", "clustered"])
def test_grid_fixed_h_vs_brute_force(capi, case):
    h = 1.25
    if case == "sod":
        rows, lo, hi, n = ic.sod_column(), np.array([-20.0, -2.0, -2.0]), np.array([30.0, 2.5, 2.0]), (41, 9, 7)
    elif case == "disc3000":
        rows, lo, hi, n = ic.keplerian_disc(3000, seed=41), np.array([-20.0, -15.0, -3.0]), np.array([25.0, 20.0, 3.5]), (29, 23, 11)
    else:
        rows, lo, hi, n = _clustered(), np.array([-18.0, -16.0, -14.0]), np.array([17.0, 15.0, 16.0]), (21, 19, 17)
    rows = _edge_set(rows, h, lo, hi)
    ctx, gas, _ = _ctx(capi, rows)
    got = ctx.render_density(n, bounds=(lo, hi), h=h)
    assert got.shape == n
    pos, m = positions(gas), gas["m"]
    ref = render_ref.grid_brute(pos, m, h, lo, hi, n)
    _check_field(got, ref, pos, m, h, lo, hi, n)
    ctx.close()


def test_per_particle_h_variable_context(capi):
    rows = ic.keplerian_disc_var(2000, seed=17)
    ctx, gas, _ = _ctx(capi, rows, variable=True)
    ctx.density(); ctx.update_h()
    hv = ctx.field("h")
    assert not np.all(hv == hv[0])
    lo, hi, n = np.array([-30.0, -25.0, -6.0]), np.array([28.0, 30.0, 5.0]), (25, 27, 9)
    got = ctx.render_density(n, bounds=(lo, hi))
    pos = np.stack([ctx.field(k) for k in "xyz"], axis=1)
    m = ctx.field("m")
    ref = render_ref.grid_brute(pos, m, hv, lo, hi, n)
    _check_field(got, ref, pos, m, hv, lo, hi, n)
    # a fixed-h context's "own h" is params.h
    ctx2, gas2, _ = _ctx(capi, ic.keplerian_disc(1500, seed=3))
    g2 = ctx2.render_density((15, 16, 7), bounds=(lo, hi))
    assert np.array_equal(g2, ctx2.render_density((15, 16, 7), bounds=(lo, hi), h=ctx2.params.h))
    ctx.close(); ctx2.close()


def _seq_sum(grid, axis):
    acc = np.zeros(np.delete(grid.shape, axis))
    for k in range(grid.shape[axis]):
        acc = acc + np.take(grid, k, axis=axis)
    return acc


@pytest.mark.parametrize("h", [1.25, None])
def test_projection_is_the_sequential_sum(capi, h):
    rows = ic.keplerian_disc(3000, seed=9)
    ctx, gas, _ = _ctx(capi, rows)
    for n in [(37, 29, 19), (33, 1, 13), (1, 25, 1)]:
        grid = ctx.render_density(n, h=h)
        lo, hi = ctx.render_bounds
        for axis in range(3):
            proj = ctx.render_density(n, axis=axis, h=h)
            assert np.array_equal(ctx.render_bounds[0], lo) and np.array_equal(ctx.render_bounds[1], hi)
            assert np.array_equal(proj, _seq_sum(grid, axis)), (n, axis)
            if n[axis] > 1:
                sp = ctx.render_density(n, axis=axis, h=h, spacing=True)
                assert np.array_equal(sp, _seq_sum(grid, axis) * ((hi[axis] - lo[axis]) / (n[axis] - 1))), (n, axis)
    dev = ctx.render_density((37, 29, 19), axis="z", h=h, device=True)
    assert np.array_equal(dev.cpu().numpy(), _seq_sum(ctx.render_density((37, 29, 19), h=h), 2))
    ctx.close()


def test_determinism_and_independence_of_sorted_order(capi):
    rows = ic.keplerian_disc(5000, seed=77)
    ctx, gas, _ = _ctx(capi, rows)
    a = ctx.render_density((48, 40, 12), axis=2, h=1.25)
    b = ctx.render_density((48, 40, 12), axis=2, h=1.25)
    g0 = ctx.render_density((30, 30, 10), h=1.25)
    assert np.array_equal(a, b)
    ctx.density()                                         # re-sorts the particles into cell order
    assert np.array_equal(a, ctx.render_density((48, 40, 12), axis=2, h=1.25))
    assert np.array_equal(g0, ctx.render_density((30, 30, 10), h=1.25))
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
def test_render_has_no_side_effects(capi, variable, steps):
    rows = ic.keplerian_disc_var(2500, seed=5) if variable else ic.keplerian_disc(4000, seed=5)
    runs = []
    for with_render in (False, True):
        ctx, gas, _ = _ctx(capi, rows, variable=variable)
        dt, t, dts = 1e-2, 0.0, []
        for k in range(steps):
            if with_render:
                ctx.render_density((40, 40, 8), axis=k % 3 if k % 2 else None, h=None if k % 3 else 1.25)
            dt, t = ctx.step(dt, t)
            dts.append(dt)
        if with_render:
            ctx.render_density(24, h=None)
        runs.append((_all_fields(ctx, capi), dts, t, _stats(ctx), ctx.get_sinks()))
        ctx.close()
    (f0, d0, t0, s0, k0), (f1, d1, t1, s1, k1) = runs
    assert d0 == d1 and t0 == t1
    assert [f for f in f0 if f0[f] is None] == [f for f in f1 if f1[f] is None]
    assert sum(f0[f] is not None for f in f0) >= 17
    for f in f0:
        if f0[f] is not None:
            assert np.array_equal(f0[f], f1[f]), f
    assert s0 == s1
    for f in k0:
        assert np.array_equal(k0[f], k1[f]), f


def test_selection_sinks_ghosts_clip_and_auto_bounds(capi):
    rows = ic.keplerian_disc(3000, seed=21)
    gas, sinks = ic.split_rows(rows)
    # sinks are never rendered: the central 1-Msun sink changes nothing
    c1 = capi.Context(device=0); c1.upload(gas); c1.set_sinks(sinks)
    c2 = capi.Context(device=0); c2.upload(gas)
    lo, hi = np.array([-12.0, -12.0, -3.0]), np.array([12.0, 12.0, 3.0])
    assert np.array_equal(c1.render_density((25, 25, 7), bounds=(lo, hi), h=1.25),
                          c2.render_density((25, 25, 7), bounds=(lo, hi), h=1.25))
    # ghosts (ids >= n_owned) are excluded
    n_own = 2000
    c3 = capi.Context(device=0); c3.upload(gas); c3.set_owned(n_own)
    c4 = capi.Context(device=0); c4.upload({k: v[:n_own] for k, v in gas.items()})
    for c in (c3, c4):
        c.density()
    g3 = c3.render_density((30, 30, 9), h=1.25)
    assert np.array_equal(g3, c4.render_density((30, 30, 9), h=1.25))
    assert np.array_equal(c3.render_bounds[0], c4.render_bounds[0]) and np.array_equal(c3.render_bounds[1], c4.render_bounds[1])
    # strict clip: particles exactly on the clip planes are out; auto bounds follow the clipped set
    cl, ch = np.array([-15.0, -10.0, -2.0]), np.array([15.0, 12.0, 2.0])
    g = {k: v.copy() for k, v in gas.items()}
    g["x"][:3] = cl[0]; g["y"][3:6] = ch[1]
    c5 = capi.Context(device=0); c5.upload(g)
    p5 = positions(g)
    keep = np.all((p5 > cl) & (p5 < ch), axis=1)
    img = c5.render_density((20, 18, 6), clip=(cl, ch), h=1.25)
    lo5, hi5 = c5.render_bounds
    assert np.array_equal(lo5, p5[keep].min(axis=0)) and np.array_equal(hi5, p5[keep].max(axis=0))
    ref = render_ref.grid_brute(p5[keep], g["m"][keep], 1.25, lo5, hi5, (20, 18, 6))
    assert np.max(np.abs(img - ref)) <= TOL * ref.max()
    # the descriptor carries the written-back box
    d = c5.render_desc((20, 18, 6), None, None, 1.25, (cl, ch))
    out = np.empty(20 * 18 * 6)
    assert c5.lib.sph_render_density(c5._h, C.byref(d), out.ctypes.data, out.size) == 0
    assert list(d.lo) == lo5.tolist() and list(d.hi) == hi5.tolist()
    assert np.array_equal(out.reshape(20, 18, 6), img)
    for c in (c1, c2, c3, c4, c5):
        c.close()


def test_argument_errors(capi):
    rows = ic.keplerian_disc(2000, seed=8)
    ctx, gas, _ = _ctx(capi, rows)
    lib = ctx.lib
    good = dict(shape=(10, 11, 12), bounds=((-5, -5, -2), (5, 5, 2)), axis=2, h=1.25, clip=None, spacing=True)

    def call(out_len=None, dev=False, **over):
        kw = dict(good); kw.update({k: v for k, v in over.items() if k in good})
        d = ctx.render_desc(kw["shape"], kw["bounds"], kw["axis"], kw["h"], kw["clip"], kw["spacing"])
        for k, v in over.items():
            if k not in good:
                setattr(d, k, v)
        n = ctx.render_shape(d)
        size = int(np.prod(n)) if out_len is None else out_len
        buf = np.full(max(size, 1), 7.0)
        st = lib.sph_render_density(ctx._h, C.byref(d), buf.ctypes.data, size)
        return st, buf

    st, buf = call()
    assert st == 0
    bad = [dict(shape=(0, 11, 12)), dict(out_len=10 * 12), dict(bounds=((5, -5, -2), (-5, 5, 2))), dict(h=-1.0),
           dict(axis=3), dict(axis=-2), dict(shape=(10, 11, 1)), dict(axis=None), dict(reserved=1),
           dict(clip=((100, 100, 100), (101, 101, 101)), bounds=None)]
    for b in bad:
        st, buf = call(**b)
        assert st == SPH_ERR_ARG, b
        assert np.all(buf == 7.0), b                   # nothing written
    d = ctx.render_desc(10, None, None, 1.25, None)
    assert lib.sph_render_density(ctx._h, C.byref(d), None, 1000) == SPH_ERR_ARG
    assert lib.sph_render_density(ctx._h, None, np.zeros(1000).ctypes.data, 1000) == SPH_ERR_ARG
    assert lib.sph_render_density(None, C.byref(d), np.zeros(1000).ctypes.data, 1000) == SPH_ERR_ARG
    assert lib.sph_render_density_dev(ctx._h, C.byref(d), None, 1000) == SPH_ERR_ARG
    # the context still steps
    dt, t = ctx.step(1e-2)
    assert dt > 0 and np.all(np.isfinite(ctx.field("x")))
    ctx.close()


def test_scale_1e6_per_particle_h_projection(capi):
    rows = ic.keplerian_disc_var(1_000_000, seed=99)
    ctx, gas, _ = _ctx(capi, rows, variable=True)
    ctx.density(); ctx.update_h()
    img = ctx.render_density((1024, 1024, 64), axis="z")
    lo, hi = ctx.render_bounds
    pos = np.stack([ctx.field(k) for k in "xyz"], axis=1)
    m, hv = ctx.field("m"), ctx.field("h")
    assert np.array_equal(lo, pos.min(axis=0)) and np.array_equal(hi, pos.max(axis=0))
    ax = render_ref.axes(lo, hi, (1024, 1024, 64))
    rng = np.random.default_rng(1)
    # columns inside the disc (non-zero) and a few anywhere
    nz = np.argwhere(img > 0)
    cols = np.vstack([nz[rng.choice(nz.shape[0], 224, replace=False)], rng.integers(0, 1024, (32, 2))])
    scale = img.max()
    for i, j in cols:
        gx, gy = ax[0][i], ax[1][j]
        near = (np.abs(pos[:, 0] - gx) <= 2 * hv * (1 + 1e-9)) & (np.abs(pos[:, 1] - gy) <= 2 * hv * (1 + 1e-9))
        nodes = np.stack([np.full(64, gx), np.full(64, gy), ax[2]], axis=1)
        ref = render_ref.brute(nodes, pos[near], m[near], hv[near]).sum() if near.any() else 0.0
        assert abs(img[i, j] - ref) <= TOL * scale, (i, j)
    ctx.close()
