"""GPU tests of sph_sample (include/summersph.h, "SPH interpolation at arbitrary points") on the MI355X: parity with the
numpy restatement (the fixtures, a uniform box, a variable-h disc; 0 .. 4 fields, context fields and values, both weights,
raw and normalised), the reference's imaging script, the render's own nodes, the order rule, smoothing lengths over more
than ten octaves, a constant field, ranks, a cull, no side effects on a running simulation, the errors, 10^6 particles x
10^6 points with a physical check, and the command line.

Bounds (tests/test_render_field_gpu.py holds the renders' same sums to them): num within 1e-12 of the row's largest
magnitude, den and normalised values within 1e-13 of theirs."""
import ctypes as C
import json
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gpu_support import capi, field_positions, golden_gas, make_context, over_defaults, ref_h
import render_field_ref
import sample_ref
from summersph_amd import ic, txtio
from summersph_amd import sample as smp

pytestmark = pytest.mark.gpu
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
TOL_NUM = 1e-12
TOL_DEN = 1e-13


def _ctx(capi, gas, sinks=None, variable=False, flags=0, density=True):
    return make_context(capi, gas, sinks, variable=variable, flags=over_defaults(capi, flags, variable), density=density)


def _close(got, want, tol, what=""):
    """every entry within tol of the row's largest magnitude; NaN where the restatement has NaN"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    for k in range(want.shape[0]):
        ok = np.isfinite(want[k])
        s = np.max(np.abs(want[k][ok])) if ok.any() else 0.0
        err = float(np.max(np.abs(got[k][ok] - want[k][ok]))) if ok.any() else 0.0
        print(f"    {what} row {k}: max err {err:.3e} scale {s:.3e} ratio {err / s if s > 0 else 0.0:.2e} (tol {tol:g})")
        assert err <= tol * s, (what, k, err, s)


def _points(pos, h, seed=5):
    """5000 uniform in the source box inflated by 10 %, the particles' own positions, a polar ring, and a handful more
    than 2 h_max outside the box (exact zeros)"""
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = hi - lo
    uni = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (5000, 3))
    ring, _ = smp.polar_points(0.2 * ext[0], 0.25 * ext[0], 1, 257, centre=0.5 * (lo + hi))
    reach = 2.0 * float(np.max(h))
    far = np.array([lo - 1.01 * reach, hi + 1.01 * reach, [lo[0] - 1.5 * reach, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])],
                    [0.5 * (lo[0] + hi[0]), hi[1] + 3.0 * reach, lo[2]], hi + 1e6 * ext])
    return np.concatenate([uni, pos, ring, far]), far.shape[0]


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
    pos, m, rho = field_positions(ctx), ctx.field("m"), ctx.field("rho")
    h = ref_h(ctx, capi)
    pts, n_far = _points(pos, h)
    rng = np.random.default_rng(3)
    vals = np.stack([rng.normal(size=n), pos[:, 0] * pos[:, 1]])
    names = ("vx", "vy", "u", "rho")
    A = np.concatenate([np.stack([ctx.field(f) for f in names]), vals])
    for weight in ("mass", "volume"):
        for normalise in (False, True):
            tol = TOL_DEN if normalise else TOL_NUM
            r_out, r_den, r_cnt = sample_ref.sample(pts, pos, m, h, A, rho if weight == "volume" else None, normalise=normalise)
            assert r_cnt[1] == 0 and r_cnt[0] <= pts.shape[0] - n_far
            kw = dict(weight=weight, normalise=normalise)
            tag = f"{name} {weight} {'norm' if normalise else 'raw'}"
            # the weight alone, then context fields, 1 .. 4 of them
            den, cnt = ctx.sample(pts, counts=True, **kw)[1:]
            assert cnt == r_cnt
            _close(den, r_den, TOL_DEN, tag + " den")
            assert np.all(den[-n_far:] == 0.0)
            for k in range(1, 5):
                out, den, cnt = ctx.sample(pts, fields=names[:k], weight_out=True, counts=True, **kw)
                assert cnt == r_cnt and out.shape == (k, pts.shape[0])
                _close(out, r_out[:k], tol, tag + f" K={k}")
                _close(den, r_den, TOL_DEN, tag + " den")
                assert np.all(out[:, -n_far:] == 0.0) and np.all(den[-n_far:] == 0.0)
            # values rows, and a mix with a context field
            out = ctx.sample(pts, fields=(capi.SAMPLE_VALUES, capi.SAMPLE_VALUES), values=vals, **kw)
            _close(out, r_out[4:6], tol, tag + " values")
            out = ctx.sample(pts, fields=("vx", capi.SAMPLE_VALUES), values=vals, **kw)
            _close(out, r_out[[0, 5]], tol, tag + " mix")
    ctx.close()


def test_against_the_imaging_script(capi):
    g = load_golden("render_script12k")
    n = g["script_x"].size
    gas = {"x": g["script_x"], "y": g["script_y"], "z": g["script_z"], "m": g["script_mass"], "vx": np.zeros(n), "vy": np.zeros(n),
           "vz": np.zeros(n), "u": np.full(n, 0.25), "alpha": np.zeros(n)}
    ctx = _ctx(capi, gas, density=False)
    b, res = g["bounds"], int(g["grid_resolution"])
    ax = [np.linspace(b[a], b[3 + a], res) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    t0 = time.perf_counter()
    den = ctx.sample(pts, h=float(g["h"]))
    print(f"script grid: {pts.shape[0]} points in {time.perf_counter() - t0:.3f} s (the script: {float(g['script_seconds']):.1f} s)")
    img, ref = den.reshape(res, res, res).sum(axis=2), g["projected_density"]
    err = float(np.max(np.abs(img - ref)))
    print(f"script image: max err {err:.3e} of max {ref.max():.3e}: {err / ref.max():.2e}")
    assert err <= 1e-12 * ref.max()
    assert np.all(img[ref == 0] == 0.0)
    ctx.close()


@pytest.mark.parametrize("variable", [False, True])
def test_against_the_render(capi, variable):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000, seed=8) if variable else ic.keplerian_disc(20000, seed=8))
    ctx = _ctx(capi, gas, sinks, variable=variable)
    shape, bounds = (48, 48, 16), ((-45.0, -40.0, -6.0), (40.0, 45.0, 5.0))
    ax = [np.linspace(bounds[0][a], bounds[1][a], shape[a]) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    for weight in ("mass", "volume"):
        img, wimg = ctx.render_field("vx", shape, bounds=bounds, weight=weight, weight_out=True)
        out, den = ctx.sample(pts, fields=("vx",), weight=weight, weight_out=True)
        assert np.count_nonzero(wimg) > 0.5 * wimg.size
        _close(out[0], img.ravel(), TOL_NUM, f"render {weight} num")
        _close(den, wimg.ravel(), TOL_DEN, f"render {weight} den")
        assert np.array_equal(den == 0.0, wimg.ravel() == 0.0)
    ctx.close()


# ---- order rule ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)


@pytest.mark.parametrize("variable", [False, True])
def test_order_rule_bitwise(capi, variable):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(40000, seed=15) if variable else ic.keplerian_disc(40000, seed=15))
    a = _ctx(capi, gas, sinks, variable=variable, density=False)
    pos = field_positions(a)
    pts, _ = _points(pos[::7], gas["h"] if variable else 2.5, seed=9)
    pts[11] = [np.nan, 0.0, 0.0]
    pts[12] = [0.0, np.inf, 0.0]
    kw = {"fields": ("vx", "vy", "vz", "u"), "weight_out": True, "counts": True}
    h0 = a.field("h") if variable else None
    r0 = a.sample(pts, **kw)
    assert r0[2][1] == 2 and np.all(np.isnan(r0[0][:, 11:13])) and np.all(np.isnan(r0[1][11:13]))
    _same(r0[:2], a.sample(pts, **kw)[:2])                          # repeated
    perm = np.random.default_rng(4).permutation(pts.shape[0])
    rp = a.sample(pts[perm], **kw)                                 # any order of the points
    assert np.array_equal(rp[0], r0[0][:, perm], equal_nan=True) and np.array_equal(rp[1], r0[1][perm], equal_nan=True)
    assert rp[2] == r0[2]
    sub = np.sort(np.random.default_rng(5).choice(pts.shape[0], 1234, replace=False))
    rs = a.sample(pts[sub], **kw)                                  # a subset
    assert np.array_equal(rs[0], r0[0][:, sub], equal_nan=True) and np.array_equal(rs[1], r0[1][sub], equal_nan=True)
    for i in (0, 4999, 5003, pts.shape[0] - 1):                    # one point alone
        r1 = a.sample(pts[i:i + 1], **kw)
        assert np.array_equal(r1[0][:, 0], r0[0][:, i]) and r1[1][0] == r0[1][i]
    # the three-array form and the device form against the host form
    _same(r0[:2], a.sample((pts[:, 0], pts[:, 1], pts[:, 2]), **kw)[:2])
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(pts).to(dev)
    rd = a.sample(dp, device=True, **kw)
    assert isinstance(rd[0], torch.Tensor) and rd[2] == r0[2]
    _same(r0[:2], (rd[0].cpu().numpy(), rd[1].cpu().numpy()))
    vals = np.random.default_rng(2).normal(size=(2, a.n))
    hv = a.sample(pts, fields=("u", capi.SAMPLE_VALUES), values=vals, normalise=True)
    dv = a.sample([dp[:, k].contiguous() for k in range(3)], fields=("u", capi.SAMPLE_VALUES),
                  values=torch.from_numpy(vals).to(dev), normalise=True, device=True)
    assert np.array_equal(hv, dv.cpu().numpy(), equal_nan=True)
    a.density()                                                    # re-sorted slots
    if variable:
        a.upload_field("h", h0)                                    # the density pass iterated h: the uploaded one again
    _same(r0[:2], a.sample(pts, **kw)[:2])
    c = _ctx(capi, gas, sinks, variable=variable, flags=capi.FLAG_HASHED_GRID)
    assert c.grid_info().kind == 1
    if variable:
        c.upload_field("h", h0)
    _same(r0[:2], c.sample(pts, **kw)[:2])
    c.close()
    a.close()


def test_smoothing_lengths_over_ten_octaves(capi):
    gas, sinks = ic.split_rows(ic.uniform_box(5000))
    n = gas["x"].size
    rng = np.random.default_rng(23)
    edge = float(max(gas[k].max() - gas[k].min() for k in "xyz"))
    gas["h"] = 0.5 * edge * 2.0 ** rng.uniform(-11.0, 0.0, n)      # log-uniform over 11 octaves up to half the box edge
    gas["h"][77] = 1.01 * edge                                     # 2 h > the box diagonal: reaches every point
    ctx = _ctx(capi, gas, sinks, variable=True, density=False)
    h = ctx.field("h")
    assert np.array_equal(h, gas["h"]) and np.log2(h.max() / h.min()) >= 10.0
    pos, m = field_positions(ctx), ctx.field("m")
    pts = np.concatenate([rng.uniform(pos.min(axis=0) - 2.0, pos.max(axis=0) + 2.0, (2000, 3)), pos[:1000]])
    vals = np.stack([np.sin(pos[:, 0]), pos[:, 1] - pos[:, 2]])
    levels = np.unique(h.view(np.uint64) >> np.uint64(51)).size    # occupied half octaves
    ctx.sample(pts[:10])                                           # warm-up (scratch, code objects)
    t0 = time.perf_counter()
    out, den, cnt = ctx.sample(pts, fields=(capi.SAMPLE_VALUES,) * 2, values=vals, weight_out=True, counts=True)
    dt = time.perf_counter() - t0
    print(f"wide h: {levels} occupied half-octave levels, {pts.shape[0]} points in {dt * 1e3:.2f} ms")
    assert cnt == (pts.shape[0], 0)
    for k in range(2):
        rn, rd = render_field_ref.brute(pts, pos, m, vals[k], h)
        _close(out[k], rn, TOL_NUM, f"wide h num {k}")
    _close(den, rd, TOL_DEN, "wide h den")
    outn = ctx.sample(pts, fields=(capi.SAMPLE_VALUES,) * 2, values=vals, normalise=True)
    for k in range(2):
        rn, rd = render_field_ref.brute(pts, pos, m, vals[k], h)
        _close(outn[k], render_field_ref.ratio(rn, rd), TOL_DEN, f"wide h normalised {k}")
    ctx.close()


@pytest.mark.parametrize("variable", [False, True])
def test_constant_field(capi, variable):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000, seed=6) if variable else ic.keplerian_disc(20000, seed=6))
    ctx = _ctx(capi, gas, sinks, variable=variable)
    pts, n_far = _points(field_positions(ctx), ref_h(ctx, capi))
    for weight in ("mass", "volume"):
        out, den = ctx.sample(pts, fields=(capi.SAMPLE_VALUES,), values=np.full(ctx.n, 3.0), weight=weight, normalise=True,
                              weight_out=True)
        hit = den != 0
        assert hit.sum() > 20000 and not hit[-n_far:].any()
        assert np.max(np.abs(out[0][hit] - 3.0)) <= 1e-13 * 3.0
        assert np.all(out[0][~hit] == 0.0)
    ctx.close()


def test_ranks_add_up(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(30000, seed=17))
    n = gas["x"].size
    one = _ctx(capi, gas, sinks, variable=True, density=False)
    pts, _ = _points(field_positions(one), gas["h"])
    kw = {"fields": ("vx", "u"), "weight_out": True, "counts": True}
    o1, d1, c1 = one.sample(pts, **kw)
    one.close()
    half = n // 2
    num, den = np.zeros_like(o1), np.zeros_like(d1)
    for first in (True, False):
        ids = np.arange(n) if first else np.concatenate([np.arange(half, n), np.arange(half)])
        ctx = _ctx(capi, {k: v[ids] for k, v in gas.items()}, sinks, variable=True, density=False)
        ctx.set_owned(half if first else n - half)
        o, d, c = ctx.sample(pts, **kw)
        # the ghosts are no sources: the restatement over the owned half alone
        sub = {k: v[ids] for k, v in gas.items()}
        rp = np.stack([sub["x"], sub["y"], sub["z"]], axis=1)
        ro, rd, rc = sample_ref.sample(pts, rp, sub["m"], sub["h"], np.stack([sub["vx"], sub["u"]]), n_owned=half if first else n - half)
        assert c == rc
        _close(o, ro, TOL_NUM, "rank num")
        _close(d, rd, TOL_DEN, "rank den")
        assert c[0] < c1[0]
        num += o
        den += d
        ctx.close()
    _close(num, o1, TOL_NUM, "ranks num")
    _close(den, d1, TOL_DEN, "ranks den")


def test_after_accrete_and_cull(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=12))
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])
    ctx = _ctx(capi, gas, sinks)
    ctx.forces()
    assert ctx.accrete_and_cull() > 0 and ctx.n < 20000
    pos = field_positions(ctx)
    vals = np.stack([pos[:, 0] + 2.0 * pos[:, 1], np.arange(ctx.n, dtype=np.float64)])
    pts, _ = _points(pos, 2.5)
    out, den, cnt = ctx.sample(pts, fields=(capi.SAMPLE_VALUES, capi.SAMPLE_VALUES, "rho"), values=vals, weight_out=True, counts=True)
    r_out, r_den, r_cnt = sample_ref.sample(pts, pos, ctx.field("m"), 2.5, np.concatenate([vals, ctx.field("rho")[None]]))
    assert cnt == r_cnt
    _close(out, r_out, TOL_NUM, "cull num")
    _close(den, r_den, TOL_DEN, "cull den")
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    pts, _ = smp.polar_points(12.0, 60.0, 40, 64)
    runs = []
    for with_sample in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_sample:
                before = {k: ctx.field(k) for k in ("x", "vx", "rho", "ax", "du")}
                ctx.sample(pts, fields=("vx", "vy", "rho", "u"), weight="volume", weight_out=True)
                ctx.sample(pts, fields=("u",), normalise=True, h=1.0, clip=((0, 0, -1), (50, 50, 1)))
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


def test_errors(capi):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc(3000, seed=37))
    ctx = _ctx(capi, gas, sinks, density=False)
    lib = ctx.lib
    n, m = ctx.n, 50
    pts = np.ascontiguousarray(np.random.default_rng(1).uniform(-20, 20, (3, m)))
    out = np.full(4 * m, 7.0)
    w = np.full(m, 7.0)
    vals = np.zeros((4, n))
    cnt = (C.c_int64 * 2)(7, 7)

    def call(d, values=None, n_out=None, o=out, wt=w, mm=m, p=(0, 1, 2), ctxh=None):
        nf = d.n_fields if d is not None else 1
        ptr = [None if k is None else pts[k].ctypes.data for k in p]
        return lib.sph_sample(ctx._h if ctxh is None else ctxh, None if d is None else C.byref(d), mm, *ptr,
                              None if values is None else values.ctypes.data, None if o is None else o.ctypes.data,
                              nf * mm if n_out is None else n_out, None if wt is None else wt.ctypes.data, cnt)

    def untouched():
        return np.all(out == 7.0) and np.all(w == 7.0) and tuple(cnt) == (7, 7)

    def is_arg(st):
        return st == SPH_ERR_ARG and untouched() and b"sph_sample" in lib.sph_last_error(ctx._h)

    D = capi.sample_desc
    for f in ("rho", "ax", "h"):                                   # rho stale, rates stale, no h field on a fixed-h context
        assert call(D((f,))) == SPH_ERR_STATE and untouched() and b"sph_sample" in lib.sph_last_error(ctx._h)
    assert call(D(("u",), weight="volume")) == SPH_ERR_STATE and untouched()     # the volume weight needs rho
    assert is_arg(call(None))
    assert is_arg(call(D(("u",)), p=(0, None, 2)))
    assert is_arg(call(D(("u",)), mm=-1, n_out=m))
    assert is_arg(call(D(("u",)), mm=2 ** 31, n_out=2 ** 31))
    for k in (-1, 5):
        d = D(("u",)); d.n_fields = k
        assert is_arg(call(d, n_out=max(k, 0) * m)), k
    for bad in (-2, 19, 100):
        d = D(("u", "vx")); d.fields[1] = bad
        assert is_arg(call(d)), bad
    assert is_arg(call(D((capi.SAMPLE_VALUES,))))                   # values missing
    assert is_arg(call(D(("u",)), values=vals))                     # values given, none asked for
    assert is_arg(call(D(("u", "vx")), n_out=2 * m - 1))
    assert is_arg(call(D(("u",)), o=None))
    assert is_arg(call(D(()), wt=None))
    d = D(("u",)); d.weight = 2
    assert is_arg(call(d))
    for bad in (2, 4, -1):
        d = D(("u",)); d.flags = bad
        assert is_arg(call(d)), bad
    d = D(("u",)); d.reserved = 1
    assert is_arg(call(d))
    for bad in (-1.0, np.nan):
        assert is_arg(call(D(("u",), h=bad))), bad
    assert is_arg(call(D(("u",), clip=((np.nan, 0, 0), (1, 1, 1)))))
    assert is_arg(call(D(("u",), clip=((0, 0, 0), (1, 1, np.nan)))))
    assert lib.sph_sample(None, C.byref(D(("u",))), m, *(pts[k].ctypes.data for k in range(3)), None, out.ctypes.data, m,
                          None, None) == SPH_ERR_ARG
    # the good calls: n_points == 0 writes no row; optional outputs may be null
    assert call(D(("u",)), mm=0, p=(None, None, None)) == 0 and np.all(out == 7.0) and tuple(cnt) == (0, 0)
    assert call(D(("u",)), wt=None) == 0 and np.all(out[:m] != 7.0) and np.all(out[m:] == 7.0) and cnt[0] > 0
    assert call(D((capi.SAMPLE_VALUES,)), values=vals) == 0
    assert call(D(()), o=None) == 0 and np.all(w != 7.0)
    ctx.density()
    assert call(D(("rho", "P", "c"), weight="volume")) == 0
    # an empty source set: zeros, not an error
    o, dn, c = ctx.sample(pts.T, fields=("u",), clip=((1e9,) * 3, (2e9,) * 3), weight_out=True, counts=True, normalise=True)
    assert c == (0, 0) and np.all(o == 0.0) and np.all(dn == 0.0)
    # (params.h <= 0 on a fixed-h context cannot be reached through sph_ctx_create, which refuses such parameters)
    ctx.close()
    # a bad source h (variable h): SPH_ERR_STATE in the host form, d_counts[0] == -1 and NaN outputs in the device form
    gv, sv = ic.split_rows(ic.keplerian_disc_var(3000, seed=38))
    v = _ctx(capi, gv, sv, variable=True, density=False)
    for bad in (-1.0, 0.0, np.inf, np.nan):
        h = gv["h"].copy()
        h[17] = bad
        v.upload_field("h", h)
        with pytest.raises(capi.SphError) as e:
            v.sample(pts.T, fields=("u",))
        assert e.value.status == SPH_ERR_STATE and "sph_sample" in str(e.value)
        dp = torch.from_numpy(np.ascontiguousarray(pts.T)).to(torch.device("cuda", 0))
        do, dw, dc = v.sample(dp, fields=("u", "vx"), weight_out=True, counts=True, device=True)
        assert dc[0] == -1 and bool(do.isnan().all()) and bool(dw.isnan().all())
        x17 = v.field("x")[17]
        assert v.sample(pts.T, counts=True, clip=((x17 + 1e-9, -np.inf, -np.inf), (np.inf,) * 3))[2][0] >= 0     # 17 outside: fine
        assert v.sample(pts.T, counts=True, h=2.0)[2][0] > 0
    v.close()


def _smoothed_midplane_density(sigma, h, H):
    """Sigma * int W(r, h) N(z; 0, H) d^3r by quadrature: the kernel-smoothed midplane density of a disc of uniform
    surface density Sigma and Gaussian scale height H"""
    q = np.linspace(0.0, 2.0, 4001)
    w = np.where(q <= 1.0, 1 - 1.5 * q ** 2 + 0.75 * q ** 3, 0.25 * (2 - q) ** 3) / (np.pi * h ** 3)
    r = q * h
    # shells: int W(r) 4 pi r^2 <N(z)>_shell dr, <N>_shell = (1 / 2r) int_-r^r N(z) dz = erf(r / (sqrt(2) H)) / (2 r)
    from math import erf
    shell = np.array([erf(x / (np.sqrt(2.0) * H)) / (2.0 * x) if x > 0 else 1.0 / (np.sqrt(2.0 * np.pi) * H) for x in r])
    f = w * 4.0 * np.pi * r ** 2 * shell
    return sigma * float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(r)))


def test_million_particles_million_points(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(1_000_000, seed=5))
    ctx = _ctx(capi, gas, sinks, density=False)
    pos, m = field_positions(ctx), ctx.field("m")
    R = np.hypot(pos[:, 0], pos[:, 1])
    r_in, r_out = 10.0, float(R.max())
    polar, shape = smp.polar_points(30.0, r_out - 30.0, 512, 2048)
    rng = np.random.default_rng(19)
    pts = np.concatenate([polar, rng.uniform(pos.min(axis=0), pos.max(axis=0), (50000, 3))])
    assert pts.shape[0] >= 1_000_000
    ctx.sample(pts[:1000], fields=("u",))                          # warm-up
    t0 = time.perf_counter()
    out, den, cnt = ctx.sample(pts, fields=("vx", "vy"), weight_out=True, counts=True)
    dt = time.perf_counter() - t0
    print(f"10^6 particles x {pts.shape[0]} points, 2 fields: host form {dt:.3f} s; {cnt[0]} points reached")
    ids = np.sort(rng.choice(pts.shape[0], 2000, replace=False))
    r_out2, r_den, _ = sample_ref.sample(pts[ids], pos, m, 2.5, np.stack([ctx.field("vx"), ctx.field("vy")]))
    _close(out[:, ids], r_out2, TOL_NUM, "10^6 num")
    _close(den[ids], r_den, TOL_DEN, "10^6 den")
    # the map's mean density against the analytic midplane value of this disc smoothed by the kernel
    sigma = m.sum() / (np.pi * (r_out ** 2 - r_in ** 2))
    want = _smoothed_midplane_density(sigma, 2.5, float(pos[:, 2].std()))
    rings = den[:polar.shape[0]].reshape(shape).mean(axis=1) / want
    print("ring means / analytic:", np.array2string(rings[::32], precision=3), f"map mean {rings.mean():.4f}")
    assert abs(rings.mean() - 1.0) <= 0.03
    ctx.close()


def test_cli_matches_context_sample(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    my = np.random.default_rng(8).uniform(-30, 30, (7, 11, 3))
    np.save(tmp_path / "pts.npy", my)
    cases = [(["--polar", "12", "40", "16", "32"], smp.polar_points(12.0, 40.0, 16, 32)),
             (["--points", str(tmp_path / "pts.npy")], (my.reshape(-1, 3), (7, 11)))]
    for k, (args, (pts, shape)) in enumerate(cases):
        out = tmp_path / f"s{k}.npz"
        r = subprocess.run([sys.executable, "-m", "summersph_amd.sample", str(save), "-o", str(out), "--fields", "rho,u,vy",
                            "--normalise", "--json"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        z = np.load(out)
        o, den, cnt = ctx.sample(pts, fields=("rho", "u", "vy"), normalise=True, weight_out=True, counts=True)
        assert np.array_equal(z["points"], pts) and tuple(z["shape"]) == tuple(shape)
        for i, f in enumerate(("rho", "u", "vy")):
            assert np.array_equal(z[f], o[i], equal_nan=True), f
        assert np.array_equal(z["weight"], den, equal_nan=True)
        assert (int(z["n_hit"]), int(z["n_nonfinite"])) == cnt and int(z["desc_flags"]) == capi.SAMPLE_NORMALISE
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["n_hit"] == cnt[0] and j["n_points"] == pts.shape[0]
    ctx.close()
