"""GPU tests of sph_trace (include/summersph.h, "field lines of an SPH-interpolated vector field") on the MI355X: bitwise
equality with a numpy RK4 whose stage velocities are Context.sample calls (the test that pins the arithmetic), parity with
the numpy restatement, the order rule, stride, the stops, a constant field, no side effects on a running simulation, the
errors and the command line.

Bounds: the composition is bitwise; against the restatement status and n_done are equal for every seed (tests/
test_trace_cpu.py::test_seed_set_is_decisive holds the condition) and the path is within 1e-12 of the largest finite
coordinate (tests/test_sample_gpu.py's TOL_NUM); a constant field is followed to 1e-13 n_steps of the largest coordinate."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gpu_support import capi, make_context, over_defaults, positions
import trace_ref
from summersph_amd import ic, txtio
from summersph_amd import trace as trc

pytestmark = pytest.mark.gpu
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
TOL_NUM = 1e-12


def _ctx(capi, gas, sinks=None, variable=False, flags=0, density=True):
    return make_context(capi, gas, sinks, variable=variable, flags=over_defaults(capi, flags, variable), density=density)


def _golden(capi, name, density=True):
    gas, sinks = ic.split_rows(load_golden(name)["ic"])
    return _ctx(capi, gas, sinks, variable="discv" in name, density=density), gas, sinks


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def _sampler(ctx, fields, values=None, carry=None, **kw):
    """Context.sample as trace_ref's sampler: the normalised values of the three components (and the carry) and den"""
    f = tuple(fields) + (() if carry is None else (carry,))

    def s(q):
        return ctx.sample(q, fields=f, values=values, normalise=True, weight_out=True, **kw)
    return s


@pytest.mark.parametrize("name", ["disc3000_eval", "discv3000_eval", "bin2000_eval"])
def test_bitwise_against_the_composition(capi, name):
    ctx, gas, sinks = _golden(capi, name)
    pos = positions(gas)
    n = ctx.n
    h = gas["h"] if "h" in gas else float(ctx.params.h)
    seeds = trace_ref.parity_seeds(pos, h, 11, n=257, n_far=16)
    seeds[200] = [np.nan, 1.0, 1.0]
    if len(sinks["x"]) > 1:
        omega, centre = trc.sink_frame(sinks, 1)
    else:
        omega, centre = (0.001, -0.002, 0.01), (0.5, -0.25, 0.125)
    g = np.nan_to_num(ctx.gradients(("vx", "vy", "vz"), corrected=False)[0])
    curl = np.stack([g[2][1] - g[1][2], g[0][2] - g[2][0], g[1][0] - g[0][1]])         # the vorticity at the particles
    vals = np.concatenate([curl, np.random.default_rng(3).normal(size=(1, n))])
    V = capi.TRACE_VALUES
    cases = [
        dict(ds=1.5),
        dict(ds=0.75, arclength=True),
        dict(ds=-1.5, omega=omega, centre=centre, normal=(0.1, -0.2, 1.0), carry="rho", weight="volume"),
        dict(ds=-0.75, arclength=True, omega=omega, centre=centre, normal=(0.0, 0.0, 2.0), carry="u", h=3.0,
             clip=((-30.0, -30.0, -np.inf), (30.0, 35.0, np.inf))),
        dict(ds=0.5, arclength=True, fields=(V, V, V), values=vals, carry=V),
        dict(ds=20.0, fields=("vx", V, "vz"), values=vals, carry="vy", box=((-35.0, -35.0, -5.0), (35.0, 35.0, 5.0))),
    ]
    for kw in cases:
        ds = kw.pop("ds")
        got = ctx.trace(seeds, 3, ds, counts=True, **kw)
        skw = {k: kw[k] for k in ("weight", "h", "clip") if k in kw}
        tkw = {k: kw[k] for k in ("arclength", "omega", "centre", "normal", "box") if k in kw}
        sampler = _sampler(ctx, kw.get("fields", ("vx", "vy", "vz")), kw.get("values"), kw.get("carry"), **skw)
        want = trace_ref.trace_with(sampler, seeds, 3, ds, carry="carry" in kw, **tkw)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), kw
        assert np.array_equal(got[0], want[0], equal_nan=True), kw
        if "carry" in kw:
            assert np.array_equal(got[3], want[3], equal_nan=True), kw
        assert got[-1] == tuple(np.bincount(want[1], minlength=5)) and got[1][200] == capi.TRACE_NONFINITE
        if "box" in kw:
            assert np.count_nonzero(want[1] == capi.TRACE_LEFT_BOX) >= 16 and np.count_nonzero(want[1] == capi.TRACE_DONE) >= 1, kw
        else:
            assert np.count_nonzero(want[1] == capi.TRACE_DONE) >= 150, kw     # most lines run all their steps
    ctx.close()


@pytest.mark.parametrize("case", trace_ref.PARITY_CASES, ids=lambda c: f"{c[0]}-h{c[1]}-{'arc' if c[2] else 'time'}")
def test_parity_with_the_restatement(capi, case):
    name, h, arclength, ds, gen_seed = case
    ctx, gas, _ = _golden(capi, name, density=False)
    seeds, (r_path, r_status, r_done) = trace_ref.parity_case(gas, h, arclength, ds, gen_seed)
    path, status, done = ctx.trace(seeds, trace_ref.PARITY_STEPS, ds, arclength=arclength, h=h)
    print(f"    {name} h {h} arclength {arclength}: status counts {np.bincount(status, minlength=5)} "
          f"(restatement {np.bincount(r_status, minlength=5)})")
    assert np.array_equal(status, r_status) and np.array_equal(done, r_done)          # every seed, none excluded
    assert np.array_equal(np.isnan(path), np.isnan(r_path))
    scale = np.nanmax(np.abs(r_path))
    err = np.nanmax(np.abs(path - r_path))
    print(f"    path: max err {err:.3e} scale {scale:.3e} ratio {err / scale:.2e} (tol {TOL_NUM:g})")
    assert err <= TOL_NUM * scale
    ctx.close()


@pytest.mark.parametrize("variable", [False, True])
def test_order_rule_bitwise(capi, variable):
    import torch
    name = "discv3000_eval" if variable else "disc3000_eval"
    a, gas, sinks = _golden(capi, name, density=False)
    h0 = gas["h"] if variable else 2.5
    seeds = trace_ref.parity_seeds(positions(gas), h0, 21, n=65, n_far=6)
    seeds[7] = [0.0, np.inf, 0.0]
    kw = dict(arclength=True, carry="u", omega=(0.0, 0.0, 0.004), normal=(0.0, 0.1, 1.0), stride=2, counts=True)
    r0 = a.trace(seeds, 8, 0.6, **kw)
    assert r0[1][7] == capi.TRACE_NONFINITE and sum(r0[4]) == 65 and r0[4][capi.TRACE_DONE] >= 40
    r1 = a.trace(seeds, 8, 0.6, **kw)                               # two calls in a row
    _same(r0[:4], r1[:4])
    assert r0[4] == r1[4]
    rr = a.trace(seeds[::-1], 8, 0.6, **kw)                         # the seeds reversed
    _same([r0[0][:, :, ::-1], r0[1][::-1], r0[2][::-1], r0[3][:, ::-1]], rr[:4])
    assert rr[4] == r0[4]
    sub = np.sort(np.random.default_rng(5).choice(65, 23, replace=False))
    rs = a.trace(seeds[sub], 8, 0.6, **kw)                          # a subset
    _same([r0[0][:, :, sub], r0[1][sub], r0[2][sub], r0[3][:, sub]], rs[:4])
    for i in (0, 7, 33, 64):                                        # one seed alone (M = 1)
        r = a.trace(seeds[i:i + 1], 8, 0.6, **kw)
        _same([r0[0][:, :, i:i + 1], r0[1][i:i + 1], r0[2][i:i + 1], r0[3][:, i:i + 1]], r[:4])
    r64 = a.trace(seeds[:64], 8, 0.6, **kw)                         # a full wavefront, and one lane more above
    _same([r0[0][:, :, :64], r0[1][:64], r0[2][:64], r0[3][:, :64]], r64[:4])
    _same(r0[:4], a.trace((seeds[:, 0], seeds[:, 1], seeds[:, 2]), 8, 0.6, **kw)[:4])
    dev = torch.device("cuda", 0)                                   # the device form
    rd = a.trace(torch.from_numpy(seeds).to(dev), 8, 0.6, device=True, **kw)
    assert isinstance(rd[0], torch.Tensor) and rd[1].dtype == torch.int32 and rd[4] == r0[4]
    _same(r0[:4], [t.cpu().numpy() for t in rd[:4]])
    a.density()                                                     # re-sorted slots
    if variable:
        a.upload_field("h", h0)                                     # the density pass iterated h: the uploaded one again
    _same(r0[:4], a.trace(seeds, 8, 0.6, **kw)[:4])
    c = _ctx(capi, gas, sinks, variable=variable, flags=capi.FLAG_HASHED_GRID)
    assert c.grid_info().kind == 1
    if variable:
        c.upload_field("h", h0)
    _same(r0[:4], c.trace(seeds, 8, 0.6, **kw)[:4])
    c.close()
    a.close()


def test_stride(capi):
    ctx, gas, _ = _golden(capi, "discv3000_eval", density=False)
    seeds = trace_ref.parity_seeds(positions(gas), gas["h"], 31, n=100, n_far=10)
    kw = dict(carry="u", box=((-30.0, -30.0, -6.0), (30.0, 30.0, 6.0)))
    full = ctx.trace(seeds, 12, 8.0, **kw)
    assert len(set(full[2].tolist())) > 3                            # lines that stop at different vertices
    for stride in (4, 12, 3):
        part = ctx.trace(seeds, 12, 8.0, stride=stride, **kw)
        assert part[0].shape == (12 // stride + 1, 3, 100)
        _same([full[0][::stride], full[1], full[2], full[3][::stride]], part)
    ctx.close()


def test_stops(capi):
    ctx, gas, _ = _golden(capi, "disc3000_eval", density=False)
    pos, n = positions(gas), ctx.n
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    mid = 0.5 * (lo + hi)
    h = float(ctx.params.h)
    reach, edge = 2.0 * h, 2.0 * h * (1.0 + 1e-6)
    inner = pos[np.argsort(np.abs(np.hypot(pos[:, 0], pos[:, 1]) - 20.0))[:40]]      # 40 particles' places: inside the gas
    far = np.array([lo - 3.0 * reach, hi + 3.0 * reach, [hi[0] + 2.5 * edge, mid[1], mid[2]], [mid[0], lo[1] - 40.0 * edge, mid[2]]])
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, -np.inf, 0.0]])
    seeds = np.concatenate([far, bad, inner])
    M = seeds.shape[0]
    path, status, done, car, cnt = ctx.trace(seeds, 6, 0.5, arclength=True, carry="u", counts=True)
    assert np.all(status[:4] == capi.TRACE_LEFT_GAS) and np.all(done[:4] == 0)
    assert np.array_equal(path[0, :, :4], far.T) and np.all(np.isnan(path[1:, :, :4]))
    assert np.all(car[0, :4] == 0.0) and np.all(np.isnan(car[1:, :4]))
    assert np.all(status[4:6] == capi.TRACE_NONFINITE) and np.all(done[4:6] == 0)
    assert np.all(np.isnan(path[:, :, 4:6])) and np.all(np.isnan(car[:, 4:6]))
    assert np.all(status[6:] == capi.TRACE_DONE) and np.all(done[6:] == 6) and np.all(np.isfinite(path[:, :, 6:]))
    assert np.all(car[:, 6:] > 0.0)
    assert sum(cnt) == M and cnt == tuple(np.bincount(status, minlength=5))
    # a tight box: the crossing vertex is recorded, later rows are NaN; a seed outside it stops at once
    s0 = inner[0]
    box = (s0 - 0.4, s0 + 0.4)
    two = np.stack([s0, s0 + [0.0, 0.4, 0.0]])                       # the second sits on the box's face: not strictly inside
    path, status, done, car, cnt = ctx.trace(two, 6, 0.5, arclength=True, carry="u", box=box, counts=True)
    assert list(status) == [capi.TRACE_LEFT_BOX] * 2 and cnt == (0, 0, 2, 0, 0)
    k = int(done[0])
    assert 1 <= k <= 2 and done[1] == 0
    inside = np.all((path[:, :, 0] > box[0]) & (path[:, :, 0] < box[1]), axis=1)
    assert np.all(inside[:k]) and np.all(np.isfinite(path[k, :, 0])) and not inside[k] and np.all(np.isnan(path[k + 1:, :, 0]))
    assert np.all(car[:k + 1, 0] > 0.0) and np.all(np.isnan(car[k + 1:, 0]))
    assert np.array_equal(path[0, :, 1], two[1]) and np.all(np.isnan(path[1:, :, 1])) and car[0, 1] > 0.0
    # a field of exact zeros: STAGNANT with ARCLENGTH, a line that stays on its seed bitwise in time mode
    V, zeros = capi.TRACE_VALUES, np.zeros((3, n))
    path, status, done = ctx.trace(seeds, 6, 0.5, arclength=True, fields=(V, V, V), values=zeros)
    assert np.all(status[6:] == capi.TRACE_STAGNANT) and np.all(done[6:] == 0) and np.all(status[:4] == capi.TRACE_LEFT_GAS)
    assert np.array_equal(path[0, :, 6:], inner.T) and np.all(np.isnan(path[1:, :, 6:]))
    path, status, done = ctx.trace(seeds, 6, 0.5, fields=(V, V, V), values=zeros)
    assert np.all(status[6:] == capi.TRACE_DONE) and np.all(done[6:] == 6)
    assert np.all(path[:, :, 6:] == inner.T[None])
    # an empty source set: every finite seed leaves the gas at once
    path, status, done, cnt = ctx.trace(seeds, 6, 0.5, clip=((1e9,) * 3, (2e9,) * 3), counts=True)
    assert np.all(np.delete(status, [4, 5]) == capi.TRACE_LEFT_GAS) and np.all(done == 0) and cnt == (0, M - 2, 0, 0, 2)
    ok = np.isfinite(seeds).all(axis=1)
    assert np.array_equal(path[0][:, ok], seeds[ok].T) and np.all(np.isnan(path[0][:, ~ok])) and np.all(np.isnan(path[1:]))
    ctx.close()


@pytest.mark.parametrize("variable", [False, True])
def test_constant_field(capi, variable):
    """independent of the restatement: in a constant field c every RK4 step adds ds c, with ARCLENGTH ds c / |c|"""
    ctx, gas, _ = _golden(capi, "discv3000_eval" if variable else "disc3000_eval", density=False)
    pos, n, S, ds = positions(gas), ctx.n, 16, 0.25
    seeds = pos[::30] + 0.1
    cvec = np.array([0.3, -0.2, 0.1])
    V = capi.TRACE_VALUES
    vals = np.repeat(cvec[:, None], n, axis=1)
    for arclength in (False, True):
        path, status, done = ctx.trace(seeds, S, ds, arclength=arclength, fields=(V, V, V), values=vals)
        fin = status == capi.TRACE_DONE
        assert fin.sum() >= 80 and np.all(done[fin] == S) and np.all((status == capi.TRACE_DONE) | (status == capi.TRACE_LEFT_GAS))
        scale = np.max(np.abs(path[:, :, fin]))
        tol = 1e-13 * S * scale
        step = cvec / np.linalg.norm(cvec) if arclength else cvec
        want = seeds.T[None, :, :] + (np.arange(S + 1) * ds)[:, None, None] * step[None, :, None]
        err = np.max(np.abs(path[:, :, fin] - want[:, :, fin]))
        print(f"    variable {variable} arclength {arclength}: {fin.sum()} lines, max err {err:.3e} (tol {tol:.3e})")
        assert err <= tol
        if arclength:
            seg = np.sqrt((np.diff(path[:, :, fin], axis=0) ** 2).sum(axis=1))
            assert np.max(np.abs(seg - abs(ds))) <= tol
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    seeds, _ = trc.ring_seeds(25.0, 64)
    runs = []
    for with_trace in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_trace:
                before = {k: ctx.field(k) for k in ("x", "vx", "rho", "ax", "du")}
                ctx.trace(seeds, 8, 0.5, arclength=True, carry="rho", weight="volume", omega=(0.0, 0.0, 0.01))
                ctx.trace(seeds, 4, -2.0, fields=("ax", "ay", "az"), h=1.0, clip=((0, 0, -1), (50, 50, 1)), stride=2)
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
    path = np.full(3 * 9 * m, 7.0)
    car = np.full(9 * m, 7.0)
    status = np.full(m, 77, dtype=np.int32)
    done = np.full(m, 77, dtype=np.int32)
    vals = np.zeros((4, n))
    cnt = (C.c_int64 * 5)(7, 7, 7, 7, 7)
    DEF = object()

    def call(d, values=None, n_path=None, pa=path, ca=None, st=status, nd=done, mm=m, p=(0, 1, 2), ctxh=None):
        ptr = [None if k is None else pts[k].ctypes.data for k in p]
        if n_path is None:
            n_path = 3 * (d.n_steps // max(d.stride, 1) + 1) * mm if d is not None else 0
        if ca is DEF:
            ca = car
        return lib.sph_trace(ctx._h if ctxh is None else ctxh, None if d is None else C.byref(d), mm, *ptr,
                             None if values is None else values.ctypes.data, None if pa is None else pa.ctypes.data, n_path,
                             None if ca is None else ca.ctypes.data, None if st is None else st.ctypes.data,
                             None if nd is None else nd.ctypes.data, cnt)

    def untouched():
        return (np.all(path == 7.0) and np.all(car == 7.0) and np.all(status == 77) and np.all(done == 77)
                and tuple(cnt) == (7,) * 5)

    def is_arg(st):
        return st == SPH_ERR_ARG and untouched() and b"sph_trace" in lib.sph_last_error(ctx._h)

    def D(n_steps=8, ds=0.5, **kw):
        return capi.trace_desc(n_steps, ds, **kw)

    def mod(**attrs):
        d = D()
        for k, v in attrs.items():
            setattr(d, k, v)
        return d
    V = capi.TRACE_VALUES
    # stale fields: rho and the rates before sph_density / sph_forces, no h field on a fixed-h context, rho for the weight
    for f in ("rho", "ax", "h"):
        assert call(D(fields=("vx", f, "vz"))) == SPH_ERR_STATE and untouched() and b"sph_trace" in lib.sph_last_error(ctx._h)
        assert call(D(carry=f), ca=DEF) == SPH_ERR_STATE and untouched()
    assert call(D(weight="volume")) == SPH_ERR_STATE and untouched()
    assert is_arg(call(None))
    assert is_arg(call(D(), p=(0, None, 2)))
    assert is_arg(call(D(), mm=-1, n_path=27 * m))
    assert is_arg(call(D(), mm=2 ** 31, n_path=27 * 2 ** 31))
    for bad in (0.0, np.nan, np.inf, -np.inf):
        assert is_arg(call(D(ds=bad))), bad
    for bad in (0, -1, 65536):
        assert is_arg(call(mod(n_steps=bad), n_path=27 * m)), bad
    for bad in (0, -2, 3, 16):
        assert is_arg(call(mod(stride=bad), n_path=27 * m)), bad
    for bad in (-2, -3, 19, 100):
        d = D(); d.fields[1] = bad
        assert is_arg(call(d)), bad
    for bad in (-3, 19, 100):
        assert is_arg(call(mod(carry=bad), ca=DEF)), bad
    assert is_arg(call(D(fields=("vx", V, "vz"))))                   # values missing
    assert is_arg(call(D(carry=V), ca=DEF))
    assert is_arg(call(D(), values=vals))                            # values given, none asked for
    assert is_arg(call(D(), n_path=27 * m - 1))
    assert is_arg(call(D(stride=2), n_path=27 * m))
    assert is_arg(call(D(), pa=None)) and is_arg(call(D(), st=None)) and is_arg(call(D(), nd=None))
    assert is_arg(call(D(), ca=DEF))                                 # carry_out without a carry
    assert is_arg(call(D(carry="u")))                                # a carry without carry_out
    for bad in (4, 8, -1):
        assert is_arg(call(mod(flags=bad))), bad
    for k in (0, 1):
        d = D(); d.reserved[k] = 1
        assert is_arg(call(d)), k
    for bad in ((0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0)):
        assert is_arg(call(D(normal=bad))), bad
    assert is_arg(call(D(omega=(0.0, np.nan, 0.0)))) and is_arg(call(D(omega=(np.inf, 0.0, 0.0))))
    assert is_arg(call(D(centre=(0.0, 0.0, np.nan)))) and is_arg(call(D(centre=(0.0, -np.inf, 0.0))))
    assert is_arg(call(D(box=((np.nan, 0, 0), (1, 1, 1))))) and is_arg(call(D(box=((0, 0, 0), (1, np.nan, 1)))))
    assert is_arg(call(D(clip=((np.nan, 0, 0), (1, 1, 1))))) and is_arg(call(D(clip=((0, 0, 0), (1, 1, np.nan)))))
    for bad in (-1.0, np.nan):
        assert is_arg(call(D(h=bad))), bad
    assert is_arg(call(mod(weight=2)))
    assert lib.sph_trace(None, C.byref(D()), m, *(pts[k].ctypes.data for k in range(3)), None, path.ctypes.data, 27 * m, None,
                         status.ctypes.data, done.ctypes.data, None) == SPH_ERR_ARG
    # the good calls: n_seeds == 0 writes no row; a zero normal is ignored without SPH_TRACE_PLANAR
    assert call(D(), mm=0, p=(None, None, None)) == 0 and np.all(path == 7.0) and np.all(status == 77) and tuple(cnt) == (0,) * 5
    assert call(D(carry=V, fields=("vx", V, "vz")), values=vals, ca=DEF) == 0
    assert np.all(path != 7.0) and np.all(car != 7.0) and np.all(status != 77) and np.all(done != 77) and sum(cnt) == m
    ctx.density()
    assert call(D(carry="rho", weight="volume"), ca=DEF) == 0
    ctx.close()
    # a bad source h (variable h): SPH_ERR_STATE in the host form, d_counts[0] == -1 and NaN outputs in the device form
    gv, sv = ic.split_rows(ic.keplerian_disc_var(3000, seed=38))
    v = _ctx(capi, gv, sv, variable=True, density=False)
    dp = torch.from_numpy(np.ascontiguousarray(pts.T)).to(torch.device("cuda", 0))
    for bad in (-1.0, 0.0, np.inf, np.nan):
        h = gv["h"].copy()
        h[17] = bad
        v.upload_field("h", h)
        with pytest.raises(capi.SphError) as e:
            v.trace(pts.T, 4, 0.5)
        assert e.value.status == SPH_ERR_STATE and "sph_trace" in str(e.value)
        dpath, dst, dnd, dcar, dc = v.trace(dp, 4, 0.5, carry="u", counts=True, device=True)
        assert dc == (-1, 0, 0, 0, 0) and bool(dpath.isnan().all()) and bool(dcar.isnan().all()) and bool((dnd == 0).all())
        assert sum(v.trace(pts.T, 4, 0.5, counts=True, h=2.0)[3]) == m
    v.close()


def test_cli_matches_context_trace(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    seeds, _ = trc.ring_seeds(25.0, 16)
    common = ["--ring", "25", "16", "--steps", "8", "--ds", "0.5", "--stride", "2", "--arclength", "--planar", "0", "0", "1",
              "--omega", "0", "0", "0.01", "--carry", "rho", "--json"]
    kw = dict(arclength=True, normal=(0.0, 0.0, 1.0), omega=(0.0, 0.0, 0.01), carry="rho", stride=2, counts=True)
    for both in (False, True):
        out = tmp_path / f"t{int(both)}.npz"
        r = subprocess.run([sys.executable, "-m", "summersph_amd.trace", str(save), "-o", str(out)] + common +
                           (["--both"] if both else []), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        z = np.load(out)
        assert np.array_equal(z["seeds"], seeds) and tuple(z["shape"]) == (16,)
        if both:
            path, (su, sd), (nu, nd), car, cnt = trc.both_ways(ctx, seeds, 8, 0.5, **kw)
            assert path.shape == (9, 3, 16) and np.array_equal(path[4], seeds.T)
            assert np.array_equal(z["status_up"], su) and np.array_equal(z["n_done_up"], nu)
        else:
            path, sd, nd, car, cnt = ctx.trace(seeds, 8, 0.5, **kw)
        assert np.array_equal(z["path"], path, equal_nan=True) and np.array_equal(z["carry"], car, equal_nan=True)
        assert np.array_equal(z["status"], sd) and np.array_equal(z["n_done"], nd) and tuple(z["counts"]) == cnt
        assert int(z["desc_flags"]) == capi.TRACE_ARCLENGTH | capi.TRACE_PLANAR and int(z["desc_n_steps"]) == 8
        j = json.loads(r.stdout.strip().splitlines()[-1])
        assert j["n_seeds"] == 16 and j["done"] == cnt[0] and j["rows"] == path.shape[0]
    ctx.close()
