"""GPU tests of sph_cube (include/summersph.h, "spectral cubes") on the MI355X: parity with the numpy restatement
(tests/cube_ref.py) over the sample tests' sets, views, image and channel shapes; the line-profile regimes; mass in
velocity; footprint edges; determinism; ranks; a cull; no side effects on a running simulation; the errors; 10^6 particles
with a physical check; and the command line.

Bound: every voxel within 1e-12 of the cube's largest magnitude (global, not per channel: a difference of erf values
carries an absolute error of about 1e-16 of the column term, which is arbitrarily large relative to a far-wing channel)."""
import ctypes as C
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import cube_ref
from gpu_support import capi, golden_gas, make_context
from summersph_amd import cube as cb
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
TOL = 1e-12
ALONG_X = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])       # u^ = y^, v^ = z^, w^ = x^


_ctx = functools.partial(make_context, density=True)      # every call here reads rho unless it says density=False


def _set(capi, name, density=True):
    if name == "box20000":
        gas, sinks = ic.split_rows(ic.uniform_box(20000))
        return _ctx(capi, gas, sinks, density=density)
    if name == "discvar20000":
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000))
        return _ctx(capi, gas, sinks, variable=True, density=density)
    gas, sinks = golden_gas(name)
    return _ctx(capi, gas, sinks, variable="discv" in name, density=density)


def _state(ctx, capi, with_c=True):
    pos = np.stack([ctx.field("x"), ctx.field("y"), ctx.field("z")], axis=1)
    vel = np.stack([ctx.field("vx"), ctx.field("vy"), ctx.field("vz")], axis=1)
    h = ctx.field("h") if ctx.params.flags & capi.FLAG_VARIABLE_H else float(ctx.params.h)
    return pos, vel, ctx.field("m"), h, (ctx.field("c") if with_c else None)


def _ref(state, kw):
    pos, vel, m, h, c = state
    kw = dict(kw)
    if kw.get("h") is not None:
        h = kw["h"]
    kw.pop("h", None)
    return cube_ref.cube(pos, vel, m, h, c=c, **kw)


def _close(got, want, what, tol=TOL):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    s = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print(f"    {what}: max err {err:.3e} scale {s:.3e} ratio {err / s if s > 0 else 0.0:.2e} (tol {tol:g})")
    assert s > 0.0, what
    assert err <= tol * s, (what, err, s)


def _image(P, h, half=16, c=None, spacing=0.8):
    """a node box of spacing 0.8 median h (a typical footprint covers a few nodes) about a particle at the median distance
    from the set's centre, not symmetric about it"""
    step = spacing * float(np.median(h))
    R = np.linalg.norm(P[:, :2] - P[:, :2].mean(axis=0), axis=1)
    c = P[np.argsort(R)[R.size // 2], :2] if c is None else c
    return ((c[0] - (half + 0.3) * step, c[1] - (half - 1) * step), (c[0] + half * step, c[1] + (half - 0.6) * step))


def _chan(V, n_chan):
    """channels over the central 96 % of the line-of-sight velocities: a few particles fall outside the range"""
    lo, hi = np.quantile(V, [0.02, 0.98])
    if not hi > lo:
        lo, hi = lo - 1.0, lo + 1.0
    dv = (hi - lo) / n_chan
    return lo + 0.5 * dv, dv


SETS = ["disc3000_eval", "discv3000_eval", "bin2000_eval", "box20000", "discvar20000"]


@pytest.mark.parametrize("name", SETS)
def test_parity_with_the_restatement(capi, name):
    ctx = _set(capi, name)
    state = _state(ctx, capi)
    pos, vel, m, h, c = state

    def kw_h(extra, h):
        return extra["h"] if extra.get("h") is not None else h
    rng = np.random.default_rng(4)
    vals = rng.normal(size=ctx.n) + 0.5
    centre, v_ref = pos.mean(axis=0) + np.array([1.5, -2.0, 0.25]), np.array([0.05, -0.02, 0.01])
    hmed = float(np.median(h)) if not np.isscalar(h) else h
    cases = []
    for tag, rot, extra in (("identity n17", np.eye(3), dict(n_chan=17, sigma_floor="dv")),
                            ("40/30 two chunks values per-velocity", cb.view(40.0, 30.0),
                             dict(n_chan=capi.CUBE_CHUNK + 1, sigma_scale=0.3, values=vals, per_velocity=True)),
                            ("along x one channel h clip", ALONG_X, dict(n_chan=1, h=1.3 * hmed, clip=True, sigma_floor="dv")),
                            ("centre v_ref 40/30 azimuth", cb.view(40.0, 30.0, 75.0),
                             dict(n_chan=17, centre=centre, v_ref=v_ref, sigma_scale=0.2, sigma_floor="dv", values=vals))):
        P, V = cube_ref.project(rot, pos, vel, extra.get("centre", (0, 0, 0)), extra.get("v_ref", (0, 0, 0)))
        n_chan = extra["n_chan"]
        v0, dv = _chan(V, n_chan)
        if n_chan == 1:                                   # the single wide channel: every weight exactly 1
            v0, dv = 0.5 * (V.min() + V.max()), 40.0 * (V.max() - V.min() + 1.0)
        kw = dict(shape=(33, 31), bounds=_image(P, kw_h(extra, h), spacing=0.4 if ctx.n > 5000 else 0.8), v0=v0, dv=dv, rot=rot)
        kw.update(extra)
        if kw.get("sigma_floor") == "dv":                 # the wide channel: every profile well inside it
            kw["sigma_floor"] = 0.7 * dv if n_chan > 1 else 0.05 * (V.max() - V.min() + 1.0)
        if kw.get("clip") is True:
            lo, hi = pos.min(axis=0), pos.max(axis=0)
            kw["clip"] = (lo + 0.2 * (hi - lo), (hi[0] + 1.0, hi[1] - 0.1 * (hi[1] - lo[1]), np.inf))
        cases.append((tag, kw))
    for tag, kw in cases:
        got = ctx.cube(**kw)
        want = _ref(state, kw)
        assert got.shape == (kw["n_chan"], 33, 31)
        _close(got, want, f"{name} {tag}")
    ctx.close()


def test_line_profile_regimes(capi):
    gas, sinks = golden_gas("disc3000_eval")
    gas = {k: v.copy() for k, v in gas.items()}
    n_chan, v0, dv = 16, -1.0, 0.125
    e = cube_ref.edges(v0, dv, n_chan)
    gas["vz"][:4] = [e[5], e[0], e[n_chan], np.nextafter(e[n_chan], -np.inf)]    # on an edge, on e_0, on e_n, just inside
    gas["vz"][4:] = np.random.default_rng(2).uniform(e[0] - 0.3, e[-1] + 0.3, gas["vz"].size - 4)
    for j, (ox, oy) in enumerate(((-3.0, 2.0), (4.0, -1.5), (-2.0, -4.0)), start=1):     # inside the image, about particle 0
        gas["x"][j], gas["y"][j], gas["z"][j] = gas["x"][0] + ox, gas["y"][0] + oy, gas["z"][0] + 0.1 * j
    gas["u"] *= np.random.default_rng(3).uniform(0.3, 3.0, gas["u"].size)          # a varying sound speed
    ctx = _ctx(capi, gas, sinks)
    state = _state(ctx, capi)
    pos, vel, m, h, c = state
    assert np.ptp(c) > 0.2 * c.mean()
    P, V = cube_ref.project(np.eye(3), pos, vel)
    assert V[0] == e[5] and V[1] == e[0] and V[2] == e[n_chan]
    base = dict(shape=(33, 31), bounds=_image(P, h, c=P[0, :2]), v0=v0, dv=dv, n_chan=n_chan)
    # sigma = 0: top-hat binning; the total over the image nodes of one particle goes into exactly one channel
    got = ctx.cube(**base)
    want = _ref(state, base)
    _close(got, want, "sigma 0")
    alone = dict(base, clip=((pos[0] - 1e-9).tolist(), (pos[0] + 1e-9).tolist()))
    assert all(np.all((P[j, :2] > base["bounds"][0]) & (P[j, :2] < base["bounds"][1])) for j in range(4))
    one = ctx.cube(**alone)
    lit = np.flatnonzero(one.reshape(n_chan, -1).sum(axis=1))
    assert list(lit) == [5], lit                                                   # e_5 <= V < e_6
    for j, k in ((1, 0), (3, n_chan - 1)):
        alone = dict(base, clip=((pos[j] - 1e-9).tolist(), (pos[j] + 1e-9).tolist()))
        assert list(np.flatnonzero(ctx.cube(**alone).reshape(n_chan, -1).sum(axis=1))) == [k], j
    alone = dict(base, clip=((pos[2] - 1e-9).tolist(), (pos[2] + 1e-9).tolist()))
    assert not ctx.cube(**alone).any()                                             # V == e_n: in no channel
    for tag, kw in (("sigma dv/50", dict(sigma_floor=dv / 50.0)), ("sigma 100 dv n", dict(sigma_floor=100.0 * dv * n_chan)),
                    ("sigma scale c", dict(sigma_scale=0.4)), ("scale and floor", dict(sigma_scale=0.4, sigma_floor=dv / 3))):
        kw = dict(base, **kw)
        _close(ctx.cube(**kw), _ref(state, kw), tag)
    ctx.close()
    # a stale c: refused with sigma_scale > 0 only
    ctx = _ctx(capi, gas, sinks, density=False)
    with pytest.raises(capi.SphError) as ei:
        ctx.field("c")
    assert ei.value.status == SPH_ERR_STATE
    with pytest.raises(capi.SphError) as ei:
        ctx.cube(**dict(base, sigma_scale=0.4))
    assert ei.value.status == SPH_ERR_STATE
    got = ctx.cube(**dict(base, sigma_floor=dv / 3))
    _close(got, _ref(state, dict(base, sigma_floor=dv / 3)), "stale c, sigma_scale 0")
    ctx.close()


def test_mass_in_velocity(capi):
    ctx = _set(capi, "disc3000_eval")
    state = _state(ctx, capi)
    pos, vel, m, h, c = state
    rot = cb.view(40.0, 30.0)
    P, V = cube_ref.project(rot, pos, vel)
    sigma, dv, n_chan = 0.13, 0.125, 41
    v0 = -0.5 * (n_chan - 1) * dv
    e = cube_ref.edges(v0, dv, n_chan)
    assert e[0] < (V - 8.5 * sigma).min() and (V + 8.5 * sigma).max() < e[-1]     # every profile lies inside the channels
    kw = dict(shape=(33, 31), bounds=_image(P, h), rot=rot)
    got = ctx.cube(v0=v0, dv=dv, n_chan=n_chan, sigma_floor=sigma, **kw)
    wide = ctx.cube(v0=0.0, dv=e[-1] - e[0], n_chan=1, sigma_floor=sigma, **kw)
    _close(got.sum(axis=0), wide[0], "channel sum against the wide channel")
    _close(wide, _ref(state, dict(kw, v0=0.0, dv=e[-1] - e[0], n_chan=1, sigma_floor=sigma)), "wide channel")
    ctx.close()


def test_footprint_edges(capi):
    gas, sinks = golden_gas("disc3000_eval")
    gas = {k: v.copy() for k, v in gas.items()}
    hh = 0.5
    # nodes on the integers of [0, 8] x [0, 6]; the first particles are placed by hand
    gas["x"][:5] = [9.25, 8.75, 5.0, -1.5, 4.0]      # outside by 2.5 h; straddling the edge; 2 h from node (4, 3) ...
    gas["y"][:5] = [3.0, 3.0, 3.0, 7.25, 7.0]        # ... (6, 3), (5, 2), (5, 4); a corner out of reach; 2 h above the top edge
    ctx = _ctx(capi, gas, sinks, density=False)
    state = _state(ctx, capi, with_c=False)
    pos = state[0]
    base = dict(shape=(9, 7), bounds=((0.0, 0.0), (8.0, 6.0)), v0=0.0, dv=1e3, n_chan=1, h=hh)
    _close(ctx.cube(**base), _ref(state, base), "hand-placed")

    def only(j, **kw):
        return ctx.cube(**dict(base, clip=((pos[j] - 1e-9).tolist(), (pos[j] + 1e-9).tolist()), **kw))[0]
    out = only(0)
    assert not out.any() and not np.signbit(out).any()                 # more than 2 h outside: exact +0.0 everywhere
    out = only(1)
    assert out[8, 3] > 0.0 and out[7, 3] == 0.0 and np.count_nonzero(out) == 1
    out = only(2)                                                      # nodes exactly 2 h away get +0.0
    assert out[5, 3] > 0.0 and np.count_nonzero(out) == 1
    for iu, iv in ((4, 3), (6, 3), (5, 2), (5, 4)):
        assert out[iu, iv] == 0.0 and not np.signbit(out[iu, iv])
    assert not only(3).any()
    out = only(4)
    assert not out.any() and not np.signbit(out).any()                 # the node (4, 6) is exactly 2 h away
    # n_u = 1 and n_v = 1: the single node sits at lo
    for shape in ((1, 7), (9, 1), (1, 1)):
        kw = dict(base, shape=shape, bounds=((3.0, 2.0), (8.0, 6.0)), n_chan=3, v0=-0.2, dv=0.2, sigma_floor=0.1, h=None)
        _close(ctx.cube(**kw), _ref(state, kw), f"shape {shape}")
    # an empty selection: zeros
    out = ctx.cube(**dict(base, clip=((1e6,) * 3, (2e6,) * 3), n_chan=5))
    assert out.shape == (5, 9, 7) and not out.any()
    far = ctx.cube(**dict(base, bounds=((1e5, 1e5), (1e5 + 8.0, 1e5 + 6.0))))
    assert not far.any()
    ctx.close()


def test_determinism(capi):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=31))
    ctx = _ctx(capi, gas, sinks)
    rot = cb.view(40.0, 30.0)
    kw = dict(shape=(40, 37), bounds=((-60.0, -50.0), (55.0, 60.0)), v0=-3.0, dv=6.0 / 33, n_chan=34, rot=rot, sigma_scale=0.5,
              sigma_floor=0.05)
    a = ctx.cube(**kw)
    assert a.any()
    assert np.array_equal(a, ctx.cube(**kw))                                       # a repeated call
    d = ctx.cube(device=True, **kw)
    assert isinstance(d, torch.Tensor) and d.is_cuda and np.array_equal(d.cpu().numpy(), a)      # host against _dev
    vals = np.random.default_rng(1).normal(size=ctx.n)
    dv_ = ctx.cube(device=True, values=torch.as_tensor(vals, device=d.device), **kw)
    assert np.array_equal(dv_.cpu().numpy(), ctx.cube(values=vals, **kw))
    # the context's sorted order does not enter: after a few steps the cube of the state in place is bitwise the cube of
    # a fresh context holding that state (same ids, another sorted order).  The (cell, id) rule of the renders is kept.
    ctx.run(3, 1e-3)
    state = {k: ctx.field(k) for k in capi.FIELDS[:9]}
    kw = dict(kw, sigma_scale=0.0, sigma_floor=0.2)                    # c is a derived field: it is not part of the state
    b = ctx.cube(**kw)
    assert not np.array_equal(a, b)
    fresh = _ctx(capi, state, sinks, density=False)
    assert np.array_equal(fresh.cube(**kw), b)
    fresh.close()
    # uploaded in another order the ids change and with them the order of a cell's terms: equal within the bound
    perm = np.random.default_rng(2).permutation(ctx.n)
    other = _ctx(capi, {k: v[perm] for k, v in state.items()}, sinks, density=False)
    _close(other.cube(**kw), b, "re-upload in another order")
    other.close()
    ctx.close()


def test_linearity_across_ranks(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(12000, seed=17))
    n = gas["x"].size
    rot = cb.view(55.0, 10.0)
    kw = dict(shape=(33, 31), bounds=((-50.0, -40.0), (45.0, 50.0)), v0=-2.0, dv=0.25, n_chan=17, rot=rot, sigma_floor=0.2)
    one = _ctx(capi, gas, sinks, variable=True, density=False)
    whole = one.cube(**kw)
    one.close()
    half = n // 2
    total = np.zeros_like(whole)
    for first in (True, False):
        ids = np.arange(n) if first else np.concatenate([np.arange(half, n), np.arange(half)])
        sub = {k: v[ids] for k, v in gas.items()}
        ctx = _ctx(capi, sub, sinks, variable=True, density=False)
        owned = half if first else n - half
        ctx.set_owned(owned)
        part = ctx.cube(**kw)
        # the ghosts contribute nothing: the restatement over the owned half alone
        pos = np.stack([sub["x"], sub["y"], sub["z"]], axis=1)
        vel = np.stack([sub["vx"], sub["vy"], sub["vz"]], axis=1)
        _close(part, cube_ref.cube(pos, vel, sub["m"], sub["h"], n_owned=owned, **kw), "rank")
        total += part
        ctx.close()
    _close(total, whole, "sum of the ranks")


def test_after_accrete_and_cull(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=12))
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])
    ctx = _ctx(capi, gas, sinks)
    ctx.forces()
    assert ctx.accrete_and_cull() > 0 and ctx.n < 20000
    state = _state(ctx, capi)
    vals = np.arange(ctx.n, dtype=np.float64) + 1.0                   # read in the survivors' order
    kw = dict(shape=(33, 31), bounds=((-40.0, -40.0), (40.0, 35.0)), v0=-2.0, dv=0.25, n_chan=17, rot=cb.view(40.0, 30.0),
              sigma_scale=0.5, values=vals)
    _close(ctx.cube(**kw), _ref(state, kw), "after a cull")
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    kw = dict(shape=(33, 31), bounds=((-50.0, -50.0), (50.0, 50.0)), v0=-3.0, dv=0.2, n_chan=33, rot=cb.view(40.0, 30.0))
    runs = []
    for with_cube in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_cube:
                before = {k: ctx.field(k) for k in ("x", "vx", "rho", "c", "ax", "du")}
                ctx.cube(sigma_scale=0.3, **kw)
                ctx.cube(sigma_floor=0.1, h=1.0, clip=((0, 0, -1), (50, 50, 1)), values=before["rho"], device=False, **kw)
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
    gas, sinks = ic.split_rows(ic.keplerian_disc(3000, seed=37))
    ctx = _ctx(capi, gas, sinks, density=False)
    lib = ctx.lib
    out = np.full(5 * 4 * 3, 7.0)

    def call(d, out_len=60, o=out, desc=True):
        return lib.sph_cube(ctx._h, C.byref(d) if desc else None, None, None if o is None else o.ctypes.data, out_len)

    def good():
        return capi.cube_desc((4, 3), ((-10.0, -10.0), (10.0, 10.0)), -1.0, 0.5, 5, sigma_floor=0.1)
    assert call(good()) == 0 and not (out == 7.0).any()
    out[:] = 7.0
    bad = []
    for field, value in (("n_chan", 0), ("n_chan", -3), ("n_u", 0), ("n_v", -1), ("dv", 0.0), ("dv", -0.5), ("dv", np.inf),
                         ("dv", np.nan), ("sigma_scale", -1e-3), ("sigma_floor", -1.0), ("sigma_floor", np.nan), ("reserved", 1),
                         ("h", -1.0), ("h", np.nan), ("flags", 2), ("flags", 4), ("v0", np.nan)):
        d = good()
        setattr(d, field, value)
        bad.append((f"{field}={value}", d))
    for field, idx, value in (("lo", 0, 11.0), ("hi", 1, -11.0), ("lo", 1, np.nan), ("hi", 0, np.inf), ("clip_lo", 2, np.nan),
                              ("clip_hi", 0, np.nan), ("centre", 1, np.inf), ("v_ref", 2, np.nan)):
        d = good()
        getattr(d, field)[idx] = value
        bad.append((f"{field}[{idx}]={value}", d))
    rots = {"scaled": 1.001 * np.eye(3), "left-handed": np.diag([1.0, 1.0, -1.0]), "sheared": np.array([[1, 1e-9, 0], [0, 1, 0], [0, 0, 1.0]]),
            "nan": np.full((3, 3), np.nan), "zero": np.zeros((3, 3))}
    for tag, r in rots.items():
        d = good()
        d.rot[:] = r.reshape(9).tolist()
        bad.append((f"rot {tag}", d))
    for tag, d in bad:
        assert call(d) == SPH_ERR_ARG, tag
    assert call(good(), out_len=59) == SPH_ERR_ARG and call(good(), out_len=61) == SPH_ERR_ARG
    assert call(good(), o=None) == SPH_ERR_ARG and call(good(), desc=False) == SPH_ERR_ARG
    assert (out == 7.0).all()                                         # nothing was written
    assert lib.sph_cube_dev(ctx._h, C.byref(good()), None, None, 60) == SPH_ERR_ARG
    # a rotation within 1e-12 of orthonormal is taken
    d = good()
    d.rot[:] = (cb.view(33.0, 21.0, 5.0) * (1.0 + 2e-13)).reshape(9).tolist()
    assert call(d) == 0
    with pytest.raises(ValueError):
        ctx.cube((4, 3), ((-1, -1), (1, 1)), 0.0, 1.0, 2, values=np.zeros(ctx.n + 1))
    ctx.close()


def _antisymmetry_residual(cube, v):
    """mean |m1(u, v) + m1(-u, -v)| / 2 over the pixels with column > 0 on both sides, in units of the peak |m1|"""
    m0, m1, _, _ = cb.moments(cube, v)
    flip = m1[::-1, ::-1]
    ok = (m0 > 0) & (m0[::-1, ::-1] > 0)
    return float(np.mean(np.abs(m1[ok] + flip[ok])) / 2.0 / np.nanmax(np.abs(m1))), int(ok.sum())


@pytest.mark.timeout(600)
def test_million_particles(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(1_000_000, seed=5))
    ctx = _ctx(capi, gas, sinks, density=False)
    state = _state(ctx, capi, with_c=False)
    pos, vel, m, h, _ = state
    rot = cb.view(40.0, 0.0)
    P, V = cube_ref.project(rot, pos, vel)
    ext = float(np.abs(P[:, :2]).max())
    n, n_chan, sigma = 256, 64, 0.1
    vmax = float(np.abs(V).max()) + 8.6 * sigma
    v0, dv = cb.vrange_channels(-vmax, vmax, n_chan)
    kw = dict(shape=(n, n), bounds=((-ext, -ext), (ext, ext)), v0=v0, dv=dv, n_chan=n_chan, rot=rot, sigma_floor=sigma)
    got = ctx.cube(**kw)
    scale = float(np.abs(got).max())
    # 256 random voxels among the lit ones, brute force over the particles whose footprint covers the pixel
    rng = np.random.default_rng(9)
    lit = np.argwhere(got > 1e-6 * scale)
    pick = lit[rng.choice(lit.shape[0], 256, replace=False)]
    gu = np.linspace(-ext, ext, n)
    want = cube_ref.voxels(pos, vel, m, h, gu, gu, pick[:, 1:], v0, dv, n_chan, pick[:, 0], rot, sigma_floor=sigma)
    err = float(np.max(np.abs(got[pick[:, 0], pick[:, 1], pick[:, 2]] - want)))
    print(f"    256 voxels: max err {err:.3e} of scale {scale:.3e}: {err / scale:.2e}")
    assert err <= TOL * scale
    # mass in velocity: every profile lies inside the channels
    wide = ctx.cube(**dict(kw, v0=0.0, dv=2.0 * vmax, n_chan=1))
    _close(got.sum(axis=0), wide[0], "channel sum against the wide channel")
    # the moment-1 map of the axisymmetric disc is antisymmetric under (u, v) -> (-u, -v) about the star; what is left is
    # particle noise, which the numpy restatement of a 10^5-particle draw of the same disc bounds
    res, npix = _antisymmetry_residual(got, cb.channels(v0, dv, n_chan))
    g5, _ = ic.split_rows(ic.keplerian_disc(100_000, seed=5))
    p5 = np.stack([g5["x"], g5["y"], g5["z"]], axis=1)
    v5 = np.stack([g5["vx"], g5["vy"], g5["vz"]], axis=1)
    ref5 = cube_ref.cube(p5, v5, g5["m"], h, **kw)
    res5, npix5 = _antisymmetry_residual(ref5, cb.channels(v0, dv, n_chan))
    print(f"    moment-1 antisymmetry residual: GPU 10^6 particles {res:.3e} over {npix} pixels, numpy 10^5 particles {res5:.3e} "
          f"over {npix5} pixels")
    assert npix > 1000 and res <= res5
    ctx.close()


def test_cli_matches_context_cube(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    out, fits = tmp_path / "cube.npz", tmp_path / "cube.fits"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.cube", str(save), "-o", str(out), "--inc", "40", "--pa", "30",
                        "--extent", "120", "--size", "48", "--vrange", "-3", "3", "--nchan", "24", "--sigma-scale", "0.3",
                        "--fits", str(fits), "--json"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    v0, dv = cb.vrange_channels(-3.0, 3.0, 24)
    want = ctx.cube((48, 48), ((-60.0, -60.0), (60.0, 60.0)), v0, dv, 24, rot=cb.view(40.0, 30.0), sigma_scale=0.3)
    z = np.load(out)
    assert want.any() and np.array_equal(z["cube"], want)
    assert np.array_equal(z["v"], cb.channels(v0, dv, 24)) and np.array_equal(z["rot"], cb.view(40.0, 30.0))
    m0, m1, m2, peak = cb.moments(want, z["v"])
    assert np.array_equal(z["moment0"], m0) and np.array_equal(z["moment1"], m1, equal_nan=True)
    hdr, data = cb.read_fits(str(fits))
    assert np.array_equal(data, want) and (hdr["NAXIS1"], hdr["NAXIS2"], hdr["NAXIS3"]) == (48, 48, 24)
    assert hdr["CRVAL3"] == v0 and hdr["CDELT3"] == dv and hdr["BITPIX"] == -64
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["shape"] == [24, 48, 48] and j["pixels_lit"] == int((m0 > 0).sum())
    ctx.close()
