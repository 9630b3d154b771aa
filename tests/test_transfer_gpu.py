"""GPU tests of sph_transfer (include/summersph.h, "emission-absorption images") on the MI355X: parity with the numpy
restatement (tests/transfer_ref.py) over the sample and cube tests' sets, views and input sources; the smallest shapes that
can break the tile lists and the gather; the order of the compositing; the cross-check against sph_cube; determinism; no
side effects on a running simulation; the errors; 10^6 particles with a physical check; and the command line.

Bound.  Planes 0, 1 and 2 (I + T background, tau, T) each within 1e-12 of that plane's largest reference magnitude at
every node.  Plane 3 (the depth of the tau_surface surface) within 1e-12 of the largest |D| the reference reports, NaN
where the reference has NaN.  A node may be left out only where the reference's tau just before or after crossing
tau_surface (plane 3) or tau_max (every plane: the node stops one particle earlier or later) lies within 1e-9 relative of
that threshold; such nodes must be at most 1 % of the nodes the reference lights, which is asserted on the reference
alone."""
import ctypes as C
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
import cube_ref
from gpu_support import capi, make_context
import transfer_ref
from summersph_amd import cube as cb
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
TOL = 1e-12
ALONG_X = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])       # u^ = y^, v^ = z^, w^ = x^: edge-on
FLIP = np.diag([-1.0, 1.0, -1.0])                                              # (u^, v^, w^) -> (-u^, v^, -w^)


_ctx = functools.partial(make_context, density=True)      # every call here reads rho unless it says density=False


def _set(capi, name):
    if name == "box20000":
        gas, sinks = ic.split_rows(ic.uniform_box(20000))
        return _ctx(capi, gas, sinks)
    if name == "discvar20000":
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000))
        return _ctx(capi, gas, sinks, variable=True)
    gas, sinks = ic.split_rows(load_golden(name + "_eval")["ic"])
    return _ctx(capi, gas, sinks, variable="discv" in name)


def _state(ctx, capi):
    pos = np.stack([ctx.field("x"), ctx.field("y"), ctx.field("z")], axis=1)
    h = ctx.field("h") if ctx.params.flags & capi.FLAG_VARIABLE_H else float(ctx.params.h)
    return pos, ctx.field("m"), h


def _gas(pos, m, u=None, h=None):
    """an upload of particles at rest"""
    n = pos.shape[0]
    g = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": np.zeros(n), "vy": np.zeros(n), "vz": np.zeros(n),
         "u": np.full(n, 0.25) if u is None else np.asarray(u, dtype=np.float64).copy(), "m": np.asarray(m, dtype=np.float64).copy(),
         "alpha": np.zeros(n)}
    if h is not None:
        g["h"] = np.asarray(h, dtype=np.float64).copy()
    return g


def _ref(state, kw, fields=None, info=None):
    """the restatement of Context.transfer(**kw); field names among source / kappa are looked up in `fields`"""
    pos, m, h = state
    kw = dict(kw)
    if kw.get("h") is not None:
        h = kw["h"]
    kw.pop("h", None)
    for key in ("source", "kappa"):
        if isinstance(kw.get(key), str):
            kw[key] = fields[kw[key]]
    kw.setdefault("kappa", None)
    if "source" not in kw:
        kw["source"] = fields["u"]                            # Context.transfer's default
    return transfer_ref.transfer(pos, m, h, info=info, **kw)


def _check(got, state, kw, what, fields=None, need_surface=False):
    """the scoring rule of the module's docstring; returns the reference and its info"""
    info = {}
    want = _ref(state, kw, fields, info)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    lit = want[1] > 0.0
    skip_all = info["near_stop"]
    skip_surf = info["near_surface"] | skip_all
    assert lit.any(), what
    assert skip_surf.sum() <= 0.01 * lit.sum(), (what, int(skip_surf.sum()), int(lit.sum()))      # on the reference alone
    line = f"    {what}:"
    for k, name in enumerate(("I", "tau", "T")):
        s = float(np.max(np.abs(want[k])))
        err = float(np.max(np.abs(got[k] - want[k])[~skip_all]))
        line += f" {name} {err:.2e}/{s:.2e}"
        assert err <= TOL * s, (what, name, err, s)
    g3, w3 = got[3][~skip_surf], want[3][~skip_surf]
    assert np.array_equal(np.isnan(g3), np.isnan(w3)), (what, int(np.isnan(g3).sum()), int(np.isnan(w3).sum()))
    seen = ~np.isnan(w3)
    if need_surface:
        assert seen.any() and not seen.all(), what
    if seen.any():
        s = float(np.max(np.abs(w3[seen])))
        err = float(np.max(np.abs(g3[seen] - w3[seen])))
        line += f" surf {err:.2e}/{s:.2e} ({int(seen.sum())} nodes)"
        assert err <= TOL * s, (what, "surf", err, s)
    print(line + f" stopped {int(info['stopped'].sum())} lit {int(lit.sum())} left out {int(skip_surf.sum())}")
    return want, info


def _image(P, h, half=16, c=None, spacing=0.8):
    """a node box of spacing 0.8 median h about a particle at the median distance from the set's centre, 33 x 31 nodes at
    half = 16, not symmetric about it"""
    step = spacing * float(np.median(h))
    R = np.linalg.norm(P[:, :2] - P[:, :2].mean(axis=0), axis=1)
    c = P[np.argsort(R)[R.size // 2], :2] if c is None else c
    return ((c[0] - (half + 0.3) * step, c[1] - (half - 1) * step), (c[0] + half * step, c[1] + (half - 0.6) * step))


def _median_tau(state, kw, fields=None):
    """the reference's median total optical depth over the nodes it lights, at kappa_scale = 1 and without a stop"""
    tau = _ref(state, dict(kw, kappa_scale=1.0, tau_max=np.inf), fields)[1]
    assert (tau > 0).any()
    return float(np.median(tau[tau > 0]))


SETS = ["sod1000", "disc3000", "discv3000", "box20000", "discvar20000"]


@pytest.mark.parametrize("name", SETS)
def test_parity_with_the_restatement(capi, name):
    ctx = _set(capi, name)
    state = _state(ctx, capi)
    pos, m, h = state
    fields = {k: ctx.field(k) for k in ("u", "rho")}
    rng = np.random.default_rng(4)
    K = rng.uniform(0.0, 2.0, ctx.n)
    S = rng.normal(size=ctx.n) + 0.5                                   # both signs
    hmed = float(np.median(h)) if not np.isscalar(h) else h
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    clip = (lo + 0.2 * (hi - lo), (hi[0] + 1.0, hi[1] - 0.1 * (hi[1] - lo[1]), np.inf))
    spacing = 0.4 if ctx.n > 5000 else 0.8
    for tag, rot, extra, target, stop in (
            ("face-on S field K array", np.eye(3), dict(source="u", kappa=K), 2.0, None),
            ("40/30 S array K field background", cb.view(40.0, 30.0), dict(source=S, kappa="rho", background=0.75), 1.0, None),
            ("along x h clip K one", ALONG_X, dict(source="u", h=1.3 * hmed, clip=clip, tau_surface=0.5), 1.5, None),
            ("flipped 40/30 stop at the median", FLIP @ cb.view(40.0, 30.0), dict(source=S, kappa=K, centre=(0.5, -0.25, 0.1)), 4.0, 1.0)):
        P, _ = cube_ref.project(rot, pos, np.zeros_like(pos), extra.get("centre", (0, 0, 0)))
        kw = dict(shape=(33, 31), bounds=_image(P, extra.get("h", h), spacing=spacing), rot=rot, **extra)
        med = _median_tau(state, kw, fields)
        kw["kappa_scale"] = target / med                               # the median lit node has tau = target
        if stop is not None:
            kw["tau_max"] = stop * target                              # about half of the lit nodes stop
        got = ctx.transfer(**kw)
        assert got.shape == (4, 33, 31)
        want, info = _check(got, state, kw, f"{name} {tag}", fields, need_surface=True)
        if stop is not None:
            frac = info["stopped"].sum() / (want[1] > 0).sum()
            assert 0.25 <= frac <= 0.75, frac
    ctx.close()


def _tile_case(seed, n, extent=7.0, hlo=0.8, hhi=1.5):
    """n particles within reach of the 8 x 8 nodes on the integers of [0, 7]^2: one tile"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0.0, extent, n), rng.uniform(0.0, extent, n), rng.normal(0.0, 3.0, n)], axis=1)
    return pos, rng.uniform(0.5, 1.5, n), rng.uniform(hlo, hhi, n), rng.uniform(0.0, 2.0, n), rng.normal(size=n)


def _small(capi, pos, m, h):
    ctx = _ctx(capi, _gas(pos, m, h=h), variable=True, density=False)
    return ctx, (pos, m, h)


@pytest.mark.parametrize("n", [127, 128, 129, 257])
def test_lds_batch_edges(capi, n):
    pos, m, h, K, S = _tile_case(20 + n, n)
    ctx, state = _small(capi, pos, m, h)
    base = dict(shape=(8, 8), bounds=((0.0, 0.0), (7.0, 7.0)), source=S, kappa=K)
    med = _median_tau(state, base)
    for tag, kw in (("thin", dict(kappa_scale=1e-3 / med)), ("tau 3", dict(kappa_scale=3.0 / med)),
                    ("stop", dict(kappa_scale=6.0 / med, tau_max=5.0, background=-0.5))):
        _check(ctx.transfer(**dict(base, **kw)), state, dict(base, **kw), f"{n} records {tag}")
    # every record reaches every node of the tile: the whole list is walked by all 64 lanes
    wide = dict(base, h=8.0, kappa_scale=0.5 * 3.0 / med)
    _check(ctx.transfer(**wide), state, wide, f"{n} records wide")
    ctx.close()


def test_footprints_wider_than_tiles(capi):
    rng = np.random.default_rng(31)
    n_big, n_small = 60, 400
    pos = np.stack([rng.uniform(-2.0, 34.0, n_big + n_small), rng.uniform(-2.0, 32.0, n_big + n_small),
                    rng.normal(0.0, 4.0, n_big + n_small)], axis=1)
    h = np.concatenate([rng.uniform(5.0, 12.0, n_big), rng.uniform(0.6, 1.4, n_small)])     # 4 h: up to six tiles across
    m = np.concatenate([rng.uniform(20.0, 60.0, n_big), rng.uniform(0.5, 1.5, n_small)])
    K, S = rng.uniform(0.0, 2.0, pos.shape[0]), rng.normal(size=pos.shape[0])
    ctx, state = _small(capi, pos, m, h)
    base = dict(shape=(33, 31), bounds=((0.0, 0.0), (32.0, 30.0)), source=S, kappa=K)
    med = _median_tau(state, base)
    for rot in (np.eye(3), FLIP):
        kw = dict(base, rot=rot, kappa_scale=2.0 / med, centre=(16.0, 0.0, 0.0) if rot is FLIP else (0.0, 0.0, 0.0))
        if rot is FLIP:
            kw["bounds"] = ((-16.0, 0.0), (16.0, 30.0))
        _check(ctx.transfer(**kw), state, kw, f"wide footprints {'flipped' if rot is FLIP else 'face-on'}", need_surface=True)
    kw = dict(base, kappa_scale=8.0 / med, tau_max=6.0)
    _, info = _check(ctx.transfer(**kw), state, kw, "wide footprints stop")
    assert info["stopped"].any() and not info["stopped"].all()
    ctx.close()


def test_equal_depths_fall_to_the_id(capi):
    # a flat sheet at z = 0 seen face-on, ids shuffled against position, the zeros of both signs: every depth compares equal,
    # so the id alone orders the compositing; tau of order one per particle and a strongly varying S make the order visible
    rng = np.random.default_rng(32)
    g = np.arange(24, dtype=np.float64)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2) * 0.7 + rng.uniform(-0.1, 0.1, (576, 2))
    xy = xy[rng.permutation(576)]
    pos = np.concatenate([xy, np.where(rng.uniform(size=576) < 0.5, 0.0, -0.0)[:, None]], axis=1)
    assert np.signbit(pos[:, 2]).any() and not np.signbit(pos[:, 2]).all()
    m, h = rng.uniform(0.5, 1.5, 576), rng.uniform(0.9, 1.3, 576)
    S = 10.0 ** rng.uniform(-1.0, 1.0, 576)
    ctx, state = _small(capi, pos, m, h)
    base = dict(shape=(33, 31), bounds=((0.5, 0.5), (15.5, 15.0)), source=S)
    med = _median_tau(state, base)
    kw = dict(base, kappa_scale=6.0 / med)
    got = ctx.transfer(**kw)
    want, _ = _check(got, state, kw, "flat sheet, ids shuffled", need_surface=False)
    # the same sheet composited in the reverse id order differs by far more than the bound: the tie-break is tested
    rev = transfer_ref.transfer(pos[::-1], m[::-1], h[::-1], source=S[::-1], **{k: v for k, v in kw.items() if k != "source"})
    assert np.max(np.abs(rev[0] - want[0])) > 0.05 * np.max(want[0])
    assert np.all(got[3][~np.isnan(got[3])] == 0.0)
    ctx.close()


def test_degenerate_images(capi):
    pos, m, h, K, S = _tile_case(33, 300, extent=12.0)
    ctx, state = _small(capi, pos, m, h)
    base = dict(source=S, kappa=K, rot=cb.view(20.0, 10.0), centre=(6.0, 6.0, 0.0))
    med = _median_tau(state, dict(base, shape=(9, 9), bounds=((-4.0, -4.0), (4.0, 4.0))))
    for shape, bounds in (((1, 31), ((0.5, -4.0), (3.0, 4.0))), ((33, 1), ((-4.0, 0.25), (4.0, 3.0))), ((1, 1), ((0.1, -0.2), (1.0, 1.0))),
                          ((5, 31), ((0.5, -4.0), (0.5, 4.0))), ((33, 9), ((-4.0, -1.0), (4.0, -1.0))), ((3, 4), ((1.0, 1.0), (1.0, 1.0)))):
        kw = dict(base, shape=shape, bounds=bounds, kappa_scale=2.0 / med, tau_max=4.0)
        got = ctx.transfer(**kw)
        want, _ = _check(got, state, kw, f"shape {shape} bounds {bounds}")
        if bounds[0][0] == bounds[1][0]:                               # a flat axis: every node of it is the same point
            assert np.array_equal(got[:, :1].repeat(shape[0], axis=1), got, equal_nan=True)
    # no particle reaches a node: the background, tau 0, T 1, no surface
    far = ctx.transfer(shape=(9, 7), bounds=((1e5, 1e5), (1e5 + 8.0, 1e5 + 6.0)), source=S, background=0.3)
    assert np.all(far[0] == 0.3) and not far[1].any() and np.all(far[2] == 1.0) and np.isnan(far[3]).all()
    none = ctx.transfer(shape=(9, 7), bounds=((0.0, 0.0), (8.0, 6.0)), source=S, clip=((1e6,) * 3, (2e6,) * 3), background=-1.0)
    assert np.all(none[0] == -1.0) and not none[1].any() and np.all(none[2] == 1.0) and np.isnan(none[3]).all()
    ctx.close()


def test_stops_inside_a_tile(capi):
    rng = np.random.default_rng(34)
    # (a) an opaque blob over the left half of one tile, a thin veil over all of it: some lanes stop, others never do
    nb, nv = 150, 200
    blob = np.stack([rng.uniform(-0.5, 2.5, nb), rng.uniform(-0.5, 7.5, nb), rng.normal(0.0, 2.0, nb)], axis=1)
    veil = np.stack([rng.uniform(-0.5, 7.5, nv), rng.uniform(-0.5, 7.5, nv), rng.normal(0.0, 2.0, nv)], axis=1)
    pos = np.concatenate([blob, veil])
    m = np.concatenate([np.full(nb, 40.0), np.full(nv, 0.02)])
    h = np.concatenate([rng.uniform(0.5, 0.7, nb), rng.uniform(0.8, 1.2, nv)])
    S = rng.normal(size=nb + nv)
    ctx, state = _small(capi, pos, m, h)
    kw = dict(shape=(8, 8), bounds=((0.0, 0.0), (7.0, 7.0)), source=S, tau_max=8.0)
    _, info = _check(ctx.transfer(**kw), state, kw, "half of a tile stops", need_surface=True)
    assert info["stopped"][:3].all() and not info["stopped"][5:].any()
    ctx.close()
    # (b) 100 heavy wide particles in front of 400 others: all 64 lanes stop inside the first batch of 128 records
    nf, nr = 100, 400
    front = np.stack([rng.uniform(0.0, 7.0, nf), rng.uniform(0.0, 7.0, nf), rng.uniform(-20.0, -10.0, nf)], axis=1)
    rest = np.stack([rng.uniform(0.0, 7.0, nr), rng.uniform(0.0, 7.0, nr), rng.uniform(0.0, 10.0, nr)], axis=1)
    pos = np.concatenate([rest, front])
    m, h = np.concatenate([np.full(nr, 1.0), np.full(nf, 30.0)]), np.concatenate([rng.uniform(0.8, 1.2, nr), np.full(nf, 6.0)])
    S = rng.normal(size=nf + nr)
    ctx, state = _small(capi, pos, m, h)
    kw = dict(shape=(8, 8), bounds=((0.0, 0.0), (7.0, 7.0)), source=S, tau_max=5.0)
    got = ctx.transfer(**kw)
    want, info = _check(got, state, kw, "a tile stops in its first batch")
    assert info["stopped"].all() and np.nanmax(want[3]) < -10.0          # the surface lies in the front layer
    # (c) K = 0 particles in front of opaque ones add nothing, whatever their S
    K = np.concatenate([np.ones(nr), np.zeros(nf)])
    Sb = S.copy(); Sb[nr:] = 1e6
    kw = dict(shape=(8, 8), bounds=((0.0, 0.0), (7.0, 7.0)), source=Sb, kappa=K, kappa_scale=3.0)
    got = ctx.transfer(**kw)
    _check(got, state, kw, "K = 0 in front")
    alone = ctx.transfer(**dict(kw, clip=((-np.inf, -np.inf, -1.0), (np.inf, np.inf, np.inf))))
    assert np.array_equal(got, alone, equal_nan=True)
    ctx.close()


def _two_layers(seed=35):
    """hot and thin (z = -2) over cold and thick (z = +2), seen down z"""
    rng = np.random.default_rng(seed)
    n1, n2 = 1500, 1500
    pos = np.concatenate([np.stack([rng.uniform(-2.0, 18.0, n), rng.uniform(-2.0, 17.0, n), z + 0.1 * rng.normal(size=n)], axis=1)
                          for n, z in ((n1, -2.0), (n2, 2.0))])
    m = np.concatenate([np.full(n1, 0.12), np.full(n2, 1.5)])
    h = rng.uniform(0.8, 1.2, n1 + n2)
    u = np.concatenate([np.full(n1, 10.0), np.full(n2, 1.0)])
    return pos, m, h, u


def test_order_matters(capi):
    pos, m, h, u = _two_layers()
    ctx = _ctx(capi, _gas(pos, m, u=u, h=h), variable=True, density=False)
    state, fields = (pos, m, h), {"u": u}
    kw = dict(shape=(33, 31), bounds=((0.0, 0.0), (16.0, 15.0)), source="u", kappa_scale=0.5)
    front = ctx.transfer(**kw)
    want, _ = _check(front, state, kw, "hot thin layer in front", fields)
    kwb = dict(kw, rot=FLIP, bounds=((-16.0, 0.0), (0.0, 15.0)))
    back = ctx.transfer(**kwb)
    _check(back, state, kwb, "cold thick layer in front", fields)
    # the same lines of sight (u mirrored), the same tau, another image: an optically thin pass could not tell them apart
    a, b = front[0], back[0][::-1]
    assert np.max(np.abs(front[1] - back[1][::-1])) <= 1e-12 * np.max(front[1])
    assert 0.2 < np.median(front[1]) and np.max(np.abs(a - b)) > 0.1 * max(a.max(), b.max())
    assert np.median(a) > 1.5 * np.median(b)                          # the hot layer shows when it is in front
    ctx.close()


def test_against_the_cube(capi):
    ctx = _set(capi, "disc3000")
    state = _state(ctx, capi)
    pos, m, h = state
    rng = np.random.default_rng(36)
    K, S = rng.uniform(0.0, 2.0, ctx.n), rng.uniform(0.0, 3.0, ctx.n)
    rot = cb.view(40.0, 30.0)
    P, _ = cube_ref.project(rot, pos, np.zeros_like(pos))
    img = dict(shape=(33, 31), bounds=_image(P, h), rot=rot)
    wide = dict(v0=0.0, dv=1e6, n_chan=1)                               # sigma = 0 and one channel that holds every V
    med = _median_tau(state, dict(img, source=S, kappa=K))
    scale = 2.0 / med
    tau = ctx.transfer(source=S, kappa=K, kappa_scale=scale, **img)[1]
    col = ctx.cube(values=scale * K, **img, **wide)[0]
    err = float(np.max(np.abs(tau - col)))
    print(f"    tau against the one-channel cube of kappa: {err:.2e} of {col.max():.2e}")
    assert col.max() > 1.0 and err <= TOL * col.max()
    # optically thin: I within [thin (1 - tau), thin] of the cube of kappa S
    scale = 5e-4 / float(np.max(tau) / (2.0 / med))
    out = ctx.transfer(source=S, kappa=K, kappa_scale=scale, **img)
    thin = ctx.cube(values=scale * K * S, **img, **wide)[0]
    assert 0.0 < out[1].max() < 1e-3
    slack = 1e-12 * thin.max()
    assert np.all(out[0] <= thin + slack) and np.all(out[0] >= thin * (1.0 - out[1]) - slack)
    assert np.max(np.abs(out[0] - thin)) <= 1e-3 * thin.max() and thin.max() > 0.0
    ctx.close()


def test_determinism(capi):
    import torch
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=31))
    ctx = _ctx(capi, gas, sinks)
    rng = np.random.default_rng(1)
    K, S = rng.uniform(0.0, 2.0, ctx.n), rng.normal(size=ctx.n)
    kw = dict(shape=(40, 37), bounds=((-60.0, -50.0), (55.0, 60.0)), rot=cb.view(40.0, 30.0))
    scale = 3.0 / float(np.median(ctx.transfer(source="u", kappa=K, **kw)[1]))       # the median node has tau = 3
    kw.update(kappa_scale=scale, tau_max=5.0)
    a = ctx.transfer(source="u", kappa=K, **kw)
    assert a[1].max() >= 5.0 and np.isfinite(a[3]).any() and np.isnan(a[3]).any()
    assert np.array_equal(a, ctx.transfer(source="u", kappa=K, **kw), equal_nan=True)                    # a repeated call
    d = ctx.transfer(source="u", kappa=torch.as_tensor(K, device="cuda:0"), device=True, **kw)
    assert isinstance(d, torch.Tensor) and d.is_cuda and np.array_equal(d.cpu().numpy(), a, equal_nan=True)   # host against _dev
    kwr = dict(kw, kappa_scale=scale / float(np.median(ctx.field("rho"))))
    b = ctx.transfer(source=S, kappa="rho", **kwr)
    d = ctx.transfer(source=torch.as_tensor(S, device="cuda:0"), kappa="rho", device=True, **kwr)
    assert np.array_equal(d.cpu().numpy(), b, equal_nan=True) and not np.array_equal(a, b, equal_nan=True)
    # the context's sorted order does not enter: the same upload binned on another grid (another h, another cell order)
    other = capi.Context(device=0, h=1.7 * ctx.params.h)
    other.upload(gas)
    other.set_sinks(sinks)
    other.density()
    assert not np.array_equal(other.field("rho"), ctx.field("rho"))
    kwh = dict(kw, h=float(ctx.params.h))
    assert np.array_equal(other.transfer(source=S, kappa=K, **kwh), ctx.transfer(source=S, kappa=K, **kwh), equal_nan=True)
    other.close()
    # and after a few steps the image of the state in place is bitwise that of a fresh context holding that state
    ctx.run(3, 1e-3)
    st = {k: ctx.field(k) for k in capi.FIELDS[:9]}
    c = ctx.transfer(source="u", kappa=K, **kw)
    assert not np.array_equal(a, c, equal_nan=True)
    fresh = _ctx(capi, st, sinks, density=False)
    assert np.array_equal(fresh.transfer(source="u", kappa=K, **kw), c, equal_nan=True)
    fresh.close()
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    kw = dict(shape=(33, 31), bounds=((-50.0, -50.0), (50.0, 50.0)), rot=cb.view(40.0, 30.0), kappa_scale=1e7)
    runs = []
    for with_call in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_call:
                before = {k: ctx.field(k) for k in ("x", "vx", "rho", "c", "ax", "du")}
                ctx.transfer(source="u", kappa="rho", **kw)
                ctx.transfer(source=before["rho"], h=1.0, clip=((0, 0, -1), (50, 50, 1)), tau_max=3.0, **kw)
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
    out = np.full(4 * 4 * 3, 7.0)
    vals = np.ones(ctx.n)

    def call(d, out_len=48, o=out, desc=True, s=None, k=None, fn=lib.sph_transfer):
        return fn(ctx._h, C.byref(d) if desc else None, None if s is None else s.ctypes.data, None if k is None else k.ctypes.data,
                  None if o is None else o.ctypes.data, out_len)

    def good(**kw):
        return capi.transfer_desc((4, 3), ((-10.0, -10.0), (10.0, 10.0)), kappa_scale=1e5, **kw)
    assert call(good()) == 0 and not (out == 7.0).any()
    assert call(good(source=vals, kappa=vals), s=vals, k=vals) == 0
    out[:] = 7.0
    bad = []
    for field, value in (("n_u", 0), ("n_v", -1), ("kappa_scale", -1e-3), ("kappa_scale", np.inf), ("kappa_scale", np.nan),
                         ("tau_surface", 0.0), ("tau_surface", -1.0), ("tau_surface", np.nan), ("tau_max", 0.0), ("tau_max", -2.0),
                         ("tau_max", np.nan), ("background", np.inf), ("background", np.nan), ("reserved", 1), ("flags", 1),
                         ("h", -1.0), ("h", np.nan), ("h", np.inf), ("source", capi.TRANSFER_ONE - 1), ("source", len(capi.FIELDS)),
                         ("kappa", -3), ("kappa", 99)):
        d = good()
        setattr(d, field, value)
        bad.append((f"{field}={value}", d))
    for field, idx, value in (("lo", 0, 11.0), ("hi", 1, -11.0), ("lo", 1, np.nan), ("hi", 0, np.inf), ("clip_lo", 2, np.nan),
                              ("clip_hi", 0, np.nan), ("centre", 1, np.inf), ("centre", 2, np.nan)):
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
    assert call(good(), out_len=47) == SPH_ERR_ARG and call(good(), out_len=12) == SPH_ERR_ARG
    assert call(good(), o=None) == SPH_ERR_ARG and call(good(), desc=False) == SPH_ERR_ARG
    # a pointer exactly when its selector is TRANSFER_VALUES
    assert call(good(), s=vals) == SPH_ERR_ARG and call(good(), k=vals) == SPH_ERR_ARG
    assert call(good(source=vals)) == SPH_ERR_ARG and call(good(kappa=vals)) == SPH_ERR_ARG
    assert call(good(source=vals, kappa=vals), s=vals) == SPH_ERR_ARG
    # a bad K or S among the selected; the same value outside the clip box is not looked at
    x = ctx.field("x")
    j = int(np.argmax(x))
    inside = ((-np.inf,) * 3, (float(x[j]) - 1e-9, np.inf, np.inf))
    for what, value, ok_outside in (("kappa", -1e-300, True), ("kappa", np.nan, True), ("kappa", np.inf, True), ("source", np.nan, True),
                                    ("source", -np.inf, True), ("source", -5.0, None), ("kappa", 0.0, None)):
        v = vals.copy()
        v[j] = value
        d = good(**{what: v})
        st = call(d, **{what[0]: v})
        assert st == (0 if ok_outside is None else SPH_ERR_ARG), (what, value, st)
        if ok_outside:
            d.clip_hi[0] = inside[1][0]
            assert call(d, **{what[0]: v}) == 0, (what, value)
    out[:] = 7.0
    v = vals.copy(); v[j] = -1.0
    assert call(good(kappa=v), k=v) == SPH_ERR_ARG and (out == 7.0).all()          # nothing was written
    assert lib.sph_transfer_dev(ctx._h, C.byref(good()), None, None, None, 48) == SPH_ERR_ARG
    # a stale field: refused exactly where sph_download_field refuses it
    for name in ("rho", "c", "ax"):
        with pytest.raises(capi.SphError) as ei:
            ctx.field(name)
        assert ei.value.status == SPH_ERR_STATE
        assert call(good(source=name)) == SPH_ERR_STATE and call(good(kappa=name)) == SPH_ERR_STATE, name
    with pytest.raises(capi.SphError) as ei:
        ctx.field("h")                                                 # a fixed-h context has no h field
    assert ei.value.status == SPH_ERR_STATE and call(good(kappa="h")) == SPH_ERR_STATE
    ctx.density()
    assert call(good(source="rho", kappa="c")) == 0 and call(good(source="ax")) == SPH_ERR_STATE
    # a rotation within 1e-12 of orthonormal is taken
    d = good()
    d.rot[:] = (cb.view(33.0, 21.0, 5.0) * (1.0 + 2e-13)).reshape(9).tolist()
    assert call(d) == 0
    with pytest.raises(ValueError):
        ctx.transfer((4, 3), ((-1, -1), (1, 1)), source=np.zeros(ctx.n + 1))
    ctx.close()


@pytest.mark.timeout(600)
def test_million_particles(capi):
    """10^6 particles at 40 degrees on 256 x 256 nodes: 256 random nodes and the minor axis against the brute force, and a
    physical check.  The disc is given u = u0 (R / 100)^-1 (hot inside) and made opaque (median tau 20).  An opaque line of
    sight shows the upper layer it meets first, S_1 (1 - e^-tau_1) of the two-sheet formula with e^-tau_1 ~ 0, at height z_s
    above the midplane; the ray reaches that layer z_s tan(i) before its midplane crossing, which on the near side of the
    minor axis (the half tilted towards the observer) lies further out (cooler) and on the far side further in (hotter).  So
    at equal distance from the star the far half is brighter than the near half."""
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(10**6, seed=5))
    gas = dict(gas)
    R = np.hypot(gas["x"], gas["y"])
    gas["u"] = 0.25 * 100.0 / R
    ctx = _ctx(capi, gas, sinks, variable=True, density=False)
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    m, h, u = gas["m"], gas["h"], gas["u"]
    rot = cb.view(40.0, 0.0)                  # w^ = (0, -sin i, cos i): y > 0 is the near side and lies at v > 0
    n, ext = 256, 300.0
    gu = np.linspace(-ext, ext, n)
    base = dict(rot=rot, source=u, tau_surface=1.0)
    rng = np.random.default_rng(9)
    axis = np.stack([np.full(n, n // 2), np.arange(n)], axis=1)          # the image column nearest u = 0: the minor axis
    pix = np.concatenate([rng.integers(0, n, (256, 2)), axis])
    thin = transfer_ref.transfer_nodes(pos, m, h, gu, gu, pix, **base)
    lit = thin[1] > 0
    kappa_scale = 20.0 / float(np.median(thin[1][lit]))
    kw = dict(base, kappa_scale=kappa_scale, tau_max=30.0, background=0.01)
    got = ctx.transfer((n, n), ((-ext, -ext), (ext, ext)), **kw)
    want = transfer_ref.transfer_nodes(pos, m, h, gu, gu, pix, **kw)
    g = got[:, pix[:, 0], pix[:, 1]]
    for k, name in enumerate(("I", "tau", "T")):
        s, err = float(np.max(np.abs(want[k]))), float(np.max(np.abs(g[k] - want[k])))
        print(f"    {pix.shape[0]} nodes, {name}: max err {err:.3e} of {s:.3e}")
        assert err <= TOL * s, name
    assert np.array_equal(np.isnan(g[3]), np.isnan(want[3])) and np.isfinite(want[3]).sum() > 300
    ok = np.isfinite(want[3])
    assert np.max(np.abs(g[3][ok] - want[3][ok])) <= TOL * np.max(np.abs(want[3][ok]))
    # the physical check on the minor axis, node k (near, v > 0) against its mirror n - 1 - k (far), both opaque
    col = got[:, n // 2, :]
    k = np.arange(n // 2, n)
    both = (col[1][k] >= 10.0) & (col[1][n - 1 - k] >= 10.0)
    near, far = col[0][k][both], col[0][n - 1 - k][both]
    print(f"    minor axis: {int(both.sum())} opaque pairs, mean far / near {float(np.mean(far / near)):.4f}, "
          f"far brighter in {int((far > near).sum())}")
    assert both.sum() >= 60 and np.mean(far / near) > 1.02 and (far > near).sum() >= 0.8 * both.sum()
    # the surface lies in front of the midplane: at the star's distance (D = 0 on u = 0 is the midplane crossing at v = 0)
    # the depth of the tau = 1 surface is that of the upper layer, nearer than the midplane point of the same ray
    vv = gu[k][both]
    assert np.all(col[3][k][both] < -vv * np.tan(np.deg2rad(40.0)))
    ctx.close()


def test_cli_matches_context_transfer(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    out = tmp_path / "img.npz"
    img = dict(shape=(48, 48), bounds=((-60.0, -60.0), (60.0, 60.0)), rot=cb.view(40.0, 30.0), source="u", kappa="rho")
    scale = 5.0 / float(ctx.transfer(**img)[1].max())
    r = subprocess.run([sys.executable, "-m", "summersph_amd.transfer", str(save), "-o", str(out), "--inc", "40", "--pa", "30",
                        "--extent", "120", "--size", "48", "--kappa-scale", repr(scale), "--source", "u", "--kappa", "rho",
                        "--tau-surface", "1", "--tau-max", "30", "--background", "0.1", "--json"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = ctx.transfer(kappa_scale=scale, tau_surface=1.0, tau_max=30.0, background=0.1, **img)
    z = np.load(out)
    assert want[1].max() > 1.0
    for k, name in enumerate(capi.TRANSFER_PLANES):
        assert np.array_equal(z[name], want[k], equal_nan=True), name
    assert np.array_equal(z["rot"], cb.view(40.0, 30.0)) and np.array_equal(z["u_nodes"], np.linspace(-60.0, 60.0, 48))
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["shape"] == [4, 48, 48] and j["pixels_lit"] == int((want[1] > 0).sum())
    assert j["pixels_surface"] == int(np.isfinite(want[3]).sum())
    ctx.close()
