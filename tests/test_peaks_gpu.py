"""GPU tests of sph_peaks (include/summersph.h, "density-peak clumps") on the MI355X: parity of labels, counts and table
with the numpy restatement (embedded clumps, a uniform box, LINK_H with variable h, the fixtures, a 10^5 disc), the
friends-of-friends limit against sph_groups itself, exact ties, long hop chains, two blobs joined by a bridge, the merge
decision one ulp either side of its threshold, the adversarial sets of test_groups_gpu.py, the order rule, no side effects
on a running simulation, the device form, the argument errors and the command line."""
import ctypes as C
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gpu_support import capi, clumped_disc, make_context
import peaks_ref
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-13
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
EXACT = ("N", "r_max", "rho_max", "x_dense", "y_dense", "z_dense", "id_dense", "id_min", "S_out", "n_peaks")
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


def _cmp(capi, got, ref, tol=TOL):
    labels, table, ng, counts = got
    rl, rt, rn, rc = ref[:4]
    print("counts", counts, "restatement", rc)
    assert ng == rn and tuple(counts) == tuple(rc)
    assert np.array_equal(labels, rl)
    assert len(table) == rn
    for k, c in enumerate(capi.PEAKS_COLUMNS):
        g, want = table[c], rt[:, k]
        if c in EXACT:
            assert np.array_equal(g, want, equal_nan=True), c
        else:
            err = np.max(np.abs(g - want), initial=0.0)
            print(c, err, tol * _scale(want))
            assert err <= tol * _scale(want), c


def _ref(capi, ctx, link, contrast, n_owned=None, h=False, **kw):
    f = _fields(ctx, h=h and ctx.params.flags & capi.FLAG_VARIABLE_H)
    hh = None if not h else (f["h"] if "h" in f else float(ctx.params.h))
    return peaks_ref.peaks(f, ctx.n if n_owned is None else n_owned, link, contrast=contrast, link_h=h, h=hh, **kw)


def _check(capi, ctx, link, contrast=2.0, n_owned=None, h=False, detail=False, **kw):
    got = ctx.peaks(link, contrast=contrast, link_h=h, **kw)
    ref = _ref(capi, ctx, link, contrast, n_owned, h, detail=detail, **kw)
    _cmp(capi, got, ref)
    return got + ((ref[4],) if detail else ())


def _gas(pos, seed=0, m=1e-6):
    rng = np.random.default_rng(seed)
    n = len(pos)
    mm = np.broadcast_to(np.asarray(m, dtype=np.float64), (n,)).copy()
    return {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": rng.normal(0, 0.1, n),
            "vy": rng.normal(0, 0.1, n), "vz": rng.normal(0, 0.1, n), "u": rng.uniform(0.1, 0.5, n),
            "m": mm, "alpha": np.ones(n)}


# ---- parity ------------------------------------------------------------------------------------------------------------
def test_parity_embedded_clumps(capi):
    gas, sinks, n0, sizes = clumped_disc(20000, 4, 400, 3)
    ctx = _ctx(capi, gas, sinks)
    lab, tab, ng, cnt = _check(capi, ctx, 2.5, contrast=1.2)
    assert cnt[1] > 100 and cnt[2] > 100
    off, own = n0, []
    for s in sizes:                                     # each clump keeps a group of its own in the percolating disc
        vals, c = np.unique(lab[off:off + s], return_counts=True)
        own.append(int(vals[np.argmax(c)]))
        off += s
    assert len(set(own)) == 4 and min(own) >= 0
    _check(capi, ctx, 2.5, contrast=2.0, min_members=5)
    _check(capi, ctx, 1.5, contrast=3.0, rho_min=float(np.median(ctx.field("rho"))))
    ctx.close()


def test_parity_uniform_box(capi):
    gas, _ = ic.split_rows(ic.uniform_box(30000, seed=5))
    ctx = _ctx(capi, gas)
    n = ctx.n
    lo, hi = ctx.bbox()
    sep = float(np.prod(hi - lo) / n) ** (1 / 3)
    _, tab, ng, cnt = _check(capi, ctx, 0.9 * sep)
    assert 100 < ng < n and cnt[1] >= ng
    _check(capi, ctx, 1.3 * sep, contrast=1.5, min_members=5)
    ctx.close()


def test_parity_link_h_variable(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000, seed=7))
    ctx = _ctx(capi, gas, sinks, variable=True)
    _, _, ng, _ = _check(capi, ctx, 0.6, h=True)
    assert ng > 10
    _check(capi, ctx, 0.8, contrast=1.3, h=True, rho_min=float(np.median(ctx.field("rho"))))
    ctx.close()
    fixed = _ctx(capi, ic.split_rows(ic.keplerian_disc(20000, seed=8))[0])
    _check(capi, fixed, 0.7, h=True)                      # params.h for every particle
    fixed.close()


@pytest.mark.parametrize("name", ["disc3000_traj", "bin2000_eval"])
def test_parity_fixtures(capi, name):
    gas, sinks = ic.split_rows(load_golden(name)["ic"])
    ctx = _ctx(capi, gas, sinks)
    _check(capi, ctx, 2.5)
    _check(capi, ctx, 2.5, contrast=1.0)
    _check(capi, ctx, 3.5, contrast=1.5, min_members=3, rho_min=float(np.median(ctx.field("rho"))))
    ctx.close()


def test_parity_1e5_disc(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(100_000, seed=11))
    ctx = _ctx(capi, gas, sinks)
    _, tab, ng, cnt = _check(capi, ctx, 2.0)
    assert cnt[1] > 1000 and cnt[2] > 1000 and np.max(tab["id_dense"]) > 65536
    ctx.close()


# ---- the friends-of-friends limit against sph_groups ---------------------------------------------------------------------
@pytest.mark.parametrize("which", ["box", "disc3000_traj"])
def test_contrast_inf_is_sph_groups_bitwise(capi, which):
    if which == "box":
        gas, sinks = ic.split_rows(ic.uniform_box(30000, seed=21))[0], None
    else:
        gas, sinks = ic.split_rows(load_golden(which)["ic"])
    ctx = _ctx(capi, gas, sinks)
    lo, hi = ctx.bbox()
    link = 0.8 * float(np.prod(hi - lo) / ctx.n) ** (1 / 3) if which == "box" else 1.5
    for kw in ({}, {"min_members": 3}):
        gl, gt, gn = ctx.groups(link, **kw)
        lab, tab, ng, cnt = ctx.peaks(link, contrast=np.inf, **kw)
        assert ng == gn > 1 and np.array_equal(lab, gl)
        for c in capi.GROUPS_COLUMNS:
            assert np.array_equal(tab[c], gt[c], equal_nan=True), c
        assert np.all(tab["S_out"] == 0)
    ctx.close()


# ---- ties, long chains, a bridge, the decision edge ---------------------------------------------------------------------
def test_ties_go_to_the_smaller_id(capi):
    k = np.arange(1000)
    a = np.stack([40.0 * (k % 32), 40.0 * (k // 32), np.zeros(1000)], axis=1)
    pos = np.empty((2000, 3))
    pos[0::2] = a
    pos[1::2] = a + [0.5, 0.0, 0.0]
    ctx = _ctx(capi, _gas(pos, 3))
    rho = ctx.field("rho")
    assert np.array_equal(rho[0::2], rho[1::2])           # equal masses, a symmetric pair: exactly equal
    for contrast in (1.0, 2.0):
        lab, tab, ng, cnt = _check(capi, ctx, 0.75, contrast=contrast)
        assert ng == 1000 and cnt == (1000, 1000, 0)
        assert np.all(tab["N"] == 2) and np.all(tab["id_dense"] % 2 == 0) and np.array_equal(lab[0::2], lab[1::2])
    ctx.close()


def test_long_hop_chains(capi):
    n = 20000
    step = 0.05 * 0.9999 ** np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(step[:-1])])
    pos = np.stack([x, np.zeros(n), np.zeros(n)], axis=1)
    ctx = _ctx(capi, _gas(pos, 5))
    lab, tab, ng, cnt, d = _check(capi, ctx, 0.075, contrast=1.0, detail=True)
    longest = int(np.max(peaks_ref.chain_lengths(d["next"], d["order"])))
    print("longest chain", longest)
    assert longest >= 1000
    ctx.close()


def _bridge():
    rng = np.random.default_rng(7)
    blobs = []
    for cx in (-15.0, 15.0):
        p = rng.normal(0, 2.5, (3000, 3))
        p = p[np.sum(p * p, axis=1) < 36.0][:1500]
        blobs.append(p + [cx, 0, 0])
    xs = np.arange(-10.0, 10.0001, 0.5)
    bridge = np.stack([xs, np.zeros(xs.size), np.zeros(xs.size)], axis=1)
    return np.concatenate(blobs + [bridge])


def test_bridge_between_two_blobs(capi):
    ctx = _ctx(capi, _gas(_bridge(), 7))
    lab, tab, ng, _ = _check(capi, ctx, 2.0, contrast=2.0, min_members=10)
    assert ng == 2 and lab[0] != lab[1500] and min(lab[0], lab[1500]) >= 0
    lab, tab, ng, _ = _check(capi, ctx, 2.0, contrast=np.inf, min_members=10)
    assert ng == 1
    assert ctx.groups(2.0, min_members=10)[2] == 1
    ctx.close()


def test_merge_decision_flips_at_its_threshold(capi):
    # five particles on a line, two peaks (the ends) and one saddle: one edge, so the merge is decided by it alone
    flips = 0
    for masses in ([5.0, 1.0, 0.5, 1.0, 4.0], [7.0, 1.0, 0.4, 1.5, 3.0], [6.0, 2.0, 0.3, 1.0, 4.5]):
        pos = np.stack([2.0 * np.arange(5), np.zeros(5), np.zeros(5)], axis=1)
        ctx = _ctx(capi, _gas(pos, 9, m=np.array(masses) * 1e-6))
        got = ctx.peaks(2.2, contrast=1.0)
        ref = _ref(capi, ctx, 2.2, 1.0, detail=True)
        _cmp(capi, got, ref)
        d = ref[4]
        assert got[3] == (2, 2, 1) and len(d["es"]) == 1
        rho = ctx.field("rho")
        S, low = float(d["es"][0]), float(min(rho[0], rho[4]))
        c0 = low / S
        for c in (np.nextafter(c0, 0.0), c0, np.nextafter(c0, np.inf)):
            merged = bool(low < np.float64(c) * np.float64(S))
            lab, tab, ng, cnt = _check(capi, ctx, 2.2, contrast=float(c))
            print("contrast", repr(float(c)), "merged", merged, "groups", ng)
            assert ng == (1 if merged else 2)
        assert not low < np.nextafter(c0, 0.0) * S        # below the quotient the product cannot pass rho
        flips += bool(low < np.nextafter(c0, np.inf) * S)
        ctx.close()
    assert flips >= 1


# ---- adversarial, as test_groups_gpu.py ----------------------------------------------------------------------------------
def test_pairs_at_exactly_b(capi):
    b = 0.75
    rows = []
    for k in range(60):
        x0 = 10.0 * k + 0.5
        for j, dx in enumerate((np.nextafter(x0 + b, 0.0) - x0, b, np.nextafter(x0 + b, np.inf) - x0)):
            rows += [(x0, 10.0 * j, 0.0), (x0 + dx, 10.0 * j, 0.0)]
    pos = np.array(rows)
    rng = np.random.default_rng(2)
    for k in range(300):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        p0 = np.array([1000.0 + 10 * k, 500.0, 0.0])
        pos = np.vstack([pos, p0, p0 + v * b * (1 + rng.integers(-3, 4) * 2.2e-16)])
    ctx = _ctx(capi, _gas(pos, 2))
    lab, _, ng, _ = _check(capi, ctx, b, contrast=np.inf)
    x = ctx.field("x")
    for k in range(60):
        base = 6 * k
        dxs = [x[base + 2 * j + 1] - x[base + 2 * j] for j in range(3)]
        assert dxs[0] < b and dxs[1] == b and dxs[2] > b
        assert lab[base] == lab[base + 1] and lab[base + 2] != lab[base + 3] and lab[base + 4] != lab[base + 5]
    _check(capi, ctx, b, contrast=1.0)
    ctx.close()


def test_coincident_particles(capi):
    rng = np.random.default_rng(4)
    pos = np.vstack([np.tile([[3.0, 4.0, 5.0]], (200, 1)), rng.uniform(-50, 50, (300, 3))])
    ctx = _ctx(capi, _gas(pos, 4))
    lab, tab, ng, cnt = _check(capi, ctx, 0.01)
    assert tab["N"][0] == 200 and np.all(lab[:200] == 0) and tab["r_max"][0] == 0.0 and tab["n_peaks"][0] == 1
    ctx.close()


def test_link_larger_than_the_box(capi):
    rng = np.random.default_rng(6)
    ctx = _ctx(capi, _gas(rng.uniform(0, 1, (4000, 3)), 6))
    lab, tab, ng, cnt = _check(capi, ctx, 10.0)           # one cell holds everything: every pair is a neighbour pair
    assert ng == 1 and tab["N"][0] == 4000 and cnt == (1, 1, 0)
    ctx.close()


def test_clumps_far_apart(capi):
    rng = np.random.default_rng(8)
    a = rng.normal(0, 0.3, (3000, 3))
    pos = np.vstack([a, a[:2000] + [1e4, 0, 0], a[:1000] + [0, -1e4, 3e3]])
    ctx = _ctx(capi, _gas(pos, 8))
    lab, tab, ng, _ = _check(capi, ctx, 0.05, min_members=2)
    assert ng > 3
    ctx.close()


def test_ghosts_are_excluded(capi):
    gas, _ = ic.split_rows(ic.uniform_box(30000, seed=9))
    ctx = _ctx(capi, gas, density=False)
    ctx.set_owned(25000)
    ctx.density()
    lab, _, ng, _ = _check(capi, ctx, 1.2, n_owned=25000)
    assert np.all(lab[25000:] == -1) and ng > 0
    ctx.close()


def test_after_accrete_and_cull(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=12))
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])
    ctx = _ctx(capi, gas, sinks)
    ctx.forces()
    assert ctx.accrete_and_cull() > 0
    assert ctx.n < 20000
    _check(capi, ctx, 2.0)
    ctx.close()


def test_clip_min_members_peak_min_max_groups_empty(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=13))
    ctx = _ctx(capi, gas, sinks)
    clip = ((-30.0, -30.0, -2.0), (30.0, 30.0, 2.0))
    lab, _, _, _ = _check(capi, ctx, 2.0, clip=clip)
    x, y, z = ctx.field("x"), ctx.field("y"), ctx.field("z")
    assert np.all(lab[(np.abs(x) >= 30) | (np.abs(y) >= 30) | (np.abs(z) >= 2)] == -1)
    _check(capi, ctx, 2.0, min_members=4)
    full_l, full_t, full_n, full_c = ctx.peaks(2.0)
    pm = float(np.median(full_t["rho_max"]))
    lab, tab, ng, cnt = _check(capi, ctx, 2.0, peak_min=pm)
    assert 0 < ng < full_n and np.all(tab["rho_max"] >= pm) and cnt[1:] == full_c[1:]
    lab, tab, ng, cnt = ctx.peaks(2.0, max_groups=7)
    assert ng == full_n > 7 and len(tab) == 7 and np.array_equal(lab, full_l) and cnt == full_c
    assert np.array_equal(tab.view(np.float64), full_t[:7].view(np.float64), equal_nan=True)
    lab, tab, ng, cnt = ctx.peaks(2.0, max_groups=0)
    assert tab is None and ng == full_n and np.array_equal(lab, full_l)
    lab, tab, ng, cnt = ctx.peaks(2.0, labels=False, max_groups=0)
    assert lab is None and cnt == full_c
    lab, tab, ng, cnt = ctx.peaks(2.0, rho_min=np.inf)
    assert ng == 0 and len(tab) == 0 and np.all(lab == -1) and cnt == (0, 0, 0)
    lab, tab, ng, cnt = ctx.peaks(2.0, clip=((1e9,) * 3, (2e9,) * 3))
    assert ng == 0 and np.all(lab == -1)
    lab, tab, ng, cnt = ctx.peaks(2.0, peak_min=np.inf)
    assert ng == 0 and np.all(lab == -1) and cnt[1:] == full_c[1:]
    ctx.close()


# ---- order rule --------------------------------------------------------------------------------------------------------
def _raw(ctx, link, **kw):
    lab, tab, ng, cnt = ctx.peaks(link, **kw)
    return lab, tab.view(np.float64).reshape(-1, 23).copy(), ng, cnt


def _same(a, b):
    return a[2] == b[2] and a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def test_order_rule_bitwise(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(40000, seed=15))
    a = _ctx(capi, gas, sinks)
    ra = _raw(a, 2.0)
    assert _same(ra, _raw(a, 2.0))                        # repeated calls (the second finds the scratch sized)
    a.groups(1.0)                                         # another pass used the scratch in between
    assert _same(ra, _raw(a, 2.0))
    rho_a = a.field("rho")
    for flags in (capi.FLAG_HASHED_GRID, capi.FLAG_NO_LDS_TILES):
        c = _ctx(capi, gas, sinks, flags=flags)
        if flags == capi.FLAG_HASHED_GRID:
            assert c.grid_info().kind == 1
        assert np.array_equal(c.field("rho"), rho_a)      # the same density sums: then the same clumps, bit for bit
        assert _same(ra, _raw(c, 2.0))
        c.close()
    a.forces()                                            # another evaluation in place: the same
    assert _same(ra, _raw(a, 2.0))
    # a permuted upload: rho comes from density sums in another neighbour order, and every decision here compares rho,
    # so the permuted context is held to the restatement on its own fields; where its rho is bitwise the permuted rho,
    # the partition is the same through the permutation
    perm = np.random.default_rng(16).permutation(gas["x"].size)
    p = _ctx(capi, {k: v[perm] for k, v in gas.items()}, sinks)
    lp, tp, npg, cp = _check(capi, p, 2.0)
    if np.array_equal(p.field("rho"), rho_a[perm]):
        # ids change, so ties may break differently; with no tie among the peaks the partition is the same
        if np.unique(rho_a).size == rho_a.size:
            assert npg == ra[2] and cp == ra[3]
            pairs = np.unique(np.stack([ra[0][perm], lp], axis=1), axis=0)
            assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
    a.close(); p.close()


# ---- side effects, device form, errors, command line --------------------------------------------------------------------
def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    runs = []
    for with_peaks in (False, True):
        ctx = _ctx(capi, gas, sinks, density=False)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            if with_peaks:
                ctx.peaks(2.0, min_members=2)
                ctx.peaks(0.8, contrast=1.5, link_h=True, max_groups=3)
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
    for kw in ({}, {"min_members": 3, "rho_min": float(np.median(ctx.field("rho"))), "contrast": 1.3}, {"link_h": True}):
        link = 0.8 if kw.get("link_h") else 2.0
        lab, tab, ng, cnt = _raw(ctx, link, **kw)
        dl, dtab, dn, dc = ctx.peaks(link, max_groups=50, device=True, **kw)
        assert isinstance(dl, torch.Tensor) and dn == ng and tuple(dc.cpu().tolist()) == cnt
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
    tab = np.empty((10, capi.PEAKS_NCOL))
    cnt = (C.c_int64 * 3)()

    def call(d, labels=lab, nl=n, table=tab, mg=10, count=True):
        return lib.sph_peaks(ctx._h, None if d is None else C.byref(d), None if labels is None else labels.ctypes.data, nl,
                             None if table is None else table.ctypes.data, mg, cnt if count else None)

    assert call(capi.peaks_desc(1.0)) == SPH_ERR_STATE                   # rho stale
    ctx.density()
    assert call(capi.peaks_desc(1.0)) == 0
    assert call(None) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0), count=False) == SPH_ERR_ARG
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(capi.peaks_desc(bad)) == SPH_ERR_ARG, bad
    for bad in (0.999, 0.0, -np.inf, np.nan):
        assert call(capi.peaks_desc(1.0, contrast=bad)) == SPH_ERR_ARG, bad
    assert call(capi.peaks_desc(1.0, contrast=1.0)) == 0 and call(capi.peaks_desc(1.0, contrast=np.inf)) == 0
    assert call(capi.peaks_desc(1.0, peak_min=np.nan)) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0, rho_min=np.nan)) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0, clip=((np.nan, 0, 0), (1, 1, 1)))) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0, clip=((0, 0, 0), (1, np.nan, 1)))) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0, min_members=0)) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0), nl=n - 1) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0), mg=-1) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0), mg=0) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0), table=None, mg=-1) == SPH_ERR_ARG
    d = capi.peaks_desc(1.0); d.flags = 2
    assert call(d) == SPH_ERR_ARG
    d = capi.peaks_desc(1.0); d.reserved = 1
    assert call(d) == SPH_ERR_ARG
    assert lib.sph_peaks(None, C.byref(capi.peaks_desc(1.0)), None, 0, None, 0, cnt) == SPH_ERR_ARG
    assert call(capi.peaks_desc(1.0), labels=None, nl=0, table=None, mg=0) == 0 and cnt[0] > 0
    # LINK_H with a bad h on a selected particle (variable h): host form refuses, device form reports counts[0] == -1
    gv, sv = ic.split_rows(ic.keplerian_disc_var(3000, seed=38))
    v = _ctx(capi, gv, sv, variable=True)
    h = v.field("h")
    h[17] = -1.0
    v.upload_field("h", h)
    v.density()
    hv = v.field("h")
    if hv[17] <= 0:                                     # the density pass keeps an uploaded h only where it iterates
        with pytest.raises(capi.SphError) as e:
            v.peaks(0.5, link_h=True)
        assert e.value.status == SPH_ERR_STATE
        dl, _, dn, dc = v.peaks(0.5, link_h=True, device=True, max_groups=4)
        assert dn == -1 and bool((dl == -1).all())
        assert v.peaks(0.5, link_h=True, clip=((v.field("x")[17] + 1e-9, -np.inf, -np.inf), (np.inf,) * 3))[2] >= 0
    v.close()
    ctx.peaks(1.0)                                        # still usable
    ctx.close()


def test_cli_matches_context_peaks(capi, tmp_path):
    gas, sinks = ic.split_rows(ic.keplerian_disc(5000, seed=41))
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "p.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.peaks", str(save), "-o", str(out), "--link", "2.0",
                        "--contrast", "1.5", "--min-members", "2", "--json", "--top", "3", "--csv", str(tmp_path / "p.csv")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = _ctx(capi, g2, s2)
    lab, tab, ng, cnt = ctx.peaks(2.0, contrast=1.5, min_members=2)
    assert int(z["n_groups"]) == ng and np.array_equal(z["labels"], lab) and tuple(z["counts"].tolist()) == cnt
    for c in capi.PEAKS_COLUMNS:
        assert np.array_equal(z[c], tab[c], equal_nan=True), c
    assert float(z["desc_contrast"]) == 1.5
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["n_groups"] == ng and len(j["table"]) == min(3, ng) and j["counts"]["n_raw_peaks"] == cnt[1]
    assert (tmp_path / "p.csv").exists()
    ctx.close()
