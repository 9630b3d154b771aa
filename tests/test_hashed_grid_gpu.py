"""The hashed cell table (grid.hip, SPH_FLAG_HASHED_GRID) on the GPU.

* far-apart particle groups, which the dense table cannot index (fixed h: SPH_ERR_GRID before; variable h: cells widened to
  many smoothing lengths), evaluate and step, against the CPU oracles;
* a forced hashed table gives bitwise the results of the dense one: the same GridDesc, the same sorted order and the same
  lower-bound answers, hence the same lists, tiles and summation order;
* two 5e5-particle discs far apart in one context against each disc alone.
"""
import threading
import time

import numpy as np
import pytest

from conftest import load_golden, rel_err
from summersph_amd import capi, ic

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

EVAL_TOL = 1e-13
VAR_TOL = 1e-13                      # tests/test_parity_var_gpu.py: one evaluation; h after update_h 1e-12
SHIFT = 1.0e4                        # AU, on every axis
STATE = "x y z vx vy vz u m alpha".split()
DERIVED = "rho P c ax ay az du dalpha".split()


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.load()


def shifted(gas, sinks, d):
    g2 = {k: v.copy() for k, v in gas.items()}
    s2 = {k: v.copy() for k, v in sinks.items()}
    for a in "xyz":
        g2[a] = g2[a] + d
        s2[a] = s2[a] + d
    return g2, s2


def cat(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a if k in b}


def far_pair(rows, d=SHIFT):
    gas, sinks = ic.split_rows(rows)
    g2, s2 = shifted(gas, sinks, d)
    return gas, g2, cat(gas, g2), cat(sinks, s2)


def make(gas, sinks, extra_flags=0, variable=False):
    p = capi.default_params(variable)
    p.flags |= extra_flags
    ctx = capi.Context(params=p, device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    return ctx


def state_of(ctx, fields):
    return {f: ctx.field(f) for f in fields}


def check_halves(ctx, n1, sinks_all, tol=EVAL_TOL):
    """each half of the far pair against the oracle of that half with every sink"""
    from oracle import orc
    full = state_of(ctx, STATE + DERIVED)
    for lo, hi in ((0, n1), (n1, full["x"].size)):
        gas = {k: full[k][lo:hi] for k in STATE}
        o = orc.Oracle(gas, sinks_all, nthreads=orc.max_threads())
        o.evaluate()
        for f in DERIVED:
            assert rel_err(full[f][lo:hi], getattr(o, f)) <= tol, (lo, f, rel_err(full[f][lo:hi], getattr(o, f)))


# ---- 1. far clusters, fixed h -----------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, capi.FLAG_NO_LDS_TILES, capi.FLAG_NO_WHOLE_TILE])
def test_far_clusters_fixed_h_vs_oracle(extra):
    g = load_golden("disc3000_eval")
    gas, _, both, sinks_all = far_pair(g["ic"])
    n1 = gas["x"].size
    ctx = make(both, sinks_all, extra)
    ctx.density(); ctx.forces()                      # SPH_ERR_GRID without the hashed table (2000^3 cells)
    gi = ctx.grid_info()
    assert gi.kind == 1 and gi.index_cells > 2.0 ** 31 and 0 < gi.occupied_cells < both["x"].size
    assert ctx.stats().n_cells == gi.occupied_cells
    check_halves(ctx, n1, sinks_all)
    dt, t = 1e-2, 0.0
    syncs = None
    for k in range(5):
        dt, t = ctx.step(dt, t)
        if k == 1:
            syncs = ctx.stats().host_syncs
    assert ctx.stats().host_syncs == syncs, "the hashed fixed-h steady state waits for the host"
    assert ctx.grid_info().kind == 1
    # the stepped state, evaluated afresh, against the oracles of the downloaded state
    s = ctx.get_sinks()
    ctx.density(); ctx.forces()
    check_halves(ctx, n1, {k: s[k] for k in "x y z vx vy vz m".split()})
    ctx.close()


# ---- 2. separated clusters, variable h ------------------------------------------------------------------
def test_separated_clusters_variable_h_vs_oracle():
    from oracle import orc, orc_v
    rows = ic.keplerian_disc_var(3000, seed=5)
    gas, sinks = ic.split_rows(rows)
    d = 4000.0
    g2, s2 = shifted(gas, sinks, d)
    both, sinks_all = cat(gas, g2), cat(sinks, s2)
    ext = [both[a].max() - both[a].min() for a in "xyz"]
    e = 2.0 * both["h"].mean()
    assert np.prod([np.floor(x / e) + 1 for x in ext]) > 2.0 ** 27           # the dense path widened the cells here
    eo = 2.0 * both["h"].max()
    assert np.prod([np.floor(x / eo) + 1 for x in ext]) <= 5e7               # the oracle's own grid stays small
    ctx = make(both, sinks_all, variable=True)
    o = orc_v.OracleV(both, sinks_all, nthreads=orc.max_threads())
    ctx.density(); ctx.forces(); o.evaluate()
    assert ctx.grid_info().kind == 1
    for f in ("rho", "omega", "ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), getattr(o, f)) <= VAR_TOL, f
    assert ctx.next_dt(1e-2) == o.next_dt(1e-2)
    ctx.update_h(); o.update_h()
    assert rel_err(ctx.field("h"), o.h) <= 1e-12
    # a few steps (with calc_smoothing after each) against the oracle's loop body
    dt = 1e-2
    for _ in range(2):
        dt_gpu, _t = ctx.step(dt)
        o.step(dt)
        dt = dt_gpu
    for f in "x y z vx vy vz u alpha h".split():
        assert rel_err(ctx.field(f), getattr(o, f)) <= 1e-10, f
    assert ctx.grid_info().kind == 1
    ctx.close()


def test_far_clusters_variable_h_steps():
    rows = ic.keplerian_disc_var(3000, seed=6)
    gas, sinks = ic.split_rows(rows)
    g2, s2 = shifted(gas, sinks, SHIFT)
    ctx = make(cat(gas, g2), cat(sinks, s2), variable=True)
    dt, t = 1e-2, 0.0
    for _ in range(3):
        dt, t = ctx.step(dt, t)
    assert ctx.grid_info().kind == 1
    for f in ("x", "rho", "h", "ax", "du"):
        assert np.all(np.isfinite(ctx.field(f))), f
    assert np.all(ctx.field("rho") > 0)
    ctx.close()


# ---- 3. forced hashed == dense, bit for bit ---------------------------------------------------------------
def run_pair(gas, sinks, flags, steps, variable=False, fields=None):
    out = []
    for forced in (0, capi.FLAG_HASHED_GRID):
        ctx = make(gas, sinks, flags | forced, variable)
        dt, t = 1e-2, 0.0
        dts = []
        for _ in range(steps):
            dt, t = ctx.step(dt, t)
            dts.append(dt)
        assert ctx.grid_info().kind == (1 if forced else 0)
        fl = fields or (capi.FIELDS if variable else capi.FIELDS[:17])
        res = {f: ctx.field(f) for f in fl}
        res["dts"] = np.array(dts)
        sk = ctx.get_sinks()
        for k in ("x", "y", "z", "vx", "vy", "vz", "m"):
            res["sink_" + k] = sk[k]
        out.append(res)
        ctx.close()
    a, b = out
    assert a.keys() == b.keys()
    for f in a:
        assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("extra", [0, capi.FLAG_NO_LDS_TILES, capi.FLAG_NO_WHOLE_TILE])
def test_forced_hashed_is_bitwise_dense_fixed_h(extra):
    gas, sinks = ic.split_rows(ic.keplerian_disc(60000, seed=11))
    run_pair(gas, sinks, extra, 4)


def test_forced_hashed_is_bitwise_dense_variable_h():
    # the re-flag pass (default) and the update_h fallback walk (its cell walk reads the table)
    gas, sinks = ic.split_rows(ic.keplerian_disc_var(20000, seed=12))
    run_pair(gas, sinks, 0, 4, variable=True)
    run_pair(gas, sinks, capi.FLAG_NO_REFLAG, 2, variable=True)


def test_forced_hashed_is_bitwise_dense_full_loop():
    gas, sinks = ic.split_rows(ic.keplerian_disc(30000, seed=13))
    run_pair(gas, sinks, capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL, 4)


def test_forced_hashed_is_bitwise_dense_sink_creation():
    g = load_golden("discv3000_traj")
    gas, sinks = ic.split_rows(g["ic"])
    run_pair(gas, sinks, capi.FLAG_SINK_CREATION, 4, variable=True)


def test_forced_hashed_is_bitwise_dense_two_rank_native_loop():
    from summersph_amd import halo
    from summersph_amd.dist import slab_bounds
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=14))
    world = 2

    def run(flags):
        hub = halo.Hub(world)
        bounds = slab_bounds(gas["x"], world)
        owner = np.searchsorted(bounds, gas["x"], side="right")
        out, errs = [None] * world, []

        def worker(rank):
            try:
                p = capi.default_params(False)
                p.flags |= flags
                ctx = capi.Context(params=p, device=0)
                h = halo.Halo.inproc(ctx, hub, rank, world)
                sel = owner == rank
                mine = {k: v[sel] for k, v in gas.items()}
                mine["gid"] = np.nonzero(sel)[0]
                ctx.set_sinks(sinks)
                h.set_slabs(bounds, 2)
                h.upload(mine)
                dt, t = 1e-2, 0.0
                for _ in range(4):
                    dt, t = h.run(1, dt, t)
                out[rank] = {"state": h.download(), "kind": ctx.grid_info().kind, "dt": dt}
                h.close(); ctx.close()
            except Exception as e:      # noqa: BLE001 -- reported below
                errs.append((rank, repr(e)))

        th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        hub.close()
        assert not errs, errs
        return out

    a, b = run(0), run(capi.FLAG_HASHED_GRID)
    for r in range(world):
        assert a[r]["kind"] == 0 and b[r]["kind"] == 1
        assert a[r]["dt"] == b[r]["dt"]
        sa, sb = a[r]["state"], b[r]["state"]
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), (r, k)


# ---- 4. at scale --------------------------------------------------------------------------------------------
def test_two_far_discs_at_scale():
    rows = ic.keplerian_disc(500000, seed=15)
    gas, g2, both, sinks_all = far_pair(rows)
    n1 = gas["x"].size

    def timed_steps(ctx, k=3):
        dt, t = 1e-3, 0.0
        ctx.step(dt, t)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            dt, t = ctx.step(dt, t)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    ctx = make(both, sinks_all)
    ctx.density(); ctx.forces()
    assert ctx.grid_info().kind == 1
    got = state_of(ctx, ("rho", "ax", "ay", "az"))
    ms_pair = timed_steps(ctx)
    ctx.close()
    ms_alone = []
    for lo, hi, half in ((0, n1, gas), (n1, 2 * n1, g2)):
        c1 = make(half, sinks_all)
        c1.density(); c1.forces()
        assert c1.grid_info().kind == 0
        for f in ("rho", "ax", "ay", "az"):
            err = rel_err(got[f][lo:hi], c1.field(f))
            assert err <= 1e-12, (lo, f, err)
        ms_alone.append(timed_steps(c1))
        c1.close()
    print(f"two discs of {n1} particles 1e4 AU apart: hashed {ms_pair:.3f} ms/step; each alone (dense) "
          f"{ms_alone[0]:.3f} + {ms_alone[1]:.3f} ms/step")
