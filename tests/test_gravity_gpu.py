"""GPU: find_forces WITH the Barnes-Hut gas self-gravity term (SPH_FLAG_SELF_GRAVITY), against the
"full_*" fixtures of the real reference and against the CPU oracle's explicit octree walk."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from gpu_support import capi, make_context
from summersph_amd import ic

pytestmark = pytest.mark.gpu


def make_ctx(capi, rows, **kw):
    gas, sinks = ic.split_rows(rows)
    return make_context(capi, gas, sinks, **kw), gas, sinks


@pytest.mark.parametrize("name", ["sod1000_eval", "disc3000_eval", "disc3000ns_eval", "bin2000_eval"])
def test_find_forces_with_gravity_vs_reference_fixture(capi, name):
    g = load_golden(name)
    ctx, gas, sinks = make_ctx(capi, g["ic"], flags=capi.FLAG_SELF_GRAVITY)
    ctx.density(); ctx.forces()
    for f in ("ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), g["full_" + f]) <= 1e-13, f
    # the gravity term on its own scale (it is ~1e-3 of the total in the disc)
    for f in ("ax", "ay", "az"):
        grav = g["full_" + f] - g["sph_" + f]
        mine = ctx.field(f) - g["sph_" + f]
        assert np.max(np.abs(mine - grav)) <= 1e-7 * np.max(np.abs(grav)), f
    assert ctx.next_dt(1e-2) == g["full_dt"][0]
    ctx.close()


@pytest.mark.parametrize("name", ["sod1000_traj", "disc3000_traj"])
def test_full_trajectory_vs_reference_fixture(capi, name):
    g = load_golden(name)
    ctx, gas, sinks = make_ctx(capi, g["ic"], flags=capi.FLAG_SELF_GRAVITY)
    dts, t = [1e-2], 0.0
    for _ in range(5):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt)
    assert dts == list(g["full_dt_seq"])
    for f in "x y z vx vy vz u alpha".split():
        assert rel_err(ctx.field(f), g["full_s5_" + f]) <= 1e-11, f
    ctx.close()


def test_gravity_vs_oracle_tree_walk_100k(capi):
    """the walk itself at scale: self-gravity of a 100k disc, GPU radix-tree walk vs the oracle's octree"""
    from oracle import orc, orc_grav
    rows = ic.keplerian_disc(100000, seed=17, m_disc=0.5)       # heavy disc: gravity matters
    ctx, gas, sinks = make_ctx(capi, rows, flags=capi.FLAG_SELF_GRAVITY)
    ctx.density(); ctx.forces()
    a_full = [ctx.field(f) for f in ("ax", "ay", "az")]
    ref, _, _ = make_ctx(capi, rows)                             # same without the gravity term
    ref.density(); ref.forces()
    t = orc_grav.Tree(gas["x"], gas["y"], gas["z"], gas["m"])
    ga = [np.zeros(100000) for _ in range(3)]
    orc_grav.gravity(t, gas["x"], gas["y"], gas["z"], *ga, nthreads=orc.max_threads())
    for k, f in enumerate(("ax", "ay", "az")):
        mine = a_full[k] - ref.field(f)
        assert np.max(np.abs(mine - ga[k])) <= 1e-9 * np.max(np.abs(ga[k])), f
    ctx.close(); ref.close()


def test_accretion_and_cull_vs_reference_fixture(capi):
    """simulate()'s loop body as it is: self-gravity, accretion by the sink, boundary cull (particle count
    shrinks) -- 3 steps against the real reference"""
    g = load_golden("acc2000_traj")
    ctx, gas, sinks = make_ctx(capi, g["ic"], flags=capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL)
    dts, t, ns = [1e-2], 0.0, [ctx.n]
    for k in range(1, 4):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt); ns.append(ctx.n)
        p = f"full_s{k}_"
        assert ctx.n == g[p + "x"].size
        for f in "x y z vx vy vz u m alpha".split():
            assert rel_err(ctx.field(f), g[p + f]) <= 1e-11, (k, f)
        s = ctx.get_sinks()
        assert abs(s["m"][0] - g[p + "sm"][0]) <= 1e-15 and abs(s["x"][0] - g[p + "sx"][0]) <= 1e-12
        # the survivors keep density, accelerations and rates of the step's last evaluation, as the reference's pack
        # leaves them -- also right after a step that removed particles (step 1: 2000 -> 1996)
        for f in "rho ax ay az du dalpha".split():
            assert rel_err(ctx.field(f), g[p + f]) <= 1e-11, (k, f)
    assert ns == [int(v) for v in g["full_n_seq"]] and ns[1] == ns[0] - 4
    assert dts == list(g["full_dt_seq"])
    ctx.close()


def test_accrete_explicit_call_and_order(capi):
    """explicit call; survivors keep their relative order (pack semantics)"""
    g = load_golden("acc2000_traj")
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    ctx.density()
    removed = ctx.accrete_and_cull()
    assert removed >= 3 and ctx.n == gas["x"].size - removed
    x_new = ctx.field("x")
    keep = np.isin(gas["x"], x_new)
    assert np.array_equal(gas["x"][keep], x_new)
    ctx.density(); ctx.forces()          # the shrunken set evaluates fine
    assert np.all(np.isfinite(ctx.field("ax")))
    ctx.close()


def test_binary_two_sinks_full_loop(capi):
    """two sinks: sink-sink forces and two accretors, simulate()'s loop body for 3 steps against the real reference"""
    g = load_golden("bin2000_traj")
    ctx, gas, sinks = make_ctx(capi, g["ic"], flags=capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL)
    dts, t, ns = [1e-2], 0.0, [ctx.n]
    for k in range(1, 4):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt); ns.append(ctx.n)
        if k in (1, 3):
            p = f"full_s{k}_"
            assert ctx.n == g[p + "x"].size
            for f in "x y z vx vy vz u m alpha".split():
                assert rel_err(ctx.field(f), g[p + f]) <= 1e-11, (k, f)
            s = ctx.get_sinks()
            assert np.max(np.abs(s["m"] - g[p + "sm"])) <= 1e-15 and np.max(np.abs(s["x"] - g[p + "sx"])) <= 1e-12
            assert np.max(np.abs(s["vy"] - g[p + "svy"])) <= 1e-12
    assert ns == [int(v) for v in g["full_n_seq"]]
    assert dts == list(g["full_dt_seq"])
    ctx.close()
    # and without self-gravity / accretion
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    dts, t = [1e-2], 0.0
    for _ in range(3):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt)
    assert dts == list(g["sph_dt_seq"])
    for f in "x y z vx vy vz u alpha".split():
        assert rel_err(ctx.field(f), g["sph_s3_" + f]) <= 1e-11, f
    s = ctx.get_sinks()
    assert np.max(np.abs(s["x"] - g["sph_s3_sx"])) <= 1e-12 and np.max(np.abs(s["vy"] - g["sph_s3_svy"])) <= 1e-12
    ctx.close()


@pytest.mark.parametrize("name,steps,extra", [("disc3000_traj", 5, 0), ("acc2000_traj", 3, "acc")])
def test_reuse_gravity_is_bitwise_neutral(capi, name, steps, extra):
    """SPH_FLAG_REUSE_GRAVITY: the start-of-step evaluation copies the Barnes-Hut term of the previous step's last walk
    (same positions, masses, h, tree) instead of walking again -- same bits, also across steps that remove particles
    (the cache is dropped with the tree)"""
    g = load_golden(name)
    flags = capi.FLAG_SELF_GRAVITY | (capi.FLAG_ACCRETE_CULL if extra == "acc" else 0)
    out = []
    for fl in (flags, flags | capi.FLAG_REUSE_GRAVITY):
        ctx, gas, sinks = make_ctx(capi, g["ic"], flags=fl)
        dts, t = [1e-2], 0.0
        for _ in range(steps):
            dt, t = ctx.step(dts[-1], t)
            dts.append(dt)
        out.append((dts, {f: ctx.field(f) for f in "x y z vx vy vz u alpha ax ay az".split()}, ctx.n))
        ctx.close()
    assert out[0][0] == out[1][0] == list(g["full_dt_seq"])[:steps + 1] and out[0][2] == out[1][2]
    for f in out[0][1]:
        assert np.array_equal(out[0][1][f], out[1][1][f]), f
