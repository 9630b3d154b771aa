"""GPU parity tests: the HIP path, called through the C ABI, against
  (1) the golden fixtures dumped from the real reference (tests/golden), and
  (2) the CPU oracle (oracle/sph_oracle.c, itself pinned to those fixtures) on seeded inputs.

Tolerances (fp64, relative to each field's maximum magnitude).  The pair terms are written in
the reference's expression order; what differs is the summation order over neighbours and FMA
contraction, so errors are a few 1e-16 per term:
    single evaluation      1e-13  (rho, P, c, a, du, dalpha)
    5-step trajectories    1e-11  (errors compound through the integrator)
    40-step trajectory     1e-9
and the adaptive-dt decision sequence must be IDENTICAL.
"""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from gpu_support import capi, make_context
from summersph_amd import ic

pytestmark = pytest.mark.gpu

EVAL_TOL = 1e-13


def make_ctx(capi, rows, **kw):
    gas, sinks = ic.split_rows(rows)
    return make_context(capi, gas, sinks, **kw), gas, sinks


@pytest.mark.parametrize("name", ["sod1000_eval", "disc3000_eval", "disc3000ns_eval", "bin2000_eval"])
def test_single_evaluation_vs_reference_fixture(capi, name):
    g = load_golden(name)
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    ctx.density()
    for f in ("rho", "P", "c"):
        assert rel_err(ctx.field(f), g[f]) <= EVAL_TOL, f
    ctx.forces()
    for f in ("ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), g["sph_" + f]) <= EVAL_TOL, f
    s = ctx.get_sinks()
    for f in ("ax", "ay", "az"):
        assert np.max(np.abs(s[f] - g["sph_s" + f])) <= 1e-12 * max(1.0, np.max(np.abs(g["sph_s" + f]))), f
    assert ctx.next_dt(1e-2) == g["sph_dt"][0]
    # state comes back in the caller's order, untouched by the internal cell sort
    for f in "x y z vx vy vz u m".split():
        assert np.array_equal(ctx.field(f), g[f]), f
    ctx.close()


@pytest.mark.parametrize("name,steps", [("sod1000_traj", (1, 5)), ("disc3000_traj", (1, 5))])
def test_trajectory_vs_reference_fixture(capi, name, steps):
    g = load_golden(name)
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    dts = [1e-2]
    t = 0.0
    for k in range(1, max(steps) + 1):
        # unfused call sequence = the body of simulate(), SUMMER_SPH.f90:894-916
        dt = dts[-1]
        ctx.density(); ctx.forces(); ctx.kick(dt); ctx.drift(dt)
        ctx.density(); ctx.forces(); ctx.kick(dt)
        t += dt
        dts.append(ctx.next_dt(dt))
        if k in steps:
            p = f"sph_s{k}_"
            for f in "x y z vx vy vz u alpha rho".split():
                assert rel_err(ctx.field(f), g[p + f]) <= 1e-11, (k, f)
            s = ctx.get_sinks()
            for f in ("x", "y", "vx", "vy"):
                assert np.max(np.abs(s[f] - g[p + "s" + f])) <= 1e-11, (k, f)
    assert dts == list(g["sph_dt_seq"])
    ctx.close()


def test_fused_step_equals_unfused_sequence(capi):
    g = load_golden("disc3000_traj")
    a, _, _ = make_ctx(capi, g["ic"])
    b, _, _ = make_ctx(capi, g["ic"])
    dt_a, t_a = 1e-2, 0.0
    dt_b, t_b = 1e-2, 0.0
    for _ in range(3):
        a.density(); a.forces(); a.kick(dt_a); a.drift(dt_a); a.density(); a.forces(); a.kick(dt_a)
        t_a += dt_a
        dt_a = a.next_dt(dt_a)
        dt_b, t_b = b.step(dt_b, t_b)
    assert (dt_a, t_a) == (dt_b, t_b)
    for f in "x y z vx vy vz u alpha".split():
        assert np.array_equal(a.field(f), b.field(f)), f     # bitwise: same kernels, same order
    c, _, _ = make_ctx(capi, g["ic"])
    dt_c, t_c = c.run(3, 1e-2, 0.0)
    assert (dt_c, t_c) == (dt_b, t_b)
    assert np.array_equal(c.field("x"), b.field("x"))
    a.close(); b.close(); c.close()


def test_long_trajectory_dt_sequence(capi):
    g = load_golden("disc3000_long")
    ctx, _, _ = make_ctx(capi, g["ic"])
    dts, t = [1e-2], 0.0
    for _ in range(40):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt)
    assert dts == list(g["sph_dt_seq"])
    for f in "x y z vx vy vz u alpha".split():
        assert rel_err(ctx.field(f), g["sph_s40_" + f]) <= 1e-9, f
    ctx.close()


def test_reuse_density_flag_is_bitwise_neutral(capi):
    g = load_golden("disc3000_traj")
    a, _, _ = make_ctx(capi, g["ic"])
    b, _, _ = make_ctx(capi, g["ic"], flags=capi.FLAG_REUSE_DENSITY)
    da, db = 1e-2, 1e-2
    for _ in range(3):
        da, _ = a.step(da); db, _ = b.step(db)
    assert da == db
    for f in "x vx u alpha".split():
        assert np.array_equal(a.field(f), b.field(f)), f
    assert b.stats().density_passes < a.stats().density_passes
    a.close(); b.close()


@pytest.mark.parametrize("n,seed", [(20000, 11), (100000, 202)])
def test_disc_vs_oracle(capi, n, seed):
    """BASELINE config 2 shape (100k fixed-h disc) and a smaller one, against the CPU oracle."""
    from oracle import orc
    rows = ic.keplerian_disc(n, seed=seed)
    ctx, gas, sinks = make_ctx(capi, rows)
    o = orc.Oracle(gas, sinks, nthreads=orc.max_threads())
    ctx.density(); ctx.forces()
    o.evaluate()
    for f in ("rho", "P", "c", "ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), getattr(o, f)) <= EVAL_TOL, f
    st = ctx.stats()
    assert st.n == n and st.nlist_mean > 10
    ctx.close()


@pytest.mark.parametrize("name", ["sod1000_eval", "disc3000_eval"])
def test_direct_gather_kernels_vs_reference_fixture(capi, name):
    """the alternative kernel sets (per-lane-gather list build; chunk-staged density/forces; tiled list + direct gathers)
    stay correct"""
    g = load_golden(name)
    for fl in (capi.FLAG_NO_LDS_TILES, capi.FLAG_NO_WHOLE_TILE):
        ctx, gas, sinks = make_ctx(capi, g["ic"], flags=fl)
        ctx.density(); ctx.forces()
        for f in ("rho", "P", "c"):
            assert rel_err(ctx.field(f), g[f]) <= EVAL_TOL, (fl, f)
        for f in ("ax", "ay", "az", "du", "dalpha"):
            assert rel_err(ctx.field(f), g["sph_" + f]) <= EVAL_TOL, (fl, f)
        ctx.close()
    ctx, gas, sinks = make_ctx(capi, g["ic"], flags=capi.FLAG_NO_LDS_TILES)
    ctx.density(); ctx.forces()
    for f in ("rho", "P", "c"):
        assert rel_err(ctx.field(f), g[f]) <= EVAL_TOL, f
    for f in ("ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), g["sph_" + f]) <= EVAL_TOL, f
    ctx.close()


def test_tiled_and_direct_kernels_agree_at_scale(capi):
    rows = ic.keplerian_disc(200000, seed=5)
    a, _, _ = make_ctx(capi, rows)
    b, _, _ = make_ctx(capi, rows, flags=capi.FLAG_NO_LDS_TILES)
    da, db = 1e-2, 1e-2
    for _ in range(2):
        da, _ = a.step(da); db, _ = b.step(db)
    assert da == db
    assert a.stats().nlist_mean == b.stats().nlist_mean        # same neighbour sets
    for f in "x vx u alpha".split():
        assert rel_err(a.field(f), b.field(f)) <= 1e-12, f
    a.close(); b.close()


def test_ring_with_viscosity_vs_oracle(capi):
    """thin ring (config 4 shape), alpha > 0 so the artificial-viscosity branch is live"""
    from oracle import orc
    rows = ic.thin_ring(30000, seed=404)
    gas, sinks = ic.split_rows(rows)
    rng = np.random.default_rng(5)
    gas["alpha"] = rng.uniform(0.05, 1.0, gas["x"].size)
    # add a converging radial velocity so v.r < 0 for many pairs
    r = np.hypot(gas["x"], gas["y"])
    gas["vx"] -= 0.3 * gas["x"] / r * np.sign(r - np.median(r))
    gas["vy"] -= 0.3 * gas["y"] / r * np.sign(r - np.median(r))
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    o = orc.Oracle(gas, sinks, nthreads=orc.max_threads())
    ctx.density(); ctx.forces(); o.evaluate()
    for f in ("rho", "ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), getattr(o, f)) <= EVAL_TOL, f
    assert np.count_nonzero(o.du) > 0.9 * o.n
    dt_g, _ = ctx.step(1e-2)
    dt_o = o.step(1e-2)
    assert dt_g == dt_o
    for f in ("x", "vx", "u", "alpha"):
        assert rel_err(ctx.field(f), getattr(o, f)) <= 1e-11, f
    ctx.close()


def test_edge_cases(capi):
    # empty set
    ctx = capi.Context(device=0)
    empty = {k: np.zeros(0) for k in "x y z vx vy vz u m".split()}
    ctx.upload(empty); ctx.set_sinks({k: np.zeros(1) for k in "x y z vx vy vz m".split()})
    ctx.density(); ctx.forces(); ctx.kick(0.01); ctx.drift(0.01)
    assert ctx.n == 0
    # one particle: rho = m W(0), no neighbours, zero SPH force
    one = {k: np.array([1.0]) for k in "x y z vx vy vz u m".split()}
    ctx.upload(one); ctx.density(); ctx.forces()
    assert ctx.field("rho")[0] == pytest.approx(1.0 / (3.14159265359 * 2.5 ** 3), rel=1e-15)
    assert ctx.field("du")[0] == 0.0
    # two far-apart clusters (sparse grid with many empty cells), ragged sizes (n not multiple of 64)
    rng = np.random.default_rng(3)
    n = 1000 + 37
    pos = rng.normal(0, 3.0, (n, 3)); pos[n // 2:] += 900.0
    gas = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(),
           "vx": rng.normal(0, 1, n), "vy": rng.normal(0, 1, n), "vz": rng.normal(0, 1, n),
           "u": rng.uniform(0.5, 2, n), "m": rng.uniform(0.5, 2, n) * 1e-3, "alpha": rng.uniform(0, 1, n)}
    sinks = {k: np.zeros(1) for k in "x y z vx vy vz m".split()}
    sinks["x"][0] = 450.0; sinks["m"][0] = 2.0
    from oracle import orc
    ctx.upload(gas); ctx.set_sinks(sinks)
    o = orc.Oracle(gas, sinks)
    ctx.density(); ctx.forces(); o.evaluate()
    for f in ("rho", "ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), getattr(o, f)) <= EVAL_TOL, f
    # the neighbour list grew past its initial capacity (dense clusters: hundreds of neighbours)
    assert ctx.stats().nlist_max > 96
    # call-order violations are reported, not crashes
    ctx.drift(0.01)
    with pytest.raises(capi.SphError):
        ctx.forces()
    ctx.close()


def test_upload_from_device_memory(capi):
    import torch
    rows = ic.keplerian_disc(4000, seed=9)
    gas, sinks = ic.split_rows(rows)
    a = capi.Context(device=0); a.upload(gas); a.set_sinks(sinks)
    b = capi.Context(device=0)
    dev = [torch.from_numpy(gas[k]).to("cuda:0") for k in "x y z vx vy vz u m alpha".split()]
    torch.cuda.synchronize()
    b.upload_dev(gas["x"].size, [t.data_ptr() for t in dev]); b.set_sinks(sinks)
    a.density(); a.forces(); b.density(); b.forces()
    assert np.array_equal(a.field("ax"), b.field("ax"))
    out = torch.empty(gas["x"].size, dtype=torch.float64, device="cuda:0")
    b.field_dev("rho", out.data_ptr(), out.numel())
    assert np.array_equal(out.cpu().numpy(), a.field("rho"))
    a.close(); b.close()


def test_north_star_acceptance_numbers(capi):
    """BASELINE.json's own criteria, stated as such: Sod shock tube L2 density error vs the reference < 1e-6 (after 5
    steps of the loop), and the Keplerian disc's energy after 40 steps equal to the reference's (same energy drift)."""
    g = load_golden("sod1000_traj")
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    dt, t = ctx.run(5, 1e-2, 0.0)
    ctx.density()
    rho = ctx.field("rho")
    l2 = np.sqrt(np.mean((rho - g["sph_s5_rho"]) ** 2)) / np.sqrt(np.mean(g["sph_s5_rho"] ** 2))
    assert l2 < 1e-6 and l2 < 1e-12            # the criterion, and what is actually achieved
    ctx.close()

    g = load_golden("disc3000_long")
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    m = gas["m"]

    def energy(vx, vy, vz, u):                 # kinetic + thermal (the potential depends on positions, compared below)
        return float(np.sum(m * (0.5 * (vx ** 2 + vy ** 2 + vz ** 2) + u)))

    e0 = energy(gas["vx"], gas["vy"], gas["vz"], gas["u"])
    dt, t = ctx.run(40, 1e-2, 0.0)
    e_mine = energy(ctx.field("vx"), ctx.field("vy"), ctx.field("vz"), ctx.field("u"))
    e_ref = energy(g["sph_s40_vx"], g["sph_s40_vy"], g["sph_s40_vz"], g["sph_s40_u"])
    assert abs(e_mine - e_ref) <= 1e-10 * abs(e_ref)
    assert abs((e_mine - e0) - (e_ref - e0)) <= 1e-7 * abs(e_ref - e0)      # the drift itself, to 7 digits
    assert rel_err(ctx.field("x"), g["sph_s40_x"]) <= 1e-9
    ctx.close()


def test_steady_state_steps_do_not_wait_for_the_device(capi):
    """the fixed-h step enqueues without host round trips: the grid is sized from the previous build's bounding box (one
    cell wider; particles outside a box are clamped into its boundary cells and still meet every neighbour) and the list
    report of the previous build is checked -- and the results are those of a run that waits for every read-back"""
    import os
    import subprocess
    import sys
    rows = ic.keplerian_disc(60_000, seed=23, nngb=85.0)
    gas, sinks = ic.split_rows(rows)
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    dt, t = ctx.run(2, 1e-2, 0.0)
    before = ctx.stats().host_syncs
    dt, t = ctx.run(10, dt, t)
    assert ctx.stats().host_syncs == before
    mine = {f: ctx.field(f) for f in "x y z vx vy vz u alpha".split()}
    lo, hi = ctx.bbox()
    assert lo[0] == mine["x"].min() and hi[1] == mine["y"].max()          # sph_get_bbox still reports the exact box
    ctx.close()
    # the same run with SPH_SYNC_EVERY_BUILD=1 (read once per process): same trajectory up to summation order
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np\n" f"sys.path.insert(0, {root!r})\n" "from summersph_amd import capi, ic\n"
            "gas, sinks = ic.split_rows(ic.keplerian_disc(60_000, seed=23, nngb=85.0))\n"
            "ctx = capi.Context(device=0); ctx.upload(gas); ctx.set_sinks(sinks)\n"
            "dt, t = ctx.run(2, 1e-2, 0.0); dt, t = ctx.run(10, dt, t)\n"
            "assert ctx.stats().host_syncs >= 20\n"
            "np.savez(sys.argv[1], dt=dt, **{f: ctx.field(f) for f in 'x y z vx vy vz u alpha'.split()})\n")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sync.npz")
        subprocess.run([sys.executable, "-c", code, path], check=True, env={**os.environ, "SPH_SYNC_EVERY_BUILD": "1"}, timeout=300)
        ref = dict(np.load(path))
    assert float(ref["dt"]) == dt
    for f in mine:
        assert rel_err(mine[f], ref[f]) <= 1e-12, f


def test_viscous_ring_trajectory_and_per_element_density(capi):
    """thin ring with a velocity dispersion (BASELINE configs[3]'s shape), 8 steps of the real reference: identical dt
    decisions, state <= 1e-10 of each field's scale, and the density of EVERY particle within 1e-11 of its own value"""
    g = load_golden("ring3000_traj")
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    dts, t = [1e-2], 0.0
    for _ in range(8):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt)
    assert dts == list(g["sph_dt_seq"])
    for f in "x y z vx vy vz u alpha".split():
        assert rel_err(ctx.field(f), g["sph_s8_" + f]) <= 1e-10, f
    rho = ctx.field("rho")
    assert np.all(rho > 0.0)
    assert float(np.max(np.abs(rho - g["sph_s8_rho"]) / g["sph_s8_rho"])) <= 1e-11
    ctx.close()


@pytest.mark.parametrize("name", ["sod1000_eval", "disc3000_eval", "bin2000_eval"])
def test_single_evaluation_per_element(capi, name):
    """relative to each element, not to the field's maximum: rho of every particle (strictly positive), and |a| of every
    particle whose acceleration is not a cancellation residue"""
    g = load_golden(name)
    ctx, gas, sinks = make_ctx(capi, g["ic"])
    ctx.density(); ctx.forces()
    rho = ctx.field("rho")
    assert float(np.max(np.abs(rho - g["rho"]) / g["rho"])) <= 1e-13
    a = np.sqrt(ctx.field("ax") ** 2 + ctx.field("ay") ** 2 + ctx.field("az") ** 2)
    aref = np.sqrt(g["sph_ax"] ** 2 + g["sph_ay"] ** 2 + g["sph_az"] ** 2)
    big = aref > 1e-3 * np.max(aref)
    assert float(np.max(np.abs(a[big] - aref[big]) / aref[big])) <= 1e-11
    ctx.close()


def test_far_outlier_costs_a_trimmed_grid_not_an_error(capi):
    """disc + one particle at 1e5 AU, no cull ('sph' mode): the bounding box would need 1e12 cells.  The grid then covers
    the bulk only (mean +- 6 sigma, trimmed), the outlier is clamped into a boundary cell and still meets exactly its own
    neighbours (none).  Every disc particle gets the sums of the disc alone, the outlier m W(0) and its sink gravity."""
    from oracle import orc
    g = load_golden("disc3000_eval")
    gas, sinks = ic.split_rows(g["ic"])
    n = gas["x"].size
    far = {k: np.append(v, 0.0) for k, v in gas.items() if isinstance(v, np.ndarray) and v.shape == (n,)}
    far["x"][n] = 1.0e5; far["y"][n] = -3.0e4; far["z"][n] = 2.0e3
    far["m"][n] = gas["m"][0]; far["u"][n] = 0.25
    far["vx"][n] = 0.1            # (a particle at rest would hold the global time step at its floor: |v| / |a| = 0, [F]:844)
    ctx = capi.Context(device=0)
    ctx.upload(far); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()
    st = ctx.stats()
    assert st.n_cells < 64 * (n + 1) + 4_100_000
    o = orc.Oracle(gas, sinks)
    o.evaluate()
    for f in ("rho", "P", "c", "ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f)[:n], getattr(o, f)) <= EVAL_TOL, f
    assert ctx.field("rho")[n] == pytest.approx(far["m"][n] / (3.14159265359 * 2.5 ** 3), rel=1e-15)
    assert ctx.field("du")[n] == 0.0
    d = np.array([far["x"][n] - sinks["x"][0], far["y"][n] - sinks["y"][0], far["z"][n] - sinks["z"][0]])
    a_sink = -sinks["m"][0] * ctx.params.G * d / np.sqrt((d ** 2).sum()) ** 3
    got = np.array([ctx.field("ax")[n], ctx.field("ay")[n], ctx.field("az")[n]])
    assert np.max(np.abs(got - a_sink)) <= 1e-14 * np.max(np.abs(a_sink))
    # and it keeps stepping: five steps, the disc follows the reference's trajectory (the outlier does not touch it;
    # its pull on the sink is 1e-13 of the disc's)
    gt = load_golden("disc3000_traj")
    dts, t = [1e-2], 0.0
    for _ in range(5):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt)
    assert dts == list(gt["sph_dt_seq"])
    for f in "x y z vx vy vz u alpha".split():
        assert rel_err(ctx.field(f)[:n], gt["sph_s5_" + f]) <= 1e-10, f
    ctx.close()


def test_positions_overwritten_in_steady_state_do_not_run_on_truncated_lists(capi):
    """in the steady state the list report (longest list) and the grid's box are read one build late.  Positions
    overwritten through sph_upload_field (not sph_upload) with a configuration whose lists exceed the capacity in place
    used to be evaluated on truncated lists, and the error appeared only at the NEXT build -- or never, for
    upload_field, density, download.  Now a field write invalidates the stale reports: the build waits for its own."""
    from oracle import orc
    rng = np.random.default_rng(77)
    n = 4000 + 21
    pos = rng.uniform(-1, 1, (n, 3)) * np.array([120.0, 120.0, 4.0])
    gas = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(),
           "vx": rng.normal(0, 1, n), "vy": rng.normal(0, 1, n), "vz": rng.normal(0, 1, n),
           "u": rng.uniform(0.5, 2, n), "m": rng.uniform(0.5, 2, n) * 1e-6, "alpha": rng.uniform(0, 1, n)}
    sinks = {k: np.zeros(1) for k in "x y z vx vy vz m".split()}
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    dt, t = ctx.run(3, 1e-4, 0.0)                        # steady state: reports are trusted one build late
    cap0 = ctx.stats().nlist_capacity
    dense = dict(gas)
    for k, s in zip("xyz", (0.12, 0.12, 1.0)):           # the same particles squeezed into 1/70 of the area
        dense[k] = gas[k] * s
    for k in "xyz":
        ctx.upload_field(k, dense[k])
    ctx.density(); ctx.forces()
    st = ctx.stats()
    assert st.nlist_max > cap0 and st.nlist_capacity >= st.nlist_max      # the list was regrown before it was used
    for k in "vx vy vz u alpha".split():
        dense[k] = ctx.field(k)
    o = orc.Oracle(dense, sinks)
    o.evaluate()
    for f in ("rho", "ax", "ay", "az", "du", "dalpha"):
        assert rel_err(ctx.field(f), getattr(o, f)) <= EVAL_TOL, f
    ctx.close()


def test_event_timing_samples_every_nth_launch(capi):
    """sph_timing_stride: only every stride-th launch of a timed group carries the HIP-event pair (bench.py samples its
    dominant kernel that way); the other groups stay untimed, and the results do not depend on it."""
    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=5, nngb=60.0))
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()
    ref = ctx.field("ax").copy()
    ctx.timing(True, only=["forces"], stride=3); ctx.timing_reset()
    for _ in range(6):
        ctx.density(); ctx.forces()
    ctx.synchronize()
    ms, launches = ctx.timing_get("forces")
    assert launches == 2 and ms > 0.0
    assert ctx.timing_get("density")[1] == 0
    ctx.timing(True, only=["forces"]); ctx.timing_reset()          # stride back to 1
    ctx.density(); ctx.forces(); ctx.synchronize()
    assert ctx.timing_get("forces")[1] == 1
    ctx.timing(False)
    assert np.array_equal(ctx.field("ax"), ref)
    ctx.close()


@pytest.mark.parametrize("flags_name", ["tile", "gather"])
def test_pairs_on_the_edge_of_the_support_and_coincident_points(capi, flags_name):
    """The pair visits carry no test of q and no mask for r = 0 (round 3): beyond 2h both table knots are the final zeros, dw(0) = 0.
    Planted pairs at exactly r = 2h, one ulp inside and outside, at r = 2h(1 +- 1e-9), and two coincident particles, in a disc
    patch dense enough for the tile kernels -- against the CPU oracle, which tests q <= 2 as the reference does (and, like it, divides by
    r = 0 for the coincident pair: those two particles' rates are NaN there and finite here)."""
    from oracle import orc
    gas, sinks = ic.split_rows(ic.keplerian_disc(30000, seed=77, nngb=70.0))
    rng = np.random.default_rng(8)
    gas["vx"] = gas["vx"] + rng.normal(0.0, 0.05, gas["x"].size)
    gas["alpha"] = np.full(gas["x"].size, 0.4)
    h = 2.5
    base = np.argsort(np.hypot(gas["x"] - 40.0, gas["y"]))[:12]           # twelve particles in the bulk take planted partners
    d = [2.0 * h, np.nextafter(2.0 * h, 0.0), np.nextafter(2.0 * h, 10.0), 2.0 * h * (1 - 1e-9), 2.0 * h * (1 + 1e-9), 0.0]
    for k, dist in enumerate(d):
        a, b = base[2 * k], base[2 * k + 1]
        gas["x"][b] = gas["x"][a] + dist
        gas["y"][b] = gas["y"][a]
        gas["z"][b] = gas["z"][a]
    flags = 0 if flags_name == "tile" else capi.FLAG_NO_WHOLE_TILE
    ctx = capi.Context(device=0, flags=flags)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()
    st = ctx.stats()
    if flags_name == "tile":
        assert st.tile_fit_pct_forces >= 90
    o = orc.Oracle(gas, sinks)
    o.evaluate()
    twins = base[10:12]                     # the coincident pair: the reference divides by r = 0 there (NaN), the kernels add zeros
    others = np.ones(gas["x"].size, bool); others[twins] = False
    assert rel_err(ctx.field("rho"), o.rho) <= EVAL_TOL                     # a coincident partner counts with W(0) in the density
    for f in ("ax", "ay", "az", "du", "dalpha"):
        got, want = ctx.field(f), getattr(o, f)
        assert np.all(np.isfinite(got)), f
        assert np.all(np.isfinite(want[others])), f
        assert rel_err(got[others], want[others]) <= EVAL_TOL, f
    ctx.close()
