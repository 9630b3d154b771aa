"""GPU: the steady state of the plain fixed-h step (sph_step / sph_run: the grid box, the longest list, the tile need and the
tile fit are believed one build late -- csrc/grid.hip grid_rebuild and grid_prepare_early, csrc/tiled.hip nlist_build_tiled,
csrc/api.hip drain_reports) on particle sets that change under the run (tests/steady_sets.py; their construction conditions
are asserted in tests/test_steady_sets_cpu.py).

After EVERY step of a steady-state run the sums of that very step are checked on the state the caller can download:
density and forces are called again (no new build: the same list, the same velocities; the trajectory is bitwise the one
without these calls), the number of list entries must equal the brute-force count of ordered pairs with 0 < r <= 2 h, rho
must be within 1e-13 of each element's own value of the oracle's density pass, and the rates are compared with the O(n^2)
restatement tests/force_terms_ref.fixed_terms at the project's per-element bar (varh_ref.rate_excess <= 1: 1e-11 of the
element plus 1e-13 of the summed magnitudes of its terms) on the first step, the last step and every step in which a
transition fires, and with the threaded C oracle at EVAL_TOL (1e-13 of the field's scale) on the others.  Every bar is one
the project already has, taken from CPU-against-CPU agreement (tests/test_steady_sets_cpu.py, tests/test_force_terms_cpu.py:
the two CPU references use <= 4e-3 of the rate bar on these sets); none comes from a GPU result.

The transitions are asserted from stats() and grid_info() against a host replay (steady_sets.capacity_replay, grid_replay)
of the positions the GPU run itself went through, so each is pinned to its step:
  regrow from the stale report       nlist_capacity follows the replay, host_syncs does not move (contraction, the run(k)
                                     variant, clumps_together)
  table regrown / radix sort / trim  n_cells and grid_info().bytes follow the replay, the trim's waits are counted
                                     (clumps_apart)
  early keys on a box left behind    the builds that take the kick + drift pass's keys, replayed from grid_prepare_early's
                                     conditions, with half the particles outside their box (clumps_drift)
  tile fit flipping                  tile_fit_pct_forces >= 90 -> < 90 on the side of 90 the replayed tile needs say, one
                                     build late, without a host wait (sheet_puffing_up)
  hashed and sticky -> dense         grid_info().kind 1, 1, 1, 1, 1, 0, ... (clumps_together)
  overflow within one step           SphError at the next build (contraction_too_fast_mid) or from the call that returns
                                     (contraction_too_fast_last), and every later evaluation refused until a fresh upload
Each run is repeated in a fresh process with SPH_SYNC_EVERY_BUILD=1 (every build waits for its own reports and box): the
same dt decisions and the same state to 1e-12 of each field's scale.

Which tests fail when a branch is reverted (each on a scratch build of the library with that one branch taken out, the
whole file run against it on the MI355X):
  the regrow from the stale report (tiled.hip)       5 fail: contraction [default, no_whole_tile], contraction as one
                                                     run, clumps_together [default, no_whole_tile] (SphError: overflow)
  the overflow check at the next build (tiled.hip)   2 fail: too_fast_mid [default, no_whole_tile] (no error raised)
  drain_reports' list check (api.hip)                4 fail: too_fast_last and too_fast_mid [default, no_whole_tile]
  the one-cell guard of the stale box (grid.hip)     9 fail: clumps_apart, clumps_drift and clumps_together, each under
                                                     the three flag sets (n_cells differs from the replay)
  refusing evaluations after an overflow (api.hip)   4 fail: too_fast_mid and too_fast_last [default, no_whole_tile]
                                                     (ctx.step() after the error succeeds)
Every other test passes on each of these builds.
The last one is the finding that came with this suite (read off drain_reports, pinned by these tests): after drain_reports
had reported an overflow -- and dropped the stale report along with the validity flags -- the next ctx.step() waited for
its own report, regrew the list and went on from the velocities that the truncated sums had kicked.  The context now
refuses every evaluation until sph_upload.
The drop of the early keys on a grid change (grid.hip, `!same_grid`) cannot be reached by a fixed-h run: grid_prepare_early
and grid_rebuild read the same box slot and take the same decisions on it, so no single revert of it can fail.  What can
go wrong there is the early keys themselves: clumps_drift runs them with half the particles outside their box.

Measured on the MI355X (21 tests, 23 s with 16 host threads for the references): rho <= 3.4e-15 per element; the rates <=
0.6 % of their per-element bar on the restatement's steps and <= 2.8e-15 of the field's scale against the oracle on the
others; every list count exact; every capacity, cell count, table size, grid kind and early-keys build as replayed; the
steady-state runs against the synchronous process <= 3.7e-15 of each field's scale with identical dt decisions; the
run(24) variant <= 8.7e-16 against the oracle (bar 1e-10) with its dt and t to the bit.  clumps_drift: early keys in builds
1, 3, 5, 7 and 8 with 934 to 774 of 1620 particles outside their box, the table regrown in steps 2, 4 and 6, rho <=
1.4e-15, the rates <= 0.55 % of their bar, against the synchronous process <= 3.3e-16, bitwise the run without early keys.
sheet_puffing_up: tile_fit_pct_forces 99 after the first evaluation, then 99, 96, 94, 94, 96, 96, 100, 4 after the eight
steps -- the host replay's 99, 96, 94, 94, 96, 96, 100, 4, 4 per build, one build late, to the digit -- with host_syncs at
3 throughout; rho <= 3.4e-15 per element and <= 2.2e-15 against the oracle under each of the three flag sets, <= 1.9e-15
against the no-whole-tile and the untiled run, <= 2.8e-16 against the synchronous process."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import steady_sets as S
import varh_ref as VR
from conftest import rel_err
from gpu_support import capi, make_context

pytestmark = pytest.mark.gpu

EVAL_TOL = 1e-13                 # tests/test_parity_gpu.py: one evaluation against the oracle, of each field's scale
FLAGSETS = ("default", "no_whole_tile", "no_lds_tiles")
STATE8 = "x y z vx vy vz u alpha".split()


def flags_of(capi, flagset):
    return {"default": 0, "no_whole_tile": capi.FLAG_NO_WHOLE_TILE, "no_lds_tiles": capi.FLAG_NO_LDS_TILES}[flagset]


def download(ctx, names):
    return {f: ctx.field(f) for f in names}


# ---- the steady-state run with its per-step checks -----------------------------------------------------------------------
def steady_run(capi, name, flagset, checks=True):
    """the set along its schedule, one ctx.step per dt.  Returns the record of the run; with checks, every step's sums are
    compared as the module docstring says and the worst figures are returned with it"""
    s = S.build(name)
    gas, clump = s["gas"], s["clump"]
    n = gas["x"].size
    ctx = make_context(capi, gas, flags=flags_of(capi, flagset))
    rec = dict(dts=[], pos=[S.positions(gas)], stats=[], kind=[], bytes=[], worst=dict(rho=0.0, rates=0.0, oracle=0.0),
               untiled=flagset == "no_lds_tiles")
    if checks:
        # build 0 (the first step starts with the same two calls): it waits for its own box and list report
        ctx.density(); ctx.forces()
        rec["stats0"], rec["kind0"], rec["bytes0"] = ctx.stats(), ctx.grid_info().kind, ctx.grid_info().bytes
        assert rec["stats0"].nlist_builds == 1 and rec["stats0"].host_syncs >= (1 if rec["untiled"] else 2)
    t = 0.0
    for k, dt in enumerate(s["dts"]):
        dt_next, t = ctx.step(dt, t)
        rec["dts"].append(dt_next)
        st = ctx.stats()
        gi = ctx.grid_info()
        rec["stats"].append(st); rec["kind"].append(gi.kind); rec["bytes"].append(gi.bytes)
        if checks:
            # the sums of this step again, on the list its trusted build made: no new build
            ctx.density(); ctx.forces()
            again = ctx.stats()
            assert (again.nlist_builds, again.grid_builds) == (st.nlist_builds, st.grid_builds), (name, k)
            assert again.host_syncs == st.host_syncs
        state = download(ctx, S.STATE)
        rec["pos"].append(S.positions(state))
        if not checks:
            continue
        tag = f"{name}/{flagset}/step {k + 1}"
        got = download(ctx, S.DERIVED)
        for f, a in list(state.items()) + list(got.items()):
            assert np.all(np.isfinite(a)), (tag, f)
        # the list: exactly the ordered pairs with 0 < r <= 2 h of the downloaded positions
        ps = S.pair_stats(rec["pos"][-1])
        entries = st.nlist_mean * n
        assert abs(entries - round(entries)) < 1e-6 and ps["entries_lo"] <= round(entries) <= ps["entries_hi"], \
            (tag, entries, ps["entries_lo"], ps["entries_hi"])
        rec.setdefault("longest", [S.pair_stats(rec["pos"][0])["longest"]]).append(ps["longest"])
        # rho per element against the oracle's density pass on the downloaded state
        ev = S.oracle_eval(state, clump)
        e_rho = float(np.max(np.abs(got["rho"] - ev["rho"]) / ev["rho"]))
        rec["worst"]["rho"] = max(rec["worst"]["rho"], e_rho)
        assert e_rho <= 1e-13, (tag, "rho", int(np.argmax(np.abs(got["rho"] - ev["rho"]) / ev["rho"])))
        rec.setdefault("evals", []).append((state, got, ev))
    rec["final"] = download(ctx, STATE8)
    rec["ctx_stats"] = ctx.stats()
    ctx.close()
    return rec


def check_rates(name, flagset, rec, special):
    """the rates of every step: the O(n^2) restatement per element on the steps in `special` (1-based), the first and the
    last; the threaded oracle at EVAL_TOL on the others"""
    clump = S.build(name)["clump"]
    nsteps = len(rec["evals"])
    for k, (state, got, ev) in enumerate(rec["evals"], start=1):
        tag = f"{name}/{flagset}/step {k}"
        if k in special or k in (1, nsteps):
            rates, scales = S.terms_ref(state, clump)
            for i, f in enumerate(S.RATES):
                ex = VR.rate_excess(np.abs(got[f] - rates[i]), np.abs(rates[i]), scales[i])
                rec["worst"]["rates"] = max(rec["worst"]["rates"], float(np.max(ex)))
                assert float(np.max(ex)) <= 1.0, (tag, f, int(np.argmax(ex)), float(np.max(ex)))
        else:
            for f in ("P", "c") + S.RATES:
                e = rel_err(got[f], ev[f])
                rec["worst"]["oracle"] = max(rec["worst"]["oracle"], e)
                assert e <= EVAL_TOL, (tag, f, e)
    print(f"{name}/{flagset}: rho {rec['worst']['rho']:.2e} (per element, bar 1e-13); share of the per-element rate bar "
          f"{rec['worst']['rates']:.2e}; against the oracle {rec['worst']['oracle']:.2e} (bar {EVAL_TOL:g})")


def check_decisions(name, rec):
    _, decisions = S.trajectory(name)
    assert rec["dts"] == decisions, (name, rec["dts"], decisions)


_CHILD = ("import sys, numpy as np\n"
          "sys.path[:0] = [{root!r}, {tests!r}]\n"
          "import steady_sets as S\n"
          "from summersph_amd import capi\n"
          "s = S.build({name!r})\n"
          "ctx = capi.Context(device=0, flags={flags}); ctx.upload(s['gas'])\n"
          "dts, t = [], 0.0\n"
          "for dt in s['dts']:\n"
          "    d, t = ctx.step(dt, t); dts.append(d)\n"
          "assert {min_syncs} * len(dts) <= ctx.stats().host_syncs\n"
          "np.savez(sys.argv[1], dts=np.array(dts), **{{f: ctx.field(f) for f in 'x y z vx vy vz u alpha'.split()}})\n")


def child_run(capi, name, flagset, switch):
    """the set along its schedule in a fresh process with the A/B switch `switch` set (such switches are read once per process)"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD.format(root=os.path.dirname(tests), tests=tests, name=name, flags=flags_of(capi, flagset),
                         min_syncs=2 if switch == "SPH_SYNC_EVERY_BUILD" else 0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "child.npz")
        subprocess.run([sys.executable, "-c", code, path], check=True, env={**os.environ, switch: "1"}, timeout=120)
        return dict(np.load(path))


def check_against_synchronous_child(capi, name, flagset, rec):
    """the same schedule in a fresh process in which every build waits for its own reports (SPH_SYNC_EVERY_BUILD): the same
    dt decisions, the state to 1e-12 of each field's scale"""
    ref = child_run(capi, name, flagset, "SPH_SYNC_EVERY_BUILD")
    assert list(ref["dts"]) == rec["dts"], name
    errs = {f: rel_err(rec["final"][f], ref[f]) for f in STATE8}
    print(f"{name}/{flagset} against the synchronous run:", {f: f"{v:.1e}" for f, v in errs.items()})
    for f, v in errs.items():
        assert v <= 1e-12, (name, f, v)


def check_untouched(capi, name, flagset, rec):
    """the extra density / forces calls after every step left the trajectory bitwise alone"""
    plain = steady_run(capi, name, flagset, checks=False)
    assert plain["dts"] == rec["dts"]
    for f in STATE8:
        assert np.array_equal(plain["final"][f], rec["final"][f]), (name, f)
    assert plain["ctx_stats"].nlist_builds == rec["ctx_stats"].nlist_builds


def check_capacity(name, rec):
    """nlist_capacity after every step is the replay's, on the positions this run went through; the steps whose build
    regrew the list from the stale report; nlist_max is the PREVIOUS build's longest list (that is what a trusted build reads)"""
    if rec["untiled"]:
        # SPH_FLAG_NO_LDS_TILES: the 32-bit list of pairs.hip waits for every build's own maximum and grows in place
        cap, grown = S.NL_CAP0, []
        for k, st in enumerate([rec["stats0"]] + rec["stats"]):
            mx = rec["longest"][k]
            if mx > cap:
                cap = mx + mx // 8 + 8
                grown.append(k)
            assert (st.nlist_capacity, st.nlist_max, st.nlist_builds) == (cap, mx, k + 1), (name, k, st.nlist_capacity, cap, mx)
        return grown
    caps = S.capacity_replay(rec["longest"])
    assert not any(c["overflow"] for c in caps)
    for k, st in enumerate(rec["stats"], start=1):
        assert st.nlist_capacity == caps[k]["cap"], (name, k, st.nlist_capacity, caps[k])
        assert st.nlist_max == rec["longest"][k - 1], (name, k, st.nlist_max, rec["longest"][k - 1:k + 1])
        assert st.nlist_builds == k + 1
    return [k for k, c in enumerate(caps) if c["regrown"]]


# ---- contraction: the list regrown from stale reports ------------------------------------------------------------------
@pytest.mark.parametrize("flagset", FLAGSETS)
def test_contraction_regrows_from_stale_reports(capi, flagset):
    name = "contraction"
    rec = steady_run(capi, name, flagset)
    regrown = check_capacity(name, rec)
    print(f"{name}/{flagset}: longest {rec['longest']}, capacity {[st.nlist_capacity for st in rec['stats']]}, regrown in steps {regrown}")
    assert len(regrown) >= 2 and rec["stats"][-1].nlist_capacity > rec["longest"][-1] > 200
    # no host wait in any step after the first build, regrows included.  (host_syncs counts the waits of grid.hip and
    # tiled.hip; the untiled list of SPH_FLAG_NO_LDS_TILES waits for every build's own maximum without counting it, so for
    # that flag set this says only that the BOX came from the previous build)
    syncs = [st.host_syncs for st in rec["stats"]]
    assert all(v == rec["stats0"].host_syncs for v in syncs), syncs
    assert all(k == 0 for k in rec["kind"])
    check_decisions(name, rec)
    check_rates(name, flagset, rec, special=set(regrown))
    if flagset == "default":
        check_untouched(capi, name, flagset, rec)
        check_against_synchronous_child(capi, name, flagset, rec)


def test_contraction_as_one_run_chains_its_own_dt_without_waiting(capi):
    """one ctx.run(k): the device chains its own dt.  ctx.run hands back the last dt decision and t only, so the dt SEQUENCE
    is compared through them: both are the oracle's to the bit (t is the running sum of the sequence, added in the same
    order; the oracle's sequence takes four different values) -- strong evidence, not the sequence itself.  The state is within the trajectory bar (1e-11 up to 5 steps, 1e-10 beyond), the
    capacity is the replay's after at least two regrows, and no step of the run waited for the host"""
    name = "contraction"
    s = S.build(name)
    k, dt0 = s["run"]
    states, dts, t_ref = S.run_trajectory(name)
    caps = S.capacity_replay([S.pair_stats(S.positions(st))["longest"] for st in states])
    assert sum(c["regrown"] for c in caps) >= 2
    ctx = make_context(capi, s["gas"])
    ctx.density(); ctx.forces()                      # the first build, with its own waits (the run starts with the same calls)
    before = ctx.stats()
    assert before.nlist_builds == 1 and before.nlist_capacity == S.NL_CAP0
    dt, t = ctx.run(k, dt0, 0.0)
    st = ctx.stats()
    assert (dt, t) == (dts[-1], t_ref), (dt, t, dts[-1], t_ref)
    assert st.host_syncs == before.host_syncs and st.nlist_builds == k + 1
    assert st.nlist_capacity == caps[-1]["cap"] > S.NL_CAP0, (st.nlist_capacity, caps[-1])
    bar = 1e-11 if k <= 5 else 1e-10
    errs = {f: rel_err(ctx.field(f), states[-1][f]) for f in STATE8}
    print(f"{name} as one run of {k} steps:", {f: f"{v:.1e}" for f, v in errs.items()}, f"(bar {bar:g})")
    for f, v in errs.items():
        assert v <= bar, (f, v)
    ctx.close()


# ---- clumps_apart: the box outruns its guard cell; table regrown, radix sort, trim -----------------------------------------------
def check_grid(name, rec, n):
    """n_cells, the grid's kind, the table's bytes and the host waits of every step against the replay of grid_rebuild on
    the positions this run went through"""
    grid = S.grid_replay(rec["pos"])
    assert rec["kind0"] == grid[0]["kind"] and (grid[0]["kind"] == 1 or rec["stats0"].n_cells == int(grid[0]["cells"]))
    cap = (rec["bytes0"] // 4 - 16) // 2 if rec["kind0"] == 0 else None
    events = dict(table=[], radix=[], trim=[], dense=[], clamped=[])
    for k, st in enumerate(rec["stats"], start=1):
        g = grid[k]
        tag = (name, k, st.n_cells, g["cells"], g["rounds"])
        assert rec["kind"][k - 1] == g["kind"], tag
        waits = st.host_syncs - (rec["stats"][k - 2] if k > 1 else rec["stats0"]).host_syncs
        if g["kind"] == 1:
            continue                                  # (n_cells counts the occupied cells of a hashed grid)
        if k > 1 and grid[k - 1]["kind"] == 1:
            events["dense"].append(k)
        if g["rounds"] == 0:
            assert st.n_cells == int(g["cells"]) and list(st.grid_dim) == [int(d) for d in g["dim"]], tag
            assert waits == 0, tag                    # the steady state: box, list report and tile fit one build late
        else:
            # the trim's moments are summed in another order on the device: a boundary within an ulp of a cell edge may fall
            # either way.  Its waits are counted, one per round
            assert all(abs(int(a) - int(b)) <= 1 for a, b in zip(st.grid_dim, g["dim"])), tag
            assert waits >= g["rounds"], tag
            events["trim"].append(k)
        table = (rec["bytes"][k - 1] // 4 - 16) // 2              # api.hip: bytes = (2 cell_cap + 16) * 4
        if cap is not None and st.n_cells + 2 > cap:
            assert table == (st.n_cells + 2) + (st.n_cells + 2) // 4, tag
            events["table"].append(k)
        elif cap is not None:
            assert table == cap, tag
        cap = table
        if not g["counting"]:
            events["radix"].append(k)
        if g["outside"].mean() >= 0.05:
            events["clamped"].append(k)
    return grid, events


@pytest.mark.parametrize("flagset", FLAGSETS)
def test_clumps_apart_clamped_particles_and_every_grid_threshold(capi, flagset):
    name = "clumps_apart"
    n = S.build(name)["gas"]["x"].size
    rec = steady_run(capi, name, flagset)
    grid, ev = check_grid(name, rec, n)
    print(f"{name}/{flagset}: n_cells {[st.n_cells for st in rec['stats']]}, table regrown in steps {ev['table']}, radix sort in "
          f"{ev['radix']}, trimmed in {ev['trim']}, >= 5 % clamped in {ev['clamped']}, host_syncs {[st.host_syncs for st in rec['stats']]}")
    cells = [st.n_cells for st in rec["stats"]]
    assert ev["table"] and ev["radix"] and ev["trim"] and min(ev["table"]) < min(ev["radix"]) < min(ev["trim"])
    assert max(cells[:min(ev["radix"]) - 1]) <= 4 * n + 1_000_000 < cells[min(ev["radix"]) - 1]
    assert grid[min(ev["trim"])]["box_cells"] > 64 * n + 4_000_000
    assert ev["clamped"] == list(range(1, len(rec["stats"]) + 1))            # every step's grid clamps particles
    check_capacity(name, rec)
    check_decisions(name, rec)
    first = [min(ev[k]) for k in ("table", "radix", "trim")]
    check_rates(name, flagset, rec, special=set(first) | {f + 1 for f in first})
    if flagset == "default":
        check_untouched(capi, name, flagset, rec)
        check_against_synchronous_child(capi, name, flagset, rec)


# ---- clumps_drift: the keys of the kick + drift pass on a box that particles have left ------------------------------------------
@pytest.mark.parametrize("flagset", FLAGSETS)
def test_clumps_drift_early_keys_with_particles_outside_the_stale_box(capi, flagset):
    """the builds that take keys, histogram and box partials from the step's kick + drift pass (grid.hip kick_drift_keys: the
    headline path's own copy of the key computation, clamping included) while about half of the particles lie outside the box
    those keys were computed for.  Which builds these are is replayed from grid_prepare_early's own conditions with the
    table capacities the run reports; their sums are checked per element like every other step's, all of them against
    the O(n^2) restatement, and the whole run is bitwise the run of a process with SPH_NO_DRIFT_KEYS set"""
    name = "clumps_drift"
    n = S.build(name)["gas"]["x"].size
    rec = steady_run(capi, name, flagset)
    grid, ev = check_grid(name, rec, n)
    tables = [(b // 4 - 16) // 2 for b in [rec["bytes0"]] + rec["bytes"]]
    early = S.early_replay(grid, tables)
    outside = [int(g["outside"].sum()) for g in grid]
    print(f"{name}/{flagset}: n_cells {[st.n_cells for st in rec['stats']]}, early keys in builds {[k for k, e in enumerate(early) if e]}, "
          f"outside {outside}, table regrown in steps {ev['table']}, host_syncs {[st.host_syncs for st in rec['stats']]}")
    assert early == S.early_replay(grid) and sum(early) >= 3 and len(ev["table"]) >= 2
    assert all(outside[k] >= 0.4 * n for k, e in enumerate(early) if e)
    assert not ev["radix"] and not ev["trim"] and all(k == 0 for k in rec["kind"])
    assert all(st.host_syncs == rec["stats0"].host_syncs for st in rec["stats"])
    check_capacity(name, rec)
    check_decisions(name, rec)
    check_rates(name, flagset, rec, special=set(range(1, len(rec["stats"]) + 1)))
    if flagset == "default":
        check_untouched(capi, name, flagset, rec)
        check_against_synchronous_child(capi, name, flagset, rec)
        plain = child_run(capi, name, flagset, "SPH_NO_DRIFT_KEYS")
        assert list(plain["dts"]) == rec["dts"]
        for f in STATE8:
            assert np.array_equal(plain[f], rec["final"][f]), (name, f, "SPH_NO_DRIFT_KEYS")


# ---- clumps_together: hashed and sticky, dense again, the meeting -----------------------------------------------------------------
@pytest.mark.parametrize("flagset", FLAGSETS)
def test_clumps_together_leaves_the_hashed_grid_and_regrows_at_the_meeting(capi, flagset):
    name = "clumps_together"
    n = S.build(name)["gas"]["x"].size
    rec = steady_run(capi, name, flagset)
    grid, ev = check_grid(name, rec, n)
    regrown = check_capacity(name, rec)
    kinds = rec["kind"]
    print(f"{name}/{flagset}: kind {kinds}, longest {rec['longest']}, capacity {[st.nlist_capacity for st in rec['stats']]}, "
          f"regrown in steps {regrown}, host_syncs {[st.host_syncs for st in rec['stats']]}")
    assert kinds[0] == 1 and len(ev["dense"]) == 1 and all(k == 0 for k in kinds[ev["dense"][0] - 1:])      # 1 -> 0, once
    assert len(regrown) >= 2 and min(regrown) > ev["dense"][0] and max(rec["longest"]) > 200
    # no host wait from the step after the grid turned dense to the end: regrows included
    syncs = [st.host_syncs for st in rec["stats"]]
    assert all(v == syncs[ev["dense"][0] - 1] for v in syncs[ev["dense"][0] - 1:]), syncs
    check_decisions(name, rec)
    check_rates(name, flagset, rec, special=set(regrown) | {ev["dense"][0] - 1, ev["dense"][0], ev["dense"][0] + 1})
    if flagset == "default":
        check_untouched(capi, name, flagset, rec)
        check_against_synchronous_child(capi, name, flagset, rec)


# ---- sheet_puffing_up: the tile fit of the forces flips, and the next build learns it from a stale report ------------------------------
_SHEET = {}


def sheet_run(capi, flagset):
    """sheet_puffing_up along its schedule under one flag set: every step's sums against the threaded C oracle on the
    downloaded state (rho per element at 1e-13, P, c and the rates at EVAL_TOL), no new build by the extra calls, the dt
    decisions the oracle's.  Returns the record (kept per flag set: the tests below share the runs)."""
    if flagset in _SHEET:
        return _SHEET[flagset]
    from test_whole_tile_gpu import FIELDS
    name = "sheet_puffing_up"
    s = S.build(name)
    ctx = make_context(capi, s["gas"], flags=flags_of(capi, flagset))
    ctx.density(); ctx.forces()
    st0 = ctx.stats()
    rec = dict(first=download(ctx, FIELDS), fits=[st0.tile_fit_pct_forces], syncs=[st0.host_syncs], pos=[S.positions(s["gas"])],
               dts=[], states=[], worst=dict(rho=0.0, oracle=0.0))
    t = 0.0
    for k, dt in enumerate(s["dts"], start=1):
        d, t = ctx.step(dt, t)
        rec["dts"].append(d)
        st = ctx.stats()
        rec["fits"].append(st.tile_fit_pct_forces); rec["syncs"].append(st.host_syncs)
        ctx.density(); ctx.forces()
        again = ctx.stats()
        assert (again.nlist_builds, again.grid_builds, again.host_syncs) == (st.nlist_builds, st.grid_builds, st.host_syncs), k
        assert st.nlist_builds == k + 1
        state, got = download(ctx, S.STATE), download(ctx, S.DERIVED)
        rec["pos"].append(S.positions(state)); rec["states"].append(state)
        ev = S.oracle_eval(state)
        e_rho = float(np.max(np.abs(got["rho"] - ev["rho"]) / ev["rho"]))
        rec["worst"]["rho"] = max(rec["worst"]["rho"], e_rho)
        assert e_rho <= 1e-13, (flagset, k, "rho")
        for f in ("P", "c") + S.RATES:
            e = rel_err(got[f], ev[f])
            rec["worst"]["oracle"] = max(rec["worst"]["oracle"], e)
            assert e <= EVAL_TOL, (flagset, k, f, e)
    rec["final"] = download(ctx, STATE8)
    ctx.close()
    check_decisions(name, rec)
    print(f"{name}/{flagset}: tile_fit_pct_forces {rec['fits']}, host_syncs {rec['syncs']}; rho {rec['worst']['rho']:.2e} (per element, "
          f"bar 1e-13), against the oracle {rec['worst']['oracle']:.2e} (bar {EVAL_TOL:g})")
    _SHEET[flagset] = rec
    return rec


def test_sheet_puffing_up_tile_fit_flips_from_a_stale_report(capi):
    """8000 particles (sized on the host replay of the tile need, see steady_sets.sheet_puffing_up): too many for the O(n^2)
    restatement, so every step is compared with the threaded C oracle (sheet_run) -- and with the SPH_FLAG_NO_WHOLE_TILE run
    of the same schedule: the first evaluation at test_whole_tile_gpu.same's bars (rho, P, c bitwise, the rates 1e-14 of the
    field's scale), the state after every step at that module's trajectory bar (1e-12).  tile_fit_pct_forces after step k is
    what the digest made of the report of build k - 1 (the trusted build reads the previous one's): it must fall on the same
    side of 90 as the host replay of that build's tile needs on the positions this run went through, start >= 90 and end
    < 90, and the flip costs no host wait.  A process that waits for every report (and so takes the same decision one
    build earlier) gives the same dt decisions and state."""
    from test_whole_tile_gpu import FIELDS, same
    name = "sheet_puffing_up"
    rec, twin = sheet_run(capi, "default"), sheet_run(capi, "no_whole_tile")
    for f in FIELDS:
        assert same(rec["first"][f], twin["first"][f], f), ("first evaluation", f)
    assert twin["fits"] == [-1] * len(twin["fits"]) and rec["dts"] == twin["dts"]
    e_twin = max(rel_err(a[f], b[f]) for a, b in zip(rec["states"], twin["states"]) for f in STATE8)
    fits, pos = rec["fits"], rec["pos"]
    # the report a trusted build digests is the previous build's: fits[k] (after step k >= 1) describes build k - 1
    boxes = [S.exact_box(pos[0])] + [S.stale_box(p) for p in pos[:-1]]
    replay = [S.tile_fit_replay(p, *bx)["fit_pct_forces"] for p, bx in zip(pos, boxes)]
    print(f"{name}: tile_fit_pct_forces {fits} (after the first evaluation, then after each step), replay per build {replay}; "
          f"against the no-whole-tile run {e_twin:.2e} (bar 1e-12)")
    assert e_twin <= 1e-12
    assert (fits[0] >= 90) == (replay[0] >= 90)
    for k in range(1, len(fits)):
        assert (fits[k] >= 90) == (replay[k - 1] >= 90), (k, fits, replay)
    assert fits[0] >= 90 and fits[-1] < 90 and replay[-1] < 90 and replay[-2] < 90
    assert all(v == rec["syncs"][0] for v in rec["syncs"]), rec["syncs"]          # the flip costs no host wait
    check_against_synchronous_child(capi, name, "default", rec)


def test_sheet_puffing_up_with_the_untiled_list(capi):
    """SPH_FLAG_NO_LDS_TILES: no tiles, so nothing to flip -- the same schedule, every step against the oracle (sheet_run), and
    the state after every step within the trajectory bar of the default run (summation order only)"""
    rec, ref = sheet_run(capi, "no_lds_tiles"), sheet_run(capi, "default")
    assert rec["fits"] == [-1] * len(rec["fits"]) and rec["dts"] == ref["dts"]
    e = max(rel_err(a[f], b[f]) for a, b in zip(rec["states"], ref["states"]) for f in STATE8)
    print(f"sheet_puffing_up/no_lds_tiles against the default run {e:.2e} (bar 1e-12)")
    assert e <= 1e-12


# ---- a list that outgrows its headroom within one step: an error, never truncated sums ---------------------------------------------
def refused_from_now_on(capi, ctx, dt):
    """no later call hands out anything of the truncated evaluation"""
    for call in (lambda: ctx.field("rho"), lambda: ctx.field("ax"), ctx.forces, ctx.density, lambda: ctx.step(dt, 0.0),
                 lambda: ctx.run(2, dt, 0.0), lambda: ctx.step(dt, 0.0), lambda: ctx.field("du"), ctx.forces):
        with pytest.raises(capi.SphError):
            call()


def evaluates_after_fresh_upload(capi, ctx, name, flagset):
    """the same context, the set uploaded afresh at the oracle's positions of the overflowing build: the first build waits
    for its own report, regrows the list and evaluates correctly"""
    states, _ = S.trajectory(name)
    state = {f: states[1][f] for f in S.STATE}
    ctx.upload(state)
    ctx.density(); ctx.forces()
    st = ctx.stats()
    ps = S.pair_stats(S.positions(state))
    assert ps["longest"] > S.NL_CAP0 and st.nlist_max == ps["longest"] and 4 * ps["longest"] <= 3 * st.nlist_capacity
    assert round(st.nlist_mean * ps["per"].size) == ps["entries"]
    got = download(ctx, S.DERIVED)
    ev = S.oracle_eval(state)
    e_rho = float(np.max(np.abs(got["rho"] - ev["rho"]) / ev["rho"]))
    rates, scales = S.terms_ref(state)
    ex = max(float(np.max(VR.rate_excess(np.abs(got[f] - rates[i]), np.abs(rates[i]), scales[i]))) for i, f in enumerate(S.RATES))
    print(f"{name}/{flagset} after a fresh upload: capacity {st.nlist_capacity}, longest {st.nlist_max}, rho {e_rho:.2e}, "
          f"share of the rate bar {ex:.2e}")
    assert e_rho <= 1e-13 and ex <= 1.0
    dt, _ = ctx.step(1e-3, 0.0)                       # and it steps again
    assert dt > 0.0 and np.all(np.isfinite(ctx.field("rho")))


TILED = ("default", "no_whole_tile")                  # the flag sets with the 16-bit tiled list, whose reports come one build late


@pytest.mark.parametrize("flagset", TILED)
def test_too_fast_mid_run_raises_at_the_next_build(capi, flagset):
    """the overflowing build is followed by more steps within the same call: the next build reads its report and refuses"""
    name = "contraction_too_fast_mid"
    s = S.build(name)
    ctx = make_context(capi, s["gas"], flags=flags_of(capi, flagset))
    with pytest.raises(capi.SphError) as err:
        ctx.run(len(s["dts"]), s["dts"][0], 0.0)
    # ctx.step along the schedule could not reach this check: every call that returns drains the reports, so step 1 itself
    # would raise (the _last test).  Within one run the build of step 2 is the first to see the report; the two checks word
    # their errors differently, which is what tells them apart here
    assert "overflowed in the previous build" in str(err.value), str(err.value)
    with pytest.raises(capi.SphError):                # (stats() drains the reports too)
        ctx.stats()
    refused_from_now_on(capi, ctx, s["dts"][1])
    evaluates_after_fresh_upload(capi, ctx, name, flagset)
    ctx.close()


@pytest.mark.parametrize("flagset", TILED)
def test_too_fast_last_build_raises_from_the_call_that_returns(capi, flagset):
    """the overflowing build is the last of the call: drain_reports, at the end of that very call"""
    name = "contraction_too_fast_last"
    s = S.build(name)
    ctx = make_context(capi, s["gas"], flags=flags_of(capi, flagset))
    ctx.density(); ctx.forces()
    assert ctx.stats().nlist_capacity == S.NL_CAP0 and ctx.stats().nlist_max <= 72
    with pytest.raises(capi.SphError) as err:
        ctx.step(s["dts"][0], 0.0)
    assert "overflowed in the last build" in str(err.value), str(err.value)
    refused_from_now_on(capi, ctx, 0.01)
    evaluates_after_fresh_upload(capi, ctx, name, flagset)
    ctx.close()


@pytest.mark.parametrize("name", S.TOO_FAST)
def test_too_fast_sets_with_the_untiled_list_regrow_in_place(capi, name):
    """SPH_FLAG_NO_LDS_TILES: the list of pairs.hip waits for every build's own maximum, so the same schedules run through
    -- with the sums of the overflowing step checked like every other"""
    rec = steady_run(capi, name, "no_lds_tiles")
    grown = check_capacity(name, rec)
    print(f"{name}/no_lds_tiles: longest {rec['longest']}, capacity {[st.nlist_capacity for st in rec['stats']]}, grown in builds {grown}")
    assert grown == [1] and rec["longest"][1] >= 1.1 * S.NL_CAP0
    check_decisions(name, rec)
    check_rates(name, "no_lds_tiles", rec, special={1})
