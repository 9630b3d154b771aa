"""GPU: the 16-bit entries of the fixed-h tiled list at their limits (csrc/tile_common.hpp: an entry is the neighbour's slot
among the records of its group's three candidate intervals, the group's tile NEED; csrc/tiled.hip nlist_build_tiled and
csrc/api.hip drain_reports: the context leaves the tiled path when a need reaches HALF of 65536 -- on the build's own report
at the first build, on the previous build's in the steady state -- and a need that reaches 65536 within one step is an
error).  The sets are tests/steady_sets.py's dense cubes and aligned rows: tens of thousands of particles with 3000 to 6000
neighbours each; their construction conditions are asserted in tests/test_steady_sets_cpu.py, and every decision asserted
here is replayed on the host (steady_sets.need_replay, list16_replay, capacity_replay) from the positions the GPU run itself
went through.

  static edge      dense_cube_32767 stays tiled at its first build (a 16-bit list by capacity and by device_bytes),
                   dense_cube_32768 leaves it there and is from then on bitwise a SPH_FLAG_NO_LDS_TILES context -- also for a
                   later upload of a small sparse set: "for good" means the context, not the upload
  the window       dense_cube_window: the largest need grows into [32768, 65535] at build 2, the only build that writes
                   entries with bit 15 set; step 2 decodes them (ListColumn<true> in density_kernel and forces_kernel, and
                   in sph_force_terms) and is still tiled, without a host wait; build 3 reads the stale report and leaves,
                   never earlier.  A process with SPH_SYNC_EVERY_BUILD leaves at build 2 itself and never writes such an
                   entry, a SPH_FLAG_NO_LDS_TILES context never writes a 16-bit entry at all: both end in the same state
  the knot         sheet_with_knot: the same window inside a sheet on which the whole-tile kernels run (see below)
  within one step  rows_aligned_*: the need goes from 28001 to 69305 in one build while no list grows: SPH_ERR_STATE from the
                   next build (mid) or from the call that returns (last), every evaluation refused until an upload
The flag sets are the default and SPH_FLAG_NO_WHOLE_TILE, each also with SPH_FLAG_HASHED_GRID for the cubes (nlist_tiled<true>
has its own interval code).

Bars: the project's own, none from a GPU result -- rho within 1e-13 of each element's own value of the oracle's density
pass; P, c and the rates within EVAL_TOL (1e-13 of the field's scale) of the oracle; the rates and the sixteen rows of
sph_force_terms within the per-element rate bar (varh_ref.rate_excess <= 1) of the restatement tests/force_terms_ref on
a sample of targets (steady_sets.edge_targets: the first and last 64 slots of every group at or above 32768 and every fourth
of its targets among them); the entry count exact.  These sums have 1000 to 5800 terms where the earlier sets have about
100: whether 1e-13 per element is reachable was decided CPU against CPU (tests/test_steady_sets_cpu.py: the threaded oracle
against an extended-precision restatement differs by <= 6.8e-15 per element, within a tenth of the bar, so the bar stays
and the derived bound (k + 8) 2^-53 rho is not needed; the two CPU references use 2 % of the rate bar).


On the cubes every group misfits its tile, the whole-tile kernels are not chosen and ListColumn<true> decodes every entry.
sheet_with_knot brings such entries into the whole-tile kernels: 700000 particles of a thin sheet whose groups fit (tile fit
92 % and 93 %: density_wt without the table, forces_q with 256-target groups) around a knot of 54000 whose groups misfit and
take the fall-back loops: half_entry and the misfit loop of density_wt, ent_of of forces_q with four lanes a target.  The
eight-lane form of that loop (half groups) is NOT reached: it needs a sheet whose 256-target groups misfit while its
half groups fit, with the knot on top; no set here has that geometry (said beside ent_of in tiled.hip).
row_entry (tile_common.hpp), the sixth decode of such an entry in the source, is called by no kernel: its definition is its
only occurrence, so no test can reach it; a comment there says so.

Measured on the MI355X (18 tests, 65 s with 16 host threads for the references):
  needs per build against the replay   dense_cube_window 29840, 31250, 34600, 36000, 36000 (7 of 141 groups write bit-15 entries
                                       at build 2); sheet_with_knot 29927, 31872, 33905, 36166 (10 of 2946 groups); rows 28001 ->
                                       69305: the GPU run's positions replay to the oracle's figures, to the digit
  the step at which a context left     dense_cube_32768: build 0; the window and the knot: build 3 under every flag set (tile fit
                                       -1, the list's bytes doubled at the capacity in place), build 2 in the synchronous process
  the knot's list                      longest 2591, 2970, 3439, 4008 per build; capacity 3896, 3896, 4464, 4464 and nlist_max 2591,
                                       2591, 2970, 4008 after the first evaluation and the three steps, as replayed
  worst rho per element                1.25e-14 (static cubes), 1.44e-14 (window), 9.6e-15 (knot), 1.37e-14 (rows); bar 1e-13
  P, c and the rates against the oracle  <= 1.9e-14 of the field's scale (bar 1e-13)
  share of the per-element rate bar    rates 2.6 %, the rows of sph_force_terms 2.2 % (window); 0.3 % and 1.6 % (knot)
  against the untiled run              the cubes bitwise; the knot <= 1.1e-15; against the synchronous process <= 9.4e-16

Which tests fail on a scratch build of the library with one thing changed (each never committed, each run against this file
alone).  The first two rows are runs of the 18 tests as they stand.  The third row counts 17 tests: that build was not run
with the knot test, which by its code does not depend on that branch (no need reaches 65536 there).  The last five rows
are runs of the 18 tests with the knot test lacking its list assertions (capacity replay, nlist_max, dt decisions), which
none of those five changes touches:
  first-build guard 2 * need -> need (tiled.hip)       4 fail: need_32768 under the four flag sets (tile fit not -1); 14 pass
  the same in the trusted guard (tiled.hip)            5 fail: the window under the four flag sets and the knot (build 3 does
                                                       not leave); 13 pass
  the prev[3] >= 65536 error removed (tiled.hip)       2 fail: rows_aligned_mid [default, no_whole_tile] (no error); 15 pass
  the rep[3] term removed from drain_reports (api.hip) 2 fail: rows_aligned_last [default, no_whole_tile] (no error); 16 pass
  ListColumn<true> masks with 0x7fff, in pairs.o       4 fail: the window under the four flag sets (rho); 14 pass, the knot among
                                                       them -- its bit-15 entries never pass through this column
  the same column in terms.o                           5 fail: the window x 4 and the knot (the rows of sph_force_terms); 13 pass
  half_entry of density_wt masks with 0x7fff           1 fails: the knot (rho of the window step off by 0.24); 17 pass
  ent_of of forces_q masks with 0x7fff                 1 fails: the knot (the rates of the window step, 0.20 of the scale); 17 pass
How the two ListColumn builds are told apart: there is one ListColumn, in tile_common.hpp, instantiated by pairs.hip
(density_kernel, forces_kernel) and by terms.hip.  The mask is put into the header and ONE object is compiled against it --
pairs.o for the one build, terms.o for the other -- and linked with the product build's other objects.
A mask, never a sign extension: e & 0x7fff stays inside the group's own intervals, so such a build is wrong but in bounds.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import force_terms_ref as FT
import steady_sets as S
import test_steady_state_adversarial_gpu as T
import varh_ref as VR
from conftest import rel_err
from gpu_support import capi, make_context

pytestmark = pytest.mark.gpu

EVAL_TOL = T.EVAL_TOL
STATE8 = T.STATE8
ERR_STATE = 5                                        # include/summersph.h: SPH_ERR_STATE
TILED = ("default", "no_whole_tile")
VARIANTS = [(f, h) for h in (False, True) for f in TILED]
TERM_ROWS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 15]          # all but the gas self-gravity rows (NaN: skipped)


def flags_of(capi, flagset, hashed=False):
    return T.flags_of(capi, flagset) | (capi.FLAG_HASHED_GRID if hashed else 0)


def list_waves(n):
    """csrc/api.hip ensure_capacity: the waves the list is allocated for"""
    return ((n + n // 16 + 64) + 63) // 64


def list_bytes(n, cap, tiled):
    """a (wave, entry) cell of the list is 64 lanes of 2 bytes (tiled) or of 4"""
    return list_waves(n) * cap * (128 if tiled else 256)


def untiled_cap(cap, longest):
    """csrc/pairs.hip nlist_build: grows in place, on the build's own maximum"""
    return cap if longest <= cap else longest + longest // 8 + 8


# ---- one evaluation against its references ------------------------------------------------------------------------------
def check_sums(tag, state, got, st, worst, ps=None, ev=None):
    """the list's entry count exact, rho per element, P, c and the rates at EVAL_TOL against the threaded oracle"""
    n = state["x"].size
    for f, a in list(state.items()) + list(got.items()):
        assert np.all(np.isfinite(a)), (tag, f)
    ps = ps or S.pair_stats_binned(S.positions(state))
    entries = st.nlist_mean * n
    assert abs(entries - round(entries)) < 1e-5 and ps["entries_lo"] <= round(entries) <= ps["entries_hi"], \
        (tag, entries, ps["entries_lo"], ps["entries_hi"])
    ev = ev or S.oracle_eval({k: state[k] for k in S.STATE})
    e_rho = float(np.max(np.abs(got["rho"] - ev["rho"]) / ev["rho"]))
    worst["rho"] = max(worst["rho"], e_rho)
    print(f"{tag}: rho {e_rho:.2e} per element (bar 1e-13)")
    assert e_rho <= 1e-13, (tag, "rho", e_rho, int(np.argmax(np.abs(got["rho"] - ev["rho"]) / ev["rho"])))
    for f in ("P", "c") + S.RATES:
        e = rel_err(got[f], ev[f])
        worst["oracle"] = max(worst["oracle"], e)
        assert e <= EVAL_TOL, (tag, f, e)
    return ps, ev


class _Rows:
    def __init__(self, ref, tg):
        self.rows, self.scale = ref.rows[:, tg], ref.scale[:, tg]


def restate(state, tg):
    return FT.fixed_terms({k: state[k] for k in S.STATE}, S.NO_SINKS, h=S.H, targets=tg)


def check_restatement(tag, state, got, tg, worst, terms=None, ref=None):
    """the rates (and, where given, the sixteen rows of sph_force_terms) of the targets tg against the restatement, per element"""
    ref = ref or restate(state, tg)
    rates, scales = ref.recomposed()
    for i, f in enumerate(S.RATES):
        ex = float(np.max(VR.rate_excess(np.abs(got[f][tg] - rates[i][tg]), np.abs(rates[i][tg]), scales[i][tg])))
        worst["rates"] = max(worst["rates"], ex)
        assert ex <= 1.0, (tag, f, ex)
    if terms is not None:
        ex = FT.excess(terms[:, tg], _Rows(ref, tg), TERM_ROWS)
        worst["terms"] = max(worst["terms"], max(ex.values()))
        assert max(ex.values()) <= 1.0, (tag, "force_terms", ex)
    print(f"{tag}: {tg.size} targets against the restatement, share of the per-element bar: rates {worst['rates']:.2e}, "
          f"sph_force_terms {worst['terms']:.2e}")


def new_worst():
    return dict(rho=0.0, oracle=0.0, rates=0.0, terms=0.0)


# ---- the static edge ---------------------------------------------------------------------------------------------------
_STATIC = {}


def static_ref(name):
    """the references of a static cube, shared by its flag sets: pair statistics, the oracle's evaluation, the replay"""
    if name not in _STATIC:
        gas = S.build(name)["gas"]
        pos = S.positions(gas)
        box = S.exact_box(pos)
        fit = S.tile_fit_replay(pos, *box)
        tg = S.edge_targets(pos, *box, fit, least=int(fit["need"].max()))
        _STATIC[name] = dict(gas=gas, ps=S.pair_stats_binned(pos), ev=S.oracle_eval(gas), fit=fit, tg=tg, terms=restate(gas, tg))
    return _STATIC[name]


def evaluate(capi, gas, flags):
    ctx = make_context(capi, gas, flags=flags)
    ctx.density(); ctx.forces()
    return ctx, ctx.stats(), T.download(ctx, S.DERIVED)


@pytest.mark.parametrize("flagset,hashed", VARIANTS)
def test_need_32767_stays_tiled_at_the_first_build(capi, flagset, hashed):
    name = "dense_cube_32767"
    ref = static_ref(name)
    gas, n = ref["gas"], ref["gas"]["x"].size
    assert int(ref["fit"]["need"].max()) == n == 32767
    ctx, st, got = evaluate(capi, gas, flags_of(capi, flagset, hashed))
    twin, st_u, _ = evaluate(capi, gas, flags_of(capi, "no_lds_tiles", hashed))
    cap = S.capacity_replay([ref["ps"]["longest"]])[0]["cap"]
    print(f"{name}/{flagset}/hashed={hashed}: tile_fit_pct {st.tile_fit_pct}, {st.tile_fit_pct_forces}; capacity {st.nlist_capacity} "
          f"(replay {cap}; untiled {st_u.nlist_capacity}), device_bytes {st.device_bytes} against {st_u.device_bytes} untiled")
    assert st.nlist_builds == 1 and st.nlist_max == ref["ps"]["longest"]
    if flagset == "default":
        assert st.tile_fit_pct != -1 and st.tile_fit_pct_forces != -1
    # a 16-bit list: the tiled build's capacity (a half of headroom, in eights), and two bytes an entry -- the untiled
    # context on the same upload differs by exactly its list
    assert st.nlist_capacity == cap and st_u.nlist_capacity == untiled_cap(S.NL_CAP0, ref["ps"]["longest"])
    assert st_u.device_bytes - st.device_bytes == list_bytes(n, st_u.nlist_capacity, False) - list_bytes(n, cap, True)
    worst = new_worst()
    check_sums(f"{name}/{flagset}/hashed={hashed}", gas, got, st, worst, ref["ps"], ref["ev"])
    check_restatement(f"{name}/{flagset}/hashed={hashed}", gas, got, ref["tg"], worst, ctx.force_terms(skip_gas_gravity=True), ref["terms"])
    ctx.close(); twin.close()


@pytest.mark.parametrize("flagset,hashed", VARIANTS)
def test_need_32768_leaves_at_the_first_build_for_good(capi, flagset, hashed):
    name = "dense_cube_32768"
    ref = static_ref(name)
    gas, n = ref["gas"], ref["gas"]["x"].size
    assert int(ref["fit"]["need"].max()) == n == 32768
    ctx, st, got = evaluate(capi, gas, flags_of(capi, flagset, hashed))
    twin, st_u, got_u = evaluate(capi, gas, flags_of(capi, "no_lds_tiles", hashed))
    print(f"{name}/{flagset}/hashed={hashed}: tile_fit_pct {st.tile_fit_pct}, {st.tile_fit_pct_forces}; capacity {st.nlist_capacity} "
          f"(untiled {st_u.nlist_capacity}), device_bytes {st.device_bytes} against {st_u.device_bytes} untiled")
    assert st.tile_fit_pct == -1 and st.tile_fit_pct_forces == -1 and st.nlist_builds == 1
    # from here on the untiled context: the same list, the same kernels on the same order -- every field to the bit
    assert st.nlist_capacity == st_u.nlist_capacity == untiled_cap(S.NL_CAP0, ref["ps"]["longest"])
    assert st.device_bytes == st_u.device_bytes and st.nlist_mean == st_u.nlist_mean
    for f in S.DERIVED:
        assert np.array_equal(got[f], got_u[f]), (name, flagset, f)
    worst = new_worst()
    check_sums(f"{name}/{flagset}/hashed={hashed}", gas, got, st, worst, ref["ps"], ref["ev"])
    check_restatement(f"{name}/{flagset}/hashed={hashed}", gas, got, ref["tg"], worst, ctx.force_terms(skip_gas_gravity=True), ref["terms"])
    # "for good" is the context's, not the upload's (tiled.hip leave_tiled_path; sph_upload does not look at it again): a
    # small sparse set uploaded afterwards is evaluated untiled, bitwise like the untiled context, and steps
    small = S.build("contraction")["gas"]
    for c in (ctx, twin):
        c.upload(small)
        c.density(); c.forces()
    st, st_u = ctx.stats(), twin.stats()
    assert st.tile_fit_pct == -1 and st.tile_fit_pct_forces == -1
    assert st.nlist_capacity == st_u.nlist_capacity and st.nlist_mean == st_u.nlist_mean
    a, b = T.download(ctx, S.DERIVED), T.download(twin, S.DERIVED)
    for f in S.DERIVED:
        assert np.array_equal(a[f], b[f]), (name, flagset, "after the upload of a small set", f)
    ev = S.oracle_eval(small)
    assert float(np.max(np.abs(a["rho"] - ev["rho"]) / ev["rho"])) <= 1e-13
    dt, _ = ctx.step(1e-3, 0.0)
    assert dt > 0.0 and ctx.stats().tile_fit_pct == -1
    ctx.close(); twin.close()


# ---- the window ----------------------------------------------------------------------------------------------------------
_WINDOW = {}
WINDOW_BUILD, LEAVING_BUILD = 2, 3                 # asserted against the replay of the run's own positions


def window_run(capi, name, flagset, hashed=False):
    """dense_cube_window or sheet_with_knot along its schedule.  After every step: density and forces again (no new build, no
    host wait) and the state downloaded; the sums of that very step against their references -- every step for the cube
    under the default flag set on the dense grid, the window step and the leaving step for its other flag sets, the window
    step for the sheet (754000 particles: an evaluation of the oracle and an exact pair count take seconds each)"""
    key = (name, flagset, hashed)
    if key in _WINDOW:
        return _WINDOW[key]
    s = S.build(name)
    tag = f"{name}/{flagset}/hashed={hashed}"
    checked = () if flagset == "no_lds_tiles" else (WINDOW_BUILD,) if name == "sheet_with_knot" else \
        range(1, len(s["dts"]) + 1) if (flagset, hashed) == ("default", False) else (WINDOW_BUILD, LEAVING_BUILD)
    ctx = make_context(capi, s["gas"], flags=flags_of(capi, flagset, hashed))
    ctx.density(); ctx.forces()
    rec = dict(pos=[S.positions(s["gas"])], stats=[ctx.stats()], table=[ctx.grid_info().bytes], dts=[], bytes=[ctx.stats().device_bytes],
               states=[], worst=new_worst(), evals={})
    t, scratch = 0.0, 0
    for k, dt in enumerate(s["dts"], start=1):
        d, t = ctx.step(dt, t)
        rec["dts"].append(d)
        st = ctx.stats()
        ctx.density(); ctx.forces()
        again = ctx.stats()
        assert (again.nlist_builds, again.grid_builds, again.host_syncs) == (st.nlist_builds, st.grid_builds, st.host_syncs), (tag, k)
        assert st.nlist_builds == k + 1
        state = T.download(ctx, S.STATE)
        rec["pos"].append(S.positions(state)); rec["stats"].append(st); rec["states"].append(state)
        rec["table"].append(ctx.grid_info().bytes)
        rec["bytes"].append(st.device_bytes - scratch)
        if k not in checked:
            continue
        got = T.download(ctx, S.DERIVED)
        ps, ev = check_sums(f"{tag}/step {k}", state, got, st, rec["worst"])
        rec["evals"][k] = (state, got, ctx.force_terms(skip_gas_gravity=True) if k == WINDOW_BUILD else None, ps["longest"])
        scratch += ctx.stats().device_bytes - st.device_bytes          # (sph_force_terms keeps a scratch of its own from its first call on)
    rec["final"] = T.download(ctx, STATE8)
    ctx.close()
    _WINDOW[key] = rec
    return rec


_WINDOW_CHILD = {}


def window_child(capi, name, flagset, hashed=False):
    """the same schedule in a fresh process in which every build waits for its own report"""
    key = (name, flagset, hashed)
    if key not in _WINDOW_CHILD:
        tests = os.path.dirname(os.path.abspath(__file__))
        code = T._CHILD.format(root=os.path.dirname(tests), tests=tests, name=name, flags=flags_of(capi, flagset, hashed), min_syncs=2)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "child.npz")
            subprocess.run([sys.executable, "-c", code, path], check=True, env={**os.environ, "SPH_SYNC_EVERY_BUILD": "1"}, timeout=120)
            _WINDOW_CHILD[key] = dict(np.load(path))
    return _WINDOW_CHILD[key]


def check_window_plan(tag, rec):
    """the replay, on the positions this run went through: the window is build 2, build 3 leaves"""
    fits, needs = S.need_replay(rec["pos"])
    plan = S.list16_replay(needs)
    assert plan == ["tiled"] * (WINDOW_BUILD + 1) + ["leaves"] + ["untiled"] * (len(needs) - LEAVING_BUILD - 1), (tag, needs, plan)
    assert needs[WINDOW_BUILD - 1] < S.LIST16_HALF <= needs[WINDOW_BUILD] < S.LIST16_FULL
    return fits, needs, plan


def check_against_other_runs(capi, tag, name, flagset, hashed, rec):
    """independent references for the encoding: a process that waits for every report leaves one build earlier and never
    writes a bit-15 entry; the untiled context writes no 16-bit entry at all.  The same dt decisions, the same state"""
    others = {"the untiled run": window_run(capi, name, "no_lds_tiles", hashed)}
    if flagset == "default":
        others["the synchronous process"] = window_child(capi, name, flagset, hashed)
    for what, ref in others.items():
        assert list(ref["dts"]) == rec["dts"], (tag, what)
        final = ref["final"] if "final" in ref else ref
        errs = {f: rel_err(rec["final"][f], final[f]) for f in STATE8}
        print(f"{tag} against {what}:", {f: f"{v:.1e}" for f, v in errs.items()})
        assert max(errs.values()) <= 1e-12, (tag, what, errs)


@pytest.mark.parametrize("flagset,hashed", VARIANTS)
def test_window_step_decodes_bit_15_entries_and_the_next_build_leaves(capi, flagset, hashed):
    name = "dense_cube_window"
    n = S.build(name)["gas"]["x"].size
    tag = f"{name}/{flagset}/hashed={hashed}"
    rec = window_run(capi, name, flagset, hashed)
    stats, pos = rec["stats"], rec["pos"]
    fits, needs, plan = check_window_plan(tag, rec)
    longest = [S.pair_stats_binned(p)["longest"] if k not in rec["evals"] else rec["evals"][k][3] for k, p in enumerate(pos)]
    caps = S.capacity_replay(longest)
    assert needs == S.need_replay([S.positions(st) for st in S.trajectory(name)[0]])[1]          # ... and the oracle's needs
    T.check_decisions(name, rec)
    over = int(np.count_nonzero(fits[WINDOW_BUILD]["need"] >= S.LIST16_HALF))
    print(f"{tag}: needs per build {needs} ({over} groups write bit-15 entries at build {WINDOW_BUILD}), {plan}; longest {longest}; "
          f"capacity {[st.nlist_capacity for st in stats]}, tile_fit_pct {[st.tile_fit_pct for st in stats]}, host_syncs "
          f"{[st.host_syncs for st in stats]}, device_bytes {[st.device_bytes for st in stats]}")
    # tiled up to and including the window step: the capacity the tiled build's replay gives (regrown from stale reports
    # only), no host wait after the first build, and -- where the whole-tile digest runs -- a tile fit that is not -1
    assert not any(c["overflow"] for c in caps)
    for k in range(LEAVING_BUILD):
        assert stats[k].nlist_capacity == caps[k]["cap"], (tag, k, stats[k].nlist_capacity, caps[k])
        assert stats[k].host_syncs == stats[0].host_syncs, (tag, k)
        if k >= 1:
            assert stats[k].nlist_max == longest[k - 1], (tag, k)                       # the PREVIOUS build's report
        if k >= 2:                                      # (step 1 also regrows the cell table: the stale box has a guard cell)
            assert rec["table"][k] == rec["table"][k - 1]
            assert rec["bytes"][k] - rec["bytes"][k - 1] == \
                list_bytes(n, caps[k]["cap"], True) - list_bytes(n, caps[k - 1]["cap"], True), (tag, k)       # two bytes an entry
        if flagset == "default":
            assert stats[k].tile_fit_pct != -1 and stats[k].tile_fit_pct_forces != -1, (tag, k)
    # the build after the window leaves, at exactly that step: the 32-bit list in the capacity that was in place (grown by
    # the untiled rule where the build's own longest list exceeds it), four bytes an entry, no tile fit any more
    cap = caps[WINDOW_BUILD]["cap"]
    for k in range(LEAVING_BUILD, len(stats)):
        grown = untiled_cap(cap, longest[k])
        assert stats[k].nlist_capacity == grown and stats[k].nlist_max == longest[k], (tag, k, stats[k].nlist_capacity, grown)
        assert stats[k].tile_fit_pct == -1 and stats[k].tile_fit_pct_forces == -1, (tag, k)
        assert rec["table"][k] == rec["table"][k - 1]
        assert rec["bytes"][k] - rec["bytes"][k - 1] == \
            list_bytes(n, grown, False) - list_bytes(n, cap, k == LEAVING_BUILD), (tag, k)        # the build that leaves frees a 16-bit list
        cap = grown
    # the sums of the window step (checked against the oracle in window_run) and sph_force_terms inside the window against
    # the restatement, on the targets around the bit-15 entries
    state, got, terms, _ = rec["evals"][WINDOW_BUILD]
    box = S.build_boxes(pos)[WINDOW_BUILD]
    tg = S.edge_targets(pos[WINDOW_BUILD], *box, fits[WINDOW_BUILD])
    check_restatement(f"{tag}/step {WINDOW_BUILD}", state, got, tg, rec["worst"], terms)
    print(f"{tag}: worst rho {rec['worst']['rho']:.2e} per element, against the oracle {rec['worst']['oracle']:.2e} (bar {EVAL_TOL:g})")
    check_against_other_runs(capi, tag, name, flagset, hashed, rec)


# ---- the knot in the sheet: bit-15 entries in the fall-back loops of the whole-tile kernels ------------------------------------
def test_knot_in_a_sheet_brings_bit_15_entries_into_the_whole_tile_kernels(capi):
    """sheet_with_knot under the default flags: nine groups in ten fit their tiles in both geometries, so density_wt and
    forces_q run; the knot's groups misfit and take those kernels' fall-back loops (half_entry and the misfit loop of
    density_wt, ent_of of forces_q with four lanes a target), at build 2 with entries at or above 32768"""
    name, flagset = "sheet_with_knot", "default"
    tag = f"{name}/{flagset}"
    clump = S.build(name)["clump"]
    rec = window_run(capi, name, flagset)
    stats, pos = rec["stats"], rec["pos"]
    fits, needs, plan = check_window_plan(tag, rec)
    print(f"{tag}: needs per build {needs}, {plan}; tile_fit_pct {[st.tile_fit_pct for st in stats]} (replay per build "
          f"{[f['fit_pct'] for f in fits]}), tile_fit_pct_forces {[st.tile_fit_pct_forces for st in stats]} (replay {[f['fit_pct_forces'] for f in fits]}), "
          f"capacity {[st.nlist_capacity for st in stats]}, host_syncs {[st.host_syncs for st in stats]}")
    # the whole-tile kernels ran up to and including the window step: both fits >= 90, as the replay of the report they were
    # digested from says (build 0: its own; later: the previous build's), with 256-target forces groups; no host wait
    for k in range(LEAVING_BUILD):
        f = fits[max(k - 1, 0)]
        assert stats[k].tile_fit_pct >= 90 and stats[k].tile_fit_pct_forces >= 90, (tag, k)
        assert f["fit_pct"] >= 90 and f["ok_d"] and f["fit_pct_forces"] >= 90 and f["ok"] and not f["half"], (tag, k)
        assert (stats[k].tile_fit_pct, stats[k].tile_fit_pct_forces) == (f["fit_pct"], f["fit_pct_forces"]), (tag, k)
        assert stats[k].host_syncs == stats[0].host_syncs, (tag, k)
    for k in range(LEAVING_BUILD, len(stats)):
        assert stats[k].tile_fit_pct == -1 and stats[k].tile_fit_pct_forces == -1, (tag, k)
    # the list, as for the cube: the capacity the tiled build's replay gives on this run's own longest lists (regrown from
    # stale reports only, never overflowing), nlist_max the PREVIOUS build's longest list, then the 32-bit list in the capacity
    # in place.  The longest lists are the knot's: counted exactly on the knot's box, 2 h wider (complete for every particle
    # inside the box; the sheet's lists are a tenth as long) -- at the window step that is the whole set's count
    longest = []
    for q in pos:
        klo, khi = q[clump == 1].min(axis=0), q[clump == 1].max(axis=0)
        sub = np.flatnonzero(np.all((q >= klo - 1.01 * S.RCUT) & (q <= khi + 1.01 * S.RCUT), axis=1))
        inside = np.all((q[sub] >= klo) & (q[sub] <= khi), axis=1)
        longest.append(int(S.pair_stats_binned(q[sub])["per"][inside].max()))
    assert longest[WINDOW_BUILD] == rec["evals"][WINDOW_BUILD][3]
    caps = S.capacity_replay(longest)
    print(f"{tag}: longest {longest}, capacity replay {[(c['cap'], c['regrown']) for c in caps]}, nlist_max {[st.nlist_max for st in stats]}")
    assert not any(c["overflow"] for c in caps)
    for k in range(LEAVING_BUILD):
        assert stats[k].nlist_capacity == caps[k]["cap"], (tag, k, stats[k].nlist_capacity, caps[k])
        assert stats[k].nlist_max == longest[max(k - 1, 0)], (tag, k, stats[k].nlist_max, longest)
    cap = caps[WINDOW_BUILD]["cap"]
    for k in range(LEAVING_BUILD, len(stats)):
        cap = untiled_cap(cap, longest[k])
        assert stats[k].nlist_capacity == cap and stats[k].nlist_max == longest[k], (tag, k, stats[k].nlist_capacity, cap)
    # the needs and the dt decisions are the oracle's along the same schedule
    assert needs == S.need_replay([S.positions(st) for st in S.trajectory(name)[0]])[1]
    T.check_decisions(name, rec)
    # the groups that write bit-15 entries misfit in both geometries -- they are served by the fall-back loops -- and hold knot
    # particles only in part (the sheet's particles of the same cells sit among them)
    fit = fits[WINDOW_BUILD]
    flagged = np.flatnonzero(fit["need"] >= S.LIST16_HALF)
    assert flagged.size >= 2 and np.all(fit["need"][flagged] > S.TILE_CAP_Q[1]) and np.all(fit["need_d"][flagged // 4] > S.TILE_CAP_D[1])
    assert all(np.count_nonzero(clump[fit["order"][256 * g:256 * (g + 1)]] == 1) >= 128 for g in flagged)
    # the sums of the window step (against the oracle: window_run), and the restatement on the targets around the bit-15
    # entries: it needs every neighbour of a target with its own density, which the box of the targets, 4 h wider, holds
    state, got, terms, _ = rec["evals"][WINDOW_BUILD]
    p = pos[WINDOW_BUILD]
    box = S.build_boxes(pos)[WINDOW_BUILD]
    # (every particle of the flagged groups' first and last 64 slots is a target, the sheet's among them; the sampled rest is
    # drawn inside the knot's box, so that the box of the targets stays small)
    knot_box = np.flatnonzero(np.all(np.abs(p) <= np.abs(p[clump == 1]).max(axis=0), axis=1))
    tg = S.edge_targets(p, *box, fit, among=knot_box)
    for g in flagged:
        assert np.all(np.isin(fit["order"][fit["lo"][0][g]:fit["lo"][0][g] + 64], tg)) and fit["len"][0][g] > 0 and fit["len"][2][g] >= 64
        assert np.all(np.isin(fit["order"][fit["lo"][2][g] + fit["len"][2][g] - 64:fit["lo"][2][g] + fit["len"][2][g]], tg))
    sub = np.flatnonzero(np.all((p >= p[tg].min(axis=0) - 2.02 * S.RCUT) & (p <= p[tg].max(axis=0) + 2.02 * S.RCUT), axis=1))
    local = np.searchsorted(sub, tg)
    assert tg.size >= 512 and np.array_equal(sub[local], tg)
    check_restatement(f"{tag}/step {WINDOW_BUILD}", {k: state[k][sub] for k in S.STATE}, {k: got[k][sub] for k in S.RATES}, local,
                      rec["worst"], terms[:, sub])
    print(f"{tag}: worst rho {rec['worst']['rho']:.2e} per element, against the oracle {rec['worst']['oracle']:.2e} (bar {EVAL_TOL:g})")
    check_against_other_runs(capi, tag, name, flagset, False, rec)


# ---- the need passing 65536 within one step ---------------------------------------------------------------------------------
_ROWS = {}


def rows_ref():
    """the references of the rows sets' common first state"""
    if not _ROWS:
        gas = S.build("rows_aligned_last")["gas"]
        _ROWS.update(gas=gas, ps=S.pair_stats_binned(S.positions(gas)), ev=S.oracle_eval(gas))
    return _ROWS


def refused_until_upload(capi, ctx, dt):
    """density, forces, step, run, sph_force_terms and an analysis call: SPH_ERR_STATE, every time"""
    calls = dict(density=ctx.density, forces=ctx.forces, step=lambda: ctx.step(dt, 0.0), run=lambda: ctx.run(2, dt, 0.0),
                 force_terms=lambda: ctx.force_terms(skip_gas_gravity=True, refresh=True),
                 render=lambda: ctx.render_field("rho", 4, axis=2), rho=lambda: ctx.field("rho"), again=ctx.density)
    for what, call in calls.items():
        with pytest.raises(capi.SphError) as err:
            call()
        assert err.value.status == ERR_STATE, (what, str(err.value))


def works_after_upload(capi, ctx, tag):
    """the same set uploaded again: the first build waits for its own report, stays tiled and evaluates correctly"""
    ref = rows_ref()
    ctx.upload(ref["gas"])
    ctx.density(); ctx.forces()
    st = ctx.stats()
    check_sums(f"{tag} after a fresh upload", ref["gas"], T.download(ctx, S.DERIVED), st, new_worst(), ref["ps"], ref["ev"])
    assert st.nlist_max == ref["ps"]["longest"]
    dt, _ = ctx.step(1e-3, 0.0)
    assert dt > 0.0 and np.all(np.isfinite(ctx.field("rho")))


def rows_start(capi, name, flagset):
    """the context after its first evaluation, checked on the state before the move"""
    ref = rows_ref()
    s = S.build(name)
    ctx = make_context(capi, s["gas"], flags=flags_of(capi, flagset))
    ctx.density(); ctx.forces()
    st = ctx.stats()
    n = ref["gas"]["x"].size
    check_sums(f"{name}/{flagset} before the move", ref["gas"], T.download(ctx, S.DERIVED), st, new_worst(), ref["ps"], ref["ev"])
    # tiled, in a capacity that the move does not outgrow: the list-overflow check, which comes first, cannot fire
    cap = S.capacity_replay([ref["ps"]["longest"]])[0]["cap"]
    assert st.nlist_capacity == cap and st.device_bytes > 0 and st.nlist_builds == 1
    if flagset == "default":
        assert st.tile_fit_pct != -1
    return s, ctx, n


@pytest.mark.parametrize("flagset", TILED)
def test_rows_aligned_mid_run_raises_at_the_next_build(capi, flagset):
    name = "rows_aligned_mid"
    s, ctx, n = rows_start(capi, name, flagset)
    with pytest.raises(capi.SphError) as err:
        ctx.run(len(s["dts"]), s["dts"][0], 0.0)
    # the list-overflow check comes first in nlist_build_tiled; no list grew, so it is the 16-bit check that speaks
    assert err.value.status == ERR_STATE and "outgrew the 16-bit entries within one step" in str(err.value), str(err.value)
    assert "overflowed in the previous build" not in str(err.value)
    refused_until_upload(capi, ctx, s["dts"][1])
    works_after_upload(capi, ctx, f"{name}/{flagset}")
    ctx.close()


@pytest.mark.parametrize("flagset", TILED)
def test_rows_aligned_last_build_raises_from_the_call_that_returns(capi, flagset):
    name = "rows_aligned_last"
    s, ctx, n = rows_start(capi, name, flagset)
    with pytest.raises(capi.SphError) as err:
        ctx.step(s["dts"][0], 0.0)
    assert err.value.status == ERR_STATE and "candidate intervals grew beyond their headroom" in str(err.value), str(err.value)
    refused_until_upload(capi, ctx, 0.01)
    works_after_upload(capi, ctx, f"{name}/{flagset}")
    ctx.close()


def test_rows_aligned_with_the_untiled_list_runs_through(capi):
    """SPH_FLAG_NO_LDS_TILES: 32-bit entries, nothing to outgrow -- the schedule of rows_aligned_mid (its first step is all of
    rows_aligned_last's) runs through, every step's sums at the bars"""
    name = "rows_aligned_mid"
    s = S.build(name)
    ctx = make_context(capi, s["gas"], flags=flags_of(capi, "no_lds_tiles"))
    worst, t, dts = new_worst(), 0.0, []
    for k, dt in enumerate(s["dts"], start=1):
        d, t = ctx.step(dt, t)
        dts.append(d)
        ctx.density(); ctx.forces()
        state = T.download(ctx, S.STATE)
        check_sums(f"{name}/no_lds_tiles/step {k}", state, T.download(ctx, S.DERIVED), ctx.stats(), worst)
        if k == 1:
            pos = S.positions(state)
            needs = S.need_replay([S.positions(s["gas"]), pos])[1]
            assert needs[0] < S.LIST16_HALF and needs[1] >= S.LIST16_FULL, needs          # the build a tiled context fails on
            tg = np.sort(np.random.default_rng(5).choice(pos.shape[0], 512, replace=False))
            check_restatement(f"{name}/no_lds_tiles/step 1", state, T.download(ctx, S.DERIVED), tg, worst)
    assert all(d > 0.0 for d in dts) and ctx.stats().tile_fit_pct == -1
    print(f"{name}/no_lds_tiles: needs {needs}; rho {worst['rho']:.2e}, oracle {worst['oracle']:.2e}, rate share {worst['rates']:.2e}")
    ctx.close()
