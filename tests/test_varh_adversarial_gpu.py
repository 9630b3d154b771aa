"""GPU: the variable-h pair passes and the h update (csrc/varh.hip: leaf boxes from sorted path keys, the cell scan pruned by
a per-cell maximum of h, the D/F/R list with its margin shell, the in-place re-flag pass, forces_v, update_h with its three
evaluation routes and three clamps) on particle sets built to break them (tests/varh_sets.py), with LIVE fields.

Two references.  Sets of up to ~3000 particles are compared with the brute-force numpy restatement tests/varh_ref.py
(the "kernel" mode of DESIGN section 2's coincident-point deviation where a set has coincident points): rho and Omega
within 1e-13 of each element's OWN value, every rate within 1e-11 of its own magnitude plus 1e-13 of the sum of the
magnitudes of its terms (a local scale: in a set with a density contrast of 1e5 the field's maximum says nothing about the
diffuse part), h after calc_smoothing within 1e-12 per element, the dt decision identical, and the number of list entries
a build produced EXACTLY equal to the restatement's count of (i, j) with j in D_i or {i, j} a force pair -- the check that
sees a pair whose kernel weight is too small to show in rho.  The full-size sets are compared with the CPU oracle
(oracle/sph_oracle_v.c, pinned to the restatement on the same families by tests/test_varh_ref_cpu.py) at the bars of
tests/test_parity_var_gpu.py.  No bar here comes from a GPU result; between the two CPU references every set meets the
project's bars with orders of margin (tests/test_varh_ref_cpu.py's docstring), so none needed a measured floor.

The construction conditions of the sets (what makes each adversarial) are asserted in tests/test_varh_ref_cpu.py.

Measured on the MI355X (153 tests, 25 s with 16 host threads for the references): rho <= 5.7e-15 and Omega <= 4.8e-15 per
element, the rates <= 1.8 % of their per-element bar (full-size sets: <= 2.4e-15 of the field's scale, |a| <= 1.9e-14 per
element), h <= 1.1e-15, every count exact.  Before the boundary cells of the list build's gap tests were made open-ended
(csrc/varh.hip axis_gap2) the far_clump cases failed on the dense trimmed grid: the clump's rho was m W(0), up to 95 % low."""
import numpy as np
import pytest

import varh_ref as VR
import varh_sets as S
from conftest import rel_err
from gpu_support import capi, make_context

pytestmark = pytest.mark.gpu

RATES = ("ax", "ay", "az", "du", "dalpha")
STATE = "x y z vx vy vz u alpha h".split()
COUNT_SETS = [n for n in S.ALL if n not in S.HAS_TIES and n not in S.HAS_COINCIDENT]
BIG = ["lattice17", "lattice33", "lattice_ties", "sheet", "plummer", "sparse_cube", "two_clusters",
       "far_clump", "far_clump_x_only", "far_clump_low"]
FLAGSETS = ("default", "no_reflag", "hashed")


def flags_of(capi, flagset):
    return {"default": 0, "no_reflag": capi.FLAG_NO_REFLAG, "hashed": capi.FLAG_HASHED_GRID}[flagset]


def make_ctx(capi, gas, flags=0):
    return make_context(capi, gas, variable=True, flags=capi.FLAG_VARIABLE_H | flags)


def mode_of(name):
    return "kernel" if name in S.HAS_COINCIDENT else "reference"


_SMALL, _BIG = {}, {}


def small_case(name):
    """(gas, VarhRef evaluated and with one calc_smoothing pass, the dt decision for dt = 1e-2)"""
    if name not in _SMALL:
        gas = S.build(name, small=True)
        ref = VR.VarhRef(gas, coincident=mode_of(name)).evaluate()
        ref.update_h()
        _SMALL[name] = (gas, ref, VR.next_dt(ref, 1e-2))
    return _SMALL[name]


def oracle_of(gas):
    from oracle import orc, orc_v
    return orc_v.OracleV(gas, S.NO_SINKS, nthreads=orc.max_threads())


def big_case(name):
    """(gas, the oracle's fields of one evaluation, its dt decision for dt = 1e-2, h and rho after update_h)"""
    if name not in _BIG:
        gas = S.build(name, small=False)
        o = oracle_of(gas)
        o.evaluate()
        out = {f: getattr(o, f).copy() for f in ("rho", "omega") + RATES}
        out["dt"] = o.next_dt(1e-2)
        o.update_h()
        out["h_new"] = o.h.copy()
        _BIG[name] = (gas, out)
    return _BIG[name]


def fields(ctx, names):
    return {f: ctx.field(f) for f in names}


def check_against_restatement(tag, got, ref):
    """one evaluation on the GPU (dict of fields) against an evaluated VarhRef, per element"""
    for f in ("rho", "omega") + RATES:
        assert np.all(np.isfinite(got[f])), (tag, f)
    e_rho = float(np.max(np.abs(got["rho"] - ref.rho) / ref.rho))
    e_om = float(np.max(np.abs(got["omega"] - ref.omega) / np.abs(ref.omega)))
    a_g, a_r = np.stack([got[f] for f in ("ax", "ay", "az")]), np.stack([ref.ax, ref.ay, ref.az])
    ex = {"a": VR.rate_excess(np.linalg.norm(a_g - a_r, axis=0), np.linalg.norm(a_r, axis=0), ref.a_scale),
          "du": VR.rate_excess(np.abs(got["du"] - ref.du), np.abs(ref.du), ref.du_scale),
          "dalpha": VR.rate_excess(np.abs(got["dalpha"] - ref.dalpha), np.abs(ref.dalpha), ref.dalpha_scale)}
    print(f"{tag}: rho {e_rho:.2e} omega {e_om:.2e} (bar 1e-13); share of the rate bars used: "
          + " ".join(f"{k} {float(np.max(v)):.2e}" for k, v in ex.items()))
    worst = int(np.argmax(np.abs(got["rho"] - ref.rho) / ref.rho))
    assert e_rho <= 1e-13, (tag, "rho", worst, got["rho"][worst], ref.rho[worst])
    assert e_om <= 1e-13, (tag, "omega")
    for k, v in ex.items():
        assert float(np.max(v)) <= 1.0, (tag, k, int(np.argmax(v)))


def check_h(tag, h_gpu, h_ref, masks=None):
    e = np.abs(h_gpu - h_ref) / h_ref
    print(f"{tag}: h after calc_smoothing {float(np.max(e)):.2e} (bar 1e-12)")
    for k, m in (masks or {}).items():
        assert float(np.max(e[m])) <= 1e-12, (tag, k, int(np.flatnonzero(m)[np.argmax(e[m])]))
    assert float(np.max(e)) <= 1e-12, (tag, int(np.argmax(e)))


def check_grid(capi, ctx, name, flagset, n):
    """far_clump: the grid is dense and trimmed to the bulk (the clump sits in clamped boundary cells); hashed where forced"""
    gi = ctx.grid_info()
    if flagset == "hashed":
        assert gi.kind == 1, name
    elif name.startswith("far_clump"):
        assert gi.kind == 0 and ctx.stats().n_cells < 64 * n + 4_100_000, (name, gi.kind, ctx.stats().n_cells)


# ---- single evaluation, counts and the h update after a build -----------------------------------------------------------
@pytest.mark.parametrize("flagset", FLAGSETS)
@pytest.mark.parametrize("name", S.ALL)
def test_evaluation_counts_and_h_update_vs_restatement(capi, name, flagset):
    gas, ref, dt_ref = small_case(name)
    n = ref.n
    ctx = make_ctx(capi, gas, flags_of(capi, flagset))
    ctx.density(); ctx.forces()
    st = ctx.stats()
    check_grid(capi, ctx, name, flagset, n)
    assert st.nlist_builds == 1 and st.nlist_reflags == 0
    tag = f"{name}/{flagset}"
    if name.startswith("far_clump"):
        _, is_clump = S.far_clump(name[10:] or "corner", n_disc=2900, n_clump=40)
        rho = ctx.field("rho")
        e = np.abs(rho - ref.rho)[is_clump] / ref.rho[is_clump]
        print(f"{tag}: rho of the clamped clump, per element: {float(np.max(e)):.2e}")
        assert float(np.max(e)) <= 1e-13, (tag, "clump rho", rho[is_clump][:4], ref.rho[is_clump][:4])
    if name in COUNT_SETS:
        entries = st.nlist_mean * n
        print(f"{tag}: list entries {entries:.1f}, restatement {ref.n_list_entries}")
        assert round(entries) == ref.n_list_entries and abs(entries - round(entries)) < 1e-6, (tag, entries, ref.n_list_entries)
    if name == "list_regrow_v":
        assert st.nlist_capacity > 96 and st.nlist_capacity >= st.nlist_max > 96, (st.nlist_capacity, st.nlist_max)
    check_against_restatement(tag, fields(ctx, ("rho", "omega") + RATES), ref)
    assert ctx.next_dt(1e-2) == dt_ref, tag
    # calc_smoothing right after a build: the list route is available
    ctx.update_h()
    masks = VR.route_classes(ref.h_record) if name == "h_routes" else None
    check_h(tag, ctx.field("h"), ref.h_new, masks)
    assert ctx.stats().nlist_reflags == 0
    ctx.close()


REEVAL_SETS = {"plummer", "clump_in_halo", "lattice17", "two_clusters", "far_clump", "h_routes"}
REFLAG_CASES = [(n, "default") for n in S.ALL] + [(n, "hashed") for n in ("plummer", "clump_in_halo", "far_clump", "h_routes")]


@pytest.mark.parametrize("name,flagset", REFLAG_CASES)
def test_reflagged_list_and_cell_walk_h_update_vs_restatement(capi, name, flagset):
    """evaluate / update_h until the lengths have settled enough for an evaluation to RE-FLAG the list in place instead of
    building it (no h grew by more than the list's margin): that evaluation against the restatement of the same state,
    then calc_smoothing on the re-flagged list, which has lost its margin shell -- every re-evaluation takes the cell walk"""
    gas, _, _ = small_case(name)
    ctx = make_ctx(capi, gas, flags_of(capi, flagset))
    if name in S.HAS_COINCIDENT:
        def advance(h):                      # (the oracle divides by zero at coincident points, as the reference does)
            r = VR.VarhRef(dict(gas, h=h), coincident="kernel").evaluate()
            r.update_h()
            return r.h_new
    else:
        o = oracle_of(gas)

        def advance(h):
            assert np.array_equal(o.h, h)
            o.evaluate(); o.update_h()
            return o.h.copy()
    h = gas["h"].copy()
    reflagged = False
    for it in range(14):
        before = ctx.stats().nlist_reflags
        ctx.density(); ctx.forces()
        reflagged = ctx.stats().nlist_reflags == before + 1
        if reflagged:
            break
        ctx.update_h()
        h = advance(h)
    tag = f"{name}/{flagset}/reflagged after {it} updates"
    assert reflagged, tag
    check_h(tag + " (lengths going in)", ctx.field("h"), h)
    ref = VR.VarhRef(dict(gas, h=h), coincident=mode_of(name)).evaluate()
    check_against_restatement(tag, fields(ctx, ("rho", "omega") + RATES), ref)
    # The lengths have settled, so hardly any particle would re-evaluate now.  Hand both sides a density that is too low by a
    # seeded factor (rho is an uploadable field; the list stays as it is): the Newton steps grow by up to ~20 % and the
    # particles re-evaluate rho with trial lengths on both sides of 1.1 h0 -- all on the cell walk.
    low = ref.rho * np.random.default_rng(7).uniform(0.4, 1.0, ref.n)
    ctx.upload_field("rho", low)
    ref.rho = low
    rec = ref.update_h()
    ctx.update_h()
    n_re = int(np.count_nonzero(rec.n_reeval))
    print(f"{tag}: {n_re} particles re-evaluated on the cell walk, largest trial {float(np.max(rec.max_trial)):.3f} h0")
    if name in REEVAL_SETS:
        assert n_re >= 200 and float(np.max(rec.max_trial)) > VR.H_MARGIN, (tag, n_re)
    check_h(tag, ctx.field("h"), ref.h_new)
    assert ctx.stats().nlist_reflags == 1
    ctx.close()


# ---- the full-size sets against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("flagset", FLAGSETS)
@pytest.mark.parametrize("name", BIG)
def test_full_size_sets_vs_oracle(capi, name, flagset):
    gas, want = big_case(name)
    n = gas["x"].size
    ctx = make_ctx(capi, gas, flags_of(capi, flagset))
    ctx.density(); ctx.forces()
    check_grid(capi, ctx, name, flagset, n)
    tag = f"{name}/{flagset}"
    got = fields(ctx, ("rho", "omega") + RATES)
    for f in got:
        assert np.all(np.isfinite(got[f])), (tag, f)
    e_rho = float(np.max(np.abs(got["rho"] - want["rho"]) / want["rho"]))
    e_om = float(np.max(np.abs(got["omega"] - want["omega"]) / np.abs(want["omega"])))
    a = np.sqrt(got["ax"] ** 2 + got["ay"] ** 2 + got["az"] ** 2)
    aref = np.sqrt(want["ax"] ** 2 + want["ay"] ** 2 + want["az"] ** 2)
    big = aref > 1e-3 * np.max(aref)
    e_a = float(np.max(np.abs(a[big] - aref[big]) / aref[big])) if np.any(big) else 0.0
    e_f = {f: rel_err(got[f], want[f]) for f in RATES}
    print(f"{tag}: rho {e_rho:.2e} omega {e_om:.2e} (per element, bar 1e-13) |a| {e_a:.2e} (per element, bar 1e-11) "
          + " ".join(f"{f} {v:.2e}" for f, v in e_f.items()) + " (field scale, bar 1e-13)")
    if name.startswith("far_clump"):
        _, is_clump = S.far_clump(name[10:] or "corner")
        e = np.abs(got["rho"] - want["rho"])[is_clump] / want["rho"][is_clump]
        assert float(np.max(e)) <= 1e-13, (tag, "clump rho", got["rho"][is_clump][:4], want["rho"][is_clump][:4])
    assert e_rho <= 1e-13 and e_om <= 1e-13, tag
    assert e_a <= 1e-11, tag
    for f, v in e_f.items():
        assert v <= 1e-13, (tag, f)
    assert ctx.next_dt(1e-2) == want["dt"], tag
    ctx.update_h()
    check_h(tag, ctx.field("h"), want["h_new"])
    ctx.close()


# ---- re-flag = build over a few steps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plummer", "clump_in_halo", "lattice17", "far_clump"])
def test_reflag_equals_build_over_steps(capi, name):
    """8 steps with and without the re-flag pass: identical dt decisions, the pass really ran, builds + re-flags of the
    one run = builds of the other, and the same state at the bar of test_reflag_equals_build_over_a_trajectory (1e-13)"""
    gas, _, _ = small_case(name)
    out = {}
    for tag, flags in (("build", capi.FLAG_NO_REFLAG), ("reflag", 0)):
        ctx = make_ctx(capi, gas, flags)
        dts, t = [1e-3], 0.0
        for _ in range(8):
            dt, t = ctx.run(1, dts[-1], t)
            dts.append(dt)
        st = ctx.stats()
        out[tag] = dict(dts=dts, reflags=st.nlist_reflags, builds=st.nlist_builds, **fields(ctx, STATE + ["rho"]))
        ctx.close()
    print(name, "builds/reflags:", out["build"]["builds"], out["build"]["reflags"], out["reflag"]["builds"], out["reflag"]["reflags"],
          {f: f"{rel_err(out['reflag'][f], out['build'][f]):.1e}" for f in STATE + ["rho"]})
    assert out["build"]["reflags"] == 0 and out["reflag"]["reflags"] >= 1
    assert out["reflag"]["builds"] + out["reflag"]["reflags"] == out["build"]["builds"]
    assert out["build"]["dts"] == out["reflag"]["dts"]
    for f in STATE + ["rho"]:
        assert rel_err(out["reflag"][f], out["build"][f]) <= 1e-13, (name, f)


# ---- short trajectories against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plummer", "clump_in_halo", "far_clump"])
def test_short_trajectory_vs_oracle(capi, name):
    """4 steps against OracleV.step: identical dt decisions, the state at the variable-h trajectory bar (1e-10)"""
    gas, _, _ = small_case(name)
    ctx = make_ctx(capi, gas)
    o = oracle_of(gas)
    dts, dto, t = [1e-3], [1e-3], 0.0
    for _ in range(4):
        dt, t = ctx.step(dts[-1], t)
        dts.append(dt)
        dto.append(o.step(dto[-1]))
    errs = {f: rel_err(ctx.field(f), getattr(o, f)) for f in STATE}
    print(name, dts, {f: f"{v:.1e}" for f, v in errs.items()})
    assert dts == dto
    for f, v in errs.items():
        assert v <= 1e-10, (name, f)
    ctx.close()


# ---- the fixed-h twin of far_clump ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags_name", ["default", "no_whole_tile", "no_lds_tiles"])
def test_far_clump_fixed_h_twin(capi, flags_name):
    """fixed h: the build scans +-1 cell without a distance test, so a clump clamped into boundary cells still meets its
    neighbours (grid.hip's comment) -- through all three kernel sets, the clump's rho per element"""
    from oracle import orc
    gas, sinks, is_clump = S.far_clump_fixed()
    n = gas["x"].size
    flags = {"default": 0, "no_whole_tile": capi.FLAG_NO_WHOLE_TILE, "no_lds_tiles": capi.FLAG_NO_LDS_TILES}[flags_name]
    ctx = capi.Context(device=0, flags=flags)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()
    assert ctx.grid_info().kind == 0 and ctx.stats().n_cells < 64 * n + 4_100_000
    o = orc.Oracle(gas, sinks, nthreads=orc.max_threads())
    o.evaluate()
    rho = ctx.field("rho")
    assert float(np.max(np.abs(rho - o.rho) / o.rho)) <= 1e-13
    own = rho[is_clump] / (gas["m"][is_clump] / (3.14159265359 * 2.5 ** 3))                  # rho over the self term m W(0)
    assert np.min(own) > 1.0 and np.median(own) > 3.0                                       # the clump members see each other
    for f in ("P", "c") + RATES:
        assert rel_err(ctx.field(f), getattr(o, f)) <= 1e-13, f
        assert rel_err(ctx.field(f)[is_clump], getattr(o, f)[is_clump]) <= 1e-13, (f, "clump")
    ctx.close()


# ---- edge cases: the variable-h twin of test_parity_gpu.test_edge_cases ------------------------------------------------------
def _tiny(pos, seed):
    pos = np.asarray(pos, dtype=np.float64)
    return S.live({"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "m": np.full(pos.shape[0], 1.0e-3)},
                  seed, h=np.full(pos.shape[0], 1.5))


def test_edge_cases_variable_h(capi):
    from oracle import orc
    # empty set through every call
    ctx = capi.Context(device=0, variable=True)
    ctx.upload({k: np.zeros(0) for k in "x y z vx vy vz u m alpha".split()})
    ctx.density(); ctx.forces(); ctx.update_h()
    ctx.step(1e-2, 0.0)
    assert ctx.n == 0
    ctx.close()
    # one particle: the root box has edge 0 and is the leaf; rho = m W(0) / (pi h^3), Omega = 2 from the self term alone,
    # no pair terms; calc_smoothing as the restatement (hn = 1.73 h for a particle alone: re-evaluated on the cell walk)
    w0 = orc.tables(2500)[0][0]
    one = _tiny([[1.0, -2.0, 0.5]], 5)
    ctx = make_ctx(capi, one)
    ctx.density(); ctx.forces()
    h = one["h"][0]
    assert ctx.field("rho")[0] == pytest.approx(one["m"][0] * w0 / (VR.KERNEL_PI * h ** 3), rel=1e-15)
    assert ctx.field("omega")[0] == pytest.approx(2.0, rel=1e-15)
    assert all(ctx.field(f)[0] == 0.0 for f in ("ax", "ay", "az", "du"))
    ref = VR.VarhRef(one).evaluate()
    ref.update_h()
    assert ref.h_record.n_reeval[0] >= 1
    ctx.update_h()
    check_h("one particle", ctx.field("h"), ref.h_new)
    ctx.close()
    # two and three particles, collinear and coplanar sets (degenerate root boxes: one or two axes of extent 0)
    sets = {"two": [[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]],
            "three": [[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [-0.5, 1.0, 2.0]],
            "collinear_axis": [[0.5 * k, 2.0, -1.0] for k in range(7)],
            "collinear_diagonal": [[0.3 * k, 0.3 * k, 0.3 * k] for k in range(6)],
            "coplanar": [[0.7 * (k % 3), 0.9 * (k // 3), 3.0] for k in range(9)]}
    for k, (name, pos) in enumerate(sets.items()):
        gas = _tiny(pos, 10 + k)
        ref = VR.VarhRef(gas).evaluate()
        ref.update_h()
        assert ref.n_list_entries >= 2, name
        for flagset in FLAGSETS:
            ctx = make_ctx(capi, gas, flags_of(capi, flagset))
            ctx.density(); ctx.forces()
            check_against_restatement(f"{name}/{flagset}", fields(ctx, ("rho", "omega") + RATES), ref)
            assert round(ctx.stats().nlist_mean * ref.n) == ref.n_list_entries, name
            assert ctx.next_dt(1e-2) == VR.next_dt(ref, 1e-2), name
            ctx.update_h()
            check_h(f"{name}/{flagset}", ctx.field("h"), ref.h_new)
            ctx.close()
