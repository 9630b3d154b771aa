"""CPU: the CONSTRUCTION CONDITIONS of the sets of tests/steady_sets.py -- what each was built to do to the steady state of
the fixed-h step is asserted here, from the CPU oracle's trajectory along the set's schedule (oracle.orc.Oracle.step, in
pieces where the oracle's own dense grid could not hold the box), so that a set which lost its property fails here
instead of letting tests/test_steady_state_adversarial_gpu.py pass vacuously.  The decisions the code will take are
replayed on the host (steady_sets.capacity_replay: csrc/tiled.hip nlist_build_tiled; steady_sets.grid_replay: csrc/grid.hip
grid_rebuild) and the GPU file asserts that they happened.

Measured (8 host threads): 18 s for the file, 12 of them the 8000-particle sheet.  contraction: longest list 58 -> 310 in eleven steps, at most x 1.24 per step,
five regrows from the stale report; too fast: 58 -> 125 in one step (capacity 96); clumps_apart: 71 % to 84 % of the
particles outside the stale box at every step, cells 6.9e3 -> 3.4e5 -> 1.8e6 -> 5.1e6 and beyond; clumps_together: 2.3e9 cells
at the first build, dense from the fifth, longest list 47 -> 330 in ten steps and back to 49 in two."""
import numpy as np
import pytest

import steady_sets as S

_CASE = {}


def case(name, run=False):
    """(set, states, positions per build, pair statistics per build, capacity replay, grid replay, dt record)"""
    key = (name, run)
    if key not in _CASE:
        s = S.build(name)
        if run:
            states, dts, t = S.run_trajectory(name)
            record = (dts, t)
        else:
            states, record = S.trajectory(name)
        pos = [S.positions(st) for st in states]
        stats = [S.pair_stats(p) for p in pos]
        _CASE[key] = (s, states, pos, stats, S.capacity_replay([p["longest"] for p in stats]), S.grid_replay(pos), record)
    return _CASE[key]


CASES = [(n, False) for n in S.SMALL + S.TOO_FAST + ["sheet_puffing_up"]] + [("contraction", True)]


@pytest.mark.parametrize("name,run", CASES)
def test_set_is_as_specified_and_stays_finite(name, run):
    s, states, pos, stats, caps, grid, record = case(name, run)
    gas = s["gas"]
    n = gas["x"].size
    assert (n <= 4000 or name == "sheet_puffing_up") and all(gas[k].shape == (n,) and gas[k].dtype == np.float64 for k in S.STATE)
    assert 0.05 <= gas["alpha"].min() and gas["alpha"].max() <= 1.0 and 0.5 <= gas["u"].min() and gas["u"].max() <= 2.0
    assert np.all(gas["m"] == S.MASS)
    again = S.BUILDERS[name]()["gas"]
    assert all(np.array_equal(gas[k], again[k]) for k in S.STATE)                       # seeded
    # the viscosity is on: approaching pairs among the neighbours of the first state (a sample of targets is enough)
    v = np.stack([gas["vx"], gas["vy"], gas["vz"]], axis=1)
    approaching = 0
    for i in range(0, n, 97):
        d = pos[0] - pos[0][i]
        near = (np.sum(d * d, axis=1) <= S.RCUT ** 2) & (np.arange(n) != i)
        approaching += int(np.count_nonzero(np.sum((v[near] - v[i]) * d[near], axis=1) < 0.0))
    assert approaching >= 50, approaching
    for k, st in enumerate(states):
        for f, a in st.items():
            assert np.all(np.isfinite(a)), (name, k, f)
        assert np.all(st["u"] > 0.0) and (k == 0 or np.all(st["rho"] > 0.0)), (name, k)
        # no pair within 1e-9 (relative) of r = 2 h: the exact counts of the GPU file are well defined, and the trajectories of
        # the oracle and of the GPU (which agree to ~1e-12) count the same pairs
        assert stats[k]["near"] == 0 and stats[k]["entries_lo"] == stats[k]["entries"] == stats[k]["entries_hi"], (name, k)
    if run:
        dts, t = record
        assert len(dts) == s["run"][0] + 1 and dts[0] == s["run"][1] and len(set(dts)) >= 3, dts       # the control acts
    else:
        assert len(record) == len(s["dts"]) and all(d > 0.0 for d in record)


@pytest.mark.parametrize("run", [False, True])
def test_contraction_regrows_from_stale_reports_and_never_overflows(run):
    s, states, pos, stats, caps, grid, record = case("contraction", run)
    longest = [p["longest"] for p in stats]
    print("contraction", "run" if run else "schedule", longest, [(c["cap"], c["regrown"]) for c in caps])
    assert longest[0] <= 72 and caps[0]["cap"] == S.NL_CAP0                    # fits the initial slots with its headroom
    ratios = [b / a for a, b in zip(longest, longest[1:])]
    assert max(ratios) < 4.0 / 3.0, max(ratios)
    assert not any(c["overflow"] for c in caps)
    assert sum(c["regrown"] for c in caps) >= 2
    if not run:
        assert longest[-1] > 200
        assert max(ratios) < 1.3                                                # a clear margin to the third of headroom
    # a regrow is decided on a report one build old: the list that crossed 3/4 is the PREVIOUS build's
    for k, c in enumerate(caps):
        if c["regrown"]:
            assert 4 * longest[k - 1] > 3 * caps[k - 1]["cap"] and longest[k] <= c["cap"] and c["cap"] % 8 == 0
    # nothing else happens to this set: one dense grid within the first table, no particle outside the stale box
    assert all(g["kind"] == 0 and g["rounds"] == 0 and not g["outside"].any() for g in grid)


@pytest.mark.parametrize("name", S.TOO_FAST)
def test_too_fast_sets_overflow_in_the_second_build_by_a_clear_margin(name):
    s, states, pos, stats, caps, grid, record = case(name)
    longest = [p["longest"] for p in stats]
    print(name, longest, [(c["cap"], c["overflow"]) for c in caps])
    assert longest[0] <= 72 and 4 * longest[0] <= 3 * S.NL_CAP0 and caps[0]["cap"] == S.NL_CAP0
    assert not caps[0]["overflow"] and caps[1]["overflow"] and not caps[1]["regrown"] and caps[1]["cap"] == S.NL_CAP0
    # >= 10 % beyond the capacity: the ~1e-12 between the oracle's and the GPU's trajectory cannot move the overflow
    assert longest[1] >= 1.1 * S.NL_CAP0, longest[1]
    assert len(s["dts"]) == (1 if name.endswith("_last") else 3)
    # the same ball as `contraction`
    ref = S.build("contraction")["gas"]
    assert all(np.array_equal(s["gas"][k], ref[k]) for k in "x y z u alpha m".split())


def _thresholds(n, first_cells):
    cap0 = (first_cells + 2) + (first_cells + 2) // 4                  # grid.hip: the first table, a quarter of headroom
    return cap0, 4 * n + 1_000_000, 64 * n + 4_000_000


def test_clumps_apart_outruns_the_guard_cell_and_passes_every_grid_threshold():
    s, states, pos, stats, caps, grid, record = case("clumps_apart")
    n, clump = pos[0].shape[0], s["clump"]
    # 27 clumps of 60 mutual neighbours (every member within 2 h of every other), and the eight stragglers
    ids, sizes = np.unique(clump, return_counts=True)
    assert ids.size == 28 and np.all(sizes[:27] == 60) and sizes[27] == S.N_STRAGGLERS
    for c in ids:
        p = pos[0][clump == c]
        d = p[:, None, :] - p[None, :, :]
        assert np.sqrt(np.max(np.sum(d * d, axis=2))) <= S.RCUT, c
    assert 40 <= stats[0]["per"][clump < 27].min() and stats[0]["per"].max() <= 80
    # the exact box grows by more than two cells per step on every axis: one guard cell per side cannot hold it
    for k in range(1, len(pos)):
        grow = np.ptp(pos[k], axis=0) - np.ptp(pos[k - 1], axis=0)
        assert np.all(grow > 2.0 * S.EDGE), (k, grow / S.EDGE)
        assert grid[k]["outside"].mean() >= 0.05, k                             # (it is two thirds and more)
    assert all(g["kind"] == 0 for g in grid)
    # the grid the code builds passes: the first table's capacity, 4 n + 1e6 (counting sort -> radix), 64 n + 4e6 (trim)
    cap0, radix, dense = _thresholds(n, int(grid[0]["cells"]))
    cells = [g["box_cells"] for g in grid]
    first = [next(k for k, c in enumerate(cells) if c + 2 > t) for t in (cap0, radix, dense)]
    print("clumps_apart cells", [f"{c:.3g}" for c in cells], "thresholds passed at builds", first,
          "outside", [round(float(g["outside"].mean()), 2) for g in grid])
    assert 1 <= first[0] < first[1] < first[2] < len(grid) - 1, first
    assert grid[first[1] - 1]["counting"] and not grid[first[1]]["counting"]
    # ... and from there on the trim cuts the stragglers off (and only them) while the lattice stays inside its 6 sigma
    for k in range(first[2], len(grid)):
        assert grid[k]["rounds"] >= 1 and grid[k]["shrunk"], k
        assert grid[k]["outside"][clump == 27].all(), k
    assert all(g["rounds"] == 0 for g in grid[:first[2]])
    # the lists stay put: nothing but the grid changes in this set
    assert not any(c["regrown"] or c["overflow"] for c in caps)


def test_clumps_together_starts_hashed_turns_dense_meets_and_passes_through():
    s, states, pos, stats, caps, grid, record = case("clumps_together")
    n, clump = pos[0].shape[0], s["clump"]
    ids, sizes = np.unique(clump, return_counts=True)
    assert 8 <= ids.size <= 27 and np.all((sizes >= 40) & (sizes <= 80))
    assert 40 <= stats[0]["per"].min()
    # the first build: even the trimmed box needs 2^31 cells -- hashed, sticky
    assert grid[0]["kind"] == 1 and grid[0]["rounds"] >= 1 and not grid[0]["shrunk"] and grid[0]["cells"] >= 2.0 ** 31
    kinds = [g["kind"] for g in grid]
    dense_from = kinds.index(0)
    print("clumps_together kinds", kinds, "cells", [f"{g['box_cells']:.3g}" for g in grid])
    assert dense_from >= 2 and all(k == 1 for k in kinds[:dense_from]) and all(k == 0 for k in kinds[dense_from:])
    # sticky: the hashed builds before it skip the dense attempt although a dense table could hold their box ...
    assert any(g["box_cells"] < S.DENSE_MAX for g in grid[1:dense_from])
    # ... until the stale box is no longer sparse
    assert grid[dense_from]["box_cells"] <= 64 * n + 4_000_000 < grid[dense_from - 1]["box_cells"]
    # the meeting: the lists grow by less than a third per step, are regrown from stale reports, and shrink again
    longest = [p["longest"] for p in stats]
    ratios = [b / a for a, b in zip(longest, longest[1:])]
    print("clumps_together longest", longest, [(c["cap"], c["regrown"]) for c in caps])
    assert max(ratios) < 1.3 and not any(c["overflow"] for c in caps)
    assert sum(c["regrown"] for c in caps) >= 2 and max(longest) > 200
    assert all(kinds[k] == 0 for k, c in enumerate(caps) if c["regrown"])         # the regrows happen on the dense grid
    assert longest[-1] < max(longest) / 4 and np.argmax(longest) < len(longest) - 1      # they pass through


def test_clumps_drift_leaves_the_stale_box_while_the_early_keys_are_in_use():
    s, states, pos, stats, caps, grid, record = case("clumps_drift")
    n = pos[0].shape[0]
    early = S.early_replay(grid)
    outside = [int(g["outside"].sum()) for g in grid]
    print("clumps_drift cells", [int(g["cells"]) for g in grid], "early keys", early, "outside", outside)
    assert all(g["kind"] == 0 and g["rounds"] == 0 and g["counting"] for g in grid)
    # every step the exact box grows by more than one guard cell per side (and by less than two)
    for k in range(1, len(pos)):
        lo0, hi0 = S.exact_box(pos[k - 1])
        lo1, hi1 = S.exact_box(pos[k])
        assert np.all(lo0 - lo1 > S.EDGE) and np.all(hi1 - hi0 > S.EDGE), k
        assert np.all(lo0 - lo1 < 2.0 * S.EDGE) and np.all(hi1 - hi0 < 2.0 * S.EDGE), k
        assert outside[k] >= 0.4 * n, (k, outside[k])
    # at least three builds take the early keys with particles outside their box, and at least two do not (table regrown)
    assert sum(early) >= 3 and sum(1 for k in range(1, len(grid)) if not early[k]) >= 2 and not early[0]
    assert all(outside[k] >= 0.4 * n for k in range(len(grid)) if early[k])
    assert not any(c["regrown"] or c["overflow"] for c in caps)


def test_sheet_puffing_up_loses_its_forces_tile_fit():
    s, states, pos, stats, caps, grid, record = case("sheet_puffing_up")
    n = pos[0].shape[0]
    assert n > 4000 and (n + 255) // 256 >= 8                                   # several groups of 256 targets
    boxes = [S.exact_box(pos[0])] + [S.stale_box(p) for p in pos[:-1]]
    fit = [S.tile_fit_replay(p, *b) for p, b in zip(pos, boxes)]
    pct = [f["fit_pct_forces"] for f in fit]
    thick = [float(p[:, 2].std()) for p in pos]
    print("sheet_puffing_up fit", pct, "half", [f["half"] for f in fit], "misfits", [f["misfits"] for f in fit],
          "z rms", [round(t, 2) for t in thick], "longest", [p["longest"] for p in stats])
    assert all(b > a for a, b in zip(thick, thick[1:])) and thick[0] < 0.5 and thick[-1] > 4.0
    # starts fitting (the whole-tile forces kernel runs), ends with more than one group in ten misfitting for at least two
    # builds in a row -- so a build after the flip is dealt by a report that already says so -- and flips once
    assert pct[0] >= 90 and fit[0]["ok"] and pct[-1] < 90 and pct[-2] < 90 and not fit[-1]["ok"]
    flips = sum(1 for a, b in zip(pct, pct[1:]) if (a >= 90) != (b >= 90))
    assert flips == 1, pct
    f_blocks = (n + 255) // 256
    assert min(fit[-1]["misfits"][1] * 10, fit[-1]["misfits"][3] * 5) > f_blocks
    # nothing else moves: one dense untrimmed grid, lists that only shrink (the first build regrows the 96 slots at once)
    assert all(g["kind"] == 0 and g["rounds"] == 0 for g in grid)
    assert stats[0]["longest"] > S.NL_CAP0 and not any(c["regrown"] or c["overflow"] for c in caps)
