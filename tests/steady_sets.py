"""Particle sets that CHANGE under a run, for the steady state of the plain fixed-h step (tests/test_steady_sets_cpu.py,
tests/test_steady_state_adversarial_gpu.py): the step believes the previous build's box, list report and tile fit, and
these sets make each of those beliefs wrong within one step.

Every set: seeded, h = 2.5, at most 4000 gas particles (tests/force_terms_ref.fixed_terms; but for the sheet), no sinks, live fields (alpha in
[0.05, 1], u in [0.5, 2], a random velocity on top of the bulk motion: the viscosity is on), masses of 1e-6 and bulk
speeds far above what the pressure adds within a step, so the motion is close to ballistic -- and a schedule: the list of
dt values handed to ctx.step one by one (the dt a step returns is compared, not used).

  contraction               a ball with v = -k x: the longest list grows by a sixth to a quarter per step, from within the initial 96
                            slots to several hundred
  contraction_too_fast_*    the same ball with a k that doubles the longest list within the first step
  clumps_apart              27 clumps of mutual neighbours on an expanding lattice, and eight fast stragglers: the box outruns
                            its guard cell every step, the cell count outgrows the table, the counting sort and the dense limit
  clumps_drift              the lattice expanding by a cell and a half per side and step inside the table in place: the builds
                            that take their keys from the kick + drift pass, with half the particles outside the box
  sheet_puffing_up          (8000 particles) a thin sheet whose vertical velocity dispersion thickens it until the forces
                            tiles no longer fit
  clumps_together           8 such clumps that start 6600 apart (2^31 cells: hashed and sticky), fly inward, meet and pass
and, for the 16-bit entries of the tiled list at their limits (tests/test_list16_edges_gpu.py; 33000 to 754000 particles with
thousands of neighbours each: the references are the cell-binned pair count, the threaded oracle and the restatement on sampled targets):
  dense_cube_32767 / _32768 a static cube of exactly 3 x 3 x 3 cells, one tile: the largest tile need is n
  dense_cube_window         36000 in 4 x 4 x 4 cells, contracting: the need grows into [32768, 65535] for exactly one build
  sheet_with_knot           such a knot inside a sheet of 700000 whose groups fit their tiles: the whole-tile kernels run
  rows_aligned_*            three blobs that move into the same cell rows in one step: the need passes 65536 while no list grows

What makes each set adversarial is asserted, from the CPU oracle's trajectory, in tests/test_steady_sets_cpu.py."""
from __future__ import annotations

import numpy as np

H = 2.5
RCUT = 2.0 * H
EDGE = 2.0 * H * (1.0 + 1e-6)          # csrc/grid.hip: the cell edge, and the guard of the stale box
MASS = 1.0e-6
NL_CAP0 = 96                           # csrc/api.hip: the list's initial slots
STATE = "x y z vx vy vz u m alpha".split()
NO_SINKS = {k: np.zeros(0) for k in "x y z vx vy vz m".split()}


def _ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    return v * (radius * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]


def _gas(rng, pos, bulk, sigma):
    n = pos.shape[0]
    v = bulk + rng.normal(0.0, sigma, (n, 3))
    out = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(),
           "vx": v[:, 0].copy(), "vy": v[:, 1].copy(), "vz": v[:, 2].copy(),
           "u": rng.uniform(0.5, 2.0, n), "m": np.full(n, MASS), "alpha": rng.uniform(0.05, 1.0, n)}
    return {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in out.items()}


# ---- the sets ------------------------------------------------------------------------------------------------------
CONTRACTION = dict(n=2000, radius=18.8, seed=11, sigma=0.05)


def _contraction(k, dts, run=None):
    c = CONTRACTION
    rng = np.random.default_rng(c["seed"])
    pos = _ball(rng, c["n"], c["radius"])
    return dict(gas=_gas(rng, pos, -k * pos, c["sigma"]), dts=list(dts), run=run, clump=None)


def contraction():
    """(1 - k dt)^-3 = 1.15 per step (the pressure of the heated gas adds to it later on); eleven steps.  Also run as ONE ctx.run(RUN_STEPS, RUN_DT0): the device chains its own dt"""
    k = 0.5
    dt = (1.0 - 1.15 ** (-1.0 / 3.0)) / k
    return _contraction(k, [dt] * 11, run=(RUN_STEPS, RUN_DT0))


RUN_STEPS, RUN_DT0 = 24, 0.01


def contraction_too_fast(where):
    """one step of (1 - k dt)^-3 = 2.6; where = "mid": two more (short) steps follow within the same call; "last": none"""
    k = 0.5
    dt = (1.0 - 2.6 ** (-1.0 / 3.0)) / k
    return _contraction(k, [dt] if where == "last" else [dt, 0.01, 0.01])


def _clumps(centres, velocities, per_clump, radius, seed, sigma, dts):
    rng = np.random.default_rng(seed)
    pos, bulk, ids = [], [], []
    for c, (ctr, vel) in enumerate(zip(centres, velocities)):
        pos.append(ctr + _ball(rng, per_clump, radius))
        bulk.append(np.broadcast_to(vel, (per_clump, 3)))
        ids.append(np.full(per_clump, c))
    return dict(gas=_gas(rng, np.concatenate(pos), np.concatenate(bulk), sigma), dts=list(dts), run=None,
                clump=np.concatenate(ids))


def clumps_apart():
    """27 clumps of 60 (radius 2.4: all mutual neighbours) on a 3 x 3 x 3 lattice of spacing 30 with its centre off the
    origin, each moving rigidly with v = K (centre - lattice centre): the lattice grows by 24 per step.  Eight stragglers
    (a knot of radius 1 beyond one corner) fly six times as fast: they stretch the exact box past the dense limit, and -- too
    few to hold the trim's mean +- 6 sigma open, which one clump in 27 would -- they are what the trim cuts off."""
    K, dt = 10.0, 0.08
    g = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
    origin = np.array([3.1, -1.7, 0.6])
    centres = origin + 30.0 * g + np.random.default_rng(20).uniform(-1.0, 1.0, g.shape)
    out = _clumps(centres, K * (centres - origin), 60, 2.4, 21, 0.2, [dt] * 9)
    far = origin + 48.0 * np.ones(3)
    knot = _clumps([far], [6.0 * K * (far - origin)], N_STRAGGLERS, 1.0, 22, 0.2, [])
    gas = {k: np.concatenate([out["gas"][k], knot["gas"][k]]) for k in STATE}
    return dict(gas=gas, dts=out["dts"], run=None, clump=np.concatenate([out["clump"], np.full(N_STRAGGLERS, 27)]))


N_STRAGGLERS = 8


def clumps_drift():
    """the same lattice at spacing 150 (61 cells per axis) growing by 7.5 per side and step, a cell and a half: the grid
    stays dense, untrimmed, within the counting sort's limit and -- two builds in three -- within the cell table in place,
    so the keys of those builds are the ones the kick + drift pass leaves behind (grid.hip kick_drift_keys), computed on a
    box that about half of the particles have left (the 26 outer clumps move 7.5 against a guard of 5)"""
    dt = 0.05
    g = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
    origin = np.array([3.1, -1.7, 0.6])
    centres = origin + 150.0 * g + np.random.default_rng(40).uniform(-1.0, 1.0, g.shape)
    return _clumps(centres, (7.5 / (150.0 * dt)) * (centres - origin), 60, 2.4, 41, 0.2, [dt] * 8)


def clumps_together():
    """8 clumps of 48 at the corners of a cube of edge 6600 (1321^3 cells, and the trim cannot shrink a box whose particles sit
    at its corners: hashed, sticky), each moving rigidly towards a point near the centre, aimed to miss it by a few units so
    that the clumps overlap in part; the schedule halves the cube until it is dense again and then takes short steps"""
    g = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    rng = np.random.default_rng(30)
    centres = 3300.0 * g + rng.uniform(-2.0, 2.0, g.shape)
    aim = rng.uniform(-2.5, 2.5, g.shape)
    vel = (aim - centres) / 1.0                               # reaches its aim point at t = 1
    return _clumps(centres, vel, 48, 2.4, 31, 0.2, TOGETHER_DTS)


def sheet_puffing_up():
    """the only set above 4000 particles: a thin sheet (58 x 29, sigma_z 0.3; 8000 particles: 32 forces groups of 256, 119 per
    cell column) with a vertical velocity dispersion of 10 that thickens it by 0.7 per step.  While z has the fewest cells
    it is the fastest axis of the cell key and the half-group forces tiles fit (the 256-target ones never do at this
    surface density); when the sheet is as many cells high as it is wide the axis order changes, a group's intervals span
    several columns and more than one group in ten no longer fits: the tile fit of the forces falls from >= 90 to a few
    per cent, and the build after that one learns it from the stale report.  Sized on the host replay of the tile need
    (tile_fit_replay), going down from 20000: at 8000 the seventh and the eighth build misfit (the schedule ends there; a still
    thicker sheet is sparse enough to fit again), at 5000 only one build does, so that no build would follow the flip."""
    n, lx, ly = 8000, 58.0, 29.0
    rng = np.random.default_rng(50)
    pos = np.stack([rng.uniform(-lx / 2, lx / 2, n), rng.uniform(-ly / 2, ly / 2, n), rng.normal(0.0, 0.3, n)], axis=1)
    bulk = np.stack([np.zeros(n), np.zeros(n), rng.normal(0.0, 10.0, n)], axis=1)
    return dict(gas=_gas(rng, pos, bulk, 0.2), dts=[0.07] * 8, run=None, clump=None)


# ---- the 16-bit list entries at their limits (tests/test_list16_edges_gpu.py) -----------------------------------------------------
# A tiled list entry is the neighbour's slot among the records of its group's three candidate intervals: the group's tile
# NEED (tile_fit_replay(...)["need"]).  The context leaves the tiled path when a need reaches HALF of 65536, on a report that
# is one build old in the steady state; so entries with bit 15 set exist only in the one build whose need has grown into
# [32768, 65535], and a need that reaches 65536 within one step is an error.  These sets hold tens of thousands of particles with
# thousands of neighbours each -- a cube of 3 x 3 x 3 cells is ONE tile: max need = n.
LIST16_HALF, LIST16_FULL = 32768, 65536


def _cube(rng, n, side):
    return rng.uniform(-0.5 * side, 0.5 * side, (n, 3))


DENSE_CUBE = dict(side=2.9 * EDGE, seed=60, sigma=0.05)


def dense_cube(n):
    """static (no schedule): n uniform points in a cube of 2.9 cell edges -- exactly 3 cells per axis, a tenth of an edge
    of slack to the fourth -- so that the group which holds a particle of the central cell needs all n records: max need =
    n, an integer count that no rounding moves.  n = 32767 is the last value a first build keeps tiled, 32768 the first
    it leaves with."""
    c = DENSE_CUBE
    rng = np.random.default_rng(c["seed"])
    pos = _cube(rng, n, c["side"])
    return dict(gas=_gas(rng, pos, np.zeros((n, 3)), c["sigma"]), dts=[], run=None, clump=None)


WINDOW = dict(n=36000, side=3.30 * EDGE, seed=61, sigma=0.05, k=0.5, shrink=0.95, steps=4)


def _window_cube():
    c = WINDOW
    rng = np.random.default_rng(c["seed"])
    pos = _cube(rng, c["n"], c["side"])
    return rng, pos, -c["k"] * pos


def dense_cube_window():
    """36000 points in a cube of 4 x 4 x 4 cells with the homologous inflow v = -k x of `contraction`, every step (dt = 0.1)
    shrinking it to 0.95 of its size (the lists grow by 1 / 0.95^3 = 1.17 per step, 1.16 to 1.19 on the oracle's
    trajectory): the largest tile need starts below 32768, is
    still below it at build 1, lies inside [32768, 65535] at build 2 -- the only build that writes entries with bit 15 set,
    and the step that decodes them -- and build 3 learns it from the stale report and leaves the tiled path."""
    c = WINDOW
    rng, pos, bulk = _window_cube()
    dt = (1.0 - c["shrink"]) / c["k"]
    return dict(gas=_gas(rng, pos, bulk, c["sigma"]), dts=[dt] * c["steps"], run=None, clump=None)


KNOT = dict(sheet=700000, side=530.0, sigma_z=0.3, knot=54000, xy=3.37 * EDGE, z=8.55 * EDGE, seed=63, sigma=0.05, k=0.5, shrink=0.95,
            steps=3)


def sheet_with_knot():
    """the only way to bring entries at or above 32768 into the whole-tile kernels: a thin sheet (700000 particles on 530 x
    530, 62 per cell column: the tiles of its groups fit, so density_wt and forces_q run) with a dense knot at its centre
    -- 54000 particles in a box of 3.4 x 3.4 x 8.55 cell edges, tall so that its lists stay at a few thousand, contracting
    like dense_cube_window.  z keeps the fewest cells and is the fastest axis of the cell key, so a group of the knot needs
    the columns around its own over the knot's whole height: its need grows through 32768 as the knot shrinks from four
    columns a side towards three.  The knot's groups misfit and take the fall-back loops of the two kernels; they are fewer
    than one group in ten of either geometry (the 1024-target density groups, the 256-target forces groups)."""
    c = KNOT
    rng = np.random.default_rng(c["seed"])
    ns, nk = c["sheet"], c["knot"]
    sheet = np.stack([rng.uniform(-0.5 * c["side"], 0.5 * c["side"], ns), rng.uniform(-0.5 * c["side"], 0.5 * c["side"], ns),
                      rng.normal(0.0, c["sigma_z"], ns)], axis=1)
    knot = rng.uniform(-0.5, 0.5, (nk, 3)) * np.array([c["xy"], c["xy"], c["z"]])
    pos = np.concatenate([sheet, knot])
    bulk = np.concatenate([np.zeros((ns, 3)), -c["k"] * knot])
    dt = (1.0 - c["shrink"]) / c["k"]
    return dict(gas=_gas(rng, pos, bulk, c["sigma"]), dts=[dt] * c["steps"], run=None,
                clump=np.concatenate([np.zeros(ns, dtype=np.int64), np.ones(nk, dtype=np.int64)]))


ROWS = dict(per=28000, blobs=3, side=2.8 * EDGE, seed=62, sigma=0.05, dt=0.1)
N_MARKERS = 2


def rows_aligned(where):
    """three dense blobs (cubes of 2.8 edges: 3 x 3 x 3 cells each, need = 28000 + the odd marker) side by side along x -- 1.2
    edges of empty space between them, more than 2 h, before and after -- that start four cell rows apart in y and move rigidly,
    in ONE step, into the same rows.  Two markers pin the box's corners and stretch y and z to more cells than x, so that x
    stays the fastest axis of the cell key: a row of cells then runs through all three blobs, and a group's middle
    intervals -- from its first candidate row to its last -- span them all.  No list grows (no pair of different blobs
    comes within 2 h), but the largest need goes from below 32768 to above 65536 within one build.
    What the kernels of that step do with the truncated entries: an entry is e mod 65536 < 65536 <= need, and EntryMap adds
    the offset of the interval that e mod 65536 falls into, so every decoded index is a record of the group's own three intervals --
    a WRONG neighbour, never an address outside the arrays.  The sums of that step are wrong and must be refused.
    where = "mid": two more (short) steps follow within the same call; "last": none."""
    c = ROWS
    rng = np.random.default_rng(c["seed"])
    e = EDGE
    pos, bulk, ids = [], [], []
    for b in range(c["blobs"]):
        corner = np.array([(0.1 + 4.0 * b) * e, (0.1 + 4.0 * b) * e, 0.1 * e])
        pos.append(corner + rng.uniform(0.0, c["side"], (c["per"], 3)))
        bulk.append(np.broadcast_to(np.array([0.0, -4.0 * b * e / c["dt"], 0.0]), (c["per"], 3)))
        ids.append(np.full(c["per"], b))
    nx = 4.0 * (c["blobs"] - 1) + 3.0                          # cells along x
    pos.append(np.array([[0.0, 0.0, 0.0], [(nx - 0.05) * e, (nx + 1.5) * e, (nx + 2.5) * e]]))     # nx, nx + 2, nx + 3 cells
    bulk.append(np.zeros((N_MARKERS, 3)))
    ids.append(np.array([c["blobs"], c["blobs"] + 1]))
    pos, bulk = np.concatenate(pos), np.concatenate(bulk)
    gas = _gas(rng, pos, bulk, c["sigma"])
    for f, a in zip(("vx", "vy", "vz"), bulk[-N_MARKERS:].T):            # the markers stay where they are
        gas[f][-N_MARKERS:] = a
    return dict(gas=gas, dts=[c["dt"]] if where == "last" else [c["dt"], 0.01, 0.01], run=None, clump=np.concatenate(ids))


# t = 1 - 2^-k for the approach (the cube halves per step); then the meeting, each dt found by bisection on the oracle so
# that the longest list grows by a little over a fifth (and written here with three digits); then three steps apart again.
# The clumps close at 1e4 length units per time unit -- they have to cross 3300 within the time a clump of this size takes
# to disperse -- so the meeting is a strong shock: the viscosity heats u from about 1 to about 1e8 there.
TOGETHER_DTS = ([0.5 ** (k + 1) for k in range(9)]
                + [3.14e-4, 1.28e-4, 1.94e-4, 1.05e-4, 1.38e-4, 1.72e-4, 1.24e-4, 9.95e-5, 1.63e-4, 6.0e-4]
                + [6.0e-4] * 2)

BUILDERS = {"contraction": contraction,
            "contraction_too_fast_mid": lambda: contraction_too_fast("mid"),
            "contraction_too_fast_last": lambda: contraction_too_fast("last"),
            "clumps_apart": clumps_apart,
            "clumps_drift": clumps_drift,
            "clumps_together": clumps_together,
            "sheet_puffing_up": sheet_puffing_up,
            "dense_cube_32767": lambda: dense_cube(32767),
            "dense_cube_32768": lambda: dense_cube(32768),
            "dense_cube_window": dense_cube_window,
            "sheet_with_knot": sheet_with_knot,
            "rows_aligned_mid": lambda: rows_aligned("mid"),
            "rows_aligned_last": lambda: rows_aligned("last")}
DENSE_STATIC = ["dense_cube_32767", "dense_cube_32768"]
ROWS_ALIGNED = ["rows_aligned_mid", "rows_aligned_last"]
SMALL = ["contraction", "clumps_apart", "clumps_drift", "clumps_together"]
TOO_FAST = ["contraction_too_fast_mid", "contraction_too_fast_last"]
_BUILT = {}


def build(name):
    """dict: gas (the nine state arrays), dts (the schedule), run ((k, dt0) or None), clump (clump number per particle or None)"""
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]


# ---- what the tests measure on a state ---------------------------------------------------------------------------------
def positions(state):
    return np.stack([state["x"], state["y"], state["z"]], axis=1)


def pair_stats(pos, tie=1e-12, chunk=512):
    """brute force over all ordered pairs (i, j), i != j, with r^2 formed as the kernels do (dx dx + dy dy + dz dz):
    longest = the longest list, entries = pairs with r <= 2 h, entries_lo / entries_hi = the same without / with the pairs
    whose r^2 lies within `tie` (relative) of (2 h)^2, near = pairs within 1e-9 of it"""
    n = pos.shape[0]
    r2cut = RCUT * RCUT
    x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    per = np.zeros(n, dtype=np.int64)
    lo = hi = near = 0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        d = x[a:b, None] - x[None, :]
        r2 = d * d
        d = y[a:b, None] - y[None, :]
        r2 += d * d
        d = z[a:b, None] - z[None, :]
        r2 += d * d
        r2[np.arange(b - a), np.arange(a, b)] = np.inf
        inside = r2 <= r2cut
        per[a:b] = np.count_nonzero(inside, axis=1)
        band = r2[np.abs(r2 - r2cut) <= r2cut * 2.0e-9]                     # the few pairs near the edge, if any
        near += int(band.size)
        tied = np.abs(band - r2cut) <= r2cut * 2.0 * tie
        lo -= int(np.count_nonzero(tied & (band <= r2cut)))
        hi += int(np.count_nonzero(tied & (band > r2cut)))
    entries = int(per.sum())
    return dict(longest=int(per.max()) if n else 0, entries=entries, entries_lo=entries + lo, entries_hi=entries + hi,
                near=near, per=per)


def host_threads():
    """the threads a numpy reference may use: what the process is granted, at most 16"""
    import os
    return max(1, min(16, len(os.sched_getaffinity(0))))


def pair_stats_binned(pos, tie=1e-12):
    """pair_stats for the sets too large for it (O(n^2) at 36000 and more): the same counts -- r^2 formed by the very same
    expression on the very same numbers, so bit for bit the same comparisons -- over the candidates of a cell grid only.
    Cells of the list's edge (a hair more than 2 h, which also covers the `near` band): a pair is at most one cell apart per
    axis; the cells of one row are consecutive in the cell-sorted order, so a cell's candidates are 9 ranges of it (found by
    bisection on the sorted keys: no table of cells, the box may hold 2^31 of them and more).  One task per occupied cell,
    on host_threads() threads (numpy releases the interpreter lock in its loops).  Equal to pair_stats on the small sets:
    tests/test_steady_sets_cpu.py."""
    from concurrent.futures import ThreadPoolExecutor
    n = pos.shape[0]
    r2cut = RCUT * RCUT
    lo = pos.min(axis=0)
    cell = np.floor((pos - lo) * (1.0 / EDGE)).astype(np.int64)
    dim = cell.max(axis=0) + 1
    key = (cell[:, 2] * dim[1] + cell[:, 1]) * dim[0] + cell[:, 0]
    order = np.argsort(key, kind="stable")
    x, y, z = (np.ascontiguousarray(pos[order, a]) for a in range(3))
    skey = key[order]
    occupied, first = np.unique(skey, return_index=True)
    last = np.r_[first[1:], n]

    def one(t):
        k, a, b = int(occupied[t]), int(first[t]), int(last[t])
        c0, c1, c2 = k % dim[0], (k // dim[0]) % dim[1], k // (dim[0] * dim[1])
        cand = []
        for o2 in range(max(c2 - 1, 0), min(c2 + 1, dim[2] - 1) + 1):
            for o1 in range(max(c1 - 1, 0), min(c1 + 1, dim[1] - 1) + 1):
                row = (o2 * dim[1] + o1) * dim[0]
                ja = int(np.searchsorted(skey, row + max(c0 - 1, 0), side="left"))
                jb = int(np.searchsorted(skey, row + min(c0 + 1, dim[0] - 1), side="right"))
                if jb > ja:
                    cand.append(np.arange(ja, jb))
        cand = np.concatenate(cand)
        cnt, nr, tl, th = np.zeros(b - a, dtype=np.int64), 0, 0, 0
        step = max(1, 4_000_000 // cand.size)
        for a0 in range(a, b, step):                     # (blocks of targets: a dense cell has hundreds, with 20000 candidates)
            b0 = min(b, a0 + step)
            d = x[a0:b0, None] - x[None, cand]
            r2 = d * d
            d = y[a0:b0, None] - y[None, cand]
            r2 += d * d
            d = z[a0:b0, None] - z[None, cand]
            r2 += d * d
            r2[cand[None, :] == np.arange(a0, b0)[:, None]] = np.inf
            band = r2[np.abs(r2 - r2cut) <= r2cut * 2.0e-9]
            tied = np.abs(band - r2cut) <= r2cut * 2.0 * tie
            cnt[a0 - a:b0 - a] = np.count_nonzero(r2 <= r2cut, axis=1)
            nr, tl, th = nr + int(band.size), tl + int(np.count_nonzero(tied & (band <= r2cut))), th + int(np.count_nonzero(tied & (band > r2cut)))
        return a, b, cnt, nr, tl, th
    per_sorted = np.zeros(n, dtype=np.int64)
    lo_ = hi_ = near = 0
    with ThreadPoolExecutor(max_workers=host_threads()) as pool:
        for a, b, cnt, nr, tl, th in pool.map(one, range(occupied.size)):
            per_sorted[a:b] = cnt
            near, lo_, hi_ = near + nr, lo_ - tl, hi_ + th
    per = np.empty(n, dtype=np.int64)
    per[order] = per_sorted
    entries = int(per.sum())
    return dict(longest=int(per.max()) if n else 0, entries=entries, entries_lo=entries + lo_, entries_hi=entries + hi_,
                near=near, per=per)


def build_boxes(pos_list):
    """the box of each build of one upload: the exact box at build 0, then the previous build's, one guard cell wider"""
    return [exact_box(pos_list[0])] + [stale_box(p) for p in pos_list[:-1]]


def need_replay(pos_list):
    """tile_fit_replay of every build: the per-group needs, and their largest"""
    fits = [tile_fit_replay(p, *b) for p, b in zip(pos_list, build_boxes(pos_list))]
    return fits, [int(f["need"].max()) for f in fits]


def list16_replay(needs):
    """csrc/tiled.hip nlist_build_tiled, csrc/api.hip drain_reports over the builds of one upload: needs[k] = the largest tile
    need of build k.  Per build: "tiled" (the build wrote 16-bit entries), "leaves" (it left the tiled path: at build 0 on
    its own report, later on the previous build's), "error" (the previous build's need had reached 65536: refused).  A last
    build whose own need reaches 65536 is "drained": the call that returns reports it."""
    out, tiled = [], True
    for k, need in enumerate(needs):
        if not tiled:
            out.append("untiled")
            continue
        seen = need if k == 0 else needs[k - 1]
        if k > 0 and seen >= LIST16_FULL:
            out.append("error")
            break
        if 2 * seen >= LIST16_FULL:
            tiled = False
            out.append("leaves")
            continue
        out.append("tiled")
    if out and out[-1] == "tiled" and needs[len(out) - 1] >= LIST16_FULL and len(out) == len(needs):
        out[-1] = "drained"
    return out


def exact_box(pos):
    return pos.min(axis=0), pos.max(axis=0)


def cells_of(lo, hi):
    """csrc/grid.hip: cells per axis of a box, and their product (as a float: it passes 2^31)"""
    dim = np.floor((np.asarray(hi) - np.asarray(lo)) * (1.0 / EDGE)) + 1.0
    return dim, float(np.prod(dim))


def stale_box(prev_pos):
    """the box grid_rebuild gives a steady-state build: the previous build's exact box, one guard cell wider per side"""
    lo, hi = exact_box(prev_pos)
    return lo - EDGE, hi + EDGE


def trimmed_box(pos, lo, hi, n):
    """grid_rebuild's trim of a box that needs more than 64 n + 4e6 cells (tests/varh_sets.grid_box_replay, from a given box)"""
    limit = 64.0 * n + 4.0e6
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    rounds = 0
    for _ in range(8):
        if not cells_of(lo, hi)[1] > limit:
            break
        inside = np.all((pos >= lo) & (pos <= hi), axis=1)
        cnt = float(inside.sum())
        if not cnt >= 1.0:
            break
        mean = pos[inside].sum(axis=0) / cnt
        sig = np.sqrt(np.maximum((pos[inside] ** 2).sum(axis=0) / cnt - mean * mean, 0.0))
        half = 6.0 * sig + 2.0 * EDGE
        nlo, nhi = np.maximum(lo, mean - half), np.minimum(hi, mean + half)
        shrunk = bool(np.any(nlo > lo) or np.any(nhi < hi))
        lo, hi = nlo, nhi
        rounds += 1
        if not shrunk:
            break
    return lo, hi, rounds


def capacity_replay(longest, cap0=NL_CAP0):
    """csrc/tiled.hip nlist_build_tiled over the builds of one upload: longest[k] = the longest list of build k.  Build 0
    waits for its own report and regrows until 4 mx <= 3 cap; build k >= 1 sees the report of build k - 1 only.
    Returns per build: cap (the capacity the build wrote into), regrown (from the stale report), overflow (its own longest
    list exceeds cap: an error at the next build or at the end of the call)."""
    def want(mx):
        return (mx + mx // 2 + 8 + 7) & ~7
    out, cap = [], cap0
    for k, mx in enumerate(longest):
        regrown = False
        if k == 0:
            while 4 * mx > 3 * cap:
                cap = want(mx)
        elif 4 * longest[k - 1] > 3 * cap:
            cap, regrown = want(longest[k - 1]), True
        out.append(dict(cap=cap, regrown=regrown, overflow=mx > cap))
    return out


# ---- the oracle along a schedule -----------------------------------------------------------------------------------------
ORACLE_CELLS = 2.0e7            # the oracle's own grid is dense over the exact box: beyond this the set is stepped in pieces


def _pieces(clump, views, reach):
    """groups of clumps whose boxes, widened by `reach`, overlap in one of the position sets `views` (union-find over at
    most 27 clumps)"""
    ids = np.unique(clump)
    root = list(range(ids.size))

    def find(a):
        while root[a] != a:
            a = root[a]
        return a
    for pos in views:
        lo = np.array([pos[clump == c].min(axis=0) - reach for c in ids])
        hi = np.array([pos[clump == c].max(axis=0) + reach for c in ids])
        for a in range(ids.size):
            for b in range(a + 1, ids.size):
                if np.all(lo[a] <= hi[b]) and np.all(lo[b] <= hi[a]):
                    root[find(a)] = find(b)
    groups = {}
    for a, c in enumerate(ids):
        groups.setdefault(find(a), []).append(c)
    return [np.flatnonzero(np.isin(clump, g)) for g in groups.values()]


def oracle_step(state, dt, clump=None, nthreads=None):
    """one oracle.orc.Oracle.step from `state` (dict of the nine arrays): the new state with the derived fields of the
    step's second evaluation, and the next dt.  A set whose exact box is too sparse for the oracle's dense grid is stepped
    piece by piece -- groups of clumps further apart than 2 h at both of the step's evaluations do not meet, so each piece's sums are the whole set's (tests/test_hashed_grid_gpu.check_halves does the same)."""
    from oracle import orc
    nthreads = nthreads or orc.max_threads()
    pos = positions(state)
    if clump is None or cells_of(*exact_box(pos))[1] <= ORACLE_CELLS:
        pieces = [np.arange(pos.shape[0])]
    else:
        # the positions of the two evaluations: now and after the drift (predicted without the opening kick; checked below)
        after = pos + dt * np.stack([state["vx"], state["vy"], state["vz"]], axis=1)
        pieces = _pieces(clump, (pos, after), 0.5 * RCUT + 1.0)
    out = {k: np.empty(pos.shape[0]) for k in STATE + orc.Oracle.DERIVED}
    cand = np.inf
    for idx in pieces:
        o = orc.Oracle({k: state[k][idx] for k in STATE}, NO_SINKS, h=H, nthreads=nthreads)
        o.step(dt)
        cand = min(cand, o.dt_candidate())
        for k in out:
            out[k][idx] = getattr(o, k)
    if len(pieces) > 1:
        new = positions(out)
        lo, hi = [new[i].min(axis=0) for i in pieces], [new[i].max(axis=0) for i in pieces]
        for a in range(len(pieces)):
            for b in range(a + 1, len(pieces)):
                gap = np.maximum(np.maximum(lo[a] - hi[b], lo[b] - hi[a]), 0.0)
                assert float(np.sqrt(np.sum(gap * gap))) > RCUT, "pieces met within the step"
    return out, float(orc.lib().orc_dt_update(cand, dt))


_TRAJ = {}


def trajectory(name):
    """the oracle along the set's schedule: states[k] = the state after k steps (states[0]: the set, no derived fields),
    next_dt[k] = the dt decision after step k + 1"""
    if name not in _TRAJ:
        s = build(name)
        states, decisions = [dict(s["gas"])], []
        for dt in s["dts"]:
            new, nxt = oracle_step(states[-1], dt, s["clump"])
            states.append(new)
            decisions.append(nxt)
        _TRAJ[name] = (states, decisions)
    return _TRAJ[name]


_RUN = {}


def run_trajectory(name):
    """the oracle along the `run` variant (the dt of each step is the previous step's decision): states, the dt sequence
    (dts[k] = the dt of step k + 1, dts[-1] = the decision after the last step) and t as sph_run accumulates it"""
    if name not in _RUN:
        s = build(name)
        k, dt = s["run"]
        states, dts, t = [dict(s["gas"])], [dt], 0.0
        for _ in range(k):
            new, nxt = oracle_step(states[-1], dts[-1], s["clump"])
            t = t + dts[-1]
            states.append(new)
            dts.append(nxt)
        _RUN[name] = (states, dts, t)
    return _RUN[name]


# ---- what the code will decide, replayed from positions ------------------------------------------------------------------
DENSE_MAX = 2147483647.0


def grid_replay(pos_list):
    """csrc/grid.hip grid_rebuild over the builds of one upload: pos_list[k] = the positions of build k (build 0: the
    uploaded set, exact box; build k >= 1: the exact box of build k - 1, one guard cell wider).  Per build: box_cells (of
    the box before any trim), cells and dim (of the grid built), kind (0 dense, 1 hashed), rounds (trim rounds, one host
    wait each), shrunk (the trim cut something off), outside (mask: particles outside the grid's box, clamped into
    boundary cells), counting (counting sort; else radix)"""
    n = pos_list[0].shape[0]
    limit = 64.0 * n + 4.0e6
    sticky, out = False, []
    for k, pos in enumerate(pos_list):
        lo, hi = exact_box(pos) if k == 0 else stale_box(pos_list[k - 1])
        box_cells = cells_of(lo, hi)[1]
        hashed, rounds, tlo, thi = False, 0, lo, hi
        if sticky:
            hashed = sticky = box_cells > limit
        if not hashed:
            tlo, thi, rounds = trimmed_box(pos, lo, hi, n)
            if cells_of(tlo, thi)[1] >= DENSE_MAX:
                hashed = sticky = True
                tlo, thi = lo, hi
        dim, cells = cells_of(tlo, thi)
        out.append(dict(box_cells=box_cells, cells=cells, dim=dim, kind=int(hashed), rounds=rounds,
                        shrunk=bool(np.any(tlo > lo) or np.any(thi < hi)), stale=k > 0,
                        outside=~np.all((pos >= tlo) & (pos <= thi), axis=1), counting=cells <= 4.0 * n + 1.0e6))
    return out


# ---- references of one evaluation on a given (downloaded) state ------------------------------------------------------------
DERIVED = "rho P c ax ay az du dalpha".split()
RATES = ("ax", "ay", "az", "du", "dalpha")


def static_pieces(state, clump):
    """the whole set, or -- where its exact box is too sparse for the oracle's dense grid -- groups of clumps further than
    2 h apart"""
    pos = positions(state)
    if clump is None or cells_of(*exact_box(pos))[1] <= ORACLE_CELLS:
        return [np.arange(pos.shape[0])]
    return _pieces(clump, (pos,), 0.5 * RCUT + 1.0)


def oracle_eval(state, clump=None):
    """the threaded C oracle's evaluation of `state`: dict of the derived fields"""
    from oracle import orc
    out = {k: np.empty(state["x"].size) for k in DERIVED}
    for idx in static_pieces(state, clump):
        o = orc.Oracle({k: state[k][idx] for k in STATE}, NO_SINKS, h=H, nthreads=orc.max_threads())
        o.evaluate()
        for k in DERIVED:
            out[k][idx] = getattr(o, k)
    return out


def terms_ref(state, clump=None, targets=None):
    """tests/force_terms_ref.fixed_terms(...).recomposed() on `state`: the five rates and the summed magnitudes of their
    terms (the scale of the project's per-element bar), each of shape (5, n).  targets: an index array -- only these
    particles' elements mean anything (the whole set in one piece: O(len(targets) n))"""
    import force_terms_ref as FT
    n = state["x"].size
    if targets is not None:
        got, sc = FT.fixed_terms({k: state[k] for k in STATE}, NO_SINKS, h=H, targets=targets).recomposed()
        return np.array(got), np.array(sc)
    rates, scales = np.empty((5, n)), np.empty((5, n))
    for idx in static_pieces(state, clump):
        got, sc = FT.fixed_terms({k: state[k][idx] for k in STATE}, NO_SINKS, h=H).recomposed()
        for k in range(5):
            rates[k][idx], scales[k][idx] = got[k], sc[k]
    return rates, scales


def rho_ref(state, targets):
    """the density sum of `targets` restated in extended precision: rho_i = sum over r_ij <= 2 h, self included, of
    m_j W(r_ij) with the oracle's table lookup (oracle.orc.lookup_kernel) and r as the oracle forms it.  Returns (rho as
    long double, the number of terms per target)"""
    from oracle import orc
    pos, m = positions(state), state["m"]
    rho, terms = np.empty(len(targets), dtype=np.longdouble), np.empty(len(targets), dtype=np.int64)
    for a, i in enumerate(targets):
        d = pos[i] - pos
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        j = np.flatnonzero(r <= RCUT)
        W, _ = orc.lookup_kernel(r[j], H)
        rho[a], terms[a] = np.sum((m[j] * W).astype(np.longdouble)), j.size
    return rho, terms


def rho_bar(rho, list_len):
    """the per-element bar of a density sum of list_len + 1 positive terms: (k + 8) 2^-53 rho.  A sum of k + 1 positive fp64
    terms in ANY order is within k 2^-53 of its exact value (each of the k additions rounds a partial sum <= rho by half an
    ulp); the 8 covers the roundings inside a term (the separation, the table's interpolation, the mass), which the two sides
    form alike"""
    return (list_len + 8.0) * 2.0 ** -53 * rho


def near_cell_faces(pos, lo, tol=1e-9):
    """how many coordinates lie within tol cell edges of an inner face of the grid that starts at lo: the particles that the
    ~1e-12 between the oracle's and the GPU's trajectory could put into another cell.  None of them: the two trajectories
    sort every particle into the same cell, and every replayed need is the same integer on both."""
    t = (pos - np.asarray(lo)) * (1.0 / EDGE)
    return int(np.count_nonzero((np.abs(t - np.round(t)) < tol) & (np.round(t) >= 1.0)))


def edge_targets(pos, lo, hi, fit, count=512, seed=0, least=LIST16_HALF, among=None):
    """the targets of the sampled restatement on a build over the box (lo, hi) (fit = tile_fit_replay(pos, lo, hi)): the
    particles in the first and the last 64 slots of the tile of every group whose need is >= `least` (32768; the cell-sorted
    neighbours of the lowest and the highest entries), every fourth target of those groups, and a seeded sample of the rest
    (of the particles `among`, an index array, where given) up to `count` (at least 128 of them)"""
    order = fit["order"]
    pick = []
    for g in np.flatnonzero(fit["need"] >= least):
        pick.append(order[256 * g:256 * (g + 1):4])
        first = next(q for q in range(3) if fit["len"][q][g] > 0)
        last = next(q for q in (2, 1, 0) if fit["len"][q][g] > 0)
        pick.append(order[fit["lo"][first][g]:fit["lo"][first][g] + 64])
        end = fit["lo"][last][g] + fit["len"][last][g]
        pick.append(order[max(end - 64, 0):end])
    pick = np.unique(np.concatenate(pick)) if pick else np.zeros(0, dtype=np.int64)
    rest = np.setdiff1d(np.arange(pos.shape[0]) if among is None else among, pick)
    extra = np.random.default_rng(seed).choice(rest, size=min(rest.size, max(count - pick.size, 128)), replace=False)
    return np.sort(np.concatenate([pick, extra]))


def early_replay(grid, tables=None):
    """csrc/grid.hip grid_prepare_early over the builds of grid_replay: per build, whether its keys, histogram and box
    partials are the ones the step's kick + drift pass left behind -- a stale box, dense, untrimmed, counting sort, and
    within the cell table in place.  tables[k]: the table's capacity after build k (from grid_info().bytes); without it
    the capacity is replayed too (build 0 allocates it; a build that needs more than it regrows it by a quarter)."""
    out, cap, sticky = [], 0, False
    for k, g in enumerate(grid):
        need = int(g["cells"]) + 2
        fits = g["kind"] == 0 and need <= cap
        out.append(bool(g["stale"] and fits and not sticky and g["rounds"] == 0 and g["counting"]
                        and g["box_cells"] <= 64.0 * g["outside"].size + 4.0e6))
        sticky = g["kind"] == 1
        if tables is not None:
            cap = tables[k]
        elif g["kind"] == 0 and need > cap:
            cap = need + need // 4
    return out


# ---- the tile fit of the forces kernel, replayed ---------------------------------------------------------------------------
TILE_CAP_D = (3836, 5087)         # csrc/tiled.hip tile_cap(5000, 4, .): records of a density tile beside the kernel table / without it
TILE_CAP_Q = (1220, 1628)         # csrc/tiled.hip tile_cap_q(5000): records of a forces tile beside the kernel table / without it


def tile_fit_replay(pos, lo, hi):
    """csrc/tiled.hip: what a list build on the dense grid over the box (lo, hi) reports about the forces geometry, and what
    nlist_build_tiled's digest makes of it.  The cell-sorted particles are cut into groups of 256 (and half groups of 128);
    a group's tile need is the summed length of its three candidate intervals of the sorted order (one per offset along the
    slowest axis: from the first candidate row of any of its targets to the last).  Returns need (per group), misfits
    (groups of 256 beside the table, without it, half groups beside the table, without it), fit_pct_forces, half (the half-group
    kernel is chosen) and ok (the whole-tile forces kernel runs).  Also: order (the cell-sorted order: order[s] = the
    particle in sorted slot s; group g holds slots 256 g .. 256 g + 255), lo and len (per interval 0, 1, 2 an array over the
    groups of 256: the interval's first sorted slot and its length; a group's tile is the three intervals one after the
    other, so entry e of a group points into them), and the density geometry: need_d (per group of 1024 targets),
    misfits_d (groups beside the table, without it), fit_pct (what stats().tile_fit_pct reports) and ok_d (density_wt runs)."""
    n = pos.shape[0]
    dim = cells_of(lo, hi)[0].astype(np.int64)
    c = np.clip(np.floor((pos - np.asarray(lo)) * (1.0 / EDGE)).astype(np.int64), 0, dim - 1)
    s = [0, 1, 2]
    for i in range(3):                                   # grid.hip: fewest cells fastest, the longest of the other two in the middle
        for j in range(i + 1, 3):
            if dim[s[j]] < dim[s[i]]:
                s[i], s[j] = s[j], s[i]
    s[1], s[2] = s[2], s[1]
    d0, d1, d2 = (int(dim[a]) for a in s)
    c0, c1, c2 = (c[:, a] for a in s)
    key = (c2 * d1 + c1) * d0 + c0
    order = np.argsort(key, kind="stable")
    c0, c1, c2 = c0[order], c1[order], c2[order]
    start = np.zeros(d0 * d1 * d2 + 1, dtype=np.int64)
    np.add.at(start, key + 1, 1)
    start = np.cumsum(start)
    lo0, hi0 = np.maximum(c0 - 1, 0), np.minimum(c0 + 1, d0 - 1)
    big = np.iinfo(np.int64).max
    need = {256: 0, 128: 0}
    ivl_lo, ivl_len = [], []                             # per interval (offset -1, 0, 1 along the slowest axis) and group of 256
    for o2 in (-1, 0, 1):
        mn, mx = np.full(n, big), np.zeros(n, dtype=np.int64)
        for o1 in (-1, 0, 1):
            a2, a1 = c2 + o2, c1 + o1
            ok = (a2 >= 0) & (a2 < d2) & (a1 >= 0) & (a1 < d1)
            row = (np.where(ok, a2, 0) * d1 + np.where(ok, a1, 0)) * d0
            jb, je = start[row + lo0], start[row + hi0 + 1]
            ok &= je > jb
            mn = np.where(ok, np.minimum(mn, jb), mn)
            mx = np.where(ok, np.maximum(mx, je), mx)
        for g in (256, 128):
            edges = np.arange(0, n, g)
            glo, ghi = np.minimum.reduceat(mn, edges), np.maximum.reduceat(mx, edges)
            need[g] = need[g] + np.where(ghi > glo, ghi - glo, 0)
            if g == 256:
                ivl_lo.append(np.where(ghi > glo, glo, 0)); ivl_len.append(np.where(ghi > glo, ghi - glo, 0))
    f_blocks = (n + 255) // 256
    half = need[128]
    if half.size < 2 * f_blocks:
        half = np.concatenate([half, np.zeros(2 * f_blocks - half.size, dtype=np.int64)])
    mis = [int(np.count_nonzero(need[256] > TILE_CAP_Q[0])), int(np.count_nonzero(need[256] > TILE_CAP_Q[1])),
           int(np.count_nonzero(half > TILE_CAP_Q[0])), int(np.count_nonzero(half > TILE_CAP_Q[1]))]
    ok_f, ok_fb, ok_h, ok_hb = mis[0] * 10 <= f_blocks, mis[1] * 10 <= f_blocks, mis[2] * 10 <= 2 * f_blocks, mis[3] * 10 <= 2 * f_blocks
    use_half = not ok_f and not ok_fb and (ok_h or ok_hb)
    if use_half:
        bigt = not ok_h
        ok, pct = (ok_hb if bigt else ok_h), 100 - (100 * mis[3 if bigt else 2]) // max(2 * f_blocks, 1)
    else:
        bigt = not ok_f and ok_fb
        ok, pct = (ok_fb if bigt else ok_f), 100 - (100 * mis[1 if bigt else 0]) // max(f_blocks, 1)
    # the density geometry (tiled.hip plan_reduce_kernel): a group of 1024 targets takes, per interval, the span of its four
    # forces groups; its tile holds TILE_CAP_D records beside the kernel table / without it
    edges, need_d = np.arange(0, f_blocks, 4), 0
    for q in range(3):
        has = ivl_len[q] > 0
        glo = np.minimum.reduceat(np.where(has, ivl_lo[q], big), edges)
        ghi = np.maximum.reduceat(np.where(has, ivl_lo[q] + ivl_len[q], 0), edges)
        need_d = need_d + np.where(ghi > glo, ghi - glo, 0)
    d_blocks = (n + 1023) // 1024
    mis_d = [int(np.count_nonzero(need_d > TILE_CAP_D[0])), int(np.count_nonzero(need_d > TILE_CAP_D[1]))]
    big_d = not mis_d[0] * 10 <= d_blocks and mis_d[1] * 10 <= d_blocks
    return dict(need=need[256], misfits=mis, fit_pct_forces=int(pct), half=use_half, ok=bool(ok), order=order, lo=ivl_lo, len=ivl_len,
                need_d=need_d, misfits_d=mis_d, fit_pct=int(100 - (100 * mis_d[1 if big_d else 0]) // max(d_blocks, 1)),
                ok_d=bool(mis_d[1 if big_d else 0] * 10 <= d_blocks))
