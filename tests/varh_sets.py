"""Adversarial particle sets for the variable-h pair passes and the h update (tests/test_varh_ref_cpu.py,
tests/test_varh_adversarial_gpu.py).

The geometric families of tests/octree_ref.py come back with LIVE fields (there u = v = alpha = 0 on purpose): seeded u in
[0.5, 2], a velocity field with converging parts (v.r < 0 for many pairs: the viscosity is on), alpha in [0.05, 1] and a
smoothing length that is no smooth function of position (half the distance to the 32nd neighbour times a seeded factor in
[0.5, 2], clipped to the variable-h defaults' range).  New here: clump_in_halo, far_clump (+ its fixed-h twin),
edge_pairs_v, h_routes, list_regrow_v -- each built to have a property that tests/test_varh_ref_cpu.py asserts.

No set has sinks: the accelerations are the SPH pair sums alone."""
from __future__ import annotations

import numpy as np

import octree_ref as R

H_LO, H_HI = 0.05, 9.9371       # inside the variable-h defaults' range; no round ceiling: 2 h must not tie with a lattice distance
SMALL = 3000                    # the brute-force restatement (tests/varh_ref.py) takes sets up to about this size
NO_SINKS = {k: np.zeros(0) for k in "x y z vx vy vz m".split()}


def live(geom, seed, h=None, factor=(0.5, 2.0)):
    """the set with live fields; h: given lengths instead of own_h (the factor applies to either)"""
    rng = np.random.default_rng(seed)
    pos = np.stack([geom["x"], geom["y"], geom["z"]], axis=1)
    n = pos.shape[0]
    c = pos.mean(axis=0) if n else np.zeros(3)
    scale = float(np.sqrt(np.mean(np.sum((pos - c) ** 2, axis=1)))) if n else 0.0
    k = rng.uniform(-0.2, 0.8, n)                      # mostly converging towards the centroid, partly diverging
    v = -(k[:, None] * (pos - c)) / (scale if scale > 0.0 else 1.0) + rng.normal(0.0, 0.2, (n, 3))
    h0 = R.own_h(geom, lo=H_LO, hi=H_HI) if h is None else np.asarray(h, dtype=np.float64)
    out = {k_: np.ascontiguousarray(geom[k_], dtype=np.float64).copy() for k_ in "xyzm"}
    out.update(vx=v[:, 0].copy(), vy=v[:, 1].copy(), vz=v[:, 2].copy(), u=rng.uniform(0.5, 2.0, n),
               alpha=rng.uniform(0.05, 1.0, n), h=np.clip(h0 * rng.uniform(factor[0], factor[1], n), H_LO, H_HI))
    return out


def take(gas, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in gas.items()}


def concat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def thin(geom, n_keep, seed):
    """a seeded subset that keeps the particles at the extremes of every axis (the root box, hence every split plane)"""
    n = geom["x"].size
    if n <= n_keep:
        return geom
    rng = np.random.default_rng(seed)
    keep = set()
    for a in "xyz":
        keep.update((int(np.argmin(geom[a])), int(np.argmax(geom[a]))))
    rest = np.setdiff1d(np.arange(n), np.fromiter(keep, dtype=np.int64))
    idx = np.sort(np.concatenate([np.fromiter(keep, dtype=np.int64), rng.choice(rest, n_keep - len(keep), replace=False)]))
    return {k: np.ascontiguousarray(v[idx]) for k, v in geom.items()}


def on_split_plane(gas, levels=4):
    """mask: the particle lies exactly on a split plane of its own octree path at some level <= levels"""
    pos = [gas["x"], gas["y"], gas["z"]]
    centre, size = R.root_box(*pos)
    c = [np.full(pos[0].shape, float(centre[a])) for a in range(3)]
    hit = np.zeros(pos[0].shape, dtype=bool)
    for _ in range(levels + 1):
        for a in range(3):
            hit |= pos[a] == c[a]
        q = 0.25 * size
        for a in range(3):
            c[a] = c[a] + np.where(pos[a] > c[a], q, -q)
        size *= 0.5
    return hit


# ---- the families of octree_ref with live fields -------------------------------------------------------------------------
def _family(name, small):
    if name == "lattice_ties":
        return thin(R.lattice(k=17), SMALL, 41) if small else R.lattice(k=17)
    if name.startswith("lattice"):
        g = R.lattice(k=int(name[7:]))
        return thin(g, SMALL, 40) if small else g
    if name == "sheet":
        return R.sheet(k=33) if small else R.sheet()
    if name == "plummer":
        return R.plummer(n=SMALL) if small else R.plummer()
    if name == "sparse_cube":
        return R.sparse_cube(n=SMALL) if small else R.sparse_cube()
    if name == "two_clusters":
        return R.two_clusters(n=SMALL) if small else R.two_clusters()
    if name == "shared_keys":
        return R.shared_keys(n=2900)
    return R.FAMILIES[name]()


GEOMETRIC = ["lattice17", "lattice33", "lattice_ties", "sheet", "line", "plummer", "sparse_cube", "two_clusters", "shared_keys",
             *[f"ragged{n}" for n in (1, 2, 3, 63, 64, 65, 127, 257)], "coincident"]


# ---- clump_in_halo -------------------------------------------------------------------------------------------------
def _ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    return v * (radius * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]


def clump_in_halo(order="natural", n_in=1500, n_out=1500, seed=51):
    """a dense ball (radius 1) inside a diffuse one (radius 60), sharp interface: a halo particle's kernel (h of a few
    units) covers clump particles whose small leaves its walk does not reach, and the reach of most pairs across the
    interface is one-sided -- which partner has the higher number then decides whether the pair exists ([V]:383).
    order: "natural" (clump first), "reversed", "random" (seeded permutation)."""
    rng = np.random.default_rng(seed)
    p = np.concatenate([_ball(rng, n_in, 1.0), _ball(rng, n_out, 60.0)])
    gas = live(R._gas(p[:, 0], p[:, 1], p[:, 2], np.full(n_in + n_out, 1.0e-4)), seed + 1)
    n = n_in + n_out
    perm = {"natural": np.arange(n), "reversed": np.arange(n)[::-1], "random": np.random.default_rng(seed + 2).permutation(n)}[order]
    return take(gas, perm), perm


# ---- far_clump -----------------------------------------------------------------------------------------------------
FAR = np.array([3000.0, 2500.0, 1500.0])


def far_clump(variant="corner", n_disc=20000, n_clump=64, seed=31):
    """a variable-h disc plus a clump of mutual neighbours (h near 8, sigma 5) far outside: the exact box needs more cells
    than a dense table may have (64 n + 4e6) but fewer than 2^27, so the grid is dense and TRIMMED to the bulk, and the
    whole clump is clamped into boundary cells.  variant: "corner" (beyond the high side of every axis), "low" (beyond the
    low side of every axis), "x_only" (beyond x only; three lone stragglers stretch the box along y and z)."""
    from summersph_amd import ic
    rows = ic.keplerian_disc_var(n_disc, seed=seed, with_sink=False)
    disc, _ = ic.split_rows_var(rows)
    rng = np.random.default_rng(seed + 100)
    centre = {"corner": FAR, "low": -FAR, "x_only": FAR * np.array([1.0, 0.0, 0.0])}[variant]
    p = centre + rng.normal(0.0, 5.0, (n_clump, 3))
    extra = [p]
    if variant == "x_only":
        extra.append(np.array([[5.0, FAR[1], FAR[2]], [-7.0, 0.8 * FAR[1], 3.0], [11.0, 2.0, 0.9 * FAR[2]]]))
    p = np.concatenate(extra)
    m = np.full(p.shape[0], disc["m"][0])
    pos = np.concatenate([np.stack([disc["x"], disc["y"], disc["z"]], axis=1), p])
    h = np.concatenate([disc["h"], np.full(p.shape[0], 8.0)])
    geom = R._gas(pos[:, 0], pos[:, 1], pos[:, 2], np.concatenate([disc["m"], m]))
    gas = live(geom, seed + 101, h=h, factor=(0.8, 1.25))
    is_clump = np.zeros(pos.shape[0], dtype=bool)
    is_clump[n_disc:n_disc + n_clump] = True
    return gas, is_clump


def far_clump_fixed(n_disc=20000, n_clump=64, seed=32, h=2.5):
    """the fixed-h twin: a fixed-h disc (with its sink) plus a far clump of mutual neighbours (sigma 0.6 h), for the tiled kernels"""
    from summersph_amd import ic
    gas, sinks = ic.split_rows(ic.keplerian_disc(n_disc, seed=seed))
    rng = np.random.default_rng(seed + 100)
    p = FAR + rng.normal(0.0, 0.6 * h, (n_clump, 3))
    add = {k: np.full(n_clump, float(np.mean(gas[k]))) for k in gas}
    add.update(x=p[:, 0], y=p[:, 1], z=p[:, 2], vx=rng.normal(0.0, 0.2, n_clump), vy=rng.normal(0.0, 0.2, n_clump),
               vz=rng.normal(0.0, 0.2, n_clump), u=rng.uniform(0.5, 2.0, n_clump))
    out = concat(gas, add)
    is_clump = np.zeros(n_disc + n_clump, dtype=bool)
    is_clump[n_disc:] = True
    return out, sinks, is_clump


def grid_box_replay(gas, h_fixed=None):
    """the box csrc/grid.hip's grid_rebuild gives the cell grid of a first build: edge 2 <h> (1 + 1e-6) (fixed h: 2 h), the
    exact bounding box unless it needs more than 64 n + 4e6 cells, else mean +- (6 sigma + 2 cells) of the particles inside
    the current box, repeated.  Returns exact_cells, cells, lo, hi, rounds, outside (mask of the particles outside the box)."""
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    n = pos.shape[0]
    edge = 2.0 * (float(np.sum(gas["h"]) / n) if h_fixed is None else h_fixed) * (1.0 + 1e-6)
    inv = 1.0 / edge
    lo, hi = pos.min(axis=0), pos.max(axis=0)

    def cells_of(lo_, hi_):
        return float(np.prod(np.floor((hi_ - lo_) * inv) + 1.0))

    exact = cells_of(lo, hi)
    limit = 64.0 * n + 4.0e6
    rounds = 0
    for _ in range(8):
        if not cells_of(lo, hi) > limit:
            break
        inside = np.all((pos >= lo) & (pos <= hi), axis=1)
        cnt = float(inside.sum())
        if not cnt >= 1.0:
            break
        mean = pos[inside].sum(axis=0) / cnt
        sig = np.sqrt(np.maximum((pos[inside] ** 2).sum(axis=0) / cnt - mean * mean, 0.0))
        half = 6.0 * sig + 2.0 * edge
        nlo, nhi = np.maximum(lo, mean - half), np.minimum(hi, mean + half)
        shrunk = bool(np.any(nlo > lo) or np.any(nhi < hi))
        lo, hi = nlo, nhi
        rounds += 1
        if not shrunk:
            break
    outside = ~np.all((pos >= lo) & (pos <= hi), axis=1)
    return dict(exact_cells=exact, cells=cells_of(lo, hi), limit=limit, lo=lo, hi=hi, rounds=rounds, outside=outside)


# ---- edge_pairs_v --------------------------------------------------------------------------------------------------
EDGE_KINDS = ["at_2hi", "at_2hj", "ulp_in_2hi", "ulp_out_2hi", "ulp_in_2hj", "ulp_out_2hj",
              "in_2hi", "out_2hi", "in_2hj", "out_2hj", "coincident"]


def edge_pairs_v(n_disc=2900, seed=61):
    """planted pairs (a, b) in a patch of a variable-h disc, b at x_a + d along x with the same y and z: d = 2 h_a, 2 h_b,
    one ulp to either side of each, 2 h (1 +- 1e-9), and d = 0; h_b = 1.37 h_a or 0.73 h_a.  x_a = 0 exactly, so that
    x_b - x_a and its square root are d to the bit.  Returns the set and {kind: (a, b)}."""
    from summersph_amd import ic
    disc, _ = ic.split_rows_var(ic.keplerian_disc_var(n_disc, seed=seed, with_sink=False))
    gas = live(R._gas(disc["x"], disc["y"], disc["z"], disc["m"]), seed + 1, h=disc["h"], factor=(0.8, 1.25))
    base = np.argsort(np.hypot(gas["x"], gas["y"] - 22.0) + np.abs(gas["z"]))[:2 * len(EDGE_KINDS)]
    pairs = {}
    for k, kind in enumerate(EDGE_KINDS):
        a, b = int(base[2 * k]), int(base[2 * k + 1])
        gas["h"][b] = gas["h"][a] * (1.37 if k % 2 == 0 else 0.73)
        ha, hb = gas["h"][a], gas["h"][b]
        d = {"at_2hi": 2.0 * ha, "at_2hj": 2.0 * hb,
             "ulp_in_2hi": np.nextafter(2.0 * ha, 0.0), "ulp_out_2hi": np.nextafter(2.0 * ha, np.inf),
             "ulp_in_2hj": np.nextafter(2.0 * hb, 0.0), "ulp_out_2hj": np.nextafter(2.0 * hb, np.inf),
             "in_2hi": 2.0 * ha * (1 - 1e-9), "out_2hi": 2.0 * ha * (1 + 1e-9),
             "in_2hj": 2.0 * hb * (1 - 1e-9), "out_2hj": 2.0 * hb * (1 + 1e-9), "coincident": 0.0}[kind]
        gas["x"][a] = 0.0
        gas["x"][b] = d
        gas["y"][b] = gas["y"][a]
        gas["z"][b] = gas["z"][a]
        pairs[kind] = (a, b)
    return gas, pairs


# ---- h_routes ------------------------------------------------------------------------------------------------------
def h_routes(n_disc=2400, seed=71, n_fringe=32, n_knot=40):
    """a set on which calc_smoothing takes every route and clause (tests/varh_ref.route_classes): a disc whose lengths
    were relaxed and then, per particle, over-estimated (x 1.1: the Newton step shrinks, no re-evaluation), slightly
    under-estimated (x 0.96: re-evaluations within 1.1 h0, the list route) or badly under-estimated (x 0.7: a trial length
    beyond 1.1 h0, the cell walk); a fringe of lone particles (hn = 1.73 h0 for a particle alone) with h0 in [6, 9.9]
    (first step beyond h_max_length: kept) and in [4, 5.6] (accepted, re-evaluated, then beyond h_iter_cap: loop left);
    and a tight knot with h just above h_min_length whose first step falls below it (kept)."""
    from oracle import orc, orc_v
    from summersph_amd import ic
    disc, _ = ic.split_rows_var(ic.keplerian_disc_var(n_disc, seed=seed, with_sink=False))
    gas = live(R._gas(disc["x"], disc["y"], disc["z"], disc["m"]), seed + 1, h=disc["h"], factor=(1.0, 1.0))
    o = orc_v.OracleV(gas, NO_SINKS, nthreads=orc.max_threads())
    for _ in range(8):                                   # relax h on the positions as they are
        o.density(); o.update_h()
    rng = np.random.default_rng(seed + 2)
    gas["h"] = np.clip(o.h * rng.choice([1.1, 0.96, 0.7], n_disc), H_LO, H_HI)
    ang = 2.0 * np.pi * np.arange(2 * n_fringe) / (2 * n_fringe)
    fr = R._gas(800.0 * np.cos(ang), 800.0 * np.sin(ang), np.zeros(2 * n_fringe), np.full(2 * n_fringe, disc["m"][0]))
    hf = np.concatenate([rng.uniform(6.0, 9.9, n_fringe), rng.uniform(4.0, 5.6, n_fringe)])
    fringe = live(fr, seed + 3, h=hf, factor=(1.0, 1.0))
    kp = np.array([25.0, 0.0, 12.0]) + _ball(rng, n_knot, 0.004)
    knot = live(R._gas(kp[:, 0], kp[:, 1], kp[:, 2], np.full(n_knot, disc["m"][0])), seed + 4, h=np.full(n_knot, 1.0))
    knot["h"] = rng.uniform(0.0101, 0.0108, n_knot)     # (live() clips to the defaults' range, whose floor is above this)
    return concat(gas, fringe, knot)


# ---- list_regrow_v -------------------------------------------------------------------------------------------------
def list_regrow_v(n_knot=500, n_halo=900, seed=81):
    """a dense knot (radius 1) in a ball of radius 9, h near 3 for all: every knot particle has hundreds of D/F entries
    and hundreds of candidates between 2 h and the margins (2.2 h_i reached, 2.14 max(h_i, h_j)) -- the list outgrows its
    initial 96 slots from both ends of a column"""
    rng = np.random.default_rng(seed)
    p = np.concatenate([_ball(rng, n_knot, 1.0), _ball(rng, n_halo, 9.0)])
    n = n_knot + n_halo
    return live(R._gas(p[:, 0], p[:, 1], p[:, 2], np.full(n, 1.0e-4)), seed + 1, h=np.full(n, 3.0), factor=(0.8, 1.25))


def margin_counts(ref, grow=1.07):
    """per particle: entries of a list build with D or F, and entries of its margin shell (csrc/varh.hip nlist_v_tiled:
    reached and within 2.2 h_i, or within 2 grow max(h_i, h_j)), from a VarhRef"""
    off = ~np.eye(ref.n, dtype=bool)
    df = (ref.in_D | ref.in_F) & off
    hmax = np.maximum(ref.h[:, None], ref.h[None, :])
    shell = off & ~df & ((ref.reach & (ref.r <= 2.2 * ref.h[:, None])) | (ref.r <= 2.0 * grow * hmax))
    return df.sum(axis=1), shell.sum(axis=1)


# ---- registry ------------------------------------------------------------------------------------------------------
def build(name, small=False):
    """the set `name` as a gas dict with live fields and h (no sinks).  small: at most ~3000 particles"""
    if name == "lattice_ties":
        # dyadic lengths on a lattice with dyadic leaf boxes: |x_i - c_j| = 2 h_j + e_j / 2 EXACTLY for many pairs -- the
        # strict '<' of the reach test decides them
        g = _family(name, small)
        rng = np.random.default_rng(999)
        return live(g, 998, h=rng.choice([1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 3.0], g["x"].size), factor=(1.0, 1.0))
    if name in GEOMETRIC:
        return live(_family(name, small), 1000 + GEOMETRIC.index(name))
    if name.startswith("clump_in_halo"):
        return clump_in_halo(order=name[14:] or "natural")[0]
    if name.startswith("far_clump"):
        variant = name[10:] or "corner"
        return far_clump(variant, n_disc=2900, n_clump=40)[0] if small else far_clump(variant)[0]
    if name == "edge_pairs_v":
        return edge_pairs_v()[0]
    if name == "h_routes":
        return h_routes()
    if name == "list_regrow_v":
        return list_regrow_v()
    raise KeyError(name)


NEW = ["clump_in_halo", "clump_in_halo_reversed", "clump_in_halo_random", "far_clump", "far_clump_x_only", "far_clump_low",
       "edge_pairs_v", "h_routes", "list_regrow_v"]
ALL = GEOMETRIC + NEW
HAS_TIES = {"lattice_ties", "edge_pairs_v"}                # pairs exactly on a support edge or a reach boundary: no count checks
HAS_COINCIDENT = {"coincident", "edge_pairs_v"}          # sets with exactly coincident points (DESIGN section 2's deviation)
