"""Node grids and particle sets that stress the binning of the image-forming passes (tests/test_image_sets_cpu.py,
tests/test_render_binning_gpu.py, tests/test_cube_binning_gpu.py): sph_render_density / sph_render_field
(summersph_amd/csrc/render.hip) and sph_cube (summersph_amd/csrc/cube.hip).

Two things, in plain numpy.

(a) A restatement of the host sizing and of the gather's staging, render_sizing() and cube_sizing().  They restate and
    MUST FOLLOW
      render.hip  render_impl, "render grid": origin lo - reach, reach = 2 h_max (1 + 1e-6), edge 2 h_max multiplied by
                  2^(1/3) while the product of ceil(ext / edge) exceeds MAX_CELLS = 2^26, dim = ceil(ext / edge);
                  cell_1d, node_coord, render_select's reach test, and gather_body's candidate cells, its intervals (one
                  per (cx, cy) of the brick's cell range), the batches of GT = 64 intervals and the chunks of CH = 256
                  records; ysegs = min(nseg, 65535)
      cube.hip    cube_run, "image-plane grid": the same with the factor 2^(1/2) against MAX_CELLS = 2^22, then the edge
                  halved while half of it still spans a tile of nodes and an eighth of the reach and the table stays
                  within MAX_CELLS; cube_gather's intervals (one per cell row of the tile's range), batches of 64, chunks
                  of CH = 128
    and return the edge, the number of enlargements and halvings, dim, ncells and, per brick, n_int and the number of
    records in every batch.  If the sizing in either file changes, these change with it, and tests/test_image_sets_cpu.py
    then says which case no longer takes the path it is named for.

(b) The cases: render_case(name) and cube_case(name), each a dict of particles, node box, n, h and the clip.  Every case
    has at most 4000 particles and at most 2000 contributing terms at any node (asserted in the CPU test)."""
from __future__ import annotations

import functools

import numpy as np

TILE = 8                 # TU = TV: node columns per workgroup side
KW = 8                   # nodes per lane along the walk axis per segment (render)
GT = 64                  # intervals per batch (both passes)
RENDER_CH = 256          # records per LDS chunk, render
CUBE_CH = 128            # records per LDS chunk, cube
RENDER_MAX_CELLS = 1 << 26
CUBE_MAX_CELLS = 1 << 22
YSEGS_MAX = 65535
REACH = 1.0 + 1e-6
CBRT2 = 1.2599210498948732
SQRT2 = 1.4142135623730951


# ---- the kernels' node and cell functions ---------------------------------------------------------------------------
def node_coords(lo, hi, n):
    """node_coord: i * step + lo with step = (hi - lo) / (n - 1), the last node exactly hi; n == 1: the single node lo"""
    lo, hi, n = float(lo), float(hi), int(n)
    if n == 1:
        return np.array([lo])
    step = (hi - lo) / (n - 1)
    g = np.arange(n, dtype=np.float64) * step + lo
    g[-1] = hi
    return g


def cell_1d(org, inv_edge, dim, p):
    t = np.floor((np.asarray(p, dtype=np.float64) - org) * inv_edge)
    return np.minimum(np.maximum(t, 0.0), float(dim - 1)).astype(np.int64)


def select(pos, clip=None, n_owned=None):
    n = pos.shape[0]
    sel = np.arange(n) < (n if n_owned is None else n_owned)
    if clip is not None:
        lo, hi = np.asarray(clip, dtype=np.float64).reshape(2, 3)
        sel &= np.all((pos > lo) & (pos < hi), axis=1)
    return sel


def _batches(lens):
    """records per batch of GT intervals"""
    nb = (lens.size + GT - 1) // GT
    pad = np.zeros(nb * GT, dtype=np.int64)
    pad[:lens.size] = lens
    return pad.reshape(nb, GT).sum(axis=1)


# ---- render.hip -----------------------------------------------------------------------------------------------------
def render_sizing(pos, h, lo, hi, n, axis=None, clip=None, bricks=True):
    """pos (N, 3), h a number or (N,), the node box lo / hi (None: SPH_RENDER_AUTO_BOUNDS), n, axis (None: 3-D mode).
    Returns dict(lo, hi, edge, enlargements, halvings = 0, dim, ncells, nsel, nseg, ysegs, tiles, bricks); bricks is a list
    of dict(tu, tv, seg, n_int, lens (records per interval), batch_records, cells (clo, chi)), empty with bricks=False."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = tuple(int(v) for v in n)
    sel = select(pos, clip)
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (pos.shape[0],))[sel]
    p = pos[sel]
    if lo is None:
        lo, hi = p.min(axis=0), p.max(axis=0)
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.where(np.array(n) == 1, lo, np.asarray(hi, dtype=np.float64))          # the kernels' copy
    W = 0 if axis is None else int(axis)
    U, V = (1 if W == 0 else 0), (1 if W == 2 else 2)
    out = dict(lo=lo, hi=hi, halvings=0, nsel=0, enlargements=0, bricks=[], W=W,
               nseg=(n[W] + KW - 1) // KW, tiles=((n[U] + TILE - 1) // TILE, (n[V] + TILE - 1) // TILE))
    out["ysegs"] = 1 if axis is not None else min(out["nseg"], YSEGS_MAX)
    if p.shape[0] == 0:
        out.update(edge=0.0, dim=(0, 0, 0), ncells=1)
        return out
    h_max = float(hh.max())
    reach = 2.0 * h_max * REACH
    org = lo - reach
    ext = (hi + reach) - org
    edge = 2.0 * h_max
    while np.prod(np.maximum(1.0, np.ceil(ext / edge))) > float(RENDER_MAX_CELLS):
        edge *= CBRT2
        out["enlargements"] += 1
    dim = np.maximum(1.0, np.ceil(ext / edge)).astype(np.int64)
    inv_edge = 1.0 / edge
    out.update(edge=edge, dim=tuple(int(d) for d in dim), ncells=int(np.prod(dim)), h_max=h_max, reach=reach)
    own = 2.0 * hh * REACH
    near = np.all((p >= lo - own[:, None]) & (p <= hi + own[:, None]), axis=1)
    q = p[near]
    out["nsel"] = int(near.sum())
    c = [cell_1d(org[a], inv_edge, dim[a], q[:, a]) for a in range(3)]
    keys = np.sort((c[0] * dim[1] + c[1]) * dim[2] + c[2])
    if not bricks:
        return out
    g = [node_coords(lo[a], hi[a], n[a]) for a in range(3)]
    for tu in range(out["tiles"][0]):
        for tv in range(out["tiles"][1]):
            for seg in range(out["nseg"]):
                i0, i1 = [0] * 3, [0] * 3
                i0[W], i1[W] = seg * KW, min(n[W], seg * KW + KW) - 1
                i0[U], i1[U] = tu * TILE, min(n[U], tu * TILE + TILE) - 1
                i0[V], i1[V] = tv * TILE, min(n[V], tv * TILE + TILE) - 1
                clo = [int(cell_1d(org[a], inv_edge, dim[a], g[a][i0[a]] - reach)) for a in range(3)]
                chi = [int(cell_1d(org[a], inv_edge, dim[a], g[a][i1[a]] + reach)) for a in range(3)]
                n1c, n2c = chi[1] - clo[1] + 1, chi[2] - clo[2] + 1
                n_int = (chi[0] - clo[0] + 1) * n1c
                r = np.arange(n_int, dtype=np.int64)
                k0 = ((clo[0] + r // n1c) * dim[1] + (clo[1] + r % n1c)) * dim[2] + clo[2]
                lens = np.searchsorted(keys, k0 + n2c) - np.searchsorted(keys, k0)
                out["bricks"].append(dict(tu=tu, tv=tv, seg=seg, n_int=int(n_int), lens=lens, batch_records=_batches(lens),
                                          cells=(clo, chi), nodes=(i0, i1)))
    return out


# ---- cube.hip -------------------------------------------------------------------------------------------------------
def cube_sizing(P, h, lo, hi, n):
    """P (N, 2): the selected particles in the image plane, h a number or (N,), the node box and n = (n_u, n_v).  Returns
    dict(edge, enlargements, halvings, dim, ncells, nsel, tiles: list of dict(tu, tv, n_int, lens, batch_records))."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    n = tuple(int(v) for v in n)
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (P.shape[0],))
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.where(np.array(n) == 1, lo, np.asarray(hi, dtype=np.float64))
    step = np.array([(hi[a] - lo[a]) / (n[a] - 1) if n[a] > 1 else 0.0 for a in range(2)])
    h_max = float(hh.max())
    reach = 2.0 * h_max * REACH
    org = lo - reach
    ext = (hi + reach) - org
    edge = 2.0 * h_max

    def cells(e):
        return float(np.prod(np.maximum(1.0, np.ceil(ext / e))))

    out = dict(enlargements=0, halvings=0, tiles=[])
    while cells(edge) > float(CUBE_MAX_CELLS):
        edge *= SQRT2
        out["enlargements"] += 1
    tile = max(TILE * step[0], TILE * step[1])
    while tile > 0.0 and 0.5 * edge >= tile and 0.5 * edge >= 0.125 * reach and cells(0.5 * edge) <= float(CUBE_MAX_CELLS):
        edge *= 0.5
        out["halvings"] += 1
    dim = np.maximum(1.0, np.ceil(ext / edge)).astype(np.int64)
    inv_edge = 1.0 / edge
    own = 2.0 * hh * REACH
    near = np.all((P >= lo - own[:, None]) & (P <= hi + own[:, None]), axis=1)
    q = P[near]
    keys = np.sort(cell_1d(org[0], inv_edge, dim[0], q[:, 0]) * dim[1] + cell_1d(org[1], inv_edge, dim[1], q[:, 1]))
    out.update(edge=edge, dim=tuple(int(d) for d in dim), ncells=int(dim[0] * dim[1]), nsel=int(near.sum()), h_max=h_max)
    g = [node_coords(lo[a], hi[a], n[a]) for a in range(2)]
    for tu in range((n[0] + TILE - 1) // TILE):
        for tv in range((n[1] + TILE - 1) // TILE):
            u0, u1 = tu * TILE, min(n[0], tu * TILE + TILE) - 1
            v0, v1 = tv * TILE, min(n[1], tv * TILE + TILE) - 1
            clo0, chi0 = (int(cell_1d(org[0], inv_edge, dim[0], x)) for x in (g[0][u0] - reach, g[0][u1] + reach))
            clo1, chi1 = (int(cell_1d(org[1], inv_edge, dim[1], x)) for x in (g[1][v0] - reach, g[1][v1] + reach))
            n_int = chi0 - clo0 + 1
            k0 = (clo0 + np.arange(n_int, dtype=np.int64)) * dim[1] + clo1
            lens = np.searchsorted(keys, k0 + (chi1 - clo1 + 1)) - np.searchsorted(keys, k0)
            out["tiles"].append(dict(tu=tu, tv=tv, n_int=int(n_int), lens=lens, batch_records=_batches(lens)))
    return out


# ---- particles ------------------------------------------------------------------------------------------------------
def _gas(pos, m, h=None, seed=0):
    """a gas dict for Context.upload: seeded velocities and u; h only where the case is a variable-h one"""
    rng = np.random.default_rng(1000 + seed)
    n = pos.shape[0]
    v = rng.normal(0.0, 1.0, (n, 3))
    out = {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "vx": v[:, 0], "vy": v[:, 1], "vz": v[:, 2],
           "u": rng.uniform(0.5, 2.0, n), "m": m}
    if h is not None:
        out["h"] = h
    return {k: np.ascontiguousarray(a, dtype=np.float64).copy() for k, a in out.items()}


def _masses(rng, n):
    return rng.uniform(1e-7, 3e-6, n)


def _clustered(rng, n):
    c = rng.uniform(-20, 20, (6, 3))
    return c[rng.integers(0, 6, n)] + rng.normal(0, rng.uniform(0.5, 4, n)[:, None], (n, 3))


def _case(pos, m, lo, hi, n, h, clip=None, hvar=None, seed=0, **more):
    return dict(gas=_gas(pos, m, hvar, seed), variable=hvar is not None, lo=None if lo is None else np.asarray(lo, dtype=np.float64),
                hi=None if hi is None else np.asarray(hi, dtype=np.float64), n=tuple(n), h=h, clip=clip, **more)


def case_pos(case):
    g = case["gas"]
    return np.stack([g["x"], g["y"], g["z"]], axis=1)


def field_values(n):
    """the signed A of the field render and the cube: sin of the particle index"""
    return np.sin(1.0 + np.arange(n, dtype=np.float64))


def render_nodes(case):
    """the node box the render uses (SPH_RENDER_AUTO_BOUNDS: the selection's min / max) and the three node axes"""
    lo, hi = case["lo"], case["hi"]
    if lo is None:
        p = case_pos(case)[select(case_pos(case), case["clip"])]
        lo, hi = p.min(axis=0), p.max(axis=0)
    return lo, hi, [node_coords(lo[a], hi[a], case["n"][a]) for a in range(3)]


def case_h(case):
    """the h the render uses: the case's one h, or the uploaded per-particle h"""
    return case["gas"]["h"] if case["h"] is None else case["h"]


# coarse: x is the walk axis of the 3-D mode, (y, z) the tile.  With h = 0.25 the cell edge is 0.5 and node 0 of every axis
# sits at cell 1 (+ 1e-6).  The y tile of nodes 0..7 spans 7 * 4.3556 + 2 * 0.5 = 31.49 -> cells 0..62: n1c = 63, so the
# brick's interval r is cell (r // 63, r % 63) of (x, y): r = 0 -> (0, 0), r = 63 -> (1, 0), r = 64 -> (1, 1), all three
# within 2h of node (0, 0) in x and y.  x node 7 sits at cell 65.6, so the brick's last cell row, 66, starts 0.21 from it: the
# brick has 67 * 63 = 4221 = 65 * 64 + 61 intervals, and the ragged 66th batch holds cell row 66 from y cell 2 on.
COARSE = dict(n=(9, 10, 9), lo=(-18.0, -19.6, -18.0), hi=(18.9, 19.6, 18.0), h=0.25, count=2500, seed=11)


def _coarse_planted(lo, hi, n, h):
    """particles within 2h of nodes of the first brick, in chosen intervals: ((x, y, z), ...)"""
    g = [node_coords(lo[a], hi[a], n[a]) for a in range(3)]
    d = 0.4 * h
    pts = [(g[0][0] - d, g[1][0] - d, g[2][0] + d),            # cell (0, 0): r = 0
           (g[0][0] + d, g[1][0] - d, g[2][0] - d),            # cell (1, 0): r = 63
           (g[0][0] + d, g[1][0] + d, g[2][3] + d),            # cell (1, 1): r = 64
           (g[0][0] + d, g[1][0] + d, g[2][3] - d)]            #   a second record of the same interval
    for k in range(1, 8):                                      # one near every x node of the brick, y node k, z node 7 - k
        pts.append((g[0][k] - d, g[1][k] + d, g[2][7 - k] - d))
    pts.append((g[0][7] + 1.2 * h, g[1][7] + d, g[2][2]))      # the brick's last cell row in x: the ragged batch
    pts.append((g[0][7] + 1.2 * h, g[1][1] + d, g[2][5]))
    return np.array(pts)


def _coarse(shift=(0.0, 0.0, 0.0)):
    c = COARSE
    rng = np.random.default_rng(c["seed"])
    pos = _clustered(rng, c["count"])
    # a slab of cell rows with no particle at all: whole batches of the first brick are empty between non-empty ones
    pos = pos[~((pos[:, 0] > -12.0) & (pos[:, 0] < -9.0))]
    pos = np.vstack([_coarse_planted(c["lo"], c["hi"], c["n"], c["h"]), pos])
    m = _masses(rng, pos.shape[0])
    s = np.asarray(shift, dtype=np.float64)
    return _case(pos + s, m, np.asarray(c["lo"]) + s, np.asarray(c["hi"]) + s, c["n"], c["h"], seed=1)


OFFSET = (1.0e7, -3.0e6, 2.0e5)


def _cells_clamped():
    """17^3 nodes over +-700, h = 1: 703^3 cells of edge 2 -> three enlargements, edge 4, 352^3 cells"""
    rng = np.random.default_rng(23)
    n, lo, hi, h = (17, 17, 17), np.full(3, -700.0), np.full(3, 700.0), 1.0
    g = node_coords(-700.0, 700.0, 17)
    idx = rng.integers(0, 17, (1500, 3))
    off = rng.normal(size=(1500, 3))
    off *= (rng.uniform(0.0, 1.9, 1500) / np.linalg.norm(off, axis=1))[:, None]
    near = g[idx] + off                                        # within 1.9 h of a node
    spread = rng.uniform(-702.0, 702.0, (1500, 3))
    edge = []
    for a in range(3):                                         # outside each of the six faces, within reach of a face node
        for side, sgn in ((0, -1.0), (16, 1.0)):
            i = rng.integers(0, 17, 3)
            p = g[i].copy(); p[a] = g[side] + sgn * 1.3
            edge.append(p)
    for sx in (0, 16):                                         # outside each of the eight corners
        for sy in (0, 16):
            for sz in (0, 16):
                s = np.array([sx, sy, sz])
                edge.append(g[s] + np.where(s == 0, -1.0, 1.0) * 0.9)
    pos = np.vstack([np.array(edge), near, spread])
    return _case(pos, _masses(rng, pos.shape[0]), lo, hi, n, h, seed=2)


CHUNK_COUNTS = (255, 256, 257, 513)


def _chunk_counts(k):
    """one brick (5^3 nodes over +-2, h = 0.5) with exactly k records within its reach; k = 513: all in one cell, on a node"""
    rng = np.random.default_rng(300 + k)
    n, lo, hi, h = (5, 5, 5), np.full(3, -2.0), np.full(3, 2.0), 0.5
    pos = np.zeros((k, 3)) if k == 513 else rng.uniform(-2.9, 2.9, (k, 3))
    far = rng.uniform(5.0, 9.0, (40, 3))                       # selected, out of reach: no record
    return _case(np.vstack([pos, far]), _masses(rng, k + 40), lo, hi, n, h, seed=3, records=k)


def _h_decades():
    rng = np.random.default_rng(41)
    n, lo, hi = (12, 11, 9), np.array([-10.0, -9.0, -6.0]), np.array([10.0, 9.0, 6.0])
    g = [node_coords(lo[a], hi[a], n[a]) for a in range(3)]
    nb = 1400
    pos = rng.uniform(lo - 1.0, hi + 1.0, (nb, 3))
    h = np.exp(rng.uniform(np.log(1e-3), np.log(8.0), nb))
    sp_pos, sp_h, kind = [], [], []
    for k in range(20):                                        # small h: exactly on a node, one ulp off, midway
        i = [rng.integers(0, n[a] - 1) for a in range(3)]
        node = np.array([g[a][i[a]] for a in range(3)])
        nxt = np.array([g[a][i[a] + 1] for a in range(3)])
        hs = float(np.exp(rng.uniform(np.log(1e-3), np.log(1e-2))))
        sp_pos += [node, np.nextafter(node, nxt), 0.5 * (node + nxt)]
        sp_h += [hs, hs, hs]
        kind += ["on", "ulp", "mid"]
    out_pos = np.array([[hi[0] + 10.0, 1.0, 0.5], [lo[0] - 12.0, -3.0, 1.0], [2.0, hi[1] + 14.0, -2.0], [-4.0, 3.0, lo[2] - 15.0],
                        [hi[0] + 9.0, hi[1] + 9.0, hi[2] + 9.0], [hi[0] + 17.0, 0.0, 0.0]])     # the last: out of reach
    pos = np.vstack([np.array(sp_pos), out_pos, pos])
    h = np.concatenate([np.array(sp_h), np.full(out_pos.shape[0], 8.0), h])
    return _case(pos, _masses(rng, pos.shape[0]), lo, hi, n, None, hvar=h, seed=4, kinds=kind)


def _flat_z():
    """coplanar particles and SPH_RENDER_AUTO_BOUNDS: lo[2] == hi[2], five coincident node planes"""
    rng = np.random.default_rng(51)
    k = 1500
    r, ph = 10.0 * np.sqrt(rng.uniform(0, 1, k)), rng.uniform(0, 2 * np.pi, k)
    pos = np.stack([r * np.cos(ph), r * np.sin(ph), np.full(k, 0.3)], axis=1)
    return _case(pos, _masses(rng, k), None, None, (21, 19, 5), 0.5, seed=5, flat=2)


def _flat_x():
    """the explicit form: lo == hi on x with nine nodes"""
    rng = np.random.default_rng(52)
    k = 1200
    pos = rng.uniform([-1.5, -6.0, -5.0], [3.5, 6.0, 5.0], (k, 3))
    return _case(pos, _masses(rng, k), (1.0, -5.0, -4.0), (1.0, 5.0, 4.5), (9, 13, 11), 0.5, seed=6, flat=0)


LONG_N = 8 * 65535 + 9


def _long_axis():
    """65 537 segments along x in 3-D mode: the gridDim.y cap and the seg += gridDim.y stride (segments 65535 and 65536 are
    the second trips of blocks 0 and 1, which also run segments 0 and 1)"""
    rng = np.random.default_rng(61)
    x = np.concatenate([[-0.4, 0.0, 0.004, 0.02, 999.97, 999.985, 999.99, 1000.0, 1000.3], rng.uniform(0.0, 1000.0, 55)])
    pos = np.stack([x, rng.uniform(-0.5, 0.5, x.size), rng.uniform(-0.5, 0.5, x.size)], axis=1)
    return _case(pos, _masses(rng, x.size), (0.0, 0.1, -0.05), (1000.0, 0.1, -0.05), (LONG_N, 1, 1), 0.5, seed=7)


def _nothing_reaches(which):
    rng = np.random.default_rng(71)
    pos = rng.uniform(20.0, 30.0, (500, 3))
    m = _masses(rng, 500)
    lo, hi, n = (-5.0, -5.0, -2.0), (5.0, 5.0, 2.0), (11, 9, 10)
    if which == "far":                                         # a non-empty selection none of which reaches the box
        return _case(pos, m, lo, hi, n, 1.0, seed=8)
    clip = ((100.0, 100.0, 100.0), (101.0, 101.0, 101.0))       # a clip that selects nothing, explicit bounds
    return _case(pos - 25.0, m, lo, hi, n, 1.0, clip=clip, seed=8)


RENDER_CASES = (["coarse", "cells_clamped"] + [f"chunk_counts_{k}" for k in CHUNK_COUNTS] +
                ["h_decades", "flat_z", "flat_x", "long_axis", "offset", "nothing_far", "nothing_clipped"])


@functools.lru_cache(maxsize=None)
def render_case(name):
    if name == "coarse":
        return _coarse()
    if name == "offset":
        return _coarse(OFFSET)
    if name == "cells_clamped":
        return _cells_clamped()
    if name.startswith("chunk_counts_"):
        return _chunk_counts(int(name.rsplit("_", 1)[1]))
    if name == "h_decades":
        return _h_decades()
    if name == "flat_z":
        return _flat_z()
    if name == "flat_x":
        return _flat_x()
    if name == "long_axis":
        return _long_axis()
    if name == "nothing_far":
        return _nothing_reaches("far")
    if name == "nothing_clipped":
        return _nothing_reaches("clipped")
    raise KeyError(name)


# ---- cube cases -----------------------------------------------------------------------------------------------------
def _rotation():
    """a right-handed orthonormal frame with no zero entry (rows u^, v^, w^)"""
    a, b, c = 0.7, -0.4, 1.1
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1.0, 0], [-np.sin(b), 0, np.cos(b)]])
    rx = np.array([[1.0, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return rz @ ry @ rx


ROT = _rotation()
CENTRE = (0.5, -1.0, 2.0)
V_REF = (0.1, 0.0, -0.2)
N_CHAN = 33                                # CUBE_CHUNK = 32: a second channel chunk of one channel
DV = 0.25
V0 = -28 * DV                              # channels centred on -7 .. 1: the frame velocities, N(0, 1), pile up about channel 28
SIGMA_FLOOR = 1.5 * DV                     # a record's 8.5 sigma reach is 12.75 channels either side: most straddle channel 31 | 32
CUBE_CHUNKS = (127, 128, 129, 257)


def _cube_case(P, w_depth, m, lo, hi, n, h, seed, **more):
    """P (N, 2) image-plane positions -> particles r = rot^T (P, depth) + centre"""
    frame = np.concatenate([P, w_depth[:, None]], axis=1)
    pos = frame @ ROT + np.asarray(CENTRE)                    # rot^T applied to every row
    gas = _gas(pos, m, None, seed)
    return dict(gas=gas, variable=False, lo=tuple(float(v) for v in lo), hi=tuple(float(v) for v in hi), n=tuple(n), h=h,
                rot=ROT, centre=CENTRE, v_ref=V_REF, v0=V0, dv=DV, n_chan=N_CHAN, sigma_floor=SIGMA_FLOOR, **more)


def _near_nodes(rng, lo, hi, n, h, count):
    g = [node_coords(lo[a], hi[a], n[a]) for a in range(2)]
    i = np.stack([rng.integers(0, n[a], count) for a in range(2)], axis=1)
    off = rng.normal(size=(count, 2))
    off *= (h * rng.uniform(0.0, 1.9, count) / np.linalg.norm(off, axis=1))[:, None]
    return np.stack([g[0][i[:, 0]], g[1][i[:, 1]]], axis=1) + off


def _cube_spread(seed, half, n, h, near, spread):
    rng = np.random.default_rng(seed)
    lo, hi = (-half, -half), (half, half)
    P = np.vstack([_near_nodes(rng, lo, hi, n, h, near), rng.uniform(-half - 2 * h, half + 2 * h, (spread, 2))])
    # outside the four sides and the four corners, within reach
    e = 1.2 * h
    extra = [(-half - e, 0.0), (half + e, 0.0), (0.0, -half - e), (0.0, half + e)] + [(sx * (half + 0.8 * h), sy * (half + 0.8 * h))
                                                                                   for sx in (-1, 1) for sy in (-1, 1)]
    P = np.vstack([np.array(extra), P])
    return _cube_case(P, rng.uniform(-5, 5, P.shape[0]), _masses(rng, P.shape[0]), lo, hi, n, h, seed)


def _cube_halved():
    """65^2 nodes over +-4 with h = 8: 3 x 3 cells of edge 16 halved twice (edge 4: half of it, 2, is below reach / 8)"""
    rng = np.random.default_rng(83)
    P = rng.uniform(-19.0, 19.0, (300, 2))
    return _cube_case(P, rng.uniform(-5, 5, 300), _masses(rng, 300), (-4.0, -4.0), (4.0, 4.0), (65, 65), 8.0, 83)


def _cube_chunks(k):
    rng = np.random.default_rng(400 + k)
    P = np.vstack([rng.uniform(-2.9, 2.9, (k, 2)), rng.uniform(5.0, 9.0, (30, 2))])
    return _cube_case(P, rng.uniform(-5, 5, k + 30), _masses(rng, k + 30), (-2.0, -2.0), (2.0, 2.0), (5, 5), 0.5, 400 + k, records=k)


def _cube_flat():
    rng = np.random.default_rng(91)
    P = rng.uniform([-1.0, -6.0], [3.0, 6.0], (800, 2))
    return _cube_case(P, rng.uniform(-5, 5, 800), _masses(rng, 800), (1.0, -5.0), (1.0, 5.0), (5, 13), 0.5, 91, flat=0)


CUBE_CASES = ["cube_coarse", "cube_clamped", "cube_halved"] + [f"cube_chunks_{k}" for k in CUBE_CHUNKS] + ["cube_flat"]


@functools.lru_cache(maxsize=None)
def cube_case(name):
    if name == "cube_coarse":          # a tile of 8 nodes spans 7 * 25 + 4 h = 175.6 -> 585 cells of 0.3 along u: 10 batches
        return _cube_spread(81, 100.0, (9, 9), 0.15, 400, 1600)
    if name == "cube_clamped":         # 2602^2 cells of edge 2 -> one enlargement; a tile spans 2279 / 2.83 = 806 cells: 13 batches
        return _cube_spread(82, 2600.0, (17, 17), 1.0, 1500, 1500)
    if name == "cube_halved":
        return _cube_halved()
    if name.startswith("cube_chunks_"):
        return _cube_chunks(int(name.rsplit("_", 1)[1]))
    if name == "cube_flat":
        return _cube_flat()
    raise KeyError(name)
