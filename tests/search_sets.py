"""Adversarial source sets for the calls that find their pairs through the hashed cell table: sph_sample, sph_trace and
sph_gradients (tests/test_search_sets_cpu.py, tests/test_sample_adversarial_gpu.py, tests/test_gradients_adversarial_gpu.py).

Three parts, numpy only, no GPU:

  sets          named particle sets, each built to reach a branch of the device-side planning (sample_levels and set_level in
                csrc/sample.hip, grad_box in csrc/gradients.hip) or of the cell arithmetic (csrc/cell_table.hpp) that the discs,
                the uniform box and the golden fixtures do not reach
  plans         plan_sample and plan_gradients restate that planning on the host.  Nothing on the device exposes it, so what
                a set claims about itself (merged levels, enlarged edges, nodes on cell faces, the walk's cost) is a property
                of its inputs, asserted on the CPU: a kernel that meets the contract cannot avoid the branch
  references    brute_sample and brute_gradients: plain all-pairs sums in np.longdouble, no tree, no cells, with what the
                per-point error bounds need (the count of reaching sources and the sums of the absolute weights)."""
from __future__ import annotations

import numpy as np

DBL_BIG = float(np.finfo(np.float64).max)
HBINS = 8192                                   # quarter octaves of a positive double: bits >> 50
HSHIFT = 50
MAX_LEVELS = 64
LEVEL_AXIS_MASK = (1 << 19) - 1
LEVEL_AXIS_CELLS = float((1 << 19) - 8)
AXIS_MASK = (1 << 21) - 1
AXIS_CELLS = float((1 << 21) - 8)
LD = np.longdouble
PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)  # pi to the long double's precision where it has one


class SearchSet:
    """name, gas (a dict for Context.upload), variable (per-particle h in gas["h"]) or the one h of a fixed-h context"""

    def __init__(self, name, pos, m, h, seed):
        rng = np.random.default_rng(1000 + seed)
        n = pos.shape[0]
        self.name = name
        self.variable = np.ndim(h) == 1
        self.h = np.ascontiguousarray(h, dtype=np.float64) if self.variable else float(h)
        self.gas = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": rng.normal(size=n),
                    "vy": rng.normal(size=n), "vz": rng.normal(size=n), "u": rng.uniform(0.5, 2.0, n),
                    "m": np.ascontiguousarray(m, dtype=np.float64), "alpha": np.zeros(n)}
        if self.variable:
            self.gas["h"] = self.h.copy()

    @property
    def n(self):
        return self.gas["x"].size

    @property
    def pos(self):
        return np.stack([self.gas["x"], self.gas["y"], self.gas["z"]], axis=1)

    @property
    def m(self):
        return self.gas["m"]

    @property
    def h_all(self):
        return self.h if self.variable else np.full(self.n, self.h)

    def context_kw(self):
        """keyword arguments of capi.Context for this set"""
        return {"variable": True} if self.variable else {"h": self.h}


# ---- the sets ----------------------------------------------------------------------------------------------------------
def _unit_mass(h, rng):
    """m = pi h^3 U(0.5, 1.5): every ws_j = m_j / (pi h_j^3) is O(1) whatever h_j"""
    return np.pi * h ** 3 * rng.uniform(0.5, 1.5, h.size)


def octaves40(seed=1):
    rng = np.random.default_rng(seed)
    n = 1536
    pos = rng.uniform(0.0, 1.0, (n, 3))
    h = 0.5 * 2.0 ** rng.uniform(-40.0, 0.0, n)
    return SearchSet("octaves40", pos, _unit_mass(h, rng), h, seed)


def levels65(seed=2):
    """4 sources in each of 65 half octaves: h = 2^-e {1.0, 1.5}, e = 0 .. 31, and h = 2^-32"""
    rng = np.random.default_rng(seed)
    h = np.repeat(np.array([f * 2.0 ** -e for e in range(33) for f in ((1.0, 1.5) if e < 32 else (1.0,))]), 4)
    pos = rng.uniform(0.0, 1.0, (h.size, 3))
    return SearchSet("levels65", pos, _unit_mass(h, rng), h, seed)


def levels64(seed=2):
    """the first 256 sources of levels65: 64 occupied half octaves"""
    s = levels65(seed)
    s.name = "levels64"
    s.gas = {k: np.ascontiguousarray(v[:256]) for k, v in s.gas.items()}
    s.h = s.gas["h"].copy()
    return s


def far_clusters(seed=3):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 0.3, (256, 3))
    b = rng.normal(0.0, 0.3, (256, 3)) + np.array([1e7, 0.0, 3e6])
    pos = np.concatenate([a, b])
    return SearchSet("far_clusters", pos, rng.uniform(0.5, 1.5, 512) * 1e-3, 0.05, seed)


FACE_LOS = (0.0, -7.3, 1e6 + 0.1)
FACE_H = 0.3
FACE_NODES = 12


def face_edge(h=FACE_H):
    """the kernel's expression of the cell edge of one h"""
    return (2.0 * h) * (1.0 + 1e-6)


def face_lattice(lo=0.0, seed=4):
    """12 x 12 x 12 nodes at lo + n (E / 2) on every axis: every second node plane is a cell face"""
    rng = np.random.default_rng(seed)
    half = face_edge() / 2.0
    ax = lo + np.arange(FACE_NODES) * half
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    pos = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    s = SearchSet(f"face_lattice[{lo:g}]", pos, rng.uniform(0.5, 1.5, pos.shape[0]), FACE_H, seed)
    s.lattice_lo, s.lattice_index = lo, np.stack(np.meshgrid(*(np.arange(FACE_NODES),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return s


HEAP_N = 300


def heap(seed=5):
    """300 particles at one position and 212 within 0.9 h of it: every one of the 512 reaches every other"""
    rng = np.random.default_rng(seed)
    c = np.array([0.3, -0.2, 0.1])
    d = rng.normal(size=(212, 3))
    d *= (0.9 * rng.uniform(0.0, 1.0, 212) ** (1.0 / 3.0) / np.sqrt((d * d).sum(axis=1)))[:, None]
    pos = np.concatenate([np.tile(c, (HEAP_N, 1)), c + d])
    return SearchSet("heap", pos, rng.uniform(0.5, 1.5, 512), 1.0, seed)


def line(seed=6):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0.0, 10.0, 256), np.full(256, 0.25), np.full(256, -0.5)], axis=1)
    return SearchSet("line", pos, rng.uniform(0.5, 1.5, 256), 0.5, seed)


def plane(seed=7):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0.0, 8.0, 256), rng.uniform(0.0, 8.0, 256), np.full(256, 0.125)], axis=1)
    return SearchSet("plane", pos, rng.uniform(0.5, 1.5, 256), 0.5, seed)


OFFSET = (2.0 ** 40, -2.0 ** 33, 2.0 ** 20)


def offset(seed=8):
    """512 sources in a 16-wide box far from the origin; the positions are the float64 sums, as they are uploaded"""
    rng = np.random.default_rng(seed)
    pos = np.array(OFFSET) + rng.uniform(0.0, 16.0, (512, 3))
    return SearchSet("offset", pos, rng.uniform(0.5, 1.5, 512), 1.0, seed)


TINY_NS = (1, 2, 63, 64, 65)


def tiny(n, seed=9):
    """n sources inside one cell: a box of 0.6 < 2 h"""
    rng = np.random.default_rng(seed + n)
    pos = np.array([-1.5, 2.0, 0.5]) + rng.uniform(0.0, 0.6, (n, 3))
    return SearchSet(f"tiny[{n}]", pos, rng.uniform(0.5, 1.5, n), 0.75, seed)


def two_scales(seed=12):
    """The seed is one whose targets all stay clear of the singular threshold: det C / (tr C / 3)^3 outside [1e-7, 1e-5]
    (tests/test_search_sets_cpu.py).  A target at 1.07e-6, as a neighbouring seed has, is a coin toss for the singular count,
    and its solve amplifies the roundings of the sums by the reciprocal of that ratio."""
    rng = np.random.default_rng(seed)
    n = 2048
    pos = rng.uniform(0.0, 1.0, (n, 3))
    small = rng.uniform(0.0, 1.0, n) < 0.6
    h = np.where(small, 0.02, 0.16) * 2.0 ** rng.uniform(-0.2, 0.2, n)
    s = SearchSet("two_scales", pos, rng.uniform(0.5, 1.5, n) / n, h, seed)
    s.small = small
    return s


SAMPLE_SETS = {"octaves40": octaves40, "levels64": levels64, "levels65": levels65, "far_clusters": far_clusters,
               "face_lattice0": lambda: face_lattice(FACE_LOS[0]), "face_lattice1": lambda: face_lattice(FACE_LOS[1]),
               "face_lattice2": lambda: face_lattice(FACE_LOS[2]), "heap": heap, "line": line, "plane": plane,
               "offset": offset, "two_scales": two_scales,
               **{f"tiny{n}": (lambda n=n: tiny(n)) for n in TINY_NS}}
GRADIENT_SETS = {k: SAMPLE_SETS[k] for k in ("far_clusters", "face_lattice0", "face_lattice1", "face_lattice2", "heap", "plane",
                                             "offset", "two_scales", *(f"tiny{n}" for n in TINY_NS))}
# the step loop's cell grid holds at most 2^21 cells of 2 h per axis (SPH_ERR_GRID beyond): far_clusters, whose purpose is an
# axis of more cells than that, cannot pass through sph_density
DENSITY_SETS = ("face_lattice0", "face_lattice1", "face_lattice2", "heap", "offset")
_cache = {}


def get(name):
    """the named set, built once"""
    if name not in _cache:
        _cache[name] = SAMPLE_SETS[name]()
    return _cache[name]


def origins(s):
    """(n, 3) the origin every particle's coordinates are taken from in the test fields: the box's lower corner (per clump
    in far_clusters).  A field of the raw coordinates would carry their rounding, 10^-9 at 10^7, into every difference."""
    pos = s.pos
    o = np.tile(pos.min(axis=0), (s.n, 1))
    if s.name == "far_clusters":
        o[256:] = pos[256:].min(axis=0)
    return o


def value_rows(s):
    """(4, n) smooth bounded functions of the position alone (coincident particles share their values), varying over h"""
    rel = (s.pos - origins(s)) / float(np.median(s.h_all))
    k = np.array([[0.9, 0.3, -0.5], [-0.2, 0.7, 0.6], [0.5, -0.4, 0.8], [0.3, 0.6, 0.2]])
    return np.ascontiguousarray(np.stack([np.sin(rel @ k[0]), np.cos(rel @ k[1]), np.sin(rel @ k[2]) + 2.0, np.cos(rel @ k[3]) - 0.5]))


LINEAR_A = np.array([[0.7, -1.3, 0.4], [-0.25, 0.5, 2.0]])
LINEAR_C = np.array([1.5, -0.75])


def linear_rows(s):
    """(2, n) the fields a . (x - origin) + c: linear around every target, with the gradient a"""
    return np.ascontiguousarray(LINEAR_C[:, None] + LINEAR_A @ (s.pos - origins(s)).T)


SAMPLE_FIELDS = ("vx", "u")                    # the context fields of the sample tests: rows 4 and 5 of sample_rows


def sample_rows(s):
    """(6, n): value_rows, then the context fields SAMPLE_FIELDS"""
    return np.concatenate([value_rows(s), np.stack([s.gas[f] for f in SAMPLE_FIELDS])])


_ref_cache = {}


def sample_reference(name):
    """(points, parts, brute_sample's dict over sample_rows, mass weight) of the named set, computed once and never changed"""
    if ("s", name) not in _ref_cache:
        s = get(name)
        pts, parts = sample_points(s)
        ref = brute_sample(pts, s.pos, s.m, s.h, sample_rows(s))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        pts.setflags(write=False)
        _ref_cache["s", name] = (pts, parts, ref)
    return _ref_cache["s", name]


GRAD_FIELDS = ("vx", "vy", "vz", "u")          # the context fields of the gradient tests: rows 4 .. 7 of gradient_rows


def gradient_rows(s):
    """(8, n): value_rows, then the context fields GRAD_FIELDS"""
    return np.concatenate([value_rows(s), np.stack([s.gas[f] for f in GRAD_FIELDS])])


# ---- the points of sph_sample ---------------------------------------------------------------------------------------------
def far_points(pos, h):
    """the five points of tests/test_sample_gpu.py more than 2 h_max outside the source box: exact zeros"""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = hi - lo
    reach = 2.0 * float(np.max(h))
    return np.array([lo - 1.01 * reach, hi + 1.01 * reach, [lo[0] - 1.5 * reach, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])],
                     [0.5 * (lo[0] + hi[0]), hi[1] + 3.0 * reach, lo[2]], hi + 1e6 * ext + 4.0 * reach])


def sample_points(s, seed=11):
    """(points (M, 3), parts): 512 uniform in the box inflated by 10 % (an axis without extent: by 1.5 h_max instead), every
    source, for 128 sources (all of fewer) the 12 points at 2 h_j (1 -+ 2^-20) along +-x, +-y, +-z (one just reached, one
    just not), for a face lattice the face centres and corners of its cells, five far points, one NaN point.  parts maps
    the names of these groups to index ranges."""
    rng = np.random.default_rng(seed)
    pos, h = s.pos, s.h_all
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    pad = 0.1 * (hi - lo) + np.where(hi > lo, 0.0, 1.5 * h.max())
    groups = [("uniform", rng.uniform(lo - pad, hi + pad, (512, 3))), ("sources", pos.copy())]
    pick = np.sort(rng.choice(s.n, min(128, s.n), replace=False))
    g = []
    for a in range(3):
        for sign in (1.0, -1.0):
            for f in (1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20):
                q = pos[pick].copy()
                q[:, a] += sign * ((2.0 * h[pick]) * f)
                g.append(q)
    groups.append(("grazing", np.concatenate(g)))
    if hasattr(s, "lattice_lo"):
        e = face_edge()
        k = np.arange(FACE_NODES // 2 + 1)
        corner = s.lattice_lo + k * e                              # the walk's expression of a cell's lower face
        centre = 0.5 * (corner[:-1] + corner[1:])
        pts = [np.stack(np.meshgrid(corner, corner, corner, indexing="ij"), axis=-1).reshape(-1, 3)]
        for a in range(3):
            ax = [centre, centre, centre]
            ax[a] = corner
            pts.append(np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3))
        groups.append(("faces", np.concatenate(pts)))
    groups.append(("far", far_points(pos, h)))
    groups.append(("nan", np.array([[0.5 * (lo[0] + hi[0]), np.nan, lo[2]]])))
    parts, at = {}, 0
    for name, p in groups:
        parts[name] = (at, at + p.shape[0])
        at += p.shape[0]
    return np.ascontiguousarray(np.concatenate([p for _, p in groups])), parts


# ---- plan restatements -----------------------------------------------------------------------------------------------------
def _bits_to_double(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def _set_level(H, ext):
    """set_level of csrc/sample.hip: (edge, 1 / edge, cull2, cmax (3), enlarged)"""
    e = (2.0 * H) * (1.0 + 1e-6)
    if not (e > 0.0 and e <= DBL_BIG):
        e = DBL_BIG
    enlarged = False
    for a in range(3):
        if ext[a] / e > LEVEL_AXIS_CELLS:
            e = (ext[a] / LEVEL_AXIS_CELLS) * (1.0 + 1e-6)
            enlarged = True
    ie = 1.0 / e
    with np.errstate(over="ignore"):
        cull2 = float((np.float64(2.0 * H) * np.float64(2.0 * H)) * (1.0 + 1e-5))
    cmax = [int(min(max(np.floor(ext[a] * ie), 0.0), float(LEVEL_AXIS_MASK))) for a in range(3)]
    return {"H": H, "edge": e, "inv_e": ie, "cull2": cull2, "cmax": cmax, "enlarged": enlarged}


def plan_sample(pos, h, g0=1):
    """sample_levels of csrc/sample.hip for the sources pos (n, 3) with h (n,) (per-particle h) or one number.  Returns a
    dict: lo, ext, bins (the occupied quarter octaves), occ (g -> occupied groups, for every g tried), g, nlev, levels (a
    list of dicts H, edge, inv_e, cull2, cmax, enlarged, count), top, level_of (n,): every source's level."""
    pos = np.asarray(pos, dtype=np.float64)
    lo = pos.min(axis=0)
    ext = pos.max(axis=0) - lo
    out = {"lo": lo, "ext": ext}
    if np.ndim(h) == 0:
        lv = _set_level(float(h), ext)
        lv["count"] = pos.shape[0]
        out.update(bins=np.zeros(0, dtype=np.int64), occ={}, g=0, nlev=1, levels=[lv], top=0,
                   level_of=np.zeros(pos.shape[0], dtype=np.int64))
        return out
    h = np.asarray(h, dtype=np.float64)
    assert np.all((h > 0.0) & (h <= DBL_BIG))
    b = (h.view(np.uint64) >> np.uint64(HSHIFT)).astype(np.int64)
    hist = np.bincount(b, minlength=HBINS)
    occ = {}
    g = g0
    while True:
        ng = HBINS >> g
        occ[g] = int(np.count_nonzero(hist.reshape(ng, 1 << g).sum(axis=1)))
        if occ[g] <= MAX_LEVELS:
            break
        g += 1
    grp = hist.reshape(HBINS >> g, 1 << g).sum(axis=1)
    ids = np.nonzero(grp)[0]
    levels = []
    for cb in ids:
        bits = (int(cb) + 1) << (HSHIFT + g)
        lv = _set_level(DBL_BIG if bits >= 0x7ff0000000000000 else _bits_to_double(bits), ext)
        lv["count"] = int(grp[cb])
        levels.append(lv)
    counts = np.array([lv["count"] for lv in levels])
    out.update(bins=np.nonzero(hist)[0], occ=occ, g=g, nlev=len(levels), levels=levels, top=int(np.argmax(counts)),
               level_of=np.searchsorted(ids, b >> g))
    return out


def level_cells(plan, pos):
    """(n, 3) the cell of every source in its own level: level_cell_axis of csrc/cell_table.hpp"""
    c = np.zeros(pos.shape, dtype=np.int64)
    for l, lv in enumerate(plan["levels"]):
        sel = plan["level_of"] == l
        f = np.floor((pos[sel] - plan["lo"]) * lv["inv_e"])
        c[sel] = np.minimum(np.maximum(f, 0.0), np.array(lv["cmax"], dtype=np.float64)).astype(np.int64)
    return c


def plan_gradients(pos, h):
    """grad_box of csrc/gradients.hip for the particles pos (n, 3) (all sources, all targets) with h (n,) or one number.
    Returns a dict: lo, ext, h_ref, edge, inv_e, cmax, enlarged, cell (n, 3), reach (n,), cells (n,): the number of cells
    grad_walk visits for every target, prod(min(2 reach + 1, cmax + 1))."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    lo = pos.min(axis=0)
    ext = pos.max(axis=0) - lo
    if np.ndim(h) == 0:
        h_ref = float(h)
        ht = np.full(n, float(h))
    else:
        ht = np.asarray(h, dtype=np.float64)
        b = np.sort(ht.view(np.uint64) >> np.uint64(HSHIFT))
        h_ref = _bits_to_double((int(b[(n - 1) // 2]) + 1) << HSHIFT)
    e = (2.0 * h_ref) * (1.0 + 1e-6)
    if not (e > 0.0 and e <= DBL_BIG):
        e = 1.0
    enlarged = False
    for a in range(3):
        if ext[a] / e > AXIS_CELLS:
            e = (ext[a] / AXIS_CELLS) * (1.0 + 1e-6)
            enlarged = True
    ie = 1.0 / e
    cmax = np.array([int(min(max(np.floor(ext[a] * ie), 0.0), float(AXIS_MASK))) for a in range(3)], dtype=np.int64)
    cell = np.minimum(np.maximum(np.floor((pos - lo) * ie), 0.0), float(AXIS_MASK)).astype(np.int64)
    reach = np.ceil((2.0 * ht) * ie + 1e-7)
    cells = np.prod(np.minimum(2.0 * reach[:, None] + 1.0, (cmax + 1.0)[None, :]), axis=1)
    return {"lo": lo, "ext": ext, "h_ref": h_ref, "edge": e, "inv_e": ie, "cmax": cmax, "enlarged": enlarged, "cell": cell,
            "reach": reach, "cells": cells}


def below_exact_cell(s):
    """a face lattice's node coordinates (n, 3) whose computed cell floor((p - lo) / E) is below the exact one, n // 2"""
    ie = 1.0 / face_edge()
    c = np.floor((s.pos - s.lattice_lo) * ie).astype(np.int64)
    return c < s.lattice_index // 2


# ---- references --------------------------------------------------------------------------------------------------------
def _w(q):
    """the cubic spline Wn(q) (1 at q = 0, 0 from q = 2) in the argument's precision"""
    t = 2 - q
    return np.where(q <= 1, 1 - q * q * LD(1.5) + q * q * q * LD(0.75), np.where(q <= 2, t * t * t * LD(0.25), LD(0)))


def brute_sample(points, pos, m, h, A=None, rho=None, mask=None, chunk=256):
    """All pairs in long double.  points (M, 3); pos (N, 3), m (N,), h (N,) or a number, A (K, N) or None, rho (N,) for the
    volume weight, mask (N,) the sources (None: all).  Returns a dict: den (M,), num (K, M) (long double; NaN at a
    non-finite point), K (M,) the sources with q <= 2, S (M,) = sum |ws_j| and SA (K, M) = sum |ws_j A_j| over those, counts
    = (points with den != 0, non-finite points)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    N, M = pos.shape[0], points.shape[0]
    A = np.zeros((0, N)) if A is None else np.asarray(A, dtype=np.float64).reshape(-1, N)
    sel = np.arange(N) if mask is None else np.nonzero(mask)[0]
    hl = np.broadcast_to(np.asarray(h, dtype=np.float64), (N,))[sel].astype(LD)
    w = np.asarray(m, dtype=np.float64)[sel].astype(LD)
    if rho is not None:
        w = w / np.asarray(rho, dtype=np.float64)[sel].astype(LD)
    ws = w / (PI_LD * hl * hl * hl)
    wa = ws[None, :] * A[:, sel].astype(LD)
    ps = pos[sel].astype(LD)
    fin = np.isfinite(points).all(axis=1)
    den, num = np.zeros(M, dtype=LD), np.zeros((A.shape[0], M), dtype=LD)
    Kp, S, SA = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=LD), np.zeros((A.shape[0], M), dtype=LD)
    ids = np.nonzero(fin)[0]
    for s in range(0, ids.size, chunk):
        i = ids[s:s + chunk]
        d = points[i].astype(LD)[:, None, :] - ps[None, :, :]
        q = np.sqrt((d * d).sum(axis=2)) / hl[None, :]
        wn = _w(q)
        inside = q <= 2
        den[i] = (wn * ws[None, :]).sum(axis=1)
        Kp[i] = inside.sum(axis=1)
        S[i] = (inside * np.abs(ws)[None, :]).sum(axis=1)
        for k in range(A.shape[0]):
            num[k, i] = (wn * wa[k][None, :]).sum(axis=1)
            SA[k, i] = (inside * np.abs(wa[k])[None, :]).sum(axis=1)
    counts = (int(np.count_nonzero(den[fin] != 0)), int(M - fin.sum()))
    den[~fin] = np.nan
    num[:, ~fin] = np.nan
    return {"den": den, "num": num, "K": Kp, "S": S, "SA": SA, "counts": counts}


def brute_gradients(pos, m, A, h, corrected=True, chunk=128):
    """All pairs in long double, every particle a source and a target with its own h (h (N,) or a number): DESIGN section
    12's rho~ = sigma_i sum m_j Wn, C = sum m_j f x x^T, b_k = sum m_j f (A_i - A_j) x (x = r_i - r_j, the pairs with x = 0
    only in rho~), grad = C^-1 b (corrected) or (sigma_i / h_i^2) b / rho~.  Returns a dict: grad (K, 3, N) float64 (NaN at a
    singular target), rho (N,) float64, ratio (N,) det C / (tr C / 3)^3, singular (N,), K (N,): the sources within 2 h_i."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, N).astype(LD)
    K = A.shape[0]
    hl = np.broadcast_to(np.asarray(h, dtype=np.float64), (N,)).astype(LD)
    ml = np.asarray(m, dtype=np.float64).astype(LD)
    pl = pos.astype(LD)
    grad = np.full((K, 3, N), np.nan)
    rho, ratio = np.zeros(N), np.zeros(N)
    sing = np.zeros(N, dtype=bool)
    reach = np.zeros(N, dtype=np.int64)
    for s in range(0, N, chunk):
        i = np.arange(s, min(s + chunk, N))
        x = pl[i][:, None, :] - pl[None, :, :]
        d2 = (x * x).sum(axis=2)
        hi = hl[i][:, None]
        q = np.sqrt(d2) / hi
        inside = q <= 2
        reach[i] = inside.sum(axis=1)
        sig = 1 / (PI_LD * hl[i] ** 3)
        sw = (ml[None, :] * _w(q)).sum(axis=1)
        rho[i] = (sig * sw).astype(np.float64)
        pair = inside & (d2 != 0)
        qs = np.where(pair, q, LD(1))
        t = 2 - qs
        f = np.where(pair, np.where(qs <= 1, 3 - LD(2.25) * qs, LD(0.75) * t * t / qs), LD(0))
        mf = ml[None, :] * f
        C = np.einsum("tj,tja,tjb->tab", mf, x, x)
        b = np.einsum("tj,ktj,tja->tka", mf, A[:, i][:, :, None] - A[:, None, :], x)
        det = np.array([_det3(c) for c in C], dtype=LD)
        t3 = (C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]) / 3
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio[i] = (det / (t3 * t3 * t3)).astype(np.float64)
        sg = ~(det > LD(1e-6) * t3 * t3 * t3)
        sing[i] = sg
        for r, ti in enumerate(i):
            if corrected:
                if not sg[r]:
                    grad[:, :, ti] = (_adj3(C[r]) @ b[r].T / det[r]).T.astype(np.float64)
            else:
                with np.errstate(invalid="ignore", divide="ignore"):
                    grad[:, :, ti] = (b[r] / (hl[ti] * hl[ti] * sw[r])).astype(np.float64)
    return {"grad": grad, "rho": rho, "ratio": ratio, "singular": sing, "K": reach}


def _adj3(c):
    return np.array([[c[1, 1] * c[2, 2] - c[1, 2] * c[1, 2], c[0, 2] * c[1, 2] - c[0, 1] * c[2, 2], c[0, 1] * c[1, 2] - c[0, 2] * c[1, 1]],
                     [c[0, 2] * c[1, 2] - c[0, 1] * c[2, 2], c[0, 0] * c[2, 2] - c[0, 2] * c[0, 2], c[0, 1] * c[0, 2] - c[0, 0] * c[1, 2]],
                     [c[0, 1] * c[1, 2] - c[0, 2] * c[1, 1], c[0, 1] * c[0, 2] - c[0, 0] * c[1, 2], c[0, 0] * c[1, 1] - c[0, 1] * c[0, 1]]],
                    dtype=LD)


def _det3(c):
    a = _adj3(c)
    return c[0, 0] * a[0, 0] + c[0, 1] * a[0, 1] + c[0, 2] * a[0, 2]


# ---- the sample bound ------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -53


def sample_bounds(ref):
    """(bound of den (M,), bound of num (K, M)): (K_p + 32) 2^-53 times S_p and SA_p.  A sequential sum of K_p terms loses at
    most K_p / 2 ulp of sum |term|; each Wn carries a few ulp of 1 (the error of q times |dWn/dq| <= 1.5, the polynomial's
    roundings) and each ws_j a few ulp of itself: the 32."""
    f = (ref["K"] + 32) * LD(EPS)
    return f * ref["S"], f[None, :] * ref["SA"]


def normalised_bounds(ref):
    """(the reference's num / den (0 where den == 0), its bound (K, M)): the two bounds through the quotient, plus the
    division's own rounding; +inf where the bound of den is not below |den| (the quotient is then not determined)"""
    bd, bn = sample_bounds(ref)
    den, num = ref["den"], ref["num"]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den != 0, num / den, LD(0))
        room = np.abs(den) - bd
        b = np.where(room > 0, (bn + np.abs(r) * bd) / room + LD(EPS) * np.abs(r), LD(np.inf))
    b = np.where((den == 0)[None, :], LD(0), b)
    return r, b
