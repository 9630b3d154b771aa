"""Plain numpy restatement of the octree path keys (csrc/gravity.hip grav_keys, csrc/accrete.hip acc_keys) and the
adversarial particle sets of tests/test_octree_adversarial_gpu.py.

A particle's key is its path down the reference's pointer octree ([F]:208-217, 190-198): bbox-midpoint root, edge = the
largest extent, child bit set by a STRICT '>' against the node centre (points on a split plane go to the low child),
3 bits per level (x | y << 1 | z << 2), 21 levels = 63 bits."""
from __future__ import annotations

import numpy as np

LEVELS = 21


def root_box(x, y, z):
    """(centre[3], edge) of the reference's root node, [F]:803-808"""
    lo = np.array([np.min(x), np.min(y), np.min(z)])
    hi = np.array([np.max(x), np.max(y), np.max(z)])
    return (hi + lo) / 2.0, float(np.max(hi - lo))


def path_keys(x, y, z, centre=None, size=None):
    """63-bit path keys (uint64), the same floating-point operations as the kernels"""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    if centre is None:
        centre, size = root_box(x, y, z)
    c = [np.full(x.shape, float(centre[a])) for a in range(3)]
    s = float(size)
    key = np.zeros(x.shape, dtype=np.uint64)
    for _ in range(LEVELS):
        b = [p > cc for p, cc in zip((x, y, z), c)]
        ch = b[0].astype(np.uint64) | (b[1].astype(np.uint64) << np.uint64(1)) | (b[2].astype(np.uint64) << np.uint64(2))
        key = (key << np.uint64(3)) | ch
        q = 0.25 * s
        for a in range(3):
            c[a] = c[a] + np.where(b[a], q, -q)
        s = s * 0.5
    return key


def common_levels(a, b):
    """number of leading 3-bit levels two keys share (21 for equal keys)"""
    a = np.asarray(a, dtype=np.uint64); b = np.asarray(b, dtype=np.uint64)
    out = np.full(np.broadcast(a, b).shape, LEVELS, dtype=np.int64)
    for lv in range(LEVELS, 0, -1):
        sh = np.uint64(3 * (LEVELS - lv))
        out = np.where((a >> sh) != (b >> sh), lv - 1, out)
    return out


def octree_node_count(keys):
    """nodes of the reference's octree over these keys, provided no two keys coincide (a node is split while it holds
    more than one particle): the root plus, per level, every distinct prefix whose parent prefix is shared"""
    keys = np.asarray(keys, dtype=np.uint64)
    total = 1
    for lv in range(1, LEVELS + 1):
        par = keys >> np.uint64(3 * (LEVELS - lv + 1))
        cur = keys >> np.uint64(3 * (LEVELS - lv))
        pu, pc = np.unique(par, return_counts=True)
        shared = np.isin(par, pu[pc >= 2])
        total += np.unique(cur[shared]).size
    return total


# ---- adversarial particle sets -----------------------------------------------------------------------------------
def _gas(x, y, z, m):
    n = x.size
    zeros = np.zeros(n)
    # u = v = alpha = 0: pressure and viscosity vanish, the SPH term adds exact zeros, a is the Barnes-Hut term alone
    return {"x": np.ascontiguousarray(x, dtype=np.float64), "y": np.ascontiguousarray(y, dtype=np.float64),
            "z": np.ascontiguousarray(z, dtype=np.float64), "vx": zeros.copy(), "vy": zeros.copy(), "vz": zeros.copy(),
            "u": zeros.copy(), "m": np.ascontiguousarray(m, dtype=np.float64), "alpha": zeros.copy()}


def lattice(k=33, spacing=2.0, origin=0.0, m=2.0 ** -10):
    """k^3 cubic lattice: with k = 2^j + 1 the root edge is a power of two times the spacing, so lattice points lie on
    the split planes of every level down to the spacing"""
    g = origin + spacing * np.arange(k, dtype=np.float64)
    x, y, z = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    return _gas(x, y, z, np.full(x.size, m))


def sheet(k=129, spacing=1.0, m=2.0 ** -10):
    """exactly flat: z = 0 for all, a square lattice in the plane (split planes again)"""
    g = spacing * np.arange(k, dtype=np.float64)
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    return _gas(x, y, np.zeros(x.size), np.full(x.size, m))


def line(k=2049, spacing=0.5, m=2.0 ** -10):
    x = spacing * np.arange(k, dtype=np.float64)
    return _gas(x, np.zeros(k), np.zeros(k), np.full(k, m))


def coincident(n=100, m=2.0 ** -8):
    """root edge 0: every path key is 0"""
    return _gas(np.full(n, 3.25), np.full(n, -1.5), np.full(n, 7.0), np.full(n, m))


def plummer(n=20000, a=30.0, r_max=300.0, n_heavy=8, seed=11):
    """Plummer sphere (central over edge density ~1e5) with a few particles 1000x heavier than the rest"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, n)
    r = a / np.sqrt(u ** (-2.0 / 3.0) - 1.0)
    while np.any(r > r_max):
        bad = r > r_max
        r[bad] = a / np.sqrt(rng.uniform(0.0, 1.0, bad.sum()) ** (-2.0 / 3.0) - 1.0)
    mu = rng.uniform(-1.0, 1.0, n)
    ph = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - mu * mu)
    m = np.full(n, 1.0e-5)
    m[rng.choice(n, n_heavy, replace=False)] = 1.0e-2
    return _gas(r * s * np.cos(ph), r * s * np.sin(ph), r * mu, m)


def sparse_cube(n=20000, edge=4000.0, seed=12):
    """<< 1 particle per cell: 64 consecutive cell-sorted targets span the box and walk very different trees"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-edge / 2, edge / 2, (3, n))
    return _gas(p[0], p[1], p[2], rng.uniform(0.5e-3, 2.0e-3, n))


def two_clusters(n=6000, sep=1.0e4, radius=20.0, seed=13):
    """two balls ~1e4 apart (hashed cell table); the wave at the boundary between them holds targets of both"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(3, n))
    v *= radius * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=0)
    v[0, n // 2:] += sep
    v[1, n // 2:] += 0.3 * sep
    return _gas(v[0], v[1], v[2], np.full(n, 1.0e-3))


def level21_centres(x, y, z, centre, size):
    """centres of the particles' level-21 boxes (the boxes a 63-bit key names)"""
    c = [np.full(np.shape(x), float(centre[a])) for a in range(3)]
    s = float(size)
    for _ in range(LEVELS):
        q = 0.25 * s
        for a, p in enumerate((x, y, z)):
            c[a] = c[a] + np.where(p > c[a], q, -q)
        s = s * 0.5
    return np.stack(c)


def shared_keys(n=3000, edge=1000.0, n_pairs=40, n_straddle=8, seed=14):
    """a uniform cloud (root edge ~1000, far below 0.025 * 2^21, where the level-21 truncation cannot change gravity)
    with planted pairs and a triple closer than edge / 2^21 that share their 63-bit path keys (the partner sits between
    the particle and the centre of its level-21 box), and pairs as close that straddle a level-21 box face (keys differ)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-edge / 2, edge / 2, (3, n))
    c, s = root_box(*p)
    inner = np.flatnonzero(np.all(np.abs(p) < 0.45 * edge, axis=0))
    pick = rng.choice(inner, n_pairs + n_straddle, replace=False)
    cc = level21_centres(*p[:, pick], c, s)
    q = p[:, pick]
    twins = q[:, :n_pairs] + 0.5 * (cc[:, :n_pairs] - q[:, :n_pairs])
    third = q[:, :1] + 0.25 * (cc[:, :1] - q[:, :1])
    # straddling pairs: both 0.1 box edges from the box's upper x face, one on either side
    e21 = s / 2.0 ** LEVELS
    st = cc[:, n_pairs:].copy()
    a, b = st.copy(), st.copy()
    a[0] += 0.4 * e21
    b[0] += 0.6 * e21
    m = rng.uniform(0.5e-3, 2.0e-3, n + n_pairs + 1 + 2 * n_straddle)
    return _gas(*np.concatenate([p, twins, third, a, b], axis=1), m)


def ragged(n, seed=15):
    """n random particles in a small ball: a single partial wave (or a few)"""
    rng = np.random.default_rng(seed + n)
    p = rng.uniform(-6.0, 6.0, (3, n))
    return _gas(p[0], p[1], p[2], rng.uniform(0.5e-3, 2.0e-3, n))


FAMILIES = {
    "lattice33": lattice,
    "sheet": sheet,
    "line": line,
    "coincident": coincident,
    "plummer": plummer,
    "sparse_cube": sparse_cube,
    "two_clusters": two_clusters,
    "shared_keys": shared_keys,
    **{f"ragged{n}": (lambda n=n: ragged(n)) for n in (1, 2, 3, 63, 64, 65, 127, 257)},
}


def own_h(gas, k=32, lo=0.05, hi=10.0):
    """a per-particle smoothing length for the variable-h runs: half the distance to the k-th neighbour, clipped to the
    variable-h defaults' range"""
    from scipy.spatial import cKDTree
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    n = pos.shape[0]
    if n < 2:
        return np.full(n, 2.5)
    d, _ = cKDTree(pos).query(pos, k=min(k, n - 1) + 1)
    return np.clip(0.5 * d[:, -1], lo, hi)
