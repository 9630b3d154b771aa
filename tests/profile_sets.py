"""Particle sets that put sph_profile (summersph_amd/csrc/profile.hip; include/summersph.h, "disc profiles") where a binning
kernel goes wrong (tests/test_profile_sets_cpu.py, tests/test_profile_adversarial_gpu.py): particles exactly ON ring,
sector, z-cut and shell edges and on their representable neighbours, bins whose populations straddle the piece and wavefront
sizes of the sorted reduction, and disc normals on both sides of the frame rule's switch.

Every set is a plain function returning (gas, sinks_or_None, call_kwargs, note): the upload dict in id order, the sinks, the
keyword arguments of Context.profile, and a dict of what the set promises (asserted against tests/profile_ref.py alone in
the CPU test).  The exact sets live in the lab frame (normal = z^, so e1 = x^, e2 = y^) with every particle on a coordinate
axis: X or Y is exactly 0, R = sqrt(x x + 0) = |x| exactly and phi is one of 0, +-pi/2, -pi.  |x| is 0 or far above 1e-150 (a
subnormal x would square to 0).  Their contexts use PARAMS (h = 2, G = 1), so that with m a power of two and integer
velocities every one of the 20 terms is a dyadic rational.

  ring_edge_sets(case)   (a) one particle at every edge[k] of profile_ref.edges and at its two neighbours, m = 1 and
                         alpha_i = 2^i within an upload of at most 50: sum m alpha of a bin is the bitmask of its members
  million_rings()        (b) n_r = 2^20 rings of width 2^-20 from 2^20 on: exact edges, five of them occupied
  sectors(n_phi, cm)     (c) the four axes, both signed zeros of the negative x axis, and the centre itself
  z_cut(z_max)           (d) particles at |z| = Z_CUT and just inside; z_max = 0 and -1 select nothing; z = 1e300
  piece_shapes(n_phi)    (e) one ring per population of POPULATIONS: order-free exact sums, shuffled ids, 500 ghosts;
                         layered=True: the same particles lifted to z = LAYER * (rank in their ring and axis), the only
                         form of the set that a density pass can take (see there)
  auto_shell(which)      (f) SPH_PROFILE_AUTO_NORMAL over the shell [2, 8) with particles at |r'| = 2, 5 and 8
  frame_branch(normal)   (g) the 20 000-particle disc of test_profile_gpu.test_frames turned to normals on both sides of
                         |n^_x| = 0.9"""
from __future__ import annotations

import functools
import math

import numpy as np

import profile_ref

PARAMS = dict(h=2.0, G=1.0)
FIELDS = "x y z vx vy vz u m alpha".split()
MAX_UPLOAD = 50                      # 2^49 is the largest alpha of an upload: every bitmask sum is exact

# the four in-plane axes as (x, y) unit steps, and the sector phi = atan2 puts them in
AXES = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def _gas(n, **cols):
    g = {k: np.zeros(n) for k in FIELDS}
    g["m"] = np.ones(n)
    g["u"] = np.ones(n)
    for k, v in cols.items():
        g[k] = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)), dtype=np.float64).copy()
    return g


def _bitmask(n):
    return 2.0 ** np.arange(n)


def _on_axes(R, axis):
    """x, y of radii R on the axes AXES[axis]"""
    ax = np.array(AXES)[np.asarray(axis) % 4]
    return ax[:, 0] * R, ax[:, 1] * R


def _small_velocities(n, seed):
    """non-zero integers in [-3, 3]"""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 4, (3, n)) * rng.choice([-1, 1], (3, n))
    return v.astype(np.float64)


# ---- (a) ring edges ---------------------------------------------------------------------------------------------------
ULP1 = 2.0 ** -52
RING_CASES = {
    "linear":      (10.0, 60.0, 12, False),
    "log":         (10.0, 60.0, 12, True),
    "from_zero":   (0.0, 7.0, 7, False),                      # includes R = 0
    "log_37":      (0.3, 91.7, 37, True),                     # the log() guess is off by one near edges
    "non_dyadic":  (0.1, 0.7, 6, False),
    "four_ulps":   (1.0, 1.0 + 64 * ULP1, 16, False),         # rings four ulps wide
    "one_ulp":     (1.0, 1.0 + 16 * ULP1, 16, False),         # rings one ulp wide
}
ULP_CASES = ("four_ulps", "one_ulp")


def ring_edge_radii(case):
    """the radii of a case in upload order: edge[k] - 1 ulp, edge[k], edge[k] + 1 ulp for every k (no negative and no
    subnormal radius); the ulp cases: every representable R from two below r_min to two above r_max"""
    r0, r1, nr, log = RING_CASES[case]
    e = profile_ref.edges(r0, r1, nr, log)
    if case in ULP_CASES:
        R, stop = [np.nextafter(np.nextafter(r0, -np.inf), -np.inf)], np.nextafter(np.nextafter(r1, np.inf), np.inf)
        while R[-1] < stop:
            R.append(np.nextafter(R[-1], np.inf))
        return np.array(R)
    R = []
    for v in e:
        R += [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)] if v > 0 else [v]
    return np.array(R)


def ring_edge_sets(case):
    """(a): a list of sets, each an upload of at most MAX_UPLOAD particles"""
    r0, r1, nr, log = RING_CASES[case]
    R = ring_edge_radii(case)
    out = []
    for first in range(0, R.size, MAX_UPLOAD):
        r = R[first:first + MAX_UPLOAD]
        n = r.size
        x, y = _on_axes(r, first + np.arange(n))              # the axes in turn: X = 0 or Y = 0, of either sign
        v = _small_velocities(n, 100 + first)
        gas = _gas(n, x=x, y=y, vx=v[0], vy=v[1], vz=v[2], alpha=_bitmask(n))
        kw = dict(r_min=r0, r_max=r1, n_r=nr, log=log)
        out.append((gas, None, kw, dict(case=case, R=r, edges=profile_ref.edges(r0, r1, nr, log))))
    return out


# ---- (b) a million rings ----------------------------------------------------------------------------------------------
MILLION = 1 << 20
MILLION_K = (0, 1, 1 << 19, MILLION - 1, MILLION)


def million_rings():
    r0 = float(MILLION)
    e = r0 + np.array(MILLION_K, dtype=np.float64) / MILLION              # exact: the widths are 2^-20, an ulp is 2^-32
    R = np.stack([np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)], axis=1).reshape(-1)
    n = R.size
    x, y = _on_axes(R, np.arange(n))
    v = _small_velocities(n, 7)
    gas = _gas(n, x=x, y=y, vx=v[0], vy=v[1], vz=v[2], alpha=_bitmask(n))
    # ring of every particle: edge[k] - ulp lies in k - 1 (none for k = 0), edge[k] and edge[k] + ulp in k (none for k = n_r)
    ring = np.stack([np.array(MILLION_K) - 1, MILLION_K, MILLION_K], axis=1).reshape(-1)
    ring[ring >= MILLION] = -1
    kw = dict(r_min=r0, r_max=r0 + 1.0, n_r=MILLION, sums_only=True)
    return gas, None, kw, dict(R=R, ring=ring, occupied=sorted(set(int(k) for k in ring if k >= 0)))


# ---- (c) sectors and the axes -----------------------------------------------------------------------------------------
SECTOR_NPHI = (1, 2, 3, 4, 6, 8, 64)
SECTORS_EXPECTED = {4: [2, 3, 0, 0, 1, 2], 64: [32, 48, 0, 0, 16, 32]}


def sectors(n_phi, central_mass=0.0):
    """+x, +y, the negative x axis with Y = +0.0 (phi = +pi, folded to -pi) and with Y = -0.0 (phi = -pi as it comes: z is
    -0.0 too, or the dot product's last term would turn Y into +0.0), -y, and the centre"""
    x = np.array([5.0, 0.0, -5.0, -5.0, 0.0, 0.0])
    y = np.array([0.0, 5.0, 0.0, -0.0, -5.0, 0.0])
    z = np.array([0.0, 0.0, 0.0, -0.0, 0.0, 0.0])
    v = _small_velocities(6, 11)
    gas = _gas(6, x=x, y=y, z=z, vx=v[0], vy=v[1], vz=v[2], alpha=_bitmask(6))
    kw = dict(r_min=0.0, r_max=10.0, n_r=1, n_phi=n_phi, centre=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), float(central_mass)))
    return gas, None, kw, dict(expected=SECTORS_EXPECTED.get(n_phi), raw_phi=[0.0, math.pi / 2, math.pi, -math.pi, -math.pi / 2, 0.0])


# ---- (d) the z cut ----------------------------------------------------------------------------------------------------
Z_CUT = 1.5
Z_CALLS = (Z_CUT, 0.0, -1.0, np.inf)


def z_cut(z_max):
    """R = 5 on the four axes in turn; z = +-Z_CUT (outside: the cut is strict), the neighbours inside, 0, and 1e300"""
    inside = float(np.nextafter(Z_CUT, 0.0))
    z = np.array([Z_CUT, -Z_CUT, inside, -inside, 0.0, -0.0, 1e300])
    n = z.size
    x, y = _on_axes(np.full(n, 5.0), np.arange(n))
    v = _small_velocities(n, 13)
    gas = _gas(n, x=x, y=y, z=z, vx=v[0], vy=v[1], vz=v[2], alpha=_bitmask(n))
    member = {Z_CUT: [2, 3, 4, 5], 0.0: [], -1.0: [], np.inf: list(range(n))}[z_max]
    kw = dict(r_min=0.0, r_max=10.0, n_r=1, z_max=z_max)
    return gas, None, kw, dict(members=member)


# ---- (e) the piece shapes ---------------------------------------------------------------------------------------------
POPULATIONS = (0, 1, 63, 64, 65, 0, 1023, 1024, 1025, 0, 0, 2047, 2048, 2049, 4096, 0, 65535, 65536, 65537, 3)
N_GHOSTS = 500
PIECE_CENTRAL_MASS = 4.0
LAYER = 8.0                          # above 2 h (1 + 1e-6): particles of one ring and axis are no neighbours of each other


@functools.lru_cache(maxsize=None)
def _piece_shapes(layered):
    rng = np.random.default_rng(2024)
    ring = np.repeat(np.arange(len(POPULATIONS)), POPULATIONS)
    n = ring.size
    axis = np.concatenate([np.arange(p) % 4 for p in POPULATIONS]).astype(np.int64)   # member i of a ring on axis i mod 4
    rank = np.concatenate([np.arange(p) // 4 for p in POPULATIONS]).astype(np.float64)
    x, y = _on_axes(ring + 1.0, axis)
    cols = dict(x=x, y=y, z=LAYER * rank if layered else np.zeros(n), vx=rng.integers(-3, 4, n), vy=rng.integers(-3, 4, n),
                vz=rng.integers(-3, 4, n), u=rng.integers(1, 5, n), m=np.full(n, 0.5), alpha=rng.integers(0, 2, n))
    perm = rng.permutation(n)                                  # the upload order: ids have nothing to do with the rings
    gx, gy = _on_axes(np.array([r + 1.0 for r in rng.choice(np.nonzero(POPULATIONS)[0], N_GHOSTS)]), rng.integers(0, 4, N_GHOSTS))
    ghosts = dict(x=gx, y=gy, z=-LAYER * (1.0 + np.arange(N_GHOSTS)) if layered else np.zeros(N_GHOSTS),
                  vx=rng.integers(-3, 4, N_GHOSTS), vy=rng.integers(-3, 4, N_GHOSTS), vz=rng.integers(-3, 4, N_GHOSTS),
                  u=rng.integers(1, 5, N_GHOSTS), m=np.full(N_GHOSTS, 0.5), alpha=rng.integers(0, 2, N_GHOSTS))
    gas = {k: np.ascontiguousarray(np.concatenate([np.asarray(cols[k], dtype=np.float64)[perm],
                                                   np.asarray(ghosts[k], dtype=np.float64)])) for k in FIELDS}
    for a in gas.values():
        a.setflags(write=False)
    return gas, ring[perm], axis[perm]


def piece_shapes(n_phi=1, layered=False):
    """Ring k is [k + 1, k + 2) and holds POPULATIONS[k] particles, all at R = k + 1 (on its lower edge), dealt over the four
    axes: with n_phi = 4 the axes are four sectors, which quarters every run and moves every start.  m = 0.5, integer
    velocities in [-3, 3], u in [1, 4], alpha in {0, 1}, h = 2, G = 1, central mass 4: every term is a multiple of 1/8 and the
    sums are exact in any order.  The first n_owned ids are a random permutation of the particles; N_GHOSTS ghost rows at
    occupied radii follow.

    layered=False is the set with z = 0.  Its particles share 80 positions, up to 16 385 at one: any density pass would
    have to list tens of thousands of neighbours per particle.  layered=True is the same set, id by id, with member i of a
    ring lifted to z = LAYER (i // 4) (the ghosts below the plane, one per layer): nobody has more than a few neighbours,
    so this form can be cell-sorted; R, phi, the bins and all the sums but those of z', z' z', l and e are the same.  r' / |r'|
    is then irrational, so 8 e is no integer: the layered form is exact with central mass 0 (e = 0) and its e sums are
    compared in the reduction's shape instead."""
    gas, ring, axis = _piece_shapes(bool(layered))
    n_owned = ring.size
    kw = dict(r_min=1.0, r_max=1.0 + len(POPULATIONS), n_r=len(POPULATIONS), n_phi=n_phi,
              centre=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), PIECE_CENTRAL_MASS))
    sector = np.array([2, 3, 0, 1])[axis]                      # +x: phi = 0, +y: pi/2, -x: -pi, -y: -pi/2
    return gas, None, kw, dict(n_owned=n_owned, ring=ring, bin=ring * n_phi + (sector if n_phi == 4 else 0))


# ---- (f) the AUTO_NORMAL shell ----------------------------------------------------------------------------------------
SHELL = (2.0, 8.0)
SHELL_NORMAL = np.array([0.0, 1.0, 1.0]) / math.sqrt(2.0)


def auto_shell(which="shell"):
    """|r'| = 5 with l = (0, 0, 5); |r'| = 8 exactly (outside) with l = (5000, 0, 0); |r'| = 2 exactly (inside) with
    l = (0, 5, 0).  which: "shell" [2, 8): L = (0, 5, 5); "above_2" (2 + ulp, 8): the third is out, L = (0, 0, 5);
    "through_8" [2, 8 + ulp): the second is in, L = (5000, 5, 5); "only_8" [6, 8): nobody, SPH_ERR_STATE"""
    gas = _gas(3, x=[5.0, 0.0, 0.0], y=[0.0, 8.0, 0.0], z=[0.0, 0.0, 2.0], vx=[0.0, 0.0, 2.5], vy=[1.0, 0.0, 0.0],
               vz=[0.0, 625.0, 0.0], alpha=_bitmask(3))
    lo, hi = {"shell": SHELL, "above_2": (float(np.nextafter(2.0, np.inf)), 8.0),
              "through_8": (2.0, float(np.nextafter(8.0, np.inf))), "only_8": (6.0, 8.0)}[which]
    L = {"shell": (0.0, 5.0, 5.0), "above_2": (0.0, 0.0, 5.0), "through_8": (5000.0, 5.0, 5.0), "only_8": None}[which]
    kw = dict(r_min=lo, r_max=hi, n_r=3, normal="auto")
    return gas, None, kw, dict(L=L)


# ---- (g) both branches of the frame rule ------------------------------------------------------------------------------
FRAME_NORMALS = ((1.0, 0.0, 0.0), (0.91, 0.41, 0.0), (0.89, 0.45, 0.0))       # a = y^, a = y^, a = x^
FRAME_CASE = (10.0, 60.0, 10, 4, False)


def rotation_to(normal):
    """a proper rotation that takes z^ to normal / |normal|"""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    a = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    return np.stack([a, np.cross(n, a), n], axis=1)


@functools.lru_cache(maxsize=None)
def _frame_disc():
    import test_profile_gpu as existing                       # its disc and its transform, as test_frames uses them
    return existing._disc(20000, 17)


def frame_branch(normal):
    """the disc of test_frames turned so that its normal is `normal`; the particles near an edge are dropped as the parity
    tests drop them: this set is about the frame"""
    import test_profile_gpu as existing
    gas, sinks = _frame_disc()
    rot = rotation_to(normal)
    g, s = existing._transform(gas, sinks, rot)
    r0, r1, nr, nphi, log = FRAME_CASE
    centre = (float(s["x"][0]), float(s["y"][0]), float(s["z"][0]))
    g = existing._drop_edges(g, [FRAME_CASE], centre=centre, normal=normal)
    kw = dict(r_min=r0, r_max=r1, n_r=nr, n_phi=nphi, log=log, sink=0, normal=tuple(normal))
    return g, s, kw, dict(rot=rot, a_is_y=abs(normal[0] / np.linalg.norm(normal)) > 0.9)


# ---- the restatement's answer to a set --------------------------------------------------------------------------------
def reference(gas, kw, shape="pieces", n_owned=None, only_bins=None, normal=None, sinks=None):
    """profile_ref.profile_sums of a set's call (PARAMS' h and G), returning (sums, bin per particle)"""
    c, cv, cm = kw.get("centre") or ((0, 0, 0), (0, 0, 0), 0.0)
    if kw.get("sink") is not None:
        k = kw["sink"]
        c, cv, cm = [sinks[a][k] for a in "xyz"], [sinks[a][k] for a in ("vx", "vy", "vz")], sinks["m"][k]
    nrm = kw.get("normal", (0, 0, 1)) if normal is None else normal
    with np.errstate(over="ignore"):
        return profile_ref.profile_sums(gas, PARAMS["h"], PARAMS["G"], kw["r_min"], kw["r_max"], kw["n_r"], kw.get("n_phi", 1),
                                        kw.get("log", False), kw.get("z_max", np.inf), c, cv, cm, nrm, shape=shape,
                                        only_bins=only_bins, n_owned=n_owned)
