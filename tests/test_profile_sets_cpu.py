"""CPU tests of tests/profile_sets.py and of profile_ref.piece_sum: every set is what its docstring promises, by the numpy
restatement (tests/profile_ref.py) alone, so that tests/test_profile_adversarial_gpu.py cannot hide behind a bad input --
strictly increasing edge tables, sqrt(x x) == |x| for every uploaded radius, particles exactly on the edges and on their
representable neighbours, the expected sectors of the axes, the populations of the piece-shape set and its exactness under
any order, and the normals on both sides of the frame rule's switch."""
import math

import numpy as np
import pytest

import profile_ref
import profile_sets as S


def _frame(gas, kw, normal=(0, 0, 1)):
    pos = np.stack([gas[k] for k in "xyz"], axis=1)
    vel = np.stack([gas[k] for k in ("vx", "vy", "vz")], axis=1)
    return profile_ref.frame(pos, vel, np.zeros(3), np.zeros(3), normal)


def _on_an_axis(gas):
    return np.all((gas["x"] == 0) | (gas["y"] == 0))


def _radius_is_exact(gas, fr):
    r = np.maximum(np.abs(gas["x"]), np.abs(gas["y"]))
    assert np.all((r == 0) | (r > 1e-150))
    assert np.array_equal(np.sqrt(r * r), r) and np.array_equal(fr["R"], r)
    return r


def _masks(sums):
    return sums[:, 12]                                          # sum m alpha: with m = 1 and alpha = 2^i the members' bitmask


# ---- (a) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(S.RING_CASES))
def test_ring_edge_sets(case):
    r0, r1, nr, log = S.RING_CASES[case]
    e = profile_ref.edges(r0, r1, nr, log)
    assert e[0] == r0 and e[nr] == r1 and np.all(np.diff(e) > 0)
    sets = S.ring_edge_sets(case)
    R_all = np.concatenate([note["R"] for _, _, _, note in sets])
    # every edge, its neighbour below and its neighbour above are there
    for v in e:
        want = [v] if v == 0 else [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]
        assert np.all(np.isin(want, R_all)), v
    if case in S.ULP_CASES:
        assert np.array_equal(np.diff(R_all) > 0, np.ones(R_all.size - 1, bool))
        assert R_all[2] == r0 and R_all[-3] == r1 and np.all(np.diff(R_all[2:]) == S.ULP1)      # every representable value
    seen = np.zeros(nr, dtype=np.int64)
    for gas, sinks, kw, note in sets:
        n = gas["x"].size
        assert n <= S.MAX_UPLOAD and sinks is None and _on_an_axis(gas)
        assert np.all(gas["m"] == 1.0) and np.array_equal(gas["alpha"], 2.0 ** np.arange(n))
        fr = _frame(gas, kw)
        R = _radius_is_exact(gas, fr)
        assert np.array_equal(R, note["R"])
        sums, b = S.reference(gas, kw)
        k = np.searchsorted(e, R, side="right") - 1              # the rule, against the table
        want = np.where((R >= r0) & (R < r1), k, -1)
        assert np.array_equal(b, want)
        mask = np.zeros(nr)
        for i in np.flatnonzero(want >= 0):
            mask[want[i]] += 2.0 ** i
        assert np.array_equal(_masks(sums), mask)
        seen += np.bincount(want[want >= 0], minlength=nr)
    # every ring holds its lower edge, that edge's upper neighbour and the next edge's lower neighbour (R = 0 has no
    # upper neighbour here); the ulp cases: every value there is
    per_ring = np.full(nr, 1 if case == "one_ulp" else (4 if case == "four_ulps" else 3))
    if r0 == 0:
        per_ring[0] = 2
    assert np.array_equal(seen, per_ring)


# ---- (b) --------------------------------------------------------------------------------------------------------------
def test_million_rings():
    gas, _, kw, note = S.million_rings()
    n_r = kw["n_r"]
    assert n_r == 1 << 20 and kw["sums_only"]
    e = profile_ref.edges(kw["r_min"], kw["r_max"], n_r)
    assert np.all(np.diff(e) == 2.0 ** -20)                      # exact, so strictly increasing
    assert np.array_equal(e[list(S.MILLION_K)], kw["r_min"] + np.array(S.MILLION_K) / n_r)
    fr = _frame(gas, kw)
    R = _radius_is_exact(gas, fr)
    assert _on_an_axis(gas) and np.array_equal(R, note["R"])
    assert np.array_equal(R[1::3], e[list(S.MILLION_K)])
    assert np.array_equal(R[0::3], np.nextafter(R[1::3], -np.inf)) and np.array_equal(R[2::3], np.nextafter(R[1::3], np.inf))
    call = {k: v for k, v in kw.items() if k != "sums_only"}
    sums, b = S.reference(gas, call, only_bins=note["occupied"])
    assert np.array_equal(b, note["ring"])
    assert note["occupied"] == [0, 1, (1 << 19) - 1, 1 << 19, n_r - 2, n_r - 1]
    assert np.array_equal(np.flatnonzero(sums[:, 0]), note["occupied"]) and sums[:, 0].sum() == 12


# ---- (c) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_phi", S.SECTOR_NPHI)
def test_sectors(n_phi):
    gas, _, kw, note = S.sectors(n_phi)
    fr = _frame(gas, kw)
    _radius_is_exact(gas, fr)
    raw = np.arctan2(fr["Y"], fr["X"])
    assert np.array_equal(raw, note["raw_phi"])                # both +pi (to be folded) and -pi reach the bin rule
    assert np.array_equal(np.signbit(fr["Y"][2:4]), [False, True])
    b = profile_ref.bins(fr, kw["r_min"], kw["r_max"], 1, n_phi)
    assert np.all(b >= 0) and b[2] == b[3] == 0 and b[5] == b[0]           # the centre is selected: phi = atan2(0, 0) = 0
    if note["expected"] is not None:
        assert list(b) == note["expected"]
    assert S.SECTORS_EXPECTED[4] == [2, 3, 0, 0, 1, 2] and S.SECTORS_EXPECTED[64] == [32, 48, 0, 0, 16, 32]
    if n_phi & (n_phi - 1) == 0 and n_phi >= 4:                 # 0 and +-pi/2 are sector edges: the upper sector has them
        pe = np.array([-math.pi + (2.0 * math.pi * j) / n_phi for j in range(n_phi)])
        assert np.all(np.isin([0.0, math.pi / 2, -math.pi / 2], pe))
    for cm in (0.0, 4.0):
        g, _, k2, _ = S.sectors(n_phi, cm)
        sums, b2 = S.reference(g, k2)
        assert np.array_equal(b2, b) and np.all(np.isfinite(sums)) and sums[:, 0].sum() == 6
        assert np.array_equal(sums, S.reference(g, k2, shape="sequential")[0])      # integers and quarters: exact
        assert np.any(sums[:, 17:] != 0) == (cm > 0)
    # the centre particle alone: finite, v_R = v_phi = 0, e = 0 (its l and w vanish, r' / |r'| = 0)
    one = {k: v[5:] for k, v in gas.items()}
    s1, _ = S.reference(one, S.sectors(1, 4.0)[2])
    assert np.all(gas["vx"] != 0) and np.all(gas["vy"] != 0) and np.all(gas["vz"] != 0)
    assert s1[0, 0] == 1 and np.all(s1[0, [2, 5, 6, 8, 9, 14, 15, 16, 17, 18, 19]] == 0) and s1[0, 7] == gas["vz"][5]


# ---- (d) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_max", S.Z_CALLS)
def test_z_cut(z_max):
    gas, _, kw, note = S.z_cut(z_max)
    fr = _frame(gas, kw)
    _radius_is_exact(gas, fr)
    assert np.array_equal(fr["Z"], gas["z"])
    inside = np.nextafter(S.Z_CUT, 0.0)
    assert list(gas["z"][:4]) == [S.Z_CUT, -S.Z_CUT, inside, -inside] and gas["z"][6] == 1e300
    sums, b = S.reference(gas, kw)
    assert list(np.flatnonzero(b >= 0)) == note["members"]
    assert _masks(sums)[0] == sum(2.0 ** i for i in note["members"])
    if z_max <= 0:
        assert np.all(sums == 0)
        t = profile_ref.finish(sums, 0.0, 10.0, 1, 1, False, (0, 0, 1), 5.0 / 3.0, 2.0 / 3.0, 1.0)
        c = {n: i for i, n in enumerate(profile_ref.COLUMNS)}
        zero = [c[n] for n in ("N", "M", "Sigma")]
        assert np.all(t[0, zero] == 0) and np.all(np.isnan(t[0, [c["R_mean"], c["H"], c["Omega"], c["kappa"], c["Q"], c["peri"]]]))
    if z_max == np.inf:
        assert sums[0, 4] == np.inf and not np.any(np.isnan(sums))           # m z' z' of z' = 1e300 overflows, nothing else


# ---- (e) --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pieces():
    out = {}
    for layered in (False, True):
        gas, _, kw, note = S.piece_shapes(1, layered)
        if layered:
            kw = dict(kw, centre=((0, 0, 0), (0, 0, 0), 0.0))
        fr = _frame(gas, kw)
        q = profile_ref.moments(fr, gas["m"], gas["u"], gas["alpha"], S.PARAMS["h"], S.PARAMS["G"], kw["centre"][2])
        out[layered] = (gas, kw, note, fr, q)
    return out


@pytest.mark.parametrize("layered", [False, True])
def test_piece_shapes_populations_and_ghosts(pieces, layered):
    gas, kw, note, fr, q = pieces[layered]
    n, n_owned = gas["x"].size, note["n_owned"]
    assert n_owned == sum(S.POPULATIONS) == 210116 and n == n_owned + S.N_GHOSTS
    assert S.POPULATIONS == (0, 1, 63, 64, 65, 0, 1023, 1024, 1025, 0, 0, 2047, 2048, 2049, 4096, 0, 65535, 65536, 65537, 3)
    R = _radius_is_exact(gas, fr)
    assert _on_an_axis(gas)
    e = profile_ref.edges(kw["r_min"], kw["r_max"], kw["n_r"])
    assert np.array_equal(e, np.arange(1.0, 22.0)) and np.all(np.isin(R, e[:-1]))          # everybody on a lower edge
    for n_phi in (1, 4):
        g2, _, k2, note2 = S.piece_shapes(n_phi, layered)
        b = profile_ref.bins(fr, k2["r_min"], k2["r_max"], k2["n_r"], n_phi)
        assert np.array_equal(b[:n_owned], note2["bin"])
        cnt = np.bincount(b[:n_owned], minlength=20 * n_phi).reshape(20, n_phi)
        assert tuple(cnt.sum(axis=1)) == S.POPULATIONS
        if n_phi == 4:                                           # the axes quarter the runs: sector 2 (+x) takes the odd one
            assert np.all(cnt.max(axis=1) - cnt.min(axis=1) <= 1) and cnt[18].tolist() == [16384, 16384, 16385, 16384]
    # the upload order is shuffled: the rings' members are spread over the ids
    assert not np.all(np.diff(note["ring"]) >= 0) and abs(np.corrcoef(np.arange(n_owned), note["ring"])[0, 1]) < 0.01
    # the ghosts sit at occupied radii and would be counted if they were owned
    gb = profile_ref.bins(fr, kw["r_min"], kw["r_max"], kw["n_r"], 1)[n_owned:]
    assert np.all(gb >= 0) and np.all(np.array(S.POPULATIONS)[gb] > 0)
    if layered:                                                  # no two rows share a position; same ring and axis: LAYER apart
        pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
        assert np.unique(pos, axis=0).shape[0] == n and S.LAYER > 2.0 * S.PARAMS["h"] * (1.0 + 1e-6)
        flat = S.piece_shapes(1, False)[0]
        assert all(np.array_equal(gas[k], flat[k]) for k in S.FIELDS if k != "z")
    else:
        assert np.all(gas["z"] == 0)


@pytest.mark.parametrize("layered", [False, True])
def test_piece_shapes_are_exact_in_any_order(pieces, layered):
    gas, kw, note, fr, q = pieces[layered]
    n_owned = note["n_owned"]
    assert np.array_equal(q * 8.0, np.round(q * 8.0))                       # every term a multiple of 1/8
    seq, b = S.reference(gas, kw, shape="sequential", n_owned=n_owned)
    # and no partial sum of any order can leave the 53 bits: 8 sum |term| < 2^53 (flat: the largest |sum| is 65537 (0.5 * 19))
    assert np.array_equal(seq * 8.0, np.round(seq * 8.0)) and np.abs(q[:n_owned]).sum(axis=0).max() * 8.0 < 2.0 ** 53
    assert layered or np.max(np.abs(seq)) == 65537 * (0.5 * 19.0)
    assert np.array_equal(seq[:, 0], S.POPULATIONS) and np.array_equal(seq[:, 1], 0.5 * np.array(S.POPULATIONS))
    # under a random permutation of the ids
    perm = np.random.default_rng(5).permutation(n_owned)
    shuffled = {k: v[:n_owned][perm] for k, v in gas.items()}
    assert np.array_equal(S.reference(shuffled, kw, shape="sequential")[0], seq)
    # in the library's shape
    assert np.array_equal(S.reference(gas, kw, shape="pieces", n_owned=n_owned)[0], seq)
    for n_phi in (4,):
        k4 = dict(kw, n_phi=n_phi)
        s4 = S.reference(gas, k4, shape="pieces", n_owned=n_owned)[0]
        assert np.array_equal(s4, S.reference(gas, k4, shape="sequential", n_owned=n_owned)[0])
        assert np.array_equal(s4.reshape(20, 4, -1).sum(axis=1), seq)
    if not layered:
        assert np.any(seq[:, 17:] != 0)                                     # the eccentricity sums are live
    else:
        assert np.any(seq[:, 3] != 0) and np.all(seq[:, 17:] == 0)


def test_piece_sum_shape():
    rng = np.random.default_rng(1)
    # lane l's own sum first, then the butterfly: three terms are added as (t0 + t2) + t1, not t0 + t1 + t2
    q = np.zeros((3, 20)); q[:, 1] = [1.0, 2.0 ** -53, 2.0 ** -53]
    assert profile_ref.piece_sum(q)[1] == 1.0 and np.add.accumulate(q, axis=0)[-1][1] == 1.0
    q[:, 1] = [2.0 ** -53, 1.0, 2.0 ** -53]
    assert profile_ref.piece_sum(q)[1] == 1.0 + 2.0 ** -52                 # (t0 + t2) + t1
    assert np.add.accumulate(q, axis=0)[-1][1] == 1.0                      # (t0 + t1) + t2: t0 + t1 ties to even
    # position 64 goes to lane 0 (1 + t ties to 1 before lane 1's t arrives); 65 goes to lane 1 (t + t first)
    tiny = 2.0 ** -53
    q = np.zeros((66, 20)); q[0, 1] = 1.0; q[64, 1] = tiny; q[1, 1] = tiny
    assert profile_ref.piece_sum(q)[1] == 1.0
    q = np.zeros((66, 20)); q[0, 1] = 1.0; q[65, 1] = tiny; q[1, 1] = tiny
    assert profile_ref.piece_sum(q)[1] == 1.0 + 2.0 ** -52
    # positions 1024 and 1025 are a piece of their own: added to each other before the first piece's 1
    q = np.zeros((1026, 20)); q[0, 1] = 1.0; q[1024:, 1] = tiny
    assert profile_ref.piece_sum(q)[1] == 1.0 + 2.0 ** -52 and np.add.accumulate(q, axis=0)[-1][1] == 1.0
    q = np.zeros((1026, 20)); q[0, 1] = 1.0; q[[1, 33], 1] = tiny            # lanes 1 and 33 meet in the butterfly's first round
    assert profile_ref.piece_sum(q)[1] == 1.0 + 2.0 ** -52
    q = np.zeros((1026, 20)); q[0, 1] = 1.0; q[[2, 3], 1] = tiny             # lanes 2 and 3 only in its last, after lane 0 took each
    assert profile_ref.piece_sum(q)[1] == 1.0
    q = np.zeros((1026, 20)); q[0, 1] = 1.0; q[1023:1025, 1] = tiny          # either side of the piece boundary
    assert profile_ref.piece_sum(q)[1] == 1.0
    assert np.all(profile_ref.piece_sum(np.zeros((0, 20))) == 0)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 70000):
        q = rng.normal(size=(n, 20))
        got, want = profile_ref.piece_sum(q), np.array([math.fsum(q[:, s]) for s in range(20)])
        assert np.max(np.abs(got - want)) <= 1e-13 * np.sum(np.abs(q), axis=0).max()


def test_pieces_agree_with_the_sequential_sum_on_a_disc():
    import test_profile_gpu as existing
    gas, sinks = existing._disc(20000, 5)
    args = (gas, 2.5, 1.0, 10.0, 60.0, 12, 4, False, 2.5, (0, 0, 0), (0, 0, 0), 1.0)
    a, ba = profile_ref.profile_sums(*args)
    b, bb = profile_ref.profile_sums(*args, shape="pieces")
    assert np.array_equal(ba, bb) and np.array_equal(a[:, 0], b[:, 0]) and not np.array_equal(a, b)
    for s in range(1, 20):
        assert existing.rel_err(b[:, s], a[:, s]) <= 1e-12, s


# ---- (f) --------------------------------------------------------------------------------------------------------------
def test_auto_shell():
    for which in ("shell", "above_2", "through_8", "only_8"):
        gas, _, kw, note = S.auto_shell(which)
        r = np.sqrt((gas["x"] * gas["x"] + gas["y"] * gas["y"]) + gas["z"] * gas["z"])
        assert list(r) == [5.0, 8.0, 2.0]
        fr = _frame(gas, kw)
        q = profile_ref.moments(fr, gas["m"], gas["u"], gas["alpha"], 2.0, 1.0, 0.0)
        assert q[:, 14:17].tolist() == [[0, 0, 5], [5000, 0, 0], [0, 5, 0]]
        inside = (r >= kw["r_min"]) & (r < kw["r_max"])
        L = q[inside, 14:17].sum(axis=0)
        assert (note["L"] is None and not inside.any()) or tuple(L) == note["L"]
        assert kw["normal"] == "auto"
    n, _, _ = profile_ref.axes((0.0, 5.0, 5.0))
    assert np.max(np.abs(n - S.SHELL_NORMAL)) <= 4 * np.finfo(float).eps


# ---- (g) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normal", S.FRAME_NORMALS)
def test_frame_branch(normal):
    gas, sinks, kw, note = S.frame_branch(normal)
    n, e1, e2 = profile_ref.axes(normal)
    assert (abs(n[0]) > 0.9) == note["a_is_y"] == (normal != S.FRAME_NORMALS[2])
    a = np.array([0.0, 1.0, 0.0]) if note["a_is_y"] else np.array([1.0, 0.0, 0.0])
    t = a - np.dot(a, n) * n
    assert np.allclose(e1, t / np.linalg.norm(t), atol=1e-15) and np.allclose(e2, np.cross(n, e1), atol=1e-15)
    rot = note["rot"]
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-15) and np.linalg.det(rot) > 0 and np.allclose(rot[:, 2], n, atol=1e-15)
    L = np.sum(gas["m"] * np.cross(np.stack([gas[k] for k in "xyz"], axis=1), np.stack([gas[k] for k in ("vx", "vy", "vz")], axis=1)).T, axis=1)
    assert np.dot(L / np.linalg.norm(L), n) > 0.9999             # the disc's own normal is the one handed over
    centre = tuple(float(sinks[k][0]) for k in "xyz")
    assert not profile_ref.edge_margin(gas, *S.FRAME_CASE, centre=centre, normal=normal).any()
    sums, b = S.reference(gas, kw, shape="sequential", sinks=sinks)
    assert sums[:, 0].sum() > 5000 and np.all(sums[:, 0] > 50)
