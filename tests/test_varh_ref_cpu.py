"""CPU: the variable-h oracle (oracle/sph_oracle_v.c through orc_v.OracleV: leaves, density, forces, update_h) against the
brute-force numpy restatement tests/varh_ref.py on the adversarial sets of tests/varh_sets.py -- the first time the oracle
is pinned outside discs -- and the CONSTRUCTION CONDITIONS of those sets: what each was built to contain is asserted here,
so a set that lost its property fails instead of letting tests/test_varh_adversarial_gpu.py pass vacuously.

Bars (the project's own): leaf boxes bitwise; rho and Omega 1e-13 of the element's own value; h after
calc_smoothing 1e-12 per element; rates per element |d| <= 1e-11 |value_i| + 1e-13 S_i with S_i the sum of the magnitudes
of the terms that make up the element (a sum of up to ~1e3 fp64 terms carries a rounding error of up to ~1e3 * 1.1e-16 of
that, whatever is left after cancellation).  Measured between the two references: rho <= 3.9e-15, Omega <= 2.4e-15 (|Omega|
>= 2 on every set: the Newton step is nowhere ill-conditioned), h <= 8.5e-16, rates <= 4e-3 of their bar."""
import numpy as np
import pytest

import varh_ref as VR
import varh_sets as S


_REF = {}


def ref_of(name):
    """(gas, VarhRef in the reference's coincident-point mode, evaluated, with one calc_smoothing pass)"""
    if name not in _REF:
        gas = S.build(name, small=True)
        ref = VR.VarhRef(gas).evaluate()
        ref.update_h()
        _REF[name] = (gas, ref)
    return _REF[name]


def oracle_of(gas):
    from oracle import orc, orc_v
    return orc_v.OracleV(gas, S.NO_SINKS, nthreads=orc.max_threads())


@pytest.mark.parametrize("name", S.ALL)
def test_oracle_vs_brute_force(name):
    gas, ref = ref_of(name)
    o = oracle_of(gas)
    o.leaves()
    assert np.array_equal(o.lc.reshape(-1, 3), ref.lc) and np.array_equal(o.ls, ref.ls)      # bitwise
    assert np.array_equal(o.root, ref.root)
    assert np.array_equal(np.signbit(o.ls), ref.unresolved)
    assert int(ref.unresolved.sum()) == {"coincident": 100, "edge_pairs_v": 2}.get(name, 0)
    if name == "coincident":
        return          # root edge 0: every point unresolved, the reference's sums are empty (0 / 0 from there on)
    ok = ~ref.unresolved                        # (the oracle divides by rho = 0 for an unresolved point, as the reference does)
    o.evaluate()
    assert np.all(ref.rho[ok] > 0.0)
    assert np.max(np.abs(o.rho - ref.rho)[ok] / ref.rho[ok]) <= 1e-13
    assert np.max(np.abs(o.omega - ref.omega)[ok] / np.abs(ref.omega[ok])) <= 1e-13
    a_o, a_r = np.stack([o.ax, o.ay, o.az]), np.stack([ref.ax, ref.ay, ref.az])
    ex = VR.rate_excess(np.linalg.norm(a_o - a_r, axis=0), np.linalg.norm(a_r, axis=0), ref.a_scale)
    assert np.max(ex[ok]) <= 1.0, ("a", np.max(ex[ok]))
    for f, sc in (("du", ref.du_scale), ("dalpha", ref.dalpha_scale)):
        ex = VR.rate_excess(np.abs(getattr(o, f) - getattr(ref, f)), np.abs(getattr(ref, f)), sc)
        assert np.max(ex[ok]) <= 1.0, (f, np.max(ex[ok]))
    o.update_h()
    assert np.max(np.abs(o.h - ref.h_new)[ok] / ref.h_new[ok]) <= 1e-12
    assert np.max(np.abs(o.rho - ref.rho_new)[ok] / ref.rho_new[ok]) <= 1e-12        # calc_smoothing leaves its last trial's rho


def test_kernel_mode_differs_only_at_coincident_points():
    """tests/varh_ref.py's two coincident-point modes: on edge_pairs_v (one coincident pair) they give different sums for
    the pair itself and for whoever reaches it, the same sums for everyone else; without coincident points, the same sets"""
    gas, ref = ref_of("edge_pairs_v")
    ker = VR.VarhRef(gas, coincident="kernel").evaluate()
    twins = np.flatnonzero(ref.unresolved)
    assert twins.size == 2
    w0 = ker.w[0] / (VR.KERNEL_PI * ker.h[twins] ** 3)
    assert np.all(ker.rho[twins] >= (gas["m"][twins].sum()) * w0 * (1 - 1e-15))         # self and twin, both with W(0)
    assert np.all(np.isfinite(ker.ax)) and np.all(np.isfinite(ker.du)) and np.all(np.isfinite(ker.omega))
    sees = ker.reach[:, twins].any(axis=1)
    same = ~sees
    same[twins] = False
    assert same.sum() > 2000
    assert np.array_equal(ker.rho[same], ref.rho[same])
    gas2, ref2 = ref_of("ragged65")
    ker2 = VR.VarhRef(gas2, coincident="kernel")
    assert np.array_equal(ker2.in_D, ref2.in_D) and np.array_equal(ker2.in_F, ref2.in_F)


# ---- construction conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [True, False])
@pytest.mark.parametrize("variant", ["corner", "x_only", "low"])
def test_far_clump_lies_outside_a_trimmed_dense_grid(variant, small):
    """the replay of grid_rebuild's trim: the exact box needs more cells than a dense table may have and fewer than the
    2^27 where a variable-h context goes hashed; after the trim at least 32 clump particles lie outside the box, each
    with at least 8 members of its density set outside too"""
    gas, is_clump = S.far_clump(variant, n_disc=2900, n_clump=40) if small else S.far_clump(variant)
    n = gas["x"].size
    box = S.grid_box_replay(gas)
    assert box["limit"] < box["exact_cells"] < 2.0 ** 27
    assert box["rounds"] >= 1 and box["cells"] <= box["limit"] and box["cells"] < 64 * n + 4_100_000
    out = box["outside"] & is_clump
    assert out.sum() >= 32
    o = oracle_of(gas)
    o.leaves()
    assert np.all(o.ls > 0.0)
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    lc = o.lc.reshape(-1, 3)
    lim = VR.reach_limit(gas["h"], o.ls)
    for i in np.flatnonzero(out):
        reach = np.all(np.abs(pos[i][None, :] - lc) < lim[:, None], axis=1)
        r = np.linalg.norm(pos - pos[i], axis=1)
        D = reach & (r <= 2.0 * gas["h"][i])
        D[i] = False
        assert np.count_nonzero(D & box["outside"]) >= 8, i
    side = {"corner": pos[out] > box["hi"], "low": pos[out] < box["lo"],
            "x_only": (pos[out] > box["hi"]) == np.array([True, False, False])}[variant]
    assert np.all(side)


def test_far_clump_fixed_twin_lies_outside_a_trimmed_grid():
    gas, sinks, is_clump = S.far_clump_fixed()
    box = S.grid_box_replay(gas, h_fixed=2.5)
    assert box["exact_cells"] > box["limit"] and box["cells"] <= box["limit"]
    out = box["outside"] & is_clump
    assert out.sum() >= 32
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    for i in np.flatnonzero(out):
        r = np.linalg.norm(pos - pos[i], axis=1)
        assert np.count_nonzero((r <= 5.0) & box["outside"]) - 1 >= 8, i


def test_clump_in_halo_has_one_sided_pairs_that_the_numbering_decides():
    gas, ref = ref_of("clump_in_halo")
    assert ref.n_support_no_reach >= 200         # r <= 2 h_i and i's walk does not reach j's small leaf
    assert ref.n_asym_pairs >= 200               # force pairs in support whose reach is one-sided
    for order in ("reversed", "random"):
        g2, perm = S.clump_in_halo(order)
        ref2 = VR.VarhRef(g2)
        # the same particles under another numbering: slot s of the permuted set is particle perm[s]
        renum = VR.VarhRef(gas, number=np.argsort(perm))
        assert np.array_equal(ref2.in_F, renum.in_F[np.ix_(perm, perm)])
        assert np.array_equal(ref2.in_D, ref.in_D[np.ix_(perm, perm)])          # the density sets do not depend on it
        flipped = np.count_nonzero(renum.in_F != ref.in_F) // 2
        assert flipped >= 50, (order, flipped)
        if order == "reversed":
            assert flipped == ref.n_asym_pairs   # every one-sided pair changes side


def test_h_routes_populates_every_route_and_clause():
    _, ref = ref_of("h_routes")
    counts = {k: int(v.sum()) for k, v in VR.route_classes(ref.h_record).items()}
    assert set(counts) == {"no_reeval", "list_route", "cell_walk_route", "kept_max", "kept_min", "left_cap"}
    assert all(v >= 20 for v in counts.values()), counts


@pytest.mark.parametrize("name", ["lattice17", "lattice33", "lattice_ties"])
@pytest.mark.parametrize("small", [True, False])
def test_lattice_points_lie_on_split_planes(name, small):
    gas = S.build(name, small=small)
    assert np.count_nonzero(S.on_split_plane(gas, levels=4)) >= 100


def test_lattice_ties_has_exact_reach_ties_inside_the_kernel_support():
    """lattice_ties: >= 100 ordered pairs with max_k |x_i - c_j| == 2 h_j + e_j / 2 to the bit and r < 0.9 * 2 h_i -- a reach
    test with '<=' would add a weighty term to rho_i"""
    _, ref = ref_of("lattice_ties")
    lim = VR.reach_limit(ref.h, ref.ls)
    dmax = np.zeros((ref.n, ref.n))
    for a in range(3):
        dmax = np.maximum(dmax, np.abs(ref.pos[:, a][:, None] - ref.lc[:, a][None, :]))
    tie = dmax == lim[None, :]
    assert not np.any(tie & ref.reach)
    assert np.count_nonzero(tie & (ref.r < 0.9 * 2.0 * ref.h[:, None])) >= 100


def test_edge_pairs_compare_to_the_support_as_meant():
    gas, ref = ref_of("edge_pairs_v")
    _, pairs = S.edge_pairs_v()
    h = ref.h
    for kind, (a, b) in pairs.items():
        r = ref.r[a, b]
        assert r == ref.r[b, a] == abs(gas["x"][b] - gas["x"][a])
        assert h[a] != h[b]
        hh = h[a] if kind.endswith("hi") else h[b]
        if kind.startswith("at_"):
            assert r == 2.0 * hh and r / hh == 2.0
        elif kind.startswith("ulp_in"):
            assert r < 2.0 * hh and np.nextafter(r, np.inf) == 2.0 * hh
        elif kind.startswith("ulp_out"):
            assert r > 2.0 * hh and np.nextafter(r, 0.0) == 2.0 * hh
        elif kind.startswith("in_"):
            assert 0.0 < 1.0 - r / (2.0 * hh) < 2e-9
        elif kind.startswith("out_"):
            assert 0.0 < r / (2.0 * hh) - 1.0 < 2e-9
        else:
            assert r == 0.0 and ref.unresolved[a] and ref.unresolved[b]


COUNT_SETS = [n for n in S.ALL if n not in S.HAS_TIES and n not in S.HAS_COINCIDENT]


@pytest.mark.parametrize("name", COUNT_SETS)
def test_count_sets_have_no_pair_near_an_edge(name):
    """the sets on which the GPU test compares list COUNTS exactly: no pair within relative 1e-11 of a support edge
    (r = 2 h_i or 2 h_j) or of a reach boundary, so that no rounding of r^2, 4 h^2 (1 + 1e-12) or the box test decides
    a membership.  (edge_pairs_v and lattice_ties have such pairs on purpose and are not counted.)"""
    _, ref = ref_of(name)
    support, reach_b = VR.edge_margins(ref)
    assert support > 1e-11 and reach_b > 1e-11, (support, reach_b)


def test_list_regrow_outgrows_the_initial_capacity_from_both_ends():
    _, ref = ref_of("list_regrow_v")
    df, shell = S.margin_counts(ref)
    assert df.max() > 96 and shell.max() > 96
    assert np.count_nonzero((df > 96) & (shell > 96)) >= 64         # a whole wave's worth of columns grow from both ends
