"""CPU tests of tests/search_sets.py: every adversarial set has the property it is named for (read from the host
restatements of the device-side plans), no set handed to sph_gradients can make grad_walk spin (the cost cap) or sum more
than 512 terms, and the all-pairs long-double references agree with the float64 restatements the GPU tests of sph_sample
and sph_gradients already trust -- which fixes the bounds of the adversarial GPU tests from the references alone."""
import numpy as np
import pytest

import gradients_ref
import sample_ref
import search_sets as S
from test_gradients_gpu import _cmp

CELLS_PER_TARGET = 1e4         # the cost cap: grad_walk visits every cell of a target's reach
CELLS_IN_ALL = 1e7
TERMS = 512                    # (512 + 16) 2^-53 = 5.9e-14 < the 1e-13 that _cmp holds rho~ to


# ---- the sets' claims --------------------------------------------------------------------------------------------------
def test_octaves40_merges_levels_and_enlarges_half_of_them():
    s = S.get("octaves40")
    assert s.n == 1536 and np.log2(s.h.max() / s.h.min()) > 39.0
    ws = s.m / (np.pi * s.h ** 3)
    assert 0.5 <= ws.min() and ws.max() <= 1.5
    p0, p1 = S.plan_sample(s.pos, s.h, 0), S.plan_sample(s.pos, s.h, 1)
    print("octaves40: occupied groups", p0["occ"], "levels", p1["nlev"], "enlarged", sum(lv["enlarged"] for lv in p1["levels"]),
          "sources in enlarged levels", sum(lv["count"] for lv in p1["levels"] if lv["enlarged"]))
    assert p0["occ"][0] > 64 and p0["g"] == 2                      # merging runs from width 0 too
    assert p1["occ"][1] > 64 and p1["g"] == 2
    assert p1["bins"].size == p0["occ"][0]
    enl = [lv["enlarged"] for lv in p1["levels"]]
    assert sum(enl) >= 10 and len(enl) - sum(enl) >= 10
    assert enl == sorted(enl, reverse=True)                        # the small levels are the enlarged ones
    for lv in p1["levels"]:
        assert max(lv["cmax"]) < (1 << 19) - 8
        assert lv["edge"] >= (2.0 * lv["H"]) * (1.0 + 1e-6)
    # the start widths: each gives a valid plan; from 7 on fewer than 64 groups exist, at 13 the one level is unbounded
    for w, nlev in ((2, 40), (3, 20), (7, 2), (8, 1), (13, 1)):
        p = S.plan_sample(s.pos, s.h, w)
        assert p["g"] == w and p["nlev"] == nlev and (S.HBINS >> w < 64) == (w >= 8)
    p13 = S.plan_sample(s.pos, s.h, 13)
    assert p13["levels"][0]["H"] == S.DBL_BIG and p13["levels"][0]["cull2"] == np.inf and p13["levels"][0]["cmax"] == [0, 0, 0]


def test_levels64_and_levels65_sit_on_either_side_of_the_level_limit():
    a, b = S.get("levels64"), S.get("levels65")
    assert a.n == 256 and b.n == 260
    for k in "xyzm":
        assert np.array_equal(a.gas[k], b.gas[k][:256])
    assert np.array_equal(a.h, b.h[:256]) and np.all(b.h[256:] == 2.0 ** -32)
    pa, pb = S.plan_sample(a.pos, a.h), S.plan_sample(b.pos, b.h)
    assert pa["occ"] == {1: 64} and pa["g"] == 1 and pa["nlev"] == 64            # occ <= 64 holds: no merge
    assert np.array_equal(np.bincount(pa["level_of"]), np.full(64, 4)) and pa["level_of"].max() == 63
    assert pb["occ"][1] == 65 and pb["g"] == 2 and pb["nlev"] == 33              # 65 groups: one merge
    assert any(lv["enlarged"] for lv in pa["levels"]) and not pa["levels"][63]["enlarged"]


def test_far_clusters_enlarges_both_plans():
    s = S.get("far_clusters")
    ps, pg = S.plan_sample(s.pos, s.h), S.plan_gradients(s.pos, s.h)
    assert ps["levels"][0]["enlarged"] and pg["enlarged"]
    assert ps["ext"][0] / S.face_edge(s.h) > S.AXIS_CELLS
    assert max(ps["levels"][0]["cmax"]) <= (1 << 19) - 8 and pg["cmax"].max() <= (1 << 21) - 8
    cs, cg = S.level_cells(ps, s.pos), pg["cell"]
    for c in (cs, cg):                                             # every clump in one cell
        assert len(np.unique(c[:256], axis=0)) == 1 and len(np.unique(c[256:], axis=0)) == 1
    # more cells of 2 h than the step loop's grid can index: sph_density refuses this set (see search_sets.DENSITY_SETS)
    assert "far_clusters" not in S.DENSITY_SETS


@pytest.mark.parametrize("k", range(3))
def test_face_lattice_puts_nodes_below_their_exact_cell(k):
    s = S.get(f"face_lattice{k}")
    assert s.n == 12 ** 3 and s.lattice_lo == S.FACE_LOS[k]
    below = S.below_exact_cell(s)
    per_axis = [np.unique(s.lattice_index[:, a][below[:, a]]) for a in range(3)]
    print(f"{s.name}: node planes in the cell below the exact one, per axis:", [list(v) for v in per_axis])
    assert all(v.size >= 1 for v in per_axis) and all(np.all(v % 2 == 0) for v in per_axis)
    # neighbours at q = 1.000001 inside and 2.000002 outside: nothing ties at q = 2
    r = S.brute_gradients(s.pos, s.m, S.value_rows(s)[:1], s.h)
    inner = np.all((s.lattice_index >= 2) & (s.lattice_index <= 9), axis=1)
    assert np.all(r["K"][inner] == 27)
    d = (s.pos[:, None, 0] - s.pos[None, :12 * 12 * 12:144, 0]) / s.h      # along x: every node plane against every other
    assert not np.any(np.abs(np.abs(d) - 2.0) < 1e-6)


def test_heap_line_plane_offset_tiny():
    s = S.get("heap")
    assert np.all(s.pos[:S.HEAP_N] == s.pos[0]) and len(np.unique(s.pos, axis=0)) == 213
    assert np.all(S.plan_gradients(s.pos, s.h)["cmax"] == 0)
    assert np.all(np.ptp(S.get("line").pos, axis=0)[1:] == 0.0) and np.ptp(S.get("plane").pos, axis=0)[2] == 0.0
    assert S.plan_sample(S.get("line").pos, S.get("line").h)["levels"][0]["cmax"][1:] == [0, 0]
    assert S.plan_sample(S.get("plane").pos, S.get("plane").h)["levels"][0]["cmax"][2] == 0
    o = S.get("offset")
    assert np.all(np.abs(o.pos.min(axis=0) - np.array(S.OFFSET)) < 1.0) and np.all(np.ptp(o.pos, axis=0) < 16.0)
    for n in S.TINY_NS:
        t = S.get(f"tiny{n}")
        assert t.n == n and S.plan_sample(t.pos, t.h)["levels"][0]["cmax"] == [0, 0, 0]


def test_two_scales_cell_edge_follows_the_lower_median():
    s = S.get("two_scales")
    p = S.plan_gradients(s.pos, s.h)
    assert s.small.sum() > s.n // 2 and s.h[s.small].max() <= p["h_ref"] < 0.04
    lo, e = gradients_ref.cell_edge(s.pos, s.h)
    assert e == p["edge"] and np.array_equal(lo, p["lo"]) and not p["enlarged"]
    wide = ~s.small
    assert p["reach"][wide].max() == 8 and np.all(p["cmax"] >= 17)
    assert p["cells"].max() == 17 ** 3 and p["cells"][wide].min() < 17 ** 3      # +-8 cells, clamped by cmax at the borders


def test_sample_points_hold_every_group():
    for name in ("octaves40", "face_lattice1", "tiny1"):
        s = S.get(name)
        pts, parts = S.sample_points(s)
        assert pts.shape[0] <= 5000 and parts["uniform"] == (0, 512) and parts["sources"] == (512, 512 + s.n)
        a, b = parts["grazing"]
        assert b - a == 12 * min(128, s.n)
        assert parts["far"][1] - parts["far"][0] == 5 and np.isnan(pts[parts["nan"][0]]).any()
        assert ("faces" in parts) == name.startswith("face")
        _, _, ref = S.sample_reference(name)
        assert np.all(ref["K"][slice(*parts["far"])] == 0)
        if name == "tiny1":                                        # one just reached, one just not
            assert np.array_equal(ref["K"][a:b], np.tile([1, 0], 6)) and np.all(ref["den"][a:b:2] != 0)


# ---- the caps of sph_gradients -------------------------------------------------------------------------------------------
_brute = {}


def _brute_gradients(name, corrected):
    if (name, corrected) not in _brute:
        s = S.get(name)
        _brute[name, corrected] = S.brute_gradients(s.pos, s.m, S.gradient_rows(s), s.h, corrected=corrected)
    return _brute[name, corrected]


@pytest.mark.parametrize("name", S.GRADIENT_SETS)
def test_cost_cap_of_the_gradient_sets(name):
    """A condition, not a measurement: no GPU test may be handed a set on which grad_walk would spin."""
    s = S.get(name)
    p = S.plan_gradients(s.pos, s.h)
    print(f"{name}: E {p['edge']:.6g} cmax {list(p['cmax'])} cells per target <= {p['cells'].max():.0f}, in all {p['cells'].sum():.3g}")
    assert p["cells"].max() <= CELLS_PER_TARGET and p["cells"].sum() <= CELLS_IN_ALL
    assert _brute_gradients(name, True)["K"].max() <= TERMS
    if name == "heap":
        assert _brute_gradients(name, True)["K"].min() == TERMS


@pytest.mark.parametrize("name", ["face_lattice0", "face_lattice1", "face_lattice2", "two_scales", "far_clusters"])
def test_linear_anchor_sets_are_well_conditioned(name):
    """The corrected form gives a linear field's gradient back within 1e-11 only where the solve does not amplify the sums'
    roundings beyond it: the error is about 2^-53 / ratio (measured on the float64 restatement: 3.2e-12 at 1.4e-5), so the
    sets of that test keep every non-singular target at ratio >= 1e-5, and every singular one below 1e-7, clear of the
    1e-6 threshold whichever way the last bits fall."""
    r = _brute_gradients(name, True)["ratio"]
    with np.errstate(invalid="ignore"):
        assert not np.any((r >= 1e-7) & (r < 1e-5)), np.sort(r[(r >= 1e-7) & (r < 1e-5)])
    assert np.count_nonzero(r >= 1e-5) >= 40


def test_two_scales_cost_is_the_stated_one():
    p = S.plan_gradients(S.get("two_scales").pos, S.get("two_scales").h)
    assert p["cells"].max() == 4913 and 3.0e6 < p["cells"].sum() < 3.6e6


# ---- the references against the restatements ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SAMPLE_SETS)
def test_sample_ref_agrees_with_the_all_pairs_sums(name):
    s = S.get(name)
    pts, parts, ref = S.sample_reference(name)
    out, den, cnt = sample_ref.sample(pts, s.pos, s.m, s.h, S.sample_rows(s))
    bd, bn = S.sample_bounds(ref)
    assert cnt == ref["counts"] and cnt[1] == 1
    fin = np.isfinite(pts).all(axis=1)
    assert np.all(np.isnan(den[~fin])) and np.all(np.isnan(out[:, ~fin]))
    ed, en = np.abs(den[fin] - ref["den"][fin]), np.abs(out[:, fin] - ref["num"][:, fin])
    zero = ref["K"][fin] == 0
    assert np.all(den[fin][zero] == 0.0) and np.all(out[:, fin][:, zero] == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rd = float(np.nanmax(np.where(zero, 0, ed / bd[fin])))
        rn = float(np.nanmax(np.where(zero[None, :] | (bn[:, fin] == 0), 0, en / bn[:, fin])))
    print(f"{name}: M {pts.shape[0]} K_p <= {ref['K'].max()}; float64 restatement at {rd:.3f} (den) {rn:.3f} (num) of the bound")
    assert np.all(ed <= bd[fin]) and np.all(en <= bn[:, fin])


def _cmp_any(g, rg, rho, rrho, ratio):
    """_cmp; where no target has a finite row (every one singular) there is no scale: the NaN patterns and rho~ alone"""
    if np.isfinite(rg).any():
        _cmp(g, rg, rho, rrho, ratio=ratio)
    else:
        assert np.all(np.isnan(g))
        _cmp(np.zeros((1, 1)), np.zeros((1, 1)), rho, rrho)


@pytest.mark.parametrize("corrected", [True, False])
@pytest.mark.parametrize("name", S.GRADIENT_SETS)
def test_gradients_ref_agrees_with_the_all_pairs_sums(name, corrected):
    s = S.get(name)
    b = _brute_gradients(name, corrected)
    inf = {}
    g, rho, nt, ns = gradients_ref.gradients(s.pos, s.m, S.gradient_rows(s), s.h_all, corrected=corrected, info=inf)
    assert nt == s.n and ns == (int(b["singular"].sum()) if corrected else 0)
    _cmp_any(g, b["grad"], rho, b["rho"], b["ratio"] if corrected else None)
