"""GPU tests of sph_render_density and sph_render_field (include/summersph.h) on node grids that stress their binning
(tests/image_sets.py; tests/test_image_sets_cpu.py asserts the path every case takes): many interval batches with empty
ones between, the MAX_CELLS clamp, exact chunk counts of the LDS staging, h over four decades, flat node axes, more
segments than gridDim.y holds, a far offset, and selections that reach nothing.

EVERY node is compared with the extended-precision reference (tests/image_ref.py), each against its own term scale:
    |got_g - ref_g| <= TOL S_g,   S_g = sum_{j : q_gj <= 2} |ws_j A_j|   (A = 1 for the density and the denominator)
with the project's TOL = 1e-12.  Why it holds: a term's absolute error is a few ulp of ws_j |A_j| (W / sigma <= 1), and a
sequential sum of at most 2000 terms (the cases' bound) adds at most 2000 * 2^-53 = 2.2e-13 of S_g.  A column sum adds
its nodes' values in order, so its scale is the sum of their S_g (long_axis' column along x adds 64 particles' terms at
about 51 000 nodes: the worst-case bound of a sequential sum, terms * 2^-53, is then 6e-12 of S and above TOL, the error
of positive terms grows far slower, and the 1e-15 observed is printed).  Nodes with no particle within 2 h (1 + 1e-12) must
be exactly 0.0.  Measured on the MI355X, worst |got - ref| / S over all cases: density 1.1e-15 (columns 1.3e-15), field
render 1.1e-15 (columns 1.4e-15)."""
import functools

import numpy as np
import pytest

from gpu_support import capi, make_context
import image_ref
import image_sets as S

pytestmark = pytest.mark.gpu
TOL = 1e-12
WORST = {}


def _nodes(case):
    pos = S.case_pos(case)
    sel = S.select(pos, case["clip"])
    if case["lo"] is None:
        return (sel,) + tuple(S.render_nodes(case))
    return sel, case["lo"], case["hi"], [S.node_coords(case["lo"][a], case["hi"][a], case["n"][a]) for a in range(3)]


@functools.lru_cache(maxsize=None)
def _mass_ref(name):
    """the mass weight's extended-precision num, den, S_num, S_den and the reached nodes: computed once, never written to"""
    case = S.render_case(name)
    sel, lo, hi, g = _nodes(case)
    pos = S.case_pos(case)
    out = image_ref.render(pos, case["gas"]["m"], S.field_values(pos.shape[0]), S.case_h(case), g, sel)
    for a in out:
        a.setflags(write=False)
    return out


def _seq_sum(grid, axis):
    """the column sums, node by node in increasing index"""
    if grid.shape[axis] > 64:
        return np.take(np.cumsum(grid, axis=axis), -1, axis=axis)
    acc = np.zeros(np.delete(grid.shape, axis))
    for k in range(grid.shape[axis]):
        acc = acc + np.take(grid, k, axis=axis)
    return acc


def _check(got, ref, s, near, what):
    assert got.shape == ref.shape, what
    err = np.abs(got.astype(image_ref.LD) - ref)
    pos = np.asarray(s > 0)
    ratio = float(np.max(err[pos] / s[pos])) if pos.any() else 0.0
    key = what.split(":")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"    {what}: worst |got - ref| / S = {ratio:.2e} over {int(pos.sum())} of {got.size} nodes")
    assert np.all(err <= TOL * s), (what, ratio)
    assert np.all(got[~near] == 0.0), what


def _project(ref, s, near, axis, scale=1.0):
    return ref.sum(axis=axis) * image_ref.LD(scale), s.sum(axis=axis) * image_ref.LD(abs(scale)), near.any(axis=axis)


def _spacing_axis(n, order=(2, 1, 0)):
    return next((a for a in order if n[a] > 1), None)


def _kw(case, lo, hi):
    return dict(bounds=None if case["lo"] is None else (lo, hi), h=case["h"], clip=case["clip"])


@pytest.mark.parametrize("name", S.RENDER_CASES)
def test_density_every_node(capi, name):
    case = S.render_case(name)
    n = case["n"]
    sel, lo, hi, g = _nodes(case)
    _, den, _, s_den, near = _mass_ref(name)
    ctx = make_context(capi, case["gas"], variable=case["variable"])
    kw = _kw(case, lo, hi)
    grid = ctx.render_density(n, **kw)
    if case["lo"] is None:
        assert np.array_equal(ctx.render_bounds[0], lo) and np.array_equal(ctx.render_bounds[1], hi)
    _check(grid, den, s_den, near, f"density 3-D: {name}")
    assert np.array_equal(grid, ctx.render_density(n, **kw))                   # two calls are bitwise equal
    if name.startswith("nothing"):
        assert not grid.any()
    else:
        assert grid.max() > 0
    sp = _spacing_axis(n)
    for axis in range(3):
        proj = ctx.render_density(n, axis=axis, **kw)
        seq = _seq_sum(grid, axis)
        assert np.array_equal(proj, seq), (name, axis)                         # bitwise the sequential sum of the 3-D grid
        _check(proj, *_project(den, s_den, near, axis), f"density column: {name} axis {axis}")
        if axis == sp:
            step = (hi[axis] - lo[axis]) / (n[axis] - 1)
            got = ctx.render_density(n, axis=axis, spacing=True, **kw)
            assert np.array_equal(got, seq * step), (name, axis)
            _check(got, *_project(den, s_den, near, axis, step), f"density column: {name} axis {axis} spacing")
    flat = case.get("flat")
    if flat is not None:
        # every node of the flat axis coincides: its planes are one plane, its column the n-fold sequential addition of it,
        # and SPH_RENDER_SPACING multiplies by a spacing of 0
        plane = np.take(grid, 0, axis=flat)
        acc = np.zeros(plane.shape)
        for k in range(n[flat]):
            assert np.array_equal(np.take(grid, k, axis=flat), plane)
            acc = acc + plane
        assert np.array_equal(ctx.render_density(n, axis=flat, **kw), acc) and acc.max() > 0
        assert not ctx.render_density(n, axis=flat, spacing=True, **kw).any()
    ctx.close()


def _field_case(capi, name, weight):
    case = S.render_case(name)
    sel, lo, hi, g = _nodes(case)
    ctx = make_context(capi, case["gas"], variable=case["variable"])
    a = S.field_values(ctx.n)
    if weight == "mass":
        ref = _mass_ref(name)
    else:
        ctx.density()
        rho, m = ctx.field("rho"), ctx.field("m")
        assert np.array_equal(m, case["gas"]["m"]) and np.all(rho > 0)
        if case["variable"]:
            assert np.array_equal(ctx.field("h"), case["gas"]["h"])
        ref = image_ref.render(S.case_pos(case), m / rho, a, S.case_h(case), g, sel)
    return case, ctx, a, lo, hi, ref


def _field_checks(name, weight, case, ctx, a, lo, hi, ref):
    num, den, s_num, s_den, near = ref
    n = case["n"]
    kw = dict(weight=weight, weight_out=True, **_kw(case, lo, hi))
    got, gw = ctx.render_field(a, n, **kw)
    _check(got, num, s_num, near, f"field {weight} num 3-D: {name}")
    _check(gw, den, s_den, near, f"field {weight} den 3-D: {name}")
    again = ctx.render_field(a, n, **kw)
    assert np.array_equal(got, again[0]) and np.array_equal(gw, again[1])
    if name.startswith("nothing"):
        assert not got.any() and not gw.any()                                  # the image is zeros, and so is weight_out
    else:
        assert np.abs(got).max() > 0 and gw.max() > 0
    axis = _spacing_axis(n, (1, 2, 0))
    step = (hi[axis] - lo[axis]) / (n[axis] - 1)
    col, cw = ctx.render_field(a, n, axis=axis, spacing=True, **kw)
    assert np.array_equal(col, _seq_sum(got, axis) * step) and np.array_equal(cw, _seq_sum(gw, axis) * step)
    _check(col, *_project(num, s_num, near, axis, step), f"field {weight} num column: {name} axis {axis} spacing")
    _check(cw, *_project(den, s_den, near, axis, step), f"field {weight} den column: {name} axis {axis} spacing")
    flat = case.get("flat")
    if flat is not None:
        plane, acc = np.take(got, 0, axis=flat), 0.0
        for k in range(n[flat]):
            acc = acc + plane
        assert np.array_equal(ctx.render_field(a, n, axis=flat, **kw)[0], acc)


@pytest.mark.parametrize("name", S.RENDER_CASES)
def test_field_mass_weight_every_node(capi, name):
    case, ctx, a, lo, hi, ref = _field_case(capi, name, "mass")
    _field_checks(name, "mass", case, ctx, a, lo, hi, ref)
    # the denominator of the mass weight is bitwise the density render
    assert np.array_equal(ctx.render_field(a, case["n"], weight="mass", weight_out=True, **_kw(case, lo, hi))[1],
                          ctx.render_density(case["n"], **_kw(case, lo, hi)))
    ctx.close()


@pytest.mark.parametrize("name", [c for c in S.RENDER_CASES if c != "h_decades"] + ["h_decades"])
def test_field_volume_weight_every_node(capi, name):
    case, ctx, a, lo, hi, ref = _field_case(capi, name, "volume")
    _field_checks(name, "volume", case, ctx, a, lo, hi, ref)
    ctx.close()


def test_offset_is_the_translated_case():
    """offset is coarse moved by (1e7, -3e6, 2e5), particles and nodes together; its reference above is the brute force on
    those translated float64 inputs"""
    a, b = S.render_case("coarse"), S.render_case("offset")
    assert np.array_equal(S.case_pos(b), S.case_pos(a) + np.asarray(S.OFFSET)) and np.array_equal(b["lo"], a["lo"] + np.asarray(S.OFFSET))
    assert np.abs(np.asarray(_mass_ref("offset")[1], dtype=np.float64)).max() > 0


def test_print_worst():
    for k in sorted(WORST):
        print(f"    WORST {k}: {WORST[k]:.2e}")
