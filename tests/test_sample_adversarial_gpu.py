"""GPU tests of sph_sample and sph_trace on the adversarial sets of tests/search_sets.py: merged and enlarged levels, the
level limit from both sides, every start width of SPH_SAMPLE_LEVEL_WIDTH, nodes and points on cell faces, degenerate boxes,
a heap of coincident sources, a set far from the origin, the smallest tables and the point counts around a wavefront and a
block.  tests/test_search_sets_cpu.py asserts that each set reaches its branch.

Bound.  Every point is measured against its own sums, not against the row's maximum (with h over 40 octaves that would
check the points next to the smallest particle only):  |den - den_ref| <= (K_p + 32) 2^-53 S_p  and  |num_k - num_ref| <=
(K_p + 32) 2^-53 SA_p, with K_p the sources that reach the point, S_p = sum |ws_j| and SA_p = sum |ws_j A_j| over them
(search_sets.sample_bounds; the reference is the all-pairs sum in long double).  Normalised outputs: the same two bounds
through the quotient.  A point no source reaches gives exact zeros, a NaN point NaN, and the counts must be the
reference's: a source that grazes a point at q = 2 - 2^-19 adds 2^-59 of its weight, so den != 0 there."""
import numpy as np
import pytest

from gpu_support import capi, make_context
import sample_ref
import search_sets as S
import trace_ref

pytestmark = pytest.mark.gpu


def _ctx(capi, s, density=False):
    return make_context(capi, s.gas, density=density, **s.context_kw())


def _ratio(err, bound):
    """the largest err / bound; err must be 0 where the bound is"""
    assert np.all(err[bound == 0] == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, 0)
    return float(np.max(r)) if r.size else 0.0


def _check(tag, ref, den=None, out=None, rows=(), cnt=None, normalise=False, sub=None):
    """den (M,), out (K, M) of the rows `rows` of the reference's values and the counts against the reference (at its
    points `sub`); prints and returns the largest ratio of error to bound"""
    idx = np.arange(ref["den"].size) if sub is None else np.asarray(sub)
    rden, K = ref["den"][idx], ref["K"][idx]
    bd, bn = S.sample_bounds(ref)
    nan = np.isnan(rden)
    zero = ~nan & (K == 0)
    worst = []
    if den is not None:
        assert np.array_equal(np.isnan(den), nan), tag
        assert np.all(den[zero] == 0.0), tag
        worst.append(_ratio(np.abs(den[~nan] - rden[~nan]), bd[idx][~nan]))
    if out is not None:
        rows = list(rows)
        assert out.shape == (len(rows), idx.size), tag
        if normalise:
            want, bound = S.normalised_bounds(ref)
        else:
            want, bound = ref["num"], bn
        want, bound = want[rows][:, idx], bound[rows][:, idx]
        assert np.array_equal(np.isnan(out), np.broadcast_to(nan, out.shape)), tag
        assert np.all(out[:, zero] == 0.0), tag
        worst.append(_ratio(np.abs(out[:, ~nan] - want[:, ~nan]), bound[:, ~nan]))
    if cnt is not None:
        if sub is None:
            assert cnt == ref["counts"], (tag, cnt, ref["counts"])
        else:
            assert cnt == (int(np.count_nonzero(rden[~nan] != 0)), int(nan.sum())), tag
    w = max(worst) if worst else 0.0
    print(f"    {tag}: largest error / bound {w:.3f}")
    assert w <= 1.0, (tag, w)
    return w


def _all_forms(capi, ctx, tag, pts, ref, vals, fields=S.SAMPLE_FIELDS, field_rows=(4, 5), **kw):
    """the weight alone, K = 1 .. 4 values rows, the context fields and a mix, raw and normalised"""
    V = capi.SAMPLE_VALUES
    den, cnt = ctx.sample(pts, counts=True, **kw)[1:]
    worst = [_check(tag + " den", ref, den=den, cnt=cnt)]
    for normalise in (False, True):
        t = tag + (" norm" if normalise else " raw")
        for k in range(1, 5):
            out, den, cnt = ctx.sample(pts, fields=(V,) * k, values=vals[:k], normalise=normalise, weight_out=True, counts=True, **kw)
            worst.append(_check(f"{t} K={k}", ref, den, out, range(k), cnt, normalise))
        for k in range(1, len(fields) + 1):
            out = ctx.sample(pts, fields=fields[:k], normalise=normalise, **kw)
            worst.append(_check(f"{t} {fields[:k]}", ref, None, out, field_rows[:k], None, normalise))
        out = ctx.sample(pts, fields=(fields[0], V, fields[1], V), values=vals, normalise=normalise, **kw)
        worst.append(_check(f"{t} mix", ref, None, out, (field_rows[0], 1, field_rows[1], 3), None, normalise))
    print(f"{tag}: largest error / bound over all forms {max(worst):.3f}")


@pytest.mark.parametrize("name", S.SAMPLE_SETS)
def test_every_set_mass_weight(capi, name):
    s = S.get(name)
    pts, parts, ref = S.sample_reference(name)
    a, b = parts["grazing"]
    assert np.any(ref["K"][a:b] > 0) and ref["counts"][1] == 1
    ctx = _ctx(capi, s)
    _all_forms(capi, ctx, name, pts, ref, S.value_rows(s))
    ctx.close()


@pytest.mark.parametrize("name", S.DENSITY_SETS)
def test_volume_weight_on_the_fixed_h_sets(capi, name):
    s = S.get(name)
    pts = S.sample_reference(name)[0]
    ctx = _ctx(capi, s, density=True)
    rho = ctx.field("rho")
    assert np.all(rho > 0.0)
    rows = np.concatenate([S.value_rows(s), np.stack([s.gas["vx"], rho])])
    ref = S.brute_sample(pts, s.pos, s.m, s.h, rows, rho=rho)
    _all_forms(capi, ctx, name + " volume", pts, ref, S.value_rows(s), fields=("vx", "rho"), weight="volume")
    ctx.close()


def test_far_clusters_is_outside_the_step_loops_grid(capi):
    """why far_clusters has no volume weight and no state after sph_density: an axis of more than 2^21 cells of 2 h is what
    makes grad_box enlarge its edge, and it is what the step loop's cell grid refuses (SPH_ERR_GRID)"""
    ctx = _ctx(capi, S.get("far_clusters"))
    with pytest.raises(capi.SphError) as e:
        ctx.density()
    assert e.value.status == 6
    assert ctx.sample(S.get("far_clusters").pos[:3], counts=True)[2] == (3, 0)      # the analysis call is untouched by it
    ctx.close()


@pytest.mark.parametrize("width", [0, 1, 2, 3, 7, 8, 13])
@pytest.mark.parametrize("name", ["octaves40", "levels65"])
def test_every_start_width_meets_the_bound(capi, monkeypatch, name, width):
    """sample_build reads SPH_SAMPLE_LEVEL_WIDTH at every call.  The level order differs between widths, so the results are
    not bitwise the same; each must meet the bound."""
    s = S.get(name)
    pts, _, ref = S.sample_reference(name)
    plan = S.plan_sample(s.pos, s.h, width)
    print(f"{name} width {width}: g {plan['g']} levels {plan['nlev']} enlarged {sum(lv['enlarged'] for lv in plan['levels'])}")
    monkeypatch.setenv("SPH_SAMPLE_LEVEL_WIDTH", str(width))
    ctx = _ctx(capi, s)
    V = capi.SAMPLE_VALUES
    vals = S.value_rows(s)
    out, den, cnt = ctx.sample(pts, fields=(V, V), values=vals[:2], weight_out=True, counts=True)
    _check(f"{name} width {width} raw", ref, den, out, (0, 1), cnt)
    out = ctx.sample(pts, fields=("u", V), values=vals[:2], normalise=True)
    _check(f"{name} width {width} norm", ref, None, out, (5, 1), None, True)
    ctx.close()


def test_the_level_limit_from_both_sides(capi):
    """levels64 fills the 64 levels (index 63 in the key), levels65 merges once: the 256 sources they share, sampled at
    their own positions, meet the bound in both"""
    a, b = S.get("levels64"), S.get("levels65")
    pts = np.ascontiguousarray(a.pos)
    V = capi.SAMPLE_VALUES
    for s in (a, b):
        vals = S.value_rows(s)
        ref = S.brute_sample(pts, s.pos, s.m, s.h, vals[:2])
        assert ref["K"].min() >= 1
        ctx = _ctx(capi, s)
        out, den, cnt = ctx.sample(pts, fields=(V, V), values=vals[:2], weight_out=True, counts=True)
        _check(f"{s.name} at the shared sources", ref, den, out, (0, 1), cnt)
        assert cnt == (256, 0)
        ctx.close()


@pytest.mark.parametrize("name", ["tiny65", "heap"])
def test_point_counts_around_a_wavefront_and_a_block(capi, name):
    s = S.get(name)
    pts, _, ref = S.sample_reference(name)
    order = np.random.default_rng(21).permutation(pts.shape[0])
    ctx = _ctx(capi, s)
    V = capi.SAMPLE_VALUES
    vals = S.value_rows(s)
    for m in (1, 63, 64, 65, 255, 256, 257):
        sub = order[:m]
        out, den, cnt = ctx.sample(pts[sub], fields=(V, V, V), values=vals[:3], weight_out=True, counts=True)
        _check(f"{name} M={m}", ref, den, out, (0, 1, 2), cnt, sub=sub)
    ctx.close()


# ---- order rule ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)


@pytest.mark.parametrize("name", ["octaves40", "far_clusters", "face_lattice1"])
def test_order_rule_bitwise(capi, name):
    import torch
    s = S.get(name)
    pts, parts, _ = S.sample_reference(name)
    ctx = _ctx(capi, s)
    kw = {"fields": ("vx", "vy", "vz", "u"), "weight_out": True, "counts": True}
    r0 = ctx.sample(pts, **kw)
    _same(r0[:2], ctx.sample(pts, **kw)[:2])                       # repeated
    perm = np.random.default_rng(4).permutation(pts.shape[0])
    rp = ctx.sample(pts[perm], **kw)                               # any order of the points
    assert np.array_equal(rp[0], r0[0][:, perm], equal_nan=True) and np.array_equal(rp[1], r0[1][perm], equal_nan=True)
    assert rp[2] == r0[2]
    alone = [0, parts["sources"][0] + 7, parts["grazing"][0], parts["grazing"][0] + 1, parts["far"][0], parts["nan"][0]]
    alone += [parts["faces"][0], parts["faces"][1] - 1] if "faces" in parts else []
    for i in alone:                                                # one point alone
        r1 = ctx.sample(pts[i:i + 1], **kw)
        assert np.array_equal(r1[0][:, 0], r0[0][:, i], equal_nan=True) and np.array_equal(r1[1][:1], r0[1][i:i + 1], equal_nan=True)
    dev = torch.device("cuda", 0)
    rd = ctx.sample(torch.from_numpy(np.array(pts)).to(dev), device=True, **kw)     # the device form
    assert rd[2] == r0[2]
    _same(r0[:2], (rd[0].cpu().numpy(), rd[1].cpu().numpy()))
    if name in ("face_lattice1",):                                 # a fresh upload against the state after sph_density
        ctx.density()
        _same(r0[:2], ctx.sample(pts, **kw)[:2])
    ctx.close()


@pytest.mark.parametrize("name", ["octaves40", "far_clusters", "face_lattice1"])
def test_trace_is_bitwise_the_composition_of_samples(capi, name):
    s = S.get(name)
    pos, h = s.pos, s.h_all
    seeds = trace_ref.parity_seeds(pos, h, 31, n=64, n_far=8)
    lo, reach = pos.min(axis=0), 2.0 * h.max()
    seeds[:5] = S.far_points(pos, h)
    seeds[5:8] = lo - reach * np.array([[1.5, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 3.0, 3.0]])
    seeds[40] = [np.nan, seeds[40, 1], seeds[40, 2]]
    V = capi.TRACE_VALUES
    vals = S.value_rows(s)[:3]
    ds = 0.05 * float(np.median(h)) if name != "octaves40" else 0.01

    def sampler(q):
        return ctx.sample(q, fields=(capi.SAMPLE_VALUES,) * 3, values=vals, normalise=True, weight_out=True)

    ctx = _ctx(capi, s)
    for arclength in (False, True):
        got = ctx.trace(seeds, 3, ds, fields=(V, V, V), values=vals, arclength=arclength, counts=True)
        want = trace_ref.trace_with(sampler, seeds, 3, ds, arclength=arclength)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), arclength
        assert np.array_equal(got[0], want[0], equal_nan=True), arclength
        assert got[-1] == tuple(np.bincount(want[1], minlength=5)) and got[1][40] == capi.TRACE_NONFINITE
        assert got[-1] == (55, 8, 0, 0, 1) and np.all(want[1][:8] == capi.TRACE_LEFT_GAS), arclength
    ctx.close()


@pytest.mark.parametrize("k", range(3))
def test_strict_clip_on_a_lattice_plane(capi, k):
    """a clip plane exactly on a node plane excludes that plane's sources; one ulp outside, it includes them"""
    s_name = f"face_lattice{k}"
    s = S.get(s_name)
    pts = S.sample_reference(s_name)[0]
    pos = s.pos
    planes = np.unique(pos[:, 0])
    assert planes.size == S.FACE_NODES
    V = capi.SAMPLE_VALUES
    vals = S.value_rows(s)
    ctx = _ctx(capi, s)
    inf = np.inf
    n_src = []
    for lo_x, hi_y in ((planes[3], planes[8]), (np.nextafter(planes[3], -inf), np.nextafter(planes[8], inf))):
        clip = ((lo_x, -inf, -inf), (inf, hi_y, inf))
        mask = sample_ref.sources_mask(pos, clip=clip)
        n_src.append(int(mask.sum()))
        ref = S.brute_sample(pts, pos, s.m, s.h, vals[:1], mask=mask)
        out, den, cnt = ctx.sample(pts, fields=(V,), values=vals[:1], clip=clip, weight_out=True, counts=True)
        _check(f"{s_name} clip {n_src[-1]} sources", ref, den, out, (0,), cnt)
    assert n_src == [8 * 8 * 12, 9 * 9 * 12]
    ctx.close()
