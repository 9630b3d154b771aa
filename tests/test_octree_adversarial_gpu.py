"""GPU: the Barnes-Hut tree (csrc/gravity.hip: path keys, radix tree, both walks) and the accretion pass (csrc/accrete.hip)
on particle sets built to break them -- points on split planes, degenerate root boxes, strong clustering, shared 63-bit
path keys, lanes of one wave that walk very different trees, partial waves -- against the CPU oracle's explicit octree
(oracle/sph_oracle_grav.c, which recurses to depth 1000 like the reference).

The gas is uploaded with u = v = alpha = 0 and no sinks: pressure, viscosity and sink terms are exact zeros, so the
accelerations forces() leaves are the Barnes-Hut term alone (test_gravity_free_context_is_exactly_zero checks that).
The sets themselves and a numpy restatement of the path keys are in tests/octree_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import capi, make_context, with_variable_h
import octree_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = list(R.FAMILIES)
MODES = ("fixed", "var")
KEY_TIES = {"shared_keys", "coincident"}       # sets with coinciding path keys (their tie order is the slot order)


_CASES = {}


def case(name, mode):
    """(gas, h): fixed h uses the context's h = 2.5 (nq 5000); variable h each particle's own (nq 2500)"""
    if name not in _CASES:
        g = R.FAMILIES[name]()
        _CASES[name] = (g, R.own_h(g))
    g, h = _CASES[name]
    return g, (h if mode == "var" else None)


def make_ctx(capi, gas, h, flags=0):
    var = h is not None
    return make_context(capi, dict(gas, h=h) if var else gas, variable=var, flags=with_variable_h(capi, flags, var))


def accel(ctx):
    return np.stack([ctx.field(f) for f in ("ax", "ay", "az")])


def sources(gas):
    """the particles as external gravity sources: {x, y, z, m} records on the device and their exact bounding box"""
    import torch
    src = torch.tensor(np.stack([gas["x"], gas["y"], gas["z"], gas["m"]], axis=1), dtype=torch.float64, device="cuda:0")
    lo_hi = np.array([gas["x"].min(), gas["y"].min(), gas["z"].min(), gas["x"].max(), gas["y"].max(), gas["z"].max()])
    return src, lo_hi


def gpu_gravity(capi, name, mode, ext=False):
    gas, h = case(name, mode)
    ctx = make_ctx(capi, gas, h, capi.FLAG_SELF_GRAVITY)
    keep = None
    if ext:
        keep, lo_hi = sources(gas)
        ctx.set_gravity_sources_dev(gas["x"].size, keep.data_ptr(), lo_hi)
    ctx.density(); ctx.forces()
    a = accel(ctx)
    nq = ctx.params.nq
    ctx.close()
    del keep
    return a, nq


_WALK = {}


def default_walk(capi, name, mode):
    if (name, mode) not in _WALK:
        _WALK[name, mode] = gpu_gravity(capi, name, mode)
    return _WALK[name, mode]


def oracle_gravity(name, mode, nq):
    from oracle import orc, orc_grav
    gas, h = case(name, mode)
    x, y, z, m = (gas[k] for k in "xyzm")
    t = orc_grav.Tree(x, y, z, m)
    ga = [np.zeros(x.size) for _ in range(3)]
    orc_grav.gravity(t, x, y, z, *ga, h=2.5, h_var=h, nq=nq, nthreads=orc.max_threads())
    t.free()
    return np.stack(ga)


def per_target_excess(a, ref):
    """|da_i| / (1e-9 |a_i| + 1e-12 max|a|) per target (<= 1 passes): 0 where they agree exactly, inf where the bar is 0"""
    d = np.linalg.norm(a - ref, axis=0)
    an = np.linalg.norm(ref, axis=0)
    bar = 1e-9 * an + 1e-12 * an.max()
    ex = np.zeros(d.size)
    nz = d > 0.0
    ex[nz] = np.where(bar[nz] > 0.0, d[nz] / np.where(bar[nz] > 0.0, bar[nz], 1.0), np.inf)
    return ex


def test_gravity_free_context_is_exactly_zero(capi):
    """u = v = alpha = 0 and no sinks: without SPH_FLAG_SELF_GRAVITY every acceleration is exactly 0, in both modes, so
    what the tests below compare is the Barnes-Hut term alone"""
    for name in ("lattice33", "plummer", "coincident", "ragged65"):
        for mode in MODES:
            gas, h = case(name, mode)
            ctx = make_ctx(capi, gas, h)
            ctx.density(); ctx.forces()
            assert np.all(accel(ctx) == 0.0), (name, mode)
            ctx.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_gravity_per_target_vs_oracle_octree(capi, name, mode):
    """every target within 1e-9 of its own |a| plus 1e-12 of the field's max|a| of the oracle's walk of the reference's
    octree.  Observed on the MI355X: at most 0.044 of that bar (sparse cube, fixed h), 0.0043 (shared keys, fixed h),
    below 1e-3 on every other family, and exact zeros where the field is zero (one particle, all coincident)."""
    a, nq = default_walk(capi, name, mode)
    ref = oracle_gravity(name, mode, nq)
    assert np.all(np.isfinite(a))
    ex = per_target_excess(a, ref)
    worst = int(np.argmax(ex))
    print(f"{name} {mode}: worst target {worst} uses {ex[worst]:.3g} of the bar")
    assert ex[worst] <= 1.0, (worst, a[:, worst], ref[:, worst])


def _child_results(tmp_path):
    """the per-lane walk (SPH_GRAV_WAVE=0, read once per process) in a child process: every family's gravity in both
    modes, and two fixed-h steps with SPH_FLAG_REUSE_GRAVITY"""
    path = tmp_path / "lane.npz"
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {HERE!r})\n"
        "import test_octree_adversarial_gpu as T\n"
        "from summersph_amd import capi\n"
        "capi.load()\n"
        "out = {}\n"
        "for name in T.NAMES:\n"
        "    for mode in T.MODES:\n"
        "        out[name + '/' + mode] = T.gpu_gravity(capi, name, mode)[0]\n"
        "    out[name + '/steps'] = T.two_steps(capi, name, capi.FLAG_REUSE_GRAVITY)\n"
        "np.savez(sys.argv[1], **out)\n"
    )
    subprocess.run([sys.executable, "-c", code, str(path)], check=True, env={**os.environ, "SPH_GRAV_WAVE": "0"},
                   timeout=600)
    return dict(np.load(path))


def two_steps(capi, name, flags=0):
    gas, _ = case(name, "fixed")
    ctx = make_ctx(capi, gas, None, capi.FLAG_SELF_GRAVITY | flags)
    t = 0.0
    for _ in range(2):
        _, t = ctx.step(1e-3, t)
    out = np.stack([ctx.field(f) for f in "x y z vx vy vz ax ay az".split()])
    ctx.close()
    return out


def test_wave_walk_is_bitwise_the_per_lane_walk(capi, tmp_path):
    """the wave walk (64 targets per wave, lanes asleep until their rope) accumulates exactly each lane's
    own walk, so it equals the per-lane grav_walk bit for bit -- on every family, in both modes, where the lanes of one
    wave disagree most; and two steps with the per-lane walk and SPH_FLAG_REUSE_GRAVITY equal two wave-walk steps"""
    lane = _child_results(tmp_path)
    for name in NAMES:
        for mode in MODES:
            assert np.array_equal(lane[name + "/" + mode], default_walk(capi, name, mode)[0]), (name, mode)
        assert np.array_equal(lane[name + "/steps"], two_steps(capi, name)), name


@pytest.mark.parametrize("mode", MODES)
def test_external_sources_equal_the_in_context_tree(capi, mode):
    """sph_set_gravity_sources_dev with the context's own particles and their exact box: same root, keys and order, and
    the own leaf adds fma(-f, 0, a) = a, so the result is bitwise the in-context tree's -- except where path keys
    coincide: the tie order is then the source order instead of the slot order, the pairwise sums run in another order,
    and the per-target bar against the oracle applies"""
    for name in NAMES:
        a, nq = gpu_gravity(capi, name, mode, ext=True)
        if name in KEY_TIES:
            ex = per_target_excess(a, oracle_gravity(name, mode, nq))
            assert ex.max() <= 1.0, name
        else:
            assert np.array_equal(a, default_walk(capi, name, mode)[0]), name


# ---- accretion -----------------------------------------------------------------------------------------------------
def _sinks(pos, rad, m=1.0):
    s = {k: np.array([v]) for k, v in zip("xyz", pos)}
    s.update({k: np.zeros(1) for k in ("vx", "vy", "vz")})
    s["m"] = np.array([m]); s["radius"] = np.array([rad])
    return s


def _planted(tweak):
    """a small cloud with six particles planted at L1 distance radius from the sink (tweak 0), or 1 ulp inside (-1) or
    outside (+1) along their largest offset -- one set per case, so that no two planted particles share a path key"""
    rng = np.random.default_rng(21)
    p = rng.uniform(-20.0, 20.0, (3, 2000))
    s, rad = np.array([1.0, 2.0, 3.0]), 4.0
    offs = []
    for d in ([rad, 0, 0], [0, -rad, 0], [0, 0, rad], [2.0, 2.0, 0.0], [-1.0, 0.0, -3.0], [0.0, 2.5, -1.5]):
        d = np.array(d, dtype=np.float64)
        k = int(np.argmax(np.abs(d)))
        q = s + d
        if tweak:
            q[k] = np.nextafter(q[k], s[k] if tweak < 0 else q[k] + d[k])
        offs.append(q)
    p = np.concatenate([p, np.array(offs).T], axis=1)
    rng2 = np.random.default_rng(22)
    v = rng2.normal(0.0, 0.1, p.shape)
    gas = R._gas(p[0], p[1], p[2], rng2.uniform(0.5e-3, 2.0e-3, p.shape[1]))
    gas["vx"], gas["vy"], gas["vz"] = v[0].copy(), v[1].copy(), v[2].copy()
    return gas, _sinks(s, rad)


ACC_CASES = {
    # centred lattice, sink on a lattice point, dyadic radius: the box tests hit exact ties
    "lattice_s400_r8": lambda: (R.lattice(k=33, spacing=2.0, origin=-32.0), _sinks((4.0, 0.0, 0.0), 8.0)),
    "lattice_s224_r8": lambda: (R.lattice(k=33, spacing=2.0, origin=-32.0), _sinks((2.0, 2.0, 4.0), 8.0)),
    "lattice_s004_r12": lambda: (R.lattice(k=33, spacing=2.0, origin=-32.0), _sinks((0.0, 0.0, 4.0), 12.0)),
    "plummer_core": lambda: (R.plummer(), _sinks((0.0, 0.0, 0.0), 6.0)),
    "planted_at": lambda: _planted(0),
    "planted_in": lambda: _planted(-1),
    "planted_out": lambda: _planted(1),
}


def oracle_accrete(gas, sinks, variant):
    from oracle import orc_grav
    o = orc_grav.OracleFull(gas, sinks)
    o.tree = orc_grav.Tree(o.x, o.y, o.z, o.m)
    removed = o.accrete_and_cull(variant=variant)
    return o, removed


def check_accretion(ctx, gas, sinks, o, removed, got_removed, tag):
    assert got_removed == removed and ctx.n == o.n, tag
    for f in "x y z vx vy vz m".split():
        assert np.array_equal(ctx.field(f), getattr(o, f)), (tag, f)        # the survivors, in the caller's order
    s = ctx.get_sinks()
    for k in "x y z vx vy vz m".split():
        assert abs(s[k][0] - getattr(o, "s" + k)[0]) <= 1e-15 * max(abs(getattr(o, "s" + k)[0]), 1.0), (tag, k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(ACC_CASES))
def test_accretion_vs_oracle_on_ties(capi, name, mode):
    """the removed set, the survivors' order and the sink's mass, position and velocity against the oracle's walk of the
    reference's octree: [F]'s rule (leaf centre, variant 0) for fixed h, [V]'s (L1 distance, variant 1) for variable h.
    No pair here is closer than root / 2^21 (the level-21 leaf centre is a documented deviation for accretion)."""
    gas, sinks = ACC_CASES[name]()
    k = R.path_keys(gas["x"], gas["y"], gas["z"])
    assert np.unique(k).size == k.size
    variant = 1 if mode == "var" else 0
    o, removed = oracle_accrete(gas, sinks, variant)
    assert removed > 0 or name.startswith("planted"), name     # the case exercises accretion
    if name.startswith("planted") and variant == 1:
        # [V]'s rule is dr < radius: of the planted particles only those 1 ulp inside may go
        gone = ~np.isin(gas["m"][-6:], o.m)                     # (the masses are all different)
        assert np.any(gone) if name == "planted_in" else not np.any(gone), gone
    ctx = make_ctx(capi, gas, R.own_h(gas) if mode == "var" else None)
    ctx.set_sinks(sinks)
    ctx.density()
    got = ctx.accrete_and_cull()
    check_accretion(ctx, gas, sinks, o, removed, got, name)
    ctx.close()


def test_accretion_through_the_external_source_tree(capi):
    """the multi-GPU accretion pass (sph_accrete_mark_dev / sph_accrete_apply_dev, which replays the box chain from the
    external source set's keys) on one context whose sources are its own particles: the same as the oracle"""
    import torch
    for name in ("lattice_s400_r8", "lattice_s224_r8", "lattice_s004_r12"):
        gas, sinks = ACC_CASES[name]()
        o, removed = oracle_accrete(gas, sinks, 0)
        ctx = make_ctx(capi, gas, None, capi.FLAG_SELF_GRAVITY)
        ctx.set_sinks(sinks)
        src, lo_hi = sources(gas)
        ctx.set_gravity_sources_dev(gas["x"].size, src.data_ptr(), lo_hi)
        ctx.density()
        part = torch.empty(448, dtype=torch.float64, device="cuda:0")
        ctx.accrete_mark_dev(0, part.data_ptr())
        allp = part.view(1, -1).contiguous()
        keep = torch.empty(gas["x"].size, dtype=torch.int32, device="cuda:0")
        got = ctx.accrete_apply_dev(allp.data_ptr(), 1, 448, keep.data_ptr())
        ctx.set_gravity_sources_dev(0, 0, None)
        check_accretion(ctx, gas, sinks, o, removed, got, name)
        ctx.close()
