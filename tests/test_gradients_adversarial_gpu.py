"""GPU tests of sph_gradients on the adversarial sets of tests/search_sets.py: an enlarged cell edge, nodes on cell faces, a
heap of coincident particles, a planar set, a set far from the origin, the smallest tables, and two scales of h whose wide
targets reach +-8 cells.  tests/test_search_sets_cpu.py asserts that each set reaches its branch, that no target visits more
than 10^4 cells (grad_walk's reach is unbounded: a set beyond that cap must not be handed to the call) and that no target
sums more than 512 sources, which keeps the worst case of a sum, (512 + 16) 2^-53 = 5.9e-14, inside the 1e-13 that
tests/test_gradients_gpu.py's _cmp holds rho~ to: the project's rule is used unchanged."""
import numpy as np
import pytest

from gpu_support import capi, make_context
import gradients_ref
import search_sets as S
from test_gradients_gpu import _cmp

pytestmark = pytest.mark.gpu
FIXED_H_DENSITY = [n for n in S.GRADIENT_SETS if n in S.DENSITY_SETS]


def _ctx(capi, s, density=False):
    return make_context(capi, s.gas, density=density, **s.context_kw())


WORST = [0.0]


def _worst(g, rg, rho, rrho):
    """the largest error in units of _cmp's bounds (1e-12 of a field's largest gradient, 1e-13 of rho~), for the report"""
    w = 0.0
    for k in range(g.shape[0]):
        ok = np.isfinite(rg[k]) & np.isfinite(g[k])
        if ok.any() and np.max(np.abs(rg[k][ok])) > 0.0:
            w = max(w, float(np.max(np.abs(g[k] - rg[k])[ok]) / (1e-12 * np.max(np.abs(rg[k][ok])))))
    ok = np.isfinite(rrho) & np.isfinite(rho)
    return max(w, float(np.max(np.abs(rho[ok] - rrho[ok]) / np.abs(rrho[ok])) / 1e-13)) if ok.any() else w


def _cmp_any(g, rg, rho, rrho, ratio):
    """_cmp; where no target has a finite row (every one singular) there is no scale: the NaN patterns and rho~ alone"""
    WORST[0] = max(WORST[0], _worst(g, rg, rho, rrho))
    if np.isfinite(rg).any():
        _cmp(g, rg, rho, rrho, ratio=ratio)
    else:
        assert np.all(np.isnan(g))
        _cmp(np.zeros((1, 1)), np.zeros((1, 1)), rho, rrho)


@pytest.mark.parametrize("corrected", [True, False])
@pytest.mark.parametrize("name", S.GRADIENT_SETS)
def test_parity_with_the_restatement(capi, name, corrected):
    import torch
    s = S.get(name)
    rows = S.gradient_rows(s)
    vals = np.ascontiguousarray(rows[:4])
    inf = {}
    rg, rr, nt, ns = gradients_ref.gradients(s.pos, s.m, rows, s.h_all, corrected=corrected, info=inf)
    ratio = inf["ratio"] if corrected else None
    assert nt == s.n
    ctx = _ctx(capi, s)
    V = capi.GRAD_VALUES
    WORST[0] = 0.0
    for k in range(1, 5):
        g, rho, cnt = ctx.gradients(fields=S.GRAD_FIELDS[:k], corrected=corrected, rho=True)
        assert cnt == (nt, ns), (k, cnt, nt, ns)
        _cmp_any(g, rg[4:4 + k], rho, rr, ratio)
        g, rho, cnt = ctx.gradients(fields=(V,) * k, values=vals[:k], corrected=corrected, rho=True)
        assert cnt == (nt, ns)
        _cmp_any(g, rg[:k], rho, rr, ratio)
    # the device form: bitwise the host form
    h = ctx.gradients(fields=("vx", V, "u", V), values=vals, corrected=corrected, rho=True)
    d = ctx.gradients(fields=("vx", V, "u", V), values=torch.from_numpy(vals).to(torch.device("cuda", 0)), corrected=corrected,
                      rho=True, device=True)
    _cmp_any(h[0], rg[[4, 1, 7, 3]], h[1], rr, ratio)
    assert np.array_equal(h[0], d[0].cpu().numpy(), equal_nan=True) and np.array_equal(h[1], d[1].cpu().numpy()) and h[2] == d[2]
    print(f"{name} {'corrected' if corrected else 'standard'}: {nt} targets, {ns} singular; largest error / bound {WORST[0]:.3f}")
    ctx.close()


# ---- physical anchors that do not pass through the restatement -------------------------------------------------------------
@pytest.mark.parametrize("name", ["face_lattice0", "face_lattice1", "face_lattice2", "two_scales", "far_clusters"])
def test_linear_fields_are_exact(capi, name):
    s = S.get(name)
    ctx = _ctx(capi, s)
    g, _, (nt, ns) = ctx.gradients(fields=(capi.GRAD_VALUES,) * 2, values=S.linear_rows(s))
    ok = np.isfinite(g[0, 0])
    assert nt == s.n and ok.sum() == nt - ns and ok.sum() >= 40          # far_clusters is sparse: 42 of 512 have a solvable C
    for k in range(2):
        err = float(np.max(np.abs(g[k][:, ok] - S.LINEAR_A[k][:, None])))
        print(f"{name}: linear field {k}: {ok.sum()} targets, max error {err:.3e} of {np.max(np.abs(S.LINEAR_A[k])):g}")
        assert err <= 1e-11 * np.max(np.abs(S.LINEAR_A[k]))
    ctx.close()


@pytest.mark.parametrize("corrected", [True, False])
def test_heap_members_get_the_same_row(capi, corrected):
    s = S.get("heap")
    ctx = _ctx(capi, s)
    g, rho, (nt, ns) = ctx.gradients(fields=(capi.GRAD_VALUES,) * 4, values=S.value_rows(s), corrected=corrected, rho=True)
    assert (nt, ns) == (512, 0) and np.all(np.isfinite(g))
    n = S.HEAP_N
    assert np.array_equal(g[:, :, :n], np.repeat(g[:, :, :1], n, axis=2)) and np.all(rho[:n] == rho[0])
    assert len(np.unique(g[0, 0, n:])) > 200
    ctx.close()


def test_a_single_particle(capi):
    s = S.get("tiny1")
    ctx = _ctx(capi, s)
    g, rho, cnt = ctx.gradients(fields=("u",), rho=True)
    want = s.m[0] / (np.pi * s.h ** 3)
    assert cnt == (1, 1) and np.all(np.isnan(g)) and abs(rho[0] - want) <= 4 * 2.0 ** -53 * want
    g, rho, cnt = ctx.gradients(fields=("u",), corrected=False, rho=True)
    assert cnt == (1, 0) and np.all(g == 0.0) and abs(rho[0] - want) <= 4 * 2.0 ** -53 * want
    ctx.close()


def test_plane_is_singular_in_the_corrected_form_only(capi):
    s = S.get("plane")
    ctx = _ctx(capi, s)
    g, rho, (nt, ns) = ctx.gradients(rho=True)
    assert nt == ns == s.n and np.all(np.isnan(g)) and np.all(np.isfinite(rho))
    g, _, (nt, ns) = ctx.gradients(corrected=False, fields=("vx", "vy", "x"))
    assert (nt, ns) == (s.n, 0) and np.all(np.isfinite(g)) and np.all(g[:, 2] == 0.0)
    ctx.close()


# ---- order rule --------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2]


@pytest.mark.parametrize("name", ["far_clusters", "face_lattice0", "face_lattice1", "face_lattice2", "heap", "plane", "offset", "tiny65"])
def test_order_rule_bitwise(capi, name):
    s = S.get(name)
    ctx = _ctx(capi, s)
    kw = {"fields": ("vx", "vy", "vz", "u"), "rho": True}
    r0 = ctx.gradients(**kw)
    _same(r0, ctx.gradients(**kw))                                 # repeated
    pos = s.pos
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    pad = 0.5 * (hi - lo) + 1.0
    _same(r0, ctx.gradients(clip=(tuple(lo - pad), tuple(hi + pad)), **kw))      # a clip that contains every target
    for corrected in (True, False):
        c0 = ctx.gradients(corrected=corrected, **kw)
        _same(c0, ctx.gradients(corrected=corrected, clip=(tuple(lo - pad), tuple(hi + pad)), **kw))
    if name in FIXED_H_DENSITY:                                    # a fresh upload against the state after sph_density
        ctx.density()
        _same(r0, ctx.gradients(**kw))
    ctx.close()
