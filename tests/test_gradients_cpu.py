"""CPU tests of the SPH gradients (sph_gradients): the ABI mirrors (ctypes, Fortran) against the C header, the register
budget of the gradient kernels, the numpy restatement against a naive O(N^2) double loop, its exactness on linear fields,
its rho~ against the reference's density, the Keplerian vorticity, a planar (singular) set, and the command line's
parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT, load_golden
import gradients_ref
from summersph_amd import ic

FIELDS = ["clip_lo", "clip_hi", "h", "fields", "n_fields", "flags", "reserved"]


def test_gradients_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_gradients_desc", FIELDS,
                   ['printf("consts %d %d %d\\n", SPH_GRAD_CORRECTED, SPH_GRAD_MAX_FIELDS, SPH_GRAD_VALUES);'])
    assert int(got["size"]) == ctypes.sizeof(capi.GradientsDesc) == 88
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.GradientsDesc, f).offset, f
    assert got["consts"] == f"{capi.GRAD_CORRECTED} {capi.GRAD_MAX_FIELDS} {capi.GRAD_VALUES}" == "1 4 -1"
    assert "sph_gradients" in capi.SYMBOLS and "sph_gradients_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_GRAD_CORRECTED = 1, SPH_GRAD_MAX_FIELDS = 4, SPH_GRAD_VALUES = -1", binding)
    d = capi.gradients_desc(("u", capi.GRAD_VALUES), corrected=False, h=1.5, clip=((0, 1, 2), (3, 4, 5)))
    assert (d.n_fields, d.flags, d.h, list(d.reserved)) == (2, 0, 1.5, [0, 0])
    assert list(d.fields) == [capi.FIELDS.index("u"), -1, 0, 0]
    assert list(d.clip_lo) == [0, 1, 2] and list(d.clip_hi) == [3, 4, 5]
    d = capi.gradients_desc()
    assert d.flags == capi.GRAD_CORRECTED and d.h == 0.0 and d.n_fields == 3
    assert list(d.fields)[:3] == [3, 4, 5] and list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3
    for bad in ((), ("u",) * 5):
        with pytest.raises(ValueError):
            capi.gradients_desc(bad)


def test_velocity_derivatives_of_a_linear_flow():
    from summersph_amd import capi
    # v = M x: grad[k, a] = M[k, a]
    M = np.array([[0.1, -2.0, 0.3], [1.5, 0.2, -0.7], [0.4, 0.9, -0.3]])
    g = np.repeat(M[:, :, None], 5, axis=2)
    v = capi.velocity_derivatives(g)
    assert np.allclose(v["divv"], np.trace(M))
    assert np.allclose(v["curl"][:, 0], [M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    assert np.allclose(v["curl_mag"], np.linalg.norm(v["curl"][:, 0]))


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "grad_caller", """program grad_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_gradients_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: out(:, :, :), rho(:)
  integer(c_int64_t) :: nt, ns
  integer(c_int) :: st
  ctx = c_null_ptr
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%h = 0.0_c_double
  d%fields = [SPH_F_VX, SPH_F_VY, SPH_F_VZ, SPH_GRAD_VALUES]
  d%n_fields = 3
  d%flags = SPH_GRAD_CORRECTED
  d%reserved = 0
  if (c_sizeof(d) /= 88) stop 1
  allocate(out(10, 3, 3), rho(10))
  st = sph_gradients(ctx, d, c_null_ptr, c_loc(out), 90_c_int64_t, c_loc(rho), nt, ns)
  st = sph_gradients_dev(ctx, d, c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr)
  print *, st, nt, ns
end program grad_caller
""")


@needs_hipcc
def test_gradient_kernels_fit_the_register_budget():
    k = resource_usage("gradients.hip", containing("grad_"))
    for name in ("grad_select", "grad_box", "grad_keys", "grad_gather", "grad_tails"):
        assert sum(name in n for n in k) == 1, name
    walks = [n for n in k if "grad_walk" in n]
    assert len(walks) == 8, walks
    for kk in (1, 2, 3, 4):
        for corr in (0, 1):
            assert sum(f"grad_walkILi{kk}ELb{corr}E" in n for n in walks) == 1, (kk, corr)
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def _rel(got, want, mask):
    s = np.max(np.abs(want[..., mask]))
    return float(np.max(np.abs(got[..., mask] - want[..., mask])) / s)


def test_restatement_matches_the_naive_double_loop():
    rng = np.random.default_rng(11)
    n = 500
    pos = rng.uniform(0, 6, (n, 3))
    m = rng.uniform(0.5, 1.5, n)
    A = np.stack([np.sin(pos[:, 0]) + pos[:, 1] ** 2, np.cos(pos[:, 2] * pos[:, 0]), rng.normal(size=n)])
    for h in (0.9, rng.uniform(0.6, 1.4, n)):
        for corrected in (True, False):
            g, rho, nt, ns = gradients_ref.gradients(pos, m, A, h, corrected=corrected)
            gn, rn, sn = gradients_ref.naive(pos, m, A, h, corrected=corrected)
            assert nt == n
            assert np.max(np.abs(rho - rn) / rn) <= 1e-13
            assert ns == int(sn.sum())
            ok = ~sn
            assert np.array_equal(np.isnan(g[0, 0]), sn)
            for k in range(3):
                assert _rel(g[k], gn[k], ok) <= 1e-9, (k, corrected)


def test_clip_ghosts_and_only_select_the_targets():
    rng = np.random.default_rng(12)
    pos = rng.uniform(0, 5, (400, 3))
    pos[7] = [np.nan, 0, 0]
    m = np.ones(400)
    A = pos[:, 0].copy()
    clip = ((1, 1, 1), (4, 4, 4))
    g, rho, nt, _ = gradients_ref.gradients(pos, m, A, 0.8, n_owned=300, clip=clip)
    t = gradients_ref.targets_mask(pos, 300, clip)
    assert nt == int(t.sum()) and not t[7] and not t[300:].any()
    assert np.array_equal(np.isfinite(rho), t)
    assert np.all(np.isnan(g[:, :, ~t]))
    ids = np.nonzero(t)[0][::5]
    g2, rho2, _, _ = gradients_ref.gradients(pos, m, A, 0.8, n_owned=300, clip=clip, only=ids)
    assert np.array_equal(g2[:, :, ids], g[:, :, ids]) and np.array_equal(rho2[ids], rho[ids])


def _linear(pos, seed):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(4, 3))
    c0 = rng.normal(size=4)
    return G, c0[:, None] + G @ pos.T


@pytest.mark.parametrize("which", ["box", "disc", "disc_var"])
def test_corrected_form_is_exact_for_linear_fields(which):
    if which == "box":
        gas, _ = ic.split_rows(ic.uniform_box(6000, seed=3))
        hs = [2.5, np.random.default_rng(1).uniform(2.0, 3.0, 6000)]
    elif which == "disc":
        gas, _ = ic.split_rows(ic.keplerian_disc(6000, seed=4))
        hs = [2.5]
    else:
        gas, _ = ic.split_rows(ic.keplerian_disc_var(6000, seed=4))
        hs = [gas["h"]]
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    G, A = _linear(pos, 5)
    for h in hs:
        g, _, nt, ns = gradients_ref.gradients(pos, gas["m"], A, h, corrected=True)
        ok = np.isfinite(g[0, 0])
        assert nt == len(pos) and ok.sum() == nt - ns and ns < 0.01 * nt
        for k in range(4):
            err = np.abs(g[k][:, ok] - G[k][:, None])
            assert np.max(err) <= 1e-11 * np.max(np.abs(G[k])), (which, k)


def test_rho_matches_the_reference_density(golden):
    e = golden("disc3000_eval")
    pos = np.stack([e["x"], e["y"], e["z"]], axis=1)
    _, rho, nt, _ = gradients_ref.gradients(pos, e["m"], e["u"], 2.5, corrected=False)
    assert nt == 3000
    rel = np.abs(rho - e["rho"]) / e["rho"]
    assert np.max(rel) <= 1e-6


def test_singular_targets_of_disc3000(golden):
    e = golden("disc3000_eval")
    pos = np.stack([e["x"], e["y"], e["z"]], axis=1)
    g, rho, nt, ns = gradients_ref.gradients(pos, e["m"], np.stack([e["vx"], e["vy"]]), 2.5)
    assert (nt, ns) == (3000, 6)
    assert int(np.isnan(g[0, 0]).sum()) == 6 and np.all(np.isfinite(rho))


def keplerian_cut(gas, r_in=10.0, margin=10.0, zcut=2.5):
    """targets of the vorticity check: |z| < zcut and at least margin from either edge of the disc"""
    r = np.hypot(gas["x"], gas["y"])
    r_out = r.max()
    sel = (np.abs(gas["z"]) < zcut) & (r > r_in + margin) & (r < r_out - margin)
    return sel, r


def vorticity_error(gas, g):
    sel, r = keplerian_cut(gas)
    omega = np.sqrt(ic.G_DP * 1.0 / r ** 3)
    wz = g[1, 0] - g[0, 1]
    err = np.abs(wz - omega / 2) / (omega / 2)
    return err[sel]


def test_keplerian_vorticity_is_half_omega():
    gas, _ = ic.split_rows(ic.keplerian_disc(20000, seed=5))
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    sel, _ = keplerian_cut(gas)
    ids = np.nonzero(sel)[0]
    A = np.stack([gas["vx"], gas["vy"], gas["vz"]])
    gc, _, _, _ = gradients_ref.gradients(pos, gas["m"], A, 2.5, corrected=True, only=ids)
    gs, _, _, _ = gradients_ref.gradients(pos, gas["m"], A, 2.5, corrected=False, only=ids)
    ec, es = vorticity_error(gas, gc), vorticity_error(gas, gs)
    print(f"omega_z vs Omega/2: corrected median {np.median(ec):.4f} p90 {np.percentile(ec, 90):.4f}; "
          f"standard median {np.median(es):.4f} p90 {np.percentile(es, 90):.4f}")
    assert np.median(ec) <= 0.03
    divv, _ = gradients_ref.velocity_derivatives(gc)
    r = np.hypot(gas["x"], gas["y"])[sel]
    assert np.median(np.abs(divv[sel]) / np.sqrt(ic.G_DP / r ** 3)) <= 0.02


def test_planar_set_is_all_singular():
    rng = np.random.default_rng(13)
    n = 800
    pos = np.zeros((n, 3))
    pos[:, :2] = rng.uniform(0, 8, (n, 2))
    A = pos[:, 0] * 2.0 + pos[:, 1]
    g, rho, nt, ns = gradients_ref.gradients(pos, np.ones(n), A, 1.0, corrected=True)
    assert nt == ns == n and np.all(np.isnan(g)) and np.all(np.isfinite(rho))
    g, _, _, ns = gradients_ref.gradients(pos, np.ones(n), A, 1.0, corrected=False)
    assert ns == 0 and np.all(np.isfinite(g)) and np.all(g[0, 2] == 0.0)


def test_cli_refuses_bad_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, gradients
    assert gradients.parse_fields("vx,vy,vz") == ["vx", "vy", "vz"]
    for bad in ("", "vx,nope", "u,u,u,u,u", "vx,,vy"):
        with pytest.raises(ValueError):
            gradients.parse_fields(bad)

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    monkeypatch.setattr(gradients, "read_save", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the save file was read")))
    base = ["missing.txt", "-o", str(tmp_path / "o.npz")]
    for extra in (["--h", "-1"], ["--h", "nan"], ["--h", "inf"], ["--clip", "0,0,0,1,1"], ["--clip", "0,0,0,1,1,nan"],
                  ["--fields", "vx,bogus"], ["--fields", "h"], ["--fields", "u,u,u,u,u"], ["--fields", ""]):
        with pytest.raises(SystemExit) as e:
            gradients.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
