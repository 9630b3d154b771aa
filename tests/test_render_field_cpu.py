"""CPU tests of the field rendering (sph_render_field): the ABI mirrors (ctypes, Fortran) against the C header, the
register budget of the field kernels, the numpy restatement against a scalar loop, and the command line's refusal of
--field with --script-compat."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import render_field_ref
import render_ref

FIELDS = ["base", "field", "weight", "normalise", "reserved"]


def test_render_field_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_render_field_desc", FIELDS,
                   ['printf("consts %d %d %d\\n", SPH_RENDER_FIELD_VALUES, SPH_RENDER_WEIGHT_MASS, SPH_RENDER_WEIGHT_VOLUME);',
                    'printf("base_size %zu\\n", sizeof(sph_render_desc));'])
    assert int(got["size"]) == ctypes.sizeof(capi.RenderFieldDesc) == 144
    assert int(got["base_size"]) == 128
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.RenderFieldDesc, f).offset, f
    assert got["consts"] == f"{capi.RENDER_FIELD_VALUES} {capi.RENDER_WEIGHT_MASS} {capi.RENDER_WEIGHT_VOLUME}" == "-1 0 1"
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_RENDER_FIELD_VALUES = -1, SPH_RENDER_WEIGHT_MASS = 0, SPH_RENDER_WEIGHT_VOLUME = 1", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "field_caller", """program field_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_render_field_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: img(:, :), wgt(:, :), vals(:)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%base%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%base%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%base%h = 0.0_c_double
  d%base%n = [128, 64, 32]
  d%base%axis = 1
  d%base%flags = SPH_RENDER_AUTO_BOUNDS
  d%base%reserved = 0
  d%field = SPH_F_VY
  d%weight = SPH_RENDER_WEIGHT_MASS
  d%normalise = 1
  d%reserved = 0
  allocate(img(d%base%n(3), d%base%n(1)), wgt(d%base%n(3), d%base%n(1)), vals(10))
  if (c_sizeof(d) /= 144) stop 1
  st = sph_render_field(ctx, d, c_null_ptr, img, c_loc(wgt), int(size(img), c_int64_t))
  d%field = SPH_RENDER_FIELD_VALUES
  d%weight = SPH_RENDER_WEIGHT_VOLUME
  st = sph_render_field(ctx, d, c_loc(vals), img, c_null_ptr, int(size(img), c_int64_t))
  st = sph_render_field_dev(ctx, d, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t)
  print *, st
end program field_caller
""")


@needs_hipcc
def test_field_kernels_fit_the_register_budget():
    k = resource_usage("render.hip", containing("render_", "field_gather"))
    field = {n: r for n, r in k.items() if "field_gather" in n or "render_field_records" in n}
    assert sum("field_gather" in n for n in field) == 6             # walk axis 0 / 1 / 2, with and without den
    assert sum("render_field_records" in n for n in field) == 1
    for name, r in field.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)             # 4 waves / SIMD by registers
    assert sum("render_gather" in n for n in k) == 3                 # the density gathers are still the only ones


def test_numpy_restatement_matches_a_scalar_loop():
    rng = np.random.default_rng(3)
    n = 50
    pos = rng.uniform(-3, 3, (n, 3))
    m = rng.uniform(0.5, 2.0, n)
    rho = rng.uniform(0.1, 1.0, n)
    a = rng.normal(0, 1, n)
    h = rng.uniform(0.6, 1.4, n)
    lo, hi, shape = np.array([-3.5, -3.0, -2.0]), np.array([3.0, 3.5, 2.5]), (7, 6, 5)
    ax = render_ref.axes(lo, hi, shape)

    def w_scalar(r, hj):
        q = r / hj
        s = 1.0 / (math.pi * hj ** 3)
        if q <= 1:
            return s * (1 - 1.5 * q * q + 0.75 * q ** 3)
        return s * 0.25 * (2 - q) ** 3 if q <= 2 else 0.0

    for w in (m, m / rho):
        num, den = render_field_ref.grid_brute(pos, w, a, h, lo, hi, shape)
        for i in range(shape[0]):
            for j in range(shape[1]):
                for k in range(shape[2]):
                    sn = sd = 0.0
                    for p in range(n):
                        r = math.sqrt((ax[0][i] - pos[p, 0]) ** 2 + (ax[1][j] - pos[p, 1]) ** 2 + (ax[2][k] - pos[p, 2]) ** 2)
                        t = w[p] * w_scalar(r, h[p])
                        sn += t * a[p]
                        sd += t
                    assert abs(num[i, j, k] - sn) <= 1e-13 * max(1.0, abs(sn)), (i, j, k)
                    assert abs(den[i, j, k] - sd) <= 1e-13 * max(1.0, sd), (i, j, k)
        assert np.any(den == 0) and np.any(den > 0)
        img, wgt = render_field_ref.image(num, den, axis=1, normalise=True)
        nz = wgt > 0
        assert np.allclose(img[nz], num.sum(axis=1)[nz] / den.sum(axis=1)[nz], rtol=0, atol=0)
        assert np.all(img[~nz] == 0.0)
        img2, wgt2 = render_field_ref.image(num, den, axis=2, normalise=False, scale=0.5)
        assert np.array_equal(img2, num.sum(axis=2) * 0.5) and np.array_equal(wgt2, den.sum(axis=2) * 0.5)


def test_cli_refuses_field_with_script_compat(tmp_path, monkeypatch):
    from summersph_amd import capi, render

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    monkeypatch.setattr(render, "read_save", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the save file was read")))
    for argv in (["missing.txt", "-o", str(tmp_path / "o.npy"), "--field", "vz", "--script-compat"],
                 ["missing.txt", "-o", str(tmp_path / "o.npy"), "--field-sum"],
                 ["missing.txt", "-o", str(tmp_path / "o.npy"), "--weight-out", str(tmp_path / "w.npy")]):
        with pytest.raises(SystemExit) as e:
            render.main(argv)
        assert e.value.code == 2, argv
    assert not (tmp_path / "o.npy").exists()
