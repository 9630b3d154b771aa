"""CPU tests of sph_gravity_at: the ABI mirrors (ctypes, Fortran) against the C header, the register budget of the new
kernels, the numpy restatement against itself (gamma q^3 is the force's mass fraction, a = -grad Phi) and the command
line's parsing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from abi_support import containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import energy_ref
import gravity_at_ref as ref


def test_header_constants_and_prototypes_match_capi(tmp_path):
    from summersph_amd import capi
    hdr = open(os.path.join(ROOT, "include", "summersph.h")).read()
    for name, val in (("GAS", 1), ("SINKS", 2), ("SPLIT", 4)):
        assert re.search(rf"#define SPH_GRAVAT_{name}\s+{val}\b", hdr)
        assert getattr(capi, "GRAVAT_" + name) == val
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int sph_gravity_at(sph_ctx *ctx, const sph_gravity_at_desc *d, int64_t n_points, const double *px, "
            "const double *py, const double *pz, const double *ph, double *host_out, int64_t n_out, int64_t *counts);") in flat
    assert ("int sph_gravity_at_dev(sph_ctx *ctx, const sph_gravity_at_desc *d, int64_t n_points, const double *d_px, "
            "const double *d_py, const double *d_pz, const double *d_ph, double *d_out, int64_t n_out, int64_t *d_counts);") in flat
    assert {"sph_gravity_at", "sph_gravity_at_dev"} <= set(capi.SYMBOLS)
    assert capi.GRAVAT_REF_SOFT2 == ref.SOFT2 == energy_ref.SOFT2
    lib = capi.load()
    for f in (lib.sph_gravity_at, lib.sph_gravity_at_dev):
        assert [t.__name__ for t in f.argtypes] == ["c_void_p", "LP_GravityAtDesc", "c_long"] + ["c_void_p"] * 5 + ["c_long", "c_void_p"]
    assert ctypes.sizeof(capi.GravityAtDesc) == 32
    assert [(n, getattr(capi.GravityAtDesc, n).offset) for n, _ in capi.GravityAtDesc._fields_] == \
        [("h", 0), ("soft2", 8), ("flags", 16), ("reserved", 20)]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "summersph.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(sph_gravity_at_desc), offsetof(sph_gravity_at_desc, soft2), offsetof(sph_gravity_at_desc, flags), '
                   'offsetof(sph_gravity_at_desc, reserved), SPH_GRAVAT_GAS | SPH_GRAVAT_SINKS | SPH_GRAVAT_SPLIT); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c")], check=True)
    assert subprocess.run([str(tmp_path / "c")], check=True, capture_output=True, text=True).stdout.split() == \
        ["32", "8", "16", "20", "7"]
    d = capi.gravity_at_desc(h=1.5, soft2=0.0, gas=True, sinks=False)
    assert (d.h, d.soft2, d.flags, list(d.reserved)) == (1.5, 0.0, 1, [0, 0, 0])
    assert capi.gravity_at_desc(split=True).flags == 7 and capi.gravity_at_desc().soft2 == 0.0025
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_GRAVAT_GAS = 1, SPH_GRAVAT_SINKS = 2, SPH_GRAVAT_SPLIT = 4", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    exe = fortran_links(tmp_path, "gravity_at_caller", """program gravity_at_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(c_ptr) :: ctx
  type(sph_gravity_at_desc) :: d
  real(c_double), allocatable, target :: p(:, :), out(:, :)
  integer(c_int64_t), target :: counts(2)
  integer(c_int) :: st
  ctx = c_null_ptr
  allocate(p(10, 3), out(10, 8))
  d%h = 2.5_c_double
  d%soft2 = 0.0025_c_double
  d%flags = ior(ior(SPH_GRAVAT_GAS, SPH_GRAVAT_SINKS), SPH_GRAVAT_SPLIT)
  d%reserved = 0
  if (c_sizeof(d) /= 32) stop 3
  st = sph_gravity_at(ctx, d, 10_c_int64_t, c_loc(p(1, 1)), c_loc(p(1, 2)), c_loc(p(1, 3)), c_null_ptr, c_loc(out), &
                      80_c_int64_t, c_loc(counts))
  if (st /= 1) stop 1
  st = sph_gravity_at_dev(ctx, d, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t, &
                          c_null_ptr)
  if (st /= 1) stop 2
end program gravity_at_caller
""")
    assert subprocess.run([str(exe)]).returncode == 0        # a null context is SPH_ERR_ARG before any device is touched


@needs_hipcc
def test_gravity_at_kernels_fit_the_register_budget():
    k = resource_usage("gravity_at.hip", containing("gravat_"))
    k.update(resource_usage("gravity.hip", containing("grav_field_points")))
    for name in ("gravat_point_keys", "gravat_finish", "grav_field_points"):
        assert sum(name in n for n in k) == 1, name
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def test_gamma_is_the_force_mass_fraction_over_q_cubed():
    q = np.linspace(1e-3, 3.0, 30001)
    assert np.max(np.abs(ref.gamma_kernel(q) * q**3 - energy_ref.grav_table_poly(q))) <= 2e-14
    assert ref.gamma_kernel(np.array([0.0]))[0] == 4.0 / 3.0
    for qe in (1.0, 2.0):                                    # continuous across the pieces
        lo, hi = ref.gamma_kernel(np.array([np.nextafter(qe, 0.0)]))[0], ref.gamma_kernel(np.array([qe]))[0]
        assert abs(lo - hi) <= 1e-14
    # phi'(q) = q gamma(q), by central differences away from the joints: a step of 1e-5 keeps both the truncation
    # (h^2 |d3 phi| / 6 < 1e-10) and the rounding (1e-16 |phi| / h ~ 1e-11) under the bound
    h = 1e-5
    dphi = (energy_ref.phi_kernel(q + h) - energy_ref.phi_kernel(q - h)) / (2 * h)
    inner = (np.abs(q - 1.0) > 2 * h) & (np.abs(q - 2.0) > 2 * h)
    assert np.max(np.abs(dphi[inner] - (q * ref.gamma_kernel(q))[inner])) <= 1e-9


@pytest.mark.parametrize("soft2", [0.0, ref.SOFT2])
def test_restatement_acceleration_is_minus_grad_phi(soft2):
    """one source of mass m, h = 2.5: points along a skew line at q in all three pieces and next to q = 1 and q = 2"""
    G, hp, m = 39.478416442871094, 2.5, 1e-3
    src = (np.array([0.3]), np.array([-0.2]), np.array([0.1]), np.array([m]))
    u = np.array([0.6, -0.48, 0.64])
    qs = np.array([0.05, 0.4, 0.999, 1.0, 1.001, 1.5, 1.999, 2.0, 2.001, 3.0, 40.0])
    pts = np.array([0.3, -0.2, 0.1]) + (qs * hp)[:, None] * u
    out, scale = ref.gas_field(pts, hp, src, G, soft2)
    eps = 1e-5
    for k in range(3):
        e = np.zeros(3); e[k] = eps
        up, _ = ref.gas_field(pts + e, hp, src, G, soft2)
        dn, _ = ref.gas_field(pts - e, hp, src, G, soft2)
        grad = (up[0] - dn[0]) / (2 * eps)
        # central differences: O(eps^2 phi''') + rounding O(1e-16 |phi| / eps); at the joints phi''' jumps, phi'' does not
        assert np.max(np.abs(out[1 + k] + grad)) <= 1e-8 * (G * m / hp**2), k
    assert np.array_equal(scale, np.abs(out))
    # on the source with soft2 = 0: -1.4 G m / h and no pull
    o0, _ = ref.gas_field(np.array([[0.3, -0.2, 0.1]]), hp, src, G, 0.0)
    assert o0[0, 0] == -1.4 * (G * m / hp) and np.all(o0[1:, 0] == 0.0)


def test_sink_restatement():
    G = 2.0
    sinks = {"x": np.array([0.0, 5.0]), "y": np.array([0.0, 0.0]), "z": np.array([0.0, 0.0]), "m": np.array([3.0, 0.0])}
    out, scale = ref.sink_field(np.array([[2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [5.0, 0.0, 0.0]]), sinks, G)
    assert out[0, 0] == -3.0 and out[1, 0] == -1.5 and out[2, 0] == 0.0 and out[3, 0] == 0.0
    assert out[0, 1] == -np.inf and np.all(np.isnan(out[1:, 1]))
    assert out[0, 2] == -6.0 / 5.0                         # the massless sink at the point adds nothing
    assert np.array_equal(scale[:, 0], np.abs(out[:, 0]))


def test_cli_parsing_and_cylindrical():
    from summersph_amd import gravity as gv
    ap = gv.build_parser()
    a = ap.parse_args(["s.txt", "-o", "g.npz", "--rotation-curve", "10", "60", "25", "64", "--theta", "0.3"])
    gv.check_args(ap, a)
    assert a.rotation_curve == ["10", "60", "25", "64"] and a.theta == 0.3 and not a.particles and a.polar is None
    a = ap.parse_args(["s.txt", "-o", "g.npz", "--particles", "--variable", "--split", "--soft2", "0"])
    gv.check_args(ap, a)
    assert a.particles and a.variable and a.split and a.soft2 == 0.0 and a.h is None
    a = ap.parse_args(["s.txt", "-o", "g.npz", "--polar", "10", "60", "4", "8", "--no-sinks", "--h", "1.5", "--json"])
    gv.check_args(ap, a)
    from summersph_amd.sample import points_from_args
    pts, shape = points_from_args(a)
    assert pts.shape == (32, 3) and shape == (4, 8) and a.no_sinks and not a.no_gas
    for bad in (["--polar", "1", "2", "3", "4", "--no-gas", "--no-sinks"], ["--polar", "1", "2", "3", "4", "--split", "--no-gas"],
                ["--particles", "--h", "-1"], ["--particles", "--soft2", "-1"], ["--particles", "--theta", "0"],
                ["--polar", "1", "2", "3", "4", "--variable"], ["--particles", "--polar", "1", "2", "3", "4"], []):
        with pytest.raises(SystemExit):
            b = ap.parse_args(["s.txt", "-o", "g.npz"] + bad)
            gv.check_args(ap, b)
    # cylindrical components in an inclined frame: a pull towards the axis, a swirl about it, a lift along it
    rng = np.random.default_rng(3)
    centre, normal = (1.0, -2.0, 0.5), (0.3, -0.2, 0.9)
    n, e1, e2 = gv.frame(normal)
    R, ph, z = rng.uniform(1.0, 5.0, 20), rng.uniform(-np.pi, np.pi, 20), rng.uniform(-1.0, 1.0, 20)
    er = np.cos(ph)[:, None] * e1 + np.sin(ph)[:, None] * e2
    ephi = -np.sin(ph)[:, None] * e1 + np.cos(ph)[:, None] * e2
    pts = np.asarray(centre) + R[:, None] * er + z[:, None] * n
    acc = (-2.0 / R**2)[:, None] * er + (0.5 * R)[:, None] * ephi + 0.25 * n
    g_r, g_phi, g_z = gv.cylindrical(acc.T, pts, centre, normal)
    assert np.max(np.abs(g_r + 2.0 / R**2)) <= 1e-14 and np.max(np.abs(g_phi - 0.5 * R)) <= 1e-14
    assert np.max(np.abs(g_z - 0.25)) <= 1e-14
    vc2 = gv.rotation_curve(np.repeat((-2.0 / R**2)[None, :] * er.T, 1, axis=0), pts, (4, 5), centre, normal)
    assert np.max(np.abs(vc2 - (2.0 / R).reshape(4, 5).mean(axis=1))) <= 1e-14
