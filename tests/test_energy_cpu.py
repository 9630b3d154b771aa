"""CPU tests of sph_energy: the ABI mirrors (ctypes, Fortran) against the C header, the register budget of the new kernels,
the softening potential against the force's grav_table polynomial, the numpy restatement against the numbers of the
reference's own trajectory fixture, and the command line's parsing."""
import os
import re
import subprocess

import numpy as np
import pytest

from abi_support import containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT, load_golden
import energy_ref


def test_header_constant_and_prototypes_match_capi(tmp_path):
    from summersph_amd import capi
    hdr = open(os.path.join(ROOT, "include", "summersph.h")).read()
    assert re.search(r"#define SPH_ENERGY_NSUM 28\b", hdr)
    assert "int sph_energy(sph_ctx *ctx, int64_t src_offset, double *host_sums, double *host_phi, int64_t n_phi);" in hdr
    assert "int sph_energy_dev(sph_ctx *ctx, int64_t src_offset, double *d_sums, double *d_phi, int64_t n_phi);" in hdr
    assert capi.ENERGY_NSUM == 28 == len(capi.ENERGY_SUMS) == energy_ref.NSUM
    assert capi.ENERGY_SUMS == energy_ref.SUMS
    assert {"sph_energy", "sph_energy_dev"} <= set(capi.SYMBOLS)
    lib = capi.load()
    for f in (lib.sph_energy, lib.sph_energy_dev):
        assert [t.__name__ for t in f.argtypes] == ["c_void_p", "c_long", "c_void_p", "c_void_p", "c_long"]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "summersph.h"\nint main(void) { printf("%d\\n", SPH_ENERGY_NSUM); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c")], check=True)
    assert subprocess.run([str(tmp_path / "c")], check=True, capture_output=True, text=True).stdout.strip() == "28"
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_ENERGY_NSUM = 28", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "energy_caller", """program energy_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: sums(:), phi(:)
  integer(c_int) :: st
  ctx = c_null_ptr
  allocate(sums(SPH_ENERGY_NSUM), phi(10))
  st = sph_energy(ctx, 0_c_int64_t, c_loc(sums), c_loc(phi), 10_c_int64_t)
  if (st /= 1) stop 1
  st = sph_energy_dev(ctx, 0_c_int64_t, c_null_ptr, c_null_ptr, 0_c_int64_t)
  if (st /= 1) stop 2
  print *, 'E = ', sums(12) + sums(13) + sums(14) + sums(15) + sums(27) + sums(28)
end program energy_caller
""")


@needs_hipcc
def test_energy_kernels_fit_the_register_budget():
    k = resource_usage("energy.hip", containing("energy_"))
    k.update(resource_usage("gravity.hip", containing("grav_potential_wave")))
    for name in ("energy_stage", "energy_box", "energy_pieces", "energy_final", "grav_potential_wave"):
        assert sum(name in n for n in k) == 1, name
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def test_softening_potential_matches_the_force_polynomial():
    q = np.linspace(1e-3, 3.0, 30001)
    h = 1e-6
    dphi = (energy_ref.phi_kernel(q + h) - energy_ref.phi_kernel(q - h)) / (2 * h)    # central difference
    inner = np.abs(q - 1.0) > 2 * h
    inner &= np.abs(q - 2.0) > 2 * h
    # the analytic derivative: q^2 phi'(q) is the grav_table polynomial to 1e-12
    def dphi_exact(q):
        return np.where(q < 1.0, (4 / 3) * q - 1.2 * q**3 + 0.5 * q**4,
                        np.where(q < 2.0, (8 / 3) * q - 3 * q**2 + 1.2 * q**3 - q**4 / 6 - 1 / (15 * q**2), 1 / q**2))
    assert np.max(np.abs(q**2 * dphi_exact(q) - energy_ref.grav_table_poly(q))) <= 1e-12
    assert np.max(np.abs(dphi[inner] - dphi_exact(q[inner]))) <= 1e-6
    for qe in (1.0, 2.0):
        lo, hi = energy_ref.phi_kernel(np.array([np.nextafter(qe, 0.0)])), energy_ref.phi_kernel(np.array([qe]))
        assert abs(lo[0] - hi[0]) <= 1e-14
    assert energy_ref.phi_kernel(np.array([2.0]))[0] == -0.5
    assert abs(energy_ref.phi_kernel(np.array([0.0]))[0] + 1.4) == 0.0


def test_restatement_reproduces_the_fixture_numbers():
    g = load_golden("disc3000_traj")
    G = float(np.float32(39.47841760435743))
    e = {}
    for p, sg in (("sph_s1_", False), ("sph_s5_", False), ("full_s5_", True)):
        gas, sinks = energy_ref.rows_to_dicts(g, p)
        e[p] = energy_ref.totals(energy_ref.energy_sums(gas, sinks, G, 2.5, sg)[0])
    assert f"{e['sph_s1_']['E']:.6e}" == "-5.551292e-03"
    assert f"{e['sph_s5_']['E']:.6e}" == "-5.551265e-03"
    assert abs(e["sph_s5_"]["E"] - e["sph_s1_"]["E"]) / abs(e["sph_s1_"]["E"]) == pytest.approx(5e-6, rel=0.1)
    p0 = e["sph_s1_"]["P"]
    assert np.max(np.abs(e["sph_s5_"]["P"] - p0)) <= 1e-12 * np.max(np.abs(p0))
    assert f"{e['full_s5_']['W_self']:.2e}" == "-7.97e-05"
    assert abs(e["full_s5_"]["P"][2]) == pytest.approx(2e-10, rel=0.05)


def test_cli_parsing(tmp_path, monkeypatch):
    from summersph_amd import energy
    seen = {}

    def fake(gas, sinks, variable=False, self_gravity=True, theta=None, phi=False, device=0):
        seen.update(n=gas.shape[0], ns=sinks.shape[0], variable=variable, sg=self_gravity, theta=theta, phi=phi)
        sums = np.arange(28, dtype=np.float64)
        from summersph_amd import capi
        out = capi.energy_total(sums)
        out["sums"] = sums
        if phi:
            out["phi"] = -np.ones(gas.shape[0])
        return out

    monkeypatch.setattr(energy, "energy_rows", fake)
    save = tmp_path / "s.txt"
    save.write_text("header\n" + "1 2 3 4 5 6 7 8 9\n" * 3 + "0 0 0 0 0 0 0 1\n")
    assert energy.main([str(save), "--json"]) == 0
    assert seen == dict(n=3, ns=1, variable=False, sg=True, theta=None, phi=False)
    assert energy.main([str(save), "--no-self-gravity", "--theta", "0.7", "--phi", str(tmp_path / "p.npy")]) == 0
    assert seen == dict(n=3, ns=1, variable=False, sg=False, theta=0.7, phi=True)
    assert np.array_equal(np.load(tmp_path / "p.npy"), -np.ones(3))
    with pytest.raises(SystemExit):
        energy.main([str(save), "--theta", "-1"])
    from summersph_amd import capi
    d = capi.energy_total(np.arange(28, dtype=np.float64))
    assert d["E"] == 11 + 12 + 13 + 14 + 26 + 27
    assert d["P"].tolist() == [25.0, 27.0, 29.0] and d["L"].tolist() == [31.0, 33.0, 35.0]
