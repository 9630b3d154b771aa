"""CPU tests of the disc profiles (sph_profile): the ABI mirrors (ctypes, Fortran) against the C header, the register
budget of the profile kernels, sph_profile_finish (host code in the library, no device) against the numpy restatement,
the restatement against the analytic Keplerian disc, and the command line's parsing."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import profile_ref

FIELDS = ["centre", "centre_v", "central_mass", "normal", "r_min", "r_max", "z_max", "n_r", "n_phi", "sink", "flags", "reserved"]


def test_profile_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_profile_desc", FIELDS,
                   ['printf("consts %d %d %d %d\\n", SPH_PROFILE_LOG, SPH_PROFILE_AUTO_NORMAL, SPH_PROFILE_NSUM, SPH_PROFILE_NCOL);',
                    'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == ctypes.sizeof(capi.ProfileDesc) == 128
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.ProfileDesc, f).offset, f
    assert got["consts"] == f"{capi.PROFILE_LOG} {capi.PROFILE_AUTO_NORMAL} {capi.PROFILE_NSUM} {capi.PROFILE_NCOL}" == "1 2 20 29"
    assert got["abi"] == "1"
    assert len(capi.PROFILE_COLUMNS) == capi.PROFILE_NCOL == profile_ref.NCOL and capi.PROFILE_COLUMNS == profile_ref.COLUMNS
    assert len(capi.PROFILE_SUMS) == capi.PROFILE_NSUM
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_PROFILE_LOG = 1, SPH_PROFILE_AUTO_NORMAL = 2, SPH_PROFILE_NSUM = 20, SPH_PROFILE_NCOL = 29", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "profile_caller", """program profile_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_profile_desc) :: d
  type(sph_params) :: p
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: sums(:, :), table(:, :)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%centre = 0.0_c_double
  d%centre_v = 0.0_c_double
  d%central_mass = 1.0_c_double
  d%normal = [0.0_c_double, 0.0_c_double, 1.0_c_double]
  d%r_min = 1.0_c_double
  d%r_max = 10.0_c_double
  d%z_max = ieee_value(1.0_c_double, ieee_positive_inf)
  d%n_r = 4
  d%n_phi = 2
  d%sink = -1
  d%flags = SPH_PROFILE_LOG
  d%reserved = 0
  if (c_sizeof(d) /= 128) stop 1
  allocate(sums(SPH_PROFILE_NSUM, 8), table(SPH_PROFILE_NCOL, 8))
  sums = 1.0_c_double
  st = sph_params_default(p)
  st = sph_profile_finish(d, p, sums, table, 8_c_int64_t)
  if (st /= SPH_OK) stop 2
  st = sph_profile(ctx, d, c_loc(sums), c_null_ptr, 8_c_int64_t)
  st = sph_profile_dev(ctx, d, c_null_ptr, 8_c_int64_t)
  print *, st, table(1, 1)
end program profile_caller
""")


@needs_hipcc
def test_profile_kernels_fit_the_register_budget():
    k = resource_usage("profile.hip", containing("profile_"))
    for name in ("profile_keys", "profile_starts", "profile_pieces", "profile_final"):
        assert sum(name in n for n in k) == 1, name
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)             # 4 waves / SIMD by registers


def _finish_both(sums, r0, r1, nr, nphi, log, normal):
    from summersph_amd import capi
    p = capi.default_params()
    d = capi.profile_desc(r0, r1, nr, nphi, log=log, normal=normal)
    t = capi.profile_finish(d, p, sums)
    got = np.stack([t[c] for c in capi.PROFILE_COLUMNS], axis=1)
    want = profile_ref.finish(sums, r0, r1, nr, nphi, log, normal, p.gamma, p.gamma_m1, p.G)
    return got, want


def _agree(got, want, tol=1e-14):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    scale = np.maximum(np.abs(want[ok]), 1e-300)
    assert np.all(np.abs(got[ok] - want[ok]) <= tol * scale + 4e-16 * (np.abs(want[ok]) < 1e-2)), np.max(np.abs(got[ok] - want[ok]) / scale)


def test_finish_matches_the_restatement():
    rng = np.random.default_rng(7)
    for nr, nphi, log, normal in ((6, 1, False, (0, 0, 1)), (5, 4, True, (0.3, -0.2, 1.0)), (3, 2, False, (1.0, 0.2, 0.1))):
        sums = rng.uniform(0.5, 2.0, (nr * nphi, 20))
        sums[:, 0] = np.round(sums[:, 0] * 100)
        sums[:, 6] = rng.uniform(5.0, 6.0, nr * nphi) * sums[:, 1]        # rotation that rises with R: kappa^2 > 0 or < 0
        got, want = _finish_both(sums, 1.5, 20.0, nr, nphi, log, normal)
        _agree(got, want)


def test_finish_edge_cases():
    from summersph_amd import capi
    rng = np.random.default_rng(8)
    sums = rng.uniform(0.5, 2.0, (5, 20))
    sums[2] = 0.0                                                       # an empty ring
    got, want = _finish_both(sums, 1.0, 6.0, 5, 1, False, (0, 0, 1))
    _agree(got, want)
    c = {n: i for i, n in enumerate(capi.PROFILE_COLUMNS)}
    assert got[2, c["N"]] == 0 and got[2, c["M"]] == 0 and got[2, c["Sigma"]] == 0
    for name in ("R_mean", "H", "u_mean", "Omega", "kappa", "Q", "j", "tilt", "ecc", "peri"):
        assert np.isnan(got[2, name and c[name]]), name
    assert np.isnan(got[1, c["kappa"]]) and np.isnan(got[3, c["kappa"]])   # their neighbour is missing
    # kappa^2 < 0: angular momentum falling outwards
    s = np.zeros((3, 20))
    s[:, 0] = s[:, 1] = 1.0
    s[:, 2] = [1.0, 2.0, 3.0]
    s[:, 6] = [3.0, 1.0, 0.2]
    got, want = _finish_both(s, 0.5, 3.5, 3, 1, False, (0, 0, 1))
    _agree(got, want)
    assert np.all(np.isnan(got[:, c["kappa"]])) and np.all(np.isnan(got[:, c["Q"]]))
    # one ring: no neighbours for kappa
    got, want = _finish_both(rng.uniform(0.5, 2.0, (1, 20)), 1.0, 2.0, 1, 1, False, (0, 0, 1))
    _agree(got, want)
    assert np.isnan(got[0, c["kappa"]]) and np.isfinite(got[0, c["Sigma"]])


def test_finish_refuses_bad_arguments():
    from summersph_amd import capi
    p = capi.default_params()
    sums = np.zeros((4, 20))
    for kw in (dict(n_r=4, n_phi=2), dict(n_r=4, r_min=5.0, r_max=5.0), dict(n_r=4, normal=(0, 0, 0)),
               dict(n_r=4, r_min=0.0, log=True)):
        a = dict(r_min=1.0, r_max=5.0); a.update(kw)
        with pytest.raises(capi.SphError):
            capi.profile_finish(capi.profile_desc(**a), p, sums)


def test_restatement_recovers_the_keplerian_disc():
    from summersph_amd import capi, ic
    n, r_in, m_disc = 200_000, 10.0, 0.01
    rows = ic.keplerian_disc(n, seed=3, r_in=r_in, m_disc=m_disc)
    gas, sinks = ic.split_rows(rows)
    r_out = float(np.max(np.hypot(gas["x"], gas["y"])))
    p = capi.default_params()
    G = ic.G_DP
    nr = 40
    r0, r1 = r_in, r_out * (1 - 1e-9)
    sums, _ = profile_ref.profile_sums(gas, p.h, G, r0, r1, nr, 1, True, np.inf, (0, 0, 0), (0, 0, 0), 1.0)
    t = profile_ref.finish(sums, r0, r1, nr, 1, True, (0, 0, 1), p.gamma, p.gamma_m1, G)
    c = {name: i for i, name in enumerate(profile_ref.COLUMNS)}
    sigma0 = m_disc / (math.pi * (r_out ** 2 - r_in ** 2))
    N = t[:, c["N"]]
    assert np.all(np.abs(t[:, c["Sigma"]] / sigma0 - 1) < 5 / np.sqrt(N))          # Poisson noise
    R = t[:, c["R_mean"]]
    assert np.max(np.abs(t[:, c["Omega"]] / np.sqrt(G * 1.0 / R ** 3) - 1)) < 1e-3
    kk = t[:, c["kappa"]] / t[:, c["Omega"]]
    assert np.max(np.abs(kk - 1)) < 1e-2                                             # bin-width bias of the differences
    assert np.all(np.abs(t[:, c["H"]] / 2.5 - 1) < 5 / np.sqrt(2 * N))               # sampling noise of a Gaussian width
    # the orbits are circular in the midplane (v = v_K(R) at height z is not a circular 3-D orbit): e of the flat disc
    flat = dict(gas); flat["z"] = np.zeros_like(gas["z"])
    sf, _ = profile_ref.profile_sums(flat, p.h, G, r0, r1, nr, 1, True, np.inf, (0, 0, 0), (0, 0, 0), 1.0)
    tf = profile_ref.finish(sf, r0, r1, nr, 1, True, (0, 0, 1), p.gamma, p.gamma_m1, G)
    assert np.max(tf[:, c["ecc"]]) < 1e-6


def test_cli_parses_centre_and_normal_specs(tmp_path, monkeypatch):
    from summersph_amd import capi, profile
    assert profile.parse_centre("sink:0") == ("sink", 0)
    assert profile.parse_centre("sink:3") == ("sink", 3)
    assert profile.parse_centre("1,-2.5,3e2") == ("point", (1.0, -2.5, 300.0))
    assert profile.parse_normal("auto") == "auto"
    assert profile.parse_normal("0,1,1") == (0.0, 1.0, 1.0)
    for bad in ("sink:", "sink:-1", "sink:x", "1,2", "a,b,c", "1,2,nan", ""):
        with pytest.raises(ValueError):
            profile.parse_centre(bad)
    for bad in ("0,0,0", "1,2", "automatic", "inf,0,1"):
        with pytest.raises(ValueError):
            profile.parse_normal(bad)

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    monkeypatch.setattr(profile, "read_save", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the save file was read")))
    base = ["missing.txt", "-o", str(tmp_path / "o.npz"), "--rmin", "1", "--rmax", "5", "--bins", "4"]
    for extra in (["--centre", "sink:-1"], ["--centre", "1,2"], ["--normal", "0,0,0"], ["--normal", "up"], ["--bins", "0"],
                  ["--rmin", "6"], ["--rmin", "0", "--log"], ["--nphi", "0"]):
        with pytest.raises(SystemExit) as e:
            profile.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
