"""CPU tests of the binding energies (sph_bound): the ABI mirrors (ctypes, Fortran) against the C header, the register
budget of the bound kernels, the numpy restatement against closed forms and a hand-made four-particle set, and the
command line's parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import bound_ref

FIELDS = ["h", "soft2", "min_members", "max_members", "max_rounds", "flags", "reserved"]


def test_bound_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_bound_desc", FIELDS,
                   ['printf("consts %d %d %d\\n", SPH_BOUND_THERMAL, SPH_BOUND_NCOL, SPH_ABI_VERSION);'])
    assert int(got["size"]) == ctypes.sizeof(capi.BoundDesc) == 48
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.BoundDesc, f).offset, f
    assert got["consts"] == f"{capi.BOUND_THERMAL} {capi.BOUND_NCOL} 1" == "1 24 1"
    assert capi.BOUND_COLUMNS == bound_ref.COLUMNS and len(capi.BOUND_COLUMNS) == capi.BOUND_NCOL == bound_ref.NCOL
    assert "sph_bound" in capi.SYMBOLS and "sph_bound_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_BOUND_THERMAL = 1, SPH_BOUND_NCOL = 24", binding)
    d = capi.bound_desc(h=0.5, soft2=0.0, thermal=True, max_rounds=7, min_members=3, max_members=1000)
    assert (d.h, d.soft2, d.min_members, d.max_members, d.max_rounds, d.flags) == (0.5, 0.0, 3, 1000, 7, 1)
    assert list(d.reserved) == [0, 0]
    d = capi.bound_desc()
    assert (d.h, d.soft2, d.min_members, d.max_members, d.max_rounds, d.flags) == (0.0, 0.001 * 2.5, 1, 2**31 - 1, 0, 0)
    t = capi.bound_table(np.arange(48.0).reshape(2, 24))
    assert t["N0"].tolist() == [0.0, 24.0] and t["e_most_bound"].tolist() == [23.0, 47.0]


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "bound_caller", """program bound_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_bound_desc) :: d
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable, target :: labels(:), bound_labels(:)
  real(c_double), allocatable, target :: out(:, :), table(:, :)
  integer(c_int64_t), target :: counts(4)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%h = 0.0_c_double
  d%soft2 = 0.0025_c_double
  d%min_members = 2_c_int64_t
  d%max_members = 100000_c_int64_t
  d%max_rounds = 16
  d%flags = SPH_BOUND_THERMAL
  d%reserved = 0
  if (c_sizeof(d) /= 48) stop 1
  allocate(labels(10), bound_labels(10), out(10, 2), table(SPH_BOUND_NCOL, 4))
  labels = -1
  st = sph_bound(ctx, d, c_loc(labels), 10_c_int64_t, 4_c_int64_t, c_loc(bound_labels), c_loc(out), 20_c_int64_t, &
                 c_loc(table), c_loc(counts))
  st = sph_bound_dev(ctx, d, c_null_ptr, 0_c_int64_t, 0_c_int64_t, c_null_ptr, c_null_ptr, 0_c_int64_t, c_null_ptr, c_null_ptr)
  print *, st
end program bound_caller
""")


@needs_hipcc
def test_bound_kernels_fit_the_register_budget():
    k = resource_usage("bound.hip", containing("bound_"))
    for name in ("bound_fill", "bound_keys", "bound_starts", "bound_gather", "bound_init", "bound_momE", "bound_mom_final",
                 "bound_plan", "bound_pairs", "bound_sumsE", "bound_sums_final", "bound_scatter", "bound_counts"):
        assert sum(name in n for n in k) == 1, name
    assert len(k) == 13
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def _two(v_rel, m1=0.3, m2=0.7, r=1.0, G=2.0):
    """two bodies r apart on the x axis, relative velocity v_rel along y, moving with a common bulk velocity"""
    bulk = np.array([3.0, -1.0, 0.5])
    v1 = bulk + np.array([0.0, v_rel * m2 / (m1 + m2), 0.0])
    v2 = bulk - np.array([0.0, v_rel * m1 / (m1 + m2), 0.0])
    return {"x": np.array([5.0, 5.0 + r]), "y": np.array([1.0, 1.0]), "z": np.array([-2.0, -2.0]),
            "vx": np.array([v1[0], v2[0]]), "vy": np.array([v1[1], v2[1]]), "vz": np.array([v1[2], v2[2]]),
            "u": np.array([7.0, 9.0]), "m": np.array([m1, m2])}


def test_restatement_two_bodies_closed_form():
    G, m1, m2, r = 2.0, 0.3, 0.7, 1.0
    lab = np.zeros(2, dtype=np.int32)
    f = _two(0.1)
    bl, e, phi, t, cnt, _ = bound_ref.bound(f, lab, 2, 1, G, 0.4, soft2=0.0)       # r > 2 h: the Newtonian potential
    assert np.allclose(phi, [-G * m2 / r, -G * m1 / r], rtol=4e-16, atol=0)
    assert abs(t[0, 4] + G * m1 * m2 / r) <= 4e-16 * G * m1 * m2 / r                   # W = -G m1 m2 / r
    assert np.allclose(t[0, 12:15], [3.0, -1.0, 0.5], rtol=1e-15) and np.allclose(t[0, 9:12], [5.7, 1.0, -2.0], rtol=1e-15)
    assert t[0, 1] == 1.0 and t[0, 0] == 2 and t[0, 3] == m1 * 7.0 + m2 * 9.0
    assert cnt == [2, 0, 0, 0] and bl.tolist() == [0, 0] and t[0, 21] == 0 and t[0, 19] == 2
    # body 1 moves at v_rel m2 / M in the pair's frame: unbound exactly when 0.5 (v_rel m2 / M)^2 exceeds G m2 / r
    v1_crit = np.sqrt(2 * G * m2 / r)                       # its critical speed
    for fac, bound1 in ((0.999999, True), (1.000001, False)):
        f = _two(fac * v1_crit * (m1 + m2) / m2)
        bl, e, phi, t, cnt, _ = bound_ref.bound(f, lab, 2, 1, G, 0.4, soft2=0.0)
        assert (e[0] < 0) == bound1 and (bl[0] == 0) == bound1
        assert abs(e[0] - (0.5 * (fac * v1_crit) ** 2 - G * m2 / r)) <= 1e-14 * G * m2 / r
    # thermal: u_i joins e_i and U joins E
    f = _two(0.1)
    _, e_t, _, t_t, _, _ = bound_ref.bound(f, lab, 2, 1, G, 0.4, soft2=0.0, thermal=True)
    _, e_0, _, t_0, _, _ = bound_ref.bound(f, lab, 2, 1, G, 0.4, soft2=0.0)
    assert np.allclose(e_t - e_0, [7.0, 9.0], rtol=1e-14) and abs((t_t[0, 5] - t_0[0, 5]) - t_0[0, 3]) < 1e-14
    # inside the softening: two coincident bodies see phi(0) = -1.4
    f = _two(0.0, r=0.0)
    _, _, phi, _, _, _ = bound_ref.bound(f, lab, 2, 1, G, 0.4, soft2=0.0, check_margin=False)
    assert np.allclose(phi, [-1.4 * G * m2 / 0.4, -1.4 * G * m1 / 0.4], rtol=1e-15)


def _four():
    """A and B: a cold pair; C: light, bound only while D is in the set; D: fast, unbound at once (G = 1, all separations
    beyond 2 h)"""
    return {"x": np.array([0.0, 1.0, 0.0, 0.0]), "y": np.array([0.0, 0.0, 1.5, 3.0]), "z": np.zeros(4),
            "vx": np.array([0.0, 0.0, 1.65, 0.0]), "vy": np.zeros(4), "vz": np.array([0.0, 0.0, 0.748, 3.0]),
            "u": np.full(4, 0.01), "m": np.array([1.0, 1.0, 0.01, 1.0])}


def test_restatement_round_rule_on_four_particles():
    f = _four()
    lab = np.zeros(4, dtype=np.int32)
    kw = dict(G=1.0, h=0.1, soft2=0.0)
    bl, e, phi, t, cnt, info = bound_ref.bound(f, lab, 4, 1, max_rounds=5, **kw)
    assert info["evaluations"][0] == 3 and t[0, 20] == 2 and t[0, 21] == 0           # D leaves, then C, then converged
    assert bl.tolist() == [0, 0, -1, -1] and t[0, 0] == 4 and t[0, 7] == 2 and t[0, 19] == 2
    assert e[3] > 0 and e[2] > 0 and e[0] < 0 and e[1] < 0
    assert abs(phi[3] + (1 / 3.0 + 1 / np.sqrt(10.0) + 0.01 / 1.5)) < 1e-15          # D's Phi: of the first evaluation
    assert abs(phi[2] + (1 / 1.5 + 1 / np.sqrt(3.25))) < 1e-15                       # C's: of the second, D gone
    assert abs(phi[0] + 1.0) < 1e-15 and abs(t[0, 17] + 1.0) < 1e-15 and t[0, 8] == 2.0   # the pair alone
    assert abs(t[0, 4] + (1.0 + 1 / 3.0 + 1 / np.sqrt(10.0) + 0.01 * (1 / 1.5 + 1 / np.sqrt(3.25) + 1 / 1.5))) < 1e-14
    assert t[0, 22] in (0, 1) and cnt == [4, 0, 0, 0]
    # no removal allowed: one evaluation, column 19 counts the e < 0 members of S_0
    bl, e, _, t, cnt, info = bound_ref.bound(f, lab, 4, 1, max_rounds=0, **kw)
    assert info["evaluations"][0] == 1 and t[0, 20] == 0 and t[0, 21] == 1 and t[0, 7] == 4 and t[0, 19] == 3
    assert bl.tolist() == [0, 0, 0, -1] and cnt == [4, 0, 0, 1]
    bl, _, _, t, cnt, _ = bound_ref.bound(f, lab, 4, 1, max_rounds=1, **kw)
    assert t[0, 20] == 1 and t[0, 21] == 1 and t[0, 7] == 3 and t[0, 19] == 2 and bl.tolist() == [0, 0, -1, -1]
    # the set falls below min_members when C leaves: dissolved after the second evaluation
    bl, e, _, t, cnt, info = bound_ref.bound(f, lab, 4, 1, max_rounds=5, min_members=3, **kw)
    assert info["evaluations"][0] == 2 and t[0, 21] == 2 and t[0, 20] == 1 and cnt == [4, 0, 1, 0]
    assert np.all(bl == -1) and t[0, 7] == 0 and t[0, 8] == 0 and t[0, 19] == 0 and t[0, 22] == -1
    assert np.all(np.isnan(t[0, 9:19])) and np.isnan(t[0, 23]) and t[0, 0] == 4 and np.isfinite(t[0, 4])
    assert np.all(np.isfinite(e))
    # the caps, labels outside 0 .. n_groups - 1, ghosts
    bl, e, _, t, cnt, _ = bound_ref.bound(f, lab, 4, 1, max_members=3, **kw)
    assert t[0, 21] == 3 and t[0, 0] == 4 and np.all(np.isnan(t[0, 1:21])) and np.all(np.isnan(e)) and cnt == [4, 1, 0, 0]
    bl, e, _, t, cnt, _ = bound_ref.bound(f, np.array([0, 0, 5, -1], dtype=np.int32), 4, 2, max_rounds=5, **kw)
    assert cnt == [2, 0, 1, 0] and bl.tolist() == [0, 0, -1, -1] and t[0, 7] == 2 and t[1, 0] == 0 and t[1, 21] == 2
    assert np.isnan(e[2]) and np.isnan(e[3])
    bl, e, _, t, cnt, _ = bound_ref.bound(f, lab, 2, 1, max_rounds=5, **kw)              # C and D are ghosts
    assert cnt == [2, 0, 0, 0] and t[0, 0] == 2 and t[0, 20] == 0 and bl.tolist() == [0, 0, -1, -1]


def test_restatement_refuses_a_marginal_member():
    v1_crit = np.sqrt(2 * 2.0 * 0.7 / 1.0)                  # body 1's critical speed in the pair's frame
    f = _two((1 + 1e-12) * v1_crit * (0.3 + 0.7) / 0.7)
    with pytest.raises(AssertionError):
        bound_ref.bound(f, np.zeros(2, dtype=np.int32), 2, 1, 2.0, 0.4, soft2=0.0)


def test_blob_set_meets_the_precondition():
    G = float(np.float32(39.47841760435743))
    gas, _, lab, n_owned, ng = bound_ref.blob_set(G)
    assert ng == 12 and n_owned == gas["x"].size - bound_ref.N_GHOST
    mem = bound_ref.members(gas, lab, n_owned, ng)
    assert [m.size for m in mem] == list(bound_ref.SIZES)
    assert np.any(lab[n_owned:] >= 0) and np.any(lab[:n_owned] == -1) and np.any(lab[:n_owned] >= ng)
    _, _, _, t, cnt, info = bound_ref.bound(gas, lab, n_owned, ng, G, 0.3, max_rounds=16)
    assert info["margin"] > 1e-6
    kinds = np.array(bound_ref.KINDS)
    assert np.all(t[kinds == "cold", 20][1:] == 0) and np.all(t[kinds == "cold", 21][1:] == 0)
    assert np.all(t[kinds == "hot", 21] == 2) and np.max(t[kinds == "halo", 20]) >= 3


def test_cli_parses_bound_options_and_refuses_bad_ones(tmp_path, monkeypatch):
    from summersph_amd import capi, groups

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    monkeypatch.setattr(groups, "read_save", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the save file was read")))
    base = ["missing.txt", "-o", str(tmp_path / "o.npz"), "--link", "1"]
    for extra in (["--thermal"], ["--unbind", "3"], ["--bound-h", "0.5"], ["--max-members", "10"],
                  ["--bound", "--unbind", "-1"], ["--bound", "--max-members", "0"], ["--bound", "--bound-h", "0"],
                  ["--bound", "--bound-h", "-1"], ["--bound", "--bound-h", "nan"], ["--bound", "--bound-h", "inf"],
                  ["--bound", "--unbind", "x"], ["--bound", "--min-members", "0"]):
        with pytest.raises(SystemExit) as e:
            groups.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
    # good options reach the reading of the save file, with the descriptor's values
    seen = {}

    def rows(gas, sinks, link, rho_min, min_members, link_h, clip, variable, device, bound):
        seen.update(bound or {}, asked=bound is not None)
        raise KeyboardInterrupt
    monkeypatch.setattr(groups, "read_save", lambda *a, **k: (np.zeros((0, 9)), np.zeros((0, 8))))
    monkeypatch.setattr(groups, "groups_rows", rows)
    with pytest.raises(KeyboardInterrupt):
        groups.main(base + ["--bound", "--thermal", "--unbind", "8", "--bound-h", "0.25", "--max-members", "5000",
                            "--min-members", "4"])
    assert seen == {"asked": True, "h": 0.25, "thermal": True, "max_rounds": 8, "min_members": 4, "max_members": 5000}
    seen.clear()
    with pytest.raises(KeyboardInterrupt):
        groups.main(base)
    assert seen == {"asked": False}
