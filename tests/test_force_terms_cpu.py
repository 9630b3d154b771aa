"""CPU: the restatement of sph_force_terms (tests/force_terms_ref.py) pinned to the oracles, the construction conditions of
the sets tests/test_force_terms_gpu.py runs (tests/force_terms_sets.py), the numpy helpers and the command line of
summersph_amd.terms, and the binding.

The bar between the restatement's recomposed rows and the oracles' totals is varh_ref.rate_excess, the project's bar for
rates: 1e-11 of the element's magnitude plus 1e-13 of the summed scales of the rows involved.  Both sides are CPU
references; the shares of that bar they use are printed (measured: fixed-h sets <= 2.6e-3, variable-h sets <= 1.5e-3)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, fortran_links, library, needs_fc
import force_terms_ref as FR
import force_terms_sets as TS
import varh_ref as VR
from conftest import ROOT, load_golden

TOTALS = ("ax", "ay", "az", "du", "dalpha")


def _shares(tag, got, want, scales):
    worst = {}
    for f, g, w, s in zip(TOTALS, got, want, scales):
        worst[f] = float(np.max(VR.rate_excess(np.abs(g - w), np.abs(w), s))) if g.size else 0.0
    print(f"{tag}: share of the rate bar used: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for f, v in worst.items():
        assert v <= 1.0, (tag, f, v)


# ---- 1. the restatement against the oracles ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["disc3000_eval", "sod1000_eval", "bin2000_eval"])
def test_fixed_restatement_recomposes_to_the_oracle(name):
    from oracle import orc
    from summersph_amd import ic
    gas, sinks = ic.split_rows(load_golden(name)["ic"])
    gas = {k: np.array(v, dtype=np.float64) for k, v in gas.items()}
    gas["alpha"] = np.random.default_rng(7).uniform(0.05, 1.0, gas["x"].size)        # the reader's alpha is 0: no viscosity
    t = FR.fixed_terms(gas, sinks)
    o = orc.Oracle(gas, sinks, nthreads=orc.max_threads())
    o.evaluate()
    got, scales = t.recomposed()
    assert np.all(t.rows[FR.A_G] == 0.0)
    _shares(name, got, [getattr(o, f) for f in TOTALS], scales)
    assert np.all(t.rows[FR.DU_V] >= 0.0) and t.min_pair_duV >= 0.0               # every pair term of the heating is >= 0
    assert np.any(t.rows[FR.DU_V] > 0.0) == (t.n_approaching > 0)                 # (the Sod column starts at rest)


def test_variable_restatement_recomposes_to_the_oracle_on_discv3000():
    from oracle import orc, orc_v
    gas, sinks, ref, t = TS.variable_case("discv3000")
    o = orc_v.OracleV(gas, sinks, nthreads=orc.max_threads())
    o.evaluate()
    got, scales = t.recomposed()
    _shares("discv3000", got, [getattr(o, f) for f in TOTALS], scales)


@pytest.mark.parametrize("name", ["clump_in_halo", "h_routes"])
def test_variable_restatement_recomposes_to_varh_ref(name):
    gas, sinks, ref, t = TS.variable_case(name)
    assert sinks is None and np.all(t.rows[FR.A_S] == 0.0)
    ref.forces()
    got, scales = t.recomposed()
    _shares(name, got, [getattr(ref, f) for f in TOTALS], scales)


# ---- 2. what the sets are built to have ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TS.FIXED)
def test_fixed_set_construction(name):
    gas, sinks, t = TS.fixed_case(name)
    n = gas["x"].size
    assert n <= 4000 and not np.any(np.isnan(t.rows))
    if n >= 3:
        assert t.n_approaching > 0 and t.n_receding > 0, name
    elif n == 2:
        assert t.n_pairs == 1 and t.n_approaching == 1 and t.rows[FR.DU_V][0] > 0.0      # one pair, approaching: viscosity on
    assert t.n_coincident == (1 if name in TS.HAS_COINCIDENT else 0)
    assert int(np.count_nonzero(t.list_len == 0)) == TS.HAS_EMPTY_LIST.get(name, 0), name
    if name in ("n63", "n64", "n65"):
        assert n == int(name[1:])
    if name == "disc2":
        assert np.asarray(sinks["x"]).size == 2 and np.all(np.asarray(sinks["m"]) > 0.0)
    if name == "inside_2h":
        r = np.sqrt((gas["x"][11] - gas["x"][10]) ** 2 + (gas["y"][11] - gas["y"][10]) ** 2 + (gas["z"][11] - gas["z"][10]) ** 2)
        assert r == 2.0 * TS.H * (1.0 - 1e-9) and 0.0 < r < 2.0 * TS.H
    if name == "isolated":
        lone = int(np.flatnonzero(t.list_len == 0)[0])
        for k in list(range(0, 6)) + [FR.DU_P, FR.DU_V, FR.AL_SRC]:
            assert t.rows[k][lone] == 0.0
        assert np.any(t.rows[FR.A_S][:, lone] != 0.0)                                   # sink gravity only
    if name == "far_clump_fixed":
        assert int(t.list_len.max()) > TS.INIT_LIST_SLOTS                                # the list has to grow
        assert np.count_nonzero(t.list_len > TS.INIT_LIST_SLOTS) >= 64                   # ... for more than a wave of targets


@pytest.mark.parametrize("name", TS.VARIABLE)
def test_variable_set_construction(name):
    gas, sinks, ref, t = TS.variable_case(name)
    assert ref.n <= 4000 and not np.any(np.isnan(t.rows))
    assert t.n_approaching > 0 and t.n_receding > 0
    n_coinc = (int(np.count_nonzero(ref.r == 0.0)) - ref.n) // 2
    assert (n_coinc >= 1) == (name in TS.HAS_COINCIDENT)
    # the list's entries are not all alike: force pairs outside the target's own density set (r > 2 h_i, or a leaf its walk
    # does not reach) exist, so an entry's flags decide what it counts for
    off = ~np.eye(ref.n, dtype=bool)
    assert np.count_nonzero(ref.in_F & ~ref.in_D & off) > 0, name
    if name == "clump_in_halo":
        assert ref.n_asym_pairs > 0


# ---- 3. summersph_amd.terms -----------------------------------------------------------------------------------------------
def _handmade():
    # five particles on the x axis at R = 1, 2, 3, 4 and 10 (the last outside every ring), one ghost column (NaN)
    x = np.array([1.0, 2.0, 3.0, 4.0, 10.0, 2.5])
    state = {"x": x, "y": np.zeros(6), "z": np.zeros(6), "vx": np.zeros(6), "vy": np.array([1.0, 1.0, 2.0, 2.0, 1.0, 1.0]),
             "vz": np.zeros(6), "m": np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])}
    rows = np.zeros((16, 6))
    rows[1] = [1.0, 1.0, 1.0, 1.0, 1.0, 0.0]          # a_P = y^: torque_z = m x
    rows[3] = [0.5, 0.0, 0.0, 0.0, 0.0, 0.0]          # a_V = x^/2 on particle 0: no torque
    rows[7] = -1.0                                    # a_S = -y^
    rows[12] = [0.1, 0.2, 0.3, 0.4, 0.5, 0.0]
    rows[13] = [1.0, 0.0, 2.0, 0.0, 3.0, 0.0]
    rows[:, 5] = np.nan
    return state, rows


def test_totals_on_handmade_rows():
    from summersph_amd import terms
    state, rows = _handmade()
    t = terms.totals(state, rows)
    m, x, vy = state["m"][:5], state["x"][:5], state["vy"][:5]
    assert np.allclose(t["force"], [[0, m.sum(), 0], [0.5, 0, 0], [0, -m.sum(), 0], [0, 0, 0]], rtol=0, atol=1e-15)
    assert np.allclose(t["torque"][:, 2], [(m * x).sum(), 0.0, -(m * x).sum(), 0.0], rtol=0, atol=1e-15)
    assert np.allclose(t["power"], [(m * vy).sum(), 0.0, -(m * vy).sum(), 0.0], rtol=0, atol=1e-15)
    assert t["du_P"] == pytest.approx((m * rows[12][:5]).sum(), abs=1e-15) and t["du_V"] == pytest.approx(1.0 + 6.0 + 15.0, abs=1e-15)
    # about another centre: r' = r - c
    t2 = terms.totals(state, rows, centre=(1.0, 0.0, 0.0))
    assert np.allclose(t2["torque"][0, 2], (m * (x - 1.0)).sum(), rtol=0, atol=1e-15)
    # a term whose rows are NaN for the targets (skip_gas_gravity) sums to NaN, the others do not
    rows[9:12, :5] = np.nan
    t3 = terms.totals(state, rows)
    assert np.all(np.isnan(t3["force"][3])) and np.all(np.isfinite(t3["force"][:3]))


def test_rings_line_up_with_profile_edges_and_an_empty_ring():
    import profile_ref as PR
    from summersph_amd import terms
    state, rows = _handmade()
    for log in (False, True):
        e = terms.ring_edges(0.5, 8.5, 4, log=log)
        assert np.array_equal(e, PR.edges(0.5, 8.5, 4, log=log))
    e = terms.ring_edges(0.5, 8.5, 4)                 # [0.5, 2.5), [2.5, 4.5), [4.5, 6.5) (empty), [6.5, 8.5) (empty)
    ring = terms.ring_index(state, e)
    assert list(ring) == [0, 0, 1, 1, -1, 1]
    pos = np.stack([state["x"], state["y"], state["z"]], axis=1)
    fr = PR.frame(pos, np.zeros_like(pos), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    assert np.array_equal(ring, PR.bins(fr, 0.5, 8.5, 4))
    tq = terms.ring_torques(state, rows, e)
    assert tq.shape == (4, 4)
    assert np.allclose(tq[0], [1 * 1 + 2 * 2, 3 * 3 + 4 * 4, 0.0, 0.0]) and np.allclose(tq[2], -tq[0]) and np.all(tq[1] == 0.0)
    ht = terms.ring_heating(state, rows, e)
    assert ht.shape == (2, 4) and np.allclose(ht[0], [1.0, 6.0, 0.0, 0.0]) and np.allclose(ht[1], [0.1 + 0.4, 0.9 + 1.6, 0.0, 0.0])
    # an edge belongs to the ring above it; a tilted normal uses sph_profile's frame
    state["x"][0] = 2.5
    assert terms.ring_index(state, e)[0] == 1
    tq_t = terms.ring_torques(state, rows, e, normal=(0.0, 0.0, -2.0))
    assert np.allclose(tq_t[0], -terms.ring_torques(state, rows, e)[0])
    with pytest.raises(ValueError):
        terms.ring_edges(0.0, 1.0, 4, log=True)


@pytest.mark.parametrize("argv", [["save.txt"], ["save.txt", "-o", "o.npz", "--rings", "1", "0.5", "4"],
                                  ["save.txt", "-o", "o.npz", "--rings", "0", "5", "4", "--log"],
                                  ["save.txt", "-o", "o.npz", "--log"], ["save.txt", "-o", "o.npz", "--normal", "0,0,0"],
                                  ["save.txt", "-o", "o.npz", "--centre", "1,2"], ["save.txt", "-o", "o.npz", "--rings", "1", "5", "0"]])
def test_command_line_argument_errors(argv, capsys):
    from summersph_amd import terms
    with pytest.raises(SystemExit) as e:
        terms.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_command_line_arguments():
    from summersph_amd import terms
    a = terms.parse_args(["s.txt", "-o", "o.npz", "--json", "--rings", "5", "50", "9", "--log", "--no-gravity", "--variable"])
    assert a.json and a.no_gravity and a.variable and a.edges.size == 10 and a.edges[0] == 5.0 and a.edges[-1] == 50.0


# ---- 4. the binding ---------------------------------------------------------------------------------------------------------
def test_descriptor_layout_rows_and_symbols(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_force_terms_desc", ["flags", "reserved"],
                   ['printf("consts %d %d\\n", SPH_TERMS_NROW, SPH_TERMS_SKIP_GAS_GRAVITY);', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == C.sizeof(capi.ForceTermsDesc) == 16
    assert int(got["flags"]) == capi.ForceTermsDesc.flags.offset == 0
    assert int(got["reserved"]) == capi.ForceTermsDesc.reserved.offset == 4
    assert got["consts"] == f"{capi.TERMS_NROW} {capi.TERMS_SKIP_GAS_GRAVITY}" == "16 1"
    assert got["abi"] == "1"                                        # the change is additive
    assert len(capi.TERM_ROWS) == 16 == FR.NROW and capi.TERM_ROWS[12:] == ["du_P", "du_V", "dalpha_source", "dalpha_decay"]
    assert "sph_force_terms" in capi.SYMBOLS and "sph_force_terms_dev" in capi.SYMBOLS
    lib = C.CDLL(library())
    for s in ("sph_force_terms", "sph_force_terms_dev"):
        assert hasattr(lib, s), s
    assert lib.sph_abi_version() == 1
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_TERMS_NROW = 16, SPH_TERMS_SKIP_GAS_GRAVITY = 1", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "terms_caller", """program terms_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_force_terms_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: out(:, :)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%flags = SPH_TERMS_SKIP_GAS_GRAVITY
  d%reserved = 0
  if (c_sizeof(d) /= 16) stop 1
  allocate(out(10, SPH_TERMS_NROW))
  st = sph_force_terms(ctx, d, c_loc(out), 160_c_int64_t)
  st = sph_force_terms_dev(ctx, d, c_null_ptr, 0_c_int64_t)
  print *, st
end program terms_caller
""")
