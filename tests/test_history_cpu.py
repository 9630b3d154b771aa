"""CPU tests of the per-step time series (sph_history): the ABI mirrors (ctypes, Fortran) against the C header, the resources
of the kernels, HistoryDesc's marshalling and every argument error that needs no device, the command line's parsing, and
the numpy restatement (tests/history_ref.py): its exact sums do not depend on the order and stay within N 2^(e - 63) of
math.fsum."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, library, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT, load_golden
import history_ref
from summersph_amd import ic

FIELDS = ["capacity", "every", "max_sinks", "flags"]
SPH_ERR_ARG = 1
CALLS = ["sph_history_begin", "sph_history_end", "sph_history_record", "sph_history_info", "sph_history_read",
         "sph_history_read_dev"]


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    library()
    m.load()
    return m


# ---- 1. the ABI mirrors ----------------------------------------------------------------------------------------------------------
def test_descriptor_layout_constants_and_symbols(capi, tmp_path):
    got = c_layout(tmp_path, "sph_history_desc", FIELDS,
                   ['printf("nhead %d\\n", SPH_HISTORY_NHEAD);', 'printf("abi %d\\n", SPH_ABI_VERSION);',
                    'printf("nsum %d\\n", SPH_ENERGY_NSUM);'])
    assert int(got["size"]) == C.sizeof(capi.HistoryDesc) == 16
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.HistoryDesc, f).offset, f
    assert int(got["nhead"]) == capi.HISTORY_NHEAD == history_ref.NHEAD == len(capi.HISTORY_COLUMNS) == 40
    assert got["abi"] == "1"                                        # the change is additive
    # the row's layout: the six leading columns, sph_energy's sums at 6, the six trailing columns
    assert capi.HISTORY_COLUMNS[:6] == ["step", "t", "dt_next", "dt_cand", "n", "ns"]
    assert capi.HISTORY_COLUMNS[6:6 + int(got["nsum"])] == capi.ENERGY_SUMS
    assert capi.HISTORY_COLUMNS[34:] == ["rho_max", "densest", "densest_x", "densest_y", "densest_z", "v_max"]
    assert capi.history_width(0) == 40 and capi.history_width(64) == 40 + 7 * 64
    lib = C.CDLL(library())
    for s in CALLS:
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_HISTORY_NHEAD = 40", binding)
    for s in CALLS:
        assert re.search(rf"bind\(C, name='{s}'\)", binding), s


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "history_caller", """program history_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_history_desc) :: d
  type(c_ptr) :: ctx
  integer(c_int64_t), target :: rows, dropped, steps
  integer(c_int32_t), target :: width
  real(c_double), allocatable, target :: buf(:, :)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%capacity = 16
  d%every = 2
  d%max_sinks = 1
  d%flags = 0
  if (c_sizeof(d) /= 16) stop 1
  allocate(buf(SPH_HISTORY_NHEAD + 7, 16))
  st = sph_history_begin(ctx, d)
  if (st == SPH_OK) stop 2
  st = sph_history_record(ctx)
  st = sph_history_info(ctx, c_loc(rows), c_loc(dropped), c_loc(steps), c_loc(width))
  st = sph_history_read(ctx, 0_c_int64_t, 16_c_int64_t, c_loc(buf))
  st = sph_history_read_dev(ctx, 0_c_int64_t, 16_c_int64_t, c_null_ptr)
  st = sph_history_end(ctx)
  if (st == SPH_OK) stop 3
  print *, st
end program history_caller
""")


# ---- 2. the kernels' resources -------------------------------------------------------------------------------------------------
@needs_hipcc
def test_history_kernels_fit_the_register_budget():
    k = resource_usage("history.hip", containing("history_"))
    for name in ("history_maxima", "history_head", "history_sums", "history_row"):
        assert sum(name in n for n in k) == 1, (name, sorted(k))
    assert len(k) == 4
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)
        if "history_sums" in name:                                  # 13 {lo, hi} accumulators per lane and still 4 waves
            assert r.get("Occupancy") >= 4, (name, r)


# ---- 3. marshalling and the refusals -----------------------------------------------------------------------------------------------
def test_desc_marshalling_and_argument_errors(capi):
    d = capi.history_desc(100, every=3, max_sinks=2)
    assert (d.capacity, d.every, d.max_sinks, d.flags) == (100, 3, 2, 0)
    d = capi.history_desc(1)
    assert (d.capacity, d.every, d.max_sinks) == (1, 1, 0)
    for bad in (dict(capacity=0), dict(capacity=-1), dict(capacity=2**31), dict(capacity=4, every=0),
                dict(capacity=4, every=-2), dict(capacity=4, max_sinks=-1), dict(capacity=4, max_sinks=65)):
        with pytest.raises(ValueError):
            capi.history_desc(**bad)
    # every call refuses a null context before anything else
    lib = capi.load()
    out = np.zeros(40)
    assert lib.sph_history_begin(None, C.byref(d)) == SPH_ERR_ARG
    assert lib.sph_history_end(None) == SPH_ERR_ARG and lib.sph_history_record(None) == SPH_ERR_ARG
    assert lib.sph_history_info(None, None, None, None, None) == SPH_ERR_ARG
    assert lib.sph_history_read(None, 0, 1, out.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_history_read_dev(None, 0, 1, out.ctypes.data) == SPH_ERR_ARG


def test_columns_of_raw_rows(capi):
    rows = np.arange(2.0 * 54).reshape(2, 54)                        # two sinks' columns
    rows[1, 35] = np.nan                                             # no densest particle
    h = capi.history_columns(rows, dropped=3)
    assert h["step"].tolist() == [0, 54] and h["step"].dtype == np.int64 and h["n"].tolist() == [4, 58]
    assert h["t"].tolist() == [1.0, 55.0] and h["dt_next"][0] == 2.0 and h["dt_cand"][0] == 3.0 and h["ns"].tolist() == [5, 59]
    assert h["K"][0] == 6.0 + 11 and h["W_ss"][0] == 33.0 and h["rho_max"][0] == 34.0 and h["v_max"][1] == 54.0 + 39
    assert h["densest"].tolist() == [35, -1] and h["densest_pos"][0].tolist() == [36.0, 37.0, 38.0]
    assert h["sinks"].shape == (2, 2, 7) and h["sinks"][0, 1].tolist() == list(np.arange(47.0, 54.0))
    assert h["dropped"] == 3 and h["rows"] is not None
    for r in range(2):
        e = capi.energy_total(rows[r, 6:34])
        assert h["E"][r] == e["E"] and np.array_equal(h["P"][r], e["P"]) and np.array_equal(h["L"][r], e["L"])
        assert np.array_equal(h["com"][r], e["com"])
    for shape in ((2, 39), (2, 41), (40,)):
        with pytest.raises(ValueError):
            capi.history_columns(np.zeros(shape))


# ---- 4. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_parses_its_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, history
    a = history.parse_args(["save275.txt", "--steps", "500", "--every", "1", "--dt", "1e-2", "-o", "hist.npz", "--json"])
    assert (a.save, a.steps, a.every, a.dt, a.out, a.json) == ("save275.txt", 500, 1, 1e-2, "hist.npz", True)
    assert a.capacity == 501 and not (a.variable or a.self_gravity or a.accrete)
    a = history.parse_args(["s.txt", "--steps", "10", "--every", "4", "--variable", "--self-gravity", "--accrete"])
    assert a.capacity == 3 and a.variable and a.self_gravity and a.accrete and a.out is None and not a.json and a.dt == 1e-2
    assert history.parse_args(["s.txt", "--steps", "10", "--capacity", "2"]).capacity == 2

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    for extra in ([], ["--steps", "-1"], ["--steps", "5", "--every", "0"], ["--steps", "5", "--dt", "0"],
                  ["--steps", "5", "--dt", "nan"], ["--steps", "5", "--capacity", "0"], ["--steps", "x"]):
        with pytest.raises(SystemExit) as e:
            history.main(["missing.txt", "-o", str(tmp_path / "o.npz")] + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
    # the summary of two hand-made rows
    rows = np.zeros((2, 40))
    rows[:, 6 + 11] = [2.0, 3.0]                                     # K: E drifts by a half
    rows[:, 6 + 5] = [4.0, 4.0]                                      # px
    rows[:, 6 + 10] = [0.0, 0.25]                                    # lz from zero: the plain difference
    s = history.summary(capi.history_columns(rows, 1))
    assert s["rows"] == 2 and s["dropped"] == 1 and s["drift"] == {"E": 0.5, "P": 0.0, "L": 0.25}
    assert s["first"] == rows[0].tolist() and s["last"] == rows[1].tolist()
    assert history.summary(capi.history_columns(np.zeros((0, 40)))) == {"rows": 0, "dropped": 0}


# ---- 5. the restatement's exact sums ------------------------------------------------------------------------------------------------
def _sets():
    gas, sinks = ic.split_rows(load_golden("disc3000_traj")["ic"])
    rng = np.random.default_rng(27)
    n = 1500
    wide = {k: rng.normal(size=n) for k in "x y z vx vy vz".split()}
    wide["u"] = rng.uniform(0.1, 1.0, n)
    wide["m"] = 10.0 ** rng.uniform(-20.0, 20.0, n)                  # masses over 40 decades
    half = {k: rng.normal(size=n // 2) for k in "x y z vx vy vz".split()}
    mirror = {k: np.concatenate([half[k], -half[k]]) for k in half}  # every r and v with its mirror image
    mirror["u"] = np.tile(rng.uniform(0.1, 1.0, n // 2), 2)
    mirror["m"] = np.tile(rng.uniform(0.5, 2.0, n // 2), 2)
    one_sink = {k: np.array([v]) for k, v in zip("x y z vx vy vz m".split(), (0.1, -0.2, 0.05, 0.0, 0.1, 0.0, 1.5))}
    return {"golden": (gas, sinks), "decades": (wide, one_sink), "mirror": (mirror, None)}


@pytest.mark.parametrize("name", ["golden", "decades", "mirror"])
def test_exact_sums_against_fsum_and_under_permutation(name):
    gas, sinks = _sets()[name]
    n = len(gas["x"])
    terms = history_ref.gas_terms(gas, sinks)
    assert sorted(terms) == history_ref.EXACT
    perm = np.random.default_rng(3).permutation(n)
    shuffled = history_ref.gas_terms({k: np.asarray(v)[perm] for k, v in gas.items()}, sinks)
    for k, t in terms.items():
        s = history_ref.exact_sum(t)
        e = history_ref.exponent(t)
        want = math.fsum(t)                                                      # every term is off by at most half a grid step
        assert abs(s - want) <= n * 2.0 ** (e - 63), (k, s, want)
        assert history_ref.exact_sum(shuffled[k]) == s, k                       # bitwise, in any order
        assert history_ref.exact_sum(t[::-1]) == s, k
    if name == "mirror":
        for k in (2, 3, 4, 5, 6, 7):                                            # sum m r and sum m v: exactly 0.0
            assert history_ref.exact_sum(terms[k]) == 0.0, k
        assert history_ref.exact_sum(terms[11]) > 0.0
    if name == "decades":
        assert history_ref.exponent(terms[1]) > 60 and np.min(terms[1]) < 1e-18


def test_restatement_rows_and_marks():
    gas, sinks = _sets()["golden"]
    rho = np.linspace(1.0, 2.0, len(gas["x"]))
    rho[[7, 90]] = 5.0                                               # a tie: the lower index
    r = history_ref.row(gas, sinks, rho, step=4, dt_words=(0.5, 0.01, 0.02), max_sinks=2)
    assert r.shape == (54,) and r[0] == 4 and r[1:4].tolist() == [0.5, 0.01, 0.02] and r[4] == r[6] == 3000 and r[5] == 1
    assert r[34] == 5.0 and r[35] == 7 and r[36] == gas["x"][7] and r[6 + 13] == 0.0
    assert r[39] == math.sqrt(np.max((gas["vx"] ** 2 + gas["vy"] ** 2) + gas["vz"] ** 2))
    assert r[40 + 6] == sinks["m"][0] and np.all(np.isnan(r[47:]))   # the second sink's columns: there is none
    assert r[21] == 1.0 and r[22] == sinks["m"][0]
    bad = {k: np.array(v, dtype=np.float64) for k, v in gas.items()}
    bad["vx"][11] = np.nan
    b = history_ref.row(bad, sinks, None)
    nan_at = [6 + k for k in (5, 9, 10, 11)] + [39]                  # m vx, the L components vx enters, K, v_max
    assert all(np.isnan(b[i]) for i in nan_at) and np.all(np.isnan(b[34:39]))
    same = [i for i in range(6, 34) if i not in nan_at]
    assert np.array_equal(b[same], r[same])
    empty = history_ref.row({k: np.zeros(0) for k in gas}, None)
    assert empty[4] == 0 and np.all(empty[6:34] == 0.0) and np.isnan(empty[34]) and empty[39] == 0.0
