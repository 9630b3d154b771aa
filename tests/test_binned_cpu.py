"""CPU tests of the binned sums (sph_binned): the edge tables of sph_binned_edges (host code in the library, no device)
against the numpy formulas, every argument error that needs no device, the ABI mirrors (ctypes, Fortran) against the C
header, the register budget of the binned kernels, binned.finish, the command line's parsing, and the numpy restatement
(tests/binned_ref.py) against a plain loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, library, needs_fc, needs_hipcc, resource_usage
import binned_ref
from conftest import ROOT

FIELDS = ["lo", "hi", "axis", "n", "n_axes", "n_q", "q", "weight", "n_rows", "flags", "reserved"]
SPH_ERR_ARG = 1


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    library()
    m.load()
    return m


# ---- 1. the edge tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,n,log", [(0.0, 1.0, 7, False), (-3.5, 12.25, 100, False), (1e-3, 1e4, 64, True),
                                         (10.0, 60.0, 12, True), (0.1, 0.5, 1, False), (2.0, 3.0, 1, True),
                                         (1.0, 1.0 + 1e-9, 1000, False), (0.0, 1048576.0, 1 << 20, False)])
def test_edges_match_the_formulas(capi, lo, hi, n, log):
    d, tab = capi.binned_desc("u", n, (lo, hi), log=(0,) if log else ())
    e = capi.binned_edges(d, tab, 0)
    want = binned_ref.edges_formula(lo, hi, n, log)
    assert e.shape == (n + 1,) and e[0] == lo and e[-1] == hi              # the last edge is hi exactly
    assert np.all(np.diff(e) > 0.0)                                        # strictly increasing
    assert np.all(np.abs(e - want) <= np.spacing(np.abs(want)))            # one ulp (pow is not correctly rounded)
    if not log:
        assert np.array_equal(e, want)


def test_edges_second_axis_and_caller_tables(capi):
    mine = np.array([0.0, 1.0, 3.0, 3.5, 1e9])
    d, tab = capi.binned_desc(("rho", "u"), (5, 4), ((1.0, 32.0), None), edges=(None, mine), log=(0,))
    assert d.flags & capi.BINNED_EDGES1 and not d.flags & capi.BINNED_EDGES0
    assert np.array_equal(capi.binned_edges(d, tab, 1), mine)              # verbatim
    assert np.array_equal(capi.binned_edges(d, tab, 0), binned_ref.edges_formula(1.0, 32.0, 5, True))
    other = np.array([-2.0, -1.0, 7.0])
    d, tab = capi.binned_desc(("rho", capi.binned_row(0)), (2, 4), edges=(other, mine), n_rows=1)
    assert tab.size == 8                                                   # axis 0's table first, then axis 1's
    assert np.array_equal(capi.binned_edges(d, tab, 0), other) and np.array_equal(capi.binned_edges(d, tab, 1), mine)


# ---- 2. the argument errors that need no device ----------------------------------------------------------------------------
def _refused(capi, d, tab=None, axis=0):
    out = np.zeros(max(int(d.n[0]), int(d.n[1]), 1) + 2)
    e = None if tab is None else np.ascontiguousarray(tab, dtype=np.float64)
    return capi.load().sph_binned_edges(C.byref(d), None if e is None else e.ctypes.data, axis, out.ctypes.data) == SPH_ERR_ARG


def test_argument_errors(capi):
    lib = capi.load()
    good = dict(axes=("rho", "u"), bins=(4, 3), ranges=((1.0, 2.0), (0.0, 1.0)), q=("alpha", capi.binned_row(1)), n_rows=2)

    def desc(**kw):
        a = dict(good); a.update(kw)
        return capi.binned_desc(**a)

    d, tab = desc()
    assert not _refused(capi, d) and not _refused(capi, d, axis=1)
    out = np.zeros(8)
    assert lib.sph_binned_edges(None, None, 0, out.ctypes.data) == SPH_ERR_ARG            # null descriptor
    assert lib.sph_binned_edges(C.byref(d), None, 0, None) == SPH_ERR_ARG                 # null output
    assert _refused(capi, d, axis=2) and _refused(capi, d, axis=-1)

    def edit(**fields):
        dd, _ = desc()
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(dd, k)[v[0]] = v[1]
            else:
                setattr(dd, k, v)
        return dd

    bad = {
        "n_axes 0": edit(n_axes=0), "n_axes 3": edit(n_axes=3),
        "n[0] 0": edit(n=(0, 0)), "n[1] -1": edit(n=(1, -1)),
        "n[1] != 1 with one axis": edit(n_axes=1),
        "product above 2^20": desc(bins=(2048, 1024))[0],
        "axis id": edit(axis=(0, 19)), "axis id -": edit(axis=(1, -3)),          # row 2 of 2 rows
        "q id": edit(q=(0, 99)), "q row": edit(q=(1, capi.binned_row(2))),
        "n_q": edit(n_q=9), "n_q -": edit(n_q=-1),
        "n_rows 17": edit(n_rows=17), "n_rows -1": edit(n_rows=-1),
        "lo nan": edit(lo=(0, np.nan)), "hi inf": edit(hi=(1, np.inf)), "lo == hi": edit(lo=(0, 2.0)), "lo > hi": edit(lo=(1, 3.0)),
        "log lo 0": desc(ranges=((1.0, 2.0), (0.0, 1.0)), log=(1,))[0],
        "log lo < 0": desc(ranges=((-1.0, 2.0), (0.0, 1.0)), log=(0,))[0],
        "weight": edit(weight=3), "weight -": edit(weight=-1),
        "flags": edit(flags=64), "reserved": edit(reserved=(2, 1)),
        "edges flag without a table": edit(flags=capi.BINNED_EDGES0),
        "coinciding computed edges": desc(ranges=((1.0, 1.0 + 4e-16), (0.0, 1.0)))[0],
    }
    for name, dd in bad.items():
        assert _refused(capi, dd), name
    assert _refused(capi, d, tab=np.zeros(5))                                          # a table without an EDGES flag
    one = dict(axes="u", bins=4, ranges=(0.0, 1.0))
    for flag in (capi.BINNED_LOG1, capi.BINNED_EDGES1):                                # a flag of axis 1 with one axis
        dd, _ = capi.binned_desc(**one)
        dd.flags |= flag
        assert _refused(capi, dd, tab=np.arange(2.0) if flag == capi.BINNED_EDGES1 else None)
    for table in ([0.0, 1.0, 1.0, 2.0, 3.0], [0.0, 1.0, 0.5, 2.0, 3.0], [0.0, 1.0, np.nan, 2.0, 3.0], [0.0, 1.0, 2.0, 3.0, np.inf],
                  [-np.inf, 1.0, 2.0, 3.0, 4.0]):
        dd, tab = capi.binned_desc("u", 4, edges=np.array(table))
        assert _refused(capi, dd, tab), table
        dd, tab = capi.binned_desc(("rho", "u"), (3, 4), ((1.0, 2.0), None), edges=(None, np.array(table)))
        assert _refused(capi, dd, tab, axis=0), table                                  # every table of the call must stand
    dd, tab = capi.binned_desc("u", 4, edges=np.arange(5.0))
    dd.flags |= capi.BINNED_LOG0                                                       # LOG together with EDGES
    dd.lo[0], dd.hi[0] = 1.0, 2.0
    assert _refused(capi, dd, tab)
    # the calls themselves refuse a null context before anything else
    sums = np.zeros(4 * 3 * 4)
    for fn in (lib.sph_binned, lib.sph_binned_dev):
        assert fn(None, C.byref(d), None, None, sums.ctypes.data, sums.size, None) == SPH_ERR_ARG


def test_python_descriptor_helper(capi):
    d, tab = capi.binned_desc("rho", 8, (1.0, 2.0), log=(0,), q=("u", 8, capi.binned_row(3)), weight="volume", n_rows=4,
                              squares=True, skip_nan=False)
    assert (d.n_axes, d.n[0], d.n[1], d.n_q, d.n_rows, d.weight) == (1, 8, 1, 3, 4, capi.BINNED_W_VOLUME)
    assert d.axis[0] == capi.FIELDS.index("rho") and list(d.q[:3]) == [6, 8, -4]
    assert d.flags == capi.BINNED_LOG0 | capi.BINNED_SQUARES and tab is None
    assert capi.binned_nsum(3, True) == 8 and capi.binned_nsum(0, False) == 2
    for kw in (dict(axes=("x", "y", "z"), bins=(1, 1, 1)), dict(axes="x", bins=(2, 2)), dict(axes="x", bins=2),
               dict(axes="x", bins=2, edges=np.arange(4.0)), dict(axes="x", bins=2, ranges=(0.0, 1.0), q=["u"] * 9)):
        with pytest.raises(ValueError):
            capi.binned_desc(**kw)


# ---- 3. the ABI mirrors ----------------------------------------------------------------------------------------------------
def test_descriptor_layout_and_symbols(capi, tmp_path):
    consts = ["SPH_BINNED_MAX_Q", "SPH_BINNED_ROW(0)", "SPH_BINNED_ROW(15)", "SPH_BINNED_W_ONE", "SPH_BINNED_W_MASS",
              "SPH_BINNED_W_VOLUME", "SPH_BINNED_LOG0", "SPH_BINNED_LOG1", "SPH_BINNED_EDGES0", "SPH_BINNED_EDGES1",
              "SPH_BINNED_SQUARES", "SPH_BINNED_SKIP_NAN"]
    got = c_layout(tmp_path, "sph_binned_desc", FIELDS,
                   ['printf("consts' + " %d" * len(consts) + '\\n", ' + ", ".join(consts) + ');', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == C.sizeof(capi.BinnedDesc) == 112
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.BinnedDesc, f).offset, f
    mine = [capi.BINNED_MAX_Q, capi.binned_row(0), capi.binned_row(15), capi.BINNED_W_ONE, capi.BINNED_W_MASS, capi.BINNED_W_VOLUME,
            capi.BINNED_LOG0, capi.BINNED_LOG1, capi.BINNED_EDGES0, capi.BINNED_EDGES1, capi.BINNED_SQUARES, capi.BINNED_SKIP_NAN]
    assert got["consts"] == " ".join(str(v) for v in mine) == "8 -1 -16 0 1 2 1 2 4 8 16 32"
    assert got["abi"] == "1"                                        # the change is additive
    lib = C.CDLL(library())
    for s in ("sph_binned", "sph_binned_dev", "sph_binned_edges"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_BINNED_SQUARES = 16, SPH_BINNED_SKIP_NAN = 32", binding)
    assert re.search(r"SPH_BINNED_LOG0 = 1, SPH_BINNED_LOG1 = 2, SPH_BINNED_EDGES0 = 4, SPH_BINNED_EDGES1 = 8", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "binned_caller", """program binned_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_binned_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: sums(:, :, :)
  real(c_double) :: edge(5)
  integer(c_int64_t), target :: counts(3)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%lo = [1.0_c_double, 0.0_c_double]
  d%hi = [16.0_c_double, 0.0_c_double]
  d%axis = [SPH_F_RHO, 0]
  d%n = [4, 1]
  d%n_axes = 1
  d%n_q = 1
  d%q = 0
  d%q(1) = SPH_F_U
  d%weight = SPH_BINNED_W_MASS
  d%n_rows = 0
  d%flags = ior(SPH_BINNED_LOG0, SPH_BINNED_SQUARES)
  d%reserved = 0
  if (c_sizeof(d) /= 112) stop 1
  st = sph_binned_edges(d, c_null_ptr, 0_c_int32_t, edge)
  if (st /= SPH_OK) stop 2
  if (edge(1) /= 1.0_c_double .or. edge(3) /= 4.0_c_double .or. edge(5) /= 16.0_c_double) stop 3
  allocate(sums(4, 1, 4))
  st = sph_binned(ctx, d, c_null_ptr, c_null_ptr, c_loc(sums), 16_c_int64_t, c_loc(counts))
  st = sph_binned_dev(ctx, d, c_null_ptr, c_null_ptr, c_null_ptr, 16_c_int64_t, c_null_ptr)
  print *, st, edge
end program binned_caller
""")


# ---- 4. the kernels' resources ---------------------------------------------------------------------------------------------
@needs_hipcc
def test_binned_kernels_fit_the_register_budget():
    k = resource_usage("binned.hip", containing("binned_"))
    for name, count in (("binned_keys", 1), ("binned_starts", 1), ("binned_pieces", 6), ("binned_final", 1)):
        assert sum(name in n for n in k) == count, (name, sorted(k))
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)             # 4 waves / SIMD by registers


# ---- 5. finish --------------------------------------------------------------------------------------------------------------
def test_finish_on_hand_computed_values():
    from summersph_amd import binned
    # two quantities with squares: N, W, wA0, wA1, wA0A0, wA1A1
    sums = np.array([[[4.0, 2.0, 6.0, -1.0, 20.0, 0.5]],           # <A0> 3, <A0 A0> 10 -> disp 1; <A1> -0.5, <A1 A1> .25 -> 0
                     [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]],             # empty: NaN
                     [[1.0, 0.5, 1.0, 2.0, 1.9999999, 8.0]]])      # <A0> 2, <A0 A0> < 4: clipped to 0; <A1> 4, <A1 A1> 16 -> 0
    N, W, mean, disp = binned.finish(sums, 2, squares=True)
    assert N.shape == W.shape == (3, 1) and mean.shape == disp.shape == (3, 1, 2)
    assert np.array_equal(N[:, 0], [4.0, 0.0, 1.0]) and np.array_equal(W[:, 0], [2.0, 0.0, 0.5])
    assert np.array_equal(mean[0, 0], [3.0, -0.5]) and np.array_equal(disp[0, 0], [1.0, 0.0])
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(disp[1]))
    assert np.array_equal(mean[2, 0], [2.0, 4.0]) and np.array_equal(disp[2, 0], [0.0, 0.0])
    N, W, mean, disp = binned.finish(sums[..., :4], 2)
    assert disp is None and np.array_equal(mean[0, 0], [3.0, -0.5])
    N, W, mean, disp = binned.finish(sums[..., :2], 0, squares=True)
    assert mean.shape == (3, 1, 0) and disp.shape == (3, 1, 0)
    with pytest.raises(ValueError):
        binned.finish(sums, 2)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------
def test_cli_parses_its_arguments(tmp_path, monkeypatch):
    from summersph_amd import binned, capi
    a = binned.parse_args(["save275.txt", "-o", "phase.npz", "--x", "rho", "--y", "u", "--bins", "128", "128", "--log", "x,y",
                           "--weight", "mass", "--q", "alpha", "--json"])
    assert a.axes == ("rho", "u") and a.bins == [128, 128] and a.log == (0, 1) and a.q == ("alpha",) and a.json
    assert a.ranges == [None, None] and a.weight == "mass" and not a.squares and not a.variable
    a = binned.parse_args(["s.txt", "-o", "o.npz", "--x", "h", "--bins", "5", "--xrange", "0.5", "2", "--variable", "--q", "u,c,omega",
                           "--squares", "--weight", "volume"])
    assert a.axes == ("h",) and a.ranges == [[0.5, 2.0]] and a.q == ("u", "c", "omega") and a.squares and a.log == ()

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    base = ["missing.txt", "-o", str(tmp_path / "o.npz")]
    for extra in (["--x", "rho"], ["--x", "density", "--bins", "4"], ["--x", "rho", "--bins", "0"], ["--x", "rho", "--bins", "4", "4"],
                  ["--x", "rho", "--y", "u", "--bins", "4"], ["--x", "rho", "--y", "u", "--bins", "2048", "1024"],
                  ["--x", "rho", "--bins", "4", "--log", "y"], ["--x", "rho", "--bins", "4", "--log", "z"],
                  ["--x", "rho", "--bins", "4", "--yrange", "0", "1"], ["--x", "rho", "--bins", "4", "--xrange", "2", "1"],
                  ["--x", "rho", "--bins", "4", "--xrange", "0", "1", "--log", "x"], ["--x", "rho", "--bins", "4", "--weight", "rho"],
                  ["--x", "h", "--bins", "4"], ["--x", "rho", "--bins", "4", "--q", "u,nothing"],
                  ["--x", "rho", "--bins", "4", "--q", ",".join(["u"] * 9)]):
        with pytest.raises(SystemExit) as e:
            binned.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()


# ---- 7. the restatement against a plain loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("two,squares,skip_nan", [(False, False, True), (True, True, True), (True, True, False), (False, True, False)])
def test_restatement_against_brute_force(two, squares, skip_nan):
    rng = np.random.default_rng(3 + two + 2 * squares + 4 * skip_nan)
    n = 200
    a0 = rng.uniform(-0.2, 1.2, n)
    a1 = np.exp(rng.uniform(-1.0, 3.0, n))
    a0[[3, 50]] = np.nan                                            # NaN axis values are outside
    a0[7], a0[8] = 0.0, 1.0                                         # on the first edge: inside; on the last: outside
    t0 = binned_ref.edges_formula(0.0, 1.0, 5)
    t1 = binned_ref.edges_formula(1.0, 10.0, 3, log=True)
    a0[9] = t0[2]                                                   # on an inner edge: the upper bin
    q = [rng.integers(-5, 6, n).astype(float), rng.normal(size=n)]
    q[1][[11, 12, 13, 50]] = np.nan
    w = rng.integers(1, 4, n).astype(float)
    owned = np.arange(n) < 180
    axes, tables = ([a0, a1], [t0, t1]) if two else ([a0], [t0])
    got, gc = binned_ref.binned_sums(axes, tables, q, w, owned, squares, skip_nan)
    want, wc = binned_ref.brute_force(axes, tables, q, w, owned, squares, skip_nan)
    assert gc == wc and sum(gc) == 180 and gc[1] >= 3 and (gc[2] > 0) == skip_nan
    assert got.shape == want.shape
    assert np.array_equal(got[..., :3], want[..., :3])              # counts, integer weights and integer quantities: exact
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() == (not skip_nan)
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] - want[ok])) <= 1e-13 * np.max(np.abs(want[ok]))
    k9 = np.flatnonzero(t0 == a0[9])[0]
    assert k9 == 2 and binned_ref.bin_index(a0[9:10], t0)[1][0] == 2
