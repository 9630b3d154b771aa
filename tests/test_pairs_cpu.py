"""CPU tests of the pair sums (sph_pairs): the numpy restatement (tests/pairs_ref.py) against a plain double loop, the edge
tables of sph_pairs_edges against the formulas and every argument error that needs no device, sph_pairs_finish on
hand-made limbs, the ABI mirrors (ctypes, Fortran) against the C header, the resources of the kernels, pairs.finish /
pairs.rdf / pairs.add_raw on hand values and the command line's parsing."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, library, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import pairs_ref

FIELDS = ["lo", "hi", "clip_lo", "clip_hi", "n_bins", "n_q", "q", "weight", "n_rows", "flags", "target_stride", "target_phase",
          "reserved"]
SPH_ERR_ARG = 1


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    library()
    m.load()
    return m


# ---- 1. the restatement against a plain double loop ---------------------------------------------------------------------------
@pytest.mark.parametrize("weight_m,velocity,scale_h,nq", [(False, False, False, 0), (True, True, False, 2), (True, True, True, 4),
                                                          (False, True, True, 1)])
def test_restatement_against_brute_force(weight_m, velocity, scale_h, nq):
    rng = np.random.default_rng(11 + weight_m + 2 * velocity + 4 * scale_h + 8 * nq)
    n = 200
    pos = rng.uniform(0.0, 1.0, (n, 3))
    pos[5] = pos[6]                                                    # a coincident pair: r = 0, u = 0
    pos[7, 1] = np.nan                                                 # not usable
    vel = rng.normal(size=(n, 3))
    m = rng.uniform(0.5, 2.0, n)
    h = rng.uniform(0.05, 0.15, n)
    A = [rng.normal(size=n) * 10.0 ** k for k in range(nq)]
    if nq:
        A[0][9] = np.inf                                               # not usable either
    edge = pairs_ref.edges_formula(0.0, 3.0 if scale_h else 0.35, 6)
    kw = dict(n_owned=180, weight_m=weight_m, velocity=velocity, scale_h=scale_h, clip=((0.1, 0.0, -1.0), (0.95, 1.0, 2.0)),
              stride=2, phase=1)
    got = pairs_ref.pairs(pos, vel, m, h, A, edge, **kw)
    want, largest, counts = pairs_ref.brute_force(pos, vel, m, h, A, edge, **kw)
    assert got["counts"] == counts and counts[1] + counts[2] == 180 and counts[2] == (2 if nq else 1) and 0 < counts[0] < 90
    assert np.array_equal(got["sums"][:, 0], want[:, 0]) and want[:, 0].sum() > 500            # N: exact
    assert got["sums"].shape == want.shape
    assert np.all(np.abs(got["sums"] - want) <= 1e-13 * largest)       # each sum against its bin's largest term
    if not weight_m:
        assert np.array_equal(got["sums"][:, 1], want[:, 0])           # w = 1: W is N
    # the limbs are the doubles
    for b in range(want.shape[0]):
        for s in range(want.shape[1]):
            total = pairs_ref.from_limbs(*got["raw"][b, s])
            assert pairs_ref.finish_int(total, got["exps"][s]) == got["sums"][b, s]


def test_restatement_edge_rule_and_bounds():
    # d2 exact: r = 5 on the inner edge goes to the upper bin, r = 13 on the last edge is outside, r = 3 on the first is inside
    pos = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 3.0], [5.0, 0.0, 12.0]])
    vel = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -2.0], [0.0, 0.0, 0.0]])
    m = np.array([1.0, 2.0, 4.0, 8.0])
    r = pairs_ref.pairs(pos, vel, m, 1.0, [], [3.0, 5.0, 13.0], weight_m=True, velocity=True, stride=4)
    assert r["counts"] == (1, 4, 0)
    assert r["sums"][:, 0].tolist() == [1.0, 1.0] and r["sums"][:, 1].tolist() == [4.0, 2.0]
    # u of (0, 1): (1 * 3 + 0 * 4) / 5 = 0.6; of (0, 2): -2 * 3 / 3 = -2
    assert r["sums"][1, 2] == 2.0 * 0.6 and r["sums"][0, 2] == 4.0 * -2.0 and r["sums"][0, 4] == 4.0 * -8.0
    # w_max = 8, v_max = 2: W2 = 64 < 2^7, W2 V = 512 < 2^10, W2 V^2 = 4096 < 2^13, W2 V^3 = 32768 < 2^16
    assert r["exps"].tolist() == [62, 7, 10, 13, 16, 13]


def test_poisson_bound_holds_for_the_gpu_tests_seed():
    """the set, the bins and the 5 sigma bound of tests/test_pairs_gpu.py::test_poisson_counts, on the restatement"""
    pos = np.random.default_rng(2024).uniform(0.0, 1.0, (3000, 3))
    edge = pairs_ref.edges_formula(0.0, 0.2, 8)
    r = pairs_ref.pairs(pos, None, np.full(3000, 1.0 / 3000), 1.0, [], edge, clip=((0.25,) * 3, (0.75,) * 3))
    E = r["counts"][0] * 3000 * (4.0 * np.pi / 3.0) * (edge[1:] ** 3 - edge[:-1] ** 3)
    assert 300 < r["counts"][0] < 450 and np.all(np.abs(r["sums"][:, 0] - E) <= 5.0 * np.sqrt(E))


# ---- 2. the edge tables and the refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,n,log", [(0.0, 1.0, 7, False), (0.05, 4.0, 64, True), (0.1, 0.5, 1, False), (2.0, 3.0, 1, True),
                                         (0.0, 8.0, 1024, False), (1e-3, 1e2, 1024, True)])
def test_edges_match_the_formulas(capi, lo, hi, n, log):
    d, tab = capi.pairs_desc((lo, hi), n, log=log)
    e = capi.pairs_edges(d, tab)
    want = pairs_ref.edges_formula(lo, hi, n, log)
    assert e.shape == (n + 1,) and e[0] == lo and e[-1] == hi and np.all(np.diff(e) > 0.0)
    # pow is not correctly rounded: two libms differ by an ulp of the power, which the product with lo can turn into two
    assert np.all(np.abs(e - want) <= 2.0 * np.spacing(np.abs(want)))
    if not log:
        assert np.array_equal(e, want)
    mine = np.array([0.0, 0.5, 0.75, 4.0])
    d, tab = capi.pairs_desc(None, 3, edges=mine)
    assert d.flags == capi.PAIRS_EDGES and np.array_equal(capi.pairs_edges(d, tab), mine)


def _refused(capi, d, tab=None):
    out = np.zeros(1100)
    e = None if tab is None else np.ascontiguousarray(tab, dtype=np.float64)
    return capi.load().sph_pairs_edges(C.byref(d), None if e is None else e.ctypes.data, out.ctypes.data) == SPH_ERR_ARG


def test_argument_errors(capi):
    lib = capi.load()
    good = dict(r_range=(0.5, 2.0), bins=4, q=("u", capi.pairs_row(1)), n_rows=2, stride=4, phase=3, velocity=True, scale_h=True)

    def desc(**kw):
        a = dict(good); a.update(kw)
        return capi.pairs_desc(**a)

    def edit(**fields):
        dd, _ = desc()
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(dd, k)[v[0]] = v[1]
            else:
                setattr(dd, k, v)
        return dd

    d, tab = desc()
    assert not _refused(capi, d)
    out = np.zeros(8)
    assert lib.sph_pairs_edges(None, None, out.ctypes.data) == SPH_ERR_ARG                  # null descriptor
    assert lib.sph_pairs_edges(C.byref(d), None, None) == SPH_ERR_ARG                       # null output
    bad = {
        "n_bins 0": edit(n_bins=0), "n_bins 1025": edit(n_bins=1025), "n_bins -1": edit(n_bins=-1),
        "lo == hi": edit(lo=2.0), "lo > hi": edit(lo=3.0), "lo nan": edit(lo=np.nan), "hi inf": edit(hi=np.inf),
        "log lo 0": desc(r_range=(0.0, 2.0), log=True)[0], "log lo < 0": desc(r_range=(-1.0, 2.0), log=True)[0],
        "stride 0": edit(target_stride=0, target_phase=0), "stride -1": edit(target_stride=-1),
        "phase == stride": edit(target_phase=4), "phase -1": edit(target_phase=-1),
        "field id": edit(q=(0, 19)), "field id 99": edit(q=(0, 99)), "row id": edit(q=(1, capi.pairs_row(2))),
        "n_q 5": edit(n_q=5), "n_q -1": edit(n_q=-1), "n_rows 17": edit(n_rows=17), "n_rows -1": edit(n_rows=-1),
        "flags": edit(flags=16), "flags -": edit(flags=-1), "reserved 0": edit(reserved=(0, 1)), "reserved 2": edit(reserved=(2, 7)),
        "weight": edit(weight=2), "weight -": edit(weight=-1), "clip nan": edit(clip_lo=(1, np.nan)),
        "edges flag without a table": edit(flags=capi.PAIRS_EDGES),
        "coinciding computed edges": desc(r_range=(1.0, 1.0 + 4e-16))[0],
    }
    for name, dd in bad.items():
        assert _refused(capi, dd), name
    assert _refused(capi, d, tab=np.arange(5.0))                                            # a table without the EDGES flag
    for table in ([0.0, 1.0, 1.0, 2.0, 3.0], [0.0, 1.0, 0.5, 2.0, 3.0], [0.0, 1.0, np.nan, 2.0, 3.0], [0.0, 1.0, 2.0, 3.0, np.inf]):
        dd, tab = capi.pairs_desc(None, 4, edges=np.array(table))
        assert _refused(capi, dd, tab), table                                               # a non-monotone or non-finite table
    dd, tab = capi.pairs_desc(None, 4, edges=np.arange(1.0, 6.0))
    assert not _refused(capi, dd, tab)
    dd.flags |= capi.PAIRS_LOG                                                              # LOG together with EDGES
    dd.lo, dd.hi = 1.0, 2.0
    assert _refused(capi, dd, tab)
    with pytest.raises(ValueError):
        capi.pairs_desc((0, 1), 4, q=["u"] * 5)
    with pytest.raises(ValueError):
        capi.pairs_desc(None, 4, edges=np.arange(4.0))
    # the calls themselves refuse a null context before anything else; finish its null pointers
    sums = np.zeros(4 * 10)
    for fn in (lib.sph_pairs, lib.sph_pairs_dev):
        assert fn(None, C.byref(d), None, None, sums.ctypes.data, sums.size, None, None, None) == SPH_ERR_ARG
    ex, raw = np.zeros(10, np.int32), np.zeros((4, 10, 2), np.uint64)
    assert lib.sph_pairs_finish(None, ex.ctypes.data, raw.ctypes.data, sums.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_pairs_finish(C.byref(d), None, raw.ctypes.data, sums.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_pairs_finish(C.byref(d), ex.ctypes.data, None, sums.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_pairs_finish(C.byref(d), ex.ctypes.data, raw.ctypes.data, None) == SPH_ERR_ARG


# ---- 3. sph_pairs_finish on hand-made limbs --------------------------------------------------------------------------------------
def test_finish_rounds_once(capi):
    values = [0, 1, -1, -12345, (1 << 64) + 5, -((1 << 64) + 5),          # the low limb has wrapped, both signs
              (1 << 53) + 1, -((1 << 53) + 1),                            # a tie: to even, 2^53
              (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6,                # ties to even, up and down
              (3 << 100) + 1, (1 << 117) + (1 << 64) + 1,                 # above a tie by a bit far below
              (1 << 117) + (1 << 64), (1 << 117) + (3 << 64),             # exactly on a tie across the limbs (even / odd)
              -((1 << 117) + (3 << 64)), (1 << 126) + 12345678901234567890, -(1 << 127), (1 << 127) - 1,
              (1 << 64) - 1, 1 << 64, -(1 << 64), (1 << 63), -(1 << 63)]
    d, _ = capi.pairs_desc((0.0, 1.0), len(values))                        # n_q = 0, no velocity: N and W per bin
    raw = np.zeros((len(values), 2, 2), dtype=np.uint64)
    for b, v in enumerate(values):
        raw[b, 0] = pairs_ref.to_limbs(abs(v) % (1 << 63))                # N: a plain count
        raw[b, 1] = pairs_ref.to_limbs(v)
        assert pairs_ref.from_limbs(*raw[b, 1]) == v
    for e in (62, 0, -40, 75):
        got = capi.pairs_finish(d, np.array([62, e], dtype=np.int32), raw)
        for b, v in enumerate(values):
            assert got[b, 0] == float(abs(v) % (1 << 63)), (b, v)
            assert got[b, 1] == pairs_ref.finish_int(v, e), (b, v, e)
    assert capi.pairs_finish(d, [62, 62], raw)[6, 1] == 2.0 ** 53 and capi.pairs_finish(d, [62, 62], raw)[8, 1] == 2.0 ** 53 + 4


# ---- 4. the ABI mirrors ----------------------------------------------------------------------------------------------------------
def test_descriptor_layout_and_symbols(capi, tmp_path):
    consts = ["SPH_PAIRS_MAX_Q", "SPH_PAIRS_MAX_BINS", "SPH_PAIRS_ROW(0)", "SPH_PAIRS_ROW(15)", "SPH_PAIRS_W_ONE", "SPH_PAIRS_W_MASS",
              "SPH_PAIRS_LOG", "SPH_PAIRS_EDGES", "SPH_PAIRS_SCALE_H", "SPH_PAIRS_VELOCITY"]
    got = c_layout(tmp_path, "sph_pairs_desc", FIELDS,
                   ['printf("consts' + " %d" * len(consts) + '\\n", ' + ", ".join(consts) + ');', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == C.sizeof(capi.PairsDesc) == 120
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.PairsDesc, f).offset, f
    mine = [capi.PAIRS_MAX_Q, capi.PAIRS_MAX_BINS, capi.pairs_row(0), capi.pairs_row(15), capi.PAIRS_W_ONE, capi.PAIRS_W_MASS,
            capi.PAIRS_LOG, capi.PAIRS_EDGES, capi.PAIRS_SCALE_H, capi.PAIRS_VELOCITY]
    assert got["consts"] == " ".join(str(v) for v in mine) == "4 1024 -1 -16 0 1 1 2 4 8"
    assert got["abi"] == "1"                                        # the change is additive
    lib = C.CDLL(library())
    for s in ("sph_pairs", "sph_pairs_dev", "sph_pairs_edges", "sph_pairs_finish"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_PAIRS_LOG = 1, SPH_PAIRS_CALLER_EDGES = 2, SPH_PAIRS_SCALE_H = 4, SPH_PAIRS_VELOCITY = 8", binding)
    assert re.search(r"SPH_PAIRS_MAX_Q = 4, SPH_PAIRS_MAX_BINS = 1024", binding)
    assert capi.pairs_nsum(0, False) == 2 and capi.pairs_nsum(4, True) == 14 and capi.pairs_nsum(1, False) == 4


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "pairs_caller", """program pairs_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_pairs_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: sums(:, :)
  integer(c_int64_t), allocatable, target :: raw(:, :, :)
  integer(c_int32_t), target :: exps(8)
  real(c_double) :: edge(5)
  integer(c_int64_t), target :: counts(3)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%lo = 1.0_c_double
  d%hi = 16.0_c_double
  d%clip_lo = -huge(1.0_c_double)
  d%clip_hi = huge(1.0_c_double)
  d%n_bins = 4
  d%n_q = 1
  d%q = 0
  d%q(1) = SPH_F_U
  d%weight = SPH_PAIRS_W_MASS
  d%n_rows = 0
  d%flags = ior(SPH_PAIRS_LOG, SPH_PAIRS_VELOCITY)
  d%target_stride = 8
  d%target_phase = 0
  d%reserved = 0
  if (c_sizeof(d) /= 120) stop 1
  st = sph_pairs_edges(d, c_null_ptr, edge)
  if (st /= SPH_OK) stop 2
  if (edge(1) /= 1.0_c_double .or. edge(3) /= 4.0_c_double .or. edge(5) /= 16.0_c_double) stop 3
  allocate(sums(8, 4), raw(2, 8, 4))
  raw = 0
  raw(1, 2, 1) = 3
  exps = 62
  st = sph_pairs_finish(d, exps, raw, sums)
  if (st /= SPH_OK .or. sums(2, 1) /= 3.0_c_double .or. sums(1, 1) /= 0.0_c_double) stop 4
  st = sph_pairs(ctx, d, c_null_ptr, c_null_ptr, c_loc(sums), 32_c_int64_t, c_loc(raw), c_loc(exps), c_loc(counts))
  st = sph_pairs_dev(ctx, d, c_null_ptr, c_null_ptr, c_null_ptr, 32_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr)
  print *, st, edge
end program pairs_caller
""")


# ---- 5. the kernels' resources -------------------------------------------------------------------------------------------------
@needs_hipcc
def test_pair_kernels_fit_the_register_budget():
    k = resource_usage("pair_stats.hip", containing("pairs_"))
    for name, count in (("pairs_select", 1), ("pairs_box", 1), ("pairs_keys", 1), ("pairs_gather", 1), ("pairs_tails", 1),
                        ("pairs_bin", 4), ("pairs_sum", 1), ("pairs_convert", 1)):
        assert sum(name in n for n in k) == count, (name, sorted(k))
    assert len(k) == 11
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


# ---- 6. finish, rdf, add_raw -----------------------------------------------------------------------------------------------------
def test_finish_on_hand_computed_values():
    from summersph_amd import pairs
    # one quantity and velocity: N, W, w dA, w dA^2, w u, w u^2, w u^3, w dv^2
    sums = np.array([[4.0, 2.0, 6.0, 20.0, -1.0, 3.0, -0.5, 9.0],
                     [0.0] * 8,
                     [1.0, 0.5, 1.0, 2.0, 0.25, 0.125, 0.0625, 0.125]])
    f = pairs.finish(sums, 1, velocity=True)
    assert np.array_equal(f["N"], [4.0, 0.0, 1.0]) and np.array_equal(f["W"], [2.0, 0.0, 0.5])
    assert f["dA"].shape == (3, 1) and f["dA"][0, 0] == 3.0 and f["dA2"][0, 0] == 10.0 and f["dA"][2, 0] == 2.0
    assert f["u"][0] == -0.5 and f["S2_par"][0] == 1.5 and f["S3_par"][0] == -0.25 and f["S2_perp"][0] == (4.5 - 1.5) / 2
    assert f["S2_perp"][2] == 0.0
    for key in ("dA", "dA2", "u", "S2_par", "S3_par", "S2_perp"):
        assert np.all(np.isnan(f[key][1])), key
    g = pairs.finish(sums[:, :2], 0)
    assert g["dA"].shape == (3, 0) and "u" not in g
    with pytest.raises(ValueError):
        pairs.finish(sums, 1)


def test_add_raw_carries(capi):
    from summersph_amd import pairs
    vals_a = [5, -5, (1 << 64) - 1, -(1 << 64), (1 << 100) + (1 << 63), -1]
    vals_b = [7, 3, 1, -1, (1 << 63), 1]
    a = np.array([pairs_ref.to_limbs(v) for v in vals_a], dtype=np.uint64)
    b = np.array([pairs_ref.to_limbs(v) for v in vals_b], dtype=np.uint64)
    c = pairs.add_raw(a, b)
    assert [pairs_ref.from_limbs(*r) for r in c] == [x + y for x, y in zip(vals_a, vals_b)]
    assert np.array_equal(pairs.add_raw(a.view(np.int64), b), c)              # the device form's int64 view: the same bits
    with pytest.raises(ValueError):
        pairs.add_raw(a, b[:3])


def test_rdf_on_hand_values(capi):
    from summersph_amd import pairs
    n = 8
    fields = {"x": np.arange(n, dtype=float), "y": np.zeros(n), "z": np.zeros(n), "rho": np.full(n, 3.0), "m": np.full(n, 0.5),
              "h": np.full(n, 2.0)}
    fields["x"][3] = np.nan
    ctx = types.SimpleNamespace(field=lambda name: fields[name].copy(), params=types.SimpleNamespace(flags=0, h=2.0))
    edges = np.array([0.0, 1.0, 2.0])
    sums = np.array([[10.0, 0.0], [0.0, 0.0]])
    # targets: ids 0 2 4 6 (stride 2), 0 <= x < 5 strictly inside (-1, 5): 0 2 4 -> 3 targets of number density 6
    t = pairs.targets(np.stack([fields["x"], fields["y"], fields["z"]], axis=1), n, ((-1, -1, -1), (5, 1, 1)), 2, 0)
    assert np.flatnonzero(t).tolist() == [0, 2, 4]
    g = pairs.rdf(ctx, sums, edges, False, ((-1, -1, -1), (5, 1, 1)), 2, 0)
    shell = 4.0 * np.pi / 3.0 * np.array([1.0, 7.0])
    assert np.allclose(g, [10.0 / (18.0 * shell[0]), 0.0], rtol=1e-15)
    g = pairs.rdf(ctx, sums, edges, True, ((-1, -1, -1), (5, 1, 1)), 2, 0)
    assert np.allclose(g, [10.0 / (18.0 * 8.0 * shell[0]), 0.0], rtol=1e-15)
    assert pairs.targets(np.zeros((4, 3)), 2).tolist() == [True, True, False, False]       # ghosts are no targets


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_parses_its_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, pairs
    a = pairs.parse_args(["save275.txt", "-o", "pairs.npz", "--r", "0.05", "4", "--bins", "64", "--log", "--scale-h", "--velocity",
                          "--q", "u", "--stride", "8", "--json"])
    assert a.r == [0.05, 4.0] and a.bins == 64 and a.log and a.scale_h and a.velocity and a.q == ("u",) and a.stride == 8
    assert a.phase == 0 and a.weight == "one" and a.clip is None and a.json and not a.variable
    a = pairs.parse_args(["s.txt", "-o", "o.npz", "--r", "0", "2", "--bins", "5", "--variable", "--q", "u,h", "--weight", "mass",
                          "--clip", "0,0,0,1,1,1", "--stride", "4", "--phase", "3"])
    assert a.q == ("u", "h") and a.clip == ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) and a.phase == 3 and not a.log

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    base = ["missing.txt", "-o", str(tmp_path / "o.npz")]
    for extra in (["--bins", "4"], ["--r", "0", "1"], ["--r", "0", "1", "--bins", "0"], ["--r", "0", "1", "--bins", "1025"],
                  ["--r", "1", "1", "--bins", "4"], ["--r", "2", "1", "--bins", "4"], ["--r", "0", "1", "--bins", "4", "--log"],
                  ["--r", "-1", "1", "--bins", "4"], ["--r", "0", "inf", "--bins", "4"],
                  ["--r", "0", "1", "--bins", "4", "--q", "u,nothing"], ["--r", "0", "1", "--bins", "4", "--q", "h"],
                  ["--r", "0", "1", "--bins", "4", "--q", "u,rho,P,c,x"], ["--r", "0", "1", "--bins", "4", "--weight", "volume"],
                  ["--r", "0", "1", "--bins", "4", "--stride", "0"], ["--r", "0", "1", "--bins", "4", "--stride", "4", "--phase", "4"],
                  ["--r", "0", "1", "--bins", "4", "--phase", "-1"], ["--r", "0", "1", "--bins", "4", "--clip", "0,0,0,1,1"],
                  ["--r", "0", "1", "--bins", "4", "--clip", "1,0,0,0,1,1"]):
        with pytest.raises(SystemExit) as e:
            pairs.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
