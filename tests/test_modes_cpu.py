"""CPU tests of the mode sums (sph_modes): the ABI mirrors (ctypes, Fortran) against the C header, the resources of the
kernels, the tables of sph_modes_tables against the formulas and every refusal that needs no device, sph_modes_finish on
hand-made limbs, the numpy restatement (tests/modes_ref.py) against its longdouble version within the spiral sums' bound,
modes.finish on hand values and the command line's parsing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, library, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import modes_ref

FIELDS = ["centre", "centre_v", "normal", "r_min", "r_max", "z_max", "p_min", "p_max", "r_ref", "n_r", "m_max", "n_p", "sink",
          "weight", "n_q", "q", "n_rows", "flags", "reserved"]
SPH_ERR_ARG = 1


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    library()
    m.load()
    return m


# ---- 1. the ABI mirrors ---------------------------------------------------------------------------------------------------------
def test_descriptor_layout_and_symbols(capi, tmp_path):
    consts = ["SPH_MODES_MAX_M", "SPH_MODES_MAX_RINGS", "SPH_MODES_MAX_P", "SPH_MODES_ROW(0)", "SPH_MODES_ROW(15)", "SPH_MODES_W_ONE",
              "SPH_MODES_W_MASS", "SPH_MODES_LOG"]
    got = c_layout(tmp_path, "sph_modes_desc", FIELDS,
                   ['printf("consts' + " %d" * len(consts) + '\\n", ' + ", ".join(consts) + ');', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == C.sizeof(capi.ModesDesc) == 168
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.ModesDesc, f).offset, f
    mine = [capi.MODES_MAX_M, capi.MODES_MAX_RINGS, capi.MODES_MAX_P, capi.modes_row(0), capi.modes_row(15), capi.MODES_W_ONE,
            capi.MODES_W_MASS, capi.MODES_LOG]
    assert got["consts"] == " ".join(str(v) for v in mine) == "8 1024 256 -1 -16 0 1 1"
    assert got["abi"] == "1"                                        # the change is additive
    lib = C.CDLL(library())
    for s in ("sph_modes", "sph_modes_dev", "sph_modes_tables", "sph_modes_finish"):
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_MODES_MAX_M = 8, SPH_MODES_MAX_RINGS = 1024, SPH_MODES_MAX_P = 256", binding)
    assert re.search(r"SPH_MODES_W_ONE = 0, SPH_MODES_W_MASS = 1, SPH_MODES_LOG = 1", binding)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "modes_caller", """program modes_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_modes_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), target :: sums(2 * 3 * (4 + 5))
  integer(c_int64_t), target :: raw(2, 2 * 3 * (4 + 5)), ring_counts(4), counts(4)
  integer(c_int32_t), target :: e
  real(c_double) :: edge(5), p(5)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%centre = 0.0_c_double
  d%centre_v = 0.0_c_double
  d%normal = [0.0_c_double, 0.0_c_double, 1.0_c_double]
  d%r_min = 1.0_c_double
  d%r_max = 16.0_c_double
  d%z_max = huge(1.0_c_double)
  d%p_min = -2.0_c_double
  d%p_max = 2.0_c_double
  d%r_ref = 1.0_c_double
  d%n_r = 4
  d%m_max = 2
  d%n_p = 5
  d%sink = -1
  d%weight = SPH_MODES_W_MASS
  d%n_q = 1
  d%q = SPH_F_U
  d%n_rows = 0
  d%flags = SPH_MODES_LOG
  d%reserved = 0
  if (c_sizeof(d) /= 168) stop 1
  st = sph_modes_tables(d, edge, p)
  if (st /= SPH_OK) stop 2
  if (edge(1) /= 1.0_c_double .or. edge(3) /= 4.0_c_double .or. edge(5) /= 16.0_c_double) stop 3
  if (p(1) /= -2.0_c_double .or. p(3) /= 0.0_c_double .or. p(5) /= 2.0_c_double) stop 4
  raw = 0
  raw(1, 2) = 3
  e = 62
  st = sph_modes_finish(d, e, raw, sums)
  if (st /= SPH_OK .or. sums(2) /= 3.0_c_double .or. sums(1) /= 0.0_c_double) stop 5
  st = sph_modes(ctx, d, c_null_ptr, c_loc(sums), 54_c_int64_t, c_loc(raw), c_loc(e), c_loc(ring_counts), c_loc(counts))
  st = sph_modes_dev(ctx, d, c_null_ptr, c_null_ptr, 54_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
  print *, st, edge
end program modes_caller
""")


# ---- 2. the kernels' resources --------------------------------------------------------------------------------------------------
@needs_hipcc
def test_mode_kernels_fit_the_register_budget():
    """No scratch and no spills anywhere; at most 128 VGPRs (four wavefronts per SIMD), except modes_spiral with six, eight and
    nine m, whose 8 (m_max + 1) accumulator registers come on top of sincos' working set: the compiler's own figures, 143, 135
    and 149, are the ceilings there (three wavefronts per SIMD; DESIGN.md section 29 says why the m are not split over two
    launches)."""
    over = {6: 143, 8: 135, 9: 149}
    k = resource_usage("modes.hip", containing("modes_"))
    for name, count in (("modes_select", 1), ("modes_head", 1), ("modes_rings", 1), ("modes_spiral", 9), ("modes_sum", 1),
                        ("modes_convert", 1)):
        assert sum(name in n for n in k) == count, (name, sorted(k))
    assert len(k) == 14
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        m1 = re.search(r"modes_spiralILi(\d)E", name)
        budget = over.get(int(m1.group(1)), 128) if m1 else 128
        assert 0 < r.get("VGPRs", 999) <= budget, (name, r)


# ---- 3. the tables and the refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_min,r_max,n_r,log", [(0.0, 1.0, 7, False), (10.0, 200.0, 40, True), (0.1, 0.5, 1, False), (2.0, 3.0, 1, True),
                                                 (0.0, 8.0, 1024, False), (1e-3, 1e2, 1024, True)])
def test_ring_edges_match_the_formulas(capi, r_min, r_max, n_r, log):
    d = capi.modes_desc((r_min, r_max), n_r, 2, log=log)
    e, p = capi.modes_tables(d)
    want = modes_ref.edges_formula(r_min, r_max, n_r, log)
    assert p.shape == (0,) and e.shape == (n_r + 1,) and e[0] == r_min and e[-1] == r_max and np.all(np.diff(e) > 0.0)
    # pow is not correctly rounded: two libms differ by an ulp of the power, which the product with r_min can turn into two
    assert np.all(np.abs(e - want) <= 2.0 * np.spacing(np.abs(want)))
    if not log:
        assert np.array_equal(e, want)
    pd = capi.profile_desc(r_min, r_max, n_r, log=log)               # sph_profile's rule: its own table, from its finish
    table = capi.profile_finish(pd, capi.Params(), np.zeros((n_r, capi.PROFILE_NSUM)))
    assert np.array_equal(table["R_lo"], e[:-1]) and np.array_equal(table["R_hi"], e[1:])


@pytest.mark.parametrize("p_min,p_max,n_p", [(-32.0, 32.0, 129), (0.5, 0.5, 1), (3.0, 7.0, 1), (-1.0, 2.0, 256), (0.0, 1.0, 2),
                                             (2.0, 2.0, 5)])
def test_p_table_matches_the_formula(capi, p_min, p_max, n_p):
    d = capi.modes_desc((1.0, 2.0), 3, 0, spiral=(p_min, p_max, n_p), r_ref=1.5)
    e, p = capi.modes_tables(d)
    assert e.shape == (4,) and np.array_equal(p, modes_ref.p_formula(p_min, p_max, n_p))
    assert p[0] == p_min and (n_p == 1 or p[-1] == p_max)
    lib, out = capi.load(), np.full(8, -1.0)
    assert lib.sph_modes_tables(C.byref(d), None, None) == 0          # either table may be left out
    assert lib.sph_modes_tables(C.byref(d), out.ctypes.data, None) == 0 and np.array_equal(out[:4], e) and out[4] == -1.0


def _refused(capi, d):
    edges, p = np.zeros(1100), np.zeros(300)
    st = capi.load().sph_modes_tables(C.byref(d), edges.ctypes.data, p.ctypes.data)
    if st == SPH_ERR_ARG:
        assert not edges.any() and not p.any()                       # nothing is written on an error
    return st == SPH_ERR_ARG


def test_argument_errors(capi):
    lib = capi.load()
    good = dict(r_range=(0.5, 2.0), n_r=4, m_max=3, q=capi.modes_row(1), n_rows=2, spiral=(-2.0, 2.0, 5), r_ref=1.5, centre=(1, 2, 3),
                centre_v=(0, 0, 0))

    def desc(**kw):
        a = dict(good); a.update(kw)
        return capi.modes_desc(**a)

    def edit(**fields):
        dd = desc()
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(dd, k)[v[0]] = v[1]
            else:
                setattr(dd, k, v)
        return dd

    d = desc()
    assert not _refused(capi, d)
    assert lib.sph_modes_tables(None, None, None) == SPH_ERR_ARG                             # null descriptor
    bad = {
        "n_r 0": edit(n_r=0), "n_r 1025": edit(n_r=1025), "n_r -1": edit(n_r=-1),
        "m_max -1": edit(m_max=-1), "m_max 9": edit(m_max=9), "n_p -1": edit(n_p=-1), "n_p 257": edit(n_p=257),
        "r_min == r_max": edit(r_min=2.0), "r_min > r_max": edit(r_min=3.0), "r_min < 0": edit(r_min=-0.5), "r_min nan": edit(r_min=np.nan),
        "r_max inf": edit(r_max=np.inf), "log r_min 0": desc(r_range=(0.0, 2.0), log=True),
        "coinciding edges": desc(r_range=(1.0, 1.0 + 4e-16)), "z_max nan": edit(z_max=np.nan),
        "normal zero": desc(normal=(0, 0, 0)), "normal nan": edit(normal=(1, np.nan)), "normal inf": edit(normal=(2, np.inf)),
        "centre nan": edit(centre=(0, np.nan)), "centre_v inf": edit(centre_v=(2, np.inf)), "sink -2": edit(sink=-2),
        "r_ref 0": edit(r_ref=0.0), "r_ref < 0": edit(r_ref=-1.0), "r_ref nan": edit(r_ref=np.nan), "r_ref inf": edit(r_ref=np.inf),
        "p_min nan": edit(p_min=np.nan), "p_max inf": edit(p_max=np.inf), "p_min -inf": edit(p_min=-np.inf),
        "p_min > p_max": edit(p_min=3.0),
        "n_q 2": edit(n_q=2), "n_q -1": edit(n_q=-1), "field id": edit(q=19), "field id 99": edit(q=99), "row id": edit(q=capi.modes_row(2)),
        "n_rows 17": edit(n_rows=17), "n_rows -1": edit(n_rows=-1), "flags": edit(flags=2), "flags -": edit(flags=-1),
        "reserved 0": edit(reserved=(0, 1)), "reserved 2": edit(reserved=(2, 7)), "weight": edit(weight=2), "weight -": edit(weight=-1),
    }
    for name, dd in bad.items():
        assert _refused(capi, dd), name
    # what only matters with spiral sums is not looked at without them; a sink's centre may be anything
    for dd in (edit(n_p=0, r_ref=0.0, p_min=np.nan), edit(sink=0, centre=(0, np.nan)), edit(n_q=0, q=99), edit(p_min=2.0)):
        assert not _refused(capi, dd)
    with pytest.raises(ValueError):
        capi.modes_desc((0, 1), 4, 2, sink=0, centre=(0, 0, 0))
    # the calls themselves refuse a null context before anything else; finish its null pointers
    sums = np.zeros(2 * 4 * 9)
    for fn in (lib.sph_modes, lib.sph_modes_dev):
        assert fn(None, C.byref(d), None, sums.ctypes.data, sums.size, None, None, None, None) == SPH_ERR_ARG
    ex, raw = np.zeros(1, np.int32), np.zeros((sums.size, 2), np.uint64)
    assert lib.sph_modes_finish(None, ex.ctypes.data, raw.ctypes.data, sums.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_modes_finish(C.byref(d), None, raw.ctypes.data, sums.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_modes_finish(C.byref(d), ex.ctypes.data, None, sums.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_modes_finish(C.byref(d), ex.ctypes.data, raw.ctypes.data, None) == SPH_ERR_ARG
    assert lib.sph_modes_finish(C.byref(edit(m_max=9)), ex.ctypes.data, raw.ctypes.data, sums.ctypes.data) == SPH_ERR_ARG


# ---- 4. sph_modes_finish on hand-made limbs -------------------------------------------------------------------------------------
def test_finish_rounds_once(capi):
    values = [0, 1, -1, -12345, (1 << 64) + 5, -((1 << 64) + 5),          # wider than 64 bits, both signs
              (1 << 53) + 1, -((1 << 53) + 1),                            # a tie: to even, 2^53
              (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6,                # ties to even, up and down
              (3 << 100) + 1, (1 << 117) + (1 << 64) + 1,                 # above a tie by a bit far below
              (1 << 117) + (1 << 64), (1 << 117) + (3 << 64),             # exactly on a tie across the limbs (even / odd)
              -((1 << 117) + (3 << 64)), (1 << 126) + 12345678901234567890, -(1 << 127), (1 << 127) - 1,
              (1 << 64) - 1, 1 << 64, -(1 << 64), (1 << 63), -(1 << 63)]
    assert len(values) == 24
    d = capi.modes_desc((0.0, 1.0), 2, 2, spiral=(0.0, 1.0, 2))            # 2 * 3 * (2 + 2) = 24 sums
    raw = np.array([modes_ref.to_limbs(v) for v in values], dtype=np.uint64)
    assert [modes_ref.from_limbs(*r) for r in raw] == values
    for e in (62, 0, -40, 75):
        ring, spiral = capi.modes_finish(d, e, raw)
        assert ring.shape == (2, 3, 2) and spiral.shape == (3, 2, 2)
        got = np.concatenate([ring.reshape(-1), spiral.reshape(-1)])
        assert got.tolist() == [modes_ref.finish_int(v, e) for v in values], e
        again = capi.modes_finish(d, np.array([e], np.int32), capi.modes_split(d, raw.view(np.int64)))   # the pair, as int64
        assert np.array_equal(again[0], ring) and np.array_equal(again[1], spiral)
    assert capi.modes_finish(d, 62, raw)[0].reshape(-1)[6] == 2.0 ** 53
    d0 = capi.modes_desc((0.0, 1.0), 12, 0)
    ring, spiral = capi.modes_finish(d0, 62, raw)
    assert spiral is None and ring.shape == (12, 1, 2) and ring[2, 0, 0] == float((1 << 64) + 5)


# ---- 5. the restatement against its longdouble version --------------------------------------------------------------------------
def _disc(n, seed, r_lo=10.0, r_hi=100.0):
    rng = np.random.default_rng(seed)
    R = np.sqrt(rng.uniform(r_lo * r_lo, r_hi * r_hi, n))
    ph = rng.uniform(-np.pi, np.pi, n)
    pos = np.stack([R * np.cos(ph), R * np.sin(ph), rng.normal(0.0, 1.0, n)], axis=1)
    return pos, rng.uniform(1e-6, 2e-6, n), rng.normal(size=n)


@pytest.mark.parametrize("normal,signed", [((0.0, 0.0, 1.0), False), ((0.3, -0.2, 1.0), True)])
def test_restatement_within_the_bound_of_the_longdouble_sums(normal, signed):
    assert np.finfo(np.longdouble).eps < 2e-19                      # 80-bit: the yardstick is finer than the bound by 2^-11
    pos, m, A = _disc(2000, 1)
    pos[17] = 0.0                                                   # a particle at the centre
    edges = modes_ref.edges_formula(0.0, 90.0, 7)
    p = modes_ref.p_formula(-32.0, 32.0, 129)
    r = modes_ref.modes(pos, m, A if signed else None, edges=edges, m_max=8, normal=normal, p=p, r_ref=10.0, n_owned=1900)
    assert r["counts"][3] == 1 and r["counts"][0] > 1000 and r["counts"][1] > 100 and sum(r["counts"][:3]) == 1900
    assert r["ring_counts"].sum() == r["counts"][0] and r["ring_counts"][0] > 0
    ring, spiral = modes_ref.truth(pos, r["w"], r["sel"], edges, 8, p, normal=normal, r_ref=10.0)
    bound = modes_ref.spiral_bound(r["ws"], r["u"], 8, p)
    err = np.abs(r["spiral"].astype(np.longdouble) - spiral).max(axis=2).astype(np.float64)
    print("worst spiral error / bound", float(np.max(err / bound)))
    assert bound.shape == err.shape == (9, 129) and np.all(err <= bound)
    # the ring sums: 2 m roundings of the recurrence, the term's own and the half quantum, against sum |w| of the ring
    ring_of = np.searchsorted(edges, modes_ref.place(pos[r["sel"]], (0, 0, 0), normal)[3], side="right") - 1
    wsum = np.bincount(ring_of, weights=np.abs(r["w"]), minlength=7)
    rerr = np.abs(r["ring"].astype(np.longdouble) - ring).astype(np.float64)
    assert np.all(rerr <= wsum[:, None, None] * (2.0 * np.arange(9)[None, :, None] + 8.0) * 2.0 ** -53)
    # the limbs are the doubles, and the centre is in ring 0's m = 0 sum but not in the spiral's
    for blk, raw in ((r["ring"], r["raw_ring"]), (r["spiral"], r["raw_spiral"])):
        for v, limbs in zip(blk.reshape(-1), raw.reshape(-1, 2)):
            assert modes_ref.finish_int(modes_ref.from_limbs(*limbs), r["exp"]) == v
    if not signed:
        assert abs(r["ring"][:, 0, 0].sum() - r["w"].sum()) <= 1e-15 * r["w"].sum()
        l0 = 64
        assert p[l0] == 0.0 and abs(r["spiral"][0, l0, 0] - (r["w"].sum() - m[17])) <= 1e-15 * r["w"].sum()


def test_restatement_on_hand_values():
    # four particles at phi = pi and one at phi = 0: C_1 = -3 w exactly, S_m = 0, C_2 = 5 w; a sixth in the second ring
    w = 2.0 ** -20
    pos = np.array([[-1.0, 0.0, 0.0]] * 4 + [[1.0, 0.0, 0.0], [0.0, 3.0, 0.5]])
    r = modes_ref.modes(pos, np.full(6, w), edges=[0.5, 2.0, 4.0], m_max=2, p=[0.0], r_ref=1.0)
    assert r["exp"] == -18 and r["counts"] == (6, 0, 0, 0) and r["ring_counts"].tolist() == [5, 1]
    assert r["ring"][0].tolist() == [[5 * w, 0.0], [-3 * w, 0.0], [5 * w, 0.0]]
    assert r["ring"][1].tolist() == [[w, 0.0], [0.0, w], [-w, 0.0]]
    assert modes_ref.from_limbs(*r["raw_ring"][0, 1, 0]) == -3 << 60 and int(r["raw_ring"][0, 1, 0, 1]) == (1 << 64) - 1
    assert r["spiral"][:, 0, 0].tolist() == [6 * w, -3 * w, 4 * w] and r["spiral"][:, 0, 1].tolist() == [0.0, w, 0.0]
    # z cut, ghosts and a NaN weight
    r = modes_ref.modes(pos, np.array([w, w, np.nan, w, w, w]), edges=[0.5, 2.0, 4.0], m_max=1, z_max=0.5, n_owned=5)
    assert r["counts"] == (4, 0, 1, 0) and r["ring"][0, 1, 0] == -2 * w
    r = modes_ref.modes(pos, np.full(6, w), edges=[0.5, 2.0, 4.0], m_max=1, z_max=0.5)
    assert r["counts"] == (5, 1, 0, 0)                              # |z'| == z_max is outside


# ---- 6. modes.finish ------------------------------------------------------------------------------------------------------------
def test_finish_on_hand_computed_values():
    from summersph_amd import modes
    ring = np.array([[[4.0, 0.0], [0.0, 2.0], [-3.0, 4.0]],
                     [[0.0, 0.0], [0.0, 0.0], [0.0, 0.0]],
                     [[2.0, 0.0], [-1.0, 0.0], [1.0, -1.0]]])
    f = modes.finish(ring)
    assert set(f) == {"A", "phase"} and f["A"].shape == f["phase"].shape == (3, 3)
    assert f["A"][0].tolist() == [1.0, 0.5, 1.25] and f["A"][2].tolist() == [1.0, 0.5, np.sqrt(2.0) / 2.0]
    assert np.all(np.isnan(f["A"][1])) and np.all(np.isnan(f["phase"][:, 0]))           # an empty ring; m = 0 has no phase
    assert f["phase"][0, 1] == np.pi / 2 and f["phase"][2, 1] == np.pi and f["phase"][2, 2] == -np.pi / 8
    assert f["phase"][0, 2] == np.arctan2(4.0, -3.0) / 2
    p = np.array([-2.0, 0.0, 4.0])
    spiral = np.array([[[1.0, 0.0], [8.0, 0.0], [0.0, 1.0]],
                       [[0.0, 2.0], [1.0, 0.0], [0.0, 0.0]],
                       [[0.0, 0.0], [0.0, 4.0], [3.0, 4.0]]])
    f = modes.finish(ring, spiral, p)
    assert f["spectrum"].tolist() == [[0.125, 1.0, 0.125], [0.25, 0.125, 0.0], [0.0, 0.5, 0.625]]      # over CS[0] at p = 0
    assert f["p_peak"].tolist() == [0.0, -2.0, 4.0]
    assert np.isnan(f["pitch"][0]) and f["pitch"][1] == np.arctan(-0.5) and f["pitch"][2] == np.arctan(0.5)
    f = modes.finish(ring, spiral[:, [0, 2]], p[[0, 2]])                                    # no p = 0: over the rings' sum of w
    assert f["spectrum"][2].tolist() == [0.0, 5.0 / 6.0]
    f = modes.finish(np.zeros((2, 3, 2)), np.zeros((3, 3, 2)), p)
    assert np.all(np.isnan(f["spectrum"])) and np.all(np.isnan(f["A"]))
    for bad in (lambda: modes.finish(ring[0]), lambda: modes.finish(ring, spiral[:2], p), lambda: modes.finish(ring, spiral),
                lambda: modes.finish(ring, spiral, p[:2])):
        with pytest.raises(ValueError):
            bad()
    a = np.array([modes_ref.to_limbs(v) for v in (5, -5, (1 << 64) - 1)], dtype=np.uint64)
    b = np.array([modes_ref.to_limbs(v) for v in (7, 3, 1)], dtype=np.uint64)
    assert [modes_ref.from_limbs(*r) for r in modes.add_raw(a, b)] == [12, -2, 1 << 64]


# ---- 7. the command line --------------------------------------------------------------------------------------------------------
def test_cli_parses_its_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, modes
    a = modes.parse_args(["save275.txt", "-o", "modes.npz", "--rings", "10", "200", "40", "--log", "--mmax", "8", "--spiral", "-32", "32",
                          "129", "--sink", "0", "--json"])
    assert a.r_range == (10.0, 200.0) and a.n_r == 40 and a.log and a.mmax == 8 and a.spiral == (-32.0, 32.0, 129) and a.sink == 0
    assert a.centre is None and a.normal == (0.0, 0.0, 1.0) and a.weight == "mass" and a.q is None and a.json and a.rref == 1.0
    a = modes.parse_args(["s.txt", "-o", "o.npz", "--rings", "0", "5", "3", "--centre", "1,2,3", "--normal", "0,1,1", "--q", "u",
                          "--weight", "one", "--zmax", "2"])
    assert a.centre == (1.0, 2.0, 3.0) and a.normal == (0.0, 1.0, 1.0) and a.q == "u" and a.spiral is None and a.mmax == 8

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    base = ["missing.txt", "-o", str(tmp_path / "o.npz")]
    ok = ["--rings", "1", "2", "4"]
    for extra in ([], ["--rings", "1", "2"], ["--rings", "1", "2", "0"], ["--rings", "1", "2", "1025"], ["--rings", "2", "2", "4"],
                  ["--rings", "3", "2", "4"], ["--rings", "-1", "2", "4"], ["--rings", "0", "2", "4", "--log"],
                  ["--rings", "1", "inf", "4"], ["--rings", "1", "2", "x"], ok + ["--mmax", "9"], ok + ["--mmax", "-1"],
                  ok + ["--spiral", "-1", "1"], ok + ["--spiral", "1", "-1", "5"], ok + ["--spiral", "-1", "1", "0"],
                  ok + ["--spiral", "-1", "1", "257"], ok + ["--spiral", "-1", "nan", "5"], ok + ["--spiral", "-1", "1", "5", "--rref", "0"],
                  ok + ["--sink", "-1"], ok + ["--sink", "0", "--centre", "0,0,0"], ok + ["--centre", "0,0"], ok + ["--normal", "0,0,0"],
                  ok + ["--normal", "0,nan,1"], ok + ["--zmax", "nan"], ok + ["--weight", "volume"], ok + ["--q", "nothing"],
                  ok + ["--q", "h"]):
        with pytest.raises(SystemExit) as e:
            modes.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
