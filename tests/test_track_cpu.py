"""CPU tests of the tracked particles (sph_track): the ABI mirrors (ctypes, Fortran) against the C header, the resources of
the kernels, the marshalling and every argument error that needs no device, the selection helpers and the dict builders
against plain numpy, the command line's parsing, and the replay of pack() (tests/track_ref.py) on hand-made keep vectors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, library, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import track_ref

FIELDS = ["capacity", "every", "flags"]
SPH_ERR_ARG = 1
CALLS = ["sph_track_begin", "sph_track_begin_dev", "sph_track_end", "sph_track_record", "sph_track_info", "sph_track_read",
         "sph_track_read_dev", "sph_track_fates", "sph_track_fates_dev"]
KERNELS = ("track_row", "track_repack", "track_bits", "track_prefix", "track_tags")


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    library()
    m.load()
    return m


# ---- 1. the ABI mirrors ----------------------------------------------------------------------------------------------------------
def test_descriptor_layout_constants_and_symbols(capi, tmp_path):
    got = c_layout(tmp_path, "sph_track_desc", FIELDS,
                   ['printf("nhead %d\\n", SPH_TRACK_NHEAD);', 'printf("ncol %d\\n", SPH_TRACK_NCOL);',
                    'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == C.sizeof(capi.TrackDesc) == 16
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.TrackDesc, f).offset, f
    assert int(got["nhead"]) == capi.TRACK_NHEAD == track_ref.NHEAD == len(capi.TRACK_HEAD) == 4
    assert int(got["ncol"]) == capi.TRACK_NCOL == track_ref.NCOL == len(capi.TRACK_COLUMNS) == 10
    assert got["abi"] == "1"                                        # the change is additive
    assert capi.TRACK_COLUMNS == "x y z vx vy vz u rho h alpha".split() == track_ref.COLUMNS
    assert capi.TRACK_HEAD == ["step", "t", "n", "n_live"] and capi.TRACK_FATES == ["fate", "step", "sink", "current_id"]
    assert (capi.TRACK_ALIVE, capi.TRACK_ACCRETED, capi.TRACK_CULLED) == (0, 1, 2)
    lib = C.CDLL(library())
    for s in CALLS:
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_TRACK_NHEAD = 4, SPH_TRACK_NCOL = 10", binding)
    for s in CALLS:
        assert re.search(rf"bind\(C, name='{s}'\)", binding), s


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "track_caller", """program track_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_track_desc) :: d
  type(c_ptr) :: ctx
  integer(c_int64_t), target :: rows, dropped, steps, nk, live
  integer(c_int32_t), target :: closed
  integer(c_int64_t) :: ids(3)
  real(c_double), allocatable, target :: head(:, :), body(:, :, :)
  integer(c_int32_t), target :: fates(4, 3)
  integer(c_int) :: st
  character(len=64) :: path
  logical :: on
  ctx = c_null_ptr
  d%capacity = 16_c_int64_t
  d%every = 2
  d%flags = 0
  ids = [0_c_int64_t, 5_c_int64_t, 2_c_int64_t]
  if (c_sizeof(d) /= 16) stop 1
  allocate(head(SPH_TRACK_NHEAD, 16), body(3, SPH_TRACK_NCOL, 16))
  st = sph_track_begin(ctx, d, 3_c_int64_t, ids)
  if (st == SPH_OK) stop 2
  st = sph_track_begin_dev(ctx, d, 3_c_int64_t, c_null_ptr)
  st = sph_track_record(ctx)
  st = sph_track_info(ctx, c_loc(rows), c_loc(dropped), c_loc(steps), c_loc(nk), c_loc(live), c_loc(closed))
  st = sph_track_read(ctx, 0_c_int64_t, 16_c_int64_t, c_loc(head), c_loc(body))
  st = sph_track_read_dev(ctx, 0_c_int64_t, 16_c_int64_t, c_null_ptr, c_null_ptr)
  st = sph_track_fates(ctx, c_loc(fates))
  st = sph_track_fates_dev(ctx, c_null_ptr)
  st = sph_track_end(ctx)
  if (st == SPH_OK) stop 3
  if (.false.) then
    st = sph_track_begin_env(ctx, 10, 4, path, on)
    st = sph_track_write(ctx, path)
  end if
  print *, st
end program track_caller
""")


# ---- 2. the kernels' resources -------------------------------------------------------------------------------------------------
@needs_hipcc
def test_track_kernels_fit_the_register_budget():
    k = resource_usage("track.hip", containing("track_"))
    for name in KERNELS:
        assert sum(name in n for n in k) == 1, (name, sorted(k))
    assert len(k) == len(KERNELS)
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 64, (name, r)             # nothing here holds more than a row's ten values
        assert r.get("Occupancy") == 8, (name, r)


# ---- 3. marshalling and the refusals -----------------------------------------------------------------------------------------------
def test_desc_marshalling_and_argument_errors(capi):
    d = capi.track_desc(100, every=3)
    assert (d.capacity, d.every, d.flags) == (100, 3, 0)
    d = capi.track_desc(2**40)                                       # an int64 capacity
    assert (d.capacity, d.every) == (2**40, 1)
    for bad in (dict(capacity=0), dict(capacity=-1), dict(capacity=2**63), dict(capacity=4, every=0), dict(capacity=4, every=-2),
                dict(capacity=4, every=2**31)):
        with pytest.raises(ValueError):
            capi.track_desc(**bad)
    assert capi.track_ids([3, 1, 2]).dtype == np.int64 and capi.track_ids(np.array([5], dtype=np.int32)).tolist() == [5]
    for bad in ([], [[1, 2]], [1.0, 2.0], 7):
        with pytest.raises(ValueError):
            capi.track_ids(bad)
    # every call refuses a null context before anything else
    lib = capi.load()
    out, ids, fates = np.zeros(40), np.zeros(2, dtype=np.int64), np.zeros(8, dtype=np.int32)
    for begin in (lib.sph_track_begin, lib.sph_track_begin_dev):
        assert begin(None, C.byref(d), 2, ids.ctypes.data) == SPH_ERR_ARG
    assert lib.sph_track_end(None) == SPH_ERR_ARG and lib.sph_track_record(None) == SPH_ERR_ARG
    assert lib.sph_track_info(None, None, None, None, None, None, None) == SPH_ERR_ARG
    for read in (lib.sph_track_read, lib.sph_track_read_dev):
        assert read(None, 0, 1, out.ctypes.data, out.ctypes.data) == SPH_ERR_ARG
    for f in (lib.sph_track_fates, lib.sph_track_fates_dev):
        assert f(None, fates.ctypes.data) == SPH_ERR_ARG


def test_columns_of_raw_rows(capi):
    head = np.arange(2.0 * 4).reshape(2, 4)
    body = np.arange(2.0 * 10 * 3).reshape(2, 10, 3)
    body[1, :, 2] = np.nan                                           # the third particle is gone in the second row
    t = capi.track_columns(head, body, dropped=5)
    assert t["step"].tolist() == [0, 4] and t["step"].dtype == np.int64 and t["t"].tolist() == [1.0, 5.0]
    assert t["n"].tolist() == [2, 6] and t["n_live"].tolist() == [3, 7] and t["dropped"] == 5
    for c, name in enumerate(capi.TRACK_COLUMNS):
        assert t[name].shape == (2, 3) and np.array_equal(t[name], body[:, c, :], equal_nan=True), name
    assert t["u"][0].tolist() == [18.0, 19.0, 20.0] and np.isnan(t["alpha"][1, 2]) and t["body"].shape == (2, 10, 3)
    assert capi.track_columns(np.zeros((0, 4)), np.zeros((0, 10, 7)))["x"].shape == (0, 7)
    for h, b in ((np.zeros((2, 3)), np.zeros((2, 10, 1))), (np.zeros((2, 4)), np.zeros((2, 9, 1))), (np.zeros((2, 4)), np.zeros((3, 10, 1))),
                 (np.zeros(4), np.zeros((1, 10, 1)))):
        with pytest.raises(ValueError):
            capi.track_columns(h, b)
    f = capi.track_fates_columns(np.array([[0, 0, -1, 7], [1, 3, 0, -1], [2, 5, -1, -1]], dtype=np.int32))
    assert f["fate"].tolist() == [0, 1, 2] and f["step"].tolist() == [0, 3, 5] and f["sink"].tolist() == [-1, 0, -1]
    assert f["current_id"].tolist() == [7, -1, -1]
    with pytest.raises(ValueError):
        capi.track_fates_columns(np.zeros((3, 3), dtype=np.int32))


# ---- 4. the selection helpers ---------------------------------------------------------------------------------------------------
def test_selection_helpers_against_numpy():
    from summersph_amd import track
    rng = np.random.default_rng(28)
    st = {k: rng.normal(size=500) * 10.0 for k in "xyz"}
    x, y, z = st["x"], st["y"], st["z"]
    got = track.sphere_ids(st, (1.0, -2.0, 0.5), 8.0)
    want = [i for i in range(500) if (x[i] - 1.0) ** 2 + (y[i] + 2.0) ** 2 + (z[i] - 0.5) ** 2 <= 64.0]
    assert got.dtype == np.int64 and got.tolist() == want and 0 < len(want) < 500
    assert track.sphere_ids(st, (0, 0, 0), 0.0).size == 0 and track.sphere_ids(st, (0, 0, 0), 1e9).size == 500
    R = np.hypot(x, y)
    got = track.ring_ids(st, 5.0, 12.0)
    assert got.tolist() == [i for i in range(500) if 25.0 <= x[i] ** 2 + y[i] ** 2 < 144.0] and np.all((R[got] > 4.99) & (R[got] < 12.01))
    thin = track.ring_ids(st, 5.0, 12.0, zmax=3.0)
    assert thin.tolist() == [i for i in got if abs(z[i]) <= 3.0] and 0 < thin.size < got.size
    assert track.ring_ids(st, 0.0, 5.0).size + got.size + track.ring_ids(st, 12.0, 1e9).size == 500      # half-open rings tile
    assert track.stride_ids(10, 3).tolist() == [0, 3, 6, 9] and track.stride_ids(10, 3, 2).tolist() == [2, 5, 8]
    assert track.stride_ids(10, 100).tolist() == [0] and track.stride_ids(0, 1).size == 0 and track.stride_ids(5, 1).tolist() == [0, 1, 2, 3, 4]
    labels = np.array([-1, 0, 2, 0, 1, 2, -1, 0], dtype=np.int32)
    assert track.label_ids(labels, 0).tolist() == [1, 3, 7] and track.label_ids(labels, [1, 2]).tolist() == [2, 4, 5]
    assert track.label_ids(labels, 9).size == 0 and track.label_ids(labels, 0).dtype == np.int64
    for call in (lambda: track.sphere_ids(st, (0, 0, 0), -1.0), lambda: track.ring_ids(st, 3.0, 2.0), lambda: track.stride_ids(5, 0),
                 lambda: track.stride_ids(5, 1, -1), lambda: track.label_ids(np.zeros((2, 2)), 0),
                 lambda: track.sphere_ids({"x": x, "y": y[:3], "z": z}, (0, 0, 0), 1.0)):
        with pytest.raises(ValueError):
            call()


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_parses_its_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, track
    a = track.parse_args(["save.txt", "--steps", "500", "--every", "5", "--dt", "1e-2", "--stride", "100", "-o", "track.npz", "--json"])
    assert (a.save, a.steps, a.every, a.dt, a.stride, a.out, a.json) == ("save.txt", 500, 5, 1e-2, 100, "track.npz", True)
    assert a.capacity == 101 and not (a.variable or a.self_gravity or a.accrete)
    a = track.parse_args(["s.txt", "--steps", "10", "--sphere", "1", "2", "3", "4", "--variable", "--self-gravity", "--accrete"])
    assert a.sphere == [1.0, 2.0, 3.0, 4.0] and a.capacity == 11 and a.variable and a.self_gravity and a.accrete
    a = track.parse_args(["s.txt", "--steps", "10", "--ring", "5", "12", "--zmax", "2", "--capacity", "3"])
    assert a.ring == [5.0, 12.0] and a.zmax == 2.0 and a.capacity == 3
    gas = np.zeros((40, 9))
    gas[:, 0] = np.arange(40.0)
    assert track.select(a, gas).tolist() == list(range(5, 12))
    np.save(tmp_path / "ids.npy", np.array([7, 3, 11]))
    a = track.parse_args(["s.txt", "--steps", "1", "--ids", str(tmp_path / "ids.npy")])
    assert track.select(a, gas).tolist() == [7, 3, 11]               # the order is kept
    assert track.select(track.parse_args(["s.txt", "--steps", "1", "--stride", "16"]), gas).tolist() == [0, 16, 32]

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    for extra in (["--steps", "5"], ["--steps", "-1", "--stride", "2"], ["--steps", "5", "--every", "0", "--stride", "2"],
                  ["--steps", "5", "--dt", "nan", "--stride", "2"], ["--steps", "5", "--stride", "0"],
                  ["--steps", "5", "--stride", "2", "--ring", "1", "2"], ["--steps", "5", "--ring", "3", "2"],
                  ["--steps", "5", "--sphere", "0", "0", "0", "-1"], ["--steps", "5", "--stride", "2", "--zmax", "1"],
                  ["--steps", "5", "--stride", "2", "--capacity", "0"]):
        with pytest.raises(SystemExit) as e:
            track.main(["missing.txt", "-o", str(tmp_path / "o.npz")] + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
    # the summary of hand-made rows and fates
    head = np.array([[0.0, 0.0, 100.0, 4.0], [3.0, 0.03, 97.0, 1.0]])
    t = capi.track_columns(head, np.zeros((2, 10, 4)), 1)
    fates = capi.track_fates_columns(np.array([[0, 0, -1, 5], [1, 1, 0, -1], [1, 2, 1, -1], [2, 2, -1, -1]], dtype=np.int32))
    s = track.summary(t, fates, 1)
    assert s == {"rows": 2, "dropped": 1, "n_tracked": 4, "n_live": 1,
                 "fates": {"alive": 1, "culled": 1, "accreted": 2, "per_sink": {"0": 1, "1": 1}},
                 "first": {"step": 0.0, "t": 0.0, "n": 100.0, "n_live": 4.0}, "last": {"step": 3.0, "t": 0.03, "n": 97.0, "n_live": 1.0}}


# ---- 6. the replay of pack() ---------------------------------------------------------------------------------------------------------
def test_replay_of_pack_on_hand_made_keep_vectors():
    ids = np.array([5, 0, 7, 3, 6])                                  # unsorted, as a caller may give them
    cases = {
        "none": (np.ones(8, int), [5, 0, 7, 3, 6], []),
        "first": ([0, 1, 1, 1, 1, 1, 1, 1], [4, -1, 6, 2, 5], [1]),
        "last": ([1, 1, 1, 1, 1, 1, 1, 0], [5, 0, -1, 3, 6], [2]),
        "all": (np.zeros(8, int), [-1] * 5, [0, 1, 2, 3, 4]),
        "alternating": ([1, 0, 1, 0, 1, 0, 1, 0], [-1, 0, -1, -1, 3], [0, 2, 3]),
        "untracked only": ([1, 0, 0, 1, 0, 1, 1, 1], [2, 0, 4, 1, 3], []),
    }
    for name, (keep, want, gone) in cases.items():
        new, removed = track_ref.replay_pack(ids, keep)
        assert new.tolist() == want and np.flatnonzero(removed).tolist() == gone, name
        # against pack() itself on an array of names
        names = np.arange(100, 108)
        packed = names[np.asarray(keep).astype(bool)]
        for k in range(5):
            assert (packed[new[k]] == names[ids[k]]) if new[k] >= 0 else (names[ids[k]] not in packed), (name, k)
    # two packs in a row, and an id that is gone stays gone
    a, r1 = track_ref.replay_pack(ids, [1, 1, 1, 0, 1, 1, 1, 1])
    b, r2 = track_ref.replay_pack(a, [0, 1, 1, 1, 1, 1, 1])
    assert a.tolist() == [4, 0, 6, -1, 5] and b.tolist() == [3, -1, 5, -1, 4]
    assert np.flatnonzero(r1).tolist() == [3] and np.flatnonzero(r2).tolist() == [1]
    # the helpers beside it
    m = np.array([1.0, 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -29, 2.0])
    assert track_ref.index_by_mass(m[[3, 0, 2]], m).tolist() == [1, -1, 2, 0]
    assert track_ref.keep_of(m, m[[0, 2, 3]]).tolist() == [True, False, True, True]
    ones = np.frombuffer(b"\xff" * 16, dtype=np.float64)             # the log's fill
    assert track_ref.same_values([1.0, ones[0]], [1.0, np.nan]) and not track_ref.same_values([1.0, 2.0], [1.0, np.nan])
    assert not track_ref.same_values([0.0], [-0.0]) and not track_ref.same_values([1.0], [1.0, 1.0]) and np.all(np.isnan(ones))
    f = {"x": np.array([1.0, 2.0, 3.0]), "u": np.array([4.0, 5.0, 6.0]), "h": 2.5, "rho": None}
    row = track_ref.body_row(f, [2, -1, 0])
    assert row.shape == (10, 3) and row[0].tolist()[::2] == [3.0, 1.0] and np.isnan(row[0, 1]) and row[6, 0] == 6.0
    assert row[8].tolist()[::2] == [2.5, 2.5] and np.all(np.isnan(row[7])) and np.all(np.isnan(row[:, 1]))
