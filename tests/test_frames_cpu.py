"""CPU tests of the movie of a run (sph_frames): the descriptor's layout against the header and the Fortran binding, the
kernels' resources, the marshalling and the command line's arguments, frames.mean, and the restatement (tests/frames_ref.py):
its footprint, its node sums and the cadence rule on hand cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, library, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import frames_ref

FIELDS = ["rot", "centre", "lo", "hi", "clip_lo", "clip_hi", "h", "dt_frame", "capacity", "n_u", "n_v", "every", "centre_sink", "nq",
          "fields", "reserved"]
CALLS = ["sph_frames_begin", "sph_frames_end", "sph_frames_record", "sph_frames_rewind", "sph_frames_info", "sph_frames_read",
         "sph_frames_read_dev", "sph_frame", "sph_frame_dev"]
KERNELS = ("frames_maxima", "frames_head", "frames_clear", "frames_splat", "frames_finish", "frames_init")


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    library()
    m.load()
    return m


# ---- 1. the ABI mirrors ----------------------------------------------------------------------------------------------------------
def test_descriptor_layout_constants_and_symbols(capi, tmp_path):
    got = c_layout(tmp_path, "sph_frames_desc", FIELDS,
                   ['printf("nhead %d\\n", SPH_FRAMES_NHEAD);', 'printf("abi %d\\n", SPH_ABI_VERSION);',
                    'printf("maxq %d\\n", SPH_FRAMES_MAX_FIELDS);', 'printf("gone %d\\n", SPH_FRAMES_SINK_GONE);'])
    assert int(got["size"]) == C.sizeof(capi.FramesDesc) == 240
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.FramesDesc, f).offset, f
    assert int(got["nhead"]) == capi.FRAMES_NHEAD == 16 and int(got["maxq"]) == capi.FRAMES_MAX_FIELDS == 3
    assert int(got["gone"]) == capi.FRAMES_SINK_GONE == 1 and capi.FRAMES_OK == 0
    assert got["abi"] == "1"                                        # the change is additive
    lib = C.CDLL(library())
    for s in CALLS:
        assert s in capi.SYMBOLS and hasattr(lib, s), s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_FRAMES_NHEAD = 16, SPH_FRAMES_MAX_FIELDS = 3", binding)
    for s in CALLS:
        assert re.search(rf"bind\(C, name='{s}'\)", binding), s


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "frames_caller", """program frames_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_frames_desc) :: d
  type(c_ptr) :: ctx
  integer(c_int64_t), target :: rows, dropped, steps
  real(c_double), allocatable, target :: head(:, :), planes(:, :, :, :)
  character(len=256) :: path
  logical :: on
  integer :: nodes
  integer(c_int) :: st
  ctx = c_null_ptr
  d%rot = 0.0_c_double
  d%rot(1) = 1.0_c_double; d%rot(5) = 1.0_c_double; d%rot(9) = 1.0_c_double
  d%centre = 0.0_c_double
  d%lo = -1.0_c_double; d%hi = 1.0_c_double
  d%clip_lo = -huge(1.0_c_double); d%clip_hi = huge(1.0_c_double)
  d%h = 0.0_c_double; d%dt_frame = 0.5_c_double
  d%capacity = 4; d%n_u = 8; d%n_v = 6; d%every = 0; d%centre_sink = -1; d%nq = 1
  d%fields = [6, 0, 0]
  d%reserved = 0
  if (c_sizeof(d) /= 240) stop 1
  allocate(head(SPH_FRAMES_NHEAD, 4), planes(6, 8, 2, 4))
  st = sph_frames_begin(ctx, d)
  if (st == SPH_OK) stop 2
  st = sph_frames_record(ctx)
  st = sph_frames_rewind(ctx)
  st = sph_frames_info(ctx, c_loc(rows), c_loc(dropped), c_loc(steps))
  st = sph_frames_read(ctx, 0_c_int64_t, 4_c_int64_t, c_loc(head), c_loc(planes))
  st = sph_frames_read_dev(ctx, 0_c_int64_t, 4_c_int64_t, c_null_ptr, c_null_ptr)
  st = sph_frame(ctx, d, c_loc(head), c_loc(planes), 96_c_int64_t)
  st = sph_frame_dev(ctx, d, c_null_ptr, c_null_ptr, 96_c_int64_t)
  st = sph_frames_end(ctx)
  if (st == SPH_OK) stop 3
  st = sph_frames_begin_env(ctx, d%lo, d%hi, 10, path, on, nodes)
  if (on) st = sph_frames_write(ctx, path, nodes)
  print *, st, SPH_FRAMES_SINK_GONE
end program frames_caller
""")


# ---- 2. the kernels' resources -------------------------------------------------------------------------------------------------
@needs_hipcc
def test_frames_kernels_have_no_scratch_and_no_spills():
    k = resource_usage("frames.hip", containing("frames_"))
    for name in KERNELS:
        assert sum(name in n for n in k) == (2 if name == "frames_splat" else 1), (name, sorted(k))      # with and without the window
    assert len(k) == len(KERNELS) + 1
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)
        assert r.get("Occupancy") >= 4, (name, r)


# ---- 3. the marshalling and the command line -------------------------------------------------------------------------------------
def test_desc_marshalling(capi):
    rot = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    d = capi.frames_desc((8, 6), ((-1.0, -2.0), (3.0, 4.0)), capacity=7, dt_frame=0.5, rot=rot, centre=(1.0, 2.0, 3.0), centre_sink=2,
                         fields=("u", "vx", "rho"), h=0.25, clip=((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)))
    assert list(d.rot) == rot.reshape(9).tolist() and list(d.centre) == [1.0, 2.0, 3.0]
    assert (list(d.lo), list(d.hi)) == ([-1.0, -2.0], [3.0, 4.0]) and (list(d.clip_lo), list(d.clip_hi)) == ([-1.0, -2.0, -3.0], [1.0, 2.0, 3.0])
    assert (d.h, d.dt_frame, d.capacity, d.n_u, d.n_v, d.every, d.centre_sink, d.nq, d.reserved) == (0.25, 0.5, 7, 8, 6, 0, 2, 3, 0)
    assert list(d.fields) == [capi.FIELDS.index(f) for f in ("u", "vx", "rho")]
    d = capi.frames_desc(5, ((0.0, 0.0), (1.0, 1.0)), capacity=3, every=4, fields="u")
    assert (d.n_u, d.n_v, d.every, d.dt_frame, d.centre_sink, d.nq, d.h) == (5, 5, 4, 0.0, -1, 1, 0.0)
    assert list(d.rot) == np.eye(3).reshape(9).tolist() and list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3
    d = capi.frames_desc(5, ((0.0, 0.0), (1.0, 1.0)), every=4, dt_frame=0.5)          # both: passed on for the library to refuse
    assert (d.every, d.dt_frame) == (4, 0.5)
    with pytest.raises(ValueError):
        capi.frames_desc((1, 2, 3), ((0.0, 0.0), (1.0, 1.0)))
    with pytest.raises(ValueError):
        capi.frames_desc(4, ((0.0, 0.0), (1.0, 1.0)), fields=("u", "u", "u", "u"))
    head = np.zeros((2, 16))
    head[:, 0], head[:, 1], head[:, 2], head[:, 3], head[:, 4:7], head[:, 7:11], head[:, 11] = [3, 6], [0.5, 1.0], 9, 8, [1, 2, 3], np.nan, [0, 1]
    c = capi.frames_columns(head, np.zeros((2, 1, 2, 2)), dropped=4)
    assert c["step"].tolist() == [3, 6] and c["t"].tolist() == [0.5, 1.0] and c["n"].tolist() == [9, 9] and c["n_sel"].tolist() == [8, 8]
    assert c["centre"].tolist() == [[1, 2, 3]] * 2 and c["status"].tolist() == [0, 1] and c["dropped"] == 4 and c["exp"].shape == (2, 4)
    with pytest.raises(ValueError):
        capi.frames_columns(np.zeros((2, 15)), None)


def test_null_context_is_refused(capi):
    lib = capi.load()
    d = capi.frames_desc(4, ((0.0, 0.0), (1.0, 1.0)))
    assert lib.sph_frames_begin(None, d) == 1 and lib.sph_frames_end(None) == 1 and lib.sph_frames_record(None) == 1
    assert lib.sph_frames_rewind(None) == 1 and lib.sph_frames_info(None, None, None, None) == 1
    assert lib.sph_frames_read(None, 0, 0, None, None) == 1 and lib.sph_frame(None, d, None, None, 16) == 1


def test_cli_parses_its_arguments():
    from summersph_amd import frames
    ap = frames.build_parser()
    a = ap.parse_args(["save275.txt", "--steps", "500", "--dt-frame", "0.5", "--size", "256", "--extent", "200", "--inc", "40", "--pa", "30",
                       "--fields", "u", "--follow-sink", "0", "-o", "movie.npz", "--png-dir", "frames/", "--json"])
    kw = frames.args_desc(a)
    assert kw["shape"] == (256, 256) and kw["bounds"] == ((-100.0, -100.0), (100.0, 100.0)) and kw["capacity"] == 501
    assert kw["dt_frame"] == 0.5 and kw["every"] == 1 and kw["centre_sink"] == 0 and kw["fields"] == ("u",) and kw["h"] is None
    from summersph_amd import cube
    assert np.array_equal(kw["rot"], cube.view(40.0, 30.0)) and kw["centre"] == (0.0, 0.0, 0.0) and kw["clip"] is None
    kw = frames.args_desc(ap.parse_args(["s.txt", "--steps", "10", "--every", "3", "--extent", "2", "--clip=-1,-2,-3,1,2,3",
                                         "--centre", "1,2,3", "--h", "0.5", "--capacity", "2", "--fields", "u,vx,rho"]))
    assert (kw["every"], kw["dt_frame"], kw["capacity"], kw["h"]) == (3, None, 2, 0.5) and kw["fields"] == ("u", "vx", "rho")
    assert kw["clip"] == ((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)) and kw["centre"] == (1.0, 2.0, 3.0)
    base = ["s.txt", "--steps", "10", "--extent", "2"]
    for bad in (base, base + ["--dt-frame", "1", "--every", "2"], base + ["--dt-frame", "0"], base + ["--dt-frame", "nan"],
                base + ["--every", "0"], base + ["--every", "1", "--size", "0"], ["s.txt", "--steps", "-1", "--extent", "2", "--every", "1"],
                ["s.txt", "--steps", "1", "--extent", "0", "--every", "1"], base + ["--every", "1", "--h", "-1"],
                base + ["--every", "1", "--follow-sink", "64"], base + ["--every", "1", "--capacity", "0"],
                base + ["--every", "1", "--dt", "0"], base + ["--every", "1", "--fields", "u,vx,rho,vy"],
                base + ["--every", "1", "--fields", "nope"], base + ["--every", "1", "--fields", "h"]):
        with pytest.raises(ValueError):
            frames.args_desc(ap.parse_args(bad))
    with pytest.raises(SystemExit) as e:
        frames.main(base)                                           # no cadence: argparse's error exit
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        frames.main(["--steps", "3"])


def test_mean_of_planes():
    from summersph_amd import frames
    p = np.array([[[2.0, 0.0], [4.0, 1.0]], [[3.0, 0.0], [-2.0, 0.5]], [[0.0, 5.0], [8.0, 0.0]]])
    m = frames.mean(p)
    assert m.shape == (2, 2, 2) and np.isnan(m[0, 0, 1]) and np.isnan(m[1, 0, 1])
    assert m[0].tolist()[1] == [-0.5, 0.5] and m[0, 0, 0] == 1.5 and m[1, 1].tolist() == [2.0, 0.0]
    assert frames.mean(np.stack([p, p])).shape == (2, 2, 2, 2)
    with pytest.raises(ValueError):
        frames.mean(np.zeros((2, 2)))


# ---- 4. the restatement ----------------------------------------------------------------------------------------------------------
def test_footprint_of_the_restatement():
    F = frames_ref.spline_column
    assert float(F(0.0)) == 1.5 and float(F(2.0)) == 0.0 and float(F(2.5)) == 0.0
    p = np.linspace(0.0, 2.0, 20001)
    f = F(p).astype(np.float64)
    assert np.all(f >= -1e-18) and np.all(np.diff(f) <= 1e-15)     # non-negative, falling
    assert abs(np.trapezoid(f * 2.0 * p, p) - 1.0) <= 1e-8          # a footprint integrates to the particle's m A
    # against direct quadrature of the cubic spline W h^3 pi along the line of sight
    def w(q):
        return np.where(q < 1, 1 - 1.5 * q ** 2 + 0.75 * q ** 3, np.where(q < 2, 0.25 * (2 - q) ** 3, 0.0))
    for b in (0.0, 0.3, 1.0, 1.7):
        z = np.linspace(0.0, 2.0, 400001)
        assert abs(2.0 * np.trapezoid(w(np.sqrt(b * b + z * z)), z) - float(F(b))) <= 1e-9, b


def test_node_sums_of_the_restatement():
    pos = np.array([[0.0, 0.0, 5.0], [1.0, 0.0, -2.0], [10.0, 10.0, 0.0]])
    m, h = np.array([2.0, 3.0, 1.0]), np.array([1.0, 0.5, 1.0])
    A = np.array([1.0, -2.0, 7.0])
    sums, mags, n_sel = frames_ref.frame(pos, m, h, [A], (3, 1), ((0.0, 0.0), (2.0, 0.0)))
    y0 = m / (np.pi * h * h)
    F = frames_ref.spline_column
    want0 = [y0[0] * 1.5 + y0[1] * 0.0, y0[0] * float(F(1.0)) + y0[1] * 1.5, 0.0]
    assert n_sel == 3 and np.allclose(sums[0, :, 0].astype(float), want0, rtol=1e-15, atol=0)
    assert np.allclose(sums[1, :, 0].astype(float), [y0[0] * 1.5, y0[0] * float(F(1.0)) - 2 * y0[1] * 1.5, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(mags[1, :, 0].astype(float), [y0[0] * 1.5, y0[0] * float(F(1.0)) + 2 * y0[1] * 1.5, 0.0], rtol=1e-15, atol=0)
    # the clip is strict and in simulation axes, whatever the view
    rot = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    _, _, n = frames_ref.frame(pos, m, h, [], (2, 2), ((0.0, 0.0), (1.0, 1.0)), rot=rot, clip=((0.0, -1.0, -3.0), (11.0, 11.0, 6.0)))
    assert n == 2                                                   # x = 0 sits on the clip's face: out
    assert frames_ref.exponent(np.array([0.0])) == 0 and frames_ref.exponent(np.array([0.5, -1.0])) == 1 and frames_ref.exponent(np.array([2.0 / 3.0])) == 1


def test_cadence_rule_on_hand_cases():
    c = frames_ref.cadence
    assert c([0.1, 0.2, 0.3, 0.4], 0.0, 0.5) == []
    assert c([0.25, 0.5, 0.75, 1.0], 0.0, 0.5) == [2, 4]            # a t that equals a threshold records
    assert c([0.4, 1.7, 1.9, 2.0, 2.4, 2.5], 0.0, 0.5) == [2, 4, 6]  # step 2 skips the thresholds 1.0 and 1.5: one frame, then k = 4
    assert c([10.4, 10.5, 10.6, 11.0], 10.0, 0.5) == [2, 4]         # t0 is the t at begin
    assert c([1.0, 2.0, 3.0], 0.0, 1e-6) == [1, 2, 3]               # at most one frame per step
    # product, then sum, in double: 3 * 0.1 is above 0.3, so a t of exactly 0.3 does not reach the third threshold
    assert 3 * 0.1 > 0.3 and c([0.1, 0.2, 0.3, 0.4], 0.0, 0.1) == [1, 2, 4]
