"""CPU tests of the field-line tracer (sph_trace): the ABI mirrors (ctypes, Fortran) against the C header, the register budget
of the trace kernels, the numpy restatement against a brute-force O(N M) form, its stops, stride, upstream steps and carry,
the seed helpers' geometry, the command line's parsing, and the condition under which the GPU parity test may compare the
status of every seed: no stage evaluation of its seed sets has a den that rounding could turn into 0."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT, load_golden
import trace_ref
from summersph_amd import ic
from summersph_amd import trace as trc

FIELDS = ["clip_lo", "clip_hi", "h", "box_lo", "box_hi", "ds", "omega", "centre", "normal", "fields", "carry", "weight", "n_steps",
          "stride", "flags", "reserved"]


def test_trace_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_trace_desc", FIELDS,
                   ['printf("consts %d %d %d %d\\n", SPH_TRACE_ARCLENGTH, SPH_TRACE_PLANAR, SPH_TRACE_VALUES, SPH_TRACE_NONE);',
                    'printf("codes %d %d %d %d %d\\n", SPH_TRACE_DONE, SPH_TRACE_LEFT_GAS, SPH_TRACE_LEFT_BOX, SPH_TRACE_STAGNANT,\n'
                    '         SPH_TRACE_NONFINITE);', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == ctypes.sizeof(capi.TraceDesc) == 224
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.TraceDesc, f).offset, f
    assert got["consts"] == f"{capi.TRACE_ARCLENGTH} {capi.TRACE_PLANAR} {capi.TRACE_VALUES} {capi.TRACE_NONE}" == "1 2 -1 -2"
    assert got["codes"] == (f"{capi.TRACE_DONE} {capi.TRACE_LEFT_GAS} {capi.TRACE_LEFT_BOX} {capi.TRACE_STAGNANT} "
                            f"{capi.TRACE_NONFINITE}") == "0 1 2 3 4"
    assert (trace_ref.DONE, trace_ref.LEFT_GAS, trace_ref.LEFT_BOX, trace_ref.STAGNANT, trace_ref.NONFINITE) == (0, 1, 2, 3, 4)
    assert got["abi"] == "1"                                        # the change is additive
    assert "sph_trace" in capi.SYMBOLS and "sph_trace_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_TRACE_ARCLENGTH = 1, SPH_TRACE_PLANAR = 2, SPH_TRACE_VALUES = -1, SPH_TRACE_NONE = -2", binding)
    d = capi.trace_desc(12, -0.25, fields=("vx", capi.TRACE_VALUES, "vz"), carry="rho", arclength=True, omega=(0, 0, 0.5),
                        centre=(1, 2, 3), normal=(0, 0, 2), box=((0, 1, 2), (3, 4, 5)), stride=4, weight="volume", h=1.5,
                        clip=((-1, -2, -3), (7, 8, 9)))
    assert (d.n_steps, d.stride, d.ds, d.weight, d.flags, d.h) == (12, 4, -0.25, 1, 3, 1.5)
    assert list(d.fields) == [capi.FIELDS.index("vx"), -1, capi.FIELDS.index("vz")] and d.carry == capi.FIELDS.index("rho")
    assert list(d.omega) == [0, 0, 0.5] and list(d.centre) == [1, 2, 3] and list(d.normal) == [0, 0, 2]
    assert list(d.box_lo) == [0, 1, 2] and list(d.box_hi) == [3, 4, 5] and list(d.clip_lo) == [-1, -2, -3]
    assert list(d.reserved) == [0, 0]
    d = capi.trace_desc(3, 1.0)
    assert (d.flags, d.carry, d.stride, d.h, d.weight) == (0, capi.TRACE_NONE, 1, 0.0, 0)
    assert list(d.fields) == [capi.FIELDS.index(f) for f in ("vx", "vy", "vz")]
    assert list(d.box_lo) == [-np.inf] * 3 and list(d.box_hi) == [np.inf] * 3 and list(d.omega) == [0.0] * 3
    with pytest.raises(ValueError):
        capi.trace_desc(3, 1.0, fields=("vx", "vy"))
    with pytest.raises(KeyError):
        capi.trace_desc(3, 1.0, weight="number")


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "trace_caller", """program trace_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_trace_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: sx(:), sy(:), sz(:), path(:, :, :), carry(:, :)
  integer(c_int32_t), allocatable, target :: status(:), n_done(:)
  integer(c_int64_t), target :: counts(5)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%box_lo = d%clip_lo
  d%box_hi = d%clip_hi
  d%h = 0.0_c_double
  d%ds = 0.5_c_double
  d%omega = [0.0_c_double, 0.0_c_double, 0.01_c_double]
  d%centre = 0.0_c_double
  d%normal = [0.0_c_double, 0.0_c_double, 1.0_c_double]
  d%fields = [SPH_F_VX, SPH_F_VY, SPH_TRACE_VALUES]
  d%carry = SPH_F_RHO
  d%weight = SPH_RENDER_WEIGHT_MASS
  d%n_steps = 8
  d%stride = 2
  d%flags = ior(SPH_TRACE_ARCLENGTH, SPH_TRACE_PLANAR)
  d%reserved = 0
  if (c_sizeof(d) /= 224) stop 1
  if (SPH_TRACE_NONFINITE /= 4 .or. SPH_TRACE_NONE /= -2) stop 2
  allocate(sx(10), sy(10), sz(10), path(10, 3, 5), carry(10, 5), status(10), n_done(10))
  st = sph_trace(ctx, d, 10_c_int64_t, c_loc(sx), c_loc(sy), c_loc(sz), c_null_ptr, c_loc(path), 150_c_int64_t, c_loc(carry), &
                 c_loc(status), c_loc(n_done), c_loc(counts))
  st = sph_trace_dev(ctx, d, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t, &
                     c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
  print *, st, counts
end program trace_caller
""")


@needs_hipcc
def test_trace_kernels_fit_the_register_budget():
    k = resource_usage("trace.hip", containing("trace_"))
    assert sum("trace_seed_keys" in n for n in k) == 1
    walks = [n for n in k if "trace_walk" in n]
    assert len(walks) == 4, walks
    for per_h in (0, 1):
        for carry in (0, 1):
            assert sum(f"trace_walkILb{per_h}ELb{carry}E" in n for n in walks) == 1, (per_h, carry)
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def _particles(n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 6.0, (n, 3))
    m = rng.uniform(0.5, 1.5, n)
    h = rng.uniform(0.6, 1.2, n)
    # a smooth swirl about the box's axis plus noise, and a scalar to carry
    c = pos - 3.0
    A = np.stack([-c[:, 1] + 0.1 * rng.normal(size=n), c[:, 0] + 0.1 * rng.normal(size=n), 0.3 * np.sin(pos[:, 0]),
                  pos[:, 2] ** 2 + 1.0])
    rho = rng.uniform(0.5, 2.0, n)
    return pos, m, h, A, rho


@pytest.mark.parametrize("arclength", [False, True])
def test_restatement_matches_the_brute_force(arclength):
    pos, m, h, A, rho = _particles(300, 31)
    rng = np.random.default_rng(32)
    seeds = np.concatenate([rng.uniform(0.5, 5.5, (60, 3)), rng.uniform(-3.0, 9.0, (20, 3))])
    kw = dict(arclength=arclength, omega=(0.0, 0.1, 0.4), centre=(3.0, 3.0, 3.0), normal=(0.2, 0.0, 1.0), stride=2, carry=True)
    for hh, r, ds in ((h, None, 0.2), (0.9, rho, -0.2)):
        got = trace_ref.trace(seeds, pos, m, hh, A, 12, ds, rho=r, **kw)
        want = trace_ref.trace_with(trace_ref.brute_sampler(pos, m, hh, A, r), seeds, 12, ds, **kw)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(np.isnan(got[0]), np.isnan(want[0])) and np.array_equal(np.isnan(got[3]), np.isnan(want[3]))
        scale = np.nanmax(np.abs(want[0]))
        assert np.nanmax(np.abs(got[0] - want[0])) <= 1e-13 * scale
        assert np.nanmax(np.abs(got[3] - want[3])) <= 1e-13 * np.nanmax(np.abs(want[3]))
        assert np.count_nonzero(got[1] == trace_ref.DONE) >= 40 and np.count_nonzero(got[1] == trace_ref.LEFT_GAS) >= 5


def _slab(q):
    """a sampler: the constant field (1, 0.5, 0) with carry x where x < 5, no gas beyond"""
    den = (q[:, 0] < 5.0).astype(np.float64)
    w = np.stack([np.ones(len(q)), np.full(len(q), 0.5), np.zeros(len(q)), q[:, 0]]) * den
    return w, den


def test_restatement_stops_stride_upstream_and_carry():
    seeds = np.array([[0.0, 0.0, 0.0], [3.25, 0.0, 0.0], [6.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 9.0, 0.0], [0.0, 0.0, np.inf]])
    box = ((-10.0, -1.0, -1.0), (10.0, 1.75, 1.0))
    path, status, done, car = trace_ref.trace_with(_slab, seeds, 8, 0.5, box=box, carry=True)
    one = trace_ref.trace_with(_slab, seeds, 8, 0.5, box=box)
    assert np.array_equal(one[0], path, equal_nan=True) and np.array_equal(one[1], status) and np.array_equal(one[2], done)
    assert list(status) == [trace_ref.LEFT_BOX, trace_ref.LEFT_GAS, trace_ref.LEFT_GAS, trace_ref.NONFINITE, trace_ref.LEFT_BOX,
                            trace_ref.NONFINITE]
    # line 0 crosses y = 1.75 with its 7th vertex (y = 1.75 is not strictly inside): recorded, then NaN
    assert done[0] == 7 and np.array_equal(path[7, :, 0], [3.5, 1.75, 0.0]) and np.all(np.isnan(path[8, :, 0]))
    assert np.array_equal(car[:8, 0], 0.5 * np.arange(8)) and np.isnan(car[8, 0])
    # line 1: the k4 stage of its 4th step would sit at x = 5.25: the step is not taken, the line ends at its last vertex
    assert done[1] == 3 and np.array_equal(path[3, :, 1], [4.75, 0.75, 0.0]) and np.all(np.isnan(path[4:, :, 1]))
    assert car[3, 1] == 4.75 and np.all(np.isnan(car[4:, 1]))
    # line 2 starts outside the gas: row 0 is the seed, its carry is sph_sample's 0.0
    assert done[2] == 0 and np.array_equal(path[0, :, 2], seeds[2]) and car[0, 2] == 0.0 and np.all(np.isnan(path[1:, :, 2]))
    # a non-finite seed: all rows NaN, row 0 included; a seed outside the box: row 0 and its carry, n_done 0
    assert np.all(np.isnan(path[:, :, 3])) and np.all(np.isnan(car[:, 3])) and done[3] == 0 and np.all(np.isnan(path[:, :, 5]))
    assert done[4] == 0 and np.array_equal(path[0, :, 4], seeds[4]) and car[0, 4] == 0.0 and np.all(np.isnan(path[1:, :, 4]))
    # stride: rows 0, 4, 8 of the full record, bitwise
    p4, s4, d4, c4 = trace_ref.trace_with(_slab, seeds, 8, 0.5, box=box, carry=True, stride=4)
    assert np.array_equal(p4, path[::4], equal_nan=True) and np.array_equal(c4, car[::4], equal_nan=True)
    assert np.array_equal(s4, status) and np.array_equal(d4, done)
    # upstream: a constant field is retraced exactly; n_steps completed and DONE
    up = trace_ref.trace_with(_slab, seeds[:1], 4, -0.5)
    assert up[1][0] == trace_ref.DONE and up[2][0] == 4 and np.array_equal(up[0][:, :, 0], -0.5 * np.arange(5)[:, None] * [1.0, 0.5, 0.0])
    # arclength: unit speed along the same direction; a zero field is STAGNANT there and stays put in time mode
    arc = trace_ref.trace_with(_slab, seeds[:1], 4, 0.5, arclength=True)
    seg = np.linalg.norm(np.diff(arc[0][:, :, 0], axis=0), axis=1)
    assert np.allclose(seg, 0.5, rtol=1e-15) and arc[1][0] == trace_ref.DONE
    still = lambda q: (np.zeros((3, len(q))), np.ones(len(q)))      # noqa: E731
    z = trace_ref.trace_with(still, seeds[:1] + 1.5, 4, 0.5, arclength=True)
    assert z[1][0] == trace_ref.STAGNANT and z[2][0] == 0 and np.all(np.isnan(z[0][1:]))
    z = trace_ref.trace_with(still, seeds[:1] + 1.5, 4, 0.5)
    assert z[1][0] == trace_ref.DONE and np.all(z[0] == 1.5)
    # the frame and PLANAR: rigid rotation seen from the co-rotating frame is at rest
    spin = lambda q: (np.stack([-0.3 * q[:, 1], 0.3 * q[:, 0], np.full(len(q), 0.2)]), np.ones(len(q)))      # noqa: E731
    r = trace_ref.trace_with(spin, np.array([[2.0, 1.0, 0.5]]), 6, 0.5, omega=(0.0, 0.0, 0.3), normal=(0.0, 0.0, 3.0))
    assert r[1][0] == trace_ref.DONE and np.all(r[0] == np.array([2.0, 1.0, 0.5])[None, :, None])


def test_seed_helpers():
    normal, centre = (0.3, -0.4, 0.8), (1.0, -2.0, 0.5)
    s, shape = trc.ring_seeds(30.0, 64, centre, normal)
    assert shape == (64,) and s.shape == (64, 3)
    n = np.asarray(normal) / np.linalg.norm(normal)
    r = s - np.asarray(centre)
    assert np.allclose(r @ n, 0.0, atol=1e-13) and np.allclose(np.linalg.norm(r, axis=1), 30.0, rtol=1e-14)
    ang = np.arccos(np.clip((r[0] @ r[1]) / 900.0, -1, 1))
    assert np.isclose(ang, 2.0 * np.pi / 64)
    s, _ = trc.ring_seeds(2.0, 4)
    assert np.allclose(s, [[2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0]], atol=1e-15)
    for bad in ((0.0, 4), (1.0, 0), (np.inf, 3)):
        with pytest.raises(ValueError):
            trc.ring_seeds(*bad)
    s, shape = trc.line_seeds((0, 0, 0), (3, 6, -9), 4)
    assert shape == (4,) and np.array_equal(s, [[0, 0, 0], [1, 2, -3], [2, 4, -6], [3, 6, -9]])
    s, shape = trc.grid_seeds((1.0, 1.0, 0.0), (1, 0, 0), (0, 1, 0), (4.0, 2.0), (5, 3))
    assert shape == (5, 3) and s.shape == (15, 3) and np.allclose(s.mean(axis=0), [1.0, 1.0, 0.0])
    # a circular binary of separation a about its barycentre, inclined: Omega = sqrt(G M / a^3) along the orbit's normal
    a, m1, m2 = 4.0, 3.0, 1.0
    Om = np.sqrt((m1 + m2) / a ** 3)
    nrm = np.array([0.0, -np.sin(0.3), np.cos(0.3)])
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.cross(nrm, [1.0, 0.0, 0.0])
    x1, x2 = -a * m2 / (m1 + m2) * e1, a * m1 / (m1 + m2) * e1
    v1, v2 = -a * m2 / (m1 + m2) * Om * e2, a * m1 / (m1 + m2) * Om * e2
    sinks = np.zeros((2, 8))
    sinks[0, :3], sinks[0, 3:6], sinks[1, :3], sinks[1, 3:6] = x1 + 5.0, v1, x2 + 5.0, v2
    omega, c = trc.sink_frame(sinks, 1)
    assert np.allclose(omega, Om * nrm, rtol=1e-14, atol=1e-16) and np.allclose(c, x1 + 5.0)
    omega2, c2 = trc.sink_frame({k: sinks[:, i] for i, k in enumerate("x y z vx vy vz".split())}, 0, about=1)
    assert np.allclose(omega2, omega, rtol=1e-14, atol=1e-16) and np.allclose(c2, x2 + 5.0)
    for bad in ((1, 1), (2, 0), (0, -1)):
        with pytest.raises(ValueError):
            trc.sink_frame(sinks, *bad)


def test_cli_parsing(tmp_path):
    ap = trc.build_parser()
    argv = ["save275.txt", "-o", "lines.npz", "--ring", "30", "64", "--steps", "200", "--ds", "0.5", "--arclength", "--planar", "0",
            "0", "1", "--corotate-sink", "1", "--both", "--carry", "rho", "--json"]
    a = ap.parse_args(argv)
    seeds, shape = trc.seeds_from_args(a)
    assert shape == (64,) and np.array_equal(seeds, trc.ring_seeds(30.0, 64)[0])
    sinks = np.zeros((2, 8))
    sinks[1, :6] = [10.0, 0.0, 0.0, 0.0, 0.3, 0.0]
    kw = trc.trace_options(a, sinks)
    assert kw["fields"] == ["vx", "vy", "vz"] and kw["carry"] == "rho" and kw["arclength"] and kw["normal"] == (0.0, 0.0, 1.0)
    assert np.allclose(kw["omega"], (0.0, 0.0, 0.03)) and kw["centre"] == (0.0, 0.0, 0.0) and kw["stride"] == 1
    assert a.both and a.json and a.steps == 200 and a.ds == 0.5 and kw["box"] is None and kw["clip"] is None
    with pytest.raises(ValueError):
        trc.trace_options(a, None)
    a = ap.parse_args(["s", "-o", "o", "--line", "0,0,0", "10,0,0", "11", "--steps", "8", "--ds", "-1", "--stride", "4", "--omega", "0",
                       "0", "0.1", "--frame-centre", "1,2,3", "--box", "0,0,0,5,5,5", "--volume", "--h", "2.0", "--fields", "ax,ay,az"])
    assert np.array_equal(trc.seeds_from_args(a)[0][:, 0], np.arange(11.0))
    kw = trc.trace_options(a)
    assert kw["omega"] == (0.0, 0.0, 0.1) and kw["centre"] == (1.0, 2.0, 3.0) and kw["box"] == ((0.0, 0.0, 0.0), (5.0, 5.0, 5.0))
    assert kw["weight"] == "volume" and kw["h"] == 2.0 and kw["fields"] == ["ax", "ay", "az"] and "normal" not in kw
    a = ap.parse_args(["s", "-o", "o", "--grid", "0,0,0", "1,0,0", "0,1,0", "20", "10", "5", "3", "--steps", "4", "--ds", "1"])
    assert trc.seeds_from_args(a)[1] == (5, 3)
    my = np.arange(24.0).reshape(2, 4, 3)
    np.save(tmp_path / "p.npy", my)
    a = ap.parse_args(["s", "-o", "o", "--seeds", str(tmp_path / "p.npy"), "--steps", "4", "--ds", "1"])
    seeds, shape = trc.seeds_from_args(a)
    assert shape == (2, 4) and np.array_equal(seeds, my.reshape(-1, 3))
    base = ["s", "-o", "o", "--ring", "3", "4"]
    for extra in (["--steps", "0", "--ds", "1"], ["--steps", "8", "--ds", "0"], ["--steps", "8", "--ds", "1", "--stride", "3"],
                  ["--steps", "8", "--ds", "1", "--carry", "nope"], ["--steps", "8", "--ds", "1", "--fields", "vx,vy"],
                  ["--steps", "8", "--ds", "1", "--planar", "0", "0", "0"], ["--steps", "8", "--ds", "1", "--h", "-1"],
                  ["--steps", "8", "--ds", "1", "--carry", "h"]):
        with pytest.raises(ValueError):
            trc.trace_options(ap.parse_args(base + extra))
    assert trc.trace_options(ap.parse_args(base + ["--steps", "8", "--ds", "1", "--carry", "h", "--variable"]))["carry"] == "h"
    for argv in (["s", "-o", "o", "--steps", "8", "--ds", "1"], base + ["--ds", "1"],
                 base + ["--steps", "8", "--ds", "1", "--omega", "0", "0", "1", "--corotate-sink", "1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)


@pytest.mark.parametrize("case", trace_ref.PARITY_CASES, ids=lambda c: f"{c[0]}-h{c[1]}-{'arc' if c[2] else 'time'}")
def test_seed_set_is_decisive(case):
    """Every stage evaluation of every line of a parity case has den exactly 0 or above 1e-6 of the median den: no line's
    LEFT_GAS stop hangs on the last bits of a sum, so the GPU's status and n_done must agree for every seed."""
    name, h, arclength, ds, gen_seed = case
    gas, _ = ic.split_rows(load_golden(name)["ic"])
    dens = []
    seeds, (path, status, done) = trace_ref.parity_case(gas, h, arclength, ds, gen_seed, dens)
    den = np.concatenate(dens)
    med = np.median(den)
    nz = den[den != 0.0]
    print(f"    {name} h {h} arclength {arclength}: {den.size} evaluations, {den.size - nz.size} zeros, smallest other den "
          f"{nz.min() / med:.2e} of the median; status counts {np.bincount(status, minlength=5)}")
    assert med > 0.0 and nz.min() > 1e-6 * med
    # the set exercises what it is for: lines that finish and lines that start outside the gas
    assert np.count_nonzero(status == trace_ref.DONE) >= 200 and np.count_nonzero(status == trace_ref.LEFT_GAS) >= 8
    assert np.all(done[status == trace_ref.DONE] == trace_ref.PARITY_STEPS)
