"""CPU tests of the spectral cubes (sph_cube): the ABI mirrors (ctypes, Fortran) against the C header, the resource use of
cube.hip's kernels, the closed form of the line-integrated spline against quadrature and its normalisation, the numpy
restatement against a brute-force sum, the viewing matrices, the moments, the position-velocity cut, the FITS writer and
the command line's parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import CSRC, c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import cube_ref
from summersph_amd import cube as cb

FIELDS = ["rot", "centre", "v_ref", "lo", "hi", "clip_lo", "clip_hi", "h", "v0", "dv", "sigma_scale", "sigma_floor", "n_u", "n_v",
          "n_chan", "flags", "reserved"]


def test_cube_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_cube_desc", FIELDS,
                   ['printf("consts %d\\n", SPH_CUBE_PER_VELOCITY);', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == ctypes.sizeof(capi.CubeDesc) == 264
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.CubeDesc, f).offset, f
    assert got["consts"] == f"{capi.CUBE_PER_VELOCITY}" == "1"
    assert got["abi"] == "1"                                        # the change is additive
    assert "sph_cube" in capi.SYMBOLS and "sph_cube_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_CUBE_PER_VELOCITY = 1", binding)
    # the channel chunk the tests size their two-chunk case by is the kernel's
    src = open(os.path.join(CSRC, "cube.hip")).read()
    assert int(re.search(r"#define CUBE_CHUNK (\d+)", src).group(1)) == capi.CUBE_CHUNK
    d = capi.cube_desc((5, 7), ((-1, -2), (3, 4)), 0.5, 0.25, 9, rot=cb.view(40, 30), centre=(1, 2, 3), v_ref=(4, 5, 6),
                       sigma_scale=0.3, sigma_floor=0.1, h=1.5, clip=((0, 1, 2), (3, 4, 5)), per_velocity=True)
    assert (d.n_u, d.n_v, d.n_chan, d.flags, d.reserved) == (5, 7, 9, 1, 0)
    assert (d.v0, d.dv, d.sigma_scale, d.sigma_floor, d.h) == (0.5, 0.25, 0.3, 0.1, 1.5)
    assert list(d.lo) == [-1, -2] and list(d.hi) == [3, 4] and list(d.centre) == [1, 2, 3] and list(d.v_ref) == [4, 5, 6]
    assert list(d.clip_lo) == [0, 1, 2] and list(d.clip_hi) == [3, 4, 5]
    assert np.array_equal(np.array(d.rot[:]).reshape(3, 3), cb.view(40, 30))
    d = capi.cube_desc(4, ((0, 0), (1, 1)), 0.0, 1.0, 1)
    assert (d.n_u, d.n_v, d.flags, d.h) == (4, 4, 0, 0.0) and list(d.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3
    with pytest.raises(ValueError):
        capi.cube_desc((1, 2, 3), ((0, 0), (1, 1)), 0.0, 1.0, 1)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "cube_caller", """program cube_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_cube_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: out(:, :, :), vals(:)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%rot = [1.0_c_double, 0.0_c_double, 0.0_c_double, 0.0_c_double, 1.0_c_double, 0.0_c_double, 0.0_c_double, 0.0_c_double, &
           1.0_c_double]
  d%centre = 0.0_c_double
  d%v_ref = 0.0_c_double
  d%lo = [-10.0_c_double, -10.0_c_double]
  d%hi = [10.0_c_double, 10.0_c_double]
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%h = 0.0_c_double
  d%v0 = -1.0_c_double
  d%dv = 0.25_c_double
  d%sigma_scale = 0.3_c_double
  d%sigma_floor = 0.0_c_double
  d%n_u = 8
  d%n_v = 6
  d%n_chan = 9
  d%flags = SPH_CUBE_PER_VELOCITY
  d%reserved = 0
  if (c_sizeof(d) /= 264) stop 1
  allocate(out(6, 8, 9), vals(10))
  st = sph_cube(ctx, d, c_loc(vals), c_loc(out), 432_c_int64_t)
  st = sph_cube_dev(ctx, d, c_null_ptr, c_null_ptr, 0_c_int64_t)
  print *, st
end program cube_caller
""")


@needs_hipcc
def test_cube_kernels_fit_the_register_budget():
    k = resource_usage("cube.hip", containing("cube_", "stats_final", "start_table"))
    for name in ("cube_stats_partial", "stats_final", "cube_select", "start_table", "cube_records", "cube_gather"):
        assert sum(name in n for n in k) == 1, name
    assert len(k) == 6, sorted(k)
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        # the front end at full occupancy; the gather is bound by its LDS (six wavefronts a CU), not by its registers
        assert 0 < r.get("VGPRs", 999) <= (168 if "cube_gather" in name else 64), (name, r)
    lds = [r for n, r in k.items() if "cube_gather" in n][0]["LDS Size"]
    from summersph_amd import capi
    assert capi.CUBE_CHUNK * 64 * 8 <= lds <= 160 * 1024 // 6, lds        # the spectrum slots + the staged records


SPECIAL = np.array([0.0, 1e-12, 1.0 - 1e-6, 1.0, 1.0 + 1e-6, 2.0 - 1e-6, 2.0])


def test_closed_form_matches_quadrature():
    p = np.concatenate([SPECIAL, np.random.default_rng(1).uniform(0.0, 2.0, 2000), [2.0 + 1e-9, 3.0]])
    f, q = cube_ref.column_kernel(p), cube_ref.column_kernel_quad(p, 64)
    err = float(np.max(np.abs(f - q)))
    print(f"    closed form against 64-node quadrature: {err:.2e}")
    assert err <= 1e-13
    assert cube_ref.column_kernel(np.array(0.0)) == 1.5
    assert np.all(f[-2:] == 0.0) and cube_ref.column_kernel(np.array(2.0)) == 0.0
    assert np.all(np.diff(cube_ref.column_kernel(np.linspace(0.0, 2.0, 4001))) <= 1e-15)      # monotone


def test_column_kernel_normalisation():
    # integral of F 2 p dp over [0, 2] = 1: Gauss-Legendre on [0, 1] and [1, 2], where F's form changes
    x, w = np.polynomial.legendre.leggauss(64)
    tot = 0.0
    for a, b in ((0.0, 1.0), (1.0, 2.0)):
        p = 0.5 * (b - a) * x + 0.5 * (b + a)
        tot += 0.5 * (b - a) * np.sum(w * cube_ref.column_kernel(p) * 2.0 * p)
    assert abs(tot - 1.0) <= 5e-14, tot
    # and of a particle's footprint on a fine image: sum of the cube over nodes and channels times the pixel area = m A
    pos, vel = np.array([[0.3, -0.2, 5.0]]), np.array([[0.0, 0.0, 0.4]])
    c = cube_ref.cube(pos, vel, np.array([2.0]), 1.0, (161, 161), ((-2.2, -2.2), (2.2, 2.2)), 0.0, 0.1, 21, sigma_floor=0.05,
                      values=np.array([3.0]))
    assert abs(c.sum() * (4.4 / 160) ** 2 - 6.0) <= 2e-3 * 6.0
    assert np.argmax(c.sum(axis=(1, 2))) == 4                        # V = 0.4: channel k is centred on v0 + k dv


def test_restatement_matches_brute_force():
    rng = np.random.default_rng(5)
    n = 400
    pos, vel = rng.uniform(-6, 6, (n, 3)), rng.normal(0, 0.5, (n, 3))
    m, h, c = rng.uniform(0.5, 1.5, n), 2.0 ** rng.uniform(-2, 1, n), rng.uniform(0.2, 1.0, n)
    rot = cb.view(40.0, 30.0, 10.0)
    kw = dict(shape=(12, 9), bounds=((-5.0, -4.0), (4.0, 5.0)), v0=-1.0, dv=0.2, n_chan=11, rot=rot, sigma_scale=0.5, sigma_floor=0.05)
    got = cube_ref.cube(pos, vel, m, h, c=c, **kw)
    gu, gv = np.linspace(-5, 4, 12), np.linspace(-4, 5, 9)
    pix = np.array([(i, j) for i in range(12) for j in range(9)])
    for k in (0, 5, 10):
        want = cube_ref.voxels(pos, vel, m, h, gu, gv, pix, -1.0, 0.2, 11, [k] * len(pix), rot, c=c, sigma_scale=0.5, sigma_floor=0.05)
        assert np.max(np.abs(got[k].reshape(-1) - want)) <= 1e-13 * np.max(np.abs(got))
    # selection: ghosts and the strict clip box; per velocity; sigma 0 puts a particle into one channel
    half = cube_ref.cube(pos, vel, m, h, c=c, n_owned=150, **kw) + cube_ref.cube(pos[150:], vel[150:], m[150:], h[150:], c=c[150:], **kw)
    assert np.max(np.abs(half - got)) <= 1e-13 * np.max(np.abs(got))
    clip = ((-3.0, -np.inf, -2.0), (3.0, 2.0, np.inf))
    sel = cube_ref.selection(pos, None, clip)
    assert 0 < sel.sum() < n
    a = cube_ref.cube(pos, vel, m, h, c=c, clip=clip, **kw)
    b = cube_ref.cube(pos[sel], vel[sel], m[sel], h[sel], c=c[sel], **kw)
    assert np.array_equal(a, b)
    assert np.array_equal(cube_ref.cube(pos, vel, m, h, c=c, per_velocity=True, **kw), got / 0.2)
    e = cube_ref.edges(-1.0, 0.2, 11)
    assert e[0] == -1.1 and np.allclose(np.diff(e), 0.2)
    w = np.diff(cube_ref.cdf(e, e[4], 0.0))
    assert list(np.flatnonzero(w)) == [4] and w[4] == 1.0              # e_k <= V < e_{k+1}
    assert not np.diff(cube_ref.cdf(e, e[11], 0.0)).any()
    w = np.diff(cube_ref.cdf(e, 0.0, 0.01))
    assert abs(w.sum() - 1.0) <= 1e-15 and np.count_nonzero(w) == 1    # the truncation: exact zeros beyond 8.5 sigma


def test_view_matrices():
    for inc, pa, az in ((0, 0, 0), (40, 30, 0), (90, 0, 0), (90, 123, 45), (140, -30, 270), (12.5, 359, 1)):
        r = cb.view(inc, pa, az)
        assert np.max(np.abs(r @ r.T - np.eye(3))) <= 1e-15 and abs(np.linalg.det(r) - 1.0) <= 1e-15, (inc, pa, az)
        assert abs(r[2, 2] - np.cos(np.deg2rad(inc))) <= 1e-15           # the inclination is the angle between w^ and z^
    assert np.array_equal(cb.view(0, 0), np.eye(3))
    for pa in (0, 30, 200):
        assert np.allclose(cb.view(0, pa)[2], [0, 0, 1], atol=1e-16)     # face-on: w^ = z^
    for pa, az in ((0, 0), (30, 60)):
        r = cb.view(90, pa, az)
        assert abs(r[2, 2]) <= 1e-16                                     # edge-on: z^ lies in the image plane
        assert abs(np.hypot(r[0, 2], r[1, 2]) - 1.0) <= 1e-15
    # the line of nodes (the disc's own axis after the azimuth turn) lies at the position angle from the u axis
    r = cb.view(40, 30, 0)
    assert np.allclose(r @ np.array([1.0, 0, 0]), [np.cos(np.deg2rad(30)), np.sin(np.deg2rad(30)), 0], atol=1e-15)
    # w^ = (0, -sin i, cos i) at pa = az = 0 points away from the observer: of a disc that turns anticlockwise about +z, the
    # side at +u (velocity along +y) has V < 0 -- it approaches -- and the side at -u recedes
    r = cb.view(40, 0)
    assert np.allclose(r[2], [0.0, -np.sin(np.deg2rad(40)), np.cos(np.deg2rad(40))], atol=1e-16)
    assert (r @ np.array([10.0, 0, 0]))[0] > 0 and (r @ np.array([0, 1.0, 0]))[2] < 0


def test_moments_of_a_gaussian_cube():
    v = cb.channels(-5.0, 0.05, 201)
    assert v[0] == -5.0 and abs(v[-1] - 5.0) < 1e-12 and v.size == 201
    mu = np.array([[-1.0, 0.0], [0.5, 2.0]])
    sg = np.array([[0.3, 0.5], [0.2, 0.4]])
    amp = np.array([[1.0, 2.0], [0.0, 3.0]])
    cube = amp * np.exp(-0.5 * ((v[:, None, None] - mu) / sg) ** 2) / (np.sqrt(2 * np.pi) * sg) * 0.05
    m0, m1, m2, peak = cb.moments(cube, v)
    ok = amp > 0
    assert np.allclose(m0[ok], amp[ok], rtol=1e-10)
    assert np.allclose(m1[ok], mu[ok], atol=1e-9) and np.allclose(m2[ok], sg[ok], rtol=1e-8)
    assert np.allclose(peak[ok], mu[ok], atol=0.025 + 1e-12)
    assert m0[1, 0] == 0.0 and np.isnan(m1[1, 0]) and np.isnan(m2[1, 0]) and np.isnan(peak[1, 0])
    with pytest.raises(ValueError):
        cb.moments(cube, v[:-1])
    assert cb.vrange_channels(-5.0, 5.0, 64) == (-5.0 + 10.0 / 128, 10.0 / 64)
    for bad in ((1.0, 1.0, 4), (0.0, 1.0, 0)):
        with pytest.raises(ValueError):
            cb.vrange_channels(*bad)


def test_pv_cut_interpolates_between_nodes():
    gu, gv = np.linspace(-4, 4, 9), np.linspace(-3, 3, 7)
    v = cb.channels(0.0, 1.0, 3)
    cube = v[:, None, None] + 2.0 * gu[None, :, None] - 0.5 * gv[None, None, :]        # linear: bilinear is exact
    pv, off = cb.pv_cut(cube, ((-4, -3), (4, 3)), (-3.3, -1.2), (2.9, 2.2), 11)
    assert pv.shape == (3, 11) and off[0] == 0.0 and np.isclose(off[-1], np.hypot(6.2, 3.4))
    s = np.linspace(0, 1, 11)
    want = v[:, None] + 2.0 * (-3.3 + 6.2 * s) - 0.5 * (-1.2 + 3.4 * s)
    assert np.allclose(pv, want, atol=1e-13)
    pv, _ = cb.pv_cut(cube, ((-4, -3), (4, 3)), (-6.0, 0.0), (4.0, 0.0), 6)
    assert np.isnan(pv[:, 0]).all() and np.isfinite(pv[:, 1:]).all()


def test_fits_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    cube = rng.normal(size=(5, 4, 3)) * 10.0 ** rng.uniform(-300, 300, (5, 4, 3))
    cube[0, 0, 0], cube[1, 1, 1] = -0.0, np.pi
    path = tmp_path / "c.fits"
    cb.write_fits(str(path), cube, ((-1.5, 2.0), (3.0, 4.0)), -0.3, 0.1, bunit="g/cm2", extra=[("INCL", 40.0, "inclination [deg]")])
    raw = path.read_bytes()
    assert len(raw) % 2880 == 0 and len(raw) == 2880 + 2880                 # one header block, 480 bytes of data padded
    head = raw[:2880].decode("ascii")
    cards = [head[k:k + 80] for k in range(0, 2880, 80)]
    assert cards[0].startswith("SIMPLE  =                    T") and cards[1].startswith("BITPIX  =                  -64")
    assert cards[2].startswith("NAXIS   =                    3")
    assert [c[:8].strip() for c in cards[:6]] == ["SIMPLE", "BITPIX", "NAXIS", "NAXIS1", "NAXIS2", "NAXIS3"]
    assert any(c.startswith("END") and c.strip() == "END" for c in cards)
    # big-endian doubles, byte for byte
    assert raw[2880:2880 + 480] == cube.astype(">f8").tobytes() and raw[2880 + 480:] == b"\0" * (2880 - 480)
    hdr, data = cb.read_fits(str(path))
    assert data.tobytes() == cube.tobytes() and data.shape == (5, 4, 3)
    assert (hdr["NAXIS1"], hdr["NAXIS2"], hdr["NAXIS3"], hdr["BITPIX"], hdr["SIMPLE"]) == (3, 4, 5, -64, True)
    assert (hdr["CRPIX1"], hdr["CRVAL1"], hdr["CDELT1"]) == (1.0, 2.0, 1.0)       # the v axis: 3 nodes on [2, 4]
    assert (hdr["CRPIX2"], hdr["CRVAL2"], hdr["CDELT2"]) == (1.0, -1.5, 1.5)      # the u axis: 4 nodes on [-1.5, 3]
    assert (hdr["CRPIX3"], hdr["CRVAL3"], hdr["CDELT3"]) == (1.0, -0.3, 0.1)
    assert hdr["CTYPE3"] == "VELO" and hdr["BUNIT"] == "g/cm2" and hdr["INCL"] == 40.0
    with pytest.raises(ValueError):
        cb.write_fits(str(path), cube[0], ((0, 0), (1, 1)), 0.0, 1.0)


def test_cli_parsing():
    ap = cb.build_parser()
    a = ap.parse_args(["save275.txt", "-o", "cube.npz", "--inc", "40", "--pa", "30", "--extent", "200", "--size", "256", "--vrange",
                       "-5", "5", "--nchan", "64", "--sigma-scale", "0.3", "--fits", "cube.fits", "--json"])
    kw = cb.args_desc(a)
    assert kw["shape"] == (256, 256) and kw["bounds"] == ((-100.0, -100.0), (100.0, 100.0)) and kw["n_chan"] == 64
    assert (kw["v0"], kw["dv"]) == cb.vrange_channels(-5.0, 5.0, 64) and np.array_equal(kw["rot"], cb.view(40.0, 30.0))
    assert kw["sigma_scale"] == 0.3 and kw["sigma_floor"] == 0.0 and kw["h"] is None and kw["clip"] is None
    assert a.fits == "cube.fits" and a.json and not a.variable and not kw["per_velocity"]
    a = ap.parse_args(["s", "-o", "o", "--extent", "50", "--vrange", "0", "2", "--azimuth", "15", "--centre", "1,2,3", "--vref",
                       "0.1,0,0", "--h", "2", "--clip", "0,1,2,3,4,5", "--per-velocity", "--sigma-floor", "0.2", "--variable"])
    kw = cb.args_desc(a)
    assert kw["centre"] == (1.0, 2.0, 3.0) and kw["v_ref"] == (0.1, 0.0, 0.0) and kw["h"] == 2.0 and kw["per_velocity"]
    assert kw["clip"] == ((0.0, 1.0, 2.0), (3.0, 4.0, 5.0)) and np.array_equal(kw["rot"], cb.view(0, 0, 15)) and a.variable
    for extra in (["--size", "0"], ["--nchan", "0"], ["--h", "-1"], ["--sigma-scale", "-0.1"], ["--centre", "1,2"], ["--clip", "1,2,3"]):
        with pytest.raises(ValueError):
            cb.args_desc(ap.parse_args(["s", "-o", "o", "--extent", "50", "--vrange", "0", "2"] + extra))
    with pytest.raises(ValueError):
        cb.args_desc(ap.parse_args(["s", "-o", "o", "--extent", "50", "--vrange", "2", "0"]))
    for argv in (["s", "-o", "o", "--vrange", "0", "1"], ["s", "-o", "o", "--extent", "5"], ["s", "--extent", "5", "--vrange", "0", "1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
