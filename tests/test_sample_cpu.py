"""CPU tests of the point sampling (sph_sample): the ABI mirrors (ctypes, Fortran) against the C header, the register
budget of the sample kernels, the numpy restatement against the O(N M) form of the field render's restatement, its
selection, zeros and NaN rules, the point-set helpers' geometry, and the command line's parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import profile_ref
import render_field_ref
import sample_ref
from summersph_amd import sample as smp

FIELDS = ["clip_lo", "clip_hi", "h", "fields", "n_fields", "weight", "flags", "reserved"]


def test_sample_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_sample_desc", FIELDS,
                   ['printf("consts %d %d %d %d %d\\n", SPH_SAMPLE_NORMALISE, SPH_SAMPLE_MAX_FIELDS, SPH_SAMPLE_VALUES,\n'
                    '         SPH_RENDER_WEIGHT_MASS, SPH_RENDER_WEIGHT_VOLUME);', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == ctypes.sizeof(capi.SampleDesc) == 88
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.SampleDesc, f).offset, f
    assert got["consts"] == (f"{capi.SAMPLE_NORMALISE} {capi.SAMPLE_MAX_FIELDS} {capi.SAMPLE_VALUES} {capi.RENDER_WEIGHT_MASS} "
                             f"{capi.RENDER_WEIGHT_VOLUME}") == "1 4 -1 0 1"
    assert got["abi"] == "1"                                        # the change is additive
    assert "sph_sample" in capi.SYMBOLS and "sph_sample_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_SAMPLE_NORMALISE = 1, SPH_SAMPLE_MAX_FIELDS = 4, SPH_SAMPLE_VALUES = -1", binding)
    d = capi.sample_desc(("u", capi.SAMPLE_VALUES), weight="volume", normalise=True, h=1.5, clip=((0, 1, 2), (3, 4, 5)))
    assert (d.n_fields, d.weight, d.flags, d.h, d.reserved) == (2, 1, 1, 1.5, 0)
    assert list(d.fields) == [capi.FIELDS.index("u"), -1, 0, 0]
    assert list(d.clip_lo) == [0, 1, 2] and list(d.clip_hi) == [3, 4, 5]
    d = capi.sample_desc()
    assert (d.n_fields, d.weight, d.flags, d.h) == (0, 0, 0, 0.0)
    assert list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3
    with pytest.raises(ValueError):
        capi.sample_desc(("u",) * 5)
    with pytest.raises(KeyError):
        capi.sample_desc(("u",), weight="number")


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "sample_caller", """program sample_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_sample_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: px(:), py(:), pz(:), out(:, :), w(:)
  integer(c_int64_t), target :: counts(2)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%h = 0.0_c_double
  d%fields = [SPH_F_RHO, SPH_F_U, SPH_SAMPLE_VALUES, 0]
  d%n_fields = 2
  d%weight = SPH_RENDER_WEIGHT_VOLUME
  d%flags = SPH_SAMPLE_NORMALISE
  d%reserved = 0
  if (c_sizeof(d) /= 88) stop 1
  allocate(px(10), py(10), pz(10), out(10, 2), w(10))
  st = sph_sample(ctx, d, 10_c_int64_t, c_loc(px), c_loc(py), c_loc(pz), c_null_ptr, c_loc(out), 20_c_int64_t, c_loc(w), &
                  c_loc(counts))
  st = sph_sample_dev(ctx, d, 0_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t, &
                      c_null_ptr, c_null_ptr)
  print *, st, counts
end program sample_caller
""")


@needs_hipcc
def test_sample_kernels_fit_the_register_budget():
    k = resource_usage("sample.hip", containing("sample_"))
    for name in ("sample_select", "sample_levels", "sample_no_sources", "sample_keys", "sample_records", "sample_tails",
                 "sample_point_keys"):
        assert sum(name in n for n in k) == 1, name
    walks = [n for n in k if "sample_walk" in n]
    assert len(walks) == 10, walks
    for kk in (0, 1, 2, 3, 4):
        for per_h in (0, 1):
            assert sum(f"sample_walkILi{kk}ELb{per_h}E" in n for n in walks) == 1, (kk, per_h)
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def _rel(got, want):
    s = np.max(np.abs(want))
    return float(np.max(np.abs(got - want)) / s)


def _particles(n, seed, wide=False):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 12.0, (n, 3))
    m = rng.uniform(0.5, 1.5, n)
    h = 2.0 ** rng.uniform(-5.0, 1.0, n) if wide else rng.uniform(0.5, 1.2, n)
    A = np.stack([np.sin(pos[:, 0]) + pos[:, 1], rng.normal(size=n), pos[:, 2] ** 2])
    rho = rng.uniform(0.5, 2.0, n)
    return pos, m, h, A, rho


@pytest.mark.parametrize("wide", [False, True])
def test_restatement_matches_the_brute_force(wide):
    pos, m, h, A, rho = _particles(3000, 21, wide)
    rng = np.random.default_rng(22)
    pts = np.concatenate([rng.uniform(-1.0, 13.0, (2500, 3)), pos[:500]])
    for hh in (h, 0.9):
        for r in (None, rho):
            out, den, cnt = sample_ref.sample(pts, pos, m, hh, A, r)
            w = m if r is None else m / r
            for k in range(3):
                bn, bd = render_field_ref.brute(pts, pos, w, A[k], hh)
                assert _rel(out[k], bn) <= 1e-13, (k, wide)
            assert _rel(den, bd) <= 1e-13
            assert cnt == (int(np.count_nonzero(bd)), 0)
            on, _, _ = sample_ref.sample(pts, pos, m, hh, A, r, normalise=True)
            for k in range(3):
                bn, bd = render_field_ref.brute(pts, pos, w, A[k], hh)
                assert _rel(on[k], render_field_ref.ratio(bn, bd)) <= 1e-13, k


def test_restatement_selection_zeros_and_nan():
    pos, m, h, A, rho = _particles(1500, 23)
    pos[7] = [np.nan, 1.0, 1.0]                                    # a non-finite source is never selected
    pts = np.concatenate([np.random.default_rng(24).uniform(0.0, 12.0, (400, 3)), [[100.0, 0, 0], [np.inf, 0, 0], [0, np.nan, 0]]])
    clip = ((1.0, -np.inf, 2.0), (9.0, 10.0, np.inf))
    sel = sample_ref.sources_mask(pos, 1000, clip)
    assert not sel[7] and not sel[1000:].any() and 0 < sel.sum() < 1000
    assert np.all((pos[sel, 0] > 1.0) & (pos[sel, 0] < 9.0) & (pos[sel, 1] < 10.0) & (pos[sel, 2] > 2.0))
    out, den, cnt = sample_ref.sample(pts, pos, m, h, A, n_owned=1000, clip=clip)
    bn, bd = render_field_ref.brute(pts[:401], pos[sel], m[sel], A[0][sel], h[sel])
    assert _rel(out[0][:401], bn) <= 1e-13 and _rel(den[:401], bd) <= 1e-13
    assert den[400] == 0.0 and np.all(out[:, 400] == 0.0)          # farther than 2 h from every source: exact zeros
    assert np.all(np.isnan(den[401:])) and np.all(np.isnan(out[:, 401:])) and cnt[1] == 2
    assert cnt[0] == int(np.count_nonzero(bd))
    # an empty source set: zeros
    out, den, cnt = sample_ref.sample(pts[:400], pos, m, h, A, clip=((50.0,) * 3, (60.0,) * 3), normalise=True)
    assert cnt == (0, 0) and np.all(out == 0.0) and np.all(den == 0.0)
    # the halves of an owned / ghost split add up to the whole
    whole = sample_ref.sample(pts[:400], pos, m, h, A)
    a = sample_ref.sample(pts[:400], pos, m, h, A, n_owned=700)
    order = np.concatenate([np.arange(700, 1500), np.arange(700)])
    b = sample_ref.sample(pts[:400], pos[order], m[order], h[order], A[:, order], n_owned=800)
    assert _rel(a[0] + b[0], whole[0]) <= 1e-13 and _rel(a[1] + b[1], whole[1]) <= 1e-13


def test_polar_points_follow_the_profile_frame():
    from summersph_amd import capi
    normal, centre = (0.3, -0.4, 0.8), (1.0, -2.0, 0.5)
    pts, shape = smp.polar_points(5.0, 45.0, 8, 16, z=0.7, centre=centre, normal=normal)
    assert shape == (8, 16) and pts.shape == (128, 3)
    d = capi.profile_desc(5.0, 45.0, 8, 16, normal=normal)
    n, e1, e2 = profile_ref.axes(d.normal[:])
    fn, f1, f2 = smp.frame(normal)
    assert np.array_equal(fn, n) and np.array_equal(f1, e1) and np.array_equal(f2, e2)
    r = pts - np.asarray(centre)
    X, Y, Z = r @ e1, r @ e2, r @ n
    assert np.allclose(Z, 0.7, rtol=0, atol=1e-13)
    R, phi = np.hypot(X, Y).reshape(shape), np.arctan2(Y, X).reshape(shape)
    edges = profile_ref.edges(5.0, 45.0, 8)
    assert np.allclose(R, (0.5 * (edges[:-1] + edges[1:]))[:, None], rtol=1e-14)
    assert np.allclose(phi, (-np.pi + 2.0 * np.pi * (np.arange(16) + 0.5) / 16)[None, :], rtol=0, atol=1e-14)
    # every point falls into the profile bin it is named after: ring k, sector j
    ring = np.searchsorted(edges, R, side="right") - 1
    sector = np.floor((phi + np.pi) / (2.0 * np.pi / 16)).astype(int)
    assert np.array_equal(ring, np.repeat(np.arange(8), 16).reshape(shape))
    assert np.array_equal(sector, np.tile(np.arange(16), 8).reshape(shape))
    # the lab frame, log radii
    pts, _ = smp.polar_points(2.0, 32.0, 4, 4, log=True)
    le = profile_ref.edges(2.0, 32.0, 4, log=True)
    assert np.all(pts[:, 2] == 0.0) and np.allclose(np.hypot(pts[:, 0], pts[:, 1]).reshape(4, 4)[:, 0], np.sqrt(le[:-1] * le[1:]))
    assert np.allclose(np.arctan2(pts[:4, 1], pts[:4, 0]), [-0.75 * np.pi, -0.25 * np.pi, 0.25 * np.pi, 0.75 * np.pi])
    for bad in ((5.0, 5.0, 4, 4), (-1.0, 5.0, 4, 4), (1.0, 5.0, 0, 4), (1.0, 5.0, 4, 0)):
        with pytest.raises(ValueError):
            smp.polar_points(*bad)
    with pytest.raises(ValueError):
        smp.polar_points(0.0, 5.0, 4, 4, log=True)
    with pytest.raises(ValueError):
        smp.polar_points(1.0, 5.0, 4, 4, normal=(0, 0, 0))


def test_rz_plane_and_line_points():
    normal = (0.0, 1.0, 1.0)
    n, e1, e2 = smp.frame(normal)
    pts, shape = smp.rz_points(10.0, 50.0, 5, -4.0, 4.0, 9, phi=0.5, centre=(1, 2, 3), normal=normal)
    assert shape == (5, 9) and pts.shape == (45, 3)
    r = pts - np.array([1.0, 2.0, 3.0])
    assert np.allclose((r @ n).reshape(shape), np.linspace(-4, 4, 9)[None, :], atol=1e-13)
    assert np.allclose(np.arctan2(r @ e2, r @ e1), 0.5) and np.allclose(np.hypot(r @ e1, r @ e2).reshape(shape)[:, 0], [14, 22, 30, 38, 46])
    # a plane: v is made orthogonal to u, the raster is centred and has the asked widths
    c = np.array([1.0, -1.0, 2.0])
    pts, shape = smp.plane_points(c, (2.0, 0.0, 0.0), (1.0, 1.0, 1.0), (10.0, 4.0), (11, 5))
    g = pts.reshape(11, 5, 3)
    du, dv = g[1, 0] - g[0, 0], g[0, 1] - g[0, 0]
    assert shape == (11, 5) and abs(np.dot(du, dv)) <= 1e-14
    assert np.allclose(du, [1.0, 0.0, 0.0]) and np.allclose(dv, np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0))
    assert np.allclose(g.mean(axis=(0, 1)), c) and np.allclose(g[5, 2], c)
    assert np.isclose(np.linalg.norm(g[-1, 0] - g[0, 0]), 10.0) and np.isclose(np.linalg.norm(g[0, -1] - g[0, 0]), 4.0)
    with pytest.raises(ValueError):
        smp.plane_points(c, (1, 0, 0), (-3, 0, 0), (1, 1), (2, 2))
    pts, shape = smp.line_points((0, 0, 0), (3, 6, -9), 4)
    assert shape == (4,) and np.array_equal(pts, [[0, 0, 0], [1, 2, -3], [2, 4, -6], [3, 6, -9]])


def test_cli_parsing(tmp_path):
    ap = smp.build_parser()
    a = ap.parse_args(["save.txt", "-o", "o.npz", "--polar", "10", "50", "8", "16", "--fields", "rho,u,vy", "--normalise"])
    pts, shape = smp.points_from_args(a)
    ref, _ = smp.polar_points(10.0, 50.0, 8, 16)
    assert shape == (8, 16) and np.array_equal(pts, ref)
    assert smp.parse_fields(a.fields) == ["rho", "u", "vy"] and a.normalise and not a.volume and a.h is None
    a = ap.parse_args(["s", "-o", "o", "--rz", "10", "50", "4", "-3", "3", "7", "--phi", "1.0", "--normal", "0,1,1", "--log"])
    assert np.array_equal(smp.points_from_args(a)[0], smp.rz_points(10.0, 50.0, 4, -3.0, 3.0, 7, 1.0, True, (0, 0, 0), (0, 1, 1))[0])
    a = ap.parse_args(["s", "-o", "o", "--plane", "0,0,1", "1,0,0", "0,1,0", "20", "10", "5", "3"])
    assert smp.points_from_args(a)[1] == (5, 3)
    a = ap.parse_args(["s", "-o", "o", "--line", "0,0,0", "10,0,0", "11", "--volume", "--h", "2.0"])
    assert np.array_equal(smp.points_from_args(a)[0][:, 0], np.arange(11.0)) and a.volume and a.h == 2.0
    my = np.arange(24.0).reshape(2, 4, 3)
    np.save(tmp_path / "p.npy", my)
    a = ap.parse_args(["s", "-o", "o", "--points", str(tmp_path / "p.npy")])
    pts, shape = smp.points_from_args(a)
    assert shape == (2, 4) and np.array_equal(pts, my.reshape(-1, 3))
    np.save(tmp_path / "q.npy", np.zeros((4, 2)))
    with pytest.raises(ValueError):
        smp.points_from_args(ap.parse_args(["s", "-o", "o", "--points", str(tmp_path / "q.npy")]))
    assert smp.parse_fields("") == [] and smp.parse_fields("h", variable=True) == ["h"]
    for bad in ("h", "rho,u,vx,vy,vz", "nope"):
        with pytest.raises(ValueError):
            smp.parse_fields(bad)
    assert smp.parse_clip("0,1,2,3,4,5") == ((0.0, 1.0, 2.0), (3.0, 4.0, 5.0))
    with pytest.raises(ValueError):
        smp.parse_clip("0,1,2,3,4")
    for argv in (["s", "-o", "o"], ["s", "-o", "o", "--polar", "1", "2", "3", "4", "--line", "0,0,0", "1,1,1", "2"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
