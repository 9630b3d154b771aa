"""CPU tests of the emission-absorption images (sph_transfer): the ABI mirrors (ctypes, Fortran) against the C header, the
resource use of transfer.hip's kernels, the numpy restatement against the closed forms it must obey (a uniform source, T
against exp(-tau), two sheets and the flipped view, the optically thin bound), against its own brute force, and the
command line's parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import transfer_ref
from summersph_amd import cube as cb

FIELDS = ["rot", "centre", "lo", "hi", "clip_lo", "clip_hi", "h", "kappa_scale", "tau_surface", "tau_max", "background", "n_u",
          "n_v", "source", "kappa", "flags", "reserved"]
FLIP = np.diag([-1.0, 1.0, -1.0])                    # (u^, v^, w^) -> (-u^, v^, -w^): the view from behind


def test_transfer_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_transfer_desc", FIELDS,
                   ['printf("consts %d %d\\n", SPH_TRANSFER_VALUES, SPH_TRANSFER_ONE);', 'printf("abi %d\\n", SPH_ABI_VERSION);'])
    assert int(got["size"]) == ctypes.sizeof(capi.TransferDesc) == 240
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.TransferDesc, f).offset, f
    assert got["consts"] == f"{capi.TRANSFER_VALUES} {capi.TRANSFER_ONE}" == "-1 -2"
    assert got["abi"] == "1"                                        # the change is additive
    assert "sph_transfer" in capi.SYMBOLS and "sph_transfer_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_TRANSFER_VALUES = -1", binding) and re.search(r"SPH_TRANSFER_ONE = -2", binding)
    d = capi.transfer_desc((5, 7), ((-1, -2), (3, 4)), rot=cb.view(40, 30), centre=(1, 2, 3), source="rho", kappa=np.zeros(3),
                           kappa_scale=2.5, tau_surface=0.5, tau_max=30.0, background=0.25, h=1.5, clip=((0, 1, 2), (3, 4, 5)))
    assert (d.n_u, d.n_v, d.source, d.kappa, d.flags, d.reserved) == (5, 7, capi.FIELDS.index("rho"), capi.TRANSFER_VALUES, 0, 0)
    assert (d.kappa_scale, d.tau_surface, d.tau_max, d.background, d.h) == (2.5, 0.5, 30.0, 0.25, 1.5)
    assert list(d.lo) == [-1, -2] and list(d.hi) == [3, 4] and list(d.centre) == [1, 2, 3]
    assert list(d.clip_lo) == [0, 1, 2] and list(d.clip_hi) == [3, 4, 5]
    assert np.array_equal(np.array(d.rot[:]).reshape(3, 3), cb.view(40, 30))
    d = capi.transfer_desc(4, ((0, 0), (1, 1)))
    assert (d.n_u, d.n_v, d.h, d.kappa_scale, d.tau_surface, d.tau_max, d.background) == (4, 4, 0.0, 1.0, 1.0, np.inf, 0.0)
    assert (d.source, d.kappa) == (capi.FIELDS.index("u"), capi.TRANSFER_ONE) and list(d.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3
    assert capi.transfer_desc(4, ((0, 0), (1, 1)), source=None, kappa=7).source == capi.TRANSFER_ONE
    with pytest.raises(ValueError):
        capi.transfer_desc((1, 2, 3), ((0, 0), (1, 1)))


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "transfer_caller", """program transfer_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_transfer_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: out(:, :, :), vals(:)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%rot = [1.0_c_double, 0.0_c_double, 0.0_c_double, 0.0_c_double, 1.0_c_double, 0.0_c_double, 0.0_c_double, 0.0_c_double, &
           1.0_c_double]
  d%centre = 0.0_c_double
  d%lo = [-10.0_c_double, -10.0_c_double]
  d%hi = [10.0_c_double, 10.0_c_double]
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%h = 0.0_c_double
  d%kappa_scale = 50.0_c_double
  d%tau_surface = 1.0_c_double
  d%tau_max = ieee_value(1.0_c_double, ieee_positive_inf)
  d%background = 0.0_c_double
  d%n_u = 8
  d%n_v = 6
  d%source = SPH_TRANSFER_VALUES
  d%kappa = SPH_TRANSFER_ONE
  d%flags = 0
  d%reserved = 0
  if (c_sizeof(d) /= 240) stop 1
  allocate(out(6, 8, 4), vals(10))
  st = sph_transfer(ctx, d, c_loc(vals), c_null_ptr, c_loc(out), 192_c_int64_t)
  st = sph_transfer_dev(ctx, d, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int64_t)
  print *, st
end program transfer_caller
""")


@needs_hipcc
def test_transfer_kernels_fit_the_register_budget():
    k = resource_usage("transfer.hip", containing("transfer_", "stats_final", "start_table"))
    names = ("transfer_stats_partial", "stats_final", "transfer_count", "transfer_select", "transfer_depth_keys",
             "transfer_records", "transfer_emit", "start_table", "transfer_gather")
    for name in names:
        assert sum(name in n for n in k) == 1, name
    assert len(k) == len(names), sorted(k)
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        # the front end at full occupancy; the gather within four wavefronts a SIMD
        assert 0 < r.get("VGPRs", 999) <= (128 if "transfer_gather" in name else 64), (name, r)
    g = [r for n, r in k.items() if "transfer_gather" in n][0]
    # six planes of one 128-record stage, the records' masks and bases, 256 pairs of 18 bytes, the nodes: at least eleven tiles a CU
    assert g["SGPRs Spill"] == 0 and 6 * 128 * 8 + 256 * 18 <= g["LDS Size"] <= 160 * 1024 // 11, g


def _sheet(rng, n, z, extent, jitter=0.0):
    pos = np.stack([rng.uniform(-extent, extent, n), rng.uniform(-extent, extent, n), z + jitter * rng.normal(size=n)], axis=1)
    return pos


def test_uniform_source_and_transmission():
    rng = np.random.default_rng(11)
    n = 600
    pos = rng.uniform(-5, 5, (n, 3))
    m, h, K = rng.uniform(0.5, 1.5, n), 2.0 ** rng.uniform(-1.5, 0.5, n), rng.uniform(0.0, 2.0, n)
    kw = dict(shape=(14, 11), bounds=((-4.0, -3.5), (3.5, 4.0)), rot=cb.view(40.0, 30.0, 10.0), kappa=K)
    for scale in (0.05, 3.0, 200.0):
        out = transfer_ref.transfer(pos, m, h, source=np.full(n, 2.5), kappa_scale=scale, **kw)
        I, tau, T, surf = out
        assert np.max(np.abs(T - np.exp(-tau))) <= 1e-12, scale
        assert np.max(np.abs(I - 2.5 * (1.0 - T))) <= 1e-12 * 2.5, scale                       # I = S (1 - T)
        assert np.array_equal(np.isnan(surf), ~(tau >= 1.0))
    assert np.isfinite(surf).any() and np.isnan(transfer_ref.transfer(pos, m, h, kappa_scale=1e-6, **kw)[3]).all()
    # a background is attenuated by T
    plain = transfer_ref.transfer(pos, m, h, source=np.full(n, 2.5), kappa_scale=3.0, **kw)
    bg = transfer_ref.transfer(pos, m, h, source=np.full(n, 2.5), kappa_scale=3.0, background=0.7, **kw)
    assert np.array_equal(bg[0], plain[0] + plain[2] * 0.7) and np.array_equal(bg[1:], plain[1:], equal_nan=True)
    # tau_max stops a node: tau is what had accumulated, at least tau_max, and deeper particles add nothing
    info, tmax = {}, float(np.median(out[1]))
    cut = transfer_ref.transfer(pos, m, h, source=np.full(n, 2.5), kappa_scale=200.0, tau_max=tmax, info=info, **kw)
    assert info["stopped"].any() and not info["stopped"].all()
    assert np.all(cut[1][info["stopped"]] >= tmax) and np.all(cut[1] <= out[1] + 1e-12)
    assert np.array_equal(cut[1][~info["stopped"]], out[1][~info["stopped"]])


def test_two_sheets_and_the_flipped_view():
    rng = np.random.default_rng(12)
    n1, n2 = 500, 700
    pos = np.concatenate([_sheet(rng, n1, -1.0, 6.0, 0.05), _sheet(rng, n2, 2.0, 6.0, 0.05)])
    n = n1 + n2
    m, h = rng.uniform(0.5, 1.5, n), rng.uniform(0.6, 1.2, n)
    S1, S2 = 3.0, 0.5
    S = np.concatenate([np.full(n1, S1), np.full(n2, S2)])
    first = np.arange(n) < n1
    kw = dict(shape=(13, 12), bounds=((-3.0, -3.0), (3.0, 3.0)), kappa_scale=0.5)
    out = transfer_ref.transfer(pos, m, h, source=S, **kw)
    tau1 = transfer_ref.transfer(pos[first], m[first], h[first], **kw)[1]
    tau2 = transfer_ref.transfer(pos[~first], m[~first], h[~first], **kw)[1]
    assert 0.2 < np.median(tau1) < 5.0 and 0.2 < np.median(tau2) < 5.0
    want = S1 * (1 - np.exp(-tau1)) + np.exp(-tau1) * S2 * (1 - np.exp(-tau2))
    assert np.max(np.abs(out[0] - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(out[1] - (tau1 + tau2))) <= 1e-12 * np.max(out[1])
    # from behind the sheets swap their roles; the image's u axis is mirrored
    back = transfer_ref.transfer(pos, m, h, source=S, rot=FLIP, **kw)
    want = (S2 * (1 - np.exp(-tau2)) + np.exp(-tau2) * S1 * (1 - np.exp(-tau1)))[::-1]
    assert np.max(np.abs(back[0] - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(back[0][::-1] - out[0])) > 0.1 * np.max(out[0])                      # the order matters
    # the surface lies in the sheet that carries tau across 1 and its depth changes sign with the view
    both = np.isfinite(out[3]) & np.isfinite(back[3][::-1])
    assert both.any() and np.all(out[3][both & (tau1 >= 1.2)] < 0.0) and np.all(back[3][::-1][both & (tau2 >= 1.2)] < 0.0)


def test_optically_thin_bound_and_brute_force():
    rng = np.random.default_rng(13)
    n = 500
    pos = rng.uniform(-5, 5, (n, 3))
    m, h = rng.uniform(0.5, 1.5, n), 2.0 ** rng.uniform(-1.5, 0.5, n)
    K, S = rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 3.0, n)
    rot = cb.view(55.0, 20.0)
    kw = dict(shape=(12, 9), bounds=((-4.0, -3.5), (3.5, 4.0)), rot=rot, source=S, kappa=K)
    for scale in (1e-4, 0.02, 1.0):
        info = {}
        out = transfer_ref.transfer(pos, m, h, kappa_scale=scale, info=info, **kw)
        thin, tau = info["thin"], out[1]
        assert np.all(out[0] <= thin * (1 + 1e-13)) and np.all(out[0] >= thin * (1.0 - tau) - 1e-13 * np.abs(thin))
    # the vectorised restatement against the scalar brute force, with a clip, ghosts, a stop and a background
    clip = ((-4.0, -np.inf, -3.0), (4.5, 3.0, np.inf))
    S2 = rng.normal(size=n)                                           # S of both signs
    kw = dict(kw, source=S2, clip=clip, n_owned=420, kappa_scale=2.0, background=-0.3, centre=(0.3, -0.2, 0.1))
    ts = float(np.median(transfer_ref.transfer(pos, m, h, **kw)[1]))      # half of the nodes reach the surface, some stop
    kw = dict(kw, tau_surface=ts, tau_max=1.5 * ts)
    out = transfer_ref.transfer(pos, m, h, **kw)
    gu, gv = np.linspace(-4.0, 3.5, 12), np.linspace(-3.5, 4.0, 9)
    pix = np.array([(i, j) for i in range(12) for j in range(9)])
    nkw = {k: v for k, v in kw.items() if k not in ("shape", "bounds")}
    brute = transfer_ref.transfer_nodes(pos, m, h, gu, gv, pix, **nkw).reshape(4, 12, 9)
    assert np.array_equal(np.isnan(out[3]), np.isnan(brute[3])) and np.isfinite(out[3]).any() and np.isnan(out[3]).any()
    for k in range(4):
        assert np.allclose(out[k], brute[k], rtol=0, atol=1e-13 * np.nanmax(np.abs(brute[k])), equal_nan=True), k
    # equal depths fall to the id; -0.0 and +0.0 are one depth
    flat = pos.copy()
    flat[:, 2] = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    order = transfer_ref.inputs(flat, m, h, None, None)[0]
    assert np.array_equal(order, np.arange(n))


def test_cli_parsing():
    from summersph_amd import transfer as tr
    ap = tr.build_parser()
    a = ap.parse_args(["save275.txt", "-o", "img.npz", "--inc", "40", "--pa", "30", "--extent", "200", "--size", "256",
                       "--kappa-scale", "50", "--source", "u", "--tau-surface", "1", "--tau-max", "30", "--png", "img.png", "--json"])
    kw = tr.args_desc(a)
    assert kw["shape"] == (256, 256) and kw["bounds"] == ((-100.0, -100.0), (100.0, 100.0))
    assert np.array_equal(kw["rot"], cb.view(40.0, 30.0)) and kw["source"] == "u" and kw["kappa"] is None
    assert (kw["kappa_scale"], kw["tau_surface"], kw["tau_max"], kw["background"]) == (50.0, 1.0, 30.0, 0.0)
    assert kw["h"] is None and kw["clip"] is None and a.png == "img.png" and a.json and not a.variable
    a = ap.parse_args(["s", "-o", "o", "--extent", "50", "--azimuth", "15", "--centre", "1,2,3", "--h", "2", "--clip", "0,1,2,3,4,5",
                       "--source", "one", "--kappa", "rho", "--background", "0.5", "--variable"])
    kw = tr.args_desc(a)
    assert kw["centre"] == (1.0, 2.0, 3.0) and kw["h"] == 2.0 and kw["clip"] == ((0.0, 1.0, 2.0), (3.0, 4.0, 5.0))
    assert kw["source"] is None and kw["kappa"] == "rho" and kw["tau_max"] == np.inf and kw["background"] == 0.5 and a.variable
    assert np.array_equal(kw["rot"], cb.view(0, 0, 15))
    for extra in (["--size", "0"], ["--h", "-1"], ["--kappa-scale", "-0.1"], ["--kappa-scale", "inf"], ["--tau-surface", "0"],
                  ["--tau-max", "-1"], ["--tau-max", "nan"], ["--background", "inf"], ["--centre", "1,2"], ["--clip", "1,2,3"],
                  ["--source", "temperature"], ["--kappa", "h"], ["--extent", "-5"]):
        with pytest.raises(ValueError):
            tr.args_desc(ap.parse_args(["s", "-o", "o", "--extent", "50"] + extra))
    for argv in (["s", "-o", "o"], ["s", "--extent", "5"], ["-o", "o", "--extent", "5"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
