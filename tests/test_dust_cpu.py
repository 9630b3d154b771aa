"""CPU tests of the tracer grains (sph_dust): the ABI mirrors (ctypes, Fortran) against the C header, the register budget
of the dust kernels, and the scheme itself on the numpy restatement: second order in the interval, exact composition of
the drag factors, and the stiff limit."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import dust_ref

FIELDS = ["capacity", "every", "record_every", "law", "flags", "rho_grain"]


def test_dust_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_dust_desc", FIELDS,
                   ['printf("consts %d %d %d %d %d\\n", SPH_DUST_EPSTEIN, SPH_DUST_FIXED_TS, SPH_DUST_REMOVE, SPH_DUST_NHEAD, '
                    'SPH_DUST_NCOL);'])
    assert int(got["size"]) == ctypes.sizeof(capi.DustDesc) == 32
    offsets = {"capacity": 0, "every": 8, "record_every": 12, "law": 16, "flags": 20, "rho_grain": 24}
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.DustDesc, f).offset == offsets[f], f
    assert got["consts"] == (f"{capi.DUST_EPSTEIN} {capi.DUST_FIXED_TS} {capi.DUST_REMOVE} {capi.DUST_NHEAD} {capi.DUST_NCOL}"
                             ) == "0 1 1 4 12"
    assert len(capi.DUST_COLUMNS) == capi.DUST_NCOL and len(capi.DUST_HEAD) == capi.DUST_NHEAD
    assert capi.DUST_FATES == ["fate", "advance", "sink"]
    assert (capi.DUST_EPSTEIN, capi.DUST_FIXED_TS) == (dust_ref.EPSTEIN, dust_ref.FIXED_TS)
    for s in ("begin", "begin_dev", "end", "advance", "info", "read", "read_dev", "state", "state_dev", "fates", "fates_dev"):
        assert "sph_dust_" + s in capi.SYMBOLS, s
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_DUST_NHEAD = 4, SPH_DUST_NCOL = 12", binding)
    d = capi.dust_desc("epstein", rho_grain=2.5, capacity=7, every=3, record_every=2, remove=True)
    assert (d.capacity, d.every, d.record_every, d.law, d.flags, d.rho_grain) == (7, 3, 2, 0, 1, 2.5)
    d = capi.dust_desc("fixed_ts")
    assert (d.capacity, d.every, d.record_every, d.law, d.flags, d.rho_grain) == (0, 1, 1, 1, 0, 0.0)
    with pytest.raises(ValueError):
        capi.dust_desc("epstein")
    with pytest.raises(ValueError):
        capi.dust_desc("stokes", rho_grain=1.0)


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "dust_caller", """program dust_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_dust_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable, target :: s(:, :), head(:, :), body(:, :, :)
  integer(c_int32_t), allocatable, target :: fates(:, :)
  integer(c_int64_t), target :: info(5)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%capacity = 3_c_int64_t
  d%every = 1
  d%record_every = 1
  d%law = SPH_DUST_EPSTEIN
  d%flags = SPH_DUST_REMOVE
  d%rho_grain = 1.0e6_c_double
  if (c_sizeof(d) /= 32) stop 1
  if (SPH_DUST_FIXED_TS /= 1) stop 2
  allocate(s(10, 7), head(SPH_DUST_NHEAD, 3), body(10, SPH_DUST_NCOL, 3), fates(3, 10))
  s = 1.0_c_double
  st = sph_dust_begin(ctx, d, 10_c_int64_t, s(:, 1), s(:, 2), s(:, 3), s(:, 4), s(:, 5), s(:, 6), s(:, 7))
  st = sph_dust_begin_dev(ctx, d, 10_c_int64_t, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
  st = sph_dust_advance(ctx)
  st = sph_dust_info(ctx, c_loc(info(1)), c_loc(info(2)), c_loc(info(3)), c_loc(info(4)), c_loc(info(5)))
  st = sph_dust_read(ctx, 0_c_int64_t, 3_c_int64_t, c_loc(head), c_loc(body))
  st = sph_dust_read_dev(ctx, 0_c_int64_t, 0_c_int64_t, c_null_ptr, c_null_ptr)
  st = sph_dust_state(ctx, c_loc(s(1, 1)), c_loc(s(1, 2)), c_loc(s(1, 3)), c_loc(s(1, 4)), c_loc(s(1, 5)), c_loc(s(1, 6)), &
                      c_loc(s(1, 7)))
  st = sph_dust_state_dev(ctx, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
  st = sph_dust_fates(ctx, c_loc(fates))
  st = sph_dust_fates_dev(ctx, c_null_ptr)
  st = sph_dust_end(ctx)
  print *, st
end program dust_caller
""")


@needs_hipcc
def test_dust_kernels_fit_the_register_budget():
    k = resource_usage("dust.hip", containing("dust_"))
    for name, count in (("dust_kick_drift", 1), ("dust_walk", 2), ("dust_head", 1)):
        assert sum(name in n for n in k) == count, (name, sorted(k))
    assert len(k) == 4
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


# ---- the scheme on the restatement alone -------------------------------------------------------------------------------
NO_SINKS = {"x": np.zeros(0), "y": np.zeros(0), "z": np.zeros(0), "m": np.zeros(0)}
ONE_SINK = {"x": np.zeros(1), "y": np.zeros(1), "z": np.zeros(1), "m": np.ones(1)}


def run(x, v, par, steps, delta, gas, sinks):
    """`steps` chained advances of delta after the re-sample at delta = 0"""
    S = {"a": np.zeros_like(x), "vg": np.zeros_like(x), "r": np.zeros(len(x))}
    o = dust_ref.advance(x, v, par, S, 0.0, gas, sinks)
    for _ in range(steps):
        o = dust_ref.advance(o["x"], o["v"], par, o["S"], delta, gas, sinks)
        assert (o["fate"] == 0).all()
    return o


def test_kepler_orbit_is_second_order_in_the_interval():
    """a circular orbit of radius 1 about a unit sink, no drag: the end-position error falls by 4 when the interval is halved.
    With 100 and 200 intervals over T = 1 the error is ~1e-6, ten orders above rounding."""
    x, v = np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]])
    none = {"rho": np.zeros(1), "vg": np.zeros((1, 3)), "u": np.zeros(1)}
    T, exact = 1.0, np.array([np.cos(1.0), np.sin(1.0), 0.0])
    err = [np.linalg.norm(run(x, v, np.ones(1), n, T / n, none, ONE_SINK)["x"][0] - exact) for n in (100, 200)]
    assert err[0] > 1e-8 and 3.5 <= err[0] / err[1] <= 4.5, err


def test_drag_in_uniform_gas_is_second_order_in_position_and_exact_in_velocity():
    """uniform gas at rest, a fixed stopping time, no gravity: v = v0 exp(-t / t_s) for any interval (the exact factors
    compose), x by the midpoint rule (second order)."""
    ts, T, v0 = 0.7, 2.0, np.array([[0.3, -1.1, 0.5]])
    gas = {"rho": np.ones(1), "vg": np.zeros((1, 3)), "u": np.ones(1)}
    exact_x = v0[0] * ts * (1.0 - np.exp(-T / ts))
    err = []
    for n in (1, 3, 40, 80):
        o = run(np.zeros((1, 3)), v0, np.full(1, ts), n, T / n, gas, NO_SINKS)
        want = v0[0] * np.exp(-T / ts)
        assert np.abs(o["v"][0] - want).max() <= 1e-14 * np.abs(want).max(), n
        if n in (40, 80):
            err.append(np.linalg.norm(o["x"][0] - exact_x))
    assert err[0] > 1e-8 and 3.5 <= err[0] / err[1] <= 4.5, err


@pytest.mark.parametrize("k", [1e6, 1e9, 1e300])
def test_a_stiff_half_kick_gives_the_terminal_velocity(k):
    rng = np.random.default_rng(5)
    v, a, vg = rng.normal(size=(50, 3)), rng.normal(size=(50, 3)) * 3.0, rng.normal(size=(50, 3))
    tau = 0.01
    r = np.full(50, k / tau)
    got = dust_ref.half_kick(v, a, vg, r, tau)
    assert np.isfinite(got).all()
    norm = lambda w: np.linalg.norm(w, axis=1)
    assert (norm(got - (vg + a / r[:, None])) <= 1e-14 * (norm(vg) + norm(a) / r)).all()
