"""CPU tests of the density rendering (sph_render_density): the ABI mirrors (ctypes, Fortran) against the C header, the
numpy restatement against the reference script's own image, the CLI's save-file parsing and row selection, and the
gather kernels' register budget (no spills, no scratch)."""
import numpy as np

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import load_golden
import render_ref
from summersph_amd import render, txtio

FIELDS = ["lo", "hi", "clip_lo", "clip_hi", "h", "n", "axis", "flags", "reserved"]


def test_render_desc_layout_matches_header(tmp_path):
    from summersph_amd.capi import RenderDesc
    got = c_layout(tmp_path, "sph_render_desc", FIELDS,
                   ['printf("auto %d spacing %d\\n", SPH_RENDER_AUTO_BOUNDS, SPH_RENDER_SPACING);'])
    assert int(got["size"]) == __import__("ctypes").sizeof(RenderDesc) == 128
    for f in FIELDS:
        assert int(got[f]) == getattr(RenderDesc, f).offset, f
    from summersph_amd import capi
    assert got["auto"] == f"{capi.RENDER_AUTO_BOUNDS} spacing {capi.RENDER_SPACING}"


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "render_caller", """program render_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_render_desc) :: d
  type(c_ptr) :: ctx
  real(c_double), allocatable :: img(:, :)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%h = 1.25_c_double
  d%n = [120, 120, 120]
  d%axis = 2
  d%flags = SPH_RENDER_AUTO_BOUNDS
  d%reserved = 0
  allocate(img(d%n(2), d%n(1)))
  st = sph_render_density(ctx, d, img, int(size(img), c_int64_t))
  if (c_sizeof(d) /= 128) stop 1
  st = sph_render_density_dev(ctx, d, c_null_ptr, 0_c_int64_t)
  print *, st
end program render_caller
""")


def test_numpy_restatement_reproduces_the_script():
    g = load_golden("render_script12k")
    pos = np.stack([g["script_x"], g["script_y"], g["script_z"]], axis=1)
    b = g["bounds"]
    res = int(g["grid_resolution"])
    grid = render_ref.grid_scatter(pos, g["script_mass"], float(g["h"]), b[:3], b[3:], (res,) * 3)
    proj = grid.sum(axis=2)
    ref = g["projected_density"]
    assert proj.shape == ref.shape == (120, 120)
    assert np.max(np.abs(proj - ref)) <= 1e-12 * ref.max()
    assert np.array_equal(proj == 0, ref == 0)


def test_save_parsing_and_script_row_selection(tmp_path):
    g = load_golden("render_script12k")
    p = tmp_path / "save.txt"
    txtio.write_save(str(p), g["gas"], g["sinks"])
    gas, sinks, skipped = render.read_save(str(p))
    assert skipped == 0 and np.array_equal(gas, g["gas"]) and np.array_equal(sinks[:, [0, 1, 2, 7]], g["sinks"][:, [0, 1, 2, 7]])
    rows = render.script_rows(gas)
    assert np.array_equal(rows[:, 0], g["script_x"]) and np.array_equal(rows[:, 2], g["script_z"])
    assert np.array_equal(rows[:, 7], g["script_mass"])

    # sinks in the middle, gas rows outside the clip at the end: the dropped row is the last gas row INSIDE the clip
    rng = np.random.default_rng(5)
    gas2 = np.zeros((30, 9)); gas2[:, :3] = rng.uniform(-90, 90, (30, 3)); gas2[:, 6] = 0.25; gas2[:, 7] = 1e-6
    gas2[27:, 1] = [150.0, -100.0, 100.0]              # outside the strict |coord| < 100 clip
    sinks2 = np.zeros((2, 8)); sinks2[:, 7] = 1.0; sinks2[1, :3] = 5.0
    with open(tmp_path / "mixed.txt", "w") as f:
        f.write(txtio.SAVE_HEADER + "\n")
        for k in range(30):
            f.write(" ".join(f"{v:.17e}" for v in gas2[k]) + "\n")
            if k == 10:
                f.write(" ".join(f"{v:.17e}" for v in sinks2[0]) + "\n")
        f.write(" ".join(f"{v:.17e}" for v in sinks2[1]) + "\n")
        f.write("1.0 2.0\n")                           # neither gas nor sink: skipped, as the script skips it
    gas3, sinks3, skipped3 = render.read_save(str(tmp_path / "mixed.txt"))
    assert gas3.shape == (30, 9) and sinks3.shape == (2, 8) and skipped3 == 1
    sel = render.script_rows(gas3)
    assert np.array_equal(sel, gas2[:26])              # rows 27..29 clipped, row 26 (the last survivor) dropped


@needs_hipcc
def test_render_kernels_do_not_spill():
    k = resource_usage("render.hip", containing("render_", "stats_final", "start_table"))
    names = " ".join(k)
    for want in ("render_gather", "render_select", "render_stats_partial", "stats_final", "render_records", "start_table"):
        assert want in names, want
    assert sum("render_gather" in n for n in k) == 3
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
