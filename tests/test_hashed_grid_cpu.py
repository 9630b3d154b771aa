"""CPU tests of the hashed cell table's interface: the ctypes and Fortran mirrors of sph_grid_info against the C header,
the flag's value, and the register budget of the new grid kernels and of the hashed instantiations of the consumers."""
import os
import re

import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
from summersph_amd import capi

FIELDS = ["kind", "dim", "occupied_cells", "table_entries", "index_cells", "bytes"]


def test_grid_info_layout_matches_header(tmp_path):
    got = c_layout(tmp_path, "sph_grid_info", FIELDS, ['printf("flag %d\\n", SPH_FLAG_HASHED_GRID);'])
    assert int(got["size"]) == __import__("ctypes").sizeof(capi.GridInfo) == 48
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.GridInfo, f).offset, f
    assert int(got["flag"]) == capi.FLAG_HASHED_GRID == 1024


def test_hashed_flag_is_unique():
    flags = {k: v for k, v in vars(capi).items() if k.startswith("FLAG_")}
    assert len(set(flags.values())) == len(flags), flags
    for k, v in flags.items():
        assert v & (v - 1) == 0, k                       # one bit each
    assert capi.FLAG_HASHED_GRID not in (8,)             # bit 8 is retired
    header = open(os.path.join(ROOT, "include", "summersph.h")).read()
    vals = [int(v) for v in re.findall(r"#define SPH_FLAG_\w+ (\d+)", header)]
    assert len(vals) == len(set(vals)) and 1024 in vals


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "grid_caller", """program grid_caller
  use, intrinsic :: iso_c_binding
  use sph_hip_binding
  implicit none
  type(sph_params) :: p
  type(sph_grid_info) :: gi
  type(c_ptr) :: ctx
  integer(c_int) :: st
  st = sph_params_default(p)
  p%flags = ior(p%flags, SPH_FLAG_HASHED_GRID)
  st = sph_ctx_create(p, 0, ctx)
  if (st == SPH_OK) st = sph_get_grid_info(ctx, gi)
  print *, st, gi%kind, gi%dim, gi%occupied_cells, gi%table_entries, gi%index_cells, gi%bytes
end program grid_caller
""")


@needs_hipcc
@pytest.mark.parametrize("src,want", [
    ("grid.hip", ["hash_keys", "hash_heads", "hash_compact", "hash_insert"]),
    ("pairs.hip", ["nlist_kernelILb1"]),
    ("tiled.hip", ["nlist_tiledILb1"]),
    ("varh.hip", ["nlist_v_tiledILb1", "update_h_kernelILb1", "cell_hmax_hashed"]),
])
def test_hashed_kernels_do_not_spill(src, want):
    k = resource_usage(src, containing(*want))
    for w in want:
        assert any(w in n for n in k), w
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
