"""CPU tests of the hashed cell table's interface: the ctypes and Fortran mirrors of sph_grid_info against the C header,
the flag's value, and the register budget of the new grid kernels and of the hashed instantiations of the consumers."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from summersph_amd import capi

FC = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "summersph_amd", "csrc")
FIELDS = ["kind", "dim", "occupied_cells", "table_entries", "index_cells", "bytes"]


def test_grid_info_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "summersph.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(sph_grid_info));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(sph_grid_info, {f}));\n' for f in FIELDS) +
                   '  printf("flag %d\\n", SPH_FLAG_HASHED_GRID);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
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


@pytest.mark.skipif(not os.path.exists(FC), reason="needs amdflang")
def test_fortran_binding_compiles_and_links(tmp_path):
    lib = os.path.join(ROOT, "summersph_amd", "libsummersph_hip.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.DEVNULL)
    caller = tmp_path / "grid_caller.f90"
    caller.write_text("""program grid_caller
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
    binding = os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")
    subprocess.run([FC, "-O1", f"-J{tmp_path}", binding, str(caller), "-L" + os.path.dirname(lib), "-lsummersph_hip",
                    "-o", str(tmp_path / "grid_caller")], check=True, cwd=tmp_path)


def _resource_usage(src, pick):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "-c", src, "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1) if pick(m.group(1)) else None
            if cur:
                kernels[cur] = {}
            continue
        m = re.search(r"remark: +([^:\[]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if cur and m:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("src,want", [
    ("grid.hip", ["hash_keys", "hash_heads", "hash_compact", "hash_insert"]),
    ("pairs.hip", ["nlist_kernelILb1"]),
    ("tiled.hip", ["nlist_tiledILb1"]),
    ("varh.hip", ["nlist_v_tiledILb1", "update_h_kernelILb1", "cell_hmax_hashed"]),
])
def test_hashed_kernels_do_not_spill(src, want):
    k = _resource_usage(src, lambda name: any(w in name for w in want))
    for w in want:
        assert any(w in n for n in k), w
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
