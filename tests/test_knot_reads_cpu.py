"""What the compiler makes of the whole-tile pair kernels (tiled.hip, gfx950): the two table knots of a visit must be two
ds_read_b64, not one ds_read2_b64 offset1:1 (pair_common.hpp table_knots_at: 8 LDS-array cycles per wave against 2 + 2), and
every variant of density_wt / forces_q must fit the 128 vector registers that four waves per SIMD leave, without spills or
scratch.  Compiles tiled.hip device-only to assembly; needs hipcc, no GPU.

Figures of this tree (the parent commit in brackets), VGPRs / VGPRs Spill / ScratchSize:
  density_wt<1024,true> 84 / 0 / 0 (86 / 0 / 0)      density_wt<1024,false> 90 / 0 / 0 (92 / 0 / 0)
  forces_q<1024,4,true> 124 / 0 / 0 (126 / 0 / 0)    forces_q<1024,4,false> 122 / 0 / 0 (127 / 0 / 0)
  forces_q<1024,8,false> 121 / 0 / 0 (127 / 0 / 0)   forces_q<1024,8,true> 128 / 0 / 0 (128 / 7 / 32)
The last one -- the half-group kernel of dense neighbourhoods -- spilled in the parent commit, around its pair loop and once per
group; DESIGN.md section 4 "Round 5" says what was parked there and how it went."""
import os
import re
import shutil
import subprocess

import pytest

from abi_support import REMARKS, hipcc_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "summersph_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")

VARIANTS = ["density_wtILi1024ELb1E", "density_wtILi1024ELb0E", "forces_qILi1024ELi4ELb1E", "forces_qILi1024ELi4ELb0E",
            "forces_qILi1024ELi8ELb1E", "forces_qILi1024ELi8ELb0E"]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(assembly per kernel, resource report per kernel) of tiled.hip"""
    out = tmp_path_factory.mktemp("knots_cpu") / "tiled.s"
    r = subprocess.run([HIPCC, *hipcc_flags(), "--cuda-device-only", "-S", REMARKS, os.path.join(CSRC, "tiled.hip"), "-o", str(out)],
                       check=True, capture_output=True, text=True, timeout=900)
    asm, name = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            asm[name] = []
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            asm[name].append(line)
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark: .*?\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+) " + re.escape("[" + REMARKS.split("=")[0]), line)
        if m and name is not None:
            usage[name][m.group(1).strip()] = m.group(2)
    return asm, usage


def pick(d, variant):
    keys = [k for k in d if variant in k]
    assert len(keys) == 1, (variant, keys)
    return d[keys[0]]


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v.endswith("Lb1E")])
def test_no_paired_knot_read_in_the_table_kernels(compiled, variant):
    body = pick(compiled[0], variant)
    assert len(body) > 500                                                  # the kernel's text was really found
    paired = [ln for ln in body if re.search(r"\bds_read2_b64\b.*\boffset1:1\s*$", ln.split(";")[0])]
    assert not paired, paired
    assert sum("ds_read_b64" in ln for ln in body) >= 2


@pytest.mark.parametrize("variant", VARIANTS)
def test_pair_kernels_fit_the_register_file(compiled, variant):
    u = pick(compiled[1], variant)
    print(variant, u)
    assert int(u["VGPRs"]) <= 128
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
