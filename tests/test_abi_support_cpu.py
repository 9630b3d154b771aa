"""CPU tests of tests/abi_support.py itself: the remark parser on recorded hipcc output, the compile flags against what the
Makefile runs, and the once-per-source compile."""
import os
import shutil
import subprocess
import types

import pytest

import abi_support as A

# hipcc's remarks for energy.hip (gfx950), two kernels of four, with the source echo hipcc prints after a header
RECORDED = """\
energy.hip:40:1: remark: Function Name: _ZN3sph12_GLOBAL__N_112energy_stageEPKdS2_S2_S2_PKilP15HIP_vector_typeIdLj4EEPd [-Rpass-analysis=kernel-resource-usage]
   40 |                                                    double *__restrict__ box_part) {
      | ^
energy.hip:40:1: remark:     TotalSGPRs: 32 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     VGPRs: 36 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:40:1: remark:     LDS Size [bytes/block]: 12288 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark: Function Name: _ZN3sph12_GLOBAL__N_110energy_boxEPKdiPd [-Rpass-analysis=kernel-resource-usage]
   67 | __global__ __launch_bounds__(WAVE) void energy_box(const double *__restrict__ box_part, int nb, double *__restrict__ out) {
      | ^
energy.hip:67:1: remark:     TotalSGPRs: 15 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     VGPRs: 28 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
energy.hip:67:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""
STAGE = "_ZN3sph12_GLOBAL__N_112energy_stageEPKdS2_S2_S2_PKilP15HIP_vector_typeIdLj4EEPd"
BOX = "_ZN3sph12_GLOBAL__N_110energy_boxEPKdiPd"


def test_parser_on_recorded_remarks():
    k = A.parse_remarks(RECORDED, A.containing("energy_stage"))
    assert list(k) == [STAGE]                                     # energy_box is rejected, with every remark below it
    # the bracketed suffix is dropped from the name; "Dynamic Stack: False" is no integer and is left out
    assert k[STAGE] == {"TotalSGPRs": 32, "VGPRs": 36, "AGPRs": 0, "ScratchSize": 0, "Occupancy": 8, "SGPRs Spill": 0,
                        "VGPRs Spill": 0, "LDS Size": 12288}
    both = A.parse_remarks(RECORDED, A.containing("energy_stage", "energy_box"))
    assert list(both) == [STAGE, BOX] and both[STAGE] == k[STAGE]
    assert both[BOX]["VGPRs"] == 28 and both[BOX]["LDS Size"] == 0
    assert A.parse_remarks(RECORDED, lambda name: name.endswith("iPd")) == {BOX: both[BOX]}
    assert A.parse_remarks(RECORDED, A.containing("groups_")) == {}


@pytest.mark.skipif(shutil.which("make") is None, reason="needs make")
def test_flags_are_the_makefile_s():
    flags = A.hipcc_flags()
    for f in ("--offload-arch=gfx950", "-O3", "-fno-gpu-rdc"):
        assert f in flags, f
    env = {k: v for k, v in os.environ.items() if k not in ("CXXFLAGS", "ARCH", "HIPCC", "MAKEFLAGS")}
    out = subprocess.run(["make", "-n", "-B", "-C", A.CSRC, "groups.o"], check=True, capture_output=True, text=True, env=env).stdout
    lines = [ln for ln in out.splitlines() if "-c groups.hip" in ln]
    assert len(lines) == 1, out
    assert lines[0].split() == [A.HIPCC, *flags, "-c", "groups.hip", "-o", "groups.o"]


def test_a_source_is_compiled_once(monkeypatch):
    calls = []

    def fake_run(cmd, **kw):
        calls.append(cmd)
        return types.SimpleNamespace(stderr=RECORDED)

    monkeypatch.setattr(A.subprocess, "run", fake_run)
    # source names no budget test asks for: the canned text stays in the cache under them, the real compiles stay too
    one, other = f"canned_{id(calls)}.hip", f"canned_{id(calls)}_b.hip"
    a = A.resource_usage(one, A.containing("energy_stage"))
    b = A.resource_usage(one, A.containing("energy_box"))
    assert len(calls) == 1 and list(a) == [STAGE] and list(b) == [BOX]
    assert calls[0] == [A.HIPCC, *A.hipcc_flags(), "-c", one, "-o", os.devnull, A.REMARKS]
    A.resource_usage(other, A.containing("energy_"))
    assert len(calls) == 2
