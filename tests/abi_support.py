"""What the CPU tests of the ABI and of the compiler's output share: the paths and skip marks, the library's own compile
flags, the kernel-resource-usage remarks of a source file, the C program that prints a struct's layout, and the Fortran
link check.  Plain functions, imported by name; each test keeps its own assertions."""
import functools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

FC = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "summersph_amd", "csrc")
BINDING = os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")
LIB = os.path.join(ROOT, "summersph_amd", "libsummersph_hip.so")
REMARKS = "-Rpass-analysis=kernel-resource-usage"

needs_fc = pytest.mark.skipif(not os.path.exists(FC), reason="needs amdflang")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def library():
    """The path of the built library; builds it first where it is missing."""
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.DEVNULL)
    return LIB


@functools.lru_cache(maxsize=None)
def hipcc_flags():
    """The flags the library's objects are compiled with: the Makefile's CXXFLAGS with $(ARCH) put in, as a tuple."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= *(\S+)", text, re.M).group(1)
    return tuple(re.search(r"^CXXFLAGS \?= *(.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split())


@functools.lru_cache(maxsize=None)
def _remarks(src):
    """hipcc's remark text for one source file of csrc, compiled once per process"""
    return subprocess.run([HIPCC, *hipcc_flags(), "-c", src, "-o", os.devnull, REMARKS],
                          cwd=CSRC, check=True, capture_output=True, text=True).stderr


def parse_remarks(out, pick):
    """{kernel: {remark: int}} of the functions whose mangled name `pick` accepts"""
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


def containing(*subs):
    """A `pick` for resource_usage: the name contains any of these substrings."""
    return lambda name: any(s in name for s in subs)


def resource_usage(src, pick):
    """{kernel: {remark: int}} for the kernels of csrc/<src> that `pick` accepts, compiled with the library's own flags"""
    return parse_remarks(_remarks(src), pick)


def c_layout(tmp_path, struct, fields, extra_printf=()):
    """Compiles a C program against include/summersph.h that prints `size`, each field's offset and the statements of
    extra_printf, one `name value` line each, and returns {name: value} with the values as text."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "summersph.h"\nint main(void) {\n'
                   f'  printf("size %zu\\n", sizeof({struct}));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof({struct}, {f}));\n' for f in fields) +
                   "".join(f"  {s}\n" for s in extra_printf) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())


def fortran_links(tmp_path, name, program_text):
    """Writes <name>.f90, compiles and links it with the Fortran binding against the library; returns the executable."""
    lib = library()
    caller = tmp_path / f"{name}.f90"
    caller.write_text(program_text)
    exe = tmp_path / name
    subprocess.run([FC, "-O1", f"-J{tmp_path}", BINDING, str(caller), "-L" + os.path.dirname(lib), "-lsummersph_hip",
                    "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)], check=True, cwd=tmp_path, stdout=subprocess.DEVNULL)
    assert exe.exists()
    return exe
