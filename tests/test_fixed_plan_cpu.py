"""The fixed-h step's host decisions (csrc/fixed_plan.hpp) and the A/B switches' parsers (csrc/switches.hpp) on the CPU.

tests/tools/fixed_plan_check.cpp includes nothing but those two headers (no HIP, no context).  Built here with
AddressSanitizer and UBSan, it checks against values written out in the program
    judge_list        what a neighbour-list report means at each of its three ages: fits, regrows (and to what), leaves the
                      tiled path, overflowed, outgrew the 16-bit entries -- at 72 / 73 / 96 / 97 of a capacity of 96 and at
                      needs of 32767 / 32768 / 65535 / 65536, and the precedence among them,
    choose_tiles      the tile verdict at n = 1 .. 10240, one misfit below, at and above each nine-in-ten limit: table against
                      table-free, full against half groups, the two forcing switches, the percentages,
    use_tile_kernel   the groups-per-CU thresholds of density_wt (groups of 1024) and forces_q (groups of 256),
    riders_allowed / ride_final   every single disqualifier,
    the parsers       presence, integer with a default, clamped integer, flag, string equality; unset, empty, "0", junk, and
                      that the once-per-process switches are read once."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ is not installed")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fixed_plan") / "fixed_plan_check")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "tools", "fixed_plan_check.cpp")], check=True)
    return exe


def test_every_rule_at_its_edges(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checks "), r.stdout
    checks, failures = (int(w.rstrip(",")) for w in r.stdout.split()[1::2])
    assert failures == 0 and checks > 250, r.stdout         # every group of checks ran


def test_the_headers_compile_alone():
    """no HIP and no context behind either header: each is a translation unit of its own for the host compiler"""
    for name in ("fixed_plan.hpp", "switches.hpp"):
        subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                       input='#include "%s"\n' % os.path.join(ROOT, "summersph_amd", "csrc", name))
