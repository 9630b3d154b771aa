"""The call-order state machine of csrc/ctx_state.hpp, walked on the CPU.

tests/tools/ctx_state_walk.cpp includes nothing but that header (no HIP).  Built here with AddressSanitizer and UBSan, it
visits every state that any sequence of the header's transitions and of the evaluation steps can reach from a fresh
context -- fixed / variable h, with and without self-gravity -- and checks after every step
    eos_valid => rho_valid => grid_valid => order_valid,   h_refresh_ok => !grid_valid,   keys_early => !order_valid,
    nl_overflowed => no evaluation stands,
    interior_done && grid_valid => no grid build since part 1,   grav_valid && grid_valid => tree_valid
(the last two in the form today's rules obey: DESIGN.md, "The context's state"), and field_ready against the table in its
comment for every field."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="g++ is not installed")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ctx_state") / "ctx_state_walk")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "tools", "ctx_state_walk.cpp")], check=True)
    return exe


def test_every_reachable_state_obeys_the_invariants(walker):
    r = subprocess.run([walker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("states "), r.stdout
    assert int(r.stdout.split()[1].rstrip(",")) > 1000          # the walk went somewhere: all four configurations


def test_a_bounded_walk_ends_early(walker):
    """the depth argument bounds the sequences (the full walk is a fixed point a few dozen steps deep)"""
    r = subprocess.run([walker, "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[1].rstrip(",")) < 1000
