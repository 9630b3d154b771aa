"""bench.py end to end on a small disc: what a plain run carries and what only --full adds, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--particles", "20000", "--steps", "3", "--warmup", "1"]
FULL_ONLY = ("ring4m_strong", "full_1e7", "variable_h", "full_simulate", "side_records", "fixed_reuse_density", "cpu_baseline")


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *argv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only():
    out = _bench()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["repeat_ms_per_step"] is None
    assert list(out["kernel_ms_per_step"]) == ["forces"]
    assert "stream_copy_GBs" not in out["roofline"]
    assert not any(k in out for k in FULL_ONLY)


@pytest.mark.gpu
def test_full_adds_repeats_kernel_table_and_stream_copy():
    out = _bench("--full", "--no-cpu", "--no-variable", "--no-extras")
    assert len(out["repeat_ms_per_step"]) == 3
    assert {"grid", "nlist", "density", "forces", "kick", "dt"} <= set(out["kernel_ms_per_step"])
    assert out["roofline"]["stream_copy_GBs"] > 0


@pytest.mark.gpu
def test_dump_outputs_are_reproducible(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    _bench("--dump-outputs", str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {n[:-4] for n in names} == set(a["dump_outputs"]["arrays"])
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.all(np.isfinite(x)), n
        assert np.array_equal(x, y), n
    assert np.load(tmp_path / "a" / "n_particles.npy").tolist() == [20000]
    assert np.load(tmp_path / "a" / "x.npy").size == 20000
    assert np.load(tmp_path / "a" / "dt_t.npy")[0] == a["final_dt"]


@pytest.mark.gpu
def test_dump_outputs_after_accretion_and_cull(tmp_path):
    out = _bench("--full-simulate", "--dump-outputs", str(tmp_path))
    n = int(np.load(tmp_path / "n_particles.npy")[0])
    assert 0 < n <= 20000
    assert np.load(tmp_path / "x.npy").size == n == np.load(tmp_path / "sample_index.npy").size
    assert np.load(tmp_path / "dt_t.npy")[0] == out["final_dt"]
