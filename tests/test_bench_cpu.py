"""bench.py's --dump-outputs writer and argument checks, without a GPU: a stub context stands in for capi.Context."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 64_000_000          # the whole dump stays below 64 MB


class StubCtx:
    """what dump_outputs reads of a context: n, field(name), get_sinks()"""

    def __init__(self, n, ns=1):
        self.n, self.ns = n, ns

    def field(self, name):
        return np.arange(self.n, dtype=np.float64) * (1.0 + len(name)) + 0.25

    def get_sinks(self):
        return {c: np.full(self.ns, float(i)) for i, c in enumerate(bench.SINK_COLUMNS)}


def _files(d):
    return {f: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("variable", [False, True])
def test_dump_stays_below_64mb_float64_and_samples_rows(tmp_path, variable):
    n = 1_000_000                                   # the headline size: above the budget in both modes
    ctx = StubCtx(n)
    shapes = bench.dump_outputs(ctx, 1.5e-2, 0.75, variable, str(tmp_path))
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert total < LIMIT, total
    got = _files(tmp_path)
    assert set(shapes) == {f[:-4] for f in got}
    assert all(a.dtype == np.float64 for a in got.values())
    idx = got["sample_index.npy"]
    k = idx.size
    assert 0 < k < n and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n and np.all(idx == np.round(idx))
    for name in "x y z vx vy vz u alpha rho ax ay az du".split() + (["h", "omega"] if variable else []):
        assert np.array_equal(got[name + ".npy"], ctx.field(name)[idx.astype(np.int64)]), name
    assert got["n_particles.npy"].tolist() == [n]
    assert got["dt_t.npy"].tolist() == [1.5e-2, 0.75]
    assert got["sinks.npy"].shape == (1, len(bench.SINK_COLUMNS))


def test_dump_sample_is_seeded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(StubCtx(100_000), 1e-2, 0.0, False, str(a))
    bench.dump_outputs(StubCtx(100_000), 1e-2, 0.0, False, str(b))
    fa, fb = _files(a), _files(b)
    assert fa.keys() == fb.keys()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa)
    assert fa["sample_index.npy"].size < 100_000


def test_dump_below_budget_keeps_every_row(tmp_path):
    ctx = StubCtx(5000, ns=0)
    bench.dump_outputs(ctx, 1e-2, 0.0, False, str(tmp_path))
    got = _files(tmp_path)
    assert np.array_equal(got["sample_index.npy"], np.arange(5000.0))
    assert np.array_equal(got["x.npy"], ctx.field("x"))
    assert got["n_particles.npy"].tolist() == [5000]
    assert got["sinks.npy"].shape == (0, len(bench.SINK_COLUMNS))


@pytest.mark.parametrize("argv,env,msg", [
    (["--steps", "0"], {}, "--steps must be >= 1"),
    (["--dump-outputs", "never_written"], {"WORLD_SIZE": "2"}, "--dump-outputs needs a single-GPU run"),
])
def test_bench_rejects_bad_arguments_before_touching_a_gpu(tmp_path, argv, env, msg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True,
                       cwd=tmp_path, env={**os.environ, **env}, timeout=120)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "never_written").exists()
