#!/usr/bin/env python3
"""Times sph_sample ("SPH interpolation at arbitrary points"); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/sample_time.py N` for the per-kernel times (sample_select ...
sample_walk and the two rocprim radix sorts).

  N          gas particles (default 10^6) of ic.keplerian_disc(N, seed=5) (fixed h = 2.5); --variable:
             ic.keplerian_disc_var(N, seed=5) (each particle's own h); --wide: ic.uniform_box(N) with h log-uniform over
             11 octaves up to half the box edge plus one particle whose 2 h covers the box (the wide-h set of the tests)
  --points M points per set (default 2^20)
  --host     also the host baseline (download + tests/sample_ref.py) on the polar map
  --ab       also the level width (quarter, half, whole octave) and the point sort (on, off), device form
  --fields K fields sampled (default 2: vx, u)

Point sets: M random points in the source box, a 512 x (M / 512) polar map of the midplane, and the nodes of a
256 x 256 x (M / 65536) np.linspace grid over the source box.  Prints one JSON line: wall time per call of the host form
(after one warm-up) and of the device form (synchronised), windows of at least 0.3 s; for the grid the unchanged
sph_render_field 3-D render of the same nodes (device form) and the ratio."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from summersph_amd import capi, ic  # noqa: E402
from summersph_amd import sample as smp  # noqa: E402

FIELDS = ("vx", "u", "vy", "vz")


def timed(fn, sync, window=0.3, min_reps=3):
    """ms per call: one warm-up, then calls until the window is full"""
    fn(); sync()
    reps, t0 = 0, time.perf_counter()
    while reps < min_reps or time.perf_counter() - t0 < window:
        fn()
        reps += 1
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--variable", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--fields", type=int, default=2, choices=range(0, 5))
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--ab", action="store_true")
    a = ap.parse_args()
    variable, wide, n, m, nf = a.variable, a.wide, a.n, a.points, a.fields
    rng = np.random.default_rng(11)
    if wide:
        gas, sinks = ic.split_rows(ic.uniform_box(n))
        edge = float(max(gas[k].max() - gas[k].min() for k in "xyz"))
        gas["h"] = 0.5 * edge * 2.0 ** rng.uniform(-11.0, 0.0, n)
        gas["h"][77] = 1.01 * edge
    else:
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(n, seed=5) if variable else ic.keplerian_disc(n, seed=5))
    per_h = variable or wide
    ctx = capi.Context(device=0, variable=per_h)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    ctx.synchronize()
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    shape = (256, 256, max(m // 65536, 1))
    ax = [np.linspace(lo[k], hi[k], shape[k]) for k in range(3)]
    sets = {"random": rng.uniform(lo, hi, (m, 3)),
            "grid": np.stack([g.ravel() for g in np.meshgrid(*ax, indexing="ij")], axis=1)}
    if not wide:
        r_out = float(np.hypot(pos[:, 0], pos[:, 1]).max())
        sets["polar"] = smp.polar_points(min(30.0, 0.2 * r_out), r_out - min(30.0, 0.2 * r_out), 512, max(m // 512, 1))[0]
    fields = FIELDS[:nf]
    dev = torch.device("cuda", 0)
    out = {"n": ctx.n, "variable": variable, "wide": wide, "fields": list(fields), "points": {k: int(v.shape[0]) for k, v in sets.items()}}
    if per_h:
        out["half_octave_levels"] = int(np.unique(gas["h"].view(np.uint64) >> np.uint64(51)).size)
    for name, pts in sets.items():
        dp = [torch.from_numpy(np.ascontiguousarray(pts[:, k])).to(dev) for k in range(3)]
        out[f"{name}_host_ms"] = timed(lambda: ctx.sample(pts, fields=fields, weight_out=True), ctx.synchronize)
        out[f"{name}_device_ms"] = timed(lambda: ctx.sample(dp, fields=fields, weight_out=True, device=True), ctx.synchronize)
        out[f"{name}_reached"] = ctx.sample(pts, counts=True)[2][0]
        if a.ab:
            for width, wname in ((0, "quarter"), (1, "half"), (2, "octave")) if per_h else ((1, "one"),):
                for psort in (1, 0):
                    os.environ["SPH_SAMPLE_LEVEL_WIDTH"], os.environ["SPH_SAMPLE_POINT_SORT"] = str(width), str(psort)
                    out[f"{name}_device_ms_{wname}_{'sorted' if psort else 'unsorted'}"] = timed(
                        lambda: ctx.sample(dp, fields=fields, weight_out=True, device=True), ctx.synchronize)
            del os.environ["SPH_SAMPLE_LEVEL_WIDTH"], os.environ["SPH_SAMPLE_POINT_SORT"]
        if name == "grid":
            # the yardstick: the unchanged 3-D field render of the same nodes (same sums, LDS-tiled), one field
            out["grid_device_ms_1field"] = timed(lambda: ctx.sample(dp, fields=fields[:1], weight_out=True, device=True), ctx.synchronize)
            out["grid_render_field_device_ms"] = timed(
                lambda: ctx.render_field(fields[0], shape, bounds=(lo, hi), weight_out=True, device=True), ctx.synchronize)
            out["grid_sample_over_render"] = out["grid_device_ms_1field"] / out["grid_render_field_device_ms"]
        del dp
    if a.host and "polar" in sets:
        import sample_ref
        t0 = time.perf_counter()
        p = np.stack([ctx.field("x"), ctx.field("y"), ctx.field("z")], axis=1)
        A = np.stack([ctx.field(f) for f in fields])
        sample_ref.sample(sets["polar"], p, ctx.field("m"), ctx.field("h") if per_h else 2.5, A)
        out.update(host_kind="download + scipy cKDTree + numpy (tests/sample_ref.py), polar map", host_s=time.perf_counter() - t0)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
