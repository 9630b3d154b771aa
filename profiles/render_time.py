#!/usr/bin/env python3
"""Times sph_render_density on the three configurations of DESIGN.md ("Density rendering"); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/render_time.py CASE` for the per-kernel times.

  a   the script's settings: 12 000-particle disc (ic.keplerian_disc(12000, seed=214) without the sink and the dropped
      row), 120^3 nodes, h = 1.25, sums along z
  b   10^6-particle variable-h disc after one h update, 1024 x 1024 x 64 nodes, z sums, per-particle h, auto bounds
  c   the same disc, 256^3 3-D grid, per-particle h

Prints one JSON line: wall time per render (after one warm-up, host form, i.e. including the two read-backs and the
output copy) and the candidate efficiency of the gather (pairs within 2h / pairs the lanes tested), the latter from a
numpy replica of the render's binning (render.hip: the grid sizing, the bricks of TU x TV x KW nodes, the cells each
brick stages; RENDER_TILE in the environment for an A/B build of another tile) and an estimate of the contributing pairs (each particle's 2h-ball volume over the node cell volume)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic, render  # noqa: E402

TU = TV = int(os.environ.get("RENDER_TILE", "8"))     # render.hip's tile (A/B builds: RENDER_TILE=16)
KW = 8
MAX_CELLS = 1 << 26


def efficiency(pos, h, lo, hi, n, axis):
    """contributing / tested node-particle pairs of one render, from a replica of render.hip's binning"""
    n = np.asarray(n)
    hmax = float(h.max())
    reach = 2.0 * hmax * (1.0 + 1e-6)
    org = lo - reach
    ext = (hi + reach) - org
    edge = 2.0 * hmax
    while np.prod(np.maximum(1.0, np.ceil(ext / edge))) > MAX_CELLS:
        edge *= 1.2599210498948732
    dim = np.maximum(1, np.ceil(ext / edge)).astype(np.int64)
    near = np.all((pos >= lo - 2 * h[:, None] * (1 + 1e-6)) & (pos <= hi + 2 * h[:, None] * (1 + 1e-6)), axis=1)
    c = np.clip(np.floor((pos[near] - org) / edge), 0, dim - 1).astype(np.int64)
    cnt = np.zeros(dim, dtype=np.int64)
    np.add.at(cnt, (c[:, 0], c[:, 1], c[:, 2]), 1)
    pre = np.zeros(dim + 1, dtype=np.int64)
    pre[1:, 1:, 1:] = cnt.cumsum(0).cumsum(1).cumsum(2)
    W = 0 if axis is None else axis
    U, V = [a for a in range(3) if a != W]
    step = np.where(n > 1, (hi - lo) / np.maximum(n - 1, 1), 0.0)

    def coord(a, i):
        return np.where(i >= n[a] - 1, hi[a], i * step[a] + lo[a])

    def cells(a, x):
        return np.clip(np.floor((x - org[a]) / edge), 0, dim[a] - 1).astype(np.int64)

    rng = {}
    for a, blk in ((W, KW), (U, TU), (V, TV)):
        i0 = np.arange(0, n[a], blk)
        i1 = np.minimum(n[a], i0 + blk) - 1
        rng[a] = (cells(a, coord(a, i0) - reach), cells(a, coord(a, i1) + reach) + 1)
    lo0, hi0 = rng[0]; lo1, hi1 = rng[1]; lo2, hi2 = rng[2]
    A = lo0[:, None, None], hi0[:, None, None]
    B = lo1[None, :, None], hi1[None, :, None]
    Cc = lo2[None, None, :], hi2[None, None, :]
    box = (pre[A[1], B[1], Cc[1]] - pre[A[0], B[1], Cc[1]] - pre[A[1], B[0], Cc[1]] - pre[A[1], B[1], Cc[0]]
           + pre[A[0], B[0], Cc[1]] + pre[A[0], B[1], Cc[0]] + pre[A[1], B[0], Cc[0]] - pre[A[0], B[0], Cc[0]])
    tested = float(box.sum()) * TU * TV * KW
    cell_vol = np.prod(np.where(n > 1, step, 1.0))
    contributing = float(np.sum(4.0 / 3.0 * np.pi * (2.0 * h[near]) ** 3) / cell_vol) if np.all(n > 1) else float("nan")
    return contributing, tested


def main():
    case = sys.argv[1] if len(sys.argv) > 1 else "a"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if case == "a":
        gas, _ = ic.split_rows(ic.keplerian_disc(12000, seed=214))
        rows = np.column_stack([gas[k] for k in "x y z vx vy vz u m".split()] + [np.zeros(gas["x"].size)])
        rows = render.script_rows(rows)
        ctx = capi.Context(device=0)
        ctx.upload({k: rows[:, i] for i, k in enumerate("x y z vx vy vz u m alpha".split())})
        kw = dict(shape=120, axis="z", h=1.25, clip=((-100.0,) * 3, (100.0,) * 3))
    else:
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(1_000_000, seed=99))
        ctx = capi.Context(device=0, variable=True)
        ctx.upload(gas); ctx.set_sinks(sinks)
        ctx.density(); ctx.update_h()
        kw = dict(shape=(1024, 1024, 64), axis="z") if case == "b" else dict(shape=256)
    img = ctx.render_density(**kw)                      # warm-up (scratch allocation, code objects)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        img = ctx.render_density(**kw)
    wall = (time.perf_counter() - t0) / reps
    lo, hi = ctx.render_bounds
    pos = np.stack([ctx.field(k) for k in "xyz"], axis=1)
    h = np.full(pos.shape[0], 1.25) if case == "a" else ctx.field("h")
    shape = (kw["shape"],) * 3 if np.isscalar(kw["shape"]) else kw["shape"]
    contributing, tested = efficiency(pos, h, lo, hi, shape, 2 if kw.get("axis") == "z" else None)
    print(json.dumps({"case": case, "n": int(pos.shape[0]), "shape": list(shape), "axis": kw.get("axis"),
                      "wall_ms_per_render": wall * 1e3, "image_max": float(img.max()),
                      "pairs_contributing_est": contributing, "pairs_tested": tested,
                      "candidate_efficiency": contributing / tested}))
    ctx.close()


if __name__ == "__main__":
    main()
