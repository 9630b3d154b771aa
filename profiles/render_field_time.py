#!/usr/bin/env python3
"""Times sph_render_field against sph_render_density on the same nodes, for the three configurations of DESIGN.md
("Field rendering"); run it under `rocprofv3 --kernel-trace --stats -- python profiles/render_field_time.py CASE` for the
per-kernel times (field_gather<W, DEN> against render_gather<W>).

  a   the script's settings: 12 000-particle disc (ic.keplerian_disc(12000, seed=214) without the sink and the dropped
      row), 120^3 nodes, h = 1.25, sums along z; mass-weighted u, normalised
  b   10^6-particle variable-h disc after one h update, 1024 x 64 x 1024 nodes projected along y (edge-on), per-particle
      h, auto bounds; mass-weighted vy, normalised (a moment-1 map)
  c   the same disc, 256^3 3-D grid, per-particle h; volume-weighted u, normalised (the Shepard interpolant)

Prints one JSON line: wall time per render of each kind (after one warm-up each, host form, i.e. including the two
read-backs and the output copies)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic, render  # noqa: E402


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
        fkw = dict(field="u", weight="mass", normalise=True)
    else:
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(1_000_000, seed=99))
        ctx = capi.Context(device=0, variable=True)
        ctx.upload(gas); ctx.set_sinks(sinks)
        ctx.density(); ctx.update_h(); ctx.density()     # rho of the current h (the volume weight of case c)
        if case == "b":
            kw = dict(shape=(1024, 64, 1024), axis="y")
            fkw = dict(field="vy", weight="mass", normalise=True)
        else:
            kw = dict(shape=256)
            fkw = dict(field="u", weight="volume", normalise=True)
    wall = {}
    for kind in ("density", "field"):
        def run():
            return ctx.render_density(**kw) if kind == "density" else ctx.render_field(fkw["field"], **kw, weight=fkw["weight"],
                                                                                         normalise=fkw["normalise"])
        img = run()                                         # warm-up (scratch allocation, code objects)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            img = run()
        wall[kind] = (time.perf_counter() - t0) / reps
        assert np.all(np.isfinite(img)) and img.any()
    shape = (kw["shape"],) * 3 if np.isscalar(kw["shape"]) else kw["shape"]
    print(json.dumps({"case": case, "n": ctx.n, "shape": list(shape), "axis": kw.get("axis"), **fkw,
                      "density_wall_ms_per_render": wall["density"] * 1e3, "field_wall_ms_per_render": wall["field"] * 1e3,
                      "field_over_density_wall": wall["field"] / wall["density"]}))
    ctx.close()


if __name__ == "__main__":
    main()
