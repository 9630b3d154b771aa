#!/usr/bin/env python3
"""Times sph_modes on a Keplerian disc beside the only way to the ring sums without it: cos m phi
and sin m phi for m = 1 .. 8 on the host, uploaded as rows of two sph_binned calls; run it under
`rocprofv3 --kernel-trace --stats -- python profiles/modes_time.py N REPS CASE` in a run of its own, one case per run, for
the per-kernel times (modes_select .. modes_convert), and under `rocprofv3 --kernel-trace --pmc SQ_ACTIVE_INST_VALU
SQ_INSTS_VALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE` for modes_spiral's VALU utilisation.

  N      gas particles of ic.keplerian_disc(N, seed=5) with its sink (default 10^6), after sph_density (cell-sorted order)
  REPS   timed repeats after one warm-up of every shape (default 5)
  CASES  comma-separated: rings (40 log rings, m_max = 8), rings_dev (its device form), spiral (also 129 wavenumbers in
         [-32, 32]), spiral_only (the difference's check: 1 ring), compose (host trigonometry + two sph_binned calls of 8
         uploaded quantity rows and the radius row each, weight m), floor (sph_binned over the same rings with SPH_F_*
         quantities only: the cost of a pass over the particles)   (default: all of them)
  OUT    a file the JSON goes to as well (default "-": only printed; profiles/modes_time.json holds a run's object under
         "wall" beside the kernel tables)

The rings span the 1st to the 99th percentile of the radius about the sink.  compose and floor need only sph_binned, so
the script also runs from a checkout without sph_modes when given those cases alone.  Wall time is a host clock around
calls that end in the host form's own read-back.  Prints (and writes) one JSON object."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402

DEFAULT = "rings,rings_dev,spiral,spiral_only,compose,floor"
N_R, M_MAX, SPIRAL = 40, 8, (-32.0, 32.0, 129)


def timed(fn, reps):
    fn()                                                     # warm-up (scratch, code objects)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    cases = (sys.argv[3] if len(sys.argv) > 3 else DEFAULT).split(",")
    path = sys.argv[4] if len(sys.argv) > 4 else "-"
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density()                                            # the cell-sorted order of a running simulation
    cx, cy = float(sinks["x"][0]), float(sinks["y"][0])
    R = np.hypot(gas["x"] - cx, gas["y"] - cy)
    r_range = (float(np.percentile(R, 1.0)), float(np.percentile(R, 99.0)))
    out = {"n": ctx.n, "reps": reps, "n_rings": N_R, "m_max": M_MAX, "r_range": list(r_range), "p_table": list(SPIRAL)}

    def compose():
        """what a caller does today: the trigonometry on the host, then sph_binned over the radius row"""
        t0 = time.perf_counter()
        phi = np.arctan2(gas["y"] - cy, gas["x"] - cx)
        rows = [np.cos(m * phi) for m in range(1, M_MAX + 1)] + [np.sin(m * phi) for m in range(1, M_MAX + 1)]
        t1 = time.perf_counter()
        res = []
        for half in (rows[:8], rows[8:]):
            values = np.stack(half + [R])
            res.append(ctx.binned(capi.binned_row(8), N_R, ranges=r_range, log=(0,), q=[capi.binned_row(k) for k in range(8)],
                                  weight="mass", values=values)[0])
        compose.host_ms.append((t1 - t0) * 1e3)
        return res
    compose.host_ms = []

    for case in cases:
        if case == "compose":
            r = timed(compose, reps)
            r["host_trig_ms_mean"] = float(np.mean(compose.host_ms[1:]))
        elif case == "floor":
            r = timed(lambda: ctx.binned("x", N_R, ranges=(-r_range[1], r_range[1]), q=("u", "vx", "vy", "vz", "rho", "P", "c", "alpha"),
                                         weight="mass"), reps)
        elif case == "rings":
            r = timed(lambda: ctx.modes(r_range, N_R, M_MAX, log=True, sink=0), reps)
            r["selected"] = ctx.modes(r_range, N_R, M_MAX, log=True, sink=0)[3][0]
        elif case == "rings_dev":
            import torch

            def dev():
                ctx.modes(r_range, N_R, M_MAX, log=True, sink=0, device=True)
                torch.cuda.synchronize()
            r = timed(dev, reps)
        elif case in ("spiral", "spiral_only"):
            n_r = N_R if case == "spiral" else 1
            r = timed(lambda: ctx.modes(r_range, n_r, M_MAX, log=True, sink=0, spiral=SPIRAL, r_ref=r_range[0]), reps)
            sel = ctx.modes(r_range, n_r, M_MAX, log=True, sink=0, spiral=SPIRAL, r_ref=r_range[0])[3][0]
            r["selected"] = sel
            r["terms"] = sel * (M_MAX + 1) * SPIRAL[2]                # (particle, m, p) terms, a cosine and a sine sum each
            r["terms_per_s"] = r["terms"] / (r["mean_ms"] * 1e-3)
        else:
            raise SystemExit(f"unknown case {case!r}")
        out[case] = r
    if "rings" in cases and "compose" in cases:
        out["rings_over_compose"] = out["rings"]["mean_ms"] / out["compose"]["mean_ms"]
    ctx.close()
    print(json.dumps(out))
    if path != "-":
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
