#!/usr/bin/env python3
"""Times sph_trace_dev on a Keplerian disc beside the only other way to get the same lines: a host
loop of 4 S sph_sample_dev calls per S RK4 steps joined by torch arithmetic, every call rebuilding the search structure
and sorting the points again.  Run `rocprofv3 --kernel-trace --stats -- python profiles/trace_time.py N 1 kernels` in a run
of its own for the per-kernel times (the sample_* build kernels, the rocprim sorts, trace_seed_keys, trace_walk).

  N     gas particles of ic.keplerian_disc(N, seed=5) / ic.keplerian_disc_var(N, seed=5) with the sink (default 10^6)
  REPS  timed repeats of every case and route, interleaved (default 5)
  MODE  "both" (default), "trace" (no yardstick) or "kernels" (every case's trace once, nothing timed: for the profiler)

Cases: fixed h and the particles' own h; 10^3 seeds x 16 steps, 10^3 seeds x 200 steps, 10^6 seeds x 16 steps.  The seeds
are particle positions + N(0, 0.1), the field is the velocity, SPH_TRACE_ARCLENGTH with ds = 0.25, so that nearly every
line runs all its steps.  The yardstick takes the same steps without any of the stops (no test for den == 0, no NaN rows):
it does less than sph_trace, never more.

Every time is a host clock around a window of calls on the context's stream that ends in sph_synchronize; a window holds
as many calls as fill 0.3 s (at least one).  Prints one JSON line: per case the minimum and maximum over REPS of the
per-call time of both routes in ms, the windows' call counts and the status counts of the lines."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402

WINDOW_S = 0.3
DS = 0.25
FIELDS = ("vx", "vy", "vz")


def window(fn, sync, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def calls_for(fn, sync):
    """a warm-up (scratch, code objects), then the number of calls that fill a window"""
    fn(); sync()
    one = window(fn, sync, 1)
    return max(1, int(math.ceil(WINDOW_S * 1e3 / one)))


def host_loop(ctx, seeds, n_steps, ds):
    """the yardstick: RK4 through 4 n_steps Context.sample(device=True) calls; returns the end points"""
    import torch
    hs, s6 = 0.5 * ds, ds / 6.0

    def v(q):
        w = ctx.sample(q, fields=FIELDS, normalise=True, device=True)
        return (w / torch.sqrt((w * w).sum(dim=0, keepdim=True))).T

    p = seeds
    for _ in range(n_steps):
        k1 = v(p)
        k2 = v(p + hs * k1)
        k3 = v(p + hs * k2)
        k4 = v(p + ds * k3)
        p = p + s6 * ((k1 + 2.0 * k2) + (2.0 * k3 + k4))
    return p


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    mode = sys.argv[3] if len(sys.argv) > 3 else "both"
    dev = torch.device("cuda", 0)
    res = {"n": n, "reps": reps, "ds": DS, "window_s": WINDOW_S, "cases": []}
    for variable in (False, True):
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(n, seed=5) if variable else ic.keplerian_disc(n, seed=5))
        ctx = capi.Context(device=0, variable=variable)
        ctx.upload(gas); ctx.set_sinks(sinks)
        ctx.density()                                        # the cell-sorted order of a running simulation
        if variable:
            ctx.upload_field("h", gas["h"])
        pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
        rng = np.random.default_rng(7)
        for m, n_steps in ((1000, 16), (1000, 200), (1_000_000, 16)):
            seeds = torch.from_numpy(pos[rng.choice(n, m, replace=m > n)] + rng.normal(scale=0.1, size=(m, 3))).to(dev)
            cols = [seeds[:, a].contiguous() for a in range(3)]
            out = {}

            def trace():
                out["r"] = ctx.trace(cols, n_steps, DS, arclength=True, device=True, counts=mode == "kernels")

            def loop():
                out["p"] = host_loop(ctx, seeds, n_steps, DS)

            def sync():
                ctx.synchronize()
                torch.cuda.synchronize(dev)
            case = {"h": "own" if variable else "fixed", "n_seeds": m, "n_steps": n_steps}
            if mode == "kernels":
                trace(); sync()
                case["status_counts"] = list(out["r"][3])
                res["cases"].append(case)
                continue
            routes = [("trace", trace)] + ([("sample_loop", loop)] if mode == "both" else [])
            calls = {name: calls_for(fn, sync) for name, fn in routes}
            times = {name: [] for name, _ in routes}
            for _ in range(reps):                            # interleaved: one window of each route per repeat
                for name, fn in routes:
                    times[name].append(window(fn, sync, calls[name]))
            for name, _ in routes:
                case[name] = {"min_ms": float(np.min(times[name])), "max_ms": float(np.max(times[name])), "calls_per_window": calls[name]}
            status = out["r"][1].cpu().numpy()
            case["status_counts"] = [int(v) for v in np.bincount(status, minlength=5)]
            if mode == "both":                               # the two routes end in the same places where the line finished
                end = out["r"][0][-1].T.cpu().numpy()
                fin = status == capi.TRACE_DONE
                case["max_abs_end_difference"] = float(np.max(np.abs(end[fin] - out["p"].cpu().numpy()[fin])))
                case["speedup_min_over_max"] = case["sample_loop"]["min_ms"] / case["trace"]["max_ms"]
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
