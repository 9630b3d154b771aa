"""Dense vs hashed cell table (SPH_FLAG_HASHED_GRID), ms per step, and the grid / list build time of each (HIP events).

    python profiles/hashed_grid_time.py [--n 1000000] [--steps 10] [--out FILE.json]

Runs: the 1e6-particle bench disc with fixed h and with variable h, each with the dense table (the default) and the forced
hashed one; then two 5e5-particle discs 1e4 AU apart on every axis in one context (hashed because the dense table cannot
hold that box) next to one such disc alone.  Per-kernel device times: add `rocprofv3 --kernel-trace --stats -- python ...`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from summersph_amd import capi, ic  # noqa: E402


def run(gas, sinks, flags, variable, steps, warmup=2):
    p = capi.default_params(variable)
    p.flags |= flags
    ctx = capi.Context(params=p, device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    dt, t = 1e-3, 0.0
    for _ in range(warmup):
        dt, t = ctx.step(dt, t)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dt, t = ctx.step(dt, t)
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    # the builds alone, bracketed by events, in a second pass of the same length
    ctx.timing(True, only=["grid", "nlist"])
    ctx.timing_reset()
    for _ in range(steps):
        dt, t = ctx.step(dt, t)
    ctx.synchronize()
    g_ms, g_n = ctx.timing_get("grid")
    l_ms, l_n = ctx.timing_get("nlist")
    gi = ctx.grid_info()
    rec = {"ms_per_step": round(ms, 4), "grid_ms": round(g_ms / max(g_n, 1), 4), "nlist_ms": round(l_ms / max(l_n, 1), 4),
           "kind": gi.kind, "dim": list(gi.dim), "occupied_cells": gi.occupied_cells, "table_entries": gi.table_entries,
           "table_bytes": gi.bytes, "host_syncs": ctx.stats().host_syncs}
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {}
    gas, sinks = ic.split_rows(ic.keplerian_disc(a.n, nngb=85.0))
    for name, fl in (("fixed_dense", 0), ("fixed_hashed", capi.FLAG_HASHED_GRID)):
        res[name] = run(gas, sinks, fl, False, a.steps)
        print(name, res[name], flush=True)
    gv, sv = ic.split_rows(ic.keplerian_disc_var(a.n))
    for name, fl in (("variable_dense", 0), ("variable_hashed", capi.FLAG_HASHED_GRID)):
        res[name] = run(gv, sv, fl, True, a.steps)
        print(name, res[name], flush=True)
    g1, s1 = ic.split_rows(ic.keplerian_disc(a.n // 2, nngb=85.0))
    g2 = {k: v.copy() for k, v in g1.items()}
    s2 = {k: v.copy() for k, v in s1.items()}
    for ax in "xyz":
        g2[ax] = g2[ax] + 1.0e4
        s2[ax] = s2[ax] + 1.0e4
    both = {k: np.concatenate([g1[k], g2[k]]) for k in g1}
    sb = {k: np.concatenate([s1[k], s2[k]]) for k in s1 if k in s2}
    res["far_pair_hashed"] = run(both, sb, 0, False, a.steps)
    print("far_pair_hashed", res["far_pair_hashed"], flush=True)
    res["one_disc_of_the_pair_dense"] = run(g1, sb, 0, False, a.steps)
    print("one_disc_of_the_pair_dense", res["one_disc_of_the_pair_dense"], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
