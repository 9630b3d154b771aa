#!/usr/bin/env python3
"""Times sph_groups on a Keplerian disc ("Friends-of-friends groups"); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/groups_time.py N` for the per-kernel times (groups_select ...
groups_final and the three rocprim radix sorts).

  N      gas particles of ic.keplerian_disc(N, seed=5) (default 10^6); fixed h = 2.5, plain FoF with b = h
  REPS   timed calls (default 3)
  --one-cell  instead: N particles in a unit cube with b = 10 (one cell holds everything: every pair is tested)

Prints one JSON line: wall time per call of the host form (labels + the 100 largest groups, after one warm-up) and of the
device form (synchronised), the group count, and the host baseline: download the fields, then scipy's cKDTree pair
search and connected components where scipy exists, else the numpy restatement tests/groups_ref.py."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from summersph_amd import capi, ic  # noqa: E402


def host_baseline(ctx, link):
    t0 = time.perf_counter()
    x, y, z = ctx.field("x"), ctx.field("y"), ctx.field("z")
    pos = np.stack([x, y, z], axis=1)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
        kind = "scipy cKDTree + connected_components"
        pairs = cKDTree(pos).query_pairs(link, output_type="ndarray")
        g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(x), len(x)))
        nc = connected_components(g, directed=False)[0]
    except ImportError:
        import groups_ref
        kind = "numpy restatement (tests/groups_ref.py)"
        nc = np.unique(groups_ref.components(len(x), groups_ref.link_pairs(pos, np.zeros(len(x)), link))).size
    return {"host_kind": kind, "host_s": time.perf_counter() - t0, "host_components": int(nc)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    one_cell = "--one-cell" in sys.argv
    n = int(args[0]) if args else 1_000_000
    reps = int(args[1]) if len(args) > 1 else 3
    if one_cell:
        rng = np.random.default_rng(5)
        p = rng.uniform(0, 1, (n, 3))
        gas = {"x": p[:, 0], "y": p[:, 1], "z": p[:, 2], "vx": np.zeros(n), "vy": np.zeros(n), "vz": np.zeros(n),
               "u": np.full(n, 0.1), "m": np.full(n, 1e-6), "alpha": np.ones(n)}
        sinks, link = None, 10.0
    else:
        gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
        link = 2.5
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    if sinks is not None:
        ctx.set_sinks(sinks)
    ctx.density()                                            # rho, and the cell-sorted order of a running simulation
    ctx.synchronize()
    out = {"n": ctx.n, "link": link, "one_cell": one_cell}
    ctx.groups(link, max_groups=100)                         # warm-up (scratch, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        lab, tab, ng = ctx.groups(link, max_groups=100)
    out["host_ms"] = (time.perf_counter() - t0) / reps * 1e3
    ctx.groups(link, max_groups=100, device=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.groups(link, max_groups=100, device=True)
    ctx.synchronize()
    out["device_ms"] = (time.perf_counter() - t0) / reps * 1e3
    out.update({"n_groups": ng, "largest": int(tab["N"][0]) if ng else 0, "in_groups_ge_2": int(np.sum(np.bincount(lab[lab >= 0]) >= 2))})
    if not one_cell:
        out.update(host_baseline(ctx, link))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
