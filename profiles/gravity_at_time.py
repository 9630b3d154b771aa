#!/usr/bin/env python3
"""Times sph_gravity_at on a Keplerian disc ("Gravity at arbitrary points"); run it under
`rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/gravity_at_time.py N M` for the per-kernel times
(the staging and the tree build over the staged records, gravat_point_keys and its radix sort, grav_field_points,
gravat_finish) next to sph_energy's grav_potential_wave on the same snapshot.

  N   gas particles of ic.keplerian_disc(N, seed=5, m_disc=0.5) with its sink (default 10^6); fixed h, theta 0.5
  M   points of a sqrt(M) x sqrt(M) polar map of the disc plane (default 10^6)

The device form is timed (synchronised, after a warm-up) in four settings, interleaved REPS times: as shipped, without the
point sort (SPH_GRAVAT_POINT_SORT=0: the points in the map's own order), and with the points shuffled, sorted and unsorted
(what the sort buys on points that come in no order).  All give bitwise the same rows, which is checked.  Prints one JSON
line: wall time per call of each setting, of the host form and of sph_energy(phi) for comparison."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402
from summersph_amd import sample as smp  # noqa: E402


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5, m_disc=0.5))
    side = max(int(round(m ** 0.5)), 1)
    pts, _ = smp.polar_points(10.0, float(np.hypot(gas["x"], gas["y"]).max()), side, side)
    ctx = capi.Context(device=0, flags=capi.FLAG_SELF_GRAVITY)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()                              # the cell-sorted order of a running simulation
    dev = torch.device("cuda", 0)
    d_pts = torch.tensor(pts, dtype=torch.float64, device=dev)
    perm = torch.randperm(pts.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    shuffled = [d_pts[perm, a].contiguous() for a in range(3)]
    ordered = [d_pts[:, a].contiguous() for a in range(3)]
    settings = {"shipped": (ordered, "1"), "no_point_sort": (ordered, "0"), "shuffled_sorted": (shuffled, "1"),
                "shuffled_unsorted": (shuffled, "0")}
    out = {"n": ctx.n, "m": int(pts.shape[0])}
    rows = {}
    times = {k: 0.0 for k in settings}
    for rep in range(reps + 1):                              # the first round warms up (scratch, tree arrays, code objects)
        for name, (p, sort) in settings.items():
            os.environ["SPH_GRAVAT_POINT_SORT"] = sort
            ctx.synchronize()
            t0 = time.perf_counter()
            phi, acc = ctx.gravity_at(p, sinks=False, device=True)
            ctx.synchronize()
            if rep:
                times[name] += time.perf_counter() - t0
            rows[name] = torch.cat([phi[None], acc])
    os.environ.pop("SPH_GRAVAT_POINT_SORT")
    for name in settings:
        out[name + "_ms"] = times[name] / reps * 1e3
        ref = rows["shipped"][:, perm] if name.startswith("shuffled") else rows["shipped"]
        out[name + "_bitwise"] = bool(torch.equal(rows[name], ref))
    ctx.gravity_at(pts, sinks=False)
    t0 = time.perf_counter()
    ctx.gravity_at(pts, sinks=False)
    out["host_ms"] = (time.perf_counter() - t0) * 1e3
    ctx.energy(phi=True)
    t0 = time.perf_counter()
    ctx.energy(phi=True)
    out["energy_host_phi_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
