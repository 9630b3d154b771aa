#!/usr/bin/env python3
"""Times sph_profile on a Keplerian disc ("Disc profiles") against a host numpy baseline that bins the
same snapshot from downloaded fields; run it under `rocprofv3 --kernel-trace --stats -- python profiles/profile_time.py N`
for the per-kernel times (profile_keys, the rocprim sort, profile_starts, profile_pieces, profile_final).

  N   gas particles of ic.keplerian_disc(N, seed=5) with its sink (default 10^6); 64 log rings x 1 sector about the sink,
      no z cut, and 64 x 16 ring sectors

Prints one JSON line: wall time per call (host form, table included, after one warm-up), the same for the device form
(sums only, synchronised), and the numpy baseline: the download of the nine fields plus an np.bincount binning of the
same 20 moments (its summation order is numpy's, not the device's)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402


def numpy_baseline(ctx, sinks, r0, r1, nr):
    f = {k: ctx.field(k) for k in "x y z vx vy vz u m alpha".split()}
    c = [sinks[k][0] for k in "xyz"]
    cv = [sinks[k][0] for k in ("vx", "vy", "vz")]
    r = [f[k] - c[a] for a, k in enumerate("xyz")]
    v = [f[k] - cv[a] for a, k in enumerate(("vx", "vy", "vz"))]
    R = np.sqrt(r[0] * r[0] + r[1] * r[1])
    e = r0 * (r1 / r0) ** (np.arange(nr + 1) / nr)
    k = np.searchsorted(e, R, side="right") - 1
    sel = (R >= r0) & (R < r1)
    k = np.where(sel, k, nr)
    m = f["m"]
    vR = (r[0] * v[0] + r[1] * v[1]) / R
    vp = (r[0] * v[1] - r[1] * v[0]) / R
    lz = r[0] * v[1] - r[1] * v[0]
    q = [np.ones_like(m), m, m * R, m * r[2], m * r[2] ** 2, m * vR, m * vp, m * v[2], m * vR ** 2, m * vp ** 2, m * v[2] ** 2,
         m * f["u"], m * f["alpha"], m * ctx.params.h, m * (r[1] * v[2] - r[2] * v[1]), m * (r[2] * v[0] - r[0] * v[2]), m * lz]
    return np.stack([np.bincount(k, weights=w, minlength=nr + 1)[:nr] for w in q], axis=1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density()                                            # the cell-sorted order of a running simulation
    R = np.hypot(gas["x"], gas["y"])
    r0, r1 = float(R.min()), float(R.max()) * 1.001
    out = {"n": ctx.n}
    for name, kw in (("rings64", dict(n_r=64)), ("sectors64x16", dict(n_r=64, n_phi=16))):
        args = dict(r_min=r0, r_max=r1, log=True, sink=0, **kw)
        ctx.profile(**args)                                  # warm-up (scratch, code objects)
        t0 = time.perf_counter()
        for _ in range(reps):
            t, s = ctx.profile(**args)
        out[name + "_host_ms"] = (time.perf_counter() - t0) / reps * 1e3
        ctx.profile(**args, device=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            d = ctx.profile(**args, device=True)
        ctx.synchronize()
        out[name + "_device_ms"] = (time.perf_counter() - t0) / reps * 1e3
        assert int(s[:, 0].sum()) == ctx.n - int(np.sum(R >= r1))
    t0 = time.perf_counter()
    base = numpy_baseline(ctx, sinks, r0, r1, 64)
    out["numpy_baseline_ms"] = (time.perf_counter() - t0) * 1e3
    _, s = ctx.profile(r0, r1, 64, log=True, sink=0)
    out["numpy_vs_gpu_max_rel_M"] = float(np.max(np.abs(base[:, 1] - s[:, 1]) / np.abs(s[:, 1])))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
