#!/usr/bin/env python3
"""Times sph_pairs on a Keplerian disc beside sph_groups at link = r_hi, the cost of the same cell
search without the binning; run it under `rocprofv3 --kernel-trace --stats -- python profiles/pairs_time.py N REPS CASE`
in a run of its own, one case per run, for the per-kernel times (pairs_select .. pairs_bin, pairs_sum, the rocprim sort).

  N      gas particles of ic.keplerian_disc(N, seed=5) with its sink (default 10^6), after sph_density (cell-sorted order)
  REPS   timed repeats after one warm-up of every shape (default 5)
  CASES  comma-separated cases "<r_hi / h>x<stride>", e.g. "2x1,8x8" (default 2x1,2x8,4x1,4x8,8x1,8x8), and "g<r_hi / h>"
         for the sph_groups yardstick (default g2,g4,g8 too)
  OUT    a file the JSON goes to as well (default "-": only printed; profiles/pairs_time.json holds a run's object under
         "wall" beside the kernel tables and the forms that lost)

Every pairs case is 64 logarithmic bins of r in [r_hi / 100, r_hi) with the velocity sums (6 sums per bin), weight one, host
form.  Wall time is a host clock around calls that end in the host form's own read-back; the pair terms are the counts
N summed over the bins (ordered pairs), so pairs_per_s is selected pair terms per second of wall time -- the candidates
the 27-cell search visits are several times as many.  Prints (and writes) one JSON object."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402

DEFAULT = "2x1,2x8,4x1,4x8,8x1,8x8,g2,g4,g8"


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
    h = float(ctx.params.h)
    out = {"n": ctx.n, "h": h, "reps": reps, "bins": 64, "sums_per_bin": 6}
    for case in cases:
        if case.startswith("g"):
            link = float(case[1:]) * h
            out[case] = timed(lambda: ctx.groups(link, labels=False), reps)
            continue
        k, stride = case.split("x")
        r_hi = float(k) * h
        kw = dict(log=True, velocity=True, stride=int(stride))
        r = timed(lambda: ctx.pairs((r_hi / 100.0, r_hi), 64, **kw), reps)
        sums, counts, _ = ctx.pairs((r_hi / 100.0, r_hi), 64, **kw)
        r["pairs"] = int(sums[:, 0].sum())
        r["targets"] = counts[0]
        r["pairs_per_s"] = r["pairs"] / (r["mean_ms"] * 1e-3)
        out[case] = r
    ctx.close()
    print(json.dumps(out))
    if path != "-":
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
