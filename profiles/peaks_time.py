#!/usr/bin/env python3
"""Times sph_peaks on a Keplerian disc ("Density-peak clumps"); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/peaks_time.py N REPS` for the per-kernel times (groups_select ...
groups_tails, peaks_gather ... peaks_table, groups_count ... groups_final and the rocprim scan, sorts and reduction).

  N      gas particles of ic.keplerian_disc(N, seed=5) (default 10^6); fixed h = 2.5, link = h, contrast 2: the set and
         the link of profiles/groups_time.py
  REPS   timed calls (default 3)
  --no-host  skip the host baseline

Prints one JSON line: wall time per call of the host form (labels + the 100 largest clumps, after one warm-up) and of the
device form (synchronised), sph_groups' host form on the same context beside it, the counts (clumps, raw peaks, edges) per
particle, what the library reports about one call (neighbour pairs that cross basins, passes over them, the host merge's
milliseconds and when the three waits and the merge ended: SPH_PEAKS_TIMING), and the host baseline: the numpy restatement tests/peaks_ref.py on the downloaded fields."""
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SPH_PEAKS_TIMING"] = "1"
from summersph_amd import capi, ic  # noqa: E402


def library_report(fn):
    """runs fn with the process's stderr in a file and returns the library's last timing line as a dict"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.findall(r"sph_peaks: pairs (\d+) edges (\d+) passes (\d+) merge_ms ([0-9.]+) waits_ms ([0-9.]+) ([0-9.]+) ([0-9.]+) "
                   r"merged_ms ([0-9.]+)", text)
    if not m:
        return {}
    p, e, k, ms, w1, w2, w3, w4 = m[-1]
    return {"cross_pairs": int(p), "passes": int(k), "merge_ms": float(ms),
            "ms_at_pair_count_edge_count_edge_list_merged": [float(w1), float(w2), float(w3), float(w4)]}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 1_000_000
    reps = int(args[1]) if len(args) > 1 else 3
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    link, contrast = 2.5, 2.0
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    ctx.density()                                            # rho, and the cell-sorted order of a running simulation
    ctx.synchronize()
    out = {"n": ctx.n, "link": link, "contrast": contrast}
    saved = os.dup(2)
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 2)                                      # the timing lines of the timed calls
    try:
        ctx.peaks(link, contrast, max_groups=100)            # warm-up (scratch, code objects)
        ctx.peaks(link, contrast, max_groups=100)
        t0 = time.perf_counter()
        for _ in range(reps):
            lab, tab, ng, cnt = ctx.peaks(link, contrast, max_groups=100)
        out["host_ms"] = (time.perf_counter() - t0) / reps * 1e3
        ctx.peaks(link, contrast, max_groups=100, device=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.peaks(link, contrast, max_groups=100, device=True)
        ctx.synchronize()
        out["device_ms"] = (time.perf_counter() - t0) / reps * 1e3
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        os.close(devnull)
    out.update(library_report(lambda: ctx.peaks(link, contrast, max_groups=100)))
    out["merge_share"] = out.get("merge_ms", 0.0) / out["host_ms"]
    ctx.groups(link, max_groups=100)
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.groups(link, max_groups=100)
    out["groups_host_ms"] = (time.perf_counter() - t0) / reps * 1e3
    out.update({"n_groups": ng, "n_raw_peaks": cnt[1], "n_edges": cnt[2], "peaks_per_particle": cnt[1] / ctx.n,
                "edges_per_particle": cnt[2] / ctx.n, "largest": int(tab["N"][0]) if ng else 0,
                "device_bytes": int(ctx.stats().device_bytes)})
    if "--no-host" not in sys.argv:
        import peaks_ref
        t0 = time.perf_counter()
        f = {k: ctx.field(k) for k in "x y z vx vy vz u m rho".split()}
        ref = peaks_ref.peaks(f, ctx.n, link, contrast=contrast)
        out.update({"host_kind": "numpy restatement (tests/peaks_ref.py)", "host_s": time.perf_counter() - t0,
                    "host_matches": bool(ref[3] == cnt and np.array_equal(ref[0], lab))})
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
