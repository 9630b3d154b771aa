#!/usr/bin/env python3
"""Times sph_force_terms beside the force pass it splits; run it under
`rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/force_terms_time.py CONFIG` for the per-kernel times
(force_terms_kernel / force_terms_v_kernel next to forces_kernel, forces_q and forces_v_kernel).

    python profiles/force_terms_time.py CONFIG [N] [REPS] [--out FILE.json]

  CONFIG  fixed            fixed h, default flags (sph_forces runs the whole-tile kernel forces_q)
          fixed_gather     fixed h, SPH_FLAG_NO_WHOLE_TILE (sph_forces runs forces_kernel, the gather sibling)
          variable         variable h (forces_v_kernel, the sibling)
          *_gravity        the same with SPH_FLAG_SELF_GRAVITY: the call with and without the tree walk
  N       gas particles of ic.keplerian_disc(N, seed=5, m_disc=0.5) / keplerian_disc_var (default 10^6), with the sink
  REPS    timed calls after one warm-up call (default 9); medians are reported

One configuration per process, so that a job can give each its own time limit.  Reported, in ms: the device time (HIP
events on the context's stream) of sph_force_terms_dev with SPH_TERMS_SKIP_GAS_GRAVITY and, with self-gravity, with the
walk; SPH_K_FORCES of one sph_forces on the same context (and SPH_K_GRAVITY with self-gravity).  The rows of the timed calls
are checked to be bitwise the same.  Prints one JSON line; --out merges it into FILE.json under the configuration's name."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402

CONFIGS = {"fixed": (False, 0), "fixed_gather": (False, capi.FLAG_NO_WHOLE_TILE), "variable": (True, 0)}


def main():
    import ctypes as C

    import torch
    args = [a for a in sys.argv[1:]]
    out_file = None
    if "--out" in args:
        k = args.index("--out")
        out_file = args[k + 1]
        del args[k:k + 2]
    name = args[0] if args else "fixed"
    n = int(args[1]) if len(args) > 1 else 1_000_000
    reps = int(args[2]) if len(args) > 2 else 9
    gravity = name.endswith("_gravity")
    variable, flags = CONFIGS[name[:-len("_gravity")] if gravity else name]
    flags |= capi.FLAG_SELF_GRAVITY if gravity else 0
    if variable:
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(n, seed=5, m_disc=0.5))
        ctx = capi.Context(device=0, variable=True, flags=capi.FLAG_VARIABLE_H | flags)
    else:
        gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5, m_disc=0.5))
        gas["alpha"] = np.full(n, 0.5)                            # the reader's alpha is 0: switch the viscosity on
        ctx = capi.Context(device=0, flags=flags)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()                                   # the cell-sorted order of a running simulation
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(ctx.stream(), device=dev)
    out = torch.empty((capi.TERMS_NROW, ctx.n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    res = {"n": ctx.n, "reps": reps, "flags": int(flags), "variable": variable}

    def timed_terms(skip):
        d = capi.ForceTermsDesc()
        d.flags = capi.TERMS_SKIP_GAS_GRAVITY if skip else 0
        ms, first = [], None
        for rep in range(reps + 1):                              # the first call warms up (scratch, code objects, the tree)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            st = ctx.lib.sph_force_terms_dev(ctx._h, C.byref(d), C.c_void_p(out.data_ptr()), out.numel())
            e1.record(stream)
            assert st == 0, st
            ctx.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
            keep = out.clone()
            assert first is None or torch.equal(torch.nan_to_num(keep), torch.nan_to_num(first))
            first = keep
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    res["terms_skip_gravity_ms"], res["terms_skip_gravity_min_ms"], res["terms_skip_gravity_max_ms"] = timed_terms(True)
    if gravity:
        res["terms_with_walk_ms"], res["terms_with_walk_min_ms"], res["terms_with_walk_max_ms"] = timed_terms(False)
    kernels = ["forces"] + (["gravity", "grav_walk"] if gravity else [])
    ctx.timing(True, only=kernels)
    per = {k: [] for k in kernels}
    for rep in range(reps + 1):
        ctx.timing_reset()
        ctx.forces()
        ctx.synchronize()
        for k in kernels:
            ms, cnt = ctx.timing_get(k)
            if rep and cnt:
                per[k].append(ms / cnt)
    ctx.timing(False)
    for k in kernels:
        res[f"sph_forces_K_{k}_ms"] = float(np.median(per[k]))
    res["forces_kernel_in_use"] = ("forces_v_kernel" if variable else
                                   ("forces_kernel (gather)" if flags & capi.FLAG_NO_WHOLE_TILE else "whole-tile / forces_q where it fits"))
    st = ctx.stats()
    res["nlist_mean"] = st.nlist_mean
    res["tile_fit_pct_forces"] = st.tile_fit_pct_forces
    ctx.close()
    print(json.dumps({name: res}))
    if out_file:
        merged = {}
        if os.path.exists(out_file):
            with open(out_file) as f:
                merged = json.load(f)
        merged[name] = res
        with open(out_file, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
