#!/usr/bin/env python3
"""Times sph_gradients on a Keplerian disc ("SPH gradients"); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/gradients_time.py N` for the per-kernel times (grad_select ...
grad_walk, the rocprim radix sort and select).

  N      gas particles (default 10^6) of ic.keplerian_disc(N, seed=5) (fixed h = 2.5), or with --variable of
         ic.keplerian_disc_var(N, seed=5) (each particle's own h)
  REPS   timed calls per case (default 3)
  --no-host  skip the host baseline (it takes seconds to minutes at 10^7)

Cases: vx, vy, vz in the corrected form (the velocity gradient), u alone (1 field) and vx, vy, vz, u (4 fields).  Prints
one JSON line: wall time per call of the host form (after one warm-up) and of the device form (synchronised) for every
case, the target and singular counts, and the host baseline for the velocity gradient: download the fields, then a
scipy cKDTree ball query and the numpy restatement tests/gradients_ref.py."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from summersph_amd import capi, ic  # noqa: E402

CASES = {"v3": ("vx", "vy", "vz"), "f1": ("u",), "f4": ("vx", "vy", "vz", "u")}


def host_baseline(ctx, variable):
    import gradients_ref
    t0 = time.perf_counter()
    pos = np.stack([ctx.field("x"), ctx.field("y"), ctx.field("z")], axis=1)
    A = np.stack([ctx.field("vx"), ctx.field("vy"), ctx.field("vz")])
    h = ctx.field("h") if variable else 2.5
    gradients_ref.gradients(pos, ctx.field("m"), A, h, corrected=True)
    return {"host_kind": "download + scipy cKDTree + numpy (tests/gradients_ref.py)", "host_s": time.perf_counter() - t0}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    variable = "--variable" in sys.argv
    n = int(args[0]) if args else 1_000_000
    reps = int(args[1]) if len(args) > 1 else 3
    rows = ic.keplerian_disc_var(n, seed=5) if variable else ic.keplerian_disc(n, seed=5)
    gas, sinks = ic.split_rows(rows)
    ctx = capi.Context(device=0, variable=variable)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    ctx.synchronize()
    out = {"n": ctx.n, "variable": variable}
    for name, fields in CASES.items():
        ctx.gradients(fields=fields)                          # warm-up (scratch, code objects)
        t0 = time.perf_counter()
        for _ in range(reps):
            _, _, cnt = ctx.gradients(fields=fields)
        out[f"{name}_host_ms"] = (time.perf_counter() - t0) / reps * 1e3
        ctx.gradients(fields=fields, device=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.gradients(fields=fields, device=True)
        ctx.synchronize()
        out[f"{name}_device_ms"] = (time.perf_counter() - t0) / reps * 1e3
        out[f"{name}_counts"] = list(cnt)
    if "--no-host" not in sys.argv:
        out.update(host_baseline(ctx, variable))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
