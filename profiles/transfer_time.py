#!/usr/bin/env python3
"""Times sph_transfer_dev ("Emission-absorption images") with HIP events on the context's stream; run
it under `rocprofv3 --kernel-trace --stats -- python profiles/transfer_time.py N --quick` for the per-kernel times
(transfer_stats_partial ... transfer_gather and the rocprim sorts and scan).

  N          gas particles (default 10^6) of ic.keplerian_disc(N, seed=5) (fixed h) and ic.keplerian_disc_var(N, seed=5)
             (each particle's own h), seen at 40 degrees inclination, position angle 30: the discs of cube_time.py
  --quick    one configuration per set (256^2, tau ~ 1) instead of the whole table
  --reps R   timed calls per configuration after one warm-up (default 5); the median is reported

Per configuration (image 256^2 / 512^2 over the projected disc; kappa_scale chosen from a first call so that the median lit
node has tau = 0.01 (thin), 1, or 30 with tau_max = 30 (opaque: half of the lit nodes stop)): ms per image (events around
the whole call: both read-backs included), the entries of the tile lists and (particle, node) pairs per second, the pair
count estimated as the footprint area pi (2 h)^2 over the node area for the particles inside the node box.  The cost a user
had without the pass for the nearest thing: one one-channel sph_cube call of the same image (the optically thin column);
the ratio is a cost comparison only, the two do not compute the same thing.  Prints one JSON line.  SUMMERSPH_LIB selects
an A/B build of the library."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402
from summersph_amd import cube as cb  # noqa: E402
from cube_time import event_ms  # noqa: E402


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rot = cb.view(40.0, 30.0)
    out = {"n": a.n, "lib": os.path.basename(capi.LIB_PATH), "rows": []}
    for variable in (False, True):
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(a.n, seed=5) if variable else ic.keplerian_disc(a.n, seed=5))
        ctx = capi.Context(device=0, variable=variable)
        ctx.upload(gas)
        ctx.set_sinks(sinks)
        ctx.synchronize()
        st = ctx.stream()
        stream = torch.cuda.ExternalStream(st, device=dev) if st else torch.cuda.default_stream(dev)
        pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
        P = pos @ rot.T
        h = gas["h"] if variable else np.full(a.n, float(ctx.params.h))
        ext = float(np.abs(P[:, :2]).max())
        for size in (256,) if a.quick else (256, 512):
            step = 2.0 * ext / (size - 1)
            pairs = float(np.sum(np.pi * (2.0 * h) ** 2) / step ** 2)
            img = dict(shape=(size, size), bounds=((-ext, -ext), (ext, ext)), rot=rot, device=True)
            cube_ms = event_ms(lambda: ctx.cube(v0=0.0, dv=1e6, n_chan=1, **img), stream, a.reps)
            tau = ctx.transfer(source="u", **img)[1]
            med = float(tau[tau > 0].median())
            for tag, target, tau_max in (("tau 1", 1.0, np.inf),) if a.quick else (("thin", 0.01, np.inf), ("tau 1", 1.0, np.inf),
                                                                                   ("opaque", 30.0, 30.0)):
                kw = dict(img, source="u", kappa_scale=target / med, tau_max=tau_max)
                ms = event_ms(lambda: ctx.transfer(**kw), stream, a.reps)
                res = ctx.transfer(**kw)
                lit = res[1] > 0
                out["rows"].append({"h": "own" if variable else "fixed", "size": size, "case": tag, "transfer_ms": round(ms, 3),
                                    "pairs": round(pairs), "pairs_per_s": round(pairs / ms * 1e3),
                                    "lit": int(lit.sum()), "stopped": int((res[1] >= tau_max).sum()) if np.isfinite(tau_max) else 0,
                                    "surface": int(torch.isfinite(res[3]).sum()), "cube_1chan_ms": round(cube_ms, 3),
                                    "transfer_over_cube": round(ms / cube_ms, 2)})
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
