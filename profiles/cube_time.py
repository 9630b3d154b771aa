#!/usr/bin/env python3
"""Times sph_cube_dev ("Spectral cubes") with HIP events on the context's stream; run it under
`rocprofv3 --kernel-trace --stats -- python profiles/cube_time.py N --quick` for the per-kernel times (cube_stats_partial
... cube_gather and the rocprim radix sort).

  N          gas particles (default 10^6) of ic.keplerian_disc(N, seed=5) (fixed h) and ic.keplerian_disc_var(N, seed=5)
             (each particle's own h), seen at 40 degrees inclination, position angle 30
  --quick    one configuration per set (256^2 x 64 channels, sigma / dv = 2) instead of the whole table
  --ab       256^2 x 64 channels at the three sigma / dv: the table of an A/B build (SUMMERSPH_LIB)
  --reps R   timed calls per configuration after one warm-up (default 5); the median is reported

Per configuration (image 256^2 / 512^2 over the projected disc, 16 / 64 / 256 channels over the line-of-sight velocities,
sigma / dv = 0.5 / 2 / 8): ms per cube (events around the whole call: both read-backs included), pair evaluations
(particle, node) per second and voxel updates per second.  The pair count is estimated as the footprint area pi (2 h)^2
over the node area for the particles inside the node box, a pair's channels as 17 sigma / dv + 1 (at most the channels).
The cost a user had without the pass: n_chan projected sph_render_field calls (64 nodes along the line of sight) of the
same image size on the same context; the ratio is a cost comparison only, the two do not compute the same integral.
Prints one JSON line.  SUMMERSPH_LIB selects an A/B build of the library."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402
from summersph_amd import cube as cb  # noqa: E402


def event_ms(fn, stream, reps):
    """median ms of fn() between two events on the context's stream, after one warm-up"""
    import torch
    fn()
    stream.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ab", action="store_true")
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
        vel = np.stack([gas["vx"], gas["vy"], gas["vz"]], axis=1)
        P, V = pos @ rot.T, vel @ rot[2]
        h = gas["h"] if variable else np.full(a.n, float(ctx.params.h))
        ext = float(np.abs(P[:, :2]).max())
        vmax = float(np.abs(V).max())
        sizes, chans, ratios = ((256,), (64,), (2.0,)) if a.quick else ((256, 512), (16, 64, 256), (0.5, 2.0, 8.0))
        if a.ab:
            sizes, chans, ratios = (256,), (64,), (0.5, 2.0, 8.0)
        for size in sizes:
            step = 2.0 * ext / (size - 1)
            inside = (np.abs(P[:, 0]) <= ext) & (np.abs(P[:, 1]) <= ext)
            pairs = float(np.sum(np.pi * (2.0 * h[inside]) ** 2) / step ** 2)
            # the parent's route to one channel: a projected field render of the same image, 64 nodes along the line of sight
            lo, hi = pos.min(axis=0), pos.max(axis=0)
            render_ms = event_ms(lambda: ctx.render_field("vz", (size, size, 64), bounds=(lo, hi), axis="z", normalise=True,
                                                          device=True), stream, a.reps)
            for n_chan in chans:
                v0, dv = cb.vrange_channels(-vmax, vmax, n_chan)
                for ratio in ratios:
                    sigma = ratio * dv
                    kw = dict(shape=(size, size), bounds=((-ext, -ext), (ext, ext)), v0=v0, dv=dv, n_chan=n_chan, rot=rot,
                              sigma_floor=sigma, device=True)
                    ms = event_ms(lambda: ctx.cube(**kw), stream, a.reps)
                    per_pair = min(17.0 * ratio + 1.0, float(n_chan))
                    out["rows"].append({"h": "own" if variable else "fixed", "size": size, "n_chan": n_chan, "sigma_over_dv": ratio,
                                        "cube_ms": round(ms, 3), "pairs": round(pairs), "pairs_per_s": round(pairs / ms * 1e3),
                                        "voxel_updates_per_s": round(pairs * per_pair / ms * 1e3),
                                        "render_field_ms": round(render_ms, 3),
                                        "n_chan_renders_over_cube": round(n_chan * render_ms / ms, 1)})
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
