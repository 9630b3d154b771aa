#!/usr/bin/env python3
"""Times sph_dust on the bench disc.  Every mode prints one JSON object; OUT ("-": none) gets it as a
file too.  profiles/dust_time.json holds a run's objects side by side.

  advance N REPS [OUT]
      device time of one advance: HIP events on the context's stream around sph_dust_advance (median of REPS after a
      warm-up) for ic.keplerian_disc(N, seed=5) after six steps (the cell-sorted order of a running simulation), with
      M = 1e3, 1e5 and 1e6 grains started on gas particles, Epstein drag.  The clock is moved on before every advance, so
      that each one kicks, drifts and samples.  Beside it, by the same events: sph_sample_dev of the same M points with the
      four fields (the yardstick: an advance is that work plus two kicks) and of one point (the build alone: select,
      levels, keys, sort, records, tails; the walk of one point is nothing).  walk_est = sample(M) - sample(1) and
      kick_sort_est = advance - sample(M) follow from them; the kernels' own times come from `one`.
  one N M REPS [OUT]
      REPS advances of M grains and nothing else after the set-up: the mode to run under
      `rocprofv3 --kernel-trace --stats -- python profiles/dust_time.py one N M REPS` for the split into the build's kernels,
      dust_kick_drift plus the grains' sort, and dust_walk.
  split TRACE.csv [OUT]
      the split of that run's kernel trace (rocprofv3's *_kernel_trace.csv): per advance, the kernels from sample_select up
      to dust_kick_drift are the build, those between dust_kick_drift and dust_walk the grains' sort; medians over the
      advances after the set-up's three, in microseconds, and the span from the first kernel's start to dust_head's end.
  steps N STEPS REPS [OUT]
      the steady-state step with no dust begun and with M = 1e5 grains at every = 1 and every = 8: one context each, all
      advanced alike, REPS rounds that alternate the three, each round one sph_run(STEPS) per context under a host clock.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

GRAINS = (1_000, 100_000, 1_000_000)


def stat(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def disc_context(n):
    from summersph_amd import capi, ic
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    return ctx, gas


def begin(ctx, m, seed=7, **kw):
    """m grains on gas particles of the state as it is, sizes that put the stopping time around the orbital time"""
    from summersph_amd import dust
    x, v = dust.from_gas(ctx.state(), m, seed)
    ctx.dust_begin(x, v, np.ones(m), law="epstein", rho_grain=1.0, capacity=1)
    ctx.dust_advance()
    rate = ctx.dust()["rate"][0]
    size = float(np.median(rate[rate > 0.0])) * 10.0          # rate is 1 / size for unit grains: t_s about 10 code times
    ctx.dust_begin(x, v, np.full(m, size), law="epstein", rho_grain=1.0, **kw)
    return x


class Clock:
    """moves the device's time word on by dt before an advance and waits for the copy"""
    def __init__(self, ctx, dt, t):
        self.ctx, self.dt, self.t = ctx, dt, t

    def tick(self):
        self.t += self.dt
        self.ctx.set_dt(self.dt, self.t)
        self.ctx.synchronize()


def mode_advance(n, reps):
    import torch
    from cube_time import event_ms
    dev = torch.device("cuda", 0)
    ctx, gas = disc_context(n)
    dt, t = ctx.run(6, 1e-2, 0.0)
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.stream(), device=dev)
    out = {"mode": "advance", "n": n, "reps": reps, "rows": []}
    for m in GRAINS:
        x = begin(ctx, m, capacity=0)
        clock = Clock(ctx, dt, t)
        ts = []
        clock.tick()
        ctx.dust_advance()                                    # warm-up; the tick (a copy and a wait) stays outside the events
        for _ in range(reps):
            clock.tick()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.dust_advance()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        adv = float(np.median(ts))
        st = ctx.dust_state(device=True)
        pts = [st["x"], st["y"], st["z"]]
        live = ctx.dust_info()["n_live"]
        ctx.dust_end()
        fields = ("vx", "vy", "vz", "u")
        smp = event_ms(lambda: ctx.sample(pts, fields=fields, normalise=True, weight_out=True, device=True), stream, reps)
        one = [p[:1].contiguous() for p in pts]
        bld = event_ms(lambda: ctx.sample(one, fields=fields, normalise=True, weight_out=True, device=True), stream, reps)
        out["rows"].append({"m": m, "live": live, "advance_ms": round(adv, 4), "advance_min_ms": round(min(ts), 4),
                            "advance_max_ms": round(max(ts), 4), "sample_dev_ms": round(smp, 4),
                            "build_ms": round(bld, 4), "walk_est_ms": round(smp - bld, 4), "kick_sort_est_ms": round(adv - smp, 4),
                            "advance_over_sample": round(adv / smp, 3)})
    ctx.close()
    return out


def mode_one(n, m, reps):
    ctx, gas = disc_context(n)
    dt, t = ctx.run(6, 1e-2, 0.0)
    begin(ctx, m, capacity=0)
    clock = Clock(ctx, dt, t)
    for _ in range(reps):
        clock.tick()
        ctx.dust_advance()
    ctx.synchronize()
    live = ctx.dust_info()["n_live"]
    ctx.close()
    return {"mode": "one", "n": n, "m": m, "reps": reps, "live": live}


def mode_split(path):
    import csv
    with open(path) as f:
        tr = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    adv, cur = [], None
    for r in tr:
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "sample_select" in name:
            cur = {"build": 0, "kick_drift": 0, "sort": 0, "walk": 0, "head": 0, "phase": "build", "t0": t0}
        if cur is None:
            continue
        if "dust_kick_drift" in name:
            cur["kick_drift"], cur["phase"] = t1 - t0, "sort"
        elif "dust_walk" in name:
            cur["walk"], cur["phase"] = t1 - t0, "head"
        elif "dust_head" in name:
            cur["head"], cur["span"] = t1 - t0, t1 - cur["t0"]
            adv.append(cur)
            cur = None
        elif cur["phase"] in ("build", "sort"):
            cur[cur["phase"]] += t1 - t0
    adv = adv[3:]                                             # begin, the t = 0 advance and the second begin do not move
    out = {"mode": "split", "advances": len(adv)}
    for k in ("build", "kick_drift", "sort", "walk", "head", "span"):
        out[k + "_us"] = round(float(np.median([a[k] for a in adv])) / 1e3, 2)
    out["kick_drift_max_us"] = round(max(a["kick_drift"] for a in adv) / 1e3, 2)
    return out


def mode_steps(n, steps, reps, m=100_000, variants=("off", "every1", "every8")):
    ctxs, clock, ms = {}, {}, {}
    for name in variants:
        ctxs[name], gas = disc_context(n)
        clock[name] = list(ctxs[name].run(6, 1e-2, 0.0))
        if name != "off":
            begin(ctxs[name], m, capacity=0, every=int(name[5:]))
        ms[name] = []
    for _ in range(reps):
        for name in variants:                                # alternated
            c = ctxs[name]
            c.synchronize()
            t0 = time.perf_counter()
            clock[name] = list(c.run(steps, *clock[name]))
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {"mode": "steps", "n": n, "m": m, "steps_per_run": steps}
    for name in variants:
        out[name] = stat(ms[name])
        out[name]["t_end"] = clock[name][1]
        if name != "off":
            out[name]["dust"] = ctxs[name].dust_info()
            out[name]["added_ms_per_step"] = out[name]["mean_ms"] - out["off"]["mean_ms"]
        ctxs[name].close()
    return out


def main():
    a = sys.argv[1:]
    mode = a[0] if a else ""
    if mode == "advance":
        out, rest = mode_advance(int(a[1]), int(a[2])), a[3:]
    elif mode == "one":
        out, rest = mode_one(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "split":
        out, rest = mode_split(a[1]), a[2:]
    elif mode == "steps":
        out, rest = mode_steps(int(a[1]), int(a[2]), int(a[3])), a[4:]
    else:
        sys.exit(__doc__)
    print(json.dumps(out))
    if rest and rest[0] != "-":
        with open(rest[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
