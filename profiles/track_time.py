#!/usr/bin/env python3
"""Times sph_track on a Keplerian disc.  Every mode prints one JSON object; OUT ("-": none) gets it
as a file too.  profiles/track_time.json holds a run's objects side by side.

  rows N K REPS [OUT]
      device time of one recorded row: HIP events on the context's stream around REPS sph_track_record calls, after a
      density pass (the cell-sorted order of a running simulation) and one warm-up row.  N gas particles of
      ic.keplerian_disc(N, seed=5), fixed h; K tracked ids, a random subset in random order.  For the kernel's own time run
      this mode under `rocprofv3 --kernel-trace --stats -- python profiles/track_time.py rows N K REPS` in a run of its
      own (track_row).
  repack N K REPS [OUT]
      one accretion pack that removes a particle, with a tracker of K ids and without: two contexts with the bound drawn
      inside the disc's outermost particles, REPS rounds that alternate the two; each round puts one more particle outside
      the bound (sph_upload_field), runs sph_density and times sph_accrete_and_cull + sph_synchronize under a host clock.
      The difference is the repack (track_repack, the bitmap's clear, track_bits, track_prefix, track_tags); their own
      times come from a `rocprofv3 --kernel-trace --stats` run of this mode.
  steps N K STEPS REPS [OUT]
      the steady-state step with the tracker off and with every = 1, 10: one context each, all advanced alike (the tracker
      changes nothing of a run), REPS rounds that alternate the three, each round one sph_run(STEPS) per context under a
      host clock (the run ends in sph_get_dt's synchronisation).
  off N STEPS REPS [OUT]
      the `off` leg of `steps` alone: the child of an A/B against another checkout (SUMMERSPH_TREE names its root; the
      package and the library are taken from there).
  ab N STEPS REPS ROUNDS OTHER_TREE [OUT]
      tracker off, this tree against OTHER_TREE (the parent commit checked out and built beside it): ROUNDS rounds of
      fresh child processes `off` in the order other, this, other, this ..., each under its own time limit.  Reports both
      means and the spread of the other tree against itself.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("SUMMERSPH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def disc_context(n, **params):
    from summersph_amd import capi, ic
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0, **params)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    return ctx, gas


def some_ids(n, k, seed=28):
    return np.random.default_rng(seed).permutation(n)[:k]


def stat(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def mode_rows(n, k, reps):
    import torch
    ctx, _ = disc_context(n)
    ctx.density()
    ctx.track_begin(some_ids(ctx.n, k), reps + 1)
    ctx.track_record()                                       # warm-up: code objects
    ctx.synchronize()
    dev = torch.device("cuda", 0)
    st = torch.cuda.ExternalStream(ctx.stream(), device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    with torch.cuda.stream(st):
        ev[0].record(st)
        for r in range(reps):
            ctx.track_record()
            ev[r + 1].record(st)
    ctx.synchronize()
    ms = [ev[r].elapsed_time(ev[r + 1]) for r in range(reps)]
    # the pass reads the id of every slot; a hit reads ten doubles and writes ten
    out = {"mode": "rows", "n": ctx.n, "k": k, "row": stat(ms), "row_bytes_read": ctx.n * 4 + k * 10 * 8, "row_bytes_written": k * 10 * 8}
    ctx.close()
    return out


def mode_repack(n, k, reps):
    _c, gas = disc_context(n)
    _c.close()
    bound = float(np.max(np.abs(np.stack([gas["x"], gas["y"], gas["z"]])))) * 1.01      # nobody is outside to begin with
    leaving = np.argsort(-np.abs(gas["x"]))[:reps + 2]       # the particles the rounds put outside, one each
    staying = np.setdiff1d(np.arange(n), leaving)
    ctxs, ms, removed = {}, {"on": [], "off": []}, {"on": 0, "off": 0}
    for name in ("on", "off"):
        ctxs[name], _ = disc_context(n, bounding_size=bound)
    ctxs["on"].track_begin(np.random.default_rng(28).permutation(staying)[:k], 1)
    for rep in range(reps + 1):                              # round 0: warm-up
        for name in ("on", "off"):
            c = ctxs[name]
            x = c.field("x")
            x[int(np.argmax(np.abs(x)))] = 2.0 * bound       # one more particle leaves
            c.upload_field("x", x)
            c.density()
            c.synchronize()
            t0 = time.perf_counter()
            gone = c.accrete_and_cull()
            c.synchronize()
            if rep:
                ms[name].append((time.perf_counter() - t0) * 1e3)
                removed[name] += gone
    out = {"mode": "repack", "n": n, "k": k, "on": stat(ms["on"]), "off": stat(ms["off"]), "removed": removed}
    out["difference_ms"] = out["on"]["mean_ms"] - out["off"]["mean_ms"]
    out["n_live"] = ctxs["on"].track_info()["n_live"]
    for c in ctxs.values():
        c.close()
    return out


def steady(ctx, warm=6):
    dt, t = ctx.run(warm, 1e-2, 0.0)
    return [dt, t]


def mode_steps(n, k, steps, reps, variants=(("off", 0), ("every1", 1), ("every10", 10))):
    ctxs, clock, ms = {}, {}, {}
    for name, every in variants:
        ctxs[name], _ = disc_context(n)
        clock[name] = steady(ctxs[name])
        if every:
            ctxs[name].track_begin(some_ids(n, k), steps * reps // every + 1, every)
        ms[name] = []
    for _ in range(reps):
        for name, _e in variants:                            # alternated
            c = ctxs[name]
            c.synchronize()
            t0 = time.perf_counter()
            clock[name] = list(c.run(steps, *clock[name]))
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {"mode": "steps", "n": n, "k": k, "steps_per_run": steps, "tree": "other" if os.environ.get("SUMMERSPH_TREE") else "this"}
    for name, _e in variants:
        out[name] = stat(ms[name])
        out[name]["t_end"] = clock[name][1]
        ctxs[name].close()
    if "every1" in out:
        out["every1_overhead_pct"] = 100.0 * (out["every1"]["mean_ms"] / out["off"]["mean_ms"] - 1.0)
    return out


def mode_ab(n, steps, reps, rounds, other):
    me = [sys.executable, os.path.abspath(__file__), "off", str(n), str(steps), str(reps)]
    got = {"other": [], "this": []}
    for _ in range(rounds):
        for who in ("other", "this"):
            env = dict(os.environ)
            if who == "other":
                env["SUMMERSPH_TREE"] = os.path.abspath(other)
            else:
                env.pop("SUMMERSPH_TREE", None)
            r = subprocess.run(me, env=env, capture_output=True, text=True, timeout=600, check=True)
            got[who].append(json.loads(r.stdout.strip().splitlines()[-1])["off"]["mean_ms"])
    o, m = np.array(got["other"]), np.array(got["this"])
    return {"mode": "ab", "n": n, "steps_per_run": steps, "reps": reps, "other_ms_per_step": got["other"],
            "this_ms_per_step": got["this"], "other_mean": float(o.mean()), "this_mean": float(m.mean()),
            "other_spread": float(o.max() - o.min()), "difference": float(m.mean() - o.mean())}


def main():
    a = sys.argv[1:]
    mode = a[0] if a else ""
    if mode == "rows":
        out, rest = mode_rows(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "repack":
        out, rest = mode_repack(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "steps":
        out, rest = mode_steps(int(a[1]), int(a[2]), int(a[3]), int(a[4])), a[5:]
    elif mode == "off":
        out, rest = mode_steps(int(a[1]), 0, int(a[2]), int(a[3]), variants=(("off", 0),)), a[4:]
    elif mode == "ab":
        out, rest = mode_ab(int(a[1]), int(a[2]), int(a[3]), int(a[4]), a[5]), a[6:]
    else:
        sys.exit(__doc__)
    print(json.dumps(out))
    if rest and rest[0] != "-":
        with open(rest[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
