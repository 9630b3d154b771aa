#!/usr/bin/env python3
"""Times sph_history on a Keplerian disc.  Every mode prints one JSON object; OUT ("-": none) gets it
as a file too.  profiles/history_time.json holds a run's objects side by side.

  rows N NS REPS [OUT]
      device time of one recorded row: HIP events on the context's stream around REPS sph_history_record calls, after a
      density pass (the cell-sorted order of a running simulation) and one warm-up row.  N gas particles of
      ic.keplerian_disc(N, seed=5), fixed h; NS = 1 keeps its sink, NS = 2 adds a second one.  For the split per kernel
      run this mode under `rocprofv3 --kernel-trace --stats -- python profiles/history_time.py rows N NS REPS` in a run of
      its own (history_maxima, history_head, history_sums, history_row).
  steps N STEPS REPS [OUT]
      the steady-state step with the history off and with every = 1, 10, 100: one context each, all advanced alike (the
      history changes nothing of a run), REPS rounds that alternate the four, each round one sph_run(STEPS) per context
      under a host clock (the run ends in sph_get_dt's synchronisation).
  off N STEPS REPS [OUT]
      the `off` leg of `steps` alone: the child of an A/B against another checkout (SUMMERSPH_TREE names its root; the
      package and the library are taken from there).
  ab N STEPS REPS ROUNDS OTHER_TREE [OUT]
      history off, this tree against OTHER_TREE (the parent commit checked out and built beside it): ROUNDS rounds of
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


def disc_context(n, ns=1):
    from summersph_amd import capi, ic
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    if ns == 2:                                              # a light companion inside the disc's inner edge
        second = dict(zip("x y z vx vy vz m".split(), (6.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.01)))
        sinks = {k: np.array([float(sinks[k][0]), second[k]]) for k in second}
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    return ctx


def stat(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def mode_rows(n, ns, reps):
    import torch
    ctx = disc_context(n, ns)
    ctx.density()
    ctx.history_begin(reps + 1)
    ctx.history_record()                                     # warm-up: code objects
    ctx.synchronize()
    dev = torch.device("cuda", 0)
    st = torch.cuda.ExternalStream(ctx.stream(), device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    with torch.cuda.stream(st):
        ev[0].record(st)
        for k in range(reps):
            ctx.history_record()
            ev[k + 1].record(st)
    ctx.synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]
    # the first pass reads 9 doubles (the state's 8 and rho) and the id of every slot, the second the 8 and the id
    out = {"mode": "rows", "n": ctx.n, "ns": ns, "row": stat(ms), "row_bytes_read": ctx.n * ((9 * 8 + 4) + (8 * 8 + 4))}
    ctx.close()
    return out


def steady(ctx, warm=6):
    dt, t = ctx.run(warm, 1e-2, 0.0)
    return [dt, t]


def mode_steps(n, steps, reps, variants=(("off", 0), ("every1", 1), ("every10", 10), ("every100", 100))):
    ctxs, clock, ms = {}, {}, {}
    for name, every in variants:
        ctxs[name] = disc_context(n)
        clock[name] = steady(ctxs[name])
        if every:
            ctxs[name].history_begin(steps * reps // every + 1, every)
        ms[name] = []
    for _ in range(reps):
        for name, _e in variants:                            # alternated
            c = ctxs[name]
            c.synchronize()
            t0 = time.perf_counter()
            clock[name] = list(c.run(steps, *clock[name]))
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {"mode": "steps", "n": n, "steps_per_run": steps, "tree": "other" if os.environ.get("SUMMERSPH_TREE") else "this"}
    for name, _e in variants:
        out[name] = stat(ms[name])
        out[name]["t_end"] = clock[name][1]
        ctxs[name].close()
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
    mode = a[0] if a else "rows"
    if mode == "rows":
        out, rest = mode_rows(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "steps":
        out, rest = mode_steps(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "off":
        out, rest = mode_steps(int(a[1]), int(a[2]), int(a[3]), variants=(("off", 0),)), a[4:]
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
