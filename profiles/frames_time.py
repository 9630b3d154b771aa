#!/usr/bin/env python3
"""Times sph_frames on a Keplerian disc.  Every mode prints one JSON object; OUT ("-": none) gets it
as a file too.  profiles/frames_time.json holds a run's objects side by side.

  frame N REPS [OUT]
      device time of one frame: HIP events on the context's stream around sph_frames_record (median of REPS after a
      warm-up), for ic.keplerian_disc(N, seed=5) (fixed h) and ic.keplerian_disc_var(N, seed=5) (each particle's own h), after
      a density pass (the cell-sorted order of a running simulation), on 256^2 and 512^2 nodes over the projected disc,
      face-on, at 40 / 30 degrees and edge-on, with one weighted plane (u); beside it sph_frame_dev (the one-shot form) and
      sph_transfer_dev's thin image of the same nodes (kappa_scale so that the median lit node has tau = 0.01): the nearest
      thing a user had before.  pairs: (particle, node) pairs estimated as in transfer_time.py.  The splat's form is the
      library's (SPH_FRAMES_SPLAT=plain: every pair straight to the global limbs).  For the kernels' own times run this
      mode under `rocprofv3 --kernel-trace --stats -- python profiles/frames_time.py frame N REPS` in a run of its own.
  one N SIZE REPS [OUT]
      one case of `frame` alone -- fixed h, 40 / 30 degrees, SIZE^2 nodes, REPS records and nothing else after the set-up:
      the mode to run under `rocprofv3 --kernel-trace --stats` for the five kernels' own times.
  splat N REPS ROUNDS [OUT]
      the two forms of the splat against each other: ROUNDS rounds of fresh child processes `frame`, window then plain.
  steps N STEPS REPS [OUT]
      the steady-state step with frames off, with every = 1 and 10, and with dt_frame set so that about one step in ten
      records (the frame's launches are enqueued every step and return at once when no frame is due): one context each,
      all advanced alike, REPS rounds that alternate the four, each round one sph_run(STEPS) per context under a host clock.
  off N STEPS REPS [OUT]
      the `off` leg of `steps` alone: the child of an A/B against another checkout (SUMMERSPH_TREE names its root).
  ab N STEPS REPS ROUNDS OTHER_TREE [OUT]
      frames off, this tree against OTHER_TREE (the parent commit checked out and built beside it): ROUNDS rounds of fresh
      child processes `off` in the order other, this, other, this ...  Reports both means and the spread of the other tree
      against itself.
  bench ROUNDS OTHER_TREE [OUT]
      `bench.py --gpus 1 --steps 20 --warmup 5 --no-variable --no-extras --no-cpu` of both trees, alternated the same way.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("SUMMERSPH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

VIEWS = (("face", 0.0, 0.0), ("inclined", 40.0, 30.0), ("edge", 90.0, 0.0))


def stat(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def mode_frame(n, reps):
    import torch
    from summersph_amd import capi, ic
    from summersph_amd import cube as cb
    from cube_time import event_ms
    dev = torch.device("cuda", 0)
    out = {"mode": "frame", "n": n, "splat": os.environ.get("SPH_FRAMES_SPLAT", "window"), "rows": []}
    for variable in (False, True):
        gas, sinks = ic.split_rows(ic.keplerian_disc_var(n, seed=5) if variable else ic.keplerian_disc(n, seed=5))
        ctx = capi.Context(device=0, variable=variable)
        ctx.upload(gas)
        ctx.set_sinks(sinks)
        ctx.density()
        ctx.synchronize()
        stream = torch.cuda.ExternalStream(ctx.stream(), device=dev)
        pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
        h = gas["h"] if variable else np.full(n, float(ctx.params.h))
        for tag, inc, pa in VIEWS:
            rot = cb.view(inc, pa)
            P = pos @ rot.T
            ext = float(np.abs(P[:, :2]).max())
            for size in (256, 512):
                step = 2.0 * ext / (size - 1)
                inside = np.all(np.abs(P[:, :2]) <= ext, axis=1)
                pairs = float(np.sum(np.pi * (2.0 * h[inside]) ** 2) / step ** 2)
                img = dict(shape=(size, size), bounds=((-ext, -ext), (ext, ext)), rot=rot)
                ctx.frames_begin(capacity=1, every=1, fields=("u",), **img)
                rec_ms = event_ms(lambda: (ctx.frames_rewind(), ctx.frames_record()), stream, reps)
                ctx.frames_end()
                one_ms = event_ms(lambda: ctx.frame(fields=("u",), device=True, **img), stream, reps)
                tau = ctx.transfer(source="u", device=True, **img)[1]
                med = float(tau[tau > 0].median())
                tr_ms = event_ms(lambda: ctx.transfer(source="u", kappa_scale=0.01 / med, device=True, **img), stream, reps)
                out["rows"].append({"h": "own" if variable else "fixed", "view": tag, "size": size, "record_ms": round(rec_ms, 4),
                                    "frame_dev_ms": round(one_ms, 4), "transfer_thin_ms": round(tr_ms, 4), "pairs": round(pairs),
                                    "pairs_per_s": round(pairs / rec_ms * 1e3), "lit": int((tau > 0).sum())})
        ctx.close()
    return out


def mode_one(n, size, reps):
    import torch
    from summersph_amd import cube as cb
    from cube_time import event_ms
    ctx, gas = disc_context(n)
    ctx.density()
    rot = cb.view(40.0, 30.0)
    P = np.stack([gas["x"], gas["y"], gas["z"]], axis=1) @ rot.T
    ext = float(np.abs(P[:, :2]).max())
    ctx.frames_begin(capacity=1, every=1, fields=("u",), shape=(size, size), bounds=((-ext, -ext), (ext, ext)), rot=rot)
    stream = torch.cuda.ExternalStream(ctx.stream(), device=torch.device("cuda", 0))
    ms = event_ms(lambda: (ctx.frames_rewind(), ctx.frames_record()), stream, reps)
    ctx.close()
    return {"mode": "one", "n": n, "size": size, "reps": reps, "record_ms": ms}


def child(args, env, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *[str(a) for a in args]], env=env, capture_output=True, text=True,
                       timeout=timeout, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def mode_splat(n, reps, rounds):
    got = {"window": [], "plain": []}
    for _ in range(rounds):
        for form in ("window", "plain"):
            env = dict(os.environ)
            env.pop("SPH_FRAMES_SPLAT", None)
            if form == "plain":
                env["SPH_FRAMES_SPLAT"] = "plain"
            got[form].append(child(["frame", n, reps], env)["rows"])
    rows = []
    for k, r in enumerate(got["window"][0]):
        w = [g[k]["record_ms"] for g in got["window"]]
        p = [g[k]["record_ms"] for g in got["plain"]]
        rows.append({"h": r["h"], "view": r["view"], "size": r["size"], "pairs": r["pairs"], "window_ms": w, "plain_ms": p,
                     "plain_over_window": round(float(np.mean(p) / np.mean(w)), 3)})
    return {"mode": "splat", "n": n, "reps": reps, "rounds": rounds, "rows": rows}


def disc_context(n):
    from summersph_amd import capi, ic
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    return ctx, gas


def mode_steps(n, steps, reps, variants=("off", "every1", "every10", "dt10")):
    ctxs, clock, ms = {}, {}, {}
    for name in variants:
        ctxs[name], gas = disc_context(n)
        clock[name] = list(ctxs[name].run(6, 1e-2, 0.0))
        ext = float(max(np.abs(gas["x"]).max(), np.abs(gas["y"]).max()))
        img = dict(shape=(256, 256), bounds=((-ext, -ext), (ext, ext)), fields=("u",), capacity=steps * reps + 1)
        if name.startswith("every"):
            ctxs[name].frames_begin(every=int(name[5:]), **img)
        elif name == "dt10":
            ctxs[name].frames_begin(dt_frame=10.0 * clock[name][0], **img)
        ms[name] = []
    for _ in range(reps):
        for name in variants:                                # alternated
            c = ctxs[name]
            c.synchronize()
            t0 = time.perf_counter()
            clock[name] = list(c.run(steps, *clock[name]))
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {"mode": "steps", "n": n, "steps_per_run": steps, "tree": "other" if os.environ.get("SUMMERSPH_TREE") else "this"}
    for name in variants:
        out[name] = stat(ms[name])
        out[name]["t_end"] = clock[name][1]
        if name != "off":
            out[name]["frames"] = ctxs[name].frames_info()
            out[name]["overhead_pct"] = 100.0 * (out[name]["mean_ms"] / out["off"]["mean_ms"] - 1.0)
        ctxs[name].close()
    return out


def alternate(run, rounds, other):
    got = {"other": [], "this": []}
    for _ in range(rounds):
        for who in ("other", "this"):
            got[who].append(run(who, os.path.abspath(other)))
    o, m = np.array(got["other"]), np.array(got["this"])
    return {"other_ms_per_step": got["other"], "this_ms_per_step": got["this"], "other_mean": float(o.mean()),
            "this_mean": float(m.mean()), "other_spread": float(o.max() - o.min()), "difference": float(m.mean() - o.mean())}


def mode_ab(n, steps, reps, rounds, other):
    def run(who, tree):
        env = dict(os.environ)
        env.pop("SUMMERSPH_TREE", None)
        if who == "other":
            env["SUMMERSPH_TREE"] = tree
        return child(["off", n, steps, reps], env, 600)["off"]["mean_ms"]
    return {"mode": "ab", "n": n, "steps_per_run": steps, "reps": reps, **alternate(run, rounds, other)}


def mode_bench(rounds, other):
    def run(who, tree):
        cwd = tree if who == "other" else ROOT
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-variable", "--no-extras",
                            "--no-cpu"], cwd=cwd, capture_output=True, text=True, timeout=900, check=True)
        return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]
    return {"mode": "bench", **alternate(run, rounds, other)}


def main():
    a = sys.argv[1:]
    mode = a[0] if a else ""
    if mode == "frame":
        out, rest = mode_frame(int(a[1]), int(a[2])), a[3:]
    elif mode == "one":
        out, rest = mode_one(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "splat":
        out, rest = mode_splat(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "steps":
        out, rest = mode_steps(int(a[1]), int(a[2]), int(a[3])), a[4:]
    elif mode == "off":
        out, rest = mode_steps(int(a[1]), int(a[2]), int(a[3]), variants=("off",)), a[4:]
    elif mode == "ab":
        out, rest = mode_ab(int(a[1]), int(a[2]), int(a[3]), int(a[4]), a[5]), a[6:]
    elif mode == "bench":
        out, rest = mode_bench(int(a[1]), a[2]), a[3:]
    else:
        sys.exit(__doc__)
    print(json.dumps(out))
    if rest and rest[0] != "-":
        with open(rest[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
