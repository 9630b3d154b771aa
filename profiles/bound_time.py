#!/usr/bin/env python3
"""Times sph_bound ("Binding energies and unbinding"); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/bound_time.py CASE` for the per-kernel times (bound_keys ...
bound_counts and the rocprim radix sort).

  CASE   disc   the friends-of-friends groups of ic.keplerian_disc(N, seed=5) (fixed h = 2.5, b = h, as section 11) with
                max_members below the percolating group: many small groups
         one    one Gaussian blob of N members, evaluated once: the pair rate
         halo   bound_ref's core + halo blob scaled to N members, max_rounds = 16
  N      members (default: disc 10^6, one and halo 10^5)
  REPS   timed calls (default 3)

Prints one JSON line: wall time per call of the host form (after one warm-up) and of the device form (synchronised),
the counts, the pair terms of one call (sum over groups and rounds of N_0 N_r, from the table; 'halo': from the
restatement's rounds where it ran) and the host baseline: download the members, then the numpy direct sum of
tests/bound_ref.py on the largest evaluated groups up to --host-members members in all (default 20000; the size the
baseline was timed at is printed, the rest is not extrapolated)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bound_ref  # noqa: E402
from summersph_amd import capi, ic  # noqa: E402


def blob(n, G, halo, seed=7):
    rng = np.random.default_rng(seed)
    v0 = np.sqrt(G * 0.01)
    p = rng.normal(0, 1.0, (n, 3))
    v = rng.normal(0, 0.1 * v0, (n, 3))
    if halo:
        nh = n // 2
        p[:nh] = rng.normal(0, 3.0, (nh, 3))
        d = rng.normal(size=(nh, 3))
        v[:nh] = d / np.linalg.norm(d, axis=1)[:, None] * (rng.uniform(0.0, 1.6, nh) * v0)[:, None]
    return {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy(), "vx": v[:, 0].copy(), "vy": v[:, 1].copy(),
            "vz": v[:, 2].copy(), "u": np.full(n, 1e-3), "m": np.full(n, 0.01 / n), "alpha": np.ones(n)}


def host_baseline(ctx, lab, ng, table, G, h, kw, budget):
    """the numpy direct sum on the downloaded members of the largest evaluated groups, budget members in all"""
    t0 = time.perf_counter()
    f = {k: ctx.field(k) for k in "x y z vx vy vz u m".split()}
    order = [g for g in np.argsort(-table["N0"], kind="stable") if table["status"][g] != 3]
    take, total = [], 0
    for g in order:
        if total + table["N0"][g] > budget and take:
            break
        take.append(int(g))
        total += int(table["N0"][g])
    sub = np.where(np.isin(lab, take), lab, -1).astype(np.int32)
    if total > budget:                                       # one group larger than the budget: its first members only
        ids = np.nonzero(sub >= 0)[0]
        sub[ids[budget:]] = -1
        total = budget
    res = bound_ref.bound(f, sub, ctx.n, ng, G, h, check_margin=False, **kw)
    return {"host_s": time.perf_counter() - t0, "host_members": total, "host_groups": len(take),
            "host_evaluations": int(res[5]["evaluations"].sum())}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    case = args[0] if args else "one"
    n = int(args[1]) if len(args) > 1 else (1_000_000 if case == "disc" else 100_000)
    reps = int(args[2]) if len(args) > 2 else 3
    budget = next((int(a.split("=")[1]) for a in sys.argv if a.startswith("--host-members=")), 20000)
    G = float(capi.default_params().G)
    if case == "disc":
        gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
        ctx = capi.Context(device=0)
        ctx.upload(gas)
        ctx.set_sinks(sinks)
        ctx.density()
        lab, gt, ng = ctx.groups(2.5, min_members=2)
        cap = int(gt["N"][1]) if ng > 1 else int(gt["N"][0])          # below the percolating group
        h, kw = 2.5, dict(max_rounds=4, max_members=cap)
    else:
        gas = blob(n, G, case == "halo")
        h = 0.3
        ctx = capi.Context(device=0, h=h)
        ctx.upload(gas)
        lab, ng = np.zeros(n, dtype=np.int32), 1
        kw = dict(max_rounds=16 if case == "halo" else 0)
    ctx.synchronize()
    out = {"case": case, "n": ctx.n, "n_groups": ng, **kw}
    ctx.bound(lab, ng, **kw)                                  # warm-up (scratch, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        bl, e, phi, tab, cnt = ctx.bound(lab, ng, **kw)
    out["host_ms"] = (time.perf_counter() - t0) / reps * 1e3
    import torch
    dl = torch.from_numpy(lab).to(f"cuda:{ctx.device}")
    ctx.bound(dl, ng, device=True, **kw)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.bound(dl, ng, device=True, **kw)
    ctx.synchronize()
    out["device_ms"] = (time.perf_counter() - t0) / reps * 1e3
    ev = tab["status"] != 3
    out.update({"counts": dict(zip(capi.BOUND_COUNTS, cnt)), "largest_evaluated": int(np.max(tab["N0"][ev], initial=0)),
                "rounds_max": int(np.nanmax(tab["rounds"][ev], initial=0)), "bound_members": int(np.sum(bl >= 0)),
                # every evaluation streams the N_0 members of the group past the live targets; an upper bound on the
                # pair terms of one call: (R + 1) N_0^2 per group
                "pair_terms_upper": float(np.sum((tab["rounds"][ev] + 1) * tab["N0"][ev] ** 2)),
                "pair_terms_round0": float(np.sum(tab["N0"][ev & (tab["N0"] >= kw.get("min_members", 1))] ** 2))})
    out.update(host_baseline(ctx, lab, ng, tab, G, h, {k: v for k, v in kw.items() if k != "max_members"}, budget))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
