#!/usr/bin/env python3
"""Times sph_binned on a Keplerian disc beside sph_profile on the same disc and beside the host numpy
route (field downloads + np.bincount / np.histogram2d); run it under
`rocprofv3 --kernel-trace --stats -- python profiles/binned_time.py N [REPS [CASES]]` in a run of its own for the per-kernel times
(binned_keys, the rocprim sort, binned_starts, binned_pieces, binned_final; profile_* for the yardstick).

  N     gas particles of ic.keplerian_disc(N, seed=5) with its sink (default 10^6), after sph_density (cell-sorted order)
  REPS  timed repeats after one warm-up of every shape (default 5)
  CASES the cases to run, e.g. "ap" (default "pabc"): one case per profiled run keeps the kernel table of a case apart

Cases:
  a  64 log bins of a caller row R, weight mass, 8 context fields as quantities + squares (18 sums per bin)
  b  256 x 256 bins of rho (log) x u, one quantity (alpha)
  c  the 16 rows of sph_force_terms_dev as quantities, binned over rho (64 log bins) in two calls of 8, device form
  p  the yardstick: sph_profile, 64 log rings about the sink (20 sums per bin)
Every wall time is a host clock around calls that end in a synchronise (the host form's own read-back; sph_synchronize
after the device form).  Prints one JSON line: per case the mean, minimum and maximum over REPS of the host and device
forms in ms, and the numpy baselines (one run each)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402

EIGHT = ("x", "y", "z", "vx", "vy", "vz", "u", "alpha")


def nothing():
    """the host forms end in their own read-back"""


def timed(fn, sync, reps):
    fn(); sync()                                             # warm-up (scratch, code objects)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"mean_ms": float(np.mean(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    cases = sys.argv[3] if len(sys.argv) > 3 else "pabc"
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density()                                            # the cell-sorted order of a running simulation
    R = np.sqrt(gas["x"] * gas["x"] + gas["y"] * gas["y"])[None, :]
    r0, r1 = float(R.min()), float(R.max()) * 1.001
    Rd = torch.from_numpy(R).to("cuda:0")
    rho = ctx.field("rho")
    rr = (float(rho.min()), float(np.nextafter(rho.max(), np.inf)))
    out = {"n": ctx.n, "reps": reps, "cases": cases}
    if "p" in cases:
        case_p(ctx, out, reps, r0, r1)
    if "a" in cases:
        case_a(ctx, out, reps, r0, r1, R, Rd)
    if "b" in cases:
        case_b(ctx, out, reps, rr)
    if "c" in cases:
        case_c(ctx, out, reps, rr)
    print(json.dumps(out))
    ctx.close()


def case_p(ctx, out, reps, r0, r1):
    # p: the yardstick
    pa = dict(r_min=r0, r_max=r1, n_r=64, log=True, sink=0)
    out["p_profile_host"] = timed(lambda: ctx.profile(sums_only=True, **pa), nothing, reps)
    out["p_profile_device"] = timed(lambda: ctx.profile(device=True, **pa), ctx.synchronize, reps)


def case_a(ctx, out, reps, r0, r1, R, Rd):
    # a: 64 log rings of a caller row, 8 quantities + squares
    aa = dict(axes=capi.binned_row(0), bins=64, ranges=(r0, r1), log=(0,), q=EIGHT, weight="mass", squares=True)
    out["a_host"] = timed(lambda: ctx.binned(values=R, **aa), nothing, reps)
    out["a_device"] = timed(lambda: ctx.binned(values=Rd, device=True, **aa), ctx.synchronize, reps)
    sa, ca = ctx.binned(values=R, **aa)
    t0 = time.perf_counter()
    f = {k: ctx.field(k) for k in EIGHT + ("m",)}
    k = np.searchsorted(capi.binned_edges(ctx.binned_desc, None, 0), R[0], side="right") - 1
    k = np.where((R[0] >= r0) & (R[0] < r1), k, 64)
    cols = [np.ones(ctx.n), f["m"]] + [f["m"] * f[q] for q in EIGHT] + [f["m"] * (f[q] * f[q]) for q in EIGHT]
    base = np.stack([np.bincount(k, weights=w, minlength=65)[:64] for w in cols], axis=1)
    out["a_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    out["a_numpy_vs_gpu_max_rel"] = float(np.max(np.abs(base - sa[:, 0]) / np.maximum(np.abs(sa[:, 0]), 1e-300)))
    assert ca[0] == ctx.n - int(np.sum(R[0] >= r1))


def case_b(ctx, out, reps, rr):
    # b: the rho-u phase diagram
    ba = dict(axes=("rho", "u"), bins=(256, 256), ranges=(rr, (0.0, 1.0)), log=(0,), q=("alpha",), weight="mass")
    out["b_host"] = timed(lambda: ctx.binned(**ba), nothing, reps)
    out["b_device"] = timed(lambda: ctx.binned(device=True, **ba), ctx.synchronize, reps)
    sb, cb = ctx.binned(**ba)
    t0 = time.perf_counter()
    f = {k: ctx.field(k) for k in ("rho", "u", "m", "alpha")}
    ex, ey = (capi.binned_edges(ctx.binned_desc, None, a) for a in (0, 1))
    hw = np.histogram2d(f["rho"], f["u"], bins=(ex, ey), weights=f["m"])[0]
    hq = np.histogram2d(f["rho"], f["u"], bins=(ex, ey), weights=f["m"] * f["alpha"])[0]
    out["b_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    out["b_numpy_vs_gpu_max_abs_over_total"] = float(max(np.max(np.abs(hw - sb[..., 1])), np.max(np.abs(hq - sb[..., 2]))) / hw.sum())
    assert cb[0] == ctx.n


def case_c(ctx, out, reps, rr):
    # c: the force_terms rows over rho, device form, two calls of 8
    rows = ctx.force_terms(device=True)
    ca_ = dict(axes="rho", bins=64, ranges=rr, log=(0,), weight="mass", squares=False, values=rows, device=True)

    def both():
        ctx.binned(q=[capi.binned_row(k) for k in range(8)], **ca_)
        ctx.binned(q=[capi.binned_row(k) for k in range(8, 16)], **ca_)
    out["c_device_two_calls"] = timed(both, ctx.synchronize, reps)
    out["c_force_terms_device"] = timed(lambda: ctx.force_terms(device=True), ctx.synchronize, reps)
    t0 = time.perf_counter()
    host = ctx.force_terms()
    f = {k: ctx.field(k) for k in ("rho", "m")}
    k = np.searchsorted(capi.binned_edges(ctx.binned_desc, None, 0), f["rho"], side="right") - 1
    base = np.stack([np.bincount(k, weights=f["m"] * host[j], minlength=64)[:64] for j in range(16)])
    out["c_numpy_ms_with_the_download_of_the_rows"] = (time.perf_counter() - t0) * 1e3
    s0 = ctx.binned(q=[capi.binned_row(k) for k in range(8, 16)], **ca_)[0].cpu().numpy()
    out["c_numpy_vs_gpu_max_rel_duP"] = float(np.max(np.abs(base[12] - s0[:, 0, 2 + 4])) / np.max(np.abs(base[12])))


if __name__ == "__main__":
    main()
