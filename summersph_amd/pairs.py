"""Pair statistics of a save file on the GPU: the pair distribution g(r) or g(r / h) (the pairing instability, particle
noise), the mean pairwise radial velocity, the longitudinal and transverse structure functions of the velocity field and
the variogram of any field.

    python -m summersph_amd.pairs SAVE.txt -o OUT.npz --r LO HI --bins N [--log] [--scale-h] [--velocity] [--q u,rho]
                                  [--weight one|mass] [--stride S] [--phase P] [--clip x0,y0,z0,x1,y1,z1] [--variable]
                                  [--json]

SAVE.txt is a save file as summersph_amd.profile reads it (9-value gas records, 10 with --variable, 8-value sink records).
The gas and the sinks are uploaded into a fresh context, sph_density runs (g needs rho) and sph_pairs (capi.Context.pairs)
sums over the ordered pairs (i, j), j != i, with LO <= r < HI (--scale-h: r / h_i).  --stride S takes every S-th particle
as a target (all particles stay sources): an unbiased estimate at 1 / S of the cost, which is how a large HI is afforded.

OUT.npz holds `sums` (n_bins, nsum: the doubles), `raw` and `exps` (the exact 128-bit sums, which add across phases, clip
boxes and files: add_raw), `edges`, `counts` (targets, sources, not usable), `g`, and the means finish() returns (`N`, `W`,
`dA`, `dA2`, and with --velocity `u`, `S2_par`, `S3_par`, `S2_perp`), `q` (the quantities' names).  --json prints a one-line
summary.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

DERIVED = ("rho", "P", "c", "omega")
RATES = ("ax", "ay", "az", "du", "dalpha")


def finish(sums, n_q, velocity=False):
    """The means per bin of raw sums [..., nsum] as a dict: N, W = sum w, dA[..., k] = <dA_k>, dA2[..., k] = <dA_k^2> and,
    with velocity, u = <u>, S2_par = <u^2>, S3_par = <u^3>, S2_perp = (<|dv|^2> - <u^2>) / 2.  NaN where W == 0."""
    s = np.asarray(sums, dtype=np.float64)
    n_q = int(n_q)
    if s.shape[-1] != 2 + 2 * n_q + (4 if velocity else 0):
        raise ValueError(f"finish: {s.shape[-1]} sums per bin for n_q = {n_q}, velocity = {bool(velocity)}")
    N, W = s[..., 0], s[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        Wd = np.where(W == 0.0, np.nan, W)
        out = {"N": N, "W": W, "dA": s[..., 2:2 + n_q] / Wd[..., None], "dA2": s[..., 2 + n_q:2 + 2 * n_q] / Wd[..., None]}
        if velocity:
            v = s[..., 2 + 2 * n_q:]
            out["u"] = v[..., 0] / Wd
            out["S2_par"] = v[..., 1] / Wd
            out["S3_par"] = v[..., 2] / Wd
            out["S2_perp"] = (v[..., 3] / Wd - out["S2_par"]) / 2.0
    return out


def add_raw(a, b):
    """The exact sum of two raw results (..., 2) uint64 {low, high} limbs of equal exponents: 128-bit two's-complement
    addition, the carry of the low limbs taken into the high ones."""
    a = np.asarray(a).view(np.uint64) if np.asarray(a).dtype == np.int64 else np.asarray(a, dtype=np.uint64)
    b = np.asarray(b).view(np.uint64) if np.asarray(b).dtype == np.int64 else np.asarray(b, dtype=np.uint64)
    if a.shape != b.shape or a.shape[-1] != 2:
        raise ValueError("add_raw: two arrays of {low, high} limbs of one shape")
    out = np.empty_like(a)
    with np.errstate(over="ignore"):
        out[..., 0] = a[..., 0] + b[..., 0]
        out[..., 1] = a[..., 1] + b[..., 1] + (out[..., 0] < a[..., 0]).astype(np.uint64)
    return out


def targets(pos, n_owned, clip=None, stride=1, phase=0, usable=None):
    """sph_pairs' target selection restated: a bool per particle in the upload order.  pos (n, 3); usable: None (finite
    positions) or the bool array of the particles whose requested quantities are all finite."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    idx = np.arange(n)
    t = (idx < int(n_owned)) & np.all(np.isfinite(pos), axis=1) & (idx % int(stride) == int(phase))
    if usable is not None:
        t &= np.asarray(usable, dtype=bool)
    if clip is not None:
        lo, hi = np.asarray(clip[0], dtype=np.float64), np.asarray(clip[1], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            t &= np.all((lo < pos) & (pos < hi), axis=1)
    return t


def rdf(ctx, sums, edges, scale_h=False, clip=None, stride=1, phase=0, n_owned=None):
    """g per bin: the counts N = sums[:, 0] over the count a uniform medium of each target's own number density would
    give, sum over the targets i of (rho_i / m_i) (4 pi / 3) (x_{b+1}^3 - x_b^3) (h_i^3 with scale_h), x the edges.  The
    targets are restated on the host (targets(); n_owned: the owned count, default all).  Needs a valid rho (SphError
    otherwise).  NaN where no pair is expected."""
    from . import capi
    e = np.asarray(edges, dtype=np.float64)
    pos = np.stack([ctx.field("x"), ctx.field("y"), ctx.field("z")], axis=1)
    rho, m = ctx.field("rho"), ctx.field("m")
    t = targets(pos, pos.shape[0] if n_owned is None else n_owned, clip, stride, phase)
    dens = rho[t] / m[t]
    if scale_h:
        h = ctx.field("h") if ctx.params.flags & capi.FLAG_VARIABLE_H else np.full(pos.shape[0], float(ctx.params.h))
        dens = dens * h[t] ** 3
    shell = (4.0 * np.pi / 3.0) * (e[1:] ** 3 - e[:-1] ** 3)
    expect = float(np.sum(dens)) * shell
    N = np.asarray(sums, dtype=np.float64)[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(expect > 0.0, N / expect, np.nan)


def parse_args(argv=None):
    from .capi import FIELDS, PAIRS_MAX_BINS, PAIRS_MAX_Q, PAIRS_WEIGHTS
    from .cli import parse_clip
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.pairs", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--r", type=float, nargs=2, required=True, metavar=("LO", "HI"), help="range of r (of r / h with --scale-h)")
    ap.add_argument("--bins", type=int, required=True, help="bins")
    ap.add_argument("--log", action="store_true", help="logarithmic bins (LO > 0)")
    ap.add_argument("--scale-h", action="store_true", help="bin r / h_i")
    ap.add_argument("--velocity", action="store_true", help="also the velocity structure functions")
    ap.add_argument("--q", default="", help="comma-separated fields whose increments are summed")
    ap.add_argument("--weight", default="one", help="one or mass")
    ap.add_argument("--stride", type=int, default=1, help="every stride-th particle is a target")
    ap.add_argument("--phase", type=int, default=0, help="which of them: 0 .. stride - 1")
    ap.add_argument("--clip", default=None, help="x0,y0,z0,x1,y1,z1: the targets' box")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--json", action="store_true", help="print a one-line JSON summary")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        a.q = tuple(t for t in a.q.split(",") if t)
        for name in a.q:
            if name not in FIELDS:
                raise ValueError(f"unknown field {name!r} (one of {' '.join(FIELDS)})")
            if name in ("h", "omega") and not a.variable:
                raise ValueError(f"field {name!r} needs --variable")
        if len(a.q) > PAIRS_MAX_Q:
            raise ValueError(f"at most {PAIRS_MAX_Q} quantities")
        if a.weight not in PAIRS_WEIGHTS:
            raise ValueError(f"--weight wants one of {' '.join(PAIRS_WEIGHTS)}")
        if not 1 <= a.bins <= PAIRS_MAX_BINS:
            raise ValueError(f"--bins wants 1 .. {PAIRS_MAX_BINS}")
        if not np.all(np.isfinite(a.r)) or not a.r[0] < a.r[1] or a.r[0] < 0.0 or (a.log and a.r[0] <= 0.0):
            raise ValueError("--r wants finite 0 <= LO < HI (LO > 0 with --log)")
        if a.stride < 1 or not 0 <= a.phase < a.stride:
            raise ValueError("--stride wants S >= 1 and --phase 0 .. S - 1")
        a.clip = None if a.clip is None else parse_clip(a.clip)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import capi
    from .cli import desc_arrays, read_save, uploaded_context
    gas, sinks = read_save(a.save, a.variable)
    with uploaded_context(gas, sinks, a.variable, a.device) as ctx:
        ctx.density()
        if set(a.q) & set(RATES):
            ctx.forces()
        sums, counts, exps, raw = ctx.pairs(a.r, a.bins, log=a.log, scale_h=a.scale_h, q=a.q, weight=a.weight, velocity=a.velocity,
                                            clip=a.clip, stride=a.stride, phase=a.phase, raw=True)
        d = ctx.pairs_desc
        edges = capi.pairs_edges(d)
        g = rdf(ctx, sums, edges, a.scale_h, a.clip, a.stride, a.phase)
    out = {"sums": sums, "raw": raw, "exps": exps, "edges": edges, "counts": np.array(counts), "g": g,
           "q": np.array(a.q, dtype=str)}
    out.update(finish(sums, len(a.q), a.velocity))
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    summary = {"gas": int(gas.shape[0]), "sinks": int(sinks.shape[0]), "bins": a.bins, "r": list(a.r), "log": a.log,
               "scale_h": a.scale_h, "velocity": a.velocity, "q": list(a.q), "weight": a.weight, "stride": a.stride,
               "phase": a.phase, "targets": counts[0], "sources": counts[1], "not_usable": counts[2],
               "pairs": int(sums[:, 0].sum())}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: {a.bins} bins of r{' / h' if a.scale_h else ''} in [{a.r[0]}, {a.r[1]}) from {gas.shape[0]} gas rows, "
              f"{counts[0]} targets, {counts[1]} sources, {summary['pairs']} pairs")
    return 0


if __name__ == "__main__":
    sys.exit(main())
