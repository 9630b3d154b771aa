"""Binned sums of a save file on the GPU: phase diagrams, distribution functions and the mean of any quantity against any
other, over one or two axes.

    python -m summersph_amd.binned SAVE.txt -o OUT.npz --x rho [--y u] --bins NX [NY] [--log x,y] [--xrange LO HI]
                                   [--yrange LO HI] [--weight one|mass|volume] [--q alpha,c] [--squares] [--variable]
                                   [--json]

SAVE.txt is a save file as summersph_amd.profile reads it (9-value gas records, 10 with --variable, 8-value sink records).
The gas and the sinks are uploaded into a fresh context and binned with sph_binned (capi.Context.binned): an axis or a
quantity is any field of capi.FIELDS.  A derived field (rho, P, c, omega, or --weight volume) has sph_density run first, a
rate (ax ay az du dalpha) sph_forces too.  A range defaults to the field's minimum and the next double above its maximum
(taken on the host), so that every particle is inside; with --log the minimum must be > 0.

OUT.npz holds `sums` (nx, ny, nsum: the raw sums, which add across files of one snapshot), `N`, `W`, `mean` and (with
--squares) `disp` as finish() returns them, `edges_x` (and `edges_y`: the tables the library used), `counts` (selected,
outside, dropped as NaN) and `q` (the quantities' names).  --json prints a one-line summary.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

DERIVED = ("rho", "P", "c", "omega")
RATES = ("ax", "ay", "az", "du", "dalpha")


def finish(sums, n_q, squares=False):
    """(N, W, mean, disp) of raw sums [..., nsum]: N the counts, W = sum w, mean[..., k] = (sum w A_k) / W and, with squares,
    disp[..., k] = sqrt(max(<A_k A_k> - <A_k>^2, 0)) (else None).  NaN where W == 0."""
    s = np.asarray(sums, dtype=np.float64)
    n_q = int(n_q)
    if s.shape[-1] != 2 + n_q * (2 if squares else 1):
        raise ValueError(f"finish: {s.shape[-1]} sums per bin for n_q = {n_q}, squares = {bool(squares)}")
    N, W = s[..., 0], s[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        Wd = np.where(W == 0.0, np.nan, W)[..., None]
        mean = s[..., 2:2 + n_q] / Wd
        disp = None
        if squares:
            disp = np.sqrt(np.maximum(s[..., 2 + n_q:2 + 2 * n_q] / Wd - mean * mean, 0.0))
    return N, W, mean, disp


def ring_radius(x, y, z, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """R of sph_profile's frame (include/summersph.h, "Frame"), numpy arrays or torch tensors, in its order of operations"""
    from .sample import frame
    _, e1, e2 = frame(normal)
    r = (x - float(centre[0]), y - float(centre[1]), z - float(centre[2]))
    X = (r[0] * float(e1[0]) + r[1] * float(e1[1])) + r[2] * float(e1[2])
    Y = (r[0] * float(e2[0]) + r[1] * float(e2[1])) + r[2] * float(e2[2])
    s = X * X + Y * Y
    return s.sqrt() if hasattr(s, "sqrt") else np.sqrt(s)


def ring_sums(ctx, rows, edges, which=(13, 12), centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), weight="mass", squares=False):
    """On the device what terms.ring_heating does on the host: the sums per ring of w * rows[k], k in `which` (default
    du_V and du_P of force_terms), over the owned gas with edges[j] <= R < edges[j + 1] in sph_profile's frame, NaN columns
    (non-targets) dropped.  rows: a (k, sph_count) float64 array in the upload order, numpy or (as force_terms(device=True)
    returns it) a torch tensor on the context's GPU, which then never leaves the device.  Returns (out, sums, counts): out
    (len(which), n_rings) = sum w A; sums the raw (n_rings, 1, nsum) sums; counts as Context.binned."""
    from . import capi
    which = tuple(int(k) for k in which)
    if not 0 < len(which) <= capi.BINNED_MAX_Q:
        raise ValueError(f"ring_sums: 1 .. {capi.BINNED_MAX_Q} rows")
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    n = ctx.n
    device = not isinstance(rows, np.ndarray)
    if device:
        import torch
        xyz = torch.empty((3, n), dtype=torch.float64, device=rows.device)
        torch.cuda.current_stream(rows.device).synchronize()   # the block may still be in use by torch's queued work
        for a, name in enumerate("xyz"):
            ctx.field_dev(name, xyz[a].data_ptr(), n)
        vals = torch.empty((1 + len(which), n), dtype=torch.float64, device=rows.device)
        vals[0] = ring_radius(xyz[0], xyz[1], xyz[2], centre, normal)
        for j, k in enumerate(which):
            vals[1 + j] = rows[k]
    else:
        vals = np.empty((1 + len(which), n))
        vals[0] = ring_radius(ctx.field("x"), ctx.field("y"), ctx.field("z"), centre, normal)
        for j, k in enumerate(which):
            vals[1 + j] = rows[k]
    sums, counts = ctx.binned(capi.binned_row(0), edges.size - 1, edges=edges, q=[capi.binned_row(1 + j) for j in range(len(which))],
                              weight=weight, values=vals, squares=squares, skip_nan=True, device=device)
    out = sums[:, 0, 2:2 + len(which)].T
    return out, sums, counts


def _axes_of(spec: str):
    ax = tuple(t for t in spec.split(",") if t)
    if not ax or any(t not in ("x", "y") for t in ax):
        raise ValueError(f"--log wants x, y or x,y, not {spec!r}")
    return ax


def parse_args(argv=None):
    from .capi import BINNED_MAX_Q, BINNED_WEIGHTS, FIELDS
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.binned", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--x", required=True, help="field of axis 0")
    ap.add_argument("--y", default=None, help="field of axis 1")
    ap.add_argument("--bins", type=int, nargs="+", required=True, help="bins per axis")
    ap.add_argument("--log", default="", help="x, y or x,y: logarithmic edges")
    ap.add_argument("--xrange", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--yrange", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--weight", default="mass", help="one, mass or volume")
    ap.add_argument("--q", default="", help="comma-separated fields to average")
    ap.add_argument("--squares", action="store_true", help="also the dispersions")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--json", action="store_true", help="print a one-line JSON summary")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        a.axes = (a.x,) if a.y is None else (a.x, a.y)
        a.q = tuple(t for t in a.q.split(",") if t)
        for name in a.axes + a.q:
            if name not in FIELDS:
                raise ValueError(f"unknown field {name!r} (one of {' '.join(FIELDS)})")
            if name in ("h", "omega") and not a.variable:
                raise ValueError(f"field {name!r} needs --variable")
        if len(a.q) > BINNED_MAX_Q:
            raise ValueError(f"at most {BINNED_MAX_Q} quantities")
        if a.weight not in BINNED_WEIGHTS:
            raise ValueError(f"--weight wants one of {' '.join(BINNED_WEIGHTS)}")
        if len(a.bins) != len(a.axes) or min(a.bins) < 1 or int(np.prod(a.bins)) > 2 ** 20:
            raise ValueError("--bins wants one count >= 1 per axis, their product <= 2^20")
        a.log = tuple("xy".index(t) for t in _axes_of(a.log)) if a.log else ()
        if a.y is None and (1 in a.log or a.yrange is not None):
            raise ValueError("--log y / --yrange without --y")
        a.ranges = [a.xrange, a.yrange][:len(a.axes)]
        for k, r in enumerate(a.ranges):
            if r is not None and (not np.all(np.isfinite(r)) or not r[0] < r[1] or (k in a.log and r[0] <= 0.0)):
                raise ValueError("a range wants finite LO < HI (LO > 0 on a logarithmic axis)")
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import capi
    from .cli import read_save, uploaded_context
    gas, sinks = read_save(a.save, a.variable)
    used = set(a.axes + a.q)
    with uploaded_context(gas, sinks, a.variable, a.device) as ctx:
        if used & set(DERIVED + RATES) or a.weight == "volume":
            ctx.density()
        if used & set(RATES):
            ctx.forces()
        ranges = []
        for k, name in enumerate(a.axes):
            r = a.ranges[k]
            if r is None:
                v = ctx.field(name)
                v = v[np.isfinite(v)]
                if v.size == 0:
                    print(f"binned: field {name} has no finite value", file=sys.stderr)
                    return 1
                r = (float(v.min()), float(np.nextafter(v.max(), np.inf)))
                if k in a.log and r[0] <= 0.0:
                    print(f"binned: --log on {name}, whose minimum is {r[0]}", file=sys.stderr)
                    return 1
            ranges.append(tuple(r))
        sums, counts = ctx.binned(a.axes, a.bins, ranges=ranges, log=a.log, q=a.q, weight=a.weight, squares=a.squares)
        d = ctx.binned_desc
        edges = [capi.binned_edges(d, None, k) for k in range(len(a.axes))]
    N, W, mean, disp = finish(sums, len(a.q), a.squares)
    out = {"sums": sums, "N": N, "W": W, "mean": mean, "counts": np.array(counts), "q": np.array(a.q, dtype=str),
           "edges_x": edges[0]}
    if len(edges) == 2:
        out["edges_y"] = edges[1]
    if disp is not None:
        out["disp"] = disp
    np.savez(a.out, **out)
    summary = {"gas": int(gas.shape[0]), "sinks": int(sinks.shape[0]), "axes": list(a.axes), "bins": list(a.bins),
               "ranges": [list(r) for r in ranges], "weight": a.weight, "q": list(a.q), "selected": counts[0],
               "outside": counts[1], "dropped": counts[2], "W": float(W.sum()), "occupied_bins": int((N > 0).sum())}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: {' x '.join(str(b) for b in a.bins)} bins of {' x '.join(a.axes)} from {gas.shape[0]} gas rows, "
              f"{counts[0]} selected, {counts[1]} outside, {counts[2]} dropped")
    return 0


if __name__ == "__main__":
    sys.exit(main())
