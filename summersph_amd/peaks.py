"""Density-peak clumps of a save file on the GPU: the basins of the density field, merged across high saddles (where
friends-of-friends percolates through a disc, this separates a fragment from the arm it sits in).

    python -m summersph_amd.peaks SAVE.txt -o OUT.npz [--csv OUT.csv] [--json] [--variable] --link B [--link-h]
                                  [--contrast C] [--rho-min R] [--peak-min P] [--min-members K]
                                  [--clip x0,y0,z0,x1,y1,z1] [--top T]
                                  [--bound [--thermal] [--unbind ROUNDS] [--bound-h H] [--max-members N]]

SAVE.txt is a save file as for `python -m summersph_amd.groups`.  The gas and the sinks are uploaded into a fresh
context, sph_density gives rho, and sph_peaks (capi.Context.peaks) lets every selected particle climb to its densest
neighbour within B (--link-h: B max(h_i, h_j)); two basins merge when the lower one's peak is below C times their saddle
(--contrast, default 2; 1: the raw basins; inf: the friends-of-friends groups).  Selected: rho >= --rho-min, strictly
inside --clip.  Clumps whose peak is below --peak-min or with fewer than --min-members members are dropped.

OUT.npz holds `labels` (int32 per gas row: the clump number, -1 in none), every table column by name
(capi.PEAKS_COLUMNS, one value per clump, largest first), `n_groups`, `counts` (capi.PEAKS_COUNTS) and the descriptor
used (`desc_*`).  --csv also writes the table as text; --json prints the counts and the table of the --top largest clumps
as one JSON line.  --bound, --thermal, --unbind, --bound-h and --max-members: as `python -m summersph_amd.groups`.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .cli import desc_arrays, parse_clip, read_save, uploaded_context


def peaks_rows(gas, sinks, link, contrast=2.0, rho_min=-np.inf, peak_min=-np.inf, min_members=1, link_h=False, clip=None,
               variable=False, device=0, bound=None):
    """Uploads the rows into a fresh context, evaluates rho and finds the clumps: (labels, table, n_groups, counts,
    descriptor); with bound (a dict of Context.bound's keyword arguments) a sixth entry, what Context.bound returns."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        ctx.density()
        labels, table, ng, counts = ctx.peaks(link, contrast=contrast, rho_min=rho_min, peak_min=peak_min,
                                              min_members=min_members, link_h=link_h, clip=clip)
        if bound is None:
            return labels, table, ng, counts, ctx.peaks_desc
        return labels, table, ng, counts, ctx.peaks_desc, ctx.bound(labels, ng, **bound)


def main(argv=None) -> int:
    from . import capi
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.peaks", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--csv", default=None, help="also write the table as CSV")
    ap.add_argument("--json", action="store_true", help="print the counts and the largest clumps as one JSON line")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--link", type=float, required=True, help="neighbour radius (--link-h: in units of h)")
    ap.add_argument("--link-h", action="store_true", help="link * max(h_i, h_j)")
    ap.add_argument("--contrast", type=float, default=2.0, help="merge when rho(lower peak) < contrast * saddle (>= 1)")
    ap.add_argument("--rho-min", type=float, default=-np.inf)
    ap.add_argument("--peak-min", type=float, default=-np.inf, help="drop clumps whose peak is below this")
    ap.add_argument("--min-members", type=int, default=1)
    ap.add_argument("--clip", default=None, help="x0,y0,z0,x1,y1,z1 (strict)")
    ap.add_argument("--top", type=int, default=20, help="clumps in the --json table")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bound", action="store_true", help="binding energies of the clumps (sph_bound)")
    ap.add_argument("--thermal", action="store_true", help="--bound: e includes u")
    ap.add_argument("--unbind", type=int, default=0, metavar="ROUNDS", help="--bound: removals of unbound members allowed")
    ap.add_argument("--bound-h", type=float, default=None, metavar="H", help="--bound: one softening length for every member")
    ap.add_argument("--max-members", type=int, default=2**31 - 1, metavar="N", help="--bound: skip larger clumps")
    a = ap.parse_args(argv)
    try:
        clip = None if a.clip is None else parse_clip(a.clip)
    except ValueError as e:
        ap.error(str(e))
    if not (np.isfinite(a.link) and a.link > 0):
        ap.error("--link must be finite and > 0")
    if not a.contrast >= 1:
        ap.error("--contrast must be >= 1")
    if np.isnan(a.rho_min) or np.isnan(a.peak_min):
        ap.error("--rho-min or --peak-min is NaN")
    if a.min_members < 1 or a.top < 0:
        ap.error("--min-members must be >= 1 and --top >= 0")
    if not a.bound and (a.thermal or a.unbind != 0 or a.bound_h is not None or a.max_members != 2**31 - 1):
        ap.error("--thermal, --unbind, --bound-h and --max-members need --bound")
    if a.unbind < 0 or a.max_members < 1:
        ap.error("--unbind must be >= 0 and --max-members >= 1")
    if a.bound_h is not None and not (np.isfinite(a.bound_h) and a.bound_h > 0):
        ap.error("--bound-h must be finite and > 0")
    bound = None
    if a.bound:
        bound = {"h": a.bound_h, "thermal": a.thermal, "max_rounds": a.unbind, "min_members": a.min_members,
                 "max_members": a.max_members}

    gas, sinks = read_save(a.save, a.variable)
    res = peaks_rows(gas, sinks, a.link, a.contrast, a.rho_min, a.peak_min, a.min_members, a.link_h, clip, a.variable,
                     a.device, bound)
    labels, table, ng, counts, d = res[:5]
    out = {"labels": labels, "n_groups": np.array(ng), "counts": np.array(counts, dtype=np.int64)}
    if a.bound:
        bl, e, phi, btab, bcnt = res[5]
        out.update({"bound_labels": bl, "e": e, "phi": phi, "bound_counts": np.array(bcnt, dtype=np.int64),
                    "bound_table": np.ascontiguousarray(btab).view(np.float64).reshape(-1, capi.BOUND_NCOL)})
    out.update({c: np.ascontiguousarray(table[c]) for c in capi.PEAKS_COLUMNS})
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    if a.csv:
        np.savetxt(a.csv, np.stack([table[c] for c in capi.PEAKS_COLUMNS], axis=1).reshape(-1, capi.PEAKS_NCOL),
                   delimiter=",", header=",".join(capi.PEAKS_COLUMNS), comments="")
    if a.json:
        top = table[:a.top]
        js = {"n_groups": ng, "counts": dict(zip(capi.PEAKS_COUNTS, (int(v) for v in counts))), "columns": capi.PEAKS_COLUMNS,
              "table": [[float(r[c]) for c in capi.PEAKS_COLUMNS] for r in top]}
        if a.bound:
            js["bound"] = {"counts": dict(zip(capi.BOUND_COUNTS, (int(v) for v in bcnt))), "columns": capi.BOUND_COLUMNS,
                           "table": [[float(r[c]) for c in capi.BOUND_COLUMNS] for r in btab[:a.top]]}
        print(json.dumps(js))
    else:
        print(f"{a.out}: {ng} clumps from {gas.shape[0]} gas rows ({sinks.shape[0]} sinks), "
              f"{int(np.sum(labels >= 0))} particles in clumps, {counts[1]} raw peaks, {counts[2]} saddles")
    return 0


if __name__ == "__main__":
    sys.exit(main())
