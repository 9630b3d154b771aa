"""Friends-of-friends groups (clumps) of a save file on the GPU: which particles form them, how many there are, and
their mass, size, spin and bulk motion.

    python -m summersph_amd.groups SAVE.txt -o OUT.npz [--csv OUT.csv] [--json] [--variable] --link B [--link-h]
                                   [--rho-min R] [--min-members K] [--clip x0,y0,z0,x1,y1,z1] [--top T]
                                   [--bound [--thermal] [--unbind ROUNDS] [--bound-h H] [--max-members N]]

SAVE.txt is a save file as for `python -m summersph_amd.profile`: records of 9 values (10 with --variable: .. alpha h)
are gas, records of 8 values are sinks.  The gas and the sinks are uploaded into a fresh context, sph_density gives rho,
and sph_groups (capi.Context.groups) links every two selected particles closer than B (--link-h: B max(h_i, h_j)).
Selected: rho >= --rho-min, strictly inside --clip.  Components with fewer than --min-members members are dropped.

OUT.npz holds `labels` (int32 per gas row: the group number, -1 in none), every table column by name
(capi.GROUPS_COLUMNS, one value per group, largest first), `n_groups` and the descriptor used (`desc_*`).  --csv also
writes the table as text; --json prints the count and the table of the --top largest groups as one JSON line.

--bound asks of every group whether it is gravitationally bound (sph_bound, capi.Context.bound): the group's own softened
potential by a direct pair sum, e = 0.5 |v - V|^2 + Phi per member (--thermal: + u), and with --unbind ROUNDS up to that
many removals of the members with e >= 0 (a set that falls below --min-members dissolves).  --bound-h H: one softening
length instead of each particle's own h; --max-members N: larger groups are skipped (the cost is the sum of N^2).
OUT.npz then also holds `bound_labels`, `e`, `phi`, `bound_table` (n_groups x capi.BOUND_COLUMNS) and `bound_counts`
(capi.BOUND_COUNTS), and --json a "bound" entry: the counts and the rows of the --top largest groups.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .cli import desc_arrays, parse_clip, read_save, uploaded_context


def groups_rows(gas, sinks, link, rho_min=-np.inf, min_members=1, link_h=False, clip=None, variable=False, device=0,
                bound=None):
    """Uploads the rows into a fresh context, evaluates rho and finds the groups: (labels, table, n_groups, descriptor);
    with bound (a dict of Context.bound's keyword arguments) a fifth entry, what Context.bound returns for these groups."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        ctx.density()
        labels, table, ng = ctx.groups(link, rho_min=rho_min, min_members=min_members, link_h=link_h, clip=clip)
        if bound is None:
            return labels, table, ng, ctx.groups_desc
        return labels, table, ng, ctx.groups_desc, ctx.bound(labels, ng, **bound)


def main(argv=None) -> int:
    from . import capi
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.groups", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--csv", default=None, help="also write the table as CSV")
    ap.add_argument("--json", action="store_true", help="print the count and the largest groups as one JSON line")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--link", type=float, required=True, help="linking length (--link-h: in units of h)")
    ap.add_argument("--link-h", action="store_true", help="link * max(h_i, h_j)")
    ap.add_argument("--rho-min", type=float, default=-np.inf)
    ap.add_argument("--min-members", type=int, default=1)
    ap.add_argument("--clip", default=None, help="x0,y0,z0,x1,y1,z1 (strict)")
    ap.add_argument("--top", type=int, default=20, help="groups in the --json table")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bound", action="store_true", help="binding energies of the groups (sph_bound)")
    ap.add_argument("--thermal", action="store_true", help="--bound: e includes u")
    ap.add_argument("--unbind", type=int, default=0, metavar="ROUNDS", help="--bound: removals of unbound members allowed")
    ap.add_argument("--bound-h", type=float, default=None, metavar="H", help="--bound: one softening length for every member")
    ap.add_argument("--max-members", type=int, default=2**31 - 1, metavar="N", help="--bound: skip larger groups")
    a = ap.parse_args(argv)
    try:
        clip = None if a.clip is None else parse_clip(a.clip)
    except ValueError as e:
        ap.error(str(e))
    if not (np.isfinite(a.link) and a.link > 0):
        ap.error("--link must be finite and > 0")
    if np.isnan(a.rho_min):
        ap.error("--rho-min is NaN")
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
    res = groups_rows(gas, sinks, a.link, a.rho_min, a.min_members, a.link_h, clip, a.variable, a.device, bound)
    labels, table, ng, d = res[:4]
    out = {"labels": labels, "n_groups": np.array(ng)}
    if a.bound:
        bl, e, phi, btab, bcnt = res[4]
        out.update({"bound_labels": bl, "e": e, "phi": phi, "bound_counts": np.array(bcnt, dtype=np.int64),
                    "bound_table": np.ascontiguousarray(btab).view(np.float64).reshape(-1, capi.BOUND_NCOL)})
    out.update({c: np.ascontiguousarray(table[c]) for c in capi.GROUPS_COLUMNS})
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    if a.csv:
        np.savetxt(a.csv, np.stack([table[c] for c in capi.GROUPS_COLUMNS], axis=1).reshape(-1, capi.GROUPS_NCOL),
                   delimiter=",", header=",".join(capi.GROUPS_COLUMNS), comments="")
    if a.json:
        top = table[:a.top]
        js = {"n_groups": ng, "columns": capi.GROUPS_COLUMNS, "table": [[float(r[c]) for c in capi.GROUPS_COLUMNS] for r in top]}
        if a.bound:
            js["bound"] = {"counts": dict(zip(capi.BOUND_COUNTS, (int(v) for v in bcnt))), "columns": capi.BOUND_COLUMNS,
                           "table": [[float(r[c]) for c in capi.BOUND_COLUMNS] for r in btab[:a.top]]}
        print(json.dumps(js))
    else:
        print(f"{a.out}: {ng} groups from {gas.shape[0]} gas rows ({sinks.shape[0]} sinks), "
              f"{int(np.sum(labels >= 0))} particles in groups")
    return 0


if __name__ == "__main__":
    sys.exit(main())
