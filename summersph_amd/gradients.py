"""SPH gradients of a save file on the GPU: vorticity, divergence and the gradient of any field at every gas particle.

    python -m summersph_amd.gradients SAVE.txt -o OUT.npz [--variable] [--fields vx,vy,vz] [--standard] [--h H]
                                      [--clip x0,y0,z0,x1,y1,z1] [--json]

SAVE.txt is a save file as for `python -m summersph_amd.profile`: records of 9 values (10 with --variable: .. alpha h)
are gas, records of 8 values are sinks.  The gas and the sinks are uploaded into a fresh context; sph_density runs only
when rho, P or c is asked for.  sph_gradients (capi.Context.gradients) then gives the gradients of up to four fields
(SPH_F_* names) in the matrix-corrected form (--standard: the difference form b / rho~), with each particle's own h or
one h for all (--h), at the gas particles strictly inside --clip.

OUT.npz holds `grad_<field>` of shape (3, n) per field (NaN rows outside the clip and, corrected, at singular
particles), `rho_sph` (rho~ of the gradient's own gather), `n_targets`, `n_singular`, and with vx, vy and vz all asked
for `divv` (n,) and `curl` (3, n); the descriptor used is in the `desc_*` entries.  --json prints the counts and the
median |div v| and omega_z as one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from . import cli
from .cli import STATE, desc_arrays, parse_clip, read_save, uploaded_context


def parse_fields(spec: str, variable: bool = False):
    """'vx,vy,vz' -> ['vx', 'vy', 'vz']: 1 .. 4 field names of capi.FIELDS (h and omega only with variable h)"""
    from . import capi
    return cli.parse_fields(spec, 1, capi.GRAD_MAX_FIELDS, variable, blanks=True)


def gradients_rows(gas, sinks, fields=("vx", "vy", "vz"), corrected=True, h=None, clip=None, variable=False, device=0):
    """Uploads the rows into a fresh context and evaluates the gradients: (grad (K, 3, n), rho~, counts, descriptor)."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        if any(f not in STATE + ["h"] for f in fields):
            ctx.density()                   # rho, P, c (and the rates' fields only after forces: stale otherwise)
        g, rho, counts = ctx.gradients(fields=fields, corrected=corrected, h=h, clip=clip, rho=True)
        return g, rho, counts, ctx.gradients_desc


def main(argv=None) -> int:
    from . import capi
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.gradients", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--fields", default="vx,vy,vz", help="1 .. 4 comma-separated field names")
    ap.add_argument("--standard", action="store_true", help="the difference form b / rho~ instead of the corrected form")
    ap.add_argument("--h", type=float, default=None, help="one h for every particle (default: each particle's own)")
    ap.add_argument("--clip", default=None, help="x0,y0,z0,x1,y1,z1 (strict)")
    ap.add_argument("--json", action="store_true", help="print the counts and medians as one JSON line")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        fields = parse_fields(a.fields, a.variable)
        clip = None if a.clip is None else parse_clip(a.clip)
    except ValueError as e:
        ap.error(str(e))
    if a.h is not None and not (np.isfinite(a.h) and a.h > 0):
        ap.error("--h must be finite and > 0")

    gas, sinks = read_save(a.save, a.variable)
    g, rho, (nt, ns), d = gradients_rows(gas, sinks, fields, not a.standard, a.h, clip, a.variable, a.device)
    out = {f"grad_{f}": g[k] for k, f in enumerate(fields)}
    out.update(rho_sph=rho, n_targets=np.array(nt), n_singular=np.array(ns))
    summary = {"n_targets": nt, "n_singular": ns}
    if all(f in fields for f in ("vx", "vy", "vz")):
        v = capi.velocity_derivatives(np.stack([g[fields.index(f)] for f in ("vx", "vy", "vz")]))
        out.update(divv=v["divv"], curl=v["curl"])
        ok = np.isfinite(v["divv"])
        summary["median_abs_divv"] = float(np.median(np.abs(v["divv"][ok]))) if ok.any() else None
        summary["median_omega_z"] = float(np.median(v["curl"][2][ok])) if ok.any() else None
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: gradients of {','.join(fields)} at {nt} of {gas.shape[0]} gas rows ({ns} singular, "
              f"{'standard' if a.standard else 'corrected'} form)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
