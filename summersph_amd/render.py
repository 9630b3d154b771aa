"""Density images of a save file on the GPU: the reference's imaging script (Density_Image.py) as a command.

    python -m summersph_amd.render SAVE.txt -o OUT.npy [--res N] [--h H] [--axis z] [--clip C] [--spacing]
                                   [--script-compat] [--png OUT.png]
                                   [--field {u,vx,vy,vz,alpha} [--field-sum] [--weight-out W.npy]]

SAVE.txt is a file in make_save's layout (SUMMER_SPH.f90:719-738): one header line, then one record per line; records
of 9 values are gas (x y z vx vy vz u m alpha), records of 8 are sinks (never rendered).  The gas rows are uploaded
into a fresh context and rendered with sph_render_density (capi.Context.render_density): the SPH interpolant
sum_j m_j W(|g - r_j|, h) with the analytic cubic spline and the double-precision pi -- the script's kernel, which is
not the simulation's REAL(4)-pi table, so an image is not the rho field.

--field renders that save-file column instead of the density with sph_render_field (Context.render_field): mass-
weighted and normalised, sum m A W / sum m W, i.e. along an axis the density-weighted line-of-sight mean (a temperature
map for u, a moment-1 map for the line-of-sight velocity).  --field-sum writes the plain sum m A W (times the node
spacing with --spacing) instead; --weight-out writes the weight sum m W (with --spacing, times the spacing) so that
images of separate files can be combined.  --field is refused with --script-compat (the script renders density only).

Defaults: 120 nodes per axis between the particles' min and max (np.linspace), each particle's own h (the context's
params.h), column sums along z.  --axis none writes the 3-D grid (x slowest).

--script-compat reproduces the script's pipeline, in its order:
  1. the clip |x|, |y|, |z| < 100 (strict);
  2. the LAST GAS ROW THAT SURVIVED THE CLIP is dropped.  The script calls that row "the sun" (it plots it as a red
     dot): in a save file the sinks come last, but the script reads only 9-value rows, so the row it drops is an
     ordinary gas particle.  This is a quirk of the script, kept here so that the images agree;
  3. bounds = min / max of what is left, 120 nodes per axis, h = 1.25, plain sums along z (no dz factor).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

SCRIPT_CLIP = 100.0
SCRIPT_RES = 120
SCRIPT_H = 1.25


def read_save(path: str):
    """(gas rows (n, 9), sink rows (ns, 8), number of skipped lines): 9-value records are gas, 8-value ones sinks; the
    header line is skipped, and so is every line with another number of values (as the script does)."""
    gas, sinks, skipped = [], [], 0
    with open(path) as f:
        f.readline()
        for line in f:
            tok = line.split()
            if len(tok) == 9:
                gas.append([float(t) for t in tok])
            elif len(tok) == 8:
                sinks.append([float(t) for t in tok])
            elif tok:
                skipped += 1
    return np.asarray(gas, dtype=np.float64).reshape(-1, 9), np.asarray(sinks, dtype=np.float64).reshape(-1, 8), skipped


def clip_mask(gas: np.ndarray, clip: float) -> np.ndarray:
    return np.all((gas[:, :3] < clip) & (gas[:, :3] > -clip), axis=1)


def script_rows(gas: np.ndarray) -> np.ndarray:
    """The gas rows Density_Image.py renders: the |coord| < 100 clip, then without the last surviving row."""
    return gas[clip_mask(gas, SCRIPT_CLIP)][:-1]


FIELD_COLUMNS = ["u", "vx", "vy", "vz", "alpha"]


def render_rows(gas: np.ndarray, res=SCRIPT_RES, h=None, axis="z", clip=None, spacing=False, device=0, field=None,
                normalise=True, weight_out=False):
    """Uploads the gas rows into a fresh fixed-h context and renders them; returns (image, (lo, hi)), or with a field and
    weight_out=True ((image, weight), (lo, hi)).  field: None = the density, else a save-file column (FIELD_COLUMNS)."""
    from . import capi
    ctx = capi.Context(device=device)
    try:
        ctx.upload({k: gas[:, i] for i, k in enumerate("x y z vx vy vz u m alpha".split())})
        cb = None if clip is None else ((-clip,) * 3, (clip,) * 3)
        ax = None if axis in (None, "none") else axis
        if field is None:
            img = ctx.render_density(res, axis=ax, h=h, clip=cb, spacing=spacing)
        else:
            img = ctx.render_field(field, res, axis=ax, h=h, clip=cb, spacing=spacing, weight="mass", normalise=normalise,
                                   weight_out=weight_out)
        return img, ctx.render_bounds
    finally:
        ctx.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file (make_save layout)")
    ap.add_argument("-o", "--out", required=True, help="output .npy")
    ap.add_argument("--res", type=int, default=SCRIPT_RES, help="nodes per axis (default 120)")
    ap.add_argument("--h", type=float, default=None, help="one smoothing length for all particles (default: their own)")
    ap.add_argument("--axis", default="z", choices=["x", "y", "z", "none"], help="projection axis; none: the 3-D grid")
    ap.add_argument("--clip", type=float, default=None, help="render only particles with |x|, |y|, |z| < CLIP")
    ap.add_argument("--spacing", action="store_true", help="multiply the column sums by the node spacing")
    ap.add_argument("--script-compat", action="store_true", help="Density_Image.py's exact pipeline (see the module text)")
    ap.add_argument("--png", default=None, help="also write an image (needs matplotlib)")
    ap.add_argument("--field", default=None, choices=FIELD_COLUMNS,
                    help="render this column, mass-weighted and normalised (the line-of-sight mean), instead of the density")
    ap.add_argument("--field-sum", action="store_true", help="with --field: the plain sum m A W, not normalised")
    ap.add_argument("--weight-out", default=None, help="with --field: also write the weight sum m W to this .npy")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.field and a.script_compat:
        ap.error("--field cannot be combined with --script-compat: the script renders density only")
    if (a.field_sum or a.weight_out) and not a.field:
        ap.error("--field-sum and --weight-out need --field")

    plt = None
    if a.png:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("--png needs matplotlib, which is not importable here", file=sys.stderr)
            return 2
    gas, sinks, skipped = read_save(a.save)
    if skipped:
        print(f"{a.save}: {skipped} lines with neither 9 nor 8 values skipped", file=sys.stderr)
    if a.script_compat:
        rows = script_rows(gas)
        img, (lo, hi) = render_rows(rows, res=SCRIPT_RES, h=SCRIPT_H, axis="z", clip=SCRIPT_CLIP, device=a.device)
        axis = "z"
    else:
        rows = gas
        img, (lo, hi) = render_rows(rows, res=a.res, h=a.h, axis=a.axis, clip=a.clip, spacing=a.spacing, device=a.device,
                                    field=a.field, normalise=not a.field_sum, weight_out=bool(a.weight_out))
        axis = a.axis
    if a.weight_out:
        img, wimg = img
        np.save(a.weight_out, wimg)
    np.save(a.out, img)
    print(f"{a.out}: {img.shape} from {rows.shape[0]} gas rows ({sinks.shape[0]} sink rows not rendered), "
          f"box {lo.tolist()} .. {hi.tolist()}, max {float(img.max()) if img.size else 0.0:.6e}")
    if plt is not None:
        if img.ndim != 2:
            print("--png needs a projection (--axis x|y|z)", file=sys.stderr)
            return 2
        a0, a1 = [k for k in range(3) if k != "xyz".index(axis)]
        if a.field is None:
            plt.imshow(img.T, origin="lower", extent=[lo[a0], hi[a0], lo[a1], hi[a1]], cmap="inferno")
            plt.colorbar(label="Integrated Density")
            plt.title(f"Integrated SPH Density (Projection along {axis.upper()})")
        else:                                          # a linear scale; velocities symmetric about 0
            what = f"{'sum m W' if a.field_sum else 'mass-weighted mean'} of {a.field}"
            if a.field.startswith("v"):
                vmax = float(np.max(np.abs(img))) or 1.0
                plt.imshow(img.T, origin="lower", extent=[lo[a0], hi[a0], lo[a1], hi[a1]], cmap="RdBu_r", vmin=-vmax, vmax=vmax)
            else:
                plt.imshow(img.T, origin="lower", extent=[lo[a0], hi[a0], lo[a1], hi[a1]], cmap="inferno")
            plt.colorbar(label=what)
            plt.title(f"SPH {what} (projection along {axis.upper()})")
        plt.xlabel("xyz"[a0]); plt.ylabel("xyz"[a1])
        plt.savefig(a.png, dpi=150)
        plt.close("all")
    return 0


if __name__ == "__main__":
    sys.exit(main())
