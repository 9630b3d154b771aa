"""Emission-absorption images of a save file on the GPU (sph_transfer): what an observer sees of gas that is not optically
thin -- intensity, optical depth, transmission and the depth of the tau = tau_surface surface -- around Context.transfer.

    python -m summersph_amd.transfer save275.txt -o img.npz --inc 40 --pa 30 --extent 200 --size 256 --kappa-scale 50 \\
        --source u --tau-surface 1 --tau-max 30 --png img.png --json

The viewing conventions are the cube's (summersph_amd.cube.view): the rows of the viewing matrix are the image axes u^, v^
and the line of sight w^, which points AWAY from the observer, so the particles are composited in ascending depth
D = w^ . (r - centre).  The opacity of a particle is kappa_scale K_j and its source function S_j; --kappa and --source name
a field each, or `one` for the constant 1."""
import argparse
import json
import sys

import numpy as np

from .cli import read_save, uploaded_context
from .cube import parse_clip, parse_vec, view

DERIVED = ("rho", "P", "c", "omega")      # fields that need a density pass (the rates are never evaluated here)


def parse_input(name, variable=False):
    """--source / --kappa: `one` -> None (the constant 1), else a field name the call can read from a fresh context"""
    from . import capi
    if name == "one":
        return None
    allowed = [f for f in capi.FIELDS[:9] + list(DERIVED[:3]) + (["h", "omega"] if variable else [])]
    if name not in allowed:
        raise ValueError(f"{name!r}: `one` or one of {allowed}")
    return name


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.transfer", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz (intensity, tau, transmission, surface, u_nodes, v_nodes, rot)")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--inc", type=float, default=0.0, help="inclination in degrees (0: face-on)")
    ap.add_argument("--pa", type=float, default=0.0, help="position angle of the line of nodes in degrees")
    ap.add_argument("--azimuth", type=float, default=0.0, help="turn of the disc about z in degrees")
    ap.add_argument("--extent", type=float, required=True, help="full width of the square image (centred on --centre)")
    ap.add_argument("--size", type=int, default=256, help="image nodes per axis")
    ap.add_argument("--source", default="u", help="source function S: a field name or `one`")
    ap.add_argument("--kappa", default="one", help="opacity K per unit mass: a field name or `one`")
    ap.add_argument("--kappa-scale", type=float, default=1.0, help="the opacity is kappa-scale K")
    ap.add_argument("--tau-surface", type=float, default=1.0, help="the optical depth whose depth the surface plane records")
    ap.add_argument("--tau-max", type=float, default=np.inf, help="a pixel stops compositing at this optical depth")
    ap.add_argument("--background", type=float, default=0.0, help="intensity behind the gas")
    ap.add_argument("--centre", default="0,0,0", help="image centre x,y,z")
    ap.add_argument("--h", type=float, default=None, help="one h for every particle (default: each particle's own)")
    ap.add_argument("--clip", default=None, help="strict particle clip box x0,y0,z0,x1,y1,z1")
    ap.add_argument("--png", default=None, help="also write the intensity as an image (needs matplotlib)")
    ap.add_argument("--json", action="store_true", help="print a one-line JSON summary")
    ap.add_argument("--device", type=int, default=0)
    return ap


def args_desc(a):
    """Context.transfer's keyword arguments from the parsed command line"""
    if a.size < 1:
        raise ValueError("--size must be >= 1")
    if not (np.isfinite(a.extent) and a.extent > 0):
        raise ValueError("--extent must be finite and > 0")
    if a.h is not None and not (np.isfinite(a.h) and a.h > 0):
        raise ValueError("--h must be finite and > 0")
    if not (np.isfinite(a.kappa_scale) and a.kappa_scale >= 0):
        raise ValueError("--kappa-scale must be finite and >= 0")
    if not a.tau_surface > 0 or not a.tau_max > 0:
        raise ValueError("--tau-surface and --tau-max must be > 0")
    if not np.isfinite(a.background):
        raise ValueError("--background must be finite")
    half = 0.5 * a.extent
    return dict(shape=(a.size, a.size), bounds=((-half, -half), (half, half)), rot=view(a.inc, a.pa, a.azimuth),
                centre=parse_vec(a.centre), source=parse_input(a.source, a.variable), kappa=parse_input(a.kappa, a.variable),
                kappa_scale=a.kappa_scale, tau_surface=a.tau_surface, tau_max=a.tau_max, background=a.background, h=a.h,
                clip=None if a.clip is None else parse_clip(a.clip))


def transfer_rows(gas, sinks, kw, variable=False, device=0):
    """Uploads the rows into a fresh context and returns its image (Context.transfer(**kw))."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        if kw.get("source") in DERIVED or kw.get("kappa") in DERIVED:
            ctx.density()
        return ctx.transfer(**kw)


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        kw = args_desc(a)
    except ValueError as e:
        ap.error(str(e))
    plt = None
    if a.png:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("--png needs matplotlib, which is not importable here", file=sys.stderr)
            return 2
    gas, sinks = read_save(a.save, a.variable)
    img = transfer_rows(gas, sinks, kw, a.variable, a.device)
    (lo_u, lo_v), (hi_u, hi_v) = kw["bounds"]
    np.savez(a.out, intensity=img[0], tau=img[1], transmission=img[2], surface=img[3], u_nodes=np.linspace(lo_u, hi_u, a.size),
             v_nodes=np.linspace(lo_v, hi_v, a.size), rot=kw["rot"])
    lit = img[1] > 0
    summary = {"shape": list(img.shape), "pixels_lit": int(lit.sum()), "pixels_surface": int(np.isfinite(img[3]).sum()),
               "tau_max": float(img[1].max()), "intensity_max": float(img[0].max())}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: image {img.shape} from {gas.shape[0]} gas rows, {summary['pixels_lit']} pixels lit, "
              f"{summary['pixels_surface']} reach tau = {a.tau_surface:g}")
    if plt is not None:
        plt.imshow(img[0].T, origin="lower", extent=[lo_u, hi_u, lo_v, hi_v], cmap="inferno")
        plt.colorbar(label=f"intensity (S = {a.source})")
        plt.xlabel("u"); plt.ylabel("v")
        plt.savefig(a.png, dpi=150)
        plt.close("all")
    return 0


if __name__ == "__main__":
    sys.exit(main())
