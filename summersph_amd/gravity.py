"""Gravitational potential and acceleration of a save file at arbitrary points on the GPU: potential maps, (R, z) cuts,
probe lines, the field at the particles, or a rotation curve split into the disc's and the sinks' part.

    python -m summersph_amd.gravity SAVE.txt -o OUT.npz [--variable] [--h H] [--soft2 S2] [--theta THETA]
           (--polar RMIN RMAX NR NPHI | --rz RMIN RMAX NR ZMIN ZMAX NZ | --plane CX,CY,CZ UX,UY,UZ VX,VY,VZ WU WV NU NV |
            --line AX,AY,AZ BX,BY,BZ N | --points PTS.npy | --particles | --rotation-curve RMIN RMAX NR NPHI)
           [--log] [--centre X,Y,Z] [--normal NX,NY,NZ] [--phi PHI] [--no-gas] [--no-sinks] [--split] [--json]

SAVE.txt is a save file as for `python -m summersph_amd.sample`.  The gas and the sinks are uploaded into a fresh context
and sph_gravity_at (capi.Context.gravity_at) gives Phi and a at every point: the Barnes-Hut field of the gas (opening
angle --theta, default the context's 0.5) softened with the points' length h -- --h, else params.h; with --variable --h is
needed except with --particles, which evaluates at the gas positions with each particle's own h -- plus the unsoftened
field of the sinks.  --no-gas / --no-sinks drop a part; --split keeps the two apart.

OUT.npz holds `points` (M, 3), `shape`, `phi` (M,) and `acc` (3, M) -- with --split (2, M) and (2, 3, M), the gas first --
`n_nonfinite`, `n_bad_h` and the descriptor in the `desc_*` entries.  --rotation-curve evaluates an (NR, NPHI) polar map
and adds `R` (NR,) and the azimuthal means of v_c^2 = -R g_R: `vc2_gas`, `vc2_sinks` (the parts computed) and `vc2`, their
sum.  A negative mean (an outward pull) is kept as it is.  --json prints a one-line summary.

cylindrical() below is pure numpy and usable on its own with capi.Context.gravity_at.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .cli import desc_arrays, parse_vec, read_save, uploaded_context
from .sample import frame, points_from_args, ring_radii


def cylindrical(acc, points, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """(g_R, g_phi, g_z) of the accelerations acc (3, M) at points (M, 3) in sample.frame's axes about centre:
    R^ = (X e1 + Y e2) / R, phi^ = (X e2 - Y e1) / R, z^ = n^ with X, Y the point's coordinates along e1, e2.  On the
    axis (R == 0) g_R and g_phi are NaN."""
    n, e1, e2 = frame(normal)
    a = np.asarray(acc, dtype=np.float64)
    rel = np.asarray(points, dtype=np.float64).reshape(-1, 3) - np.asarray(centre, dtype=np.float64)
    X, Y = rel @ e1, rel @ e2
    a1, a2, an = e1 @ a, e2 @ a, n @ a
    with np.errstate(invalid="ignore", divide="ignore"):
        R = np.sqrt(X * X + Y * Y)
        g_r = (X * a1 + Y * a2) / R
        g_phi = (X * a2 - Y * a1) / R
    return g_r, g_phi, an


def rotation_curve(acc, points, shape, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """the azimuthal mean of v_c^2 = -R g_R over a polar map of the given (n_r, n_phi) shape: (n_r,)"""
    rel = np.asarray(points, dtype=np.float64).reshape(-1, 3) - np.asarray(centre, dtype=np.float64)
    _, e1, e2 = frame(normal)
    R = np.sqrt((rel @ e1) ** 2 + (rel @ e2) ** 2)
    g_r = cylindrical(acc, points, centre, normal)[0]
    return (-(R * g_r)).reshape(shape).mean(axis=1)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.gravity", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--h", type=float, default=None, help="softening length of every point (default: params.h)")
    ap.add_argument("--soft2", type=float, default=None, help="added to the squared distance (default: the force's 0.0025)")
    ap.add_argument("--theta", type=float, default=None, help="Barnes-Hut opening angle (default: the context's)")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--polar", nargs=4, metavar=("RMIN", "RMAX", "NR", "NPHI"), help="(R, phi) map of the plane")
    g.add_argument("--rz", nargs=6, metavar=("RMIN", "RMAX", "NR", "ZMIN", "ZMAX", "NZ"), help="(R, z) cut at --phi")
    g.add_argument("--plane", nargs=7, metavar=("C", "U", "V", "WU", "WV", "NU", "NV"), help="raster in the plane (C; U, V)")
    g.add_argument("--line", nargs=3, metavar=("A", "B", "N"), help="N points from A to B")
    g.add_argument("--points", help=".npy file of shape (..., 3)")
    g.add_argument("--particles", action="store_true", help="at the gas positions (variable h: each particle's own h)")
    g.add_argument("--rotation-curve", nargs=4, metavar=("RMIN", "RMAX", "NR", "NPHI"), dest="rotation_curve",
                   help="azimuthal means of v_c^2 = -R g_R over an (R, phi) map")
    ap.add_argument("--log", action="store_true", help="logarithmic radii (--polar, --rz, --rotation-curve)")
    ap.add_argument("--centre", default="0,0,0", help="frame origin x,y,z (--polar, --rz, --rotation-curve)")
    ap.add_argument("--normal", default="0,0,1", help="plane normal nx,ny,nz, sph_profile's frame")
    ap.add_argument("--phi", type=float, default=0.0, help="azimuth of the --rz cut")
    ap.add_argument("--no-gas", action="store_true", dest="no_gas", help="leave the gas part out")
    ap.add_argument("--no-sinks", action="store_true", dest="no_sinks", help="leave the sinks' part out")
    ap.add_argument("--split", action="store_true", help="keep the gas and the sinks apart (needs both parts)")
    ap.add_argument("--json", action="store_true", help="print a summary as one JSON line")
    ap.add_argument("--device", type=int, default=0)
    return ap


def check_args(ap, a):
    """the checks that need no device: the parts, h, soft2, theta"""
    if a.no_gas and a.no_sinks:
        ap.error("--no-gas and --no-sinks leave nothing to compute")
    if a.split and (a.no_gas or a.no_sinks):
        ap.error("--split needs both parts")
    if a.h is not None and not (np.isfinite(a.h) and a.h > 0):
        ap.error("--h must be finite and > 0")
    if a.soft2 is not None and not (np.isfinite(a.soft2) and a.soft2 >= 0):
        ap.error("--soft2 must be finite and >= 0")
    if a.theta is not None and not (np.isfinite(a.theta) and a.theta > 0):
        ap.error("--theta must be finite and > 0")
    if a.variable and a.h is None and not a.particles:
        ap.error("--variable needs --h (the points have no h of their own), except with --particles")


def gravity_rows(gas, sinks, points, h=None, ph=None, soft2=None, gas_part=True, sink_part=True, split=False, theta=None,
                 variable=False, device=0):
    """Uploads the rows into a fresh context and evaluates: (phi, acc, (n_nonfinite, n_bad_h), descriptor)."""
    from . import capi
    with uploaded_context(gas, sinks, variable, device, **({} if theta is None else {"theta": float(theta)})) as ctx:
        phi, acc, cnt = ctx.gravity_at(points, h=h, ph=ph, soft2=capi.GRAVAT_REF_SOFT2 if soft2 is None else soft2, gas=gas_part,
                                       sinks=sink_part, split=split, counts=True)
        return phi, acc, cnt, ctx.gravity_at_desc


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    curve = a.rotation_curve is not None
    gas, sinks = read_save(a.save, a.variable)
    ph = None
    try:
        if a.particles:
            points, shape = np.ascontiguousarray(gas[:, :3]), (gas.shape[0],)
            if a.variable and a.h is None:
                ph = np.ascontiguousarray(gas[:, 9])
        elif curve:
            a.polar = a.rotation_curve
            points, shape = points_from_args(a)
        else:
            points, shape = points_from_args(a)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    both = not (a.no_gas or a.no_sinks)
    split = a.split or (curve and both)
    phi, acc, (n_nonfin, n_bad_h), d = gravity_rows(gas, sinks, points, a.h, ph, a.soft2, not a.no_gas, not a.no_sinks, split,
                                                    a.theta, a.variable, a.device)
    res = {}
    if curve:
        centre, normal = parse_vec(a.centre, "--centre"), parse_vec(a.normal, "--normal")
        r0, r1, nr, _ = a.rotation_curve
        res["R"] = ring_radii(float(r0), float(r1), int(nr), a.log)
        if both:
            res["vc2_gas"] = rotation_curve(acc[0], points, shape, centre, normal)
            res["vc2_sinks"] = rotation_curve(acc[1], points, shape, centre, normal)
            res["vc2"] = res["vc2_gas"] + res["vc2_sinks"]
            if not a.split:
                phi, acc = phi[0] + phi[1], acc[0] + acc[1]
        else:
            res["vc2"] = rotation_curve(acc, points, shape, centre, normal)
            res["vc2_sinks" if a.no_gas else "vc2_gas"] = res["vc2"]
    res.update(points=points, shape=np.array(shape, dtype=np.int64), phi=phi, acc=acc, n_nonfinite=np.array(n_nonfin),
               n_bad_h=np.array(n_bad_h))
    res.update(desc_arrays(d))
    np.savez(a.out, **res)
    ok = np.isfinite(phi)
    summary = {"n_points": int(points.shape[0]), "n_nonfinite": n_nonfin, "n_bad_h": n_bad_h,
               "min_phi": float(phi[ok].min()) if ok.any() else None}
    if curve:
        summary["vc2"] = res["vc2"].tolist()
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: phi and a at {points.shape[0]} points of shape {tuple(shape)} from {gas.shape[0]} gas rows and "
              f"{sinks.shape[0]} sinks")
    return 0


if __name__ == "__main__":
    sys.exit(main())
