"""SPH interpolation of a save file at arbitrary points on the GPU: unwrapped (R, phi) maps, (R, z) cuts, inclined planes,
probe lines, or any list of points.

    python -m summersph_amd.sample SAVE.txt -o OUT.npz [--variable] [--fields rho,u,vy] [--volume] [--normalise] [--h H]
           (--polar RMIN RMAX NR NPHI | --rz RMIN RMAX NR ZMIN ZMAX NZ | --plane CX,CY,CZ UX,UY,UZ VX,VY,VZ WU WV NU NV |
            --line AX,AY,AZ BX,BY,BZ N | --points PTS.npy) [--log] [--centre X,Y,Z] [--normal NX,NY,NZ] [--phi PHI]
           [--clip x0,y0,z0,x1,y1,z1] [--json]

SAVE.txt is a save file as for `python -m summersph_amd.profile`: records of 9 values (10 with --variable: .. alpha h)
are gas, records of 8 values are sinks.  The gas and the sinks are uploaded into a fresh context; sph_density runs only
when rho, P or c or the volume weight is asked for.  sph_sample (capi.Context.sample) then gives, at every point,
den = sum ws Wn and num_k = sum ws A_k Wn for up to four fields (SPH_F_* names), ws = m / (pi h^3) (--volume:
(m / rho) / (pi h^3)); --normalise stores num / den instead of num.  Without --fields the weight alone is computed: the
SPH density at the points.

OUT.npz holds `points` (M, 3), `shape` (the point set's own shape, e.g. (NR, NPHI)), `weight` (M,), one array named after
each field (M,), `n_hit` (points reached by a source) and `n_nonfinite`; the descriptor used is in the `desc_*` entries.
Reshape any of the arrays with `shape` for the map.  --json prints the counts and the mean weight as one JSON line.

The point-set helpers below are pure numpy and usable on their own with capi.Context.sample.
"""
from __future__ import annotations

import argparse
import json
import math
import sys

import numpy as np

from . import cli
from .cli import STATE, desc_arrays, parse_clip, parse_vec, read_save, uploaded_context


# ---- point sets ----------------------------------------------------------------------------------------------------------
def frame(normal=(0.0, 0.0, 1.0)):
    """(n^, e1, e2) of sph_profile's frame rule (include/summersph.h, "Frame"): n^ = normal / |normal|, a = x^ if
    |n^_x| <= 0.9 else y^, e1 = (a - (a.n^) n^) normalised, e2 = n^ x e1; n^ = z^ gives the lab axes"""
    nin = np.asarray(normal, dtype=np.float64).reshape(3)
    ln = math.sqrt((nin[0] * nin[0] + nin[1] * nin[1]) + nin[2] * nin[2])
    if not (ln > 0.0 and math.isfinite(ln)):
        raise ValueError("normal must be finite and non-zero")
    n = nin / ln
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) <= 0.9 else np.array([0.0, 1.0, 0.0])
    t = a - ((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]) * n
    e1 = t / math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    e2 = np.array([n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]])
    return n, e1, e2


def ring_radii(r_min, r_max, n_r, log=False):
    """the centres of sph_profile's rings: the midpoints (log: the geometric means) of its edges"""
    if not (n_r >= 1 and 0.0 <= r_min < r_max and math.isfinite(r_max)) or (log and r_min <= 0.0):
        raise ValueError("radii: 0 <= r_min < r_max (log: r_min > 0) and n_r >= 1")
    k = np.arange(n_r + 1, dtype=np.float64)
    e = r_min * (r_max / r_min) ** (k / n_r) if log else r_min + (k * (r_max - r_min)) / n_r
    e[-1] = r_max
    return np.sqrt(e[:-1] * e[1:]) if log else 0.5 * (e[:-1] + e[1:])


def sector_angles(n_phi):
    """the centres of sph_profile's sectors: -pi + 2 pi (j + 1/2) / n_phi"""
    if n_phi < 1:
        raise ValueError("n_phi >= 1")
    return -math.pi + (2.0 * math.pi) * (np.arange(n_phi) + 0.5) / n_phi


def polar_points(r_min, r_max, n_r, n_phi, z=0.0, log=False, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """An unwrapped (R, phi) map at height z above the plane through centre with the given normal: the points
    centre + R (cos phi e1 + sin phi e2) + z n^ at the centres of sph_profile's rings and sectors (its frame, its edges).
    Returns (points (n_r n_phi, 3), (n_r, n_phi)); point k n_phi + j is ring k, sector j, as sph_profile's bins."""
    n, e1, e2 = frame(normal)
    R, phi = ring_radii(r_min, r_max, n_r, log), sector_angles(n_phi)
    X, Y = R[:, None] * np.cos(phi)[None, :], R[:, None] * np.sin(phi)[None, :]
    p = np.asarray(centre, dtype=np.float64) + X[..., None] * e1 + Y[..., None] * e2 + float(z) * n
    return p.reshape(-1, 3), (int(n_r), int(n_phi))


def rz_points(r_min, r_max, n_r, z_min, z_max, n_z, phi=0.0, log=False, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """An (R, z) cut at azimuth phi of the same frame: R at the ring centres, z = np.linspace(z_min, z_max, n_z).
    Returns (points (n_r n_z, 3), (n_r, n_z))."""
    n, e1, e2 = frame(normal)
    R = ring_radii(r_min, r_max, n_r, log)
    Z = np.linspace(z_min, z_max, n_z)
    d = math.cos(phi) * e1 + math.sin(phi) * e2
    p = np.asarray(centre, dtype=np.float64) + R[:, None, None] * d + Z[None, :, None] * n
    return p.reshape(-1, 3), (int(n_r), int(n_z))


def plane_points(centre, u, v, extent, shape):
    """A raster in the plane through centre spanned by u and v: u is normalised, v is made orthogonal to u and normalised
    (Gram-Schmidt), extent = (width along u, width along v), shape = (n_u, n_v) np.linspace nodes centred on centre.
    Returns (points (n_u n_v, 3), (n_u, n_v))."""
    u, v = np.asarray(u, dtype=np.float64).reshape(3), np.asarray(v, dtype=np.float64).reshape(3)
    lu = np.linalg.norm(u)
    if not (lu > 0 and np.isfinite(lu)):
        raise ValueError("plane: u must be finite and non-zero")
    u = u / lu
    v = v - np.dot(v, u) * u
    lv = np.linalg.norm(v)
    if not (lv > 1e-12 and np.isfinite(lv)):
        raise ValueError("plane: v must not be parallel to u")
    v = v / lv
    nu, nv = int(shape[0]), int(shape[1])
    if nu < 1 or nv < 1:
        raise ValueError("plane: shape >= (1, 1)")
    su = np.linspace(-0.5 * extent[0], 0.5 * extent[0], nu) if nu > 1 else np.zeros(1)
    sv = np.linspace(-0.5 * extent[1], 0.5 * extent[1], nv) if nv > 1 else np.zeros(1)
    p = np.asarray(centre, dtype=np.float64) + su[:, None, None] * u + sv[None, :, None] * v
    return p.reshape(-1, 3), (nu, nv)


def line_points(a, b, n):
    """n points from a to b (np.linspace, both ends included).  Returns (points (n, 3), (n,))."""
    a, b = np.asarray(a, dtype=np.float64).reshape(3), np.asarray(b, dtype=np.float64).reshape(3)
    if n < 1:
        raise ValueError("line: n >= 1")
    return np.linspace(a, b, int(n)), (int(n),)


# ---- command line --------------------------------------------------------------------------------------------------------
def parse_fields(spec, variable=False):
    """'rho,u,vy' -> ['rho', 'u', 'vy']: 0 .. 4 field names of capi.FIELDS (h and omega only with variable h); '' -> []"""
    from . import capi
    return cli.parse_fields(spec, 0, capi.SAMPLE_MAX_FIELDS, variable)


def points_from_args(a):
    """the point set of the parsed command line: (points (M, 3), shape)"""
    centre = parse_vec(a.centre, "--centre")
    normal = parse_vec(a.normal, "--normal")
    if a.polar:
        r0, r1, nr, nphi = a.polar
        return polar_points(float(r0), float(r1), int(nr), int(nphi), 0.0, a.log, centre, normal)
    if a.rz:
        r0, r1, nr, z0, z1, nz = a.rz
        return rz_points(float(r0), float(r1), int(nr), float(z0), float(z1), int(nz), a.phi, a.log, centre, normal)
    if a.plane:
        c, u, v, wu, wv, nu, nv = a.plane
        return plane_points(parse_vec(c, "--plane"), parse_vec(u, "--plane"), parse_vec(v, "--plane"), (float(wu), float(wv)),
                            (int(nu), int(nv)))
    if a.line:
        p, q, n = a.line
        return line_points(parse_vec(p, "--line"), parse_vec(q, "--line"), int(n))
    pts = np.asarray(np.load(a.points), dtype=np.float64)
    if pts.ndim < 2 or pts.shape[-1] != 3:
        raise ValueError("--points wants an array of shape (..., 3)")
    return pts.reshape(-1, 3), tuple(pts.shape[:-1])


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.sample", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--fields", default="", help="0 .. 4 comma-separated field names (none: the weight alone)")
    ap.add_argument("--volume", action="store_true", help="volume weight m / rho instead of the mass weight")
    ap.add_argument("--normalise", action="store_true", help="num / den instead of num")
    ap.add_argument("--h", type=float, default=None, help="one h for every particle (default: each particle's own)")
    ap.add_argument("--clip", default=None, help="strict source clip box x0,y0,z0,x1,y1,z1")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--polar", nargs=4, metavar=("RMIN", "RMAX", "NR", "NPHI"), help="(R, phi) map of the plane")
    g.add_argument("--rz", nargs=6, metavar=("RMIN", "RMAX", "NR", "ZMIN", "ZMAX", "NZ"), help="(R, z) cut at --phi")
    g.add_argument("--plane", nargs=7, metavar=("C", "U", "V", "WU", "WV", "NU", "NV"), help="raster in the plane (C; U, V)")
    g.add_argument("--line", nargs=3, metavar=("A", "B", "N"), help="N points from A to B")
    g.add_argument("--points", help=".npy file of shape (..., 3)")
    ap.add_argument("--log", action="store_true", help="logarithmic radii (--polar, --rz)")
    ap.add_argument("--centre", default="0,0,0", help="frame origin x,y,z (--polar, --rz)")
    ap.add_argument("--normal", default="0,0,1", help="plane normal nx,ny,nz, sph_profile's frame (--polar, --rz)")
    ap.add_argument("--phi", type=float, default=0.0, help="azimuth of the --rz cut")
    ap.add_argument("--json", action="store_true", help="print the counts and the mean weight as one JSON line")
    ap.add_argument("--device", type=int, default=0)
    return ap


def sample_rows(gas, sinks, points, fields=(), volume=False, normalise=False, h=None, clip=None, variable=False, device=0):
    """Uploads the rows into a fresh context and samples: (out (K, M), den (M,), (n_hit, n_nonfinite), descriptor)."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        if volume or any(f not in STATE + ["h"] for f in fields):
            ctx.density()                   # rho, P, c (and the rates' fields only after forces: stale otherwise)
        out, den, cnt = ctx.sample(points, fields=fields, weight="volume" if volume else "mass", normalise=normalise, h=h,
                                   clip=clip, weight_out=True, counts=True)
        return out, den, cnt, ctx.sample_desc


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        fields = parse_fields(a.fields, a.variable)
        clip = None if a.clip is None else parse_clip(a.clip)
        points, shape = points_from_args(a)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    if a.h is not None and not (np.isfinite(a.h) and a.h > 0):
        ap.error("--h must be finite and > 0")

    gas, sinks = read_save(a.save, a.variable)
    out, den, (n_hit, n_bad), d = sample_rows(gas, sinks, points, fields, a.volume, a.normalise, a.h, clip, a.variable, a.device)
    res = {f: out[k] for k, f in enumerate(fields)}
    res.update(points=points, shape=np.array(shape, dtype=np.int64), weight=den, n_hit=np.array(n_hit), n_nonfinite=np.array(n_bad))
    res.update(desc_arrays(d))
    np.savez(a.out, **res)
    ok = np.isfinite(den)
    summary = {"n_points": int(points.shape[0]), "n_hit": n_hit, "n_nonfinite": n_bad,
               "mean_weight": float(den[ok].mean()) if ok.any() else None}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: {','.join(fields) or 'the weight'} at {points.shape[0]} points of shape {tuple(shape)} "
              f"({n_hit} reached by a source) from {gas.shape[0]} gas rows")
    return 0


if __name__ == "__main__":
    sys.exit(main())
