"""Azimuthally averaged disc profiles of a save file on the GPU: surface density, rotation, epicyclic frequency, scale
height, Toomre Q, radial drift, accretion rate, tilt, twist and eccentricity per ring.

    python -m summersph_amd.profile SAVE.txt -o OUT.npz [--csv OUT.csv] [--variable] --rmin R0 --rmax R1 --bins N
                                    [--log] [--nphi K] [--centre sink:0 | x,y,z] [--normal auto | x,y,z] [--zmax Z]

SAVE.txt is a save file: one header line, then one record per line.  Without --variable, records of 9 values are gas
(x y z vx vy vz u m alpha, make_save's layout, SUMMER_SPH.f90:719-738); with --variable, records of 10 values are gas
(.. alpha h, the variable-h host's layout).  Records of 8 values are sinks (x y z vx vy vz 0 m), last in the file.  The
gas and the sinks are uploaded into a fresh context and binned with sph_profile (capi.Context.profile): the owned gas in
rings r_min <= R < r_max (--log: logarithmic edges), each ring cut into --nphi sectors, about the centre in the frame of
the normal.

--centre sink:K centres the frame on sink K (its position, velocity and mass: the eccentricity vector is taken about its
mass); --centre x,y,z on a point at rest with no central mass (eccentricities 0).  Default: sink:0 when the file has a
sink, else the origin.  --normal auto takes the total angular momentum of the gas in the shell r_min <= |r'| < r_max;
default 0,0,1.  --zmax keeps only |z'| < Z.

OUT.npz holds every column of sph_profile_finish by name (capi.PROFILE_COLUMNS, one value per bin, bin = ring * nphi +
sector), `edges` (the n + 1 ring edges), `sums` (the raw sums, n_bins x 20, which add across files of one snapshot) and
the descriptor used (`desc_*`; the normal written back normalised).  --csv also writes the columns as text.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from .cli import desc_arrays, read_save, uploaded_context


def parse_centre(spec: str):
    """'sink:K' -> ('sink', K); 'x,y,z' -> ('point', (x, y, z)); anything else raises ValueError"""
    if spec.startswith("sink:"):
        k = int(spec[5:])
        if k < 0:
            raise ValueError(f"bad sink index in {spec!r}")
        return "sink", k
    v = [float(t) for t in spec.split(",")]
    if len(v) != 3 or not all(np.isfinite(v)):
        raise ValueError(f"--centre wants sink:K or x,y,z, not {spec!r}")
    return "point", tuple(v)


def parse_normal(spec: str):
    """'auto' -> 'auto'; 'x,y,z' -> (x, y, z), finite and not zero"""
    if spec == "auto":
        return "auto"
    v = [float(t) for t in spec.split(",")]
    if len(v) != 3 or not all(np.isfinite(v)) or not any(v):
        raise ValueError(f"--normal wants auto or a non-zero x,y,z, not {spec!r}")
    return tuple(v)


def profile_rows(gas, sinks, r_min, r_max, n_r, n_phi=1, log=False, centre=None, normal=(0.0, 0.0, 1.0), z_max=np.inf,
                 variable=False, device=0):
    """Uploads the rows into a fresh context and profiles them: (table, sums, descriptor used)."""
    kw = {}
    if centre is not None and centre[0] == "sink":
        kw["sink"] = centre[1]
    elif centre is not None:
        kw["centre"] = (centre[1], (0.0, 0.0, 0.0), 0.0)
    with uploaded_context(gas, sinks, variable, device) as ctx:
        table, sums = ctx.profile(r_min, r_max, n_r, n_phi, log=log, normal=normal, z_max=z_max, **kw)
        return table, sums, ctx.profile_desc


def main(argv=None) -> int:
    from . import capi
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.profile", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--csv", default=None, help="also write the columns as CSV")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--rmin", type=float, required=True)
    ap.add_argument("--rmax", type=float, required=True)
    ap.add_argument("--bins", type=int, required=True, help="rings")
    ap.add_argument("--log", action="store_true", help="logarithmic ring edges")
    ap.add_argument("--nphi", type=int, default=1, help="sectors per ring")
    ap.add_argument("--centre", default=None, help="sink:K or x,y,z (default sink:0 if there is a sink, else 0,0,0)")
    ap.add_argument("--normal", default="0,0,1", help="auto or x,y,z")
    ap.add_argument("--zmax", type=float, default=np.inf)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        centre = None if a.centre is None else parse_centre(a.centre)
        normal = parse_normal(a.normal)
    except ValueError as e:
        ap.error(str(e))
    if a.bins < 1 or a.nphi < 1:
        ap.error("--bins and --nphi must be >= 1")
    if not (0.0 <= a.rmin < a.rmax) or (a.log and a.rmin == 0.0):
        ap.error("need 0 <= --rmin < --rmax (and --rmin > 0 with --log)")

    gas, sinks = read_save(a.save, a.variable)
    if centre is None:
        centre = ("sink", 0) if sinks.shape[0] else ("point", (0.0, 0.0, 0.0))
    if centre[0] == "sink" and centre[1] >= sinks.shape[0]:
        ap.error(f"--centre sink:{centre[1]}: the file has {sinks.shape[0]} sinks")
    table, sums, d = profile_rows(gas, sinks, a.rmin, a.rmax, a.bins, a.nphi, a.log, centre, normal, a.zmax, a.variable,
                                  a.device)
    out = {c: np.ascontiguousarray(table[c]) for c in capi.PROFILE_COLUMNS}
    out["edges"] = np.append(table["R_lo"][::a.nphi], table["R_hi"][-1])
    out["sums"] = sums
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    if a.csv:
        np.savetxt(a.csv, np.stack([table[c] for c in capi.PROFILE_COLUMNS], axis=1), delimiter=",",
                   header=",".join(capi.PROFILE_COLUMNS), comments="")
    print(f"{a.out}: {a.bins} rings x {a.nphi} sectors from {gas.shape[0]} gas rows ({sinks.shape[0]} sinks), "
          f"{int(np.sum(table['N']))} selected, normal {list(d.normal)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
