"""Field lines of a save file's gas on the GPU: streamlines of the velocity (in the inertial frame or one that rotates with
a sink), or of any three fields, from a ring, a line, a raster or any list of seeds.

    python -m summersph_amd.trace SAVE.txt -o OUT.npz [--variable] [--fields vx,vy,vz] [--carry rho] [--volume] [--h H]
           (--ring R N | --line AX,AY,AZ BX,BY,BZ N | --grid CX,CY,CZ UX,UY,UZ VX,VY,VZ WU WV NU NV | --seeds PTS.npy)
           --steps S --ds DS [--stride K] [--arclength] [--planar NX NY NZ] [--omega OX OY OZ | --corotate-sink K [--about J]]
           [--both] [--centre X,Y,Z] [--normal NX,NY,NZ] [--box x0,y0,z0,x1,y1,z1] [--clip x0,y0,z0,x1,y1,z1] [--json]

SAVE.txt is a save file as for `python -m summersph_amd.sample`.  The gas and the sinks are uploaded into a fresh context;
sph_density runs only when rho, P or c or the volume weight is asked for.  sph_trace (capi.Context.trace) then integrates
every seed S classical RK4 steps of DS through the frozen, SPH-interpolated field: DS is a time, or with --arclength a
length along v / |v|.  --planar removes the field's component along a normal; --corotate-sink K traces in the frame that
rotates with sink K about sink J (sink_frame); --both joins an upstream and a downstream line per seed.

OUT.npz holds `path` (rows, 3, M) -- rows = S / K + 1, or 2 S / K + 1 with --both, the seed in the middle row then --,
`seeds` (M, 3), `shape`, `status` and `n_done` (with --both: `status_up`, `n_done_up` too), `carry` (rows, M) with --carry,
`counts` (the seeds per status code of capi.TRACE_STATUS; the downstream call's) and the descriptor in the `desc_*` entries.
Rows after a line's last vertex are NaN.  --json prints the counts as one JSON line.

The seed helpers below are pure numpy and usable on their own with capi.Context.trace.
"""
from __future__ import annotations

import argparse
import json
import math
import sys

import numpy as np

from . import cli
from .cli import STATE, desc_arrays, parse_clip, parse_vec, read_save, uploaded_context
from .sample import frame, line_points, plane_points


# ---- seeds and frames ----------------------------------------------------------------------------------------------------
def ring_seeds(R, n, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """n seeds on the circle of radius R about centre in the plane with the given normal (sph_profile's frame): centre +
    R (cos phi e1 + sin phi e2), phi = 2 pi j / n.  Returns (seeds (n, 3), (n,))."""
    if not (n >= 1 and R > 0.0 and math.isfinite(R)):
        raise ValueError("ring: R > 0 and n >= 1")
    _, e1, e2 = frame(normal)
    phi = (2.0 * math.pi) * np.arange(int(n)) / int(n)
    p = np.asarray(centre, dtype=np.float64) + R * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return p, (int(n),)


def line_seeds(a, b, n):
    """n seeds from a to b, both ends included (sample.line_points).  Returns (seeds (n, 3), (n,))."""
    return line_points(a, b, n)


def grid_seeds(centre, u, v, extent, shape):
    """One seed per pixel of a raster in the plane through centre spanned by u and v (sample.plane_points): the seeds of a
    line-integral-convolution image.  Returns (seeds (n_u n_v, 3), (n_u, n_v))."""
    return plane_points(centre, u, v, extent, shape)


def sink_frame(sinks, k, about=0):
    """The frame that rotates with sink k about sink `about`: (omega, centre) with omega = r x v / r^2 of the relative
    position and velocity and centre the position of `about`.  sinks: rows x y z vx vy vz ... (a save file's sink rows), or
    a dict of arrays x, y, z, vx, vy, vz."""
    if isinstance(sinks, dict):
        s = np.stack([np.asarray(sinks[f], dtype=np.float64) for f in ("x", "y", "z", "vx", "vy", "vz")], axis=1)
    else:
        s = np.asarray(sinks, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] < 6 or not (0 <= k < s.shape[0] and 0 <= about < s.shape[0]) or k == about:
        raise ValueError("sink_frame: two different sinks of the rows x y z vx vy vz ...")
    r, v = s[k, :3] - s[about, :3], s[k, 3:6] - s[about, 3:6]
    r2 = float(r @ r)
    if not (r2 > 0.0 and math.isfinite(r2)):
        raise ValueError("sink_frame: the two sinks coincide")
    return tuple(float(t) for t in np.cross(r, v) / r2), tuple(float(t) for t in s[about, :3])


def both_ways(ctx, seeds, n_steps, ds, **kw):
    """A downstream (ds) and an upstream (-ds) Context.trace call joined into one polyline per seed: path (2 n_rec + 1, 3,
    M) runs from the upstream end through the seed (row n_rec) to the downstream end, NaN beyond either end.  Returns
    (path, (status_up, status_down), (n_done_up, n_done_down)[, carry (2 n_rec + 1, M)][, counts of the downstream call]);
    host form only."""
    if kw.get("device"):
        raise ValueError("both_ways: host form only")
    down = ctx.trace(seeds, n_steps, ds, **kw)
    desc = ctx.trace_desc
    up = ctx.trace(seeds, n_steps, -ds, **kw)
    ctx.trace_desc = desc
    path = np.concatenate([up[0][:0:-1], down[0]])
    out = [path, (up[1], down[1]), (up[2], down[2])]
    if kw.get("carry") is not None:
        out.append(np.concatenate([up[3][:0:-1], down[3]]))
    if kw.get("counts"):
        out.append(down[-1])
    return tuple(out)


# ---- command line --------------------------------------------------------------------------------------------------------
def parse_fields(spec, variable=False):
    """'vx,vy,vz' -> ['vx', 'vy', 'vz']: exactly three field names of capi.FIELDS (h and omega only with variable h)"""
    return cli.parse_fields(spec, 3, 3, variable)


def seeds_from_args(a):
    """the seed set of the parsed command line: (seeds (M, 3), shape)"""
    if a.ring:
        return ring_seeds(float(a.ring[0]), int(a.ring[1]), parse_vec(a.centre, "--centre"), parse_vec(a.normal, "--normal"))
    if a.line:
        p, q, n = a.line
        return line_seeds(parse_vec(p, "--line"), parse_vec(q, "--line"), int(n))
    if a.grid:
        c, u, v, wu, wv, nu, nv = a.grid
        return grid_seeds(parse_vec(c, "--grid"), parse_vec(u, "--grid"), parse_vec(v, "--grid"), (float(wu), float(wv)),
                          (int(nu), int(nv)))
    pts = np.asarray(np.load(a.seeds), dtype=np.float64)
    if pts.ndim < 2 or pts.shape[-1] != 3:
        raise ValueError("--seeds wants an array of shape (..., 3)")
    return pts.reshape(-1, 3), tuple(pts.shape[:-1])


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.trace", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--fields", default="vx,vy,vz", help="the vector's three components (field names)")
    ap.add_argument("--carry", default=None, help="a field sampled at every recorded vertex")
    ap.add_argument("--volume", action="store_true", help="volume weight m / rho instead of the mass weight")
    ap.add_argument("--h", type=float, default=None, help="one h for every particle (default: each particle's own)")
    ap.add_argument("--clip", default=None, help="strict source clip box x0,y0,z0,x1,y1,z1")
    ap.add_argument("--box", default=None, help="the lines stop outside x0,y0,z0,x1,y1,z1")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--ring", nargs=2, metavar=("R", "N"), help="N seeds on the circle of radius R (--centre, --normal)")
    g.add_argument("--line", nargs=3, metavar=("A", "B", "N"), help="N seeds from A to B")
    g.add_argument("--grid", nargs=7, metavar=("C", "U", "V", "WU", "WV", "NU", "NV"), help="one seed per pixel of the plane (C; U, V)")
    g.add_argument("--seeds", help=".npy file of shape (..., 3)")
    ap.add_argument("--centre", default="0,0,0", help="the ring's centre x,y,z")
    ap.add_argument("--normal", default="0,0,1", help="the ring's plane normal nx,ny,nz (sph_profile's frame)")
    ap.add_argument("--steps", type=int, required=True, help="RK4 steps per line (1 .. 65535)")
    ap.add_argument("--ds", type=float, required=True, help="the step: a time, with --arclength a length; < 0 traces upstream")
    ap.add_argument("--stride", type=int, default=1, help="record every stride-th vertex (divides --steps)")
    ap.add_argument("--arclength", action="store_true", help="step along v / |v|")
    ap.add_argument("--planar", nargs=3, type=float, default=None, metavar=("NX", "NY", "NZ"),
                    help="remove the field's component along this normal")
    f = ap.add_mutually_exclusive_group()
    f.add_argument("--omega", nargs=3, type=float, default=None, metavar=("OX", "OY", "OZ"),
                   help="trace v - omega x (p - frame centre); the frame centre is --frame-centre")
    f.add_argument("--corotate-sink", type=int, default=None, metavar="K", help="the frame that rotates with sink K about sink --about")
    ap.add_argument("--about", type=int, default=0, help="the sink --corotate-sink turns about")
    ap.add_argument("--frame-centre", default="0,0,0", help="the centre of --omega's frame")
    ap.add_argument("--both", action="store_true", help="join an upstream and a downstream line per seed")
    ap.add_argument("--json", action="store_true", help="print the counts as one JSON line")
    ap.add_argument("--device", type=int, default=0)
    return ap


def trace_options(a, sinks=None):
    """the keyword arguments of Context.trace that the parsed command line asks for (sinks: the save file's sink rows)"""
    from . import capi
    if not (1 <= a.steps <= 65535) or a.stride < 1 or a.steps % a.stride:
        raise ValueError("--steps 1 .. 65535 and --stride >= 1 dividing it")
    if not (math.isfinite(a.ds) and a.ds != 0.0):
        raise ValueError("--ds must be finite and != 0")
    if a.h is not None and not (math.isfinite(a.h) and a.h > 0):
        raise ValueError("--h must be finite and > 0")
    kw = dict(fields=parse_fields(a.fields, a.variable), arclength=a.arclength, stride=a.stride,
              weight="volume" if a.volume else "mass", h=a.h, clip=None if a.clip is None else parse_clip(a.clip),
              box=None if a.box is None else parse_clip(a.box), carry=a.carry)
    if a.carry is not None and (a.carry not in capi.FIELDS or (not a.variable and a.carry in ("h", "omega"))):
        raise ValueError(f"--carry wants one field name of capi.FIELDS, not {a.carry!r}")
    if a.planar is not None:
        if not (all(math.isfinite(t) for t in a.planar) and any(t != 0.0 for t in a.planar)):
            raise ValueError("--planar wants a finite non-zero normal")
        kw["normal"] = tuple(a.planar)
    if a.omega is not None:
        kw["omega"], kw["centre"] = tuple(a.omega), parse_vec(a.frame_centre, "--frame-centre")
    elif a.corotate_sink is not None:
        if sinks is None:
            raise ValueError("--corotate-sink needs the save file's sinks")
        kw["omega"], kw["centre"] = sink_frame(sinks, a.corotate_sink, a.about)
    return kw


def trace_rows(gas, sinks, seeds, n_steps, ds, both=False, variable=False, device=0, **kw):
    """Uploads the rows into a fresh context and traces: Context.trace's tuple with counts (both: both_ways' tuple) and the
    descriptor."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        used = list(kw.get("fields", ())) + ([kw["carry"]] if kw.get("carry") is not None else [])
        if kw.get("weight") == "volume" or any(f not in STATE + ["h"] for f in used):
            ctx.density()                   # rho, P, c (and the rates' fields only after forces: stale otherwise)
        res = both_ways(ctx, seeds, n_steps, ds, counts=True, **kw) if both else ctx.trace(seeds, n_steps, ds, counts=True, **kw)
        return res, ctx.trace_desc


def main(argv=None) -> int:
    from . import capi
    ap = build_parser()
    a = ap.parse_args(argv)
    gas, sinks = read_save(a.save, a.variable)
    try:
        seeds, shape = seeds_from_args(a)
        kw = trace_options(a, sinks)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    res, d = trace_rows(gas, sinks, seeds, a.steps, a.ds, a.both, a.variable, a.device, **kw)
    out = dict(path=res[0], seeds=seeds, shape=np.array(shape, dtype=np.int64), counts=np.array(res[-1], dtype=np.int64))
    if a.both:
        out.update(status_up=res[1][0], status=res[1][1], n_done_up=res[2][0], n_done=res[2][1])
    else:
        out.update(status=res[1], n_done=res[2])
    if a.carry is not None:
        out["carry"] = res[3]
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    summary = {"n_seeds": int(seeds.shape[0]), "n_steps": a.steps, "rows": int(res[0].shape[0]),
               **{k: int(v) for k, v in zip(capi.TRACE_STATUS, res[-1])}}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: {seeds.shape[0]} lines of {a.steps} steps from {gas.shape[0]} gas rows: " +
              ", ".join(f"{v} {k}" for k, v in zip(capi.TRACE_STATUS, res[-1])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
