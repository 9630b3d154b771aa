"""Advances a save file on the GPU and records a movie of the run: column-density maps of the gas, and maps weighted by
chosen fields, appended on the device at a uniform cadence in simulation time (include/summersph.h, sph_frames).

    python -m summersph_amd.frames SAVE.txt --steps 500 --dt-frame 0.5 --size 256 --extent 200 [--inc 40 --pa 30]
                                    [--fields u,vx] [--follow-sink 0] [-o movie.npz] [--png-dir frames/] [--json]
                                    [--every K] [--dt 1e-2] [--variable] [--self-gravity] [--accrete] [--capacity ROWS]

SAVE.txt is a save file as summersph_amd.profile reads it.  The rows are uploaded into a fresh context, frame 0 is recorded
for the state as it is (after a density pass), and one sph_run of --steps steps with the first time step --dt follows;
a frame is appended whenever t passes the next multiple of --dt-frame (the reference's save rule) or, with --every, after
every K-th step, and the log is read back once at the end.  --follow-sink centres every frame on that sink's position at
the time of the frame.  -o writes planes (rows, 1 + nq, size, size), the heads' columns and the nodes as an .npz file;
--png-dir writes one image of log10 of the column density per frame (needs matplotlib).  mean(planes) turns the weighted
planes into line-of-sight means.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from .cli import desc_arrays, parse_fields, read_save, uploaded_context
from .cube import parse_clip, parse_vec, view


def mean(planes):
    """planes[..., 1:, :, :] / planes[..., :1, :, :]: the column-weighted line-of-sight means of the fields, NaN where the
    column density is 0.  planes: (1 + nq, n_u, n_v) or (rows, 1 + nq, n_u, n_v)."""
    p = np.asarray(planes, dtype=np.float64)
    if p.ndim not in (3, 4) or p.shape[-3] < 1:
        raise ValueError("mean: planes must be (1 + nq, n_u, n_v) or (rows, 1 + nq, n_u, n_v)")
    col = p[..., :1, :, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(col != 0.0, p[..., 1:, :, :] / col, np.nan)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.frames", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("--steps", type=int, required=True, help="steps to run")
    ap.add_argument("--dt-frame", type=float, default=None, help="a frame every DT_FRAME of simulation time")
    ap.add_argument("--every", type=int, default=None, help="a frame every K-th step (instead of --dt-frame)")
    ap.add_argument("--dt", type=float, default=1e-2, help="the first time step (default 1e-2)")
    ap.add_argument("--size", type=int, default=256, help="image nodes per axis")
    ap.add_argument("--extent", type=float, required=True, help="full width of the square image (centred on --centre)")
    ap.add_argument("--inc", type=float, default=0.0, help="inclination in degrees (0: face-on)")
    ap.add_argument("--pa", type=float, default=0.0, help="position angle of the line of nodes in degrees")
    ap.add_argument("--azimuth", type=float, default=0.0, help="turn of the disc about z in degrees")
    ap.add_argument("--centre", default="0,0,0", help="image centre x,y,z (added to the sink's position with --follow-sink)")
    ap.add_argument("--follow-sink", type=int, default=None, help="centre every frame on this sink")
    ap.add_argument("--fields", default="", help="up to three comma-separated field names: one weighted plane each")
    ap.add_argument("--h", type=float, default=None, help="one h for every particle (default: each particle's own)")
    ap.add_argument("--clip", default=None, help="strict particle clip box x0,y0,z0,x1,y1,z1")
    ap.add_argument("--capacity", type=int, default=None, help="frames the log holds (default: steps + 1)")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--self-gravity", action="store_true", help="with the gas self-gravity term")
    ap.add_argument("--accrete", action="store_true", help="with accretion onto the sinks and the boundary cull")
    ap.add_argument("-o", "--out", default=None, help="write the log to this .npz file")
    ap.add_argument("--png-dir", default=None, help="write one image per frame into this folder (needs matplotlib)")
    ap.add_argument("--json", action="store_true", help="print one JSON object")
    ap.add_argument("--device", type=int, default=0)
    return ap


def args_desc(a):
    """Context.frames_begin's keyword arguments from the parsed command line"""
    if a.steps < 0:
        raise ValueError("--steps must be >= 0")
    if (a.dt_frame is None) == (a.every is None):
        raise ValueError("exactly one of --dt-frame and --every")
    if a.dt_frame is not None and not (math.isfinite(a.dt_frame) and a.dt_frame > 0.0):
        raise ValueError("--dt-frame must be a positive number")
    if a.every is not None and a.every < 1:
        raise ValueError("--every must be >= 1")
    if not (math.isfinite(a.dt) and a.dt > 0.0):
        raise ValueError("--dt must be a positive number")
    if a.size < 1:
        raise ValueError("--size must be >= 1")
    if not (math.isfinite(a.extent) and a.extent > 0):
        raise ValueError("--extent must be finite and > 0")
    if a.h is not None and not (math.isfinite(a.h) and a.h > 0):
        raise ValueError("--h must be finite and > 0")
    if a.follow_sink is not None and not 0 <= a.follow_sink < 64:
        raise ValueError("--follow-sink must be 0 .. 63")
    capacity = a.steps + 1 if a.capacity is None else a.capacity
    if capacity < 1:
        raise ValueError("--capacity must be >= 1")
    half = 0.5 * a.extent
    return dict(shape=(a.size, a.size), bounds=((-half, -half), (half, half)), capacity=capacity,
                every=1 if a.every is None else a.every, dt_frame=a.dt_frame, rot=view(a.inc, a.pa, a.azimuth),
                centre=parse_vec(a.centre), centre_sink=a.follow_sink, fields=tuple(parse_fields(a.fields, 0, 3, a.variable)),
                h=a.h, clip=None if a.clip is None else parse_clip(a.clip))


def run_frames(gas, sinks, steps, kw, dt=1e-2, variable=False, self_gravity=False, accrete=False, device=0):
    """Uploads the rows into a fresh context, records frame 0 and one run of `steps` steps; (Context.frames' dict, the
    FramesDesc, the last dt, the end time)"""
    from . import capi
    flags = ((capi.FLAG_VARIABLE_H if variable else 0) | (capi.FLAG_SELF_GRAVITY if self_gravity else 0) |
             (capi.FLAG_ACCRETE_CULL if accrete else 0))
    with uploaded_context(gas, sinks, variable, device, flags=flags) as ctx:
        ctx.set_dt(dt, 0.0)
        ctx.frames_begin(**kw)
        ctx.density()
        ctx.frames_record()
        dt_end, t_end = ctx.run(steps, dt, 0.0)
        return ctx.frames(), ctx.frames_desc, dt_end, t_end


def write_pngs(plt, folder, log, bounds):
    os.makedirs(folder, exist_ok=True)
    (lo_u, lo_v), (hi_u, hi_v) = bounds
    for r in range(log["planes"].shape[0]):
        col = log["planes"][r, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            img = np.where(col > 0, np.log10(col), np.nan)
        fig, ax = plt.subplots(figsize=(5, 5))
        ax.imshow(img.T, origin="lower", extent=(lo_u, hi_u, lo_v, hi_v), cmap="inferno")
        ax.set_title(f"step {int(log['step'][r])}   t = {float(log['t'][r]):.6g}")
        fig.savefig(os.path.join(folder, f"frame_{r:05d}.png"), dpi=100)
        plt.close(fig)


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        kw = args_desc(a)
    except ValueError as e:
        ap.error(str(e))
    plt = None
    if a.png_dir:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("--png-dir needs matplotlib, which is not importable here", file=sys.stderr)
            return 2
    gas, sinks = read_save(a.save, a.variable)
    log, d, dt_end, t_end = run_frames(gas, sinks, a.steps, kw, a.dt, a.variable, a.self_gravity, a.accrete, a.device)
    (lo_u, lo_v), (hi_u, hi_v) = kw["bounds"]
    if a.out is not None:
        np.savez(a.out, **{k: np.asarray(v) for k, v in log.items()}, u_nodes=np.linspace(lo_u, hi_u, a.size),
                 v_nodes=np.linspace(lo_v, hi_v, a.size), rot=kw["rot"], dt_end=dt_end, t_end=t_end, **desc_arrays(d))
    if plt is not None:
        write_pngs(plt, a.png_dir, log, kw["bounds"])
    rows = int(log["planes"].shape[0])
    summary = {"rows": rows, "dropped": log["dropped"], "steps": log["step"].tolist(), "t": log["t"].tolist(),
               "n_sel": log["n_sel"].tolist(), "status": log["status"].tolist(), "shape": list(log["planes"].shape),
               "t_end": t_end}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.save}: {gas.shape[0]} gas rows, {sinks.shape[0]} sinks, {a.steps} steps to t = {t_end:.6g}: "
              f"{rows} frames of {log['planes'].shape[1:]} kept, {log['dropped']} dropped")
    return 0


if __name__ == "__main__":
    sys.exit(main())
