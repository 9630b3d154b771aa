"""Advances a save file on the GPU and records the trajectories and fates of chosen particles (include/summersph.h,
sph_track): where this gas went, how it was heated on the way, and which sink swallowed it.

    python -m summersph_amd.track SAVE.txt --steps 500 [--every 1] [--dt 1e-2]
                                  (--ids IDS.npy | --sphere X Y Z R | --ring R0 R1 [--zmax Z] | --stride S)
                                  [-o TRACK.npz] [--json] [--variable] [--self-gravity] [--accrete] [--capacity ROWS]

SAVE.txt is a save file as summersph_amd.profile reads it: records of 9 values (10 with --variable: .. alpha h) are gas,
records of 8 values (x y z vx vy vz 0 m) are sinks.  The rows are uploaded into a fresh context, the particles are chosen
by their row numbers (--ids: an .npy file of integers; --sphere: within R of a point; --ring: cylindrical radius in
[R0, R1), |z| <= --zmax; --stride: every S-th row), a row is recorded for the state as it is (step 0, after a density pass),
and one sph_run of --steps steps with the first time step --dt follows; every --every-th step records a row on the device,
and the log is read back once at the end.  -o writes the ids, the head's columns, body (rows, 10, K), the named columns
(capi.TRACK_COLUMNS), the fates (fates_fate, fates_step, fates_sink, fates_current_id) and n_live_end as an .npz file.
--json prints one JSON object: the tracked and the live count, the fates' tally (alive, culled, accreted per sink), and
the first and the last row's head.

The selection helpers return id arrays from a state (a dict of arrays as Context.state returns, or any mapping with x, y, z):
sphere_ids, ring_ids, stride_ids, and label_ids for the labels of Context.groups / Context.peaks.
"""
from __future__ import annotations

import argparse
import json
import math
import sys

import numpy as np

from .cli import desc_arrays, read_save, uploaded_context


# ---- selections: ids in the caller's order ----------------------------------------------------------------------------------
def _xyz(state):
    x, y, z = (np.asarray(state[k], dtype=np.float64) for k in "xyz")
    if not (x.ndim == 1 and x.shape == y.shape == z.shape):
        raise ValueError("track: x, y and z must be 1-D arrays of one length")
    return x, y, z


def sphere_ids(state, centre, radius) -> np.ndarray:
    """The particles within `radius` of `centre` (|r - centre|^2 <= radius^2), ascending"""
    x, y, z = _xyz(state)
    cx, cy, cz = (float(v) for v in centre)
    if not float(radius) >= 0.0:
        raise ValueError("track: radius must be >= 0")
    d2 = ((x - cx) ** 2 + (y - cy) ** 2) + (z - cz) ** 2
    return np.flatnonzero(d2 <= float(radius) ** 2).astype(np.int64)


def ring_ids(state, rmin, rmax, zmax=None) -> np.ndarray:
    """The particles with cylindrical radius rmin <= R < rmax about the z axis (and |z| <= zmax where given), ascending"""
    x, y, z = _xyz(state)
    if not 0.0 <= float(rmin) <= float(rmax):
        raise ValueError("track: 0 <= rmin <= rmax")
    r2 = x ** 2 + y ** 2
    sel = (r2 >= float(rmin) ** 2) & (r2 < float(rmax) ** 2)
    if zmax is not None:
        sel &= np.abs(z) <= float(zmax)
    return np.flatnonzero(sel).astype(np.int64)


def stride_ids(n, stride, offset=0) -> np.ndarray:
    """offset, offset + stride, ... below n"""
    n, stride, offset = int(n), int(stride), int(offset)
    if n < 0 or stride < 1 or offset < 0:
        raise ValueError("track: n >= 0, stride >= 1, offset >= 0")
    return np.arange(offset, n, stride, dtype=np.int64)


def label_ids(labels, group) -> np.ndarray:
    """The members of group `group` (or of any group of a sequence of them) in the labels of Context.groups / Context.peaks"""
    lab = np.asarray(labels)
    if lab.ndim != 1:
        raise ValueError("track: labels must be 1-D")
    return np.flatnonzero(np.isin(lab, np.atleast_1d(np.asarray(group)))).astype(np.int64)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.track", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("--steps", type=int, required=True, help="steps to run")
    ap.add_argument("--every", type=int, default=1, help="record every k-th step (default 1)")
    ap.add_argument("--dt", type=float, default=1e-2, help="the first time step (default 1e-2)")
    sel = ap.add_mutually_exclusive_group(required=True)
    sel.add_argument("--ids", default=None, help=".npy file of row numbers")
    sel.add_argument("--sphere", type=float, nargs=4, metavar=("X", "Y", "Z", "R"), help="within R of (X, Y, Z)")
    sel.add_argument("--ring", type=float, nargs=2, metavar=("R0", "R1"), help="cylindrical radius in [R0, R1)")
    sel.add_argument("--stride", type=int, default=None, help="every S-th row")
    ap.add_argument("--zmax", type=float, default=None, help="with --ring: |z| <= this")
    ap.add_argument("--capacity", type=int, default=None, help="rows the log holds (default: every recorded step + 1)")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--self-gravity", action="store_true", help="with the gas self-gravity term")
    ap.add_argument("--accrete", action="store_true", help="with accretion onto the sinks and the boundary cull")
    ap.add_argument("-o", "--out", default=None, help="write the rows, the named columns and the fates to this .npz file")
    ap.add_argument("--json", action="store_true", help="print one JSON object")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.steps < 0:
        ap.error("--steps must be >= 0")
    if a.every < 1:
        ap.error("--every must be >= 1")
    if not (math.isfinite(a.dt) and a.dt > 0.0):
        ap.error("--dt must be a positive number")
    if a.stride is not None and a.stride < 1:
        ap.error("--stride must be >= 1")
    if a.sphere is not None and not (all(math.isfinite(v) for v in a.sphere) and a.sphere[3] >= 0.0):
        ap.error("--sphere wants a finite point and a radius >= 0")
    if a.ring is not None and not 0.0 <= a.ring[0] <= a.ring[1]:
        ap.error("--ring wants 0 <= R0 <= R1")
    if a.zmax is not None and (a.ring is None or not a.zmax >= 0.0):
        ap.error("--zmax goes with --ring and must be >= 0")
    if a.capacity is None:
        a.capacity = a.steps // a.every + 1
    if a.capacity < 1:
        ap.error("--capacity must be >= 1")
    return a


def select(a, gas) -> np.ndarray:
    """the ids the arguments choose among the gas rows"""
    state = {k: gas[:, i] for i, k in enumerate("xyz")}
    if a.ids is not None:
        ids = np.load(a.ids)
        if ids.ndim != 1 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"{a.ids}: a 1-D array of integers is wanted")
        return ids.astype(np.int64)
    if a.sphere is not None:
        return sphere_ids(state, a.sphere[:3], a.sphere[3])
    if a.ring is not None:
        return ring_ids(state, a.ring[0], a.ring[1], a.zmax)
    return stride_ids(gas.shape[0], a.stride)


def tally(fates: dict) -> dict:
    """the fates counted: alive, culled, accreted, and the accreted per sink index"""
    from . import capi
    fate, sink = np.asarray(fates["fate"]), np.asarray(fates["sink"])
    acc = fate == capi.TRACK_ACCRETED
    per = {str(int(s)): int(np.sum(acc & (sink == s))) for s in np.unique(sink[acc])}
    return {"alive": int(np.sum(fate == capi.TRACK_ALIVE)), "culled": int(np.sum(fate == capi.TRACK_CULLED)),
            "accreted": int(np.sum(acc)), "per_sink": per}


def summary(t: dict, fates: dict, n_live: int) -> dict:
    """What --json prints for Context.track's and Context.track_fates' dicts"""
    head = t["head"]
    out = {"rows": int(head.shape[0]), "dropped": t["dropped"], "n_tracked": int(np.asarray(fates["fate"]).size),
           "n_live": int(n_live), "fates": tally(fates)}
    if head.shape[0]:
        out["first"] = dict(zip(("step", "t", "n", "n_live"), head[0].tolist()))
        out["last"] = dict(zip(("step", "t", "n", "n_live"), head[-1].tolist()))
    return out


def run_track(gas, sinks, ids, steps, every=1, dt=1e-2, capacity=None, variable=False, self_gravity=False, accrete=False, device=0):
    """Uploads the rows into a fresh context, records step 0 and one run of `steps` steps; (Context.track's dict,
    Context.track_fates' dict, Context.track_info's dict, the TrackDesc, the last dt, the end time)"""
    from . import capi
    flags = ((capi.FLAG_VARIABLE_H if variable else 0) | (capi.FLAG_SELF_GRAVITY if self_gravity else 0) |
             (capi.FLAG_ACCRETE_CULL if accrete else 0))
    with uploaded_context(gas, sinks, variable, device, flags=flags) as ctx:
        ctx.set_dt(dt, 0.0)
        ctx.track_begin(ids, steps // every + 1 if capacity is None else capacity, every)
        ctx.density()
        ctx.track_record()
        dt_end, t_end = ctx.run(steps, dt, 0.0)
        return ctx.track(), ctx.track_fates(), ctx.track_info(), ctx.track_desc, dt_end, t_end


def main(argv=None) -> int:
    a = parse_args(argv)
    gas, sinks = read_save(a.save, a.variable)
    ids = select(a, gas)
    if ids.size < 1:
        print(f"{a.save}: the selection holds no particle", file=sys.stderr)
        return 1
    t, fates, info, d, dt_end, t_end = run_track(gas, sinks, ids, a.steps, a.every, a.dt, a.capacity, a.variable, a.self_gravity,
                                                 a.accrete, a.device)
    if a.out is not None:
        np.savez(a.out, ids=ids, **{k: np.asarray(v) for k, v in t.items()}, **{"fates_" + k: v for k, v in fates.items()},
                 n_live_end=info["n_live"], dt_end=dt_end, t_end=t_end, **desc_arrays(d))
    s = summary(t, fates, info["n_live"])
    if a.json:
        print(json.dumps(s))
        return 0
    f = s["fates"]
    print(f"{a.save}: {gas.shape[0]} gas rows, {sinks.shape[0]} sinks, {ids.size} tracked, {a.steps} steps to t = {t_end:.6g}: "
          f"{s['rows']} rows kept, {s['dropped']} dropped")
    print(f"  alive {f['alive']}  culled {f['culled']}  accreted {f['accreted']}" +
          "".join(f"  sink {k}: {v}" for k, v in f["per_sink"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
