"""Advances a save file on the GPU and records the per-step time series of the run: the dt every step chose, the particle
and sink counts, the conserved totals, the peak density and the sinks' orbits (include/summersph.h, sph_history).

    python -m summersph_amd.history SAVE.txt --steps 500 [--every 1] [--dt 1e-2] [-o HIST.npz] [--json]
                                    [--variable] [--self-gravity] [--accrete] [--capacity ROWS]

SAVE.txt is a save file as summersph_amd.profile reads it: records of 9 values (10 with --variable: .. alpha h) are gas,
records of 8 values (x y z vx vy vz 0 m) are sinks.  The rows are uploaded into a fresh context, a row is recorded for the
state as it is (step 0, after a density pass), and one sph_run of --steps steps with the first time step --dt follows;
every --every-th step records a row on the device, and the log is read back once at the end.  --self-gravity adds the gas
self-gravity term, --accrete the accretion onto the sinks and the boundary cull; --capacity bounds the rows kept (default:
all).  -o writes the rows and the named columns (capi.HISTORY_COLUMNS, E, P, L, sinks ...) as an .npz file.  --json prints
one JSON object: the first and the last row, the rows kept and dropped, and the relative drift of E, |P| and |L| between
them.  W_self is not part of a row: E is the energy without the gas self-potential (take summersph_amd.energy at
snapshots for it).
"""
from __future__ import annotations

import argparse
import json
import math
import sys

import numpy as np

from .cli import desc_arrays, read_save, uploaded_context


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.history", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("--steps", type=int, required=True, help="steps to run")
    ap.add_argument("--every", type=int, default=1, help="record every k-th step (default 1)")
    ap.add_argument("--dt", type=float, default=1e-2, help="the first time step (default 1e-2)")
    ap.add_argument("--capacity", type=int, default=None, help="rows the log holds (default: every recorded step + 1)")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--self-gravity", action="store_true", help="with the gas self-gravity term")
    ap.add_argument("--accrete", action="store_true", help="with accretion onto the sinks and the boundary cull")
    ap.add_argument("-o", "--out", default=None, help="write the rows and the named columns to this .npz file")
    ap.add_argument("--json", action="store_true", help="print one JSON object")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.steps < 0:
        ap.error("--steps must be >= 0")
    if a.every < 1:
        ap.error("--every must be >= 1")
    if not (math.isfinite(a.dt) and a.dt > 0.0):
        ap.error("--dt must be a positive number")
    if a.capacity is None:
        a.capacity = a.steps // a.every + 1
    if not 1 <= a.capacity < 2**31:
        ap.error("--capacity must be 1 .. 2^31 - 1")
    return a


def drift(first: float, last: float) -> float:
    """(last - first) / |first|; the plain difference where first is 0"""
    return (last - first) / abs(first) if first != 0.0 else last - first


def summary(h: dict) -> dict:
    """What --json prints for Context.history's dict"""
    rows = h["rows"]
    if rows.shape[0] == 0:
        return {"rows": 0, "dropped": h["dropped"]}
    p, l = np.linalg.norm(h["P"], axis=1), np.linalg.norm(h["L"], axis=1)
    return {"rows": int(rows.shape[0]), "dropped": h["dropped"], "first": rows[0].tolist(), "last": rows[-1].tolist(),
            "drift": {"E": drift(float(h["E"][0]), float(h["E"][-1])), "P": drift(float(p[0]), float(p[-1])),
                      "L": drift(float(l[0]), float(l[-1]))}}


def run_history(gas, sinks, steps, every=1, dt=1e-2, capacity=None, variable=False, self_gravity=False, accrete=False, device=0):
    """Uploads the rows into a fresh context, records step 0 and one run of `steps` steps; (Context.history's dict, the
    HistoryDesc, the last dt, the end time)"""
    from . import capi
    flags = ((capi.FLAG_VARIABLE_H if variable else 0) | (capi.FLAG_SELF_GRAVITY if self_gravity else 0) |
             (capi.FLAG_ACCRETE_CULL if accrete else 0))
    with uploaded_context(gas, sinks, variable, device, flags=flags) as ctx:
        ctx.set_dt(dt, 0.0)
        ctx.history_begin(steps // every + 1 if capacity is None else capacity, every)
        ctx.density()
        ctx.history_record()
        dt_end, t_end = ctx.run(steps, dt, 0.0)
        return ctx.history(), ctx.history_desc, dt_end, t_end


def main(argv=None) -> int:
    a = parse_args(argv)
    gas, sinks = read_save(a.save, a.variable)
    h, d, dt_end, t_end = run_history(gas, sinks, a.steps, a.every, a.dt, a.capacity, a.variable, a.self_gravity, a.accrete, a.device)
    if a.out is not None:
        np.savez(a.out, **{k: np.asarray(v) for k, v in h.items()}, dt_end=dt_end, t_end=t_end, **desc_arrays(d))
    if a.json:
        print(json.dumps(summary(h)))
        return 0
    s = summary(h)
    print(f"{a.save}: {gas.shape[0]} gas rows, {sinks.shape[0]} sinks, {a.steps} steps to t = {t_end:.6g}: "
          f"{s['rows']} rows kept, {s['dropped']} dropped")
    if s["rows"]:
        for k in ("E", "P", "L"):
            print(f"  drift of {'E' if k == 'E' else '|' + k + '|':4s} {s['drift'][k]: .6e}")
        print(f"  rho_max {h['rho_max'][0]: .6e} -> {h['rho_max'][-1]: .6e}   n {h['n'][0]} -> {h['n'][-1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
