"""Advances a save file on the GPU with drag-coupled tracer grains beside the gas (include/summersph.h, sph_dust): where a mm
grain goes, compared with a micron grain -- into the arms and clumps, onto a sink, out of the disc.

    python -m summersph_amd.dust SAVE.txt --steps 500 [--dt 1e-2] [--grains 10000] [--seed 1]
                                 (--size-cm 0.1 [--rho-grain 3] | --stopping-time TS)
                                 [--every 1] [--record-every 5] [--remove] [-o DUST.npz] [--json]
                                 [--variable] [--self-gravity] [--accrete] [--capacity ROWS]

SAVE.txt is a save file as summersph_amd.profile reads it: records of 9 values (10 with --variable: .. alpha h) are gas,
records of 8 values (x y z vx vy vz 0 m) are sinks.  The rows are uploaded into a fresh context, --grains grains start at
the positions and velocities of randomly chosen gas particles (--seed), a row is recorded for t = 0, and one sph_run of
--steps steps with the first time step --dt follows; every --every-th step advances the grains on the device, every
--record-every-th advance appends a row, and the log is read back once at the end.  --size-cm and --rho-grain (g / cm^3,
default 3) give Epstein drag with the code's units taken as AU and M_sun (G = 1); --stopping-time gives every grain that
fixed stopping time in code units instead.  --remove lets the sinks accrete grains and the bound cull them.  -o writes the
head's columns (advance, t, delta, n_live), body (rows, 12, M), the named columns (capi.DUST_COLUMNS, listed in
`columns`), fates (M, 3: fate, advance, sink), par and the end state as an .npz file.  --json prints one JSON object: the
grain, row, advance and live counts, the fates' tally and the end time.

The helpers: from_gas (grains from a gas state), keplerian (grains on circular orbits about the sinks' centre of mass),
code_units (g / cm^3 and cm to M_sun / AU^3 and AU) and stopping_time (1 / rate of a row).
"""
from __future__ import annotations

import argparse
import json
import math
import sys

import numpy as np

from .cli import desc_arrays, read_save, uploaded_context

AU_CM = 1.495978707e13
MSUN_G = 1.98847e33


def from_gas(state, n, seed=0):
    """n grains at the positions and velocities of randomly chosen gas particles (without repeats while the gas has
    enough): (x (n, 3), v (n, 3)).  state: a dict of arrays as Context.state returns."""
    x = np.stack([np.asarray(state[k], dtype=np.float64) for k in "xyz"], axis=1)
    v = np.stack([np.asarray(state[k], dtype=np.float64) for k in ("vx", "vy", "vz")], axis=1)
    n = int(n)
    if n < 1 or x.shape[0] < 1:
        raise ValueError("dust: at least one grain and one gas particle are wanted")
    pick = np.random.default_rng(seed).choice(x.shape[0], n, replace=n > x.shape[0])
    return x[pick].copy(), v[pick].copy()


def keplerian(sinks, R, phi, z=0.0, G=1.0):
    """Grains on circular orbits of cylindrical radius R at azimuth phi and height z about the sinks' centre of mass, in
    its frame, with the speed sqrt(G M / R) of the sinks' total mass: (x (n, 3), v (n, 3)).  sinks: a dict with x y z vx vy
    vz m, as Context.get_sinks returns."""
    m = np.asarray(sinks["m"], dtype=np.float64)
    M = float(np.sum(m))
    if not M > 0.0:
        raise ValueError("dust: the sinks have no mass")
    c = np.array([np.sum(m * np.asarray(sinks[k], dtype=np.float64)) / M for k in "xyz"])
    cv = np.array([np.sum(m * np.asarray(sinks[k], dtype=np.float64)) / M for k in ("vx", "vy", "vz")])
    R, phi, z = np.broadcast_arrays(np.asarray(R, dtype=np.float64), np.asarray(phi, dtype=np.float64), np.asarray(z, dtype=np.float64))
    R, phi, z = R.reshape(-1), phi.reshape(-1), z.reshape(-1)
    if np.any(~(R > 0.0)):
        raise ValueError("dust: R must be > 0")
    vk = np.sqrt(G * M / R)
    x = np.stack([R * np.cos(phi), R * np.sin(phi), z], axis=1) + c
    v = np.stack([-vk * np.sin(phi), vk * np.cos(phi), np.zeros_like(R)], axis=1) + cv
    return x, v


def code_units(rho_grain_g_cm3, size_cm):
    """(rho_grain in M_sun / AU^3, size in AU): the Epstein law's two numbers in the code's units (AU, M_sun, G = 1)"""
    return float(rho_grain_g_cm3) * AU_CM ** 3 / MSUN_G, np.asarray(size_cm, dtype=np.float64) / AU_CM


def stopping_time(row):
    """t_s = 1 / rate of a row (or of all rows) of Context.dust's dict; inf where no gas is in reach"""
    r = np.asarray(row["rate"] if isinstance(row, dict) else row, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(r > 0.0, 1.0 / r, np.inf)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.dust", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("--steps", type=int, required=True, help="steps to run")
    ap.add_argument("--dt", type=float, default=1e-2, help="the first time step (default 1e-2)")
    ap.add_argument("--grains", type=int, default=10000, help="grains, started on randomly chosen gas particles")
    ap.add_argument("--seed", type=int, default=1, help="seed of the choice")
    law = ap.add_mutually_exclusive_group(required=True)
    law.add_argument("--size-cm", type=float, default=None, help="Epstein drag: the grain size in cm")
    law.add_argument("--stopping-time", type=float, default=None, help="a fixed stopping time in code units")
    ap.add_argument("--rho-grain", type=float, default=3.0, help="with --size-cm: the grains' material density in g / cm^3")
    ap.add_argument("--every", type=int, default=1, help="advance the grains every k-th step (default 1)")
    ap.add_argument("--record-every", type=int, default=1, help="append a row every k-th advance (default 1)")
    ap.add_argument("--remove", action="store_true", help="sinks accrete grains, the bound culls them")
    ap.add_argument("--capacity", type=int, default=None, help="rows the log holds (default: every recorded advance + 1)")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--self-gravity", action="store_true", help="with the gas self-gravity term (on the gas only)")
    ap.add_argument("--accrete", action="store_true", help="with accretion of gas onto the sinks and the boundary cull")
    ap.add_argument("-o", "--out", default=None, help="write the rows, the named columns, the fates and the end state to this .npz file")
    ap.add_argument("--json", action="store_true", help="print one JSON object")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.steps < 0:
        ap.error("--steps must be >= 0")
    if a.grains < 1:
        ap.error("--grains must be >= 1")
    if a.every < 1 or a.record_every < 1:
        ap.error("--every and --record-every must be >= 1")
    if not (math.isfinite(a.dt) and a.dt > 0.0):
        ap.error("--dt must be a positive number")
    for name in ("size_cm", "stopping_time"):
        v = getattr(a, name)
        if v is not None and not (math.isfinite(v) and v > 0.0):
            ap.error(f"--{name.replace('_', '-')} must be a positive number")
    if not (math.isfinite(a.rho_grain) and a.rho_grain > 0.0):
        ap.error("--rho-grain must be a positive number")
    if a.capacity is None:
        a.capacity = (a.steps // a.every) // a.record_every + 1
    if a.capacity < 0:
        ap.error("--capacity must be >= 0")
    return a


def tally(fates: dict) -> dict:
    """the fates counted: alive, accreted, culled, nonfinite, and the accreted per sink index"""
    from . import capi
    fate, sink = np.asarray(fates["fate"]), np.asarray(fates["sink"])
    acc = fate == capi.DUST_ACCRETED
    per = {str(int(s)): int(np.sum(acc & (sink == s))) for s in np.unique(sink[acc])}
    return {"alive": int(np.sum(fate == capi.DUST_ALIVE)), "accreted": int(np.sum(acc)), "culled": int(np.sum(fate == capi.DUST_CULLED)),
            "nonfinite": int(np.sum(fate == capi.DUST_NONFINITE)), "per_sink": per}


def run_dust(gas, sinks, n_grains, steps, law, par, rho_grain=None, every=1, record_every=1, remove=False, dt=1e-2, capacity=None,
             seed=1, variable=False, self_gravity=False, accrete=False, device=0):
    """Uploads the rows into a fresh context, begins n_grains grains on gas particles, records t = 0 and one run of `steps`
    steps; (Context.dust's dict, Context.dust_fates' dict, Context.dust_info's dict, Context.dust_state's dict, the
    DustDesc, the last dt, the end time)"""
    from . import capi
    flags = ((capi.FLAG_VARIABLE_H if variable else 0) | (capi.FLAG_SELF_GRAVITY if self_gravity else 0) |
             (capi.FLAG_ACCRETE_CULL if accrete else 0))
    with uploaded_context(gas, sinks, variable, device, flags=flags) as ctx:
        x, v = from_gas({k: gas[:, i] for i, k in enumerate("x y z vx vy vz".split())}, n_grains, seed)
        ctx.set_dt(dt, 0.0)
        cap = (steps // every) // record_every + 1 if capacity is None else capacity
        ctx.dust_begin(x, v, np.broadcast_to(np.asarray(par, dtype=np.float64), (x.shape[0],)).copy(), law=law, rho_grain=rho_grain,
                       capacity=cap, every=every, record_every=record_every, remove=remove)
        ctx.dust_advance()
        dt_end, t_end = ctx.run(steps, dt, 0.0)
        return ctx.dust(), ctx.dust_fates(), ctx.dust_info(), ctx.dust_state(), ctx.dust_desc, dt_end, t_end


def main(argv=None) -> int:
    from . import capi
    a = parse_args(argv)
    gas, sinks = read_save(a.save, a.variable)
    if gas.shape[0] < 1:
        print(f"{a.save}: no gas rows", file=sys.stderr)
        return 1
    if a.size_cm is not None:
        law = "epstein"
        rho_grain, par = code_units(a.rho_grain, a.size_cm)
    else:
        law, rho_grain, par = "fixed_ts", None, a.stopping_time
    d, fates, info, state, desc, dt_end, t_end = run_dust(gas, sinks, a.grains, a.steps, law, par, rho_grain, a.every, a.record_every,
                                                          a.remove, a.dt, a.capacity, a.seed, a.variable, a.self_gravity, a.accrete,
                                                          a.device)
    if a.out is not None:
        np.savez(a.out, **{k: np.asarray(v) for k, v in d.items()}, columns=np.array(capi.DUST_COLUMNS),
                 fates=np.stack([fates[k] for k in capi.DUST_FATES], axis=1), par=state["par"],
                 **{"end_" + k: state[k] for k in capi.DUST_STATE[:6]}, dt_end=dt_end, t_end=t_end, **desc_arrays(desc))
    s = {"grains": info["n_grains"], "rows": info["rows"], "dropped": info["dropped"], "advances": info["advances"],
         "live": info["n_live"], "fates": tally(fates), "t_end": t_end, "law": law}
    if a.json:
        print(json.dumps(s))
        return 0
    f = s["fates"]
    print(f"{a.save}: {gas.shape[0]} gas rows, {sinks.shape[0]} sinks, {s['grains']} grains ({law}), {a.steps} steps to t = {t_end:.6g}: "
          f"{s['advances']} advances, {s['rows']} rows kept, {s['dropped']} dropped")
    print(f"  alive {f['alive']}  accreted {f['accreted']}  culled {f['culled']}  nonfinite {f['nonfinite']}" +
          "".join(f"  sink {k}: {v}" for k, v in f["per_sink"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
