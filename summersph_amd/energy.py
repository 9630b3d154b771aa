"""Conserved totals of a save file on the GPU: kinetic, thermal and gravitational energy (gas self-gravity by the
Barnes-Hut walk, gas-sink and sink-sink terms), momentum, angular momentum and the centre of mass.

    python -m summersph_amd.energy SAVE.txt [--variable] [--no-self-gravity] [--theta T] [--phi OUT.npy] [--json]

SAVE.txt is a save file as summersph_amd.profile reads it: records of 9 values (10 with --variable: .. alpha h) are gas,
records of 8 values (x y z vx vy vz 0 m) are sinks.  The rows are uploaded into a fresh context and evaluated with
sph_energy (capi.Context.energy).  Self-gravity is on by default, because find_forces includes it ([F]:825);
--no-self-gravity leaves W_self out (the energy of a run without SPH_FLAG_SELF_GRAVITY).  --theta sets the opening angle
(default 0.5, the reference's; a tiny value opens every node: the direct sum).  --phi writes Phi_self + Phi_sink of every
gas row (in file order) as a .npy file.  --json prints one JSON object (the named sums of capi.ENERGY_SUMS, E, P, L,
com and the raw sums) instead of the table.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .cli import read_save, uploaded_context


def energy_rows(gas, sinks, variable=False, self_gravity=True, theta=None, phi=False, device=0):
    """Uploads the rows into a fresh context and returns Context.energy's dict"""
    from . import capi
    flags = (capi.FLAG_VARIABLE_H if variable else 0) | (capi.FLAG_SELF_GRAVITY if self_gravity else 0)
    kw = {"flags": flags}
    if theta is not None:
        kw["theta"] = float(theta)
    with uploaded_context(gas, sinks, variable, device, **kw) as ctx:
        return ctx.energy(phi=phi)


def to_json(e: dict) -> dict:
    """Context.energy's dict without phi, arrays as lists"""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in e.items() if k != "phi"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.energy", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--no-self-gravity", dest="self_gravity", action="store_false", help="leave the gas self-gravity out")
    ap.add_argument("--theta", type=float, default=None, help="Barnes-Hut opening angle (default 0.5)")
    ap.add_argument("--phi", default=None, help="write the potential of every gas row to this .npy file")
    ap.add_argument("--json", action="store_true", help="print one JSON object")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.theta is not None and not (np.isfinite(a.theta) and a.theta > 0.0):
        ap.error("--theta must be a positive number")

    gas, sinks = read_save(a.save, a.variable)
    e = energy_rows(gas, sinks, a.variable, a.self_gravity, a.theta, a.phi is not None, a.device)
    if a.phi is not None:
        np.save(a.phi, e["phi"])
    if a.json:
        print(json.dumps(to_json(e)))
        return 0
    print(f"{a.save}: {gas.shape[0]} gas rows, {sinks.shape[0]} sinks, self-gravity {'on' if a.self_gravity else 'off'}")
    for k in ("E", "K", "U", "W_self", "W_gs", "K_s", "W_ss", "M", "Ms"):
        print(f"  {k:7s} {e[k]: .12e}")
    for k in ("P", "L", "com"):
        print(f"  {k:7s} " + " ".join(f"{v: .12e}" for v in e[k]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
