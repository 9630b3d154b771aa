#!/usr/bin/env python3
"""Times sph_energy on a Keplerian disc with self-gravity ("Conserved totals and the potential");
run it under `rocprofv3 --kernel-trace --stats -- python profiles/energy_time.py N` for the per-kernel times
(energy_stage, energy_box, the tree build over the staged records, grav_potential_wave, energy_pieces, energy_final) next
to one sph_forces (grav_walk_wave and its tree build) of the same snapshot.

  N   gas particles of ic.keplerian_disc(N, seed=5) with its sink (default 10^6); fixed h, SPH_FLAG_SELF_GRAVITY, theta 0.5

Prints one JSON line: wall time per call of the host form with phi (after one warm-up), of the device form (synchronised)
and of one sph_forces for comparison."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from summersph_amd import capi, ic  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=5))
    ctx = capi.Context(device=0, flags=capi.FLAG_SELF_GRAVITY)
    ctx.upload(gas); ctx.set_sinks(sinks)
    ctx.density(); ctx.forces()                              # the cell-sorted order of a running simulation
    out = {"n": ctx.n}
    ctx.energy(phi=True)                                     # warm-up (scratch, tree arrays, code objects)
    t0 = time.perf_counter()
    for _ in range(reps):
        e = ctx.energy(phi=True)
    out["host_phi_ms"] = (time.perf_counter() - t0) / reps * 1e3
    ctx.energy(device=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.energy(device=True)
    ctx.synchronize()
    out["device_ms"] = (time.perf_counter() - t0) / reps * 1e3
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.forces()                                             # its tree is rebuilt: sph_energy built over the staged records
    ctx.synchronize()
    out["forces_ms"] = (time.perf_counter() - t0) * 1e3
    out.update({k: e[k] for k in ("E", "K", "U", "W_self", "W_gs")})
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
