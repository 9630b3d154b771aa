"""The rates of a save file split by physical term on the GPU, and what a disc modeller sums from them: net force, torque
and power per term, PdV work against viscous heating, torque and heating per ring.

    python -m summersph_amd.terms SAVE.txt -o OUT.npz [--json] [--rings RMIN RMAX N [--log]] [--centre x,y,z]
                                  [--normal x,y,z] [--no-gravity] [--self-gravity] [--variable]

SAVE.txt is a save file as summersph_amd.profile reads it (9-value gas records, 10 with --variable, 8-value sink records).
The gas and the sinks are uploaded into a fresh context, the density is evaluated and the rates are taken apart with
sph_force_terms (capi.Context.force_terms): a (16, n) array whose rows are capi.TERM_ROWS.  --self-gravity creates the
context with FLAG_SELF_GRAVITY (rows 9-11: the Barnes-Hut term); --no-gravity skips the tree walk (rows 9-11 NaN).

OUT.npz holds `rows`, the totals of totals() by name (`force`, `torque`, `power`: one line per term in TERMS order; `du_P`,
`du_V`) and, with --rings, `edges`, `ring_torques` (4, n_rings) and `ring_heating` (2, n_rings: sum m du_V, sum m du_P).
--json prints the totals as one JSON line.

The rings are sph_profile's (include/summersph.h, "Frame" and "Bins"): the same frame about the centre and the normal, the
same edges, ring k: edge[k] <= R < edge[k + 1] -- so they line up with a profile table of the same arguments.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

TERMS = ["pressure", "viscosity", "sinks", "self_gravity"]      # rows 0-2, 3-5, 6-8, 9-11 of capi.TERM_ROWS
ROW_DU_P, ROW_DU_V = 12, 13


def _targets(rows):
    """the columns that are targets (ghosts' columns are NaN in every row)"""
    return np.isfinite(rows[0])


def _rel(state, centre):
    return np.stack([np.asarray(state[k], dtype=np.float64) - c for k, c in zip("xyz", centre)])


def ring_edges(r_min, r_max, n_r, log=False):
    """sph_profile's ring edges (include/summersph.h, "Bins")"""
    if not (n_r >= 1 and 0.0 <= r_min < r_max and np.isfinite(r_max)) or (log and r_min <= 0.0):
        raise ValueError("rings: 0 <= r_min < r_max (log: r_min > 0) and n >= 1")
    k = np.arange(n_r + 1, dtype=np.float64)
    e = r_min * (r_max / r_min) ** (k / n_r) if log else r_min + (k * (r_max - r_min)) / n_r
    e[-1] = r_max
    return e


def ring_index(state, edges, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """ring of every particle in sph_profile's frame, -1 outside edges[0] <= R < edges[-1]"""
    from .sample import frame
    _, e1, e2 = frame(normal)
    r = _rel(state, centre)
    X = (r[0] * e1[0] + r[1] * e1[1]) + r[2] * e1[2]
    Y = (r[0] * e2[0] + r[1] * e2[1]) + r[2] * e2[2]
    R = np.sqrt(X * X + Y * Y)
    edges = np.asarray(edges, dtype=np.float64)
    k = np.searchsorted(edges, R, side="right") - 1
    return np.where((R >= edges[0]) & (R < edges[-1]), np.clip(k, 0, edges.size - 2), -1)


def totals(state, rows, centre=(0.0, 0.0, 0.0)):
    """Sums over the targets, per term of TERMS: force (4, 3) = sum m a_k, torque (4, 3) = sum m r' x a_k about the centre,
    power (4,) = sum m v . a_k; and du_P = sum m du_P, du_V = sum m du_V.  A term whose rows are NaN (rows 9-11 with
    skip_gas_gravity) sums to NaN."""
    rows = np.asarray(rows, dtype=np.float64)
    t = _targets(rows)
    m = np.asarray(state["m"], dtype=np.float64)[t]
    r = _rel(state, centre)[:, t]
    v = np.stack([np.asarray(state[k], dtype=np.float64)[t] for k in ("vx", "vy", "vz")])
    force, torque, power = np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(4)
    for k in range(4):
        a = rows[3 * k:3 * k + 3][:, t]
        force[k] = (m * a).sum(axis=1)
        torque[k] = (m * np.cross(r, a, axis=0)).sum(axis=1)
        power[k] = (m * (v * a).sum(axis=0)).sum()
    return {"force": force, "torque": torque, "power": power,
            "du_P": float((m * rows[ROW_DU_P][t]).sum()), "du_V": float((m * rows[ROW_DU_V][t]).sum())}


def _per_ring(ring, n_rings, values):
    sel = ring >= 0
    return np.bincount(ring[sel], weights=values[sel], minlength=n_rings)[:n_rings]


def ring_torques(state, rows, edges, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """(4, n_rings): sum m (r' x a_k) . n^ over the targets of every ring, per term of TERMS; an empty ring holds 0"""
    from .sample import frame
    rows = np.asarray(rows, dtype=np.float64)
    n_hat = frame(normal)[0]
    t = _targets(rows)
    ring = np.where(t, ring_index(state, edges, centre, normal), -1)
    m = np.asarray(state["m"], dtype=np.float64)
    r = _rel(state, centre)
    n_rings = np.asarray(edges).size - 1
    out = np.zeros((4, n_rings))
    for k in range(4):
        c = np.cross(r, rows[3 * k:3 * k + 3], axis=0)
        out[k] = _per_ring(ring, n_rings, m * ((c[0] * n_hat[0] + c[1] * n_hat[1]) + c[2] * n_hat[2]))
    return out


def ring_heating(state, rows, edges, centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """(2, n_rings): sum m du_V (viscous heating) and sum m du_P (PdV work) over the targets of every ring"""
    rows = np.asarray(rows, dtype=np.float64)
    ring = np.where(_targets(rows), ring_index(state, edges, centre, normal), -1)
    m = np.asarray(state["m"], dtype=np.float64)
    n_rings = np.asarray(edges).size - 1
    return np.stack([_per_ring(ring, n_rings, m * rows[ROW_DU_V]), _per_ring(ring, n_rings, m * rows[ROW_DU_P])])


def _vec3(spec, what, nonzero=False):
    v = [float(t) for t in spec.split(",")]
    if len(v) != 3 or not all(np.isfinite(v)) or (nonzero and not any(v)):
        raise ValueError(f"{what} wants x,y,z, not {spec!r}")
    return tuple(v)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.terms", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--json", action="store_true", help="print the totals as one JSON line")
    ap.add_argument("--rings", nargs=3, metavar=("RMIN", "RMAX", "N"), default=None, help="ring tables over N rings")
    ap.add_argument("--log", action="store_true", help="logarithmic ring edges")
    ap.add_argument("--centre", default="0,0,0", help="x,y,z")
    ap.add_argument("--normal", default="0,0,1", help="x,y,z")
    ap.add_argument("--no-gravity", action="store_true", help="skip the tree walk: rows 9-11 are NaN")
    ap.add_argument("--self-gravity", action="store_true", help="a context with FLAG_SELF_GRAVITY")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        a.centre = _vec3(a.centre, "--centre")
        a.normal = _vec3(a.normal, "--normal", nonzero=True)
        a.edges = None
        if a.rings is not None:
            n_r = int(a.rings[2])
            a.edges = ring_edges(float(a.rings[0]), float(a.rings[1]), n_r, a.log)
        elif a.log:
            raise ValueError("--log without --rings")
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import capi
    from .cli import read_save, uploaded_context
    gas, sinks = read_save(a.save, a.variable)
    names = "x y z vx vy vz u m alpha".split() + (["h"] if a.variable else [])
    state = {k: np.ascontiguousarray(gas[:, i]) for i, k in enumerate(names)}
    flags = (capi.FLAG_VARIABLE_H if a.variable else 0) | (capi.FLAG_SELF_GRAVITY if a.self_gravity else 0)
    with uploaded_context(gas, sinks, a.variable, a.device, flags=flags) as ctx:
        rows = ctx.force_terms(skip_gas_gravity=a.no_gravity, refresh=True)
    tot = totals(state, rows, a.centre)
    out = {"rows": rows, "row_names": np.array(capi.TERM_ROWS), "terms": np.array(TERMS), **tot}
    if a.edges is not None:
        out["edges"] = a.edges
        out["ring_torques"] = ring_torques(state, rows, a.edges, a.centre, a.normal)
        out["ring_heating"] = ring_heating(state, rows, a.edges, a.centre, a.normal)
    np.savez(a.out, **out)
    if a.json:
        print(json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in tot.items()}))
    else:
        print(f"{a.out}: {rows.shape[1]} gas rows ({sinks.shape[0]} sinks), sum m du_P {tot['du_P']:.6e}, sum m du_V {tot['du_V']:.6e}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
