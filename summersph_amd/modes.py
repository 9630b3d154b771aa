"""Spiral modes of a save file on the GPU: the azimuthal Fourier amplitudes A_m(R) of a disc's surface density per ring and
the logarithmic-spiral spectrum A(m, p) of the annulus, whose peak gives the arm number m and the pitch angle tan i = m / p.

    python -m summersph_amd.modes SAVE.txt -o OUT.npz --rings RMIN RMAX N [--log] [--mmax M] [--spiral PMIN PMAX NP]
                                  [--rref R] [--sink K | --centre x,y,z] [--normal x,y,z] [--zmax Z] [--weight one|mass]
                                  [--q FIELD] [--variable] [--json]

SAVE.txt is a save file as summersph_amd.profile reads it (9-value gas records, 10 with --variable, 8-value sink records).
The gas and the sinks are uploaded into a fresh context and sph_modes (capi.Context.modes) sums w cos m phi and w sin m phi
over the owned gas of every ring and, with --spiral, w cos / sin (m phi + p ln(R / r_ref)) over the annulus.  Every sum is
exact, so the numbers do not depend on how the particles are ordered or split over ranks.

OUT.npz holds `ring` (n_r, m_max + 1, 2: C, S), `spiral` (m_max + 1, n_p, 2: CS, SN; with --spiral), `raw_ring`, `raw_spiral`
and `exp` (the exact 128-bit sums, which add across ranks and pieces: add_raw, then capi.modes_finish), `edges`, `p`,
`ring_counts`, `counts` (selected, outside, not usable, at the centre) and what finish() returns (`A`, `phase`, and with
--spiral `spectrum`, `p_peak`, `pitch`).  --json prints a one-line summary.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from .pairs import add_raw   # the exact sum of two raw results of equal exponent (ranks, clip pieces): {low, high} limbs

__all__ = ["finish", "add_raw", "parse_args", "main"]

RATES = ("ax", "ay", "az", "du", "dalpha")
DERIVED = ("rho", "P", "c", "omega")


def finish(ring, spiral=None, p=None):
    """The amplitudes and phases of raw mode sums as a dict.  ring (n_r, m_max + 1, 2) = (C, S): A[k, m] = sqrt(C^2 + S^2) /
    C[k, 0] and phase[k, m] = atan2(S, C) / m.  With spiral (m_max + 1, n_p, 2) = (CS, SN) and the p table: spectrum[m, l] =
    sqrt(CS^2 + SN^2) / W with W = CS[0, l0] where p[l0] == 0, else the sum of the rings' C[k, 0]; per m the peak's
    wavenumber p_peak[m] and the pitch angle pitch[m] = atan(m / p_peak[m]).  NaN wherever a denominator is 0."""
    r = np.asarray(ring, dtype=np.float64)
    if r.ndim != 3 or r.shape[2] != 2:
        raise ValueError("finish: ring sums are (n_r, m_max + 1, 2)")
    m = np.arange(r.shape[1], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c0 = np.where(r[:, :1, 0] == 0.0, np.nan, r[:, :1, 0])
        out = {"A": np.hypot(r[..., 0], r[..., 1]) / c0,
               "phase": np.arctan2(r[..., 1], r[..., 0]) / np.where(m == 0.0, np.nan, m)[None, :]}
        if spiral is None:
            return out
        s = np.asarray(spiral, dtype=np.float64)
        if s.ndim != 3 or s.shape[0] != r.shape[1] or s.shape[2] != 2:
            raise ValueError("finish: spiral sums are (m_max + 1, n_p, 2)")
        if p is None or np.shape(p) != (s.shape[1],):
            raise ValueError("finish: the spiral sums want their p table (n_p,)")
        p = np.asarray(p, dtype=np.float64)
        zero = np.flatnonzero(p == 0.0)
        W = float(s[0, zero[0], 0]) if zero.size else float(np.sum(r[:, 0, 0]))
        amp = np.hypot(s[..., 0], s[..., 1]) / (np.nan if W == 0.0 else W)
        peak = p[np.argmax(np.nan_to_num(amp, nan=-np.inf), axis=1)]
        out.update({"spectrum": amp, "p_peak": peak, "pitch": np.arctan(m / np.where(peak == 0.0, np.nan, peak))})
    return out


def parse_args(argv=None):
    from .capi import FIELDS, MODES_MAX_M, MODES_MAX_P, MODES_MAX_RINGS, MODES_WEIGHTS
    from .cli import parse_vec
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.modes", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz")
    ap.add_argument("--rings", nargs=3, required=True, metavar=("RMIN", "RMAX", "N"), help="ring range and count")
    ap.add_argument("--log", action="store_true", help="logarithmic rings (RMIN > 0)")
    ap.add_argument("--mmax", type=int, default=MODES_MAX_M, help=f"highest m, 0 .. {MODES_MAX_M}")
    ap.add_argument("--spiral", nargs=3, default=None, metavar=("PMIN", "PMAX", "NP"), help="the spiral sums' wavenumbers")
    ap.add_argument("--rref", type=float, default=1.0, help="reference radius of ln(R / r_ref)")
    ap.add_argument("--sink", type=int, default=None, help="centre the frame on this sink")
    ap.add_argument("--centre", default=None, help="x,y,z: the frame's origin (default 0,0,0)")
    ap.add_argument("--normal", default="0,0,1", help="x,y,z: the disc normal")
    ap.add_argument("--zmax", type=float, default=np.inf, help="keep |z'| < ZMAX")
    ap.add_argument("--weight", default="mass", help="one or mass")
    ap.add_argument("--q", default=None, help="a field the weight is multiplied by")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--json", action="store_true", help="print a one-line JSON summary")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        a.r_range = (float(a.rings[0]), float(a.rings[1]))
        a.n_r = int(a.rings[2])
        if not np.all(np.isfinite(a.r_range)) or not 0.0 <= a.r_range[0] < a.r_range[1] or (a.log and a.r_range[0] <= 0.0):
            raise ValueError("--rings wants finite 0 <= RMIN < RMAX (RMIN > 0 with --log)")
        if not 1 <= a.n_r <= MODES_MAX_RINGS:
            raise ValueError(f"--rings wants 1 .. {MODES_MAX_RINGS} rings")
        if not 0 <= a.mmax <= MODES_MAX_M:
            raise ValueError(f"--mmax wants 0 .. {MODES_MAX_M}")
        if a.spiral is not None:
            a.spiral = (float(a.spiral[0]), float(a.spiral[1]), int(a.spiral[2]))
            if not np.all(np.isfinite(a.spiral[:2])) or a.spiral[0] > a.spiral[1] or not 1 <= a.spiral[2] <= MODES_MAX_P:
                raise ValueError(f"--spiral wants finite PMIN <= PMAX and 1 .. {MODES_MAX_P} wavenumbers")
            if not (np.isfinite(a.rref) and a.rref > 0.0):
                raise ValueError("--rref wants a finite radius > 0")
        if a.sink is not None and (a.centre is not None or a.sink < 0):
            raise ValueError("--sink wants an index >= 0 and no --centre")
        a.centre = None if a.centre is None else parse_vec(a.centre, "--centre")
        a.normal = parse_vec(a.normal, "--normal")
        if not any(a.normal):
            raise ValueError("--normal is zero")
        if np.isnan(a.zmax):
            raise ValueError("--zmax is NaN")
        if a.weight not in MODES_WEIGHTS:
            raise ValueError(f"--weight wants one of {' '.join(MODES_WEIGHTS)}")
        if a.q is not None:
            if a.q not in FIELDS:
                raise ValueError(f"unknown field {a.q!r} (one of {' '.join(FIELDS)})")
            if a.q in ("h", "omega") and not a.variable:
                raise ValueError(f"field {a.q!r} needs --variable")
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import capi
    from .cli import desc_arrays, read_save, uploaded_context
    gas, sinks = read_save(a.save, a.variable)
    with uploaded_context(gas, sinks, a.variable, a.device) as ctx:
        if a.q in DERIVED or a.q in RATES:
            ctx.density()
        if a.q in RATES:
            ctx.forces()
        ring, spiral, ring_counts, counts, exp, raw = ctx.modes(a.r_range, a.n_r, a.mmax, log=a.log, z_max=a.zmax, centre=a.centre,
                                                                sink=a.sink, normal=a.normal, weight=a.weight, q=a.q,
                                                                spiral=a.spiral, r_ref=a.rref, raw=True)
        d = ctx.modes_desc
    edges, p = capi.modes_tables(d)
    out = {"ring": ring, "raw_ring": raw[0], "exp": np.int32(exp), "edges": edges, "p": p, "ring_counts": ring_counts,
           "counts": np.array(counts)}
    if spiral is not None:
        out.update({"spiral": spiral, "raw_spiral": raw[1]})
    f = finish(ring, spiral, p if spiral is not None else None)
    out.update(f)
    out.update(desc_arrays(d))
    np.savez(a.out, **out)
    summary = {"gas": int(gas.shape[0]), "sinks": int(sinks.shape[0]), "rings": a.n_r, "r": list(a.r_range), "log": a.log,
               "m_max": a.mmax, "selected": counts[0], "outside": counts[1], "not_usable": counts[2], "at_centre": counts[3],
               "exp": int(exp)}
    if spiral is not None:
        top = np.max(np.nan_to_num(f["spectrum"], nan=-np.inf), axis=1)            # per m; the strongest m >= 1
        m_best = int(np.argmax(np.where(np.arange(a.mmax + 1) > 0, top, -np.inf))) if a.mmax else 0
        summary.update({"n_p": a.spiral[2], "m_peak": m_best, "p_peak": float(f["p_peak"][m_best]),
                        "amplitude": float(top[m_best]), "pitch": float(f["pitch"][m_best])})
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: {a.n_r} rings in [{a.r_range[0]}, {a.r_range[1]}), m <= {a.mmax}, {counts[0]} of {gas.shape[0]} gas rows")
    return 0


if __name__ == "__main__":
    sys.exit(main())
