"""A numpy restatement of one sph_history row (include/summersph.h, "Row"): built from a downloaded state and the sinks.

The gas terms are sph_energy's, with separate multiplies and adds (numpy does not contract).  An exact sum follows the
header's rules to the letter: e = frexp(max |term|)[1], every term rounded half-even to a multiple of 2^(e - 62)
(np.rint(np.ldexp(term, 62 - e))), a Python-int sum, and one conversion back (float(int) rounds half-even once, ldexp is
exact)."""
import math

import numpy as np

NHEAD = 40
EXACT = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14]         # sph_energy's sums that a row holds exactly
G_DEFAULT = float(np.float32(39.47841760435743))


def phi_sink(gas, sinks, G):
    """Phi_sink of every gas particle: -sum_s (G M_s) / |r - R_s| in sink order, massless sinks add 0"""
    x, y, z = (np.asarray(gas[k], dtype=np.float64) for k in "xyz")
    ps = np.zeros(x.shape)
    ns = 0 if sinks is None else len(sinks["m"])
    for s in range(ns):
        sm = float(sinks["m"][s])
        if sm == 0.0:
            continue
        dx, dy, dz = x - sinks["x"][s], y - sinks["y"][s], z - sinks["z"][s]
        with np.errstate(divide="ignore", invalid="ignore"):
            ps = ps - (G * sm) / np.sqrt((dx * dx + dy * dy) + dz * dz)
    return ps


def gas_terms(gas, sinks=None, G=G_DEFAULT):
    """{sum index: the per-particle terms} of the 13 exact sums"""
    x, y, z, vx, vy, vz, u, m = (np.asarray(gas[k], dtype=np.float64) for k in "x y z vx vy vz u m".split())
    with np.errstate(over="ignore", invalid="ignore"):
        return {1: m.copy(), 2: m * x, 3: m * y, 4: m * z, 5: m * vx, 6: m * vy, 7: m * vz,
                8: m * (y * vz - z * vy), 9: m * (z * vx - x * vz), 10: m * (x * vy - y * vx),
                11: (0.5 * m) * ((vx * vx + vy * vy) + vz * vz), 12: m * u, 14: m * phi_sink(gas, sinks, G)}


def exponent(terms):
    """e with max |term| < 2^e (0 for no term or a zero maximum)"""
    b = float(np.max(np.abs(terms))) if terms.size else 0.0
    return math.frexp(b)[1]


def exact_sum(terms):
    """the header's exact sum of the terms: NaN with a non-finite term"""
    t = np.asarray(terms, dtype=np.float64)
    if not np.all(np.isfinite(t)):
        return float("nan")
    e = exponent(t)
    ints = np.rint(np.ldexp(t, 62 - e))                  # |.| <= 2^62: exactly representable integers
    total = sum(ints.astype(np.int64).tolist())          # Python ints: no overflow, any order
    return math.ldexp(float(total), e - 62)


def sink_sums(sinks, G=G_DEFAULT):
    """sph_energy's sink part sums[15..28) in plain fp64, each sink's terms in the header's order (the device adds them
    in a butterfly, so only sets of one or two sinks compare bitwise)"""
    out = np.zeros(13)
    ns = 0 if sinks is None else len(sinks["m"])
    for s in range(ns):
        x, y, z, vx, vy, vz, m = (float(sinks[k][s]) for k in "x y z vx vy vz m".split())
        w = 0.0
        for t in range(s + 1, ns):
            mm = m * float(sinks["m"][t])
            if mm == 0.0:
                continue
            dx, dy, dz = x - sinks["x"][t], y - sinks["y"][t], z - sinks["z"][t]
            w = w - (G * mm) / math.sqrt((dx * dx + dy * dy) + dz * dz)
        out += np.array([1.0, m, m * x, m * y, m * z, m * vx, m * vy, m * vz, m * (y * vz - z * vy), m * (z * vx - x * vz),
                         m * (x * vy - y * vx), (0.5 * m) * ((vx * vx + vy * vy) + vz * vz), w])
    return out


def row(gas, sinks=None, rho=None, step=0, dt_words=(0.0, 0.0, 0.0), max_sinks=0, G=G_DEFAULT, sink_part=None):
    """The row of a state: gas a dict of x .. m in the download order, sinks a dict of x .. m or None, rho the downloaded
    density or None (not current), dt_words (t, next dt, candidate), sink_part sph_energy's sums[15:] where the caller has
    them (else sink_sums)."""
    n = len(gas["x"])
    ns = 0 if sinks is None else len(sinks["m"])
    r = np.full(NHEAD + 7 * max_sinks, np.nan)
    r[0] = step
    r[1:4] = dt_words
    r[4], r[5], r[6] = n, ns, n
    for k, t in gas_terms(gas, sinks, G).items():
        r[6 + k] = exact_sum(t)
    r[6 + 13] = 0.0
    r[21:34] = sink_sums(sinks, G) if sink_part is None else sink_part
    if rho is not None and n > 0 and not np.all(np.isnan(rho)):
        i = int(np.nanargmax(rho))                       # the first of the maxima
        r[34], r[35] = rho[i], i
        r[36:39] = gas["x"][i], gas["y"][i], gas["z"][i]
    vx, vy, vz = (np.asarray(gas[k], dtype=np.float64) for k in ("vx", "vy", "vz"))
    with np.errstate(over="ignore", invalid="ignore"):
        v2 = (vx * vx + vy * vy) + vz * vz
    r[39] = math.sqrt(float(np.max(v2))) if n > 0 else 0.0       # np.max propagates NaN
    for s in range(min(ns, max_sinks)):
        r[NHEAD + 7 * s:NHEAD + 7 * s + 7] = [float(sinks[k][s]) for k in "x y z vx vy vz m".split()]
    return r
