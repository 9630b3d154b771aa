"""What the command-line tools (python -m summersph_amd.profile, .groups, .sample, ...) share: the strict save-file reader,
the argument parsers, the upload of a save file's rows into a fresh context and the descriptor dump of the .npz outputs.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

STATE = "x y z vx vy vz u m alpha".split()


def read_save(path: str, variable: bool = False):
    """(gas rows (n, 9 or 10), sink rows (ns, 8)): records of 9 (10 with variable) values are gas, of 8 sinks"""
    ng = 10 if variable else 9
    gas, sinks = [], []
    with open(path) as f:
        f.readline()
        for line in f:
            tok = line.split()
            if len(tok) == ng:
                gas.append([float(t.replace("D", "E")) for t in tok])
            elif len(tok) == 8:
                sinks.append([float(t.replace("D", "E")) for t in tok])
            elif tok:
                raise ValueError(f"{path}: a record of {len(tok)} values")
    return np.asarray(gas, dtype=np.float64).reshape(-1, ng), np.asarray(sinks, dtype=np.float64).reshape(-1, 8)


def parse_clip(spec: str):
    """'x0,y0,z0,x1,y1,z1' -> ((x0, y0, z0), (x1, y1, z1)), no NaN and lo <= hi on every axis"""
    v = [float(t) for t in spec.split(",")]
    if len(v) != 6 or any(np.isnan(v)) or any(v[a] > v[3 + a] for a in range(3)):
        raise ValueError(f"--clip wants x0,y0,z0,x1,y1,z1 with x0 <= x1 ..., not {spec!r}")
    return tuple(v[:3]), tuple(v[3:])


def parse_vec(spec: str, what: str = "a vector"):
    """'x,y,z' -> (x, y, z), three finite numbers; what names the option in the error"""
    v = [float(t) for t in spec.split(",")]
    if len(v) != 3 or not all(math.isfinite(t) for t in v):
        raise ValueError(f"{what} wants three finite numbers x,y,z, not {spec!r}")
    return tuple(v)


def parse_fields(spec: str, lo: int, hi: int, variable: bool = False, blanks: bool = False):
    """'rho,u,vy' -> ['rho', 'u', 'vy']: lo .. hi field names of capi.FIELDS (h and omega only with variable h).  Empty
    names ('rho,,u', a trailing comma, '') are dropped, or with blanks=True kept and refused as unknown names."""
    from . import capi
    names = spec.split(",") if blanks else [t for t in spec.split(",") if t]
    allowed = [f for f in capi.FIELDS if variable or f not in ("h", "omega")]
    if not lo <= len(names) <= hi or any(f not in allowed for f in names):
        count = "three" if (lo, hi) == (3, 3) else f"{lo} .. {hi}"
        raise ValueError(f"--fields wants {count} comma-separated names of {allowed}, not {spec!r}")
    return names


@contextlib.contextmanager
def uploaded_context(gas, sinks, variable=False, device=0, **overrides):
    """A fresh context holding a save file's rows: the gas columns uploaded (h too with variable) and, if there are any,
    the sinks set from the sink rows' columns x y z vx vy vz . m.  overrides: Params fields (flags, theta, ...).  Closed
    on the way out, whatever happens."""
    from . import capi
    ctx = capi.Context(device=device, variable=variable, **overrides)
    try:
        ctx.upload({k: gas[:, i] for i, k in enumerate(STATE + (["h"] if variable else []))})
        if sinks.shape[0]:
            ctx.set_sinks({k: sinks[:, i] for i, k in zip((0, 1, 2, 3, 4, 5, 7), "x y z vx vy vz m".split())})
        yield ctx
    finally:
        ctx.close()


def desc_arrays(d) -> dict:
    """the fields of a descriptor (a ctypes Structure) as the `desc_*` entries of an .npz output"""
    out = {}
    for f, _ in d._fields_:
        v = getattr(d, f)
        out["desc_" + f] = np.array(v[:] if hasattr(v, "__len__") else v)
    return out
