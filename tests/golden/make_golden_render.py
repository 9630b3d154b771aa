#!/usr/bin/env python3
"""Generates render_script12k.npz from the REAL reference imaging script.

Runs only in the build container, where the reference tree exists.  It writes a 12 000-particle
`ic.keplerian_disc(12000, seed=214)` (last row: the central sink) as a save file in make_save's
layout and executes the unmodified Density_Image.py on it, in place, with three shims that touch
nothing inside the script:
  - a stub `numba` module whose `jit` is the identity (numba is not installed here);
  - the script's hard-coded `/content/save275.txt` redirected to the generated file (the name
    `open` is pre-set in the script's globals);
  - `plt.show` made a no-op (Agg backend).
The script runs 1.7 M KD-tree ball queries: expect minutes.

    python tests/golden/make_golden_render.py [REFERENCE_DIR]

Stored (float64, no pickles): the save file's gas rows (9 columns) and sink rows (8), the script's
`projected_density` (120 x 120, x slowest), its bounds xmin..zmax, h and the grid resolution, and
the script's own wall time (`script_seconds`) and the particle arrays it rendered after its clip and its
drop of the last surviving gas row (`script_x`, `script_y`, `script_z`, `script_mass`, the dropped row's `script_*_sun`).
"""
import builtins
import os
import runpy
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from summersph_amd import ic, txtio  # noqa: E402

SCRIPT_PATH = "/content/save275.txt"


def fixture_rows():
    rows = ic.keplerian_disc(12000, seed=214)
    gas8, sinks = ic.split_rows(rows)
    gas = np.column_stack([gas8[k] for k in "x y z vx vy vz u m".split()] + [np.zeros(gas8["x"].size)])
    sk = np.column_stack([sinks[k] for k in "x y z vx vy vz".split()] + [np.zeros(sinks["x"].size), sinks["m"]])
    return gas, sk


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.sep, "root", "reference")
    script = os.path.join(ref, "Density_Image.py")
    gas, sinks = fixture_rows()
    with tempfile.TemporaryDirectory() as td:
        save = os.path.join(td, "save275.txt")
        txtio.write_save(save, gas, sinks)

        numba = types.ModuleType("numba")
        numba.jit = lambda f=None, **kw: f if f is not None else (lambda g: g)
        sys.modules["numba"] = numba
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        plt.show = lambda *a, **k: None

        def redirected_open(path, *a, **k):
            return builtins.open(save if path == SCRIPT_PATH else path, *a, **k)

        t0 = time.perf_counter()
        g = runpy.run_path(script, init_globals={"open": redirected_open}, run_name="__main__")
        secs = time.perf_counter() - t0
        plt.close("all")
    out = dict(gas=gas, sinks=sinks, projected_density=np.asarray(g["projected_density"], dtype=np.float64),
               bounds=np.array([g["xmin"], g["ymin"], g["zmin"], g["xmax"], g["ymax"], g["zmax"]], dtype=np.float64),
               h=np.float64(g["h"]), grid_resolution=np.int64(g["grid_resolution"]), script_seconds=np.float64(secs),
               **{"script_" + k: np.asarray(g[k], dtype=np.float64) for k in ("x", "y", "z", "mass", "x_sun", "y_sun", "z_sun")})
    np.savez_compressed(os.path.join(HERE, "render_script12k.npz"), **out)
    print("render_script12k.npz:", out["projected_density"].shape, "max", out["projected_density"].max(), f"{secs:.1f} s")


if __name__ == "__main__":
    main()
