"""The particle sets of the sph_force_terms tests (tests/test_force_terms_cpu.py asserts what each is built to have,
tests/test_force_terms_gpu.py runs them), each with its restatement (tests/force_terms_ref.py), computed once per process.

Fixed h (h = 2.5): the 3000-particle disc fixture with its sink and with a second sink, the Sod column fixture, patches of
n = 1, 2, 63, 64, 65 mutual neighbours of the disc, a patch with a coincident pair, a patch with a pair at r = 2 h (1 - 1e-9),
a patch plus one isolated particle (its rows are sink gravity only), and varh_sets.far_clump_fixed(2800, 160) less the
rim particles without a neighbour: the smallest arguments whose lists (up to ~159 entries in the clump) outgrow the
context's initial 96 slots.  The fixtures' gas gets a seeded alpha and velocity perturbation.

Variable h: the discv3000 fixture (with its sink) and varh_sets.build(name, small=True) for clump_in_halo, edge_pairs_v (it
holds a coincident pair: the restatement's "kernel" mode) and h_routes (no sinks)."""
from __future__ import annotations

import numpy as np

import force_terms_ref as FR
import varh_ref as VR
import varh_sets as S
from conftest import load_golden

H = FR.H_FIXED
FIXED = ["disc1", "disc2", "sod1000", "n1", "n2", "n63", "n64", "n65", "coincident", "inside_2h", "isolated", "far_clump_fixed"]
VARIABLE = ["discv3000", "clump_in_halo", "edge_pairs_v", "h_routes"]
HAS_COINCIDENT = {"coincident", "edge_pairs_v"}
HAS_EMPTY_LIST = {"n1": 1, "isolated": 1}          # sets with exactly this many particles without a neighbour, on purpose
INIT_LIST_SLOTS = 96                               # a context's first neighbour list (csrc/api.hip)
_CACHE = {}


def _take(gas, idx):
    return {k: np.ascontiguousarray(np.asarray(v)[idx]) for k, v in gas.items()}


def _disc():
    from summersph_amd import ic
    gas, sinks = ic.split_rows(load_golden("disc3000_eval")["ic"])
    # the fixture's gas is at rest relative to circular motion and has alpha = 0 (the reader's start value): give it a live
    # alpha and a seeded velocity perturbation, so that the viscosity is on and pairs approach and recede
    rng = np.random.default_rng(4242)
    n = gas["x"].size
    gas = {k: np.array(v, dtype=np.float64) for k, v in gas.items()}
    gas["alpha"] = rng.uniform(0.05, 1.0, n)
    for k in ("vx", "vy", "vz"):
        gas[k] = gas[k] + rng.normal(0.0, 0.02, n)
    return gas, sinks


def _patch(n, seed_particle=1500):
    """the n particles of the disc nearest to one of them (mutual neighbours while n is small), and the disc's sink"""
    gas, sinks = _disc()
    d = np.sqrt((gas["x"] - gas["x"][seed_particle]) ** 2 + (gas["y"] - gas["y"][seed_particle]) ** 2
                + (gas["z"] - gas["z"][seed_particle]) ** 2)
    return _take(gas, np.sort(np.argsort(d, kind="stable")[:n])), sinks


def fixed_set(name):
    """(gas, sinks) of a fixed-h set"""
    if name == "disc1":
        return _disc()
    if name == "disc2":
        gas, sinks = _disc()
        two = {k: np.append(np.asarray(v, dtype=np.float64), {"x": 40.0, "y": -25.0, "z": 3.0, "vx": 0.3, "vy": 0.5, "vz": 0.0,
                                                              "m": 0.2}.get(k, 0.0)) for k, v in sinks.items() if k != "radius"}
        return gas, two
    if name == "sod1000":
        from summersph_amd import ic
        gas, sinks = ic.split_rows(load_golden("sod1000_eval")["ic"])
        rng = np.random.default_rng(4243)
        gas = {k: np.array(v, dtype=np.float64) for k, v in gas.items()}
        gas["alpha"] = rng.uniform(0.05, 1.0, gas["x"].size)
        gas["vx"] = gas["vx"] + rng.normal(0.0, 0.05, gas["x"].size)
        return gas, sinks
    if name in ("n1", "n2", "n63", "n64", "n65"):
        gas, sinks = _patch(int(name[1:]))
        if name == "n2":                                      # its one pair approaches: the viscosity is on
            sep = np.array([gas[k][1] - gas[k][0] for k in "xyz"])
            for k, s in zip(("vx", "vy", "vz"), sep / np.linalg.norm(sep)):
                gas[k][1] = gas[k][0] - 0.05 * s
        return gas, sinks
    if name in ("coincident", "inside_2h", "isolated"):
        gas, sinks = _patch(300)
        a, b = 10, 11
        if name == "coincident":
            for k in "xyz":
                gas[k][b] = gas[k][a]
        elif name == "inside_2h":
            # b at x_a + d along x, d = 2 h (1 - 1e-9); x_a = 0 exactly so that the difference and its root are d to the bit
            shift = gas["x"][a]
            gas["x"] = gas["x"] - shift
            gas["x"][a] = 0.0
            gas["x"][b] = 2.0 * H * (1.0 - 1e-9)
            gas["y"][b] = gas["y"][a]; gas["z"][b] = gas["z"][a]
            sinks = dict(sinks); sinks["x"] = np.asarray(sinks["x"], dtype=np.float64) - shift
        else:
            gas["x"][b] += 400.0; gas["y"][b] -= 300.0        # far from everything: no neighbour at all
        return gas, sinks
    if name == "far_clump_fixed":
        gas, sinks, _ = S.far_clump_fixed(n_disc=2800, n_clump=160)
        rng = np.random.default_rng(4244)
        gas = {k: np.array(v, dtype=np.float64) for k, v in gas.items()}
        gas["alpha"] = rng.uniform(0.05, 1.0, gas["x"].size)
        # less the disc particles that have no neighbour (the disc's ragged rim): no list of this set is empty
        pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
        d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
        np.fill_diagonal(d2, np.inf)
        return _take(gas, np.flatnonzero(d2.min(axis=1) <= (2.0 * H) ** 2)), sinks
    raise KeyError(name)


def fixed_case(name):
    """(gas, sinks, TermRef)"""
    if name not in _CACHE:
        gas, sinks = fixed_set(name)
        _CACHE[name] = (gas, sinks, FR.fixed_terms(gas, sinks))
    return _CACHE[name]


def variable_set(name):
    """(gas with h, sinks or None)"""
    if name == "discv3000":
        from summersph_amd import ic
        return ic.split_rows_var(load_golden("discv3000_eval")["ic"])
    return S.build(name, small=True), None


def variable_ref(gas, sinks, coincident):
    ref = VR.VarhRef(gas, coincident=coincident).density()
    return ref, FR.varh_terms(ref, sinks)


def variable_case(name):
    """(gas, sinks or None, VarhRef with density and forces, TermRef)"""
    if name not in _CACHE:
        gas, sinks = variable_set(name)
        ref, terms = variable_ref(gas, sinks, "kernel" if name in HAS_COINCIDENT else "reference")
        _CACHE[name] = (gas, sinks, ref, terms)
    return _CACHE[name]
