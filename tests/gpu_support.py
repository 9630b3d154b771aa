"""What the GPU tests share: the loaded-library fixture, the one context builder, and the few helpers that mean the same in
every file that had them.  Plain functions, imported by name."""
import numpy as np
import pytest

from conftest import load_golden
from summersph_amd import ic


@pytest.fixture(scope="module")
def capi():
    from summersph_amd import capi as m
    m.load()
    return m


def make_context(capi, gas, sinks=None, *, variable=False, flags=0, density=False, n_owned=None, **params):
    """A context on device 0 with the gas uploaded.  flags and params go to capi.Context as they are (flags = 0 is left
    out); the sinks, the owned count and the density pass only where asked for."""
    ctx = capi.Context(device=0, variable=variable, **({"flags": flags} if flags else {}), **params)
    ctx.upload(gas)
    if sinks is not None:
        ctx.set_sinks(sinks)
    if n_owned is not None:
        ctx.set_owned(n_owned)
    if density:
        ctx.density()
    return ctx


# capi.Context(flags=...) replaces the default parameters' flags, it does not add to them.  The two adjustments the tests
# make before they pass flags on:
def with_variable_h(capi, flags, variable):
    """FLAG_VARIABLE_H ORed in for a variable-h context, also where no other flag is asked for"""
    return flags | capi.FLAG_VARIABLE_H if variable else flags


def over_defaults(capi, flags, variable):
    """flags on top of the default parameters' flags; 0 stays 0, which make_context leaves out"""
    return flags | capi.default_params(variable).flags if flags else flags


def golden_gas(name):
    """(gas, sinks) of a fixture's initial conditions"""
    return ic.split_rows(load_golden(name)["ic"])


def var_params(g):
    """the context parameters a variable-h fixture was made with"""
    gamma, eta, tol, maxlen, scale = g["params"]
    return dict(gamma=gamma, gamma_m1=gamma - 1.0, eta=eta, h_tol=tol, h_max_length=maxlen, dt_scale=scale)


def positions(gas):
    """(N, 3) from an upload dict"""
    return np.stack([gas["x"], gas["y"], gas["z"]], axis=1)


def field_positions(ctx):
    """(N, 3) read back from a context"""
    return np.stack([ctx.field("x"), ctx.field("y"), ctx.field("z")], axis=1)


def ref_h(ctx, capi):
    """what a restatement takes for h: the per-particle field of a variable-h context, else the parameter"""
    return ctx.field("h") if ctx.params.flags & capi.FLAG_VARIABLE_H else float(ctx.params.h)


def clumped_disc(n_disc, k, per, seed):
    """a Keplerian disc with k Plummer clumps of `per` members embedded in holes cut for them:
    (gas, sinks, the disc's particle count, the clumps' sizes)"""
    gas, sinks = ic.split_rows(ic.keplerian_disc(n_disc, seed=seed))
    gas = dict(gas)
    rng = np.random.default_rng(seed + 1)
    rmax = float(np.max(np.sqrt(gas["x"] ** 2 + gas["y"] ** 2)))
    centres = []
    for j in range(k):
        ang = 2 * np.pi * j / k
        rc = 15.0 + (rmax - 25.0) * (j + 0.5) / k
        centres.append((rc * np.cos(ang), rc * np.sin(ang), 0.0))
    centres = np.array(centres)
    far = np.ones(gas["x"].size, bool)
    for c in centres:
        far &= (gas["x"] - c[0]) ** 2 + (gas["y"] - c[1]) ** 2 + (gas["z"] - c[2]) ** 2 > 9.0
    gas = {kk: v[far] for kk, v in gas.items()}
    blobs = []
    for c in centres:
        # Plummer (a = 0.2) truncated at 0.8: every member within 1.6 of every other
        u = rng.uniform(0, 0.95, 3 * per)
        rr = 0.2 / np.sqrt(u ** (-2.0 / 3.0) - 1.0)
        rr = rr[rr < 0.8][:per]
        d = rng.normal(size=(rr.size, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        blobs.append(c + d * rr[:, None])
    bl = np.concatenate(blobs)
    nb = len(bl)
    vk = np.sqrt(1.0 / np.hypot(bl[:, 0], bl[:, 1]))
    ph = np.arctan2(bl[:, 1], bl[:, 0])
    add = {"x": bl[:, 0], "y": bl[:, 1], "z": bl[:, 2], "vx": -vk * np.sin(ph) + rng.normal(0, 0.01, nb),
           "vy": vk * np.cos(ph) + rng.normal(0, 0.01, nb), "vz": rng.normal(0, 0.01, nb),
           "u": rng.uniform(0.1, 0.3, nb), "m": np.full(nb, gas["m"][0]), "alpha": np.ones(nb)}
    n0 = gas["x"].size
    gas = {kk: np.concatenate([gas[kk], add[kk]]) for kk in add}
    return gas, sinks, n0, [len(b) for b in blobs]
