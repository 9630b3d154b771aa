"""The fixed-h step's fused bookkeeping launches give the bits of the separate ones.

What sph_run / sph_step fuse on the plain fixed-h path (csrc/grid.hip): the opening kick + drift leaves the cell keys, the
histogram and the bounding-box partials of the next grid build behind (SPH_NO_DRIFT_KEYS switches it off), the box's final
reduction rides on cell_scatter as one more workgroup (SPH_NO_BOX_RIDE), the rank within the cell is taken inside the reorder
(SPH_NO_RANK_REORDER), and a context of one rank without ghosts no longer stores inv at every reorder but rebuilds it when
somebody asks (SPH_NO_LAZY_INV).  Minimum, maximum and integer counts do
not depend on the order, so every result must be IDENTICAL, and so must the number of host waits.

The switches are read once per process, so each side of a comparison is a fresh child process of its own (this file, run as
a script), one after the other, each under its own time limit; a child that fails ends the module.  Every child runs the
same scenarios on a 20 000-particle disc and saves what it saw:
  run      sph_run(6): state, rho, accelerations, du, sinks, dt, t; then the consumers of inv -- fields in the caller's
           order, sph_gather_fields_dev with ids, sph_energy
  calls    the same six steps through sph_density / sph_forces / sph_kick / sph_drift / sph_next_dt
  upload / scatter / owned     sph_run(3), positions overwritten (sph_upload_field, sph_scatter_fields_dev) or
           sph_set_owned, sph_run(3): the early keys must not survive what changes the particle set under them
  variable, hashed, gravacc, halo2    contexts the fusion does not cover: variable h, SPH_FLAG_HASHED_GRID, self-gravity +
           accretion, two in-process ranks of the native halo loop
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("SPH_NO_DRIFT_KEYS", "SPH_NO_BOX_RIDE", "SPH_NO_RANK_REORDER", "SPH_NO_LAZY_INV")
STATE = "x y z vx vy vz u alpha".split()
DERIVED = "rho ax ay az du".split()
N = 20000


def _record(out, tag, ctx, dt, t, derived=True):
    for f in STATE + (DERIVED if derived else []):
        out[f"{tag}/{f}"] = ctx.field(f)
    s = ctx.get_sinks()
    for k in "x y z vx vy vz m ax ay az".split():
        out[f"{tag}/sink_{k}"] = s[k]
    st = ctx.stats()
    out[f"{tag}/dt_t"] = np.array([dt, t])
    out[f"{tag}/counts"] = np.array([ctx.n, st.host_syncs, st.grid_builds, st.nlist_builds])


def _scenarios(out):
    import threading

    import torch
    from summersph_amd import capi, halo, ic
    from summersph_amd.dist import slab_bounds

    gas, sinks = ic.split_rows(ic.keplerian_disc(N, seed=41))

    def make(g=gas, s=sinks, **kw):
        ctx = capi.Context(device=0, **kw)
        ctx.upload(g)
        ctx.set_sinks(s)
        return ctx

    # ---- run: six fused steps, then everything that reads inv ---------------------------------------------------
    ctx = make()
    dt, t = ctx.run(2, 1e-2, 0.0)
    syncs = ctx.stats().host_syncs
    dt, t = ctx.run(4, dt, t)
    out["run/steady_syncs"] = np.array([ctx.stats().host_syncs - syncs])
    _record(out, "run", ctx, dt, t)
    ids = torch.from_numpy(np.random.default_rng(5).permutation(N)[:5000].astype(np.int64)).cuda()
    got = torch.empty((3, ids.numel()), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.gather_fields_dev(["x", "vy", "rho"], ids.numel(), ids.data_ptr(), got.data_ptr())
    ctx.synchronize()
    out["run/gathered"] = got.cpu().numpy()
    out["run/gathered_ids"] = ids.cpu().numpy()
    e = ctx.energy(phi=True)
    out["run/energy_sums"] = np.asarray(e["sums"])
    out["run/energy_phi"] = e["phi"]
    ctx.close()

    # ---- calls: the same six steps through the single public calls ----------------------------------------------
    ctx = make()
    dt, t = 1e-2, 0.0
    for _ in range(6):
        ctx.density(); ctx.forces(); ctx.kick(dt); ctx.drift(dt); ctx.density(); ctx.forces(); ctx.kick(dt)
        t += dt
        dt = ctx.next_dt(dt)
    _record(out, "calls", ctx, dt, t)
    ctx.close()

    # ---- the record of "keys exist" is dropped when it must be --------------------------------------------------
    for tag in ("upload", "scatter", "owned"):
        ctx = make()
        dt, t = ctx.run(3, 1e-2, 0.0)
        if tag == "upload":
            ctx.upload_field("x", ctx.field("x") * (1.0 + 1e-3))
        elif tag == "scatter":
            pos = torch.from_numpy(np.stack([ctx.field("x") * 1.5, ctx.field("y") + 0.25, ctx.field("z")])).cuda()
            torch.cuda.synchronize()
            ctx.scatter_fields_dev(["x", "y", "z"], 0, N, pos.data_ptr())
            ctx.synchronize()
        else:
            ctx.set_owned(N)
        dt, t = ctx.run(3, dt, t)
        _record(out, tag, ctx, dt, t)
        ctx.close()

    # ---- contexts the fusion does not cover ---------------------------------------------------------------------
    vgas, vsinks = ic.split_rows(ic.keplerian_disc_var(N, seed=43))
    ggas, gsinks = ic.split_rows(ic.keplerian_disc(N, seed=44, m_disc=0.5))
    for tag, g, s, kw in (("variable", vgas, vsinks, {"variable": True}),
                          ("hashed", gas, sinks, {"flags": capi.FLAG_HASHED_GRID}),
                          ("gravacc", ggas, gsinks, {"flags": capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL})):
        ctx = make(g, s, **kw)
        dt, t = ctx.run(2, 1e-2, 0.0)
        syncs = ctx.stats().host_syncs
        dt, t = ctx.run(3, dt, t)
        out[f"{tag}/steady_syncs"] = np.array([ctx.stats().host_syncs - syncs])
        _record(out, tag, ctx, dt, t, derived=False)
        ctx.close()

    world = 2
    hub = halo.Hub(world)
    bounds = slab_bounds(gas["x"], world)
    owner = np.searchsorted(bounds, gas["x"], side="right")
    errs = []

    def worker(rank):
        try:
            ctx = capi.Context(device=0)
            h = halo.Halo.inproc(ctx, hub, rank, world)
            sel = owner == rank
            mine = {k: v[sel] for k, v in gas.items()}
            mine["gid"] = np.nonzero(sel)[0]
            ctx.set_sinks(sinks)
            h.set_slabs(bounds, 2)
            h.upload(mine)
            dt, t = 1e-2, 0.0
            for _ in range(4):
                dt, t = h.run(1, dt, t)
            state = h.download()
            for f in STATE + ["gid"]:
                out[f"halo2/r{rank}_{f}"] = np.asarray(state[f])
            out[f"halo2/r{rank}_dt_t"] = np.array([dt, t])
            out[f"halo2/r{rank}_syncs"] = np.array([ctx.stats().host_syncs])
            h.close(); ctx.close()
        except Exception as e:      # noqa: BLE001 -- reported below
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    hub.close()
    assert not errs, errs


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = {}
    _scenarios(result)
    np.savez(sys.argv[1], **result)
    sys.exit(0)


import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    """fused: no switch set; unfused: every switch set.  One child after the other; the first failure ends the module."""
    d = tmp_path_factory.mktemp("step_fusion")
    res = {}
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for side, env in (("fused", base), ("unfused", {**base, **{k: "1" for k in SWITCHES}})):
        path = str(d / f"{side}.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=600, cwd=ROOT)
        res[side] = dict(np.load(path))
    return res


def _same(a, b, keys):
    assert keys, "nothing to compare"
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _tag(side, tag):
    return sorted(k for k in side if k.startswith(tag + "/"))


def test_fused_run_equals_unfused_run(sides):
    assert _tag(sides["fused"], "run") == _tag(sides["unfused"], "run")
    _same(sides["fused"], sides["unfused"], [k for k in _tag(sides["fused"], "run")
                                            if not k.startswith(("run/gathered", "run/energy"))])
    assert sides["fused"]["run/steady_syncs"][0] == 0


@pytest.mark.parametrize("side", ["fused", "unfused"])
def test_run_equals_the_single_public_calls(sides, side):
    s = sides[side]
    for f in STATE + DERIVED + ["dt_t"] + ["sink_" + k for k in "x y z vx vy vz m ax ay az".split()]:
        assert np.array_equal(s["run/" + f], s["calls/" + f]), f


@pytest.mark.parametrize("tag", ["upload", "scatter", "owned"])
def test_early_keys_are_dropped_when_positions_or_the_particle_set_change(sides, tag):
    _same(sides["fused"], sides["unfused"], _tag(sides["fused"], tag))
    if tag != "owned":       # the overwritten positions did change the run
        assert not np.array_equal(sides["fused"][tag + "/x"], sides["fused"]["run/x"])


def test_inv_on_demand(sides):
    f, u = sides["fused"], sides["unfused"]
    _same(f, u, ["run/gathered", "run/gathered_ids", "run/energy_sums", "run/energy_phi"])
    ids = f["run/gathered_ids"]
    for row, name in enumerate(("x", "vy", "rho")):      # ... and they are the caller-order fields at those ids
        assert np.array_equal(f["run/gathered"][row], f["run/" + name][ids]), name


@pytest.mark.parametrize("tag", ["variable", "hashed", "gravacc", "halo2"])
def test_other_contexts_take_the_old_launches(sides, tag):
    assert _tag(sides["fused"], tag) == _tag(sides["unfused"], tag)
    _same(sides["fused"], sides["unfused"], _tag(sides["fused"], tag))
