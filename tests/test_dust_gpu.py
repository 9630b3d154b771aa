"""GPU tests of the tracer grains (sph_dust): the gas a grain sees is sph_sample's bit for bit, one advance against the numpy
restatement (tests/dust_ref.py) from the device's own previous state, independence of the other grains and of the cell grid,
a run that is bitwise the run without grains, every / record_every and the log's bookkeeping, angular momentum where no gas
is in reach, the fates, and the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gpu_support import capi, golden_gas, make_context, over_defaults, var_params  # noqa: F401  (capi is a fixture)
import dust_ref

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def full(capi):
    return capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL


def grains_of(gas, m, seed, spread=0.05):
    """m grains near randomly chosen gas particles, with their velocities perturbed: (x (m, 3), v (m, 3))"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(gas["x"].size, m, replace=m > gas["x"].size)
    x = np.stack([gas[k][pick] for k in "xyz"], axis=1) + rng.normal(0.0, spread, (m, 3))
    v = np.stack([gas[k][pick] for k in ("vx", "vy", "vz")], axis=1) * (1.0 + rng.normal(0.0, 0.05, (m, 3)))
    return x, v


def set_clock(ctx, dt, t):
    """sph_set_dt, waited for: its copy reads a staging word that the next sph_set_dt would overwrite"""
    ctx.set_dt(dt, t)
    assert ctx.get_dt() == (dt, t)


def rows_of(ctx):
    d = ctx.dust()
    return d["head"], d["body"]


# ---- 1. the gas a grain sees is sph_sample's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variable", [("disc3000_traj", False), ("discv3000_traj", True)])
def test_gas_columns_are_sample_bit_for_bit(capi, name, variable):
    g = load_golden(name)
    gas, sinks = golden_gas(name)
    ctx = make_context(capi, gas, sinks, variable=variable, **(var_params(g) if variable else {}))
    dt, t = ctx.run(1, 1e-2, 0.0)                              # a state the step left, not the upload's
    for m in (1, 63, 64, 65, 1000):
        x, v = grains_of(gas, m, seed=m)
        x[m // 3::3, 2] += 4.0                                 # above the disc: few or no sources in reach
        x[m // 2::5] = x[m // 2::5] * 50.0 + 3.0e3             # far outside the gas box
        ctx.dust_begin(x, v, np.full(m, 0.3), law="fixed_ts", capacity=3)
        ctx.dust_advance()                                     # row 0: the positions as given, in the gas as it is
        for row in (0, 2):
            if row == 2:
                dt, t = ctx.run(2, dt, t)                      # two more rows, at moved positions in a moved gas
            body = ctx.dust(row, 1)["body"][0]
            pts = body[0:3].T.copy()
            assert row != 0 or same_bits(pts, x)
            out, den = ctx.sample(pts, fields=("vx", "vy", "vz", "u"), normalise=True, weight_out=True)
            assert same_bits(body[6], den), (m, row)
            assert same_bits(body[8:11], out[0:3]) and same_bits(body[7], out[3]), (m, row)
            empty = den == 0.0
            assert np.all(body[8:11][:, empty] == 0.0) and np.all(body[11][empty] == 0.0)
            assert np.all(body[11][~empty] == 1.0 / 0.3)
        if m == 1000:
            assert 0 < np.sum(empty) < m                       # both kinds of grain were there
        assert ctx.dust_info()["n_live"] == m
    ctx.dust_end()
    ctx.close()


# ---- 2. and 5. one advance against the restatement, no chaining ---------------------------------------------------------------
def check_advances(capi, ctx, law, rho_grain, par, every, visits):
    """`visits` times: read the device's state and last row, run `every` steps, advance dust_ref from that state over the
    row's own interval with the device's gas columns, compare"""
    P = ctx.params
    dt, t = 1e-2, 0.0
    worst_x = worst_v = 0.0
    for k in range(visits):
        st = ctx.dust_state()
        head, body = rows_of(ctx)
        prev, t_prev = body[-1], head[-1, 1]
        sinks0 = ctx.get_sinks()
        x0, v0 = np.stack([st["x"], st["y"], st["z"]], 1), np.stack([st["vx"], st["vy"], st["vz"]], 1)
        assert same_bits(x0, prev[0:3].T) and same_bits(v0, prev[3:6].T)
        S = {"a": dust_ref.sink_accel(x0, sinks0, P.G), "vg": prev[8:11].T.copy(), "r": prev[11].copy()}
        for _ in range(every):
            dt, t = ctx.step(dt, t)
        head, body = rows_of(ctx)
        assert head.shape[0] == k + 2 and head[-1, 0] == k + 2 and head[-1, 1] == t
        row, delta = body[-1], head[-1, 2]
        assert delta == t - t_prev and delta > 0.0
        sinks1 = ctx.get_sinks()
        o = dust_ref.advance(x0, v0, par, S, delta, {"rho": row[6], "vg": row[8:11].T, "u": row[7]}, sinks1, G=P.G, law=law,
                             rho_grain=rho_grain, gamma=P.gamma, gamma_m1=P.gamma_m1)
        assert np.all(o["fate"] == 0) and np.all(np.isfinite(row))
        norm = lambda w: np.linalg.norm(w, axis=1)
        ex, ev = norm(row[0:3].T - o["x"]), norm(row[3:6].T - o["v"])
        bx = 1e-13 * (norm(o["x"]) + norm(o["v"]) * delta)
        bv = 1e-13 * np.maximum(np.maximum(norm(o["v"]), norm(o["S"]["vg"])), norm(o["S"]["a"]) * delta)
        worst_x, worst_v = max(worst_x, np.max(ex / bx)), max(worst_v, np.max(ev / bv))
        print(f"visit {k}: delta {delta:.3e}  max ex/bound {np.max(ex / bx):.3e}  max ev/bound {np.max(ev / bv):.3e}")
        assert np.all(ex <= bx) and np.all(ev <= bv)
        assert np.allclose(row[11], o["S"]["r"], rtol=1e-14, atol=0.0)
        assert np.any(row[11] > 0.0)
    return worst_x, worst_v


@pytest.mark.parametrize("law,every", [("fixed_ts", 1), ("epstein", 1), ("epstein", 3)])
def test_one_advance_matches_the_restatement(capi, law, every):
    gas, sinks = golden_gas("bin2000_traj")                    # two moving sinks: the stored a and the new a differ
    ctx = make_context(capi, gas, sinks, flags=full(capi))
    m = 300
    x, v = grains_of(gas, m, seed=11)
    rng = np.random.default_rng(12)
    if law == "fixed_ts":
        par, rho_grain = rng.uniform(0.002, 0.5, m), None      # stopping times from stiff to loose against dt = 1e-2
    else:
        # sizes that put the drag rate around 1 / dt: read the rate of unit grains, then scale
        ctx.dust_begin(x, v, np.ones(m), law="epstein", rho_grain=1.0, capacity=1)
        ctx.dust_advance()
        unit = np.median(ctx.dust()["rate"][0][ctx.dust()["rate"][0] > 0.0])
        par, rho_grain = unit * rng.uniform(0.002, 0.5, m), 1.0
    ctx.dust_begin(x, v, par, law=law, rho_grain=rho_grain, capacity=8, every=every)
    ctx.dust_advance()
    visits = 5 if every == 1 else 2
    check_advances(capi, ctx, capi.DUST_LAWS[law], rho_grain or 1.0, par, every, visits)
    head, _ = rows_of(ctx)
    assert head[:, 0].tolist() == list(range(1, visits + 2))
    assert ctx.dust_info() == {"rows": visits + 1, "dropped": 0, "advances": visits + 1, "n_grains": m, "n_live": m}
    ctx.close()


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def logged(capi, gas, sinks, x, v, par, flags, steps=6, one_run=False):
    ctx = make_context(capi, gas, sinks, flags=flags)
    ctx.dust_begin(x, v, par, law="epstein", rho_grain=1.0, capacity=steps + 1)
    ctx.dust_advance()
    dt, t = 1e-2, 0.0
    if one_run:
        ctx.run(steps, dt, t)
    else:
        for _ in range(steps):
            dt, t = ctx.step(dt, t)
    head, body = rows_of(ctx)
    ctx.close()
    assert head.shape[0] == steps + 1
    return head, body


def test_a_grain_does_not_depend_on_the_others_or_on_the_grid(capi):
    gas, sinks = golden_gas("bin2000_traj")
    m = 400
    x, v = grains_of(gas, m, seed=21)
    par = np.random.default_rng(22).uniform(1e-4, 1e-1, m)
    head, body = logged(capi, gas, sinks, x, v, par, full(capi))
    assert np.all(np.isfinite(body)) and np.any(body[-1, 11] > 0.0)
    h2, b2 = logged(capi, gas, sinks, x[:m // 2], v[:m // 2], par[:m // 2], full(capi))
    assert same_bits(b2, body[:, :, :m // 2])
    h3, b3 = logged(capi, gas, sinks, x[::-1], v[::-1], par[::-1], full(capi))
    assert same_bits(b3[:, :, ::-1], body)
    h4, b4 = logged(capi, gas, sinks, x, v, par, over_defaults(capi, full(capi) | capi.FLAG_HASHED_GRID, False))
    assert same_bits(b4, body) and same_bits(h4, head)
    h5, b5 = logged(capi, gas, sinks, x, v, par, full(capi), one_run=True)
    assert same_bits(b5, body) and same_bits(h5, head)


# ---- 4. nothing else changes ----------------------------------------------------------------------------------------------------
def test_dust_changes_nothing_of_the_run(capi):
    gas, sinks = golden_gas("acc2000_traj")
    x, v = grains_of(gas, 500, seed=31)
    out = []
    for on in (True, False):
        ctx = make_context(capi, gas, sinks, flags=full(capi))
        ctx.history_begin(8)
        ctx.track_begin(np.arange(0, 2000, 7), 8)
        if on:
            ctx.dust_begin(x, v, np.full(500, 1e-3), law="epstein", rho_grain=1.0, capacity=2, remove=True)
        before = ctx.stats().host_syncs
        dts, dt, t = [], 1e-2, 0.0
        for _ in range(5):
            dt, t = ctx.step(dt, t)
            dts.append((dt, t))
        st = ctx.stats()
        fields = {f: ctx.field(f) for f in ["x", "y", "z", "vx", "vy", "vz", "u", "m", "alpha", "rho", "ax", "du"]}
        out.append((dts, fields, ctx.get_sinks(), ctx.history()["rows"], ctx.track()["body"], st.host_syncs - before, st.device_bytes))
        if on:
            assert ctx.dust_info(live=False) == {"rows": 2, "dropped": 3, "advances": 5, "n_grains": 500}
        ctx.close()
    a, b = out
    assert a[0] == b[0] and a[5] == b[5], (a[0], b[0], a[5], b[5])
    for f in a[1]:
        assert same_bits(a[1][f], b[1][f]), f
    for k in a[2]:
        assert same_bits(a[2][k], b[2][k]), k
    assert same_bits(a[3], b[3]) and same_bits(a[4], b[4])
    assert a[6] > b[6]                                                # the state, the sample, the log and the fates are counted


# ---- 5. every, record_every and the log's bookkeeping ---------------------------------------------------------------------------
def test_every_and_record_every(capi):
    gas, sinks = golden_gas("disc3000_traj")
    x, v = grains_of(gas, 100, seed=41)
    par = np.full(100, 0.05)
    ctx = make_context(capi, gas, sinks)
    ctx.history_begin(16)
    ctx.dust_begin(x, v, par, law="fixed_ts", capacity=3, every=3)
    ctx.run(10, 1e-2, 0.0)
    times = ctx.history()["rows"][:, 1]
    d = ctx.dust()
    assert d["advance"].tolist() == [1, 2, 3] and same_bits(d["t"], times[[2, 5, 8]])
    assert d["delta"][0] == times[2] and same_bits(d["delta"][1:], np.array([times[5] - times[2], times[8] - times[5]]))
    assert ctx.dust_info() == {"rows": 3, "dropped": 0, "advances": 3, "n_grains": 100, "n_live": 100}
    # record_every: advances 2 and 4 of four are rows; a log of one row drops the second
    ctx.dust_begin(x, v, par, law="fixed_ts", capacity=1, record_every=2)             # begin replaces begin
    assert ctx.dust_info() == {"rows": 0, "dropped": 0, "advances": 0, "n_grains": 100, "n_live": 100}
    ctx.run(4, 1e-2, 0.0)
    assert ctx.dust_info(live=False) == {"rows": 1, "dropped": 1, "advances": 4, "n_grains": 100}
    d = ctx.dust()
    assert d["advance"].tolist() == [2] and d["body"].shape == (1, 12, 100)
    assert ctx.dust(1)["body"].shape == (0, 12, 100) and ctx.dust(0, 0)["head"].shape == (0, 4)
    for first, count in ((-1, 1), (0, 2), (2, 0), (1, 1), (0, -1)):
        with pytest.raises(capi.SphError):
            ctx.dust(first, count)
    # capacity 0: state and fates only
    ctx.dust_begin(x, v, par, law="fixed_ts", capacity=0)
    ctx.run(2, 1e-2, 0.0)
    assert ctx.dust_info() == {"rows": 0, "dropped": 2, "advances": 2, "n_grains": 100, "n_live": 100}
    assert ctx.dust()["body"].shape == (0, 12, 100)
    moved = ctx.dust_state()
    assert not same_bits(moved["x"], x[:, 0]) and same_bits(moved["par"], par) and np.all(ctx.dust_fates()["fate"] == 0)
    ctx.close()


def test_state_begins_again_bitwise(capi):
    import torch
    gas, sinks = golden_gas("disc3000_traj")
    x, v = grains_of(gas, 200, seed=51)
    par = np.random.default_rng(52).uniform(0.01, 1.0, 200)
    logs = []
    for split in (False, True):
        ctx = make_context(capi, gas, sinks)
        ctx.dust_begin(x, v, par, law="fixed_ts", capacity=4)
        dt, t = ctx.run(2, 1e-2, 0.0)
        if split:
            st = ctx.dust_state(device=True)                  # saved and begun again, on the device
            assert all(isinstance(a, torch.Tensor) for a in st.values())
            host = ctx.dust_state()
            assert all(same_bits(st[k].cpu().numpy(), host[k]) for k in host)
            ctx.dust_begin([st["x"], st["y"], st["z"]], [st["vx"], st["vy"], st["vz"]], st["par"], law="fixed_ts", capacity=4)
        ctx.run(2, dt, t)
        d = ctx.dust(device=split)
        logs.append(d["body"].cpu().numpy() if split else d["body"])
        if split:
            f = ctx.dust_fates(device=True)
            assert f["fate"].cpu().numpy().tolist() == [0] * 200
        ctx.close()
    assert logs[0].shape == (4, 12, 200) and logs[1].shape == (2, 12, 200)
    assert same_bits(logs[1], logs[0][2:])


# ---- 6. no gas in reach: a kick-drift-kick step conserves the angular momentum ----------------------------------------------------
def test_angular_momentum_is_conserved_without_gas(capi):
    gas, sinks = golden_gas("disc3000_traj")
    ctx = make_context(capi, gas, sinks)
    h = float(ctx.params.h)
    rng = np.random.default_rng(61)
    m = 50
    R, phi = rng.uniform(5.0, 40.0, m), rng.uniform(0.0, 2.0 * np.pi, m)
    z = np.max(np.abs(gas["z"])) + 10.0 * h + rng.uniform(0.0, 5.0, m)
    sx = np.array([sinks["x"][0], sinks["y"][0], sinks["z"][0]])
    x = np.stack([R * np.cos(phi), R * np.sin(phi), z], 1) + sx
    vk = np.sqrt(ctx.params.G * sinks["m"][0] / R)
    v = np.stack([-vk * np.sin(phi), vk * np.cos(phi), rng.normal(0.0, 0.1, m) * vk], 1) * rng.uniform(0.7, 1.2, (m, 1))
    ctx.dust_begin(x, v, np.full(m, 1e-3), law="epstein", rho_grain=1.0, capacity=201)
    ctx.dust_advance()
    dt = 0.05
    for k in range(1, 201):
        set_clock(ctx, dt, k * dt)                             # the gas and the sink stay: only the clock moves
        ctx.dust_advance()
    d = ctx.dust()
    ctx.close()
    assert d["head"].shape[0] == 201 and np.all(d["rho_g"] == 0.0) and np.all(d["rate"] == 0.0)
    assert np.all(np.abs(d["delta"][1:] - dt) < 1e-12)
    pos = np.stack([d["x"], d["y"], d["z"]], -1) - sx
    L = np.cross(pos, np.stack([d["vx"], d["vy"], d["vz"]], -1))
    drift = np.linalg.norm(L - L[0], axis=-1) / np.linalg.norm(L[0], axis=-1)
    print("largest relative change of L:", drift.max())
    assert drift.max() <= 1e-12
    assert np.linalg.norm(pos[-1] - pos[0], axis=-1).min() > 1.0   # they did move


# ---- 7. fates -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove", [True, False])
def test_fates(capi, remove):
    gas, _ = golden_gas("disc3000_traj")
    sinks = {"x": np.array([0.0, 0.2]), "y": np.zeros(2), "z": np.zeros(2), "vx": np.zeros(2), "vy": np.zeros(2), "vz": np.zeros(2),
             "m": np.array([1.0, 0.5]), "radius": np.array([1.0, 2.0])}
    ctx = make_context(capi, gas, sinks)
    bound = float(ctx.params.bounding_size)
    #          into sink 1 only   into both: sink 0   a bystander      across the bound        on sink 0
    x = np.array([[2.5, 0.0, 0.5], [0.0, 3.0, 0.5], [20.0, 0.0, 0.0], [bound - 0.5, 0.0, 0.0], [0.0, 0.0, 0.0]])
    v = np.array([[-10.0, 0.0, 0.0], [0.0, -25.0, 0.0], [0.0, 0.2, 0.0], [10.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    ctx.dust_begin(x, v, np.full(5, 1e30), law="fixed_ts", capacity=4, remove=remove)
    assert ctx.dust_info()["n_live"] == 4                      # the grain on the sink left at begin: advance 0
    ctx.dust_advance()
    set_clock(ctx, 0.1, 0.1)
    ctx.dust_advance()
    set_clock(ctx, 0.1, 0.2)
    ctx.dust_advance()
    f, d, info = ctx.dust_fates(), ctx.dust(), ctx.dust_info()
    ctx.close()
    assert d["advance"].tolist() == [1, 2, 3] and np.all(np.isnan(d["body"][:, :, 4]))
    if remove:
        assert f["fate"].tolist() == [1, 1, 0, 2, 3] and f["advance"].tolist() == [2, 2, 0, 2, 0]
        assert f["sink"].tolist() == [1, 0, -1, -1, -1]
        assert d["n_live"].tolist() == [4, 1, 1] and info["n_live"] == 1
        assert np.all(np.isfinite(d["body"][0, :, :4])) and np.all(np.isnan(d["body"][1:, :, [0, 1, 3]]))
        assert np.all(np.isfinite(d["body"][:, :, 2]))
    else:
        assert f["fate"].tolist() == [0, 0, 0, 0, 3] and f["sink"].tolist() == [-1] * 5
        assert d["n_live"].tolist() == [4, 4, 4] and np.all(np.isfinite(d["body"][:, :, :4]))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_scope(capi):
    import ctypes as C
    gas, sinks = golden_gas("disc3000_traj")
    ctx = make_context(capi, gas, sinks)
    x, v = grains_of(gas, 10, seed=71)
    par = np.full(10, 0.1)

    def code(fn, *a, **k):
        with pytest.raises(capi.SphError) as e:
            fn(*a, **k)
        return e.value.status

    # the two codes, from calls whose refusal is documented elsewhere
    ARG = code(lambda: ctx._ck(ctx.lib.sph_track_begin(ctx._h, None, 1, None)))
    STATE = code(ctx.track_end)
    for fn in (ctx.dust_end, ctx.dust_advance, ctx.dust_info, ctx.dust, ctx.dust_state, ctx.dust_fates):
        assert code(fn) == STATE, fn
    for bad in (0.0, -1.0, np.nan, np.inf):
        p = par.copy(); p[7] = bad
        assert code(ctx.dust_begin, x, v, p, law="fixed_ts") == ARG, bad
        assert code(ctx.dust_begin, x, v, par, law="epstein", rho_grain=bad) == ARG, bad
    assert code(ctx.dust_begin, x, v, par, law="fixed_ts", capacity=-1) == ARG
    assert code(ctx.dust_begin, x, v, par, law="fixed_ts", every=0) == ARG
    assert code(ctx.dust_begin, x, v, par, law="fixed_ts", record_every=0) == ARG
    d = capi.dust_desc("fixed_ts")
    cols = [np.ascontiguousarray(a) for a in (*x.T, *v.T, par)]
    ptrs = [a.ctypes.data for a in cols]
    begin = lambda desc, m, pp: ctx._ck(ctx.lib.sph_dust_begin(ctx._h, desc, m, *pp))
    assert code(begin, None, 10, ptrs) == ARG
    assert code(begin, C.byref(d), 0, ptrs) == ARG
    assert code(begin, C.byref(d), 10, ptrs[:6] + [None]) == ARG and code(begin, C.byref(d), 10, [None] + ptrs[1:]) == ARG
    d.law = 2
    assert code(begin, C.byref(d), 10, ptrs) == ARG
    d.law, d.flags = 1, 2
    assert code(begin, C.byref(d), 10, ptrs) == ARG
    assert code(ctx.dust_info) == STATE                        # none of the refused calls began anything
    # ghosts and ranks refuse begin ...
    ctx.set_owned(2000)
    assert code(ctx.dust_begin, x, v, par, law="fixed_ts") == STATE
    ctx.set_owned(3000)
    ctx.set_rank(0, 2)
    assert code(ctx.dust_begin, x, v, par, law="fixed_ts") == STATE
    ctx.set_rank(0, 1)
    # ... and close dust that was begun; the rows stay readable
    for close in (lambda: ctx.set_owned(2000), lambda: ctx.set_rank(1, 2)):
        ctx.dust_begin(x, v, par, law="fixed_ts", capacity=4)
        ctx.dust_advance()
        close()
        assert code(ctx.dust_advance) == STATE
        assert ctx.dust()["body"].shape == (1, 12, 10) and ctx.dust_info()["advances"] == 1
        assert np.all(ctx.dust_fates()["fate"] == 0) and same_bits(ctx.dust_state()["x"], x[:, 0])
        ctx.set_owned(3000)
        ctx.set_rank(0, 1)
    # a new upload keeps the grains: they are sampled against the new gas
    ctx.dust_begin(x, v, par, law="fixed_ts", capacity=4)
    ctx.dust_advance()
    ctx.upload({k: np.asarray(a)[:1500] for k, a in gas.items()})
    ctx.set_sinks(sinks)
    ctx.dust_advance()
    d = ctx.dust()
    assert d["body"].shape == (2, 12, 10) and same_bits(d["x"][1], d["x"][0]) and not same_bits(d["rho_g"][1], d["rho_g"][0])
    out, den = ctx.sample(x, fields=("vx", "vy", "vz", "u"), normalise=True, weight_out=True)
    assert same_bits(d["rho_g"][1], den) and same_bits(d["body"][1, 8:11], out[:3])
    bytes_on = ctx.stats().device_bytes
    ctx.dust_end()
    assert ctx.stats().device_bytes < bytes_on and code(ctx.dust_end) == STATE
    ctx.close()


# ---- 9. the command line --------------------------------------------------------------------------------------------------------
def test_cli_runs_a_small_save_file(capi, tmp_path):
    from summersph_amd import txtio
    gas, sinks = golden_gas("disc3000_traj")
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "dust.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.dust", str(save), "--steps", "6", "--dt", "1e-2", "--grains", "200",
                        "--size-cm", "0.1", "--rho-grain", "3", "--every", "1", "--record-every", "2", "--remove", "-o", str(out),
                        "--json"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    z = np.load(out)
    assert summary["grains"] == 200 and summary["rows"] == 4 and summary["advances"] == 7
    assert z["body"].shape == (4, 12, 200) and z["head"].shape == (4, 4) and z["fates"].shape == (200, 3)
    assert z["advance"].tolist() == [1, 3, 5, 7] and list(z["columns"]) == capi.DUST_COLUMNS
    assert z["par"].shape == (200,) and np.all(z["par"] > 0.0) and summary["live"] == int(np.sum(z["fates"][:, 0] == 0))
