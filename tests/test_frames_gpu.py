"""GPU tests of the movie of a run (sph_frames): the one-shot frame against the long-double restatement (tests/frames_ref.py)
and against sph_transfer's optical depth, its independence of every order bit for bit, the log of sph_run against a twin
context stepped one step at a time with a one-shot frame after each, the cadence rule replayed on the history's t, the
bookkeeping and every argument error, the run with frames against its twin without, the smallest sets and footprints at
which the splat can go wrong, and the Fortran host and the command line end to end."""
import math

import numpy as np
import pytest

from conftest import load_golden
from gpu_support import capi, golden_gas, make_context, positions, var_params
import frames_ref
from summersph_amd import cube, frames
from track_ref import same_bits

pytestmark = pytest.mark.gpu

SPH_ERR_ARG, SPH_ERR_STATE = 1, 5
SHAPE = (65, 63)
VIEWS = {"face": (0.0, 0.0), "inclined": (40.0, 30.0), "edge": (90.0, 0.0)}
BOUND = 1e-12          # of the plane's largest reference sum of |term|: sph_cube's and sph_transfer's bound


def flat(n, seed=0, box=4.0, m=1e-3):
    """n particles at rest in a thin slab |z| < 0.1 of |x|, |y| < box"""
    rng = np.random.default_rng(seed)
    g = {"x": rng.uniform(-box, box, n), "y": rng.uniform(-box, box, n), "z": rng.uniform(-0.1, 0.1, n)}
    g.update({k: np.zeros(n) for k in ("vx", "vy", "vz")})
    g.update(u=rng.uniform(0.5, 1.5, n), m=np.full(n, m), alpha=np.ones(n))
    return g


def at(points, m=1e-3, **over):
    """particles at the given (x, y, z) rows"""
    p = np.atleast_2d(np.asarray(points, dtype=np.float64))
    n = len(p)
    g = {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy()}
    g.update({k: np.zeros(n) for k in ("vx", "vy", "vz")})
    g.update(u=np.ones(n), m=np.broadcast_to(np.asarray(m, dtype=np.float64), (n,)).copy(), alpha=np.ones(n))
    g.update({k: np.asarray(v, dtype=np.float64) for k, v in over.items()})
    return g


def check_against_ref(head, planes, gas, h, fields, shape, bounds, rot=None, centre=(0.0, 0.0, 0.0), clip=None):
    """every node within BOUND of the plane's largest reference sum of |term|; returns the worst ratio to that bound"""
    sums, mags, n_sel = frames_ref.frame(positions(gas), gas["m"], h, [gas[f] for f in fields], shape, bounds, rot, centre, clip)
    assert planes.shape == sums.shape and int(head[3]) == n_sel and int(head[2]) == len(gas["m"]) and head[11] == 0
    worst = 0.0
    for q in range(len(sums)):
        scale = float(mags[q].max())
        err = float(np.max(np.abs(planes[q].astype(np.longdouble) - sums[q])))
        print(f"plane {q}: max |err| {err:.3e}, max sum |term| {scale:.3e}, ratio to the bound {err / (BOUND * scale) if scale else 0:.3e}")
        assert err <= BOUND * scale, (q, err, scale)
        worst = max(worst, err / (BOUND * scale) if scale else 0.0)
    return worst


def image_box(gas, rot, shrink=0.9):
    """a node box that cuts the set's projected extent on every side"""
    P = frames_ref.project(positions(gas), rot, (0.0, 0.0, 0.0))
    lo, hi = P[:, :2].min(axis=0) * shrink, P[:, :2].max(axis=0) * shrink
    return ((float(lo[0]), float(lo[1])), (float(hi[0]), float(hi[1])))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("name", ["sod1000", "disc3000", "discv3000"])
def test_frame_against_the_long_double_sum_and_transfer(capi, name, view):
    g = load_golden(name + "_eval")
    gas, sinks = golden_gas(name + "_eval")
    variable = "h" in gas
    ctx = make_context(capi, gas, sinks, variable=variable, **(var_params(g) if variable else {}))
    rot = cube.view(*VIEWS[view])
    bounds = image_box(gas, rot)
    head, planes = ctx.frame(SHAPE, bounds, rot=rot, fields=("u", "vx"))
    h = gas["h"] if variable else float(ctx.params.h)
    check_against_ref(head, planes, gas, h, ("u", "vx"), SHAPE, bounds, rot)
    assert head[0] == 0 and head[1] == 0.0 and np.all(head[12:] == 0) and np.all(head[4:7] == 0)
    y0 = gas["m"] / (np.pi * (h * h))
    assert head[7:11].tolist()[:3] == [frames_ref.exponent(y0), frames_ref.exponent(y0 * gas["u"]), frames_ref.exponent(y0 * gas["vx"])]
    assert math.isnan(head[10])
    # plane 0 is sph_transfer's optical depth with kappa = 1 on the same nodes
    tau = ctx.transfer(SHAPE, bounds, rot=rot, source=None, kappa=None, tau_max=np.inf)[1]
    _, mags, _ = frames_ref.frame(positions(gas), gas["m"], h, [], SHAPE, bounds, rot)
    assert np.max(np.abs(planes[0] - tau)) <= BOUND * float(mags[0].max())
    ctx.close()


@pytest.mark.parametrize("case", ["h", "clip", "centre"])
def test_frame_with_h_override_clip_and_centre(capi, case):
    gas, sinks = golden_gas("disc3000_eval")
    ctx = make_context(capi, gas, sinks)
    rot = cube.view(40.0, 30.0)
    bounds = ((-30.0, -25.0), (28.0, 31.0))
    kw = {"h": dict(h=1.3), "clip": dict(clip=((-20.0, -35.0, -2.0), (25.0, 15.0, 3.0))), "centre": dict(centre=(3.0, -4.0, 1.0))}[case]
    head, planes = ctx.frame(SHAPE, bounds, rot=rot, fields=("vx",), **kw)
    check_against_ref(head, planes, gas, kw.get("h", float(ctx.params.h)), ("vx",), SHAPE, bounds, rot, kw.get("centre", (0.0, 0.0, 0.0)),
                      kw.get("clip"))
    assert head[4:7].tolist() == list(kw.get("centre", (0.0, 0.0, 0.0)))
    if case == "clip":
        assert 0 < head[3] < 3000
    ctx.close()


# ---- 2. order independence, bitwise ------------------------------------------------------------------------------------------------
def test_frame_does_not_depend_on_any_order(capi):
    gas, sinks = golden_gas("disc3000_eval")
    rot = cube.view(40.0, 30.0)
    kw = dict(shape=SHAPE, bounds=((-30.0, -25.0), (28.0, 31.0)), rot=rot, fields=("u", "vx"), h=2.0)
    ctx = make_context(capi, gas, sinks, density=True)
    head, planes = ctx.frame(**kw)
    again = ctx.frame(**kw)
    assert same_bits(head, again[0]) and same_bits(planes, again[1])                  # a repeated call
    dh, dp = ctx.frame(device=True, **kw)
    assert same_bits(head, dh.cpu().numpy()) and same_bits(planes, dp.cpu().numpy())  # the device form
    ctx.close()
    perm = np.random.default_rng(5).permutation(3000)
    others = {"permuted": (dict(gas={k: np.asarray(v)[perm] for k, v in gas.items()}), {}),
              "another h": ({}, dict(h=4.0)),                                           # binned with another h
              "hashed": ({}, dict(flags=capi.default_params(False).flags | capi.FLAG_HASHED_GRID))}
    for what, (g, params) in others.items():
        b = make_context(capi, g.get("gas", gas), sinks, density=True, **params)
        bh, bp = b.frame(**kw)
        b.close()
        assert same_bits(head, bh) and same_bits(planes, bp), what
    assert np.all(np.isfinite(planes)) and planes[0].max() > 0


# ---- 3. the log against a twin -----------------------------------------------------------------------------------------------------
def case_flags(capi, name):
    return capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL if name in ("acc2000_traj", "bin2000_traj") else 0


@pytest.mark.parametrize("name,steps", [("disc3000_traj", 5), ("discv3000_traj", 3), ("acc2000_traj", 3)])
def test_log_is_bitwise_the_twins_one_shot_frames(capi, name, steps):
    g = load_golden(name)
    gas, sinks = golden_gas(name)
    variable = "h" in gas
    kw = dict(variable=variable, flags=case_flags(capi, name), **(var_params(g) if variable else {}))
    fr = dict(shape=(33, 31), bounds=((-35.0, -30.0), (30.0, 35.0)), rot=cube.view(40.0, 30.0), fields=("u", "rho"))
    a = make_context(capi, gas, sinks, **kw)
    a.frames_begin(capacity=steps, **fr)
    a.run(steps, 1e-2, 0.0)
    log, info = a.frames(), a.frames_info()
    a.close()
    assert info == {"rows": steps, "dropped": 0, "steps": steps} and log["planes"].shape == (steps, 3, 33, 31)
    b = make_context(capi, gas, sinks, **kw)
    b.frames_begin(capacity=1, every=10 ** 6, **fr)                   # counts the twin's steps and records none
    dt, t = 1e-2, 0.0
    for r in range(steps):
        dt, t = b.step(dt, t)
        head, planes = b.frame(**fr)
        assert same_bits(log["head"][r], head) and same_bits(log["planes"][r], planes), r
        assert (log["step"][r], log["t"][r], log["n"][r], log["n_sel"][r], log["status"][r]) == (r + 1, t, b.n, b.n, 0), r
        assert np.all(np.isfinite(planes)) and planes[0].max() > 0 and planes[2].max() > 0
    assert b.frames_info() == {"rows": 0, "dropped": 0, "steps": steps}
    if case_flags(capi, name):
        assert b.n < len(gas["m"])                                    # the packs did happen
    b.close()


def test_frame_follows_a_sink(capi):
    gas, sinks = golden_gas("bin2000_traj")
    flags = case_flags(capi, "bin2000_traj")
    fr = dict(shape=(17, 19), bounds=((-10.0, -10.0), (10.0, 10.0)), centre=(0.5, -0.25, 0.125), centre_sink=0)
    a = make_context(capi, gas, sinks, flags=flags)
    a.frames_begin(capacity=4, **fr)
    a.run(3, 1e-2, 0.0)
    log = a.frames()
    a.frames_begin(capacity=1, every=1, shape=3, bounds=((-1.0, -1.0), (1.0, 1.0)), fields=("u",), centre_sink=5)     # no such sink
    a.frames_record()
    gone = a.frames()
    a.close()
    assert gone["status"].tolist() == [capi.FRAMES_SINK_GONE] and np.all(np.isnan(gone["planes"])) and gone["planes"].shape == (1, 2, 3, 3)
    b = make_context(capi, gas, sinks, flags=flags)
    dt, t = 1e-2, 0.0
    centres = []
    for r in range(3):
        dt, t = b.step(dt, t)
        s = b.get_sinks()
        centres.append([0.5 + s["x"][0], -0.25 + s["y"][0], 0.125 + s["z"][0]])
    head, planes = b.frame(**fr)
    b.close()
    assert same_bits(log["centre"], np.array(centres)) and np.any(log["centre"][0] != log["centre"][2])
    assert same_bits(log["planes"][2], planes) and same_bits(log["head"][2][1:], head[1:]) and log["planes"][2][0].max() > 0


# ---- 4. cadence, capacity, the bookkeeping and the errors ---------------------------------------------------------------------------
def test_time_cadence_is_the_replayed_rule(capi):
    gas, sinks = golden_gas("disc3000_traj")
    fr = dict(shape=9, bounds=((-30.0, -30.0), (30.0, 30.0)))
    ctx = make_context(capi, gas, sinks)
    ctx.history_begin(16)
    ctx.run(8, 1e-2, 0.0)
    dt_frame = float(ctx.history()["t"][-1]) / 3.3                    # some steps record and some do not
    ctx.close()
    ctx = make_context(capi, gas, sinks)
    ctx.history_begin(16)
    ctx.frames_begin(capacity=16, dt_frame=dt_frame, **fr)
    dt, t = ctx.run(8, 1e-2, 0.0)
    ts = ctx.history()["t"]
    log = ctx.frames()
    want = frames_ref.cadence(ts, 0.0, dt_frame)
    print("t", ts.tolist(), "dt_frame", dt_frame, "recorded", log["step"].tolist())
    assert log["step"].tolist() == want and 0 < len(want) < 8 and same_bits(log["t"], ts[np.array(want) - 1])
    assert ctx.frames_info() == {"rows": len(want), "dropped": 0, "steps": 8}
    # capacity 2 with 4 due frames: 2 rows, 2 dropped; t0 is the t of this begin
    ctx.frames_begin(capacity=2, dt_frame=1e-6, **fr)
    dt, t = ctx.run(4, dt, t)
    assert ctx.frames_info() == {"rows": 2, "dropped": 2, "steps": 4}
    assert ctx.frames()["step"].tolist() == [1, 2] and ctx.frames()["dropped"] == 2
    # rewind between two runs: the rows start again, the steps and the dropped count go on
    ctx.frames_rewind()
    assert ctx.frames_info() == {"rows": 0, "dropped": 2, "steps": 4}
    dt, t = ctx.run(1, dt, t)
    log = ctx.frames()
    assert log["step"].tolist() == [5] and log["t"][0] == t and ctx.frames_info()["rows"] == 1
    ctx.close()


def test_every_begin_twice_record_read_and_end(capi):
    gas, sinks = golden_gas("disc3000_traj")
    fr = dict(shape=(5, 7), bounds=((-30.0, -30.0), (30.0, 30.0)), fields=("u",))
    ctx = make_context(capi, gas, sinks)
    for call in (ctx.frames_record, ctx.frames_rewind, ctx.frames_end, ctx.frames_info, ctx.frames):
        with pytest.raises(capi.SphError) as err:
            call()
        assert err.value.status == SPH_ERR_STATE
    assert ctx.lib.sph_frames_read(ctx._h, 0, 0, None, None) == SPH_ERR_STATE
    ctx.frames_begin(capacity=3, every=2, **fr)
    dt, t = ctx.run(5, 1e-2, 0.0)
    assert ctx.frames()["step"].tolist() == [2, 4] and ctx.frames_info() == {"rows": 2, "dropped": 0, "steps": 5}
    ctx.frames_record()                                               # whatever the cadence; the number is not advanced
    ctx.frames_record()                                               # full: dropped and counted
    log = ctx.frames()
    assert log["step"].tolist() == [2, 4, 5] and ctx.frames_info() == {"rows": 3, "dropped": 1, "steps": 5}
    assert log["t"][2] == t and log["planes"].shape == (3, 2, 5, 7)
    part = ctx.frames(1, 2)
    assert same_bits(part["planes"], log["planes"][1:]) and same_bits(part["head"], log["head"][1:])
    dev = ctx.frames(0, 3, device=True)
    assert same_bits(dev["planes"].cpu().numpy(), log["planes"]) and same_bits(dev["head"].cpu().numpy(), log["head"])
    assert ctx.frames(3)["planes"].shape[0] == 0
    hd, pl = np.zeros((4, 16)), np.zeros((4, 2, 5, 7))
    for first, count in ((-1, 1), (0, 4), (2, 2), (4, 0), (0, -1)):
        assert ctx.lib.sph_frames_read(ctx._h, first, count, hd.ctypes.data, pl.ctypes.data) == SPH_ERR_ARG, (first, count)
    assert np.all(hd == 0) and np.all(pl == 0)
    assert ctx.lib.sph_frames_read(ctx._h, 1, 1, hd.ctypes.data, None) == 0 and same_bits(hd[0], log["head"][1])
    ctx.frames_begin(capacity=8, every=1, **fr)                       # a second begin: rows, steps and dropped start again
    assert ctx.frames_info() == {"rows": 0, "dropped": 0, "steps": 0}
    small = {k: np.asarray(v)[:500] for k, v in gas.items()}
    ctx.upload(small)                                                 # a new set: the recorder names no particle and stays
    ctx.frames_record()
    ctx.run(1, dt, t)
    log = ctx.frames()
    assert log["step"].tolist() == [0, 1] and log["n"].tolist() == [500, 500] and log["planes"][1][0].max() > 0
    bytes_on = ctx.stats().device_bytes
    ctx.frames_end()
    assert ctx.stats().device_bytes < bytes_on                        # the log and the limbs are given back
    ctx.run(1, dt, t)                                                 # steps record nothing again
    with pytest.raises(capi.SphError) as err:
        ctx.frames_info()
    assert err.value.status == SPH_ERR_STATE
    ctx.close()


def test_a_stale_field_is_a_nan_plane(capi):
    gas, sinks = golden_gas("disc3000_traj")
    ctx = make_context(capi, gas, sinks)                              # no density yet: sph_download_field refuses rho
    head, planes = ctx.frame(9, ((-30.0, -30.0), (30.0, 30.0)), fields=("u", "rho"))
    assert np.all(np.isnan(planes[2])) and np.all(np.isfinite(planes[:2])) and math.isnan(head[9]) and not math.isnan(head[8])
    ctx.density()
    head, planes = ctx.frame(9, ((-30.0, -30.0), (30.0, 30.0)), fields=("u", "rho"))
    assert np.all(np.isfinite(planes)) and planes[2].max() > 0
    ctx.close()


def test_every_argument_error(capi):
    gas, sinks = golden_gas("disc3000_traj")
    ctx = make_context(capi, gas, sinks)
    good = dict(shape=(5, 7), bounds=((-3.0, -3.0), (3.0, 3.0)), capacity=2)
    bad_rot = np.eye(3)
    bad_rot[0, 0] = 1.0 + 1e-9
    inf, nan = np.inf, np.nan
    cases = {"rot": dict(rot=bad_rot), "left-handed": dict(rot=np.diag([1.0, 1.0, -1.0])), "n_u": dict(shape=(0, 7)),
             "n_v": dict(shape=(5, 0)), "lo inf": dict(bounds=((-inf, -3.0), (3.0, 3.0))), "hi nan": dict(bounds=((-3.0, -3.0), (3.0, nan))),
             "lo > hi": dict(bounds=((4.0, -3.0), (3.0, 3.0))), "h < 0": dict(h=-1.0), "h inf": dict(h=inf),
             "nan clip": dict(clip=((nan, -1.0, -1.0), (1.0, 1.0, 1.0))), "centre": dict(centre=(0.0, inf, 0.0)),
             "capacity": dict(capacity=0), "neither": dict(every=0), "both": dict(every=2, dt_frame=0.5),
             "dt_frame < 0": dict(every=0, dt_frame=-1.0), "dt_frame nan": dict(every=0, dt_frame=nan), "field": dict(fields=(99,)),
             "field < 0": dict(fields=(-1,)), "sink": dict(centre_sink=64)}
    for what, over in cases.items():
        d = capi.frames_desc(**{**good, **over})
        assert ctx.lib.sph_frames_begin(ctx._h, d) == SPH_ERR_ARG, what
        if what not in ("capacity", "neither", "both", "dt_frame < 0", "dt_frame nan"):     # the one-shot form reads no cadence
            hd, pl = np.zeros(16), np.zeros((1 + d.nq) * max(d.n_u, 1) * max(d.n_v, 1))
            assert ctx.lib.sph_frame(ctx._h, d, hd.ctypes.data, pl.ctypes.data, pl.size) == SPH_ERR_ARG, what
    d = capi.frames_desc(**good)
    d.nq = 4
    assert ctx.lib.sph_frames_begin(ctx._h, d) == SPH_ERR_ARG
    d = capi.frames_desc(**good)
    d.reserved = 1
    assert ctx.lib.sph_frames_begin(ctx._h, d) == SPH_ERR_ARG
    assert ctx.lib.sph_frames_begin(ctx._h, None) == SPH_ERR_ARG
    d = capi.frames_desc(**good)
    hd, pl = np.zeros(16), np.zeros(35)
    assert ctx.lib.sph_frame(ctx._h, d, hd.ctypes.data, pl.ctypes.data, 34) == SPH_ERR_ARG
    assert ctx.lib.sph_frame(ctx._h, d, None, pl.ctypes.data, 35) == SPH_ERR_ARG
    assert ctx.lib.sph_frame(ctx._h, d, hd.ctypes.data, None, 35) == SPH_ERR_ARG
    with pytest.raises(capi.SphError) as err:
        ctx.frames_info()                                             # none of the refused begins left a log behind
    assert err.value.status == SPH_ERR_STATE
    ctx.close()


# ---- 5. no behaviour change --------------------------------------------------------------------------------------------------------
STATE = "x y z vx vy vz u m alpha".split()


def test_frames_change_nothing_of_the_run(capi):
    gas, sinks = golden_gas("acc2000_traj")
    out = []
    for on in (True, False):
        ctx = make_context(capi, gas, sinks, flags=capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL)
        if on:
            ctx.frames_begin(shape=(33, 31), bounds=((-40.0, -40.0), (40.0, 40.0)), capacity=2, fields=("u", "rho", "vx"))
        dt, t = ctx.run(3, 1e-2, 0.0)
        st = ctx.stats()
        counters = {f: (list(getattr(st, f)) if f == "grid_dim" else getattr(st, f)) for f, _ in st._fields_ if f != "device_bytes"}
        out.append((dt, t, {f: ctx.field(f) for f in STATE + ["rho", "ax", "du"]}, ctx.get_sinks(), counters, st.device_bytes))
        if on:
            assert ctx.frames_info() == {"rows": 2, "dropped": 1, "steps": 3}
        ctx.close()
    a, b = out
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4], (a[4], b[4])
    for f in a[2]:
        assert same_bits(a[2][f], b[2][f]), f
    for k in a[3]:
        assert same_bits(a[3][k], b[3][k]), k
    assert a[5] > b[5]                                                # the log and the limbs are counted


@pytest.mark.parametrize("cadence", [dict(every=1), dict(dt_frame=None)], ids=["every", "dt_frame"])
def test_frames_add_no_host_synchronisation(capi, cadence):
    gas, sinks = golden_gas("disc3000_traj")
    syncs = []
    for on in (True, False):
        ctx = make_context(capi, gas, sinks)
        dt, t = ctx.run(4, 1e-2, 0.0)
        if on:
            how = cadence if "every" in cadence else dict(dt_frame=2.5 * dt)          # about one step in three records
            ctx.frames_begin(shape=33, bounds=((-40.0, -40.0), (40.0, 40.0)), capacity=8, fields=("u",), **how)
        before = ctx.stats().host_syncs
        ctx.run(8, dt, t)                                             # into the steady state
        syncs.append(ctx.stats().host_syncs - before)
        if on:
            rows = ctx.frames_info()["rows"]
            assert rows == 8 if "every" in cadence else 0 < rows < 8, rows
        ctx.close()
    assert syncs[0] == syncs[1], syncs


# ---- 6. the smallest shapes at which the splat can go wrong -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_small_particle_counts(capi, n):
    gas = flat(n, seed=n)
    ctx = make_context(capi, gas)
    bounds = ((-3.0, -3.5), (3.5, 3.0))
    head, planes = ctx.frame((17, 15), bounds, fields=("u",), h=0.7)
    check_against_ref(head, planes, gas, 0.7, ("u",), (17, 15), bounds)
    assert planes[0].max() > 0
    ctx.close()


def test_one_more_than_a_grid_stride_of_the_maxima_pass(capi):
    n = 1024 * 256 + 1                                                # frames_maxima's blocks at most x its block, and one
    rng = np.random.default_rng(3)
    gas = flat(n, m=1e-9)
    gas["x"] = rng.uniform(100.0, 200.0, n)                           # all off the image ...
    gas["x"][-1], gas["y"][-1], gas["z"][-1], gas["m"][-1] = 0.25, -0.5, 0.0, 3.0      # ... but the heaviest, which sets the exponent
    ctx = make_context(capi, gas)
    bounds = ((-3.0, -3.0), (3.0, 3.0))
    head, planes = ctx.frame((17, 15), bounds, h=0.9)
    ctx.close()
    one = make_context(capi, {k: v[-1:] for k, v in gas.items()})
    h1, p1 = one.frame((17, 15), bounds, h=0.9)
    one.close()
    assert head[3] == n and h1[3] == 1 and head[7] == h1[7] and same_bits(planes, p1) and planes.max() > 0


def test_footprints_of_every_size_and_place(capi):
    # nodes at the integers -4 .. 4 on both axes, h = 0.2: 2 h = 0.4 is below the spacing
    shape, bounds = (9, 9), ((-4.0, -4.0), (4.0, 4.0))
    pts = [(0.5, 0.5, 0.0),                                           # between the nodes: no node in the footprint
           (1.0 + 0.3, 2.0, 0.0),                                     # exactly one node, p = 1.5
           (-2.0, 3.0, 0.0),                                          # a node at p = 0
           (-3.0 + np.nextafter(0.4, 0.0), -3.0, 0.0)]                # p within an ulp of 2
    for k, p in enumerate(pts):
        gas = at([p] if k < 3 else [p, (2.0, -1.0, 0.0)])             # the second particle gives the plane its scale
        ctx = make_context(capi, gas)
        head, planes = ctx.frame(shape, bounds, h=0.2)
        ctx.close()
        check_against_ref(head, planes, gas, 0.2, (), shape, bounds)
        lit = int(np.count_nonzero(planes[0]))
        assert lit == (0 if k == 0 else 1) or k == 3, (k, lit)
        if k == 2:
            assert abs(planes[0][2, 7] / (1.5 * (1e-3 / (np.pi * (0.2 * 0.2)))) - 1.0) <= 1e-15      # F(0) = 1.5
        if k == 3:
            assert lit in (1, 2) and abs(planes[0][1, 1]) <= 1e-15 * planes[0][6, 3]
    # footprints cut by each edge and each corner, h = 0.8; and one particle with h much larger than the image
    edge = [(-4.0 - 0.5, 0.2, 0.0), (4.0 + 0.5, -0.3, 0.0), (0.1, -4.0 - 0.5, 0.0), (0.3, 4.0 + 0.5, 0.0),
            (-4.3, -4.3, 0.0), (-4.3, 4.3, 0.0), (4.3, -4.3, 0.0), (4.3, 4.3, 0.0)]
    for gas, h in ((at(edge), 0.8), (at([(0.3, -0.2, 0.0)]), 500.0)):
        ctx = make_context(capi, gas)
        head, planes = ctx.frame(shape, bounds, h=h)
        ctx.close()
        check_against_ref(head, planes, gas, h, (), shape, bounds)
        assert planes[0].max() > 0
    assert np.all(planes[0] > 0)                                      # the large h covers every node


def test_one_node_and_a_flat_axis(capi):
    gas = flat(100, seed=2)
    ctx = make_context(capi, gas)
    head, planes = ctx.frame((1, 1), ((0.25, -0.5), (0.25, -0.5)), fields=("u",), h=1.1)
    check_against_ref(head, planes, gas, 1.1, ("u",), (1, 1), ((0.25, -0.5), (0.25, -0.5)))
    assert planes.shape == (2, 1, 1) and planes[0, 0, 0] > 0
    head, planes = ctx.frame((4, 5), ((1.0, -2.0), (1.0, 2.0)), fields=("u",), h=1.1)       # lo == hi with n > 1
    check_against_ref(head, planes, gas, 1.1, ("u",), (4, 5), ((1.0, -2.0), (1.0, 2.0)))
    assert same_bits(planes[:, 0], planes[:, 3]) and planes[0].max() > 0
    ctx.close()


def test_coincident_particles_carry_through_the_limbs(capi):
    """4096 particles in one place: every term is the same integer near 2^62 at the node under them, so the low limb
    carries every few adds.  The sum is 4096 times the device's own rounded term, which one particle's frame shows."""
    shape, bounds, h, m = (5, 5), ((-1.0, -1.0), (1.0, 1.0)), 0.9, 1.2345678901234567e-3
    one = make_context(capi, at([(0.0, 0.0, 0.0)], m=m))
    h1, p1 = one.frame(shape, bounds, h=h)
    one.close()
    many = make_context(capi, at(np.zeros((4096, 3)), m=m))
    hn, pn = many.frame(shape, bounds, h=h)
    many.close()
    e = int(h1[7])
    assert hn[7] == e and hn[3] == 4096
    fixed = np.ldexp(p1[0], 62 - e)                                   # the device's rounded terms: integers below 2^62
    assert np.all(fixed == np.rint(fixed)) and 2.0 ** 61 <= fixed[2, 2] < 2.0 ** 62
    want = np.array([[math.ldexp(float(4096 * int(v)), e - 62) for v in row] for row in fixed])
    assert same_bits(pn[0], want)


def test_mirrored_set_cancels_exactly(capi):
    rng = np.random.default_rng(11)
    n = 300
    p = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(0.1, 1.0, n)], axis=1)
    both = np.concatenate([p, p * np.array([1.0, 1.0, -1.0])])
    gas = at(both, m=np.tile(rng.uniform(1e-4, 1e-3, n), 2), vx=np.concatenate([np.ones(n), -np.ones(n)]))
    ctx = make_context(capi, gas)
    head, planes = ctx.frame((17, 15), ((-3.0, -3.0), (3.0, 3.0)), fields=("vx",), h=0.6)
    ctx.close()
    assert np.all(planes[1] == 0.0) and planes[0].max() > 0 and head[3] == 2 * n


def test_masses_over_forty_decades(capi):
    gas = flat(400, seed=4)
    gas["m"] = 10.0 ** np.linspace(-40.0, 0.0, 400)
    ctx = make_context(capi, gas)
    bounds = ((-3.0, -3.5), (3.5, 3.0))
    head, planes = ctx.frame((17, 15), bounds, fields=("u",), h=0.7)
    ctx.close()
    check_against_ref(head, planes, gas, 0.7, ("u",), (17, 15), bounds)


def test_one_nan_value_spoils_only_its_plane(capi):
    gas = flat(200, seed=6)
    gas["vx"][17] = np.nan
    ctx = make_context(capi, gas)
    head, planes = ctx.frame((9, 9), ((-3.0, -3.0), (3.0, 3.0)), fields=("u", "vx"), h=0.7)
    ctx.close()
    assert np.all(np.isnan(planes[2])) and np.all(np.isfinite(planes[:2])) and planes[1].max() > 0
    assert math.isnan(head[9]) and not math.isnan(head[7]) and not math.isnan(head[8])


def test_a_selection_that_reaches_nothing(capi):
    gas = flat(200, seed=7)
    ctx = make_context(capi, gas)
    head, planes = ctx.frame((9, 9), ((-3.0, -3.0), (3.0, 3.0)), fields=("u",), h=0.7, clip=((50.0, 50.0, 50.0), (60.0, 60.0, 60.0)))
    assert np.all(planes == 0.0) and head[3] == 0 and head[2] == 200 and head[7] == 0 and head[8] == 0
    head, planes = ctx.frame((9, 9), ((30.0, 30.0), (40.0, 40.0)), h=0.7)      # selected, but off the image
    assert np.all(planes == 0.0) and head[3] == 200
    ctx.close()


# ---- 7. the Fortran host's movie file -----------------------------------------------------------------------------------------------
def test_fortran_host_writes_the_frames_file(tmp_path):
    """SPH_FRAMES_FILE switches the file on; the run itself (its dt lines) is what it is without"""
    import os
    import subprocess
    from conftest import ROOT
    from summersph_amd import txtio
    host = os.path.join(ROOT, "summersph_amd", "host", "run_sph_hip")
    if not os.path.exists(host):
        subprocess.run(["make", "-C", os.path.dirname(host)], check=True, stdout=subprocess.DEVNULL)
    g = load_golden("disc3000_traj")
    gas, _ = golden_gas("disc3000_traj")
    icf, movie = tmp_path / "ic.txt", tmp_path / "movie.bin"
    txtio.write_ic(str(icf), g["ic"])
    off = {k: v for k, v in os.environ.items() if not k.startswith("SPH_FRAMES_")}
    runs = []
    for env in (dict(off, SPH_FRAMES_FILE=str(movie), SPH_FRAMES_EVERY="2", SPH_FRAMES_SIZE="33"), off):
        r = subprocess.run([host, str(icf), "5"], capture_output=True, text=True, cwd=tmp_path, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        runs.append([l for l in r.stdout.splitlines() if l.startswith("dt ")])
    assert runs[0] == runs[1] and len(runs[0]) == 6
    raw = movie.read_bytes()
    rows, dropped, steps, n = np.frombuffer(raw[:32], dtype=np.int64).tolist()
    assert (rows, dropped, steps, n) == (2, 0, 5, 33) and len(raw) == 32 + 8 * rows * (16 + n * n)
    head = np.frombuffer(raw[32:32 + 8 * 16 * rows]).reshape(rows, 16)
    planes = np.frombuffer(raw[32 + 8 * 16 * rows:]).reshape(rows, n, n)
    assert head[:, 0].tolist() == [2.0, 4.0] and np.all(head[:, 11] == 0) and np.all(head[:, 2] == head[:, 3]) and head[0, 2] > 0
    assert np.all(head[:, 4:7] == 0) and 0 < head[0, 1] < head[1, 1]
    assert np.all(np.isfinite(planes)) and np.all(planes >= 0) and planes[1].max() > 0
    # the node box is the initial bounding box in x and y, face-on: the column integrates to about the mass inside
    dx = (gas["x"].max() - gas["x"].min()) / (n - 1)
    dy = (gas["y"].max() - gas["y"].min()) / (n - 1)
    assert 0.5 * gas["m"].sum() < planes[0].sum() * dx * dy < 1.5 * gas["m"].sum()
    assert sorted(os.listdir(tmp_path)) == ["ic.txt", "movie.bin"]    # no other output file appears


# ---- 8. the command line end to end ------------------------------------------------------------------------------------------------
def test_cli_runs_a_save_file(tmp_path, capsys):
    import json
    g = load_golden("acc2000_traj")
    save = tmp_path / "save.txt"
    with open(save, "w") as f:                                        # a save file: gas records of 9 values, sinks of 8
        f.write("x y z vx vy vz u m alpha\n")
        for r in g["ic"]:
            f.write(" ".join(f"{v:.17e}" for v in (r if r[6] == 0.0 else list(r) + [0.0])) + "\n")
    out = tmp_path / "movie.npz"
    assert frames.main([str(save), "--steps", "3", "--every", "1", "--size", "33", "--extent", "80", "--inc", "40", "--pa", "30",
                        "--fields", "u", "--follow-sink", "0", "--self-gravity", "--accrete", "-o", str(out), "--json"]) == 0
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s["rows"] == 4 and s["dropped"] == 0 and s["steps"] == [0, 1, 2, 3] and s["shape"] == [4, 2, 33, 33] and s["status"] == [0] * 4
    z = np.load(out)
    assert z["planes"].shape == (4, 2, 33, 33) and z["n"].tolist() == [int(v) for v in g["full_n_seq"]]
    assert z["t_end"] == g["full_t_end"][0] and z["t"][3] == z["t_end"] and int(z["desc_centre_sink"]) == 0 and int(z["desc_nq"]) == 1
    assert np.all(np.isfinite(z["planes"])) and z["planes"][:, 0].max() > 0
    mean_u = frames.mean(z["planes"])
    seen = z["planes"][:, :1] > 0
    assert mean_u.shape == (4, 1, 33, 33) and np.all(np.isnan(mean_u[~seen])) and np.all(mean_u[seen] > 0)
