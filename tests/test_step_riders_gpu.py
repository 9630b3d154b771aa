"""The riders of the persistent pair kernels give the bits of the stand-alone launches.

On the plain fixed-h step sph_run lets the sinks' sums run as extra workgroups ("riders", csrc/rider_common.hpp) in the
tails of the tile kernels instead of as launches of their own: sink_accel_partial on density_wt and sink_accel_final on the
forces_q launch behind it (SPH_NO_SINK_RIDE switches the item off, SPH_NO_RIDERS the rider roles as such).  The riders run
the stand-alone kernels' own device code with their block size, items per block and order of sums, so every result must be
IDENTICAL: fields, sinks with their accelerations, dt, t, the build report as sph_get_stats shows it, and the number of host
waits.

The switches (and SPH_TILE_MIN_GROUPS_D) are read once per process, so each side of a comparison is a fresh child process
(this file, run as a script), one after the other, each under its own time limit; a child that fails ends the module.
Two kinds of child:
  small    SPH_TILE_MIN_GROUPS_D=0, so that density_wt runs with fewer groups than CUs and a ragged last group: a disc of
           20 000 particles with 0, 1 and 2 sinks, sph_run(6) and 6 x sph_run(1); the same disc under
           SPH_FLAG_HASHED_GRID; the sinkacc timing group's launch count; and the list-overflow report of
           steady_sets.contraction_too_fast("mid"): the call that raises and its message.
           Sides: riders on, all switches off, and each switch alone (SPH_NO_SINK_RIDE: the step does not ask; SPH_NO_RIDERS:
           the launchers carry none whatever they are asked).
  natural  the natural kernel selection: 270 000 particles (just over one density_wt group per CU) and 3 000 (the gather
           density kernel runs, forces_q does: the stand-alone launches must still be taken, which the sinkacc timing
           group's launch count shows).  Sides: riders on, all off.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("SPH_NO_RIDERS", "SPH_NO_SINK_RIDE")
FIELDS = "x y z vx vy vz u alpha rho ax ay az du".split()
SINK_COLS = "x y z vx vy vz m ax ay az".split()
REPORT = "nlist_capacity nlist_max tile_fit_pct tile_fit_pct_forces host_syncs grid_builds nlist_builds".split()
STEPS = 6


def _record(out, tag, ctx, dt, t):
    for f in FIELDS:
        out[f"{tag}/{f}"] = ctx.field(f)
    s = ctx.get_sinks()
    for k in SINK_COLS:
        out[f"{tag}/sink_{k}"] = s[k]
    out[f"{tag}/dt_t"] = np.array([dt, t])
    st = ctx.stats()
    out[f"{tag}/report"] = np.array([getattr(st, k) for k in REPORT], dtype=np.int64)


def _sinks(sinks, ns):
    """the disc's central sink; ns = 2 adds a light companion in the central hole, ns = 0 takes it away"""
    if ns == 0:
        return {k: np.zeros(0) for k in sinks}
    if ns == 1:
        return sinks
    two = {k: np.concatenate([v, np.zeros(1)]) for k, v in sinks.items()}
    two["x"][1], two["y"][1], two["vy"][1], two["m"][1] = 1.7, 0.3, 0.6, 0.02
    return two


def _run_both_ways(out, tag, capi, gas, sinks, **kw):
    for how in ("run", "steps"):
        ctx = capi.Context(device=0, **kw)
        ctx.upload(gas)
        ctx.set_sinks(sinks)
        dt, t = 1e-2, 0.0
        if how == "run":
            dt, t = ctx.run(STEPS, dt, t)
        else:
            for _ in range(STEPS):
                dt, t = ctx.run(1, dt, t)
        _record(out, f"{tag}/{how}", ctx, dt, t)
        ctx.close()


def _sinkacc_launches(out, tag, capi, gas, sinks):
    """which launches the sinks' sums took in three steps: the timing group counts them"""
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    ctx.timing(True, only=["sinkacc"])
    ctx.run(3, 1e-2, 0.0)
    out[f"{tag}/sinkacc_launches"] = np.array([ctx.timing_get("sinkacc")[1]])
    ctx.close()


def _small(out):
    import steady_sets as S
    from summersph_amd import capi, ic

    gas, sinks = ic.split_rows(ic.keplerian_disc(20000, seed=41))
    for ns in (0, 1, 2):
        _run_both_ways(out, f"ns{ns}", capi, gas, _sinks(sinks, ns))
    _run_both_ways(out, "hashed", capi, gas, sinks, flags=capi.FLAG_HASHED_GRID)

    _sinkacc_launches(out, "timed", capi, gas, sinks)

    # the overflow report arrives at the same call, in the same words
    s = S.build("contraction_too_fast_mid")
    ctx = capi.Context(device=0)
    ctx.upload(s["gas"])
    seen = []
    for call in ("run", "stats", "density"):
        try:
            if call == "run":
                ctx.run(len(s["dts"]), s["dts"][0], 0.0)
            elif call == "stats":
                ctx.stats()
            else:
                ctx.density()
            seen.append(f"{call}: ok")
        except capi.SphError as e:
            seen.append(f"{call}: {e}")
    out["overflow/seen"] = np.array(seen)
    ctx.close()


def _natural(out):
    from summersph_amd import capi, ic

    for n, seed in ((270000, 42), (3000, 43)):
        gas, sinks = ic.split_rows(ic.keplerian_disc(n, seed=seed))
        _run_both_ways(out, f"n{n}", capi, gas, sinks)
        _sinkacc_launches(out, f"timed{n}", capi, gas, sinks)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    result = {}
    {"small": _small, "natural": _natural}[sys.argv[1]](result)
    np.savez(sys.argv[2], **result)
    sys.exit(0)


import pytest  # noqa: E402

pytestmark = pytest.mark.gpu

SIDES = {"on": (), "off": SWITCHES, "no_sink_ride": ("SPH_NO_SINK_RIDE",), "no_riders": ("SPH_NO_RIDERS",)}


def _child(d, kind, side, extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "SPH_TILE_MIN_GROUPS_D"}
    env.update({k: "1" for k in SIDES[side]})
    env.update(extra)
    path = str(d / f"{kind}_{side}.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), kind, path], check=True, env=env, timeout=600, cwd=ROOT)
    return dict(np.load(path))


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_riders_small")
    return {side: _child(d, "small", side, {"SPH_TILE_MIN_GROUPS_D": "0"}) for side in SIDES}


@pytest.fixture(scope="module")
def natural(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_riders_natural")
    return {side: _child(d, "natural", side, {}) for side in ("on", "off")}


def _tag(side, tag):
    return sorted(k for k in side if k.startswith(tag + "/"))


def _same(a, b, tag):
    keys = _tag(a, tag)
    assert keys and keys == _tag(b, tag), tag
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


SMALL_TAGS = ["ns0", "ns1", "ns2", "hashed"]


@pytest.mark.parametrize("side", [s for s in SIDES if s != "off"])
@pytest.mark.parametrize("tag", SMALL_TAGS)
def test_small_disc_equals_the_stand_alone_launches(small, tag, side):
    """sph_run(6) and 6 x sph_run(1), fewer density_wt groups than CUs: every side against all switches off"""
    _same(small[side], small["off"], tag)


@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("tag", SMALL_TAGS)
def test_one_run_equals_single_step_runs(small, tag, side):
    """one call of six steps against six calls of one: what a launch leaves for the next does not outlive its evaluation"""
    s = small[side]
    for k in _tag(s, tag + "/run"):
        if not k.endswith("/report"):      # (host waits differ: every call that returns waits)
            assert np.array_equal(s[k], s[k.replace("/run/", "/steps/")]), k


def test_the_sums_did_ride(small):
    """three steps, two evaluations each: a partial + final launch pair per evaluation without the riders, none with them"""
    for side in ("off", "no_sink_ride", "no_riders"):
        assert small[side]["timed/sinkacc_launches"][0] == 6, side
    assert small["on"]["timed/sinkacc_launches"][0] == 0


def test_the_gather_density_pass_keeps_the_stand_alone_launches(natural):
    """3 000 particles: density_kernel runs, so nothing rides although forces_q runs -- six launch pairs on either side;
    270 000: the natural selection is density_wt, and the sums ride"""
    assert natural["on"]["timed3000/sinkacc_launches"][0] == natural["off"]["timed3000/sinkacc_launches"][0] == 6
    assert natural["off"]["timed270000/sinkacc_launches"][0] == 6 and natural["on"]["timed270000/sinkacc_launches"][0] == 0


@pytest.mark.parametrize("side", [s for s in SIDES if s != "off"])
def test_list_overflow_is_reported_at_the_same_call(small, side):
    seen = list(small["off"]["overflow/seen"])
    assert "overflowed in the previous build" in seen[0] and seen[0].startswith("run: "), seen
    assert list(small[side]["overflow/seen"]) == seen


@pytest.mark.parametrize("tag", ["n270000", "n3000"])
def test_natural_selection_equals_the_stand_alone_launches(natural, tag):
    """270 000: density_wt just over one group per CU; 3 000: the gather density kernel, stand-alone sums behind it"""
    _same(natural["on"], natural["off"], tag)
    for k in _tag(natural["on"], tag + "/run"):
        if not k.endswith("/report"):
            assert np.array_equal(natural["on"][k], natural["on"][k.replace("/run/", "/steps/")]), k
