"""The call-order state machine of the context, as a caller can observe it.

Three small contexts (the 2000-particle accretion set of tests/golden with its sink: fixed h, variable h, fixed h with
self-gravity) are brought to `sph_density` + `sph_forces`; then one mutating entry point is applied and the test records
  (a) the status of a download of every SPH_F_* field,
  (b) the status of sph_forces, sph_kick, sph_next_dt, sph_refresh_eos, sph_update_h and sph_forces_part(2) when called
      next -- each on a replay of its own,
  (c) how many grid builds, list builds, re-flags, density and force passes the following sph_density + sph_forces take,
and compares rho, P, c and the rates of that evaluation with a fresh context that was uploaded with the downloaded state.
(a) to (c) are integers; the literals below were recorded on the commit before the validity flags moved into
csrc/ctx_state.hpp, so they pin the invalidation rules as they were.

The last test is about the pinned block: sph_set_boundary_boxes with 64 boxes must not disturb a fixed-h run (the staging
used to reach into the read-back slots of the one-build-late reports)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, rel_err
from gpu_support import capi
from summersph_amd import ic
from test_parity_gpu import EVAL_TOL

pytestmark = pytest.mark.gpu

DERIVED = ["rho", "P", "c", "ax", "ay", "az", "du", "dalpha"]
PROBES = ["forces", "kick", "next_dt", "refresh_eos", "update_h", "forces_part2"]
COUNTERS = ["grid_builds", "nlist_builds", "nlist_reflags", "density_passes", "force_passes"]
DT = 1e-3


def case_kw(capi, case):
    if case == "variable":
        return dict(variable=True)
    return dict(flags=capi.FLAG_SELF_GRAVITY) if case == "gravity" else {}


class Replay:
    """a context at sph_density + sph_forces of the set (after one accretion pass where `packed`)"""

    def __init__(self, capi, case, gas, sinks, packed=False):
        self.capi, self.case = capi, case
        self.ctx = ctx = capi.Context(device=0, **case_kw(capi, case))
        self.lib, self.h = ctx.lib, ctx._h
        ctx.upload(gas); ctx.set_sinks(sinks)
        ctx.density(); ctx.forces()
        if packed:
            assert ctx.accrete_and_cull() > 0
            ctx.density(); ctx.forces()

    def close(self):
        self.ctx.close()


def mutations(case):
    up = ["up_x", "up_vx", "up_u", "up_m", "up_alpha", "up_rho"] + (["up_h"] if case == "variable" else [])
    return up + ["kick", "drift", "kick_drift_devdt", "kick_dt_candidate_dev", "update_h", "set_sinks", "set_owned",
                 "set_numbers_dev", "set_gravity_sources_dev", "replace_ghosts_dev", "accrete_some", "accrete_none",
                 "scatter_fields_dev"]


def mutate(r, name, keep):
    """applies one mutating call to the replay; returns (status, particles afterwards).  Uploads write back the values the
    context holds, so that only the validity changes; `keep` holds the device buffers until the context is closed"""
    import torch
    lib, h, ctx = r.lib, r.h, r.ctx
    n = ctx.n
    if name.startswith("up_"):
        f = name[3:]
        a = np.ascontiguousarray(ctx.field(f))
        st = lib.sph_upload_field(h, r.capi.FIELDS.index(f), a.ctypes.data, a.size)
    elif name == "kick":
        st = lib.sph_kick(h, DT)
    elif name == "drift":
        st = lib.sph_drift(h, DT)
    elif name == "kick_drift_devdt":
        ctx.set_dt(DT)
        st = lib.sph_kick_drift_devdt(h)
    elif name == "kick_dt_candidate_dev":
        ctx.set_dt(DT)
        st = lib.sph_kick_dt_candidate_dev(h)
    elif name == "update_h":
        st = lib.sph_update_h(h)
    elif name == "set_sinks":
        s = ctx.get_sinks()
        arrs = [np.ascontiguousarray(s[k]) for k in "x y z vx vy vz m".split()]
        st = lib.sph_set_sinks(h, arrs[0].size, *[a.ctypes.data for a in arrs])
    elif name == "set_owned":
        st = lib.sph_set_owned(h, n)
    elif name == "set_numbers_dev":
        t = torch.arange(n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        keep.append(t)
        st = lib.sph_set_numbers_dev(h, 0, n, C.c_void_p(t.data_ptr()))
    elif name == "set_gravity_sources_dev":
        st = lib.sph_set_gravity_sources_dev(h, 0, None, np.zeros(6).ctypes.data)
    elif name == "replace_ghosts_dev":
        st = lib.sph_replace_ghosts_dev(h, 0, None)
    elif name in ("accrete_some", "accrete_none"):
        removed = C.c_int64(0)
        st = lib.sph_accrete_and_cull(h, C.byref(removed))
        assert (removed.value > 0) == (name == "accrete_some"), (name, removed.value)
    elif name == "scatter_fields_dev":
        t = torch.from_numpy(np.stack([ctx.field("vx"), ctx.field("u")])).to("cuda:0")
        torch.cuda.synchronize()
        keep.append(t)
        f = (C.c_int32 * 2)(r.capi.FIELDS.index("vx"), r.capi.FIELDS.index("u"))
        st = lib.sph_scatter_fields_dev(h, 2, f, 0, n, C.c_void_p(t.data_ptr()))
    else:
        raise KeyError(name)
    return int(st), int(ctx.n)


def probe(r, name):
    lib, h = r.lib, r.h
    if name == "forces":
        return lib.sph_forces(h)
    if name == "kick":
        return lib.sph_kick(h, DT)
    if name == "next_dt":
        d = C.c_double(1e-2)
        return lib.sph_next_dt(h, C.byref(d))
    if name == "refresh_eos":
        return lib.sph_refresh_eos(h)
    if name == "update_h":
        return lib.sph_update_h(h)
    return lib.sph_forces_part(h, 2)


def downloads(r):
    """the status of a download of every field, one digit each (0 = accepted)"""
    out = np.zeros(r.ctx.n)
    return "".join(str(abs(int(r.lib.sph_download_field(r.h, k, out.ctypes.data, out.size))))
                   for k in range(len(r.capi.FIELDS)))


def fresh_evaluation(capi, case, ctx):
    """rho, P, c and the rates of a new context that holds what `ctx` holds"""
    gas = {k: ctx.field(k) for k in capi.FIELDS[:9]}
    if case == "variable":
        gas["h"] = ctx.field("h")
    sinks = ctx.get_sinks()
    f = capi.Context(device=0, **case_kw(capi, case))
    f.upload(gas); f.set_sinks(sinks)
    f.density(); f.forces()
    out = {k: f.field(k) for k in DERIVED}
    f.close()
    return out


def observe(capi, case, name, gas, sinks):
    """(status, n, downloads, probe statuses, counter deltas, bitwise) of one mutation + the largest relative error of the
    following evaluation against a fresh context"""
    packed = name == "accrete_none"
    keep = []
    r = Replay(capi, case, gas, sinks, packed)
    st, n = mutate(r, name, keep)
    dl = downloads(r)
    s0 = r.ctx.stats()
    before = [int(getattr(s0, k)) for k in COUNTERS]
    ev = (int(r.lib.sph_density(r.h)), int(r.lib.sph_forces(r.h)))
    s1 = r.ctx.stats()
    deltas = tuple(int(getattr(s1, k)) - b for k, b in zip(COUNTERS, before))
    bitwise, err = True, 0.0
    if ev == (0, 0):
        got = {k: r.ctx.field(k) for k in DERIVED}
        want = fresh_evaluation(capi, case, r.ctx)
        bitwise = all(np.array_equal(got[k], want[k]) for k in DERIVED)
        err = max(rel_err(got[k], want[k]) for k in DERIVED)
    r.close()
    probes = []
    for p in PROBES:
        r = Replay(capi, case, gas, sinks, packed)
        mutate(r, name, keep)
        probes.append(abs(int(probe(r, p))))
        r.close()
    return (st, n, dl, "".join(map(str, probes)), ev + deltas, bitwise), err


# case -> mutation -> (status of the call, particles afterwards, download statuses of the 19 fields, statuses of PROBES,
#                      statuses of the following sph_density and sph_forces + the deltas of COUNTERS over them,
#                      whether that evaluation equals the fresh context's bit for bit)
EXPECT = {'fixed': {'up_x': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), True),
           'up_vx': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
           'up_u': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
           'up_m': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), True),
           'up_alpha': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
           'up_rho': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
           'kick': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
           'drift': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), False),
           'kick_drift_devdt': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), False),
           'kick_dt_candidate_dev': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
           'update_h': (5, 2000, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), True),
           'set_sinks': (0, 2000, '0000000000005555555', '055055', (0, 0, 0, 0, 0, 1, 1), True),
           'set_owned': (0, 2000, '0000000005555555555', '555555', (0, 0, 1, 1, 0, 1, 1), True),
           'set_numbers_dev': (0, 2000, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), True),
           'set_gravity_sources_dev': (5, 2000, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), True),
           'replace_ghosts_dev': (0, 2000, '0000000005555555555', '555555', (0, 0, 1, 1, 0, 1, 1), True),
           'accrete_some': (0, 1997, '0000000000000000055', '555555', (0, 0, 1, 1, 0, 1, 1), False),
           'accrete_none': (0, 1997, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), False),
           'scatter_fields_dev': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True)},
 'variable': {'up_x': (0, 2000, '0000000000000000000', '500555', (0, 0, 1, 1, 0, 1, 1), True),
              'up_vx': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True),
              'up_u': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True),
              'up_m': (0, 2000, '0000000000000000000', '500555', (0, 0, 1, 1, 0, 1, 1), True),
              'up_alpha': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True),
              'up_rho': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True),
              'up_h': (0, 2000, '0000000000000000000', '500555', (0, 0, 0, 1, 0, 1, 1), True),
              'kick': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True),
              'drift': (0, 2000, '0000000000000000000', '500555', (0, 0, 1, 1, 0, 1, 1), True),
              'kick_drift_devdt': (0, 2000, '0000000000000000000', '500555', (0, 0, 1, 1, 0, 1, 1), True),
              'kick_dt_candidate_dev': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True),
              'update_h': (0, 2000, '0000000000000000000', '500555', (0, 0, 0, 1, 0, 1, 1), False),
              'set_sinks': (0, 2000, '0000000000005555500', '055005', (0, 0, 0, 0, 0, 1, 1), True),
              'set_owned': (0, 2000, '0000000005555555505', '555555', (0, 0, 1, 1, 0, 1, 1), True),
              'set_numbers_dev': (0, 2000, '0000000000000000000', '500555', (0, 0, 1, 1, 0, 1, 1), True),
              'set_gravity_sources_dev': (0, 2000, '0000000005555555505', '555555', (0, 0, 1, 1, 0, 1, 1), True),
              'replace_ghosts_dev': (0, 2000, '0000000005555555505', '555555', (0, 0, 1, 1, 0, 1, 1), True),
              'accrete_some': (0, 1996, '0000000000000000000', '555555', (0, 0, 1, 1, 0, 1, 1), True),
              'accrete_none': (0, 1996, '0000000000000000000', '000005', (0, 0, 0, 0, 0, 1, 1), True),
              'scatter_fields_dev': (0, 2000, '0000000000000000000', '500005', (0, 0, 0, 0, 0, 1, 1), True)},
 'gravity': {'up_x': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), True),
             'up_vx': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
             'up_u': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
             'up_m': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), True),
             'up_alpha': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
             'up_rho': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
             'kick': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
             'drift': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), True),
             'kick_drift_devdt': (0, 2000, '0000000000000000055', '500555', (0, 0, 1, 1, 0, 1, 1), True),
             'kick_dt_candidate_dev': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True),
             'update_h': (5, 2000, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), True),
             'set_sinks': (0, 2000, '0000000000005555555', '055055', (0, 0, 0, 0, 0, 1, 1), True),
             'set_owned': (0, 2000, '0000000005555555555', '555555', (0, 0, 1, 1, 0, 1, 1), True),
             'set_numbers_dev': (0, 2000, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), True),
             'set_gravity_sources_dev': (0, 2000, '0000000000005555555', '055055', (0, 0, 0, 0, 0, 1, 1), True),
             'replace_ghosts_dev': (0, 2000, '0000000005555555555', '555555', (0, 0, 1, 1, 0, 1, 1), True),
             'accrete_some': (0, 1997, '0000000000000000055', '555555', (0, 0, 1, 1, 0, 1, 1), True),
             'accrete_none': (0, 1997, '0000000000000000055', '000055', (0, 0, 0, 0, 0, 1, 1), True),
             'scatter_fields_dev': (0, 2000, '0000000000000000055', '500055', (0, 0, 0, 0, 0, 1, 1), True)}}


@pytest.mark.parametrize("case", ["fixed", "variable", "gravity"])
def test_call_order(capi, case):
    gas, sinks = ic.split_rows(load_golden("acc2000_traj")["ic"])
    wrong = []
    for name in mutations(case):
        got, err = observe(capi, case, name, gas, sinks)
        print(case, name, got, f"err {err:.2e}")
        want = EXPECT[case][name]
        if got[:5] != want[:5]:
            wrong.append((name, got, want))
        if not (got[5] if want[5] else err <= EVAL_TOL):       # bit for bit where the recorded run was, else one evaluation's bar
            wrong.append((name, "evaluation", got[5], err))
    assert not wrong, wrong


def test_boundary_boxes_leave_the_read_back_slots_alone(capi):
    """64 staged boxes are 384 doubles: in the old numbered block they covered both bounding-box reports, both list reports,
    the trim moments and the accretion words (staging at +128, reports from +200).  Two identical fixed-h runs, one of which
    stages 64 boxes between two steps, must stay identical"""
    rows = ic.keplerian_disc(2000, seed=11)
    gas, sinks = ic.split_rows(rows)
    rng = np.random.default_rng(5)
    lo = rng.uniform(-40.0, 40.0, (64, 3)) + 0.37
    boxes = np.concatenate([lo, lo + rng.uniform(0.5, 9.5, (64, 3))], axis=1)
    runs = []
    for stage in (False, True):
        ctx = capi.Context(device=0)
        ctx.upload(gas); ctx.set_sinks(sinks)
        dts, dt = [], 1e-2
        for k in range(6):
            if stage and k == 3:
                ctx.set_boundary_boxes(boxes)
            dt, _ = ctx.step(dt)
            dts.append(dt)
        st = ctx.stats()
        runs.append((dts, ctx.state(), int(st.host_syncs), int(st.nlist_capacity)))
        ctx.close()
    a, b = runs
    assert a[0] == b[0]
    for f in a[1]:
        assert np.array_equal(a[1][f], b[1][f]), f
    assert a[2:] == b[2:]
