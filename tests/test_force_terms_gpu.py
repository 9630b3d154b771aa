"""GPU: sph_force_terms (csrc/terms.hip: force_terms_kernel, force_terms_v_kernel and the gravity walk into scratch), the
rates of sph_forces split by physical term, on the sets of tests/force_terms_sets.py (their construction conditions are
asserted in tests/test_force_terms_cpu.py).

Parity is per row and per element against the brute-force restatement tests/force_terms_ref.py, at the project's bar for
rates (varh_ref.rate_excess): 1e-11 of the element's magnitude plus 1e-13 of the ROW'S OWN scale sum_j |term_j|.  The
recomposition (rows summed = the fields sph_forces wrote) uses the same bar with the summed scales; the per-term identities
(momentum, angular momentum and energy of the pressure and of the viscous term separately) are bounded by 1e-12 of
sum_i m_i scale_i of the rows involved, each scale carried through the products the identity forms (|r| scale for a torque,
|v| scale for a power).  The gravity rows are compared with the oracle's octree walk at rel_err <= 1e-13.  No bar here comes
from a GPU result.  Every test prints the largest share of its bar that was used.

Measured on the MI355X (80 tests, 6 s): rows of the fixed-h sets <= 2.5e-2 of their bar under every flag set, of the variable-h
sets <= 8.3e-3 (re-flagged list: 4.8e-3); recomposition <= 1.8e-3; the identities <= 3.2e-6 of theirs; the self-gravity rows
1.3e-15 against the oracle's walk."""
import ctypes as C

import numpy as np
import pytest

import force_terms_ref as FR
import force_terms_sets as TS
import varh_ref as VR
from conftest import rel_err
from gpu_support import capi

pytestmark = pytest.mark.gpu

SPH_ERR_ARG, SPH_ERR_STATE = 1, 5
RATES = ("ax", "ay", "az", "du", "dalpha")
STATE = "x y z vx vy vz u alpha".split()
PAIR_ROWS = list(range(0, 9)) + [12, 13, 14, 15]          # every row the restatement states (9-11: the gravity term)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def fixed_flags(capi, flagset):
    return {"default": 0, "no_lds_tiles": capi.FLAG_NO_LDS_TILES, "no_whole_tile": capi.FLAG_NO_WHOLE_TILE,
            "hashed": capi.FLAG_HASHED_GRID}[flagset]


def fixed_ctx(capi, gas, sinks, flags=0):
    ctx = capi.Context(device=0, flags=flags)
    ctx.upload(gas); ctx.set_sinks(sinks)
    return ctx


def variable_ctx(capi, gas, sinks, flags=0):
    ctx = capi.Context(device=0, variable=True, flags=capi.FLAG_VARIABLE_H | flags)
    ctx.upload(gas)
    if sinks is not None:
        ctx.set_sinks(sinks)
    return ctx


def check_rows(tag, rows, ref, which=PAIR_ROWS):
    ex = FR.excess(rows, ref, which)
    print(f"{tag}: largest share of the row bars used: " + " ".join(f"{k}:{v:.1e}" for k, v in ex.items() if v > 0.0))
    for k, v in ex.items():
        assert v <= 1.0, (tag, k, v)
    return max(ex.values())


def check_no_gravity_rows(rows):
    g = rows[FR.A_G]
    assert np.all(g == 0.0) and not np.any(np.signbit(g))          # +0.0 without self-gravity


def check_recomposition(tag, rows, fields, ref, grav_scale=None):
    """rows 0-11 per axis = ax..az, 12 + 13 = du, 14 + 15 = dalpha, against the summed scales"""
    _, scales = ref.recomposed()
    if grav_scale is not None:
        scales = [scales[k] + grav_scale[k] for k in range(3)] + scales[3:]
    r = rows.astype(np.longdouble)
    got = [(r[k] + r[3 + k] + r[6 + k] + r[9 + k]).astype(np.float64) for k in range(3)] + \
          [(r[12] + r[13]).astype(np.float64), (r[14] + r[15]).astype(np.float64)]
    worst = {}
    for f, g, s in zip(RATES, got, scales):
        worst[f] = float(np.max(VR.rate_excess(np.abs(g - fields[f]), np.abs(fields[f]), s)))
    print(f"{tag}: recomposition, share of the bar used: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for f, v in worst.items():
        assert v <= 1.0, (tag, f, v)


# ---- parity, fixed h ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flagset", ["default", "no_lds_tiles", "no_whole_tile", "hashed"])
@pytest.mark.parametrize("name", TS.FIXED)
def test_fixed_rows_vs_restatement(capi, name, flagset):
    gas, sinks, ref = TS.fixed_case(name)
    ctx = fixed_ctx(capi, gas, sinks, fixed_flags(capi, flagset))
    ctx.density()
    rows = ctx.force_terms()
    assert rows.shape == (16, ref.n)
    check_rows(f"{name}/{flagset}", rows, ref)
    check_no_gravity_rows(rows)
    if flagset == "hashed":
        assert ctx.grid_info().kind == 1
    if name == "far_clump_fixed":
        assert ctx.stats().nlist_capacity > TS.INIT_LIST_SLOTS           # the list grew
    if name in ("isolated", "n1"):
        lone = int(np.flatnonzero(ref.list_len == 0)[0])
        for k in list(range(0, 6)) + [12, 13, 14]:
            assert rows[k][lone] == 0.0, k                                # sink gravity (and the alpha decay) only
    ctx.close()


# ---- parity, variable h --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flagset", ["default", "no_reflag"])
@pytest.mark.parametrize("name", TS.VARIABLE)
def test_variable_rows_vs_restatement(capi, name, flagset):
    gas, sinks, vref, ref = TS.variable_case(name)
    ctx = variable_ctx(capi, gas, sinks, capi.FLAG_NO_REFLAG if flagset == "no_reflag" else 0)
    ctx.density()
    rows = ctx.force_terms()
    check_rows(f"{name}/{flagset}", rows, ref)
    check_no_gravity_rows(rows)
    ctx.close()


@pytest.mark.parametrize("flagset", ["default", "no_reflag"])
def test_variable_rows_on_a_reflagged_list(capi, flagset):
    """the list re-flagged in place after calc_smoothing (entries lose and gain their D / F flags) against the restatement
    evaluated with the lengths the context holds; SPH_FLAG_NO_REFLAG builds the list anew instead"""
    gas, sinks, _, _ = TS.variable_case("discv3000")
    ctx = variable_ctx(capi, gas, sinks, capi.FLAG_NO_REFLAG if flagset == "no_reflag" else 0)
    for it in range(10):       # the IC's h relaxes; evaluations alternate between building and re-flagging: stop after a build
        r0 = ctx.stats().nlist_reflags
        ctx.density(); ctx.forces()
        built = ctx.stats().nlist_reflags == r0
        ctx.update_h()
        if built and it >= 4:
            break
    before = ctx.stats().nlist_reflags
    ctx.density()
    assert ctx.stats().nlist_reflags == before + (1 if flagset == "default" else 0)
    rows = ctx.force_terms()
    now = dict(gas); now["h"] = ctx.field("h")
    _, ref = TS.variable_ref(now, sinks, "reference")
    check_rows(f"discv3000 after update_h/{flagset}", rows, ref)
    ctx.close()


# ---- recomposition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flagset", ["default", "no_lds_tiles", "no_whole_tile", "hashed"])
def test_fixed_rows_recompose_to_the_fields_and_leave_them_alone(capi, flagset):
    gas, sinks, ref = TS.fixed_case("disc2")
    ctx = fixed_ctx(capi, gas, sinks, fixed_flags(capi, flagset))
    ctx.density(); ctx.forces()
    before = {f: ctx.field(f) for f in RATES + ("rho", "P", "c")}
    rows = ctx.force_terms()
    after = {f: ctx.field(f) for f in before}
    for f in before:
        assert np.array_equal(before[f], after[f]), f
    check_recomposition(f"disc2/{flagset}", rows, before, ref)
    ctx.close()


def test_variable_rows_recompose_to_the_fields_and_leave_them_alone(capi):
    gas, sinks, _, ref = TS.variable_case("discv3000")
    ctx = variable_ctx(capi, gas, sinks)
    ctx.density(); ctx.forces()
    before = {f: ctx.field(f) for f in RATES + ("rho", "omega", "P", "c", "h")}
    rows = ctx.force_terms()
    for f in before:
        assert np.array_equal(before[f], ctx.field(f)), f
    check_recomposition("discv3000", rows, before, ref)
    ctx.close()


# ---- identities of the single terms (fixed h, no ghosts) -----------------------------------------------------------------------
def test_pressure_and_viscosity_conserve_separately(capi):
    gas, sinks, ref = TS.fixed_case("disc1")
    ctx = fixed_ctx(capi, gas, sinks)
    ctx.density()
    rows = ctx.force_terms().astype(np.longdouble)
    ctx.close()
    m = gas["m"].astype(np.longdouble)
    pos = [gas[k].astype(np.longdouble) for k in "xyz"]
    vel = [gas[k].astype(np.longdouble) for k in ("vx", "vy", "vz")]
    sc = ref.scale
    shares = {}
    for tag, a0, du in (("P", 0, FR.DU_P), ("V", 3, FR.DU_V)):
        a = [rows[a0 + k] for k in range(3)]
        s = [sc[a0 + k] for k in range(3)]
        for k in range(3):
            shares[f"sum m a_{tag}[{k}]"] = float(abs(np.sum(m * a[k])) / (1e-12 * np.sum(m * s[k])))
            i, j = (k + 1) % 3, (k + 2) % 3
            tq = np.sum(m * (pos[i] * a[j] - pos[j] * a[i]))
            shares[f"sum m r x a_{tag}[{k}]"] = float(abs(tq) / (1e-12 * np.sum(m * (np.abs(pos[i]) * s[j] + np.abs(pos[j]) * s[i]))))
        e = np.sum(m * (vel[0] * a[0] + vel[1] * a[1] + vel[2] * a[2] + rows[du]))
        bar = 1e-12 * np.sum(m * (np.abs(vel[0]) * s[0] + np.abs(vel[1]) * s[1] + np.abs(vel[2]) * s[2] + sc[du]))
        shares[f"sum m (v.a_{tag} + du_{tag})"] = float(abs(e) / bar)
    print("identities, share of the bar used: " + " ".join(f"{k}: {v:.1e}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v <= 1.0, (k, v)
    assert np.all(rows[FR.DU_V] >= 0.0) and np.any(rows[FR.DU_V] > 0.0)        # every pair term of the heating is >= 0
    assert np.all(rows[FR.AL_SRC] >= 0.0)


# ---- self-gravity --------------------------------------------------------------------------------------------------------------
def _heavy_disc():
    from summersph_amd import ic
    gas, sinks = ic.split_rows(ic.keplerian_disc(2000, seed=17, m_disc=0.5))
    gas = {k: np.array(v, dtype=np.float64) for k, v in gas.items()}
    rng = np.random.default_rng(18)
    gas["alpha"] = rng.uniform(0.05, 1.0, 2000)
    for k in ("vx", "vy", "vz"):
        gas[k] = gas[k] + rng.normal(0.0, 0.02, 2000)
    return gas, sinks


def _oracle_gravity(gas, h_var=None):
    from oracle import orc, orc_grav
    t = orc_grav.Tree(gas["x"], gas["y"], gas["z"], gas["m"])
    ga = [np.zeros(gas["x"].size) for _ in range(3)]
    orc_grav.gravity(t, gas["x"], gas["y"], gas["z"], *ga, h_var=h_var, nq=2500 if h_var is not None else 5000,
                     nthreads=orc.max_threads())
    return ga


def test_self_gravity_rows_fixed_h(capi):
    gas, sinks = _heavy_disc()
    ref = FR.fixed_terms(gas, sinks)
    ga = _oracle_gravity(gas)
    ctx = fixed_ctx(capi, gas, sinks, capi.FLAG_SELF_GRAVITY)
    ctx.density()
    rows0 = ctx.force_terms()                       # before any sph_forces: builds the tree sph_forces would build
    ctx.forces()
    before = {f: ctx.field(f) for f in RATES}
    rows = ctx.force_terms()
    assert np.array_equal(rows0, rows)
    for f in RATES:
        assert np.array_equal(before[f], ctx.field(f)), f          # SPH_F_AX..AZ untouched: the walk wrote to scratch
    errs = [rel_err(rows[9 + k], ga[k]) for k in range(3)]
    print("self-gravity rows vs the oracle's octree walk, rel_err: " + " ".join(f"{e:.2e}" for e in errs) + " (bar 1e-13)")
    check_rows("heavy disc", rows, ref)
    check_recomposition("heavy disc", rows, before, ref, grav_scale=[np.abs(g) for g in ga])
    skipped = ctx.force_terms(skip_gas_gravity=True)
    assert np.all(np.isnan(skipped[FR.A_G]))
    keep = [k for k in range(16) if not 9 <= k <= 11]
    assert np.array_equal(skipped[keep], rows[keep])
    ctx.close()
    for k in range(3):
        assert errs[k] <= 1e-13, (k, errs[k])


def test_self_gravity_rows_recompose_with_variable_h(capi):
    gas, sinks, _, ref = TS.variable_case("discv3000")
    ga = _oracle_gravity(gas, h_var=np.ascontiguousarray(gas["h"], dtype=np.float64))
    ctx = variable_ctx(capi, gas, sinks, capi.FLAG_SELF_GRAVITY)
    ctx.density(); ctx.forces()
    before = {f: ctx.field(f) for f in RATES}
    rows = ctx.force_terms()
    for f in RATES:
        assert np.array_equal(before[f], ctx.field(f)), f
    check_rows("discv3000 + gravity", rows, ref)
    check_recomposition("discv3000 + gravity", rows, before, ref, grav_scale=[np.abs(g) for g in ga])
    ctx.close()


# ---- ghosts ----------------------------------------------------------------------------------------------------------------------
def test_ghost_rows_are_nan_and_owned_rows_are_the_full_uploads(capi, torch):
    gas, sinks, ref = TS.fixed_case("disc1")
    n, n_own = ref.n, 1777
    full = fixed_ctx(capi, gas, sinks)
    full.density()
    rows_full = full.force_terms()
    rho = full.field("rho")
    full.close()
    ctx = fixed_ctx(capi, gas, sinks)
    ctx.set_owned(n_own)
    ctx.density()
    rho_g = torch.from_numpy(rho[None, n_own:].copy()).cuda()      # the ghosts' rho "as their owner sent it"
    torch.cuda.synchronize()
    ctx.scatter_fields_dev(["rho"], n_own, n - n_own, rho_g.data_ptr())
    ctx.refresh_eos()
    rows = ctx.force_terms()
    ctx.close()
    assert np.all(np.isnan(rows[:, n_own:]))
    assert np.all(np.isfinite(rows[:, :n_own]))
    sub = FR.TermRef(n_own)
    sub.rows, sub.scale = rows_full[:, :n_own], ref.scale[:, :n_own]
    check_rows("owned rows vs the full upload's", rows[:, :n_own], sub)
    owned = FR.TermRef(n_own)
    owned.rows, owned.scale = ref.rows[:, :n_own], ref.scale[:, :n_own]
    check_rows("owned rows vs the restatement", rows[:, :n_own], owned)


# ---- invariance and neutrality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fixed", "variable", "fixed_gravity"])
def test_forms_and_repeats_agree_bitwise(capi, torch, kind):
    if kind == "variable":
        gas, sinks, _, _ = TS.variable_case("discv3000")
        ctx = variable_ctx(capi, gas, sinks)
    else:
        gas, sinks, _ = TS.fixed_case("disc2")
        ctx = fixed_ctx(capi, gas, sinks, capi.FLAG_SELF_GRAVITY if kind == "fixed_gravity" else 0)
    ctx.density()
    a = ctx.force_terms()
    assert np.array_equal(a, ctx.force_terms(), equal_nan=True)                       # repeated
    dev = ctx.force_terms(device=True)
    assert dev.shape == (16, ctx.n) and dev.dtype == torch.float64
    assert np.array_equal(a, dev.cpu().numpy(), equal_nan=True)                       # host and device forms
    ctx.forces()
    assert np.array_equal(a, ctx.force_terms(), equal_nan=True)                       # after an intervening sph_forces
    ctx.forces()
    assert np.array_equal(a, ctx.force_terms(refresh=True), equal_nan=True)           # refresh: the same records again
    ctx.close()


@pytest.mark.parametrize("kind", ["fixed", "fixed_gravity", "variable"])
def test_a_run_with_the_call_between_steps_is_bitwise_the_run_without(capi, kind):
    runs = []
    for with_terms in (False, True):
        if kind == "variable":
            gas, sinks, _, _ = TS.variable_case("discv3000")
            ctx = variable_ctx(capi, gas, sinks)
        else:
            gas, sinks, _ = TS.fixed_case("disc1")
            ctx = fixed_ctx(capi, gas, sinks, capi.FLAG_SELF_GRAVITY if kind == "fixed_gravity" else 0)
        dts, t = [1e-2], 0.0
        for _ in range(6):
            dt, t = ctx.step(dts[-1], t)
            dts.append(dt)
            ctx.density()
            if with_terms:
                rows = ctx.force_terms()
                assert np.all(np.isfinite(rows))
        out = {f: ctx.field(f) for f in STATE + (["h"] if kind == "variable" else [])}
        out["dts"] = np.array(dts)
        out["sinks"] = np.stack([ctx.get_sinks()[k] for k in "x y z vx vy vz m".split()])
        runs.append(out)
        ctx.close()
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f


@pytest.mark.parametrize("kind", ["fixed", "fixed_gravity", "variable"])
def test_statistics_do_not_move(capi, kind):
    if kind == "variable":
        gas, sinks, _, _ = TS.variable_case("discv3000")
        ctx = variable_ctx(capi, gas, sinks)
    else:
        gas, sinks, _ = TS.fixed_case("disc1")
        ctx = fixed_ctx(capi, gas, sinks, capi.FLAG_SELF_GRAVITY if kind == "fixed_gravity" else 0)
    ctx.density(); ctx.forces()
    s0, dt0 = ctx.stats(), ctx.get_dt()
    ctx.force_terms(); ctx.force_terms(skip_gas_gravity=True); ctx.force_terms(device=True)
    s1 = ctx.stats()
    for f, _ in capi.Stats._fields_:
        if f != "device_bytes":
            a, b = getattr(s0, f), getattr(s1, f)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    assert ctx.get_dt() == dt0
    ctx.kick(1e-3)                                   # the rates are still valid: the call did not clear them
    ctx.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(capi):
    gas, sinks, ref = TS.fixed_case("n65")
    ctx = fixed_ctx(capi, gas, sinks)
    ctx.density()
    n = ctx.n
    out = np.full((16, n), 7.0)
    call = ctx.lib.sph_force_terms

    def desc(flags=0, reserved=(0, 0, 0)):
        d = capi.ForceTermsDesc()
        d.flags = flags
        d.reserved[:] = reserved
        return d
    assert call(ctx._h, None, out.ctypes.data, 16 * n) == SPH_ERR_ARG                        # null descriptor
    assert call(ctx._h, C.byref(desc()), None, 16 * n) == SPH_ERR_ARG                        # null output
    assert ctx.lib.sph_force_terms_dev(ctx._h, C.byref(desc()), None, 16 * n) == SPH_ERR_ARG
    for bad in (16 * n - 1, 16 * n + 1, n, 0, -1):
        assert call(ctx._h, C.byref(desc()), out.ctypes.data, bad) == SPH_ERR_ARG, bad       # wrong n_out
    for flags in (2, 4, 1 << 30, -1):
        assert call(ctx._h, C.byref(desc(flags)), out.ctypes.data, 16 * n) == SPH_ERR_ARG, flags
    for k in range(3):
        r = [0, 0, 0]; r[k] = 1
        assert call(ctx._h, C.byref(desc(0, r)), out.ctypes.data, 16 * n) == SPH_ERR_ARG, k  # reserved != 0
    assert call(None, C.byref(desc()), out.ctypes.data, 16 * n) == SPH_ERR_ARG
    assert np.all(out == 7.0)
    assert call(ctx._h, C.byref(desc(1)), out.ctypes.data, 16 * n) == 0                       # the known flag is accepted
    assert np.all(np.isnan(out[9:12])) and np.all(np.isfinite(out[:9]))
    ctx.close()


@pytest.mark.parametrize("variable", [False, True])
def test_state_errors(capi, variable):
    if variable:
        gas, sinks, _, _ = TS.variable_case("discv3000")
        ctx = variable_ctx(capi, gas, sinks)
    else:
        gas, sinks, _ = TS.fixed_case("n65")
        ctx = fixed_ctx(capi, gas, sinks)

    def refused():
        with pytest.raises(capi.SphError) as e:
            ctx.force_terms()
        assert e.value.status == SPH_ERR_STATE and "call sph_density first" in str(e.value)
    refused()                                        # directly after an upload
    ctx.density()
    ctx.force_terms()
    ctx.forces()
    ctx.kick(1e-3)
    refused()                                        # after a kick: the records are stale
    ctx.density()
    ctx.force_terms()
    ctx.drift(1e-3)
    refused()                                        # after a drift: the list is stale
    ctx.density(); ctx.forces()
    ctx.step(1e-3)
    refused()                                        # after a step: its closing kick
    assert np.all(np.isfinite(ctx.force_terms(refresh=True)))
    ctx.close()


def test_empty_context(capi):
    ctx = capi.Context(device=0)
    assert ctx.n == 0
    d = capi.ForceTermsDesc()
    assert ctx.lib.sph_force_terms(ctx._h, C.byref(d), None, 0) == 0
    assert ctx.lib.sph_force_terms_dev(ctx._h, C.byref(d), None, 0) == 0
    assert ctx.lib.sph_force_terms(ctx._h, C.byref(d), None, 16) == SPH_ERR_ARG
    assert ctx.force_terms().shape == (16, 0)
    ctx.close()
