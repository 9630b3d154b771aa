"""GPU tests of sph_bound (include/summersph.h, "binding energies and unbinding of clumps") on the MI355X: parity of the
labels, e, Phi, the table and the counts with the numpy restatement on twelve blobs of 1 .. 3000 members (cold, hot, a
cold core in a hot halo; coincident and massless members, labels in no group, ghosts) on a fixed-h and a variable-h
context, the descriptor's switches, the order rule bit for bit, friends-of-friends feeding the call, no side effects on a
running simulation, the argument errors and the command line.

Tolerances (derived, not measured): a same-sign chain of N <= 3000 terms is off by at most N 2^-53 = 3.3e-13 of its sum and
a term carries a few tens of ulp through phi's middle piece, hence Phi_i to 1e-12 |Phi_i|, e_i to 1e-12 (k_i + f u_i +
|Phi_i|), every table sum to 1e-12 of the sum of its terms' absolute values, R_R and V_R to 1e-12 of sum m |.| / M.  Labels,
counts, the N columns, R, status and the most bound id are exact: the restatement asserts that no e_i of the set lies within
1e-9 of zero."""
import ctypes as C
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import bound_ref
from gpu_support import capi, make_context
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPH_ERR_ARG = 1
SPH_ERR_STATE = 5
H_FIXED = 0.3
FIELDS = "x y z vx vy vz u m".split()


@functools.lru_cache(maxsize=None)
def _blobs():
    from summersph_amd import capi
    G = float(capi.default_params().G)
    return (G,) + bound_ref.blob_set(G)


@functools.lru_cache(maxsize=None)
def _ref(variable, kw):
    """the restatement on the blob set, computed once per descriptor and shared"""
    G, gas, _, lab, no, ng = _blobs()
    return bound_ref.bound(gas, lab, no, ng, G, gas["h"] if variable else H_FIXED, **dict(kw))


def _ctx(capi, gas, sinks, n_owned, variable=False, flags=0):
    return make_context(capi, gas, sinks, variable=variable, flags=flags, n_owned=None if n_owned == gas["x"].size else n_owned,
                        **({} if variable else {"h": H_FIXED}))


def _blob_ctx(capi, variable=False, flags=0):
    _, gas, sinks, lab, no, ng = _blobs()
    return _ctx(capi, gas, sinks, no, variable, flags), lab, ng


def _raw(res):
    bl, e, phi, tab, cnt = res
    return bl.copy(), e.copy(), phi.copy(), np.ascontiguousarray(tab).view(np.float64).reshape(-1, 24).copy(), tuple(cnt)


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    for k in (1, 2, 3):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a[4] == b[4]


def _close(got, want, scale, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    lim = TOL * scale[ok]
    worst = float(np.max(err / np.where(lim > 0, lim, 1.0), initial=0.0))
    print(f"{what}: max error / bound = {worst:.3g}")
    assert np.all(err <= lim), (what, worst)


def _cmp(got, ref, what=""):
    bl, e, phi, tab, cnt = _raw(got)
    rbl, re_, rphi, rtab, rcnt, info = ref
    assert list(cnt) == [int(c) for c in rcnt], what
    assert np.array_equal(bl, rbl), what
    _close(phi, rphi, np.abs(rphi), what + " Phi")
    _close(e, re_, info["e_scale"], what + " e")
    for c, name in enumerate(bound_ref.COLUMNS):
        g, w = tab[:, c].copy(), rtab[:, c].copy()
        if name in bound_ref.EXACT:
            assert np.array_equal(g, w, equal_nan=True), (what, name, g, w)
            continue
        if name == "virial0":                       # (K + f U) / |W| with W == 0 (a set of one): no number to compare
            lone = rtab[:, 4] == 0.0
            assert not np.any(np.isfinite(g[lone]))
            g[lone] = w[lone] = np.nan
        _close(g, w, info["scale"][:, c], what + " " + name)


# ---- parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variable", [False, True], ids=["fixed_h", "variable_h"])
def test_parity_blobs(capi, variable):
    ctx, lab, ng = _blob_ctx(capi, variable)
    ref = _ref(variable, (("max_rounds", 16),))
    got = ctx.bound(lab, ng, max_rounds=16)
    _cmp(got, ref, "rounds16")
    bl, e, phi, tab, cnt = got
    _, gas, _, _, no, _ = _blobs()
    kinds = np.array(bound_ref.KINDS)
    assert tab["N0"].tolist() == [float(s) for s in bound_ref.SIZES] and cnt[0] == sum(bound_ref.SIZES)
    assert np.max(tab["rounds"][kinds == "halo"]) >= 3 and np.all(tab["status"][kinds == "hot"] == 2)
    assert np.all(tab["status"][2:][kinds[2:] == "cold"] == 0) and np.all(tab["rounds"][kinds == "cold"] == 0)
    assert np.all(bl[no:] == -1) and np.all(np.isnan(e[no:])) and np.all(np.isnan(phi[no:]))      # ghosts
    out = (lab < 0) | (lab >= ng)
    assert np.all(bl[out] == -1) and np.all(np.isnan(e[out]))
    removed = (lab >= 0) & (lab < ng) & (np.arange(lab.size) < no) & (bl == -1)
    assert np.all(e[removed] >= 0)                           # a removed member keeps the e that removed it
    ctx.close()


def test_parity_coincident_members_without_softening(capi):
    ctx, lab, ng = _blob_ctx(capi)
    got = ctx.bound(lab, ng, max_rounds=16, soft2=0.0)
    _cmp(got, _ref(False, (("max_rounds", 16), ("soft2", 0.0))), "soft2=0")
    _, gas, _, _, no, _ = _blobs()
    mem = bound_ref.members(gas, lab, no, ng)[bound_ref.COINCIDENT_GROUP]
    pos = np.stack([gas[k][mem] for k in "xyz"], axis=1)
    assert np.unique(pos, axis=0).shape[0] == mem.size - 1 and np.all(np.isfinite(got[2][mem]))
    ctx.close()


def test_descriptor_switches(capi):
    ctx, lab, ng = _blob_ctx(capi)
    kinds = np.array(bound_ref.KINDS)
    # no removal allowed: one evaluation, column 19 counts the e < 0 members of S_0
    got = ctx.bound(lab, ng)
    _cmp(got, _ref(False, ()), "rounds0")
    t = got[3]
    assert np.all(t["rounds"] == 0) and np.all(t["N"] == t["N0"]) and np.all(np.isin(t["status"], (0, 1)))
    assert np.all(t["n_bound"][kinds == "halo"] < t["N0"][kinds == "halo"]) and np.all(t["n_bound"][kinds == "halo"] > 0)
    assert [int(np.sum(got[0] == g)) for g in range(ng)] == t["n_bound"].astype(int).tolist()
    # one removal on the core + halo groups: stopped at max_rounds
    got = ctx.bound(lab, ng, max_rounds=1)
    _cmp(got, _ref(False, (("max_rounds", 1),)), "rounds1")
    assert np.all(got[3]["status"][kinds == "halo"] == 1) and np.all(got[3]["rounds"][kinds == "halo"] == 1)
    assert got[4][3] == int(np.sum(got[3]["status"] == 1)) >= 4
    # the cost cap skips exactly the groups of 1025 and 3000 members
    got = ctx.bound(lab, ng, max_rounds=16, max_members=1024)
    _cmp(got, _ref(False, (("max_rounds", 16), ("max_members", 1024))), "cap1024")
    t = got[3]
    assert got[4][1] == 2 and t["status"][10] == 3 and t["status"][11] == 3 and np.all(t["status"][:10] != 3)
    raw = _raw(got)[3]
    assert np.all(np.isnan(raw[10:, 1:21])) and np.all(np.isnan(raw[10:, 22:])) and raw[10:, 0].tolist() == [1025.0, 3000.0]
    assert np.all(got[0][(lab == 10) | (lab == 11)] == -1) and np.all(np.isnan(got[1][(lab == 10) | (lab == 11)]))
    # min_members dissolves what falls below it
    got = ctx.bound(lab, ng, max_rounds=16, min_members=30)
    ref = _ref(False, (("max_rounds", 16), ("min_members", 30)))
    _cmp(got, ref, "min30")
    assert got[3]["status"][0] == 2 and got[3]["status"][1] == 2 and got[4][2] == int(np.sum(got[3]["status"] == 2)) >= 5
    ctx.close()


def test_thermal_energy_unbinds_a_cold_clump(capi):
    G, gas, sinks, lab, no, ng = _blobs()
    hot = dict(gas)
    hot["u"] = np.full(gas["u"].size, 5.0)
    ctx = _ctx(capi, hot, sinks, no)
    cold = ctx.bound(lab, ng, max_rounds=4)
    got = ctx.bound(lab, ng, max_rounds=4, thermal=True)
    _cmp(got, bound_ref.bound(hot, lab, no, ng, G, H_FIXED, max_rounds=4, thermal=True), "thermal")
    assert cold[3]["status"][8] == 0 and cold[3]["n_bound"][8] == 1023
    mem8 = (lab == 8) & (np.arange(lab.size) < no)
    assert got[3]["status"][8] == 2 and np.all(got[0] == -1) and np.all(got[1][mem8] > 0) and np.all(cold[1][mem8] < 0)
    assert got[3]["U0"][8] > 0 and got[3]["E0"][8] > 0 > cold[3]["E0"][8]
    ctx.close()


# ---- the order rule --------------------------------------------------------------------------------------------------------
def test_bitwise_invariance(capi):
    import torch
    G, gas, sinks, lab, no, ng = _blobs()
    kw = dict(max_rounds=16)
    ctx, _, _ = _blob_ctx(capi)
    a = _raw(ctx.bound(lab, ng, **kw))
    _same(a, _raw(ctx.bound(lab, ng, **kw)))                               # a repeated call
    # the device form
    dl = torch.from_numpy(lab).to("cuda:0")
    dev = ctx.bound(dl, ng, device=True, **kw)
    assert all(isinstance(t, torch.Tensor) for t in dev[:4])
    _same(a, (dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2].cpu().numpy(), dev[3].cpu().numpy(), dev[4]))
    # the slots re-sorted by a density pass
    ctx.density()
    _same(a, _raw(ctx.bound(lab, ng, **kw)))
    # one group alone: its row and its members' values
    for g in (4, 9):
        only = np.where(lab == g, lab, -1).astype(np.int32)
        b = _raw(ctx.bound(only, ng, **kw))
        mem = (lab == g) & (np.arange(lab.size) < no)
        assert np.array_equal(b[3][g], a[3][g], equal_nan=True)
        assert np.array_equal(b[0][mem], a[0][mem]) and np.array_equal(b[1][mem], a[1][mem]) and np.array_equal(b[2][mem], a[2][mem])
        assert np.all(b[0][~mem] == -1) and np.all(np.isnan(b[1][~mem])) and b[4][0] == bound_ref.SIZES[g]
        assert np.all(b[3][np.arange(ng) != g, 21] == 2) and np.all(b[3][np.arange(ng) != g, 0] == 0)
    ctx.close()
    # a hashed grid
    hctx, _, _ = _blob_ctx(capi, flags=capi.FLAG_HASHED_GRID)
    hctx.density()
    assert hctx.grid_info().kind == 1
    _same(a, _raw(hctx.bound(lab, ng, **kw)))
    hctx.close()
    # a permuted upload, labels permuted with it.  A group's sums run over its members in ascending id, so the permutation
    # moves every group to other ids (and other slots) but keeps the order of the ids within a group.
    rng = np.random.default_rng(23)
    perm = rng.permutation(no)
    for g in range(ng):
        at = np.nonzero(lab[perm] == g)[0]
        perm[at] = np.sort(perm[at])
    perm = np.concatenate([perm, np.arange(no, lab.size)])
    pg = {k: v[perm] for k, v in gas.items()}
    pctx = _ctx(capi, pg, sinks, no)
    p = _raw(pctx.bound(lab[perm], ng, **kw))
    assert np.array_equal(p[0], a[0][perm]) and p[4] == a[4]
    assert np.array_equal(p[1], a[1][perm], equal_nan=True) and np.array_equal(p[2], a[2][perm], equal_nan=True)
    cols = [c for c in range(24) if c != 22]
    assert np.array_equal(p[3][:, cols], a[3][:, cols], equal_nan=True)
    has = a[3][:, 22] >= 0
    assert np.array_equal(perm[p[3][has, 22].astype(int)], a[3][has, 22].astype(int)) and np.all(p[3][~has, 22] == -1)
    pctx.close()


def test_variable_h_device_form_and_bad_h(capi):
    import torch
    G, gas, sinks, lab, no, ng = _blobs()
    ctx, _, _ = _blob_ctx(capi, variable=True)
    a = _raw(ctx.bound(lab, ng, max_rounds=16))
    dev = ctx.bound(torch.from_numpy(lab).to("cuda:0"), ng, max_rounds=16, device=True)
    _same(a, tuple(t.cpu().numpy() for t in dev[:4]) + (dev[4],))
    # one softening length for every member instead of each particle's own: the fixed-h context's numbers
    one = _raw(ctx.bound(lab, ng, max_rounds=16, h=H_FIXED))
    fctx, _, _ = _blob_ctx(capi)
    _same(one, _raw(fctx.bound(lab, ng, max_rounds=16)))
    fctx.close()
    # a member whose own h cannot be used
    victim = int(bound_ref.members(gas, lab, no, ng)[7][5])
    h = gas["h"].copy()
    h[victim] = -1.0
    ctx.upload_field("h", h)
    with pytest.raises(capi.SphError) as err:
        ctx.bound(lab, ng)
    assert err.value.status == SPH_ERR_STATE
    dev = ctx.bound(torch.from_numpy(lab).to("cuda:0"), ng, device=True)
    assert dev[4][0] == -1 and bool(torch.all(dev[0] == -1)) and bool(torch.all(torch.isnan(dev[3])))
    assert bool(torch.all(torch.isnan(dev[1])))
    ok = lab.copy()
    ok[victim] = -1                                          # no member any more: its h does not matter
    assert ctx.bound(ok, ng)[4][0] == sum(bound_ref.SIZES) - 1
    assert ctx.bound(lab, ng, h=H_FIXED)[4][0] == sum(bound_ref.SIZES)
    ctx.close()


# ---- end to end, side effects, errors, command line --------------------------------------------------------------------------
def _two_clumps(G, seed=3, per=300):
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.normal(0, 0.3, (per, 3)), rng.normal(0, 0.3, (per, 3)) + [20.0, 0, 0],
                          rng.uniform(-40, 40, (400, 3)) * [1, 1, 0.1]])
    n = pos.shape[0]
    v0 = np.sqrt(G * 0.01 / 0.3)
    vel = rng.normal(0, 0.2 * v0, (n, 3))
    vel[per:2 * per] = rng.normal(0, 0.5 * v0, (per, 3))       # the second clump is warm: it sheds members
    gas = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": vel[:, 0].copy(), "vy": vel[:, 1].copy(),
           "vz": vel[:, 2].copy(), "u": np.full(n, 1e-3), "m": np.full(n, 0.01 / per), "alpha": np.ones(n)}
    sinks = {k: np.zeros(1) for k in "x y z vx vy vz".split()}
    sinks["m"] = np.array([1e-6])
    sinks["z"] = np.array([50.0])
    return gas, sinks


def test_groups_feed_bound(capi):
    G = float(capi.default_params().G)
    gas, sinks = _two_clumps(G)
    ctx = _ctx(capi, gas, sinks, gas["x"].size)
    ctx.density()
    lab, gt, ng = ctx.groups(0.5, min_members=50)
    assert ng == 2 and np.all(gt["N"] >= 290)
    got = ctx.bound(lab, ng, max_rounds=8, min_members=50)
    f = {k: ctx.field(k) for k in FIELDS}
    _cmp(got, bound_ref.bound(f, lab, ctx.n, ng, G, H_FIXED, max_rounds=8, min_members=50), "fof")
    t = got[3]
    assert np.array_equal(t["N0"], gt["N"])                  # the two calls agree on what the groups are
    for a, b in (("M0", "M"), ("U0", "U"), ("K0", "K_int")):
        assert np.max(np.abs(t[a] - gt[b])) <= 1e-13 * np.max(gt[b]), a
    cold = int(np.bincount(lab[:300][lab[:300] >= 0]).argmax())
    warm = 1 - cold
    assert t["status"][cold] == 0 and t["rounds"][cold] == 0 and t["N"][cold] == t["N0"][cold]   # bound as it is
    assert t["rounds"][warm] >= 1 and t["N"][warm] < t["N0"][warm]                               # the warm one sheds members
    ctx.close()


def test_no_side_effects(capi):
    gas, sinks = ic.split_rows(ic.keplerian_disc(8000, seed=29))
    lab = (np.arange(8000) % 37).astype(np.int32)
    lab[::11] = -1
    runs = []
    for with_bound in (False, True):
        ctx = capi.Context(device=0)
        ctx.upload(gas)
        ctx.set_sinks(sinks)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(4):
            dt, t = ctx.step(dt, t)
            if with_bound:
                ctx.bound(lab, 37, max_rounds=3, thermal=True)
                ctx.bound(lab, 40, h=1.0, min_members=100)
            st = ctx.stats()
            statsl.append({f: (list(getattr(st, f)) if f == "grid_dim" else getattr(st, f)) for f, _ in st._fields_
                           if f != "device_bytes"})
        runs.append(({k: ctx.field(k) for k in ("x", "y", "z", "vx", "vy", "vz", "u", "alpha", "rho", "ax", "du")}, dt, t,
                     statsl, ctx.get_sinks()))
        ctx.close()
    (f0, dt0, t0, s0, k0), (f1, dt1, t1, s1, k1) = runs
    assert dt0 == dt1 and t0 == t1 and s0 == s1
    for k in f0:
        assert np.array_equal(f0[k], f1[k]), k
    for k in k0:
        assert np.array_equal(k0[k], k1[k]), k


def test_empty_cases(capi):
    _, gas, sinks, lab, no, ng = _blobs()
    ctx, _, _ = _blob_ctx(capi)
    n = ctx.n
    bl, e, phi, tab, cnt = ctx.bound(lab, 0)
    assert cnt == (0, 0, 0, 0) and len(tab) == 0 and np.all(bl == -1) and np.all(np.isnan(e)) and np.all(np.isnan(phi))
    bl, e, phi, tab, cnt = ctx.bound(np.full(n, -1, dtype=np.int32), 3, max_rounds=2)
    assert cnt == (0, 0, 3, 0) and np.all(bl == -1) and np.all(np.isnan(e))
    assert np.all(tab["N0"] == 0) and np.all(tab["status"] == 2) and np.all(tab["N"] == 0) and np.all(np.isnan(tab["K0"]))
    ctx.close()
    empty = capi.Context(device=0)
    bl, e, phi, tab, cnt = empty.bound(np.zeros(0, dtype=np.int32), 2)
    assert cnt == (0, 0, 2, 0) and bl.size == 0 and np.all(tab["status"] == 2)
    empty.close()


def test_errors(capi):
    ctx, lab, ng = _blob_ctx(capi)
    lib, n = ctx.lib, ctx.n
    bl = np.full(n, 77, dtype=np.int32)
    out = np.full(2 * n, 7.5)
    tab = np.full((ng, capi.BOUND_NCOL), 7.5)
    cnt = (C.c_int64 * 4)(9, 9, 9, 9)

    def call(d, labels=lab, nl=n, groups=ng, b=bl, o=out, no=2 * n, t=tab, c=cnt):
        return lib.sph_bound(ctx._h, None if d is None else C.byref(d), None if labels is None else labels.ctypes.data, nl, groups,
                             None if b is None else b.ctypes.data, None if o is None else o.ctypes.data, no,
                             None if t is None else t.ctypes.data, c)

    def desc(**kw):
        return capi.bound_desc(**kw)
    bad = {"null descriptor": dict(d=None), "null labels": dict(d=desc(), labels=None),
           "no output": dict(d=desc(), b=None, o=None, no=0, t=None, c=None), "n_labels": dict(d=desc(), nl=n - 1),
           "n_out": dict(d=desc(), no=2 * n - 1), "n_groups < 0": dict(d=desc(), groups=-1),
           "n_groups 2^31": dict(d=desc(), groups=2**31), "min_members": dict(d=desc(min_members=0)),
           "max_members": dict(d=desc(max_members=0)), "max_rounds": dict(d=desc(max_rounds=-1)), "h < 0": dict(d=desc(h=-1.0)),
           "h NaN": dict(d=desc(h=np.nan)), "soft2 < 0": dict(d=desc(soft2=-1e-3)), "soft2 NaN": dict(d=desc(soft2=np.nan))}
    d = desc(); d.flags = 2
    bad["flags"] = dict(d=d)
    d = desc(); d.reserved[1] = 1
    bad["reserved"] = dict(d=d)
    for what, kw in bad.items():
        assert call(**kw) == SPH_ERR_ARG, what
        assert b"sph_bound" in lib.sph_last_error(ctx._h), what
    assert np.all(bl == 77) and np.all(out == 7.5) and np.all(tab == 7.5) and list(cnt) == [9, 9, 9, 9]   # nothing written
    assert lib.sph_bound(None, C.byref(desc()), lab.ctypes.data, n, ng, bl.ctypes.data, None, 0, None, None) == SPH_ERR_ARG
    # every output alone is enough
    assert call(desc(), o=None, no=0, t=None, c=None) == 0 and np.all(bl[lab == 8][:1] == 8)
    assert call(desc(), b=None, t=None, c=None) == 0 and np.isfinite(out[np.nonzero(lab == 8)[0][0]])
    assert call(desc(), b=None, o=None, no=0, c=None) == 0 and tab[11, 0] == 3000
    assert call(desc(), b=None, o=None, no=0, t=None) == 0 and cnt[0] == sum(bound_ref.SIZES)
    with pytest.raises(ValueError):
        ctx.bound(lab, ng, device=True)                                 # host labels in the device form
    ctx.bound(lab, ng)                                                  # still usable
    ctx.close()


def test_cli_bound_matches_context_bound(capi, tmp_path):
    G = float(capi.default_params().G)
    gas, sinks = _two_clumps(G, seed=5)
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "g.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.groups", str(save), "-o", str(out), "--link", "0.5",
                        "--min-members", "50", "--json", "--bound", "--unbind", "8", "--bound-h", "0.3", "--thermal"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z = np.load(out)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = capi.Context(device=0)
    ctx.upload(g2)
    ctx.set_sinks(s2)
    ctx.density()
    lab, _, ng = ctx.groups(0.5, min_members=50)
    b = _raw(ctx.bound(lab, ng, h=0.3, thermal=True, max_rounds=8, min_members=50))
    assert int(z["n_groups"]) == ng == 2 and np.array_equal(z["labels"], lab)
    assert np.array_equal(z["bound_labels"], b[0]) and np.array_equal(z["e"], b[1], equal_nan=True)
    assert np.array_equal(z["phi"], b[2], equal_nan=True) and np.array_equal(z["bound_table"], b[3], equal_nan=True)
    assert tuple(z["bound_counts"].tolist()) == b[4]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["n_groups"] == 2 and j["bound"]["counts"]["members"] == 600 and j["bound"]["columns"] == capi.BOUND_COLUMNS
    assert len(j["bound"]["table"]) == 2
    # without --bound the output is what it was
    out2 = tmp_path / "g2.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.groups", str(save), "-o", str(out2), "--link", "0.5",
                        "--min-members", "50", "--json"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    z2 = np.load(out2)
    assert not any(k.startswith("bound") or k in ("e", "phi") for k in z2.files)
    assert "bound" not in json.loads(r.stdout.strip().splitlines()[-1])
    ctx.close()
