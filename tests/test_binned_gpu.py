"""GPU tests of sph_binned (include/summersph.h, "binned sums") on the MI355X: parity of the sums and the counts with the
numpy restatement (tests/binned_ref.py: one and two axes, linear, logarithmic and caller's edges, every weight, 0, 1 and 8
quantities, squares, fixed and variable h), the piece boundaries of the reduction on integer-valued sets (exact), the order
rule (bitwise across sorted orders, grids, calls and forms), the bitwise tie to sph_profile, the composition with
sph_force_terms_dev and sph_gradients_dev, the selection rule, no side effects on a running simulation, the argument errors
that need a context and the command line.

TOL is sph_profile's: 1e-12 relative on a column's scale; no bin here holds more than ~10^4 particles."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

import binned_ref
import profile_ref
from conftest import ROOT, rel_err
from gpu_support import capi, make_context
from summersph_amd import ic, txtio

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPH_ERR_ARG, SPH_ERR_STATE = 1, 5
STATE = "x y z vx vy vz u m alpha".split()


def _disc(n, seed, variable=False):
    rows = ic.keplerian_disc_var(n, seed=seed) if variable else ic.keplerian_disc(n, seed=seed)
    gas, sinks = ic.split_rows(rows)
    gas = dict(gas)
    rng = np.random.default_rng(seed + 1)
    gas["u"] = rng.uniform(0.1, 0.5, gas["x"].size)        # structure in every column
    gas["alpha"] = rng.uniform(0.0, 1.0, gas["x"].size)
    gas["vz"] = rng.normal(0.0, 0.05, gas["x"].size)
    gas["vx"] = gas["vx"] + rng.normal(0.0, 0.02, gas["x"].size)
    return gas, sinks


def _counts(c):
    """the device form leaves its counts on the device"""
    return tuple(int(v) for v in c.cpu().tolist())


def _tables(capi, ctx, tab):
    d = ctx.binned_desc
    return [capi.binned_edges(d, tab, a) for a in range(d.n_axes)]


def _value(capi, ctx, src, values):
    return values[-1 - src] if isinstance(src, (int, np.integer)) and src < 0 else ctx.field(src if isinstance(src, str) else capi.FIELDS[src])


def _check(capi, ctx, axes, bins, values=None, exact=False, owned=None, **kw):
    """one call against the restatement: counts exactly, sums to TOL on each column's scale (exact: bitwise)"""
    got, counts = ctx.binned(axes, bins, values=values, **kw)
    d = ctx.binned_desc
    tab = capi.binned_desc(axes, bins, kw.get("ranges"), kw.get("edges"), kw.get("log", ()), kw.get("q", ()), kw.get("weight", "mass"),
                           d.n_rows, kw.get("squares", False), kw.get("skip_nan", True))[1]
    tables = _tables(capi, ctx, tab)
    ax = [axes] if isinstance(axes, (str, int, np.integer)) else list(axes)
    q = kw.get("q", ())
    q = [q] if isinstance(q, (str, int, np.integer)) else list(q)
    weight = kw.get("weight", "mass")
    w = 1.0 if weight == "one" else ctx.field("m") if weight == "mass" else ctx.field("m") / ctx.field("rho")
    want, wc = binned_ref.binned_sums([_value(capi, ctx, s, values) for s in ax], tables, [_value(capi, ctx, s, values) for s in q], w,
                                      owned, kw.get("squares", False), kw.get("skip_nan", True))
    assert got.shape == want.shape
    assert counts == wc, (counts, wc)
    assert np.array_equal(got[..., 0], want[..., 0])                     # counts exactly
    assert got[..., 0].sum() == counts[0]
    for s in range(1, got.shape[-1]):
        g, w = got[..., s], want[..., s]
        if exact:
            assert np.array_equal(g, w, equal_nan=True), s
        else:
            assert np.array_equal(np.isnan(g), np.isnan(w)), s
            ok = ~np.isnan(w)
            err = rel_err(g[ok], w[ok])
            print(f"column {s}: {err:.2e}")
            assert err <= TOL, (s, err)
    return got, counts


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disc(capi):
    gas, sinks = _disc(20000, 5)
    ctx = make_context(capi, gas, sinks)
    ctx.density()
    R = np.sqrt(gas["x"] * gas["x"] + gas["y"] * gas["y"])
    yield ctx, gas, R
    ctx.close()


EIGHT = ("x", "y", "z", "vx", "vy", "vz", "alpha", "rho")


@pytest.mark.parametrize("weight", ["one", "mass", "volume"])
def test_parity_one_axis_linear(capi, disc, weight):
    ctx, gas, R = disc
    got, counts = _check(capi, ctx, "u", 16, ranges=(0.12, 0.47), q=("alpha",), weight=weight)
    assert counts[0] > 15000 and counts[1] > 1000 and counts[2] == 0


@pytest.mark.parametrize("q,squares", [((), False), ((), True), (("u",), True), (EIGHT, False), (EIGHT, True)])
def test_parity_one_axis_log_of_a_caller_row(capi, disc, q, squares):
    ctx, gas, R = disc
    got, counts = _check(capi, ctx, capi.binned_row(0), 12, values=R[None, :], ranges=(10.0, 60.0), log=(0,), q=q, squares=squares)
    assert got.shape == (12, 1, 2 + len(q) * (2 if squares else 1)) and counts[0] > 5000


@pytest.mark.parametrize("weight,q,squares", [("mass", ("alpha",), False), ("volume", EIGHT, True), ("one", (), False)])
def test_parity_two_axes(capi, disc, weight, q, squares):
    ctx, gas, R = disc
    rho = ctx.field("rho")
    got, counts = _check(capi, ctx, ("rho", "u"), (32, 24), ranges=((float(rho.min()), float(rho.max())), (0.1, 0.5)), log=(0,),
                         q=q, weight=weight, squares=squares)
    assert counts[1] >= 1 and (got[..., 0] > 0).sum() > 100              # the densest particle sits on the last edge: outside


def test_parity_variable_h(capi):
    gas, sinks = _disc(6000, 9, variable=True)
    ctx = make_context(capi, gas, sinks, variable=True)
    h = gas["h"]
    _check(capi, ctx, "h", 10, ranges=(float(h.min()), float(np.nextafter(h.max(), np.inf))), q=("u", "h"), squares=True)
    ctx.density()
    got, counts = _check(capi, ctx, ("h", "rho"), (6, 5), ranges=((float(h.min()), float(h.max()) * 1.01), (1e-12, 1.0)), log=(0, 1),
                         q=("omega", "c", "P"), weight="volume", squares=True)
    assert counts[0] > 3000
    ctx.close()


# ---- the piece boundaries of the reduction -----------------------------------------------------------------------------------
POPULATIONS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)


@pytest.fixture(scope="module")
def integer_set(capi):
    n = sum(POPULATIONS)
    gas, sinks = _disc(n, 43)
    assert gas["x"].size == n
    rng = np.random.default_rng(44)
    gas["m"] = np.full(n, 2.0)                                            # w A and w A A are exact
    label = rng.permutation(np.repeat(np.arange(len(POPULATIONS)), POPULATIONS)).astype(np.float64)
    values = np.stack([label, rng.integers(-50, 51, n).astype(np.float64), rng.integers(0, 100, n).astype(np.float64)])
    ctx = make_context(capi, gas, sinks)
    yield ctx, values
    ctx.close()


@pytest.mark.parametrize("weight", ["one", "mass"])
def test_piece_boundaries_exact(capi, integer_set, weight):
    ctx, values = integer_set
    edges = np.arange(len(POPULATIONS) + 1, dtype=np.float64)
    got, counts = _check(capi, ctx, capi.binned_row(0), len(POPULATIONS), values=values, edges=edges, exact=True, weight=weight,
                         q=(capi.binned_row(1), capi.binned_row(2)), squares=True)
    assert tuple(got[:, 0, 0].astype(int)) == POPULATIONS and counts == (sum(POPULATIONS), 0, 0)
    # the same particles in a 2 x 5 grid of (label // 5, label % 5) by two rows
    v2 = np.concatenate([values, (values[0] // 5)[None, :], (values[0] % 5)[None, :]])
    g2, _ = _check(capi, ctx, (capi.binned_row(3), capi.binned_row(4)), (2, 5), values=v2, exact=True, weight=weight,
                   edges=(np.arange(3.0), np.arange(6.0)), q=(capi.binned_row(1), capi.binned_row(2)), squares=True)
    assert np.array_equal(g2.reshape(10, 1, -1), got)                    # b = k0 n[1] + k1, and the same bits


def test_one_bin_and_a_million_bins(capi, integer_set):
    ctx, values = integer_set
    got, counts = _check(capi, ctx, capi.binned_row(1), 1, values=values, ranges=(-50.0, 51.0), exact=True,
                         q=(capi.binned_row(2),), squares=True)
    assert got.shape == (1, 1, 4) and counts == (sum(POPULATIONS), 0, 0)
    # 2^20 bins, nearly all empty: the labels spread to the first bin, the last bin and a few between
    spread = values.copy()
    spread[0] = np.array([0, 1, 1023, 1024, 65535, 65536, 524288, 1048574, 1048575, 77])[values[0].astype(int)]
    n = 1 << 20
    got, counts = _check(capi, ctx, capi.binned_row(0), n, values=spread, ranges=(0.0, float(n)), exact=True, q=(capi.binned_row(1),))
    assert got.shape == (n, 1, 3) and (got[:, 0, 0] > 0).sum() == 9 and got[n - 1, 0, 0] == 2049 and got[0, 0, 0] == 0


# ---- the order rule ------------------------------------------------------------------------------------------------------------
def test_order_rule_bitwise(capi):
    import torch
    gas, sinks = _disc(20000, 13)
    R = np.sqrt(gas["x"] * gas["x"] + gas["y"] * gas["y"])[None, :]
    args = dict(axes=(capi.binned_row(0), "u"), bins=(16, 3), ranges=((5.0, 70.0), (0.1, 0.5)), log=(0,), q=("u", "alpha", "vz"),
                squares=True)
    a = make_context(capi, gas, sinks)
    s0, c0 = a.binned(values=R, **args)                        # upload order
    a.density()                                                # cell-sorted
    s1, c1 = a.binned(values=R, **args)
    s2, c2 = a.binned(values=R, **args)
    b = make_context(capi, gas, sinks, flags=capi.FLAG_HASHED_GRID)
    b.density()
    s3, c3 = b.binned(values=R, **args)
    s4, c4 = a.binned(values=torch.from_numpy(R).to("cuda:0"), device=True, **args)
    assert isinstance(s4, torch.Tensor)
    for s, c in ((s1, c1), (s2, c2), (s3, c3), (s4.cpu().numpy(), _counts(c4))):
        assert np.array_equal(s, s0) and c == c0
    assert s0[..., 0].sum() > 10000 and a.grid_info().kind == 0 and b.grid_info().kind == 1
    a.close(); b.close()


# ---- the tie to sph_profile ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
def test_ring_sums_are_bitwise_sph_profile(capi, log):
    from summersph_amd import terms
    gas, sinks = _disc(20000, 17)
    r0, r1, nr = 10.0, 60.0, 12
    keep = ~profile_ref.edge_margin(gas, r0, r1, nr, 1, log)
    gas = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape == keep.shape else v) for k, v in gas.items()}
    ctx = make_context(capi, gas, sinks)
    _, prof = ctx.profile(r0, r1, nr, log=log, sums_only=True)          # about the origin, normal z^
    R = np.sqrt(gas["x"] * gas["x"] + gas["y"] * gas["y"])[None, :]
    got, counts = ctx.binned(capi.binned_row(0), nr, edges=terms.ring_edges(r0, r1, nr, log), q=("u", "alpha"), weight="mass",
                             values=R)
    assert counts[0] == prof[:, 0].sum() > 5000
    for mine, theirs in ((0, 0), (1, 1), (2, 11), (3, 12)):              # N, sum m, sum m u, sum m alpha
        assert np.array_equal(got[:, 0, mine], prof[:, theirs]), (mine, theirs)
    ctx.close()


# ---- composition with the calls that leave rows on the device ----------------------------------------------------------------------
def test_force_terms_rows_reduce_to_ring_heating(capi):
    import torch
    from summersph_amd import binned, terms
    gas, sinks = _disc(20000, 19)
    edges = terms.ring_edges(12.0, 55.0, 9, log=True)
    R = np.sqrt(gas["x"] * gas["x"] + gas["y"] * gas["y"])
    near = np.min(np.abs(R[:, None] - edges[None, :]), axis=1) <= 1e-10 * R      # the device's R may round the other way
    gas = {k: (v[~near] if isinstance(v, np.ndarray) and v.shape == near.shape else v) for k, v in gas.items()}
    ctx = make_context(capi, gas, sinks)
    ctx.density()
    rows = ctx.force_terms(device=True)
    assert isinstance(rows, torch.Tensor)
    out, sums, counts = binned.ring_sums(ctx, rows, edges)
    assert isinstance(out, torch.Tensor) and isinstance(counts, torch.Tensor)
    counts = _counts(counts)
    host = rows.cpu().numpy()
    want = terms.ring_heating(gas, host, edges)
    for k in range(2):
        err = rel_err(out[k].cpu().numpy(), want[k])
        print(f"ring heating row {k}: {err:.2e}")
        assert err <= TOL, (k, err)
    ring = terms.ring_index(gas, edges)
    nan = np.isnan(host[12]) | np.isnan(host[13])
    assert counts == (int(((ring >= 0) & ~nan).sum()), int((ring < 0).sum()), int(((ring >= 0) & nan).sum()))
    out_h, sums_h, counts_h = binned.ring_sums(ctx, host, edges)         # the host rows give the same bits
    assert np.array_equal(sums_h, sums.cpu().numpy()) and counts_h == counts
    ctx.close()


def test_gradients_rows_on_a_clipped_target_set(capi):
    import torch
    gas, sinks = _disc(20000, 21)
    ctx = make_context(capi, gas, sinks)
    clip = ((-40.0, -40.0, -np.inf), (40.0, 25.0, np.inf))
    grad, _, (n_targets, _) = ctx.gradients(("vx", "vy", "vz"), clip=clip, device=True)
    div = (grad[0, 0] + grad[1, 1]) + grad[2, 2]
    R = np.sqrt(gas["x"] * gas["x"] + gas["y"] * gas["y"])
    values = torch.stack([torch.from_numpy(R).to(div.device), div]).contiguous()
    got, counts = ctx.binned(capi.binned_row(0), 8, ranges=(10.0, 50.0), q=(capi.binned_row(1),), values=values, squares=True,
                             device=True)
    counts = _counts(counts)
    hv = values.cpu().numpy()
    table = capi.binned_edges(ctx.binned_desc, None, 0)
    want, wc = binned_ref.binned_sums([hv[0]], [table], [hv[1]], gas["m"], None, True, True)
    inside = (R >= 10.0) & (R < 50.0)
    assert counts == wc and counts[2] == int((inside & np.isnan(hv[1])).sum()) > 1000 and counts[0] > 1000
    assert counts[0] <= n_targets
    g = got.cpu().numpy()
    assert np.array_equal(g[..., 0], want[..., 0])
    for s in range(1, 4):
        assert rel_err(g[..., s], want[..., s]) <= TOL, s
    ctx.close()


# ---- the selection rule -------------------------------------------------------------------------------------------------------------
def test_ghosts_are_excluded(capi):
    gas, sinks = _disc(20000, 23)
    ctx = make_context(capi, gas, sinks)
    ctx.set_owned(15000)
    owned = np.arange(gas["x"].size) < 15000
    got, counts = _check(capi, ctx, "u", 7, ranges=(0.15, 0.45), q=("alpha",), owned=owned)
    assert sum(counts) == 15000 and counts[0] < 15000
    ctx.close()


def test_full_coverage_and_cull(capi):
    gas, sinks = _disc(20000, 23)
    sinks = dict(sinks); sinks["radius"] = np.array([15.0])   # accretes the inner edge
    ctx = make_context(capi, gas, sinks)
    for step in range(2):
        got, counts = _check(capi, ctx, ("u", "alpha"), (5, 4), ranges=((0.0, 1.0), (0.0, 2.0)), q=("m",), weight="one")
        assert counts == (ctx.n, 0, 0) and got[..., 0].sum() == ctx.n
        assert rel_err(got[..., 2].sum(), ctx.field("m").sum()) <= 1e-13
        got, counts = _check(capi, ctx, "u", 5, ranges=(0.2, 0.3))
        assert sum(counts) == ctx.n and counts[1] > 0
        if step == 0:
            ctx.density(); ctx.forces()
            assert ctx.accrete_and_cull() > 0
    ctx.close()


def test_nan_values(capi, disc):
    ctx, gas, R = disc
    n = R.size
    values = np.stack([R, gas["u"].copy()])
    values[0, [5, 77, 4000]] = np.nan                                    # NaN axis values: outside
    inside = (R >= 10.0) & (R < 60.0)
    got, counts = _check(capi, ctx, capi.binned_row(0), 10, values=values, ranges=(10.0, 60.0), q=(capi.binned_row(1),))
    assert counts[1] == int((~inside).sum()) + int(inside[[5, 77, 4000]].sum())
    # a NaN quantity: dropped with SKIP_NAN, else it poisons its bin and only its bin
    victim = int(np.flatnonzero(inside)[100])
    values = np.stack([R, gas["u"].copy()])
    values[1, victim] = np.nan
    clean, cc = _check(capi, ctx, capi.binned_row(0), 10, values=values, ranges=(10.0, 60.0), q=(capi.binned_row(1), "alpha"))
    assert cc[2] == 1
    got, counts = _check(capi, ctx, capi.binned_row(0), 10, values=values, ranges=(10.0, 60.0), q=(capi.binned_row(1), "alpha"),
                         skip_nan=False, exact=False)
    assert counts == (cc[0] + 1, cc[1], 0)
    k = int(np.searchsorted(capi.binned_edges(ctx.binned_desc, None, 0), R[victim], "right") - 1)
    bad = np.isnan(got)
    assert bad.sum() == 1 and bad[k, 0, 2]                               # sum w A_0 of that bin; N, W and alpha's sum stand
    assert got[k, 0, 0] == clean[k, 0, 0] + 1


def test_empty_context_empty_selection_and_stale_rho(capi):
    ctx = capi.Context(device=0)
    got, counts = ctx.binned("u", 4, ranges=(0.0, 1.0), q=("alpha",), squares=True)
    assert got.shape == (4, 1, 4) and not got.any() and counts == (0, 0, 0)
    import torch
    got, counts = ctx.binned("u", 4, ranges=(0.0, 1.0), device=True)
    assert not got.cpu().numpy().any() and _counts(counts) == (0, 0, 0)
    ctx.close()
    gas, sinks = _disc(3000, 37)
    ctx = make_context(capi, gas, sinks)
    got, counts = ctx.binned("u", 4, ranges=(5.0, 6.0), q=("alpha",))
    assert not got.any() and counts == (0, ctx.n, 0)
    for kw in (dict(axes="rho", bins=4, ranges=(1e-9, 1.0)), dict(axes="u", bins=4, ranges=(0.0, 1.0), q=("P",)),
               dict(axes="u", bins=4, ranges=(0.0, 1.0), weight="volume"), dict(axes="h", bins=4, ranges=(0.0, 1.0))):
        with pytest.raises(capi.SphError) as e:
            ctx.binned(**kw)
        assert e.value.status == SPH_ERR_STATE, kw
    ctx.density()
    assert ctx.binned("rho", 4, ranges=(1e-12, 1.0), log=(0,), weight="volume")[1][0] > 0
    ctx.close()


def test_errors_that_need_a_context(capi):
    gas, sinks = _disc(3000, 37)
    ctx = make_context(capi, gas, sinks)
    lib, n = ctx.lib, ctx.n
    d, _ = capi.binned_desc("u", 4, (0.0, 1.0), q=("alpha",))
    buf, vals = np.full(4 * 3, -7.0), np.zeros((2, n))

    def call(d, values=None, edges=None, sums=buf, n_sums=12):
        return lib.sph_binned(ctx._h, C.byref(d), None if values is None else values.ctypes.data,
                              None if edges is None else edges.ctypes.data, None if sums is None else sums.ctypes.data, n_sums, None)

    assert call(d, n_sums=11) == SPH_ERR_ARG and call(d, n_sums=16) == SPH_ERR_ARG
    assert call(d, sums=None) == SPH_ERR_ARG
    assert call(d, values=vals) == SPH_ERR_ARG                            # values with n_rows == 0
    dr, _ = capi.binned_desc(capi.binned_row(1), 4, (0.0, 1.0), q=("alpha",), n_rows=2)
    assert call(dr) == SPH_ERR_ARG                                        # n_rows > 0 without values
    assert call(d, edges=np.arange(5.0)) == SPH_ERR_ARG
    de, tab = capi.binned_desc("u", 4, edges=np.array([0.0, 0.2, 0.2, 0.4, 1.0]), q=("alpha",))
    assert call(de, edges=tab) == SPH_ERR_ARG
    assert lib.sph_binned(ctx._h, None, None, None, buf.ctypes.data, 12, None) == SPH_ERR_ARG
    assert lib.sph_binned_dev(ctx._h, C.byref(d), None, None, None, 12, None) == SPH_ERR_ARG
    assert np.all(buf == -7.0)                                            # refused before the output is touched
    assert call(d) == 0 and buf[0::3].sum() == n                          # still usable
    assert call(dr, values=vals) == 0 and buf[0] == n
    ctx.close()


# ---- no side effects -------------------------------------------------------------------------------------------------------------------
def test_no_side_effects(capi):
    gas, sinks = _disc(8000, 29)
    runs = []
    for with_binned in (False, True):
        ctx = make_context(capi, gas, sinks)
        dt, t = 1e-3, 0.0
        statsl = []
        for _ in range(10):
            dt, t = ctx.step(dt, t)
            if with_binned:
                s, c = ctx.binned(("rho", "u"), (16, 8), ranges=((1e-12, 1.0), (0.0, 1.0)), log=(0,), q=("alpha", "c", "du"),
                                  weight="volume", squares=True)
                assert c[0] > 0
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


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip(capi, tmp_path):
    from summersph_amd import binned
    gas, sinks = _disc(3000, 41)
    rows = np.stack([gas[k] for k in STATE], axis=1)
    srows = np.stack([sinks[k] for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(1), sinks["m"]], axis=1)
    save = tmp_path / "save.txt"
    txtio.write_save(str(save), rows, srows)
    out = tmp_path / "phase.npz"
    r = subprocess.run([sys.executable, "-m", "summersph_amd.binned", str(save), "-o", str(out), "--x", "rho", "--y", "u", "--bins", "16",
                        "12", "--log", "x,y", "--weight", "mass", "--q", "alpha", "--squares", "--json"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    z = np.load(out)
    g2, s2 = ic.split_rows(np.concatenate([rows[:, :8], srows], axis=0))
    g2["alpha"] = rows[:, 8]
    ctx = make_context(capi, g2, s2)
    ctx.density()
    s, c = ctx.binned(("rho", "u"), (16, 12), ranges=[tuple(v) for v in info["ranges"]], log=(0, 1), q=("alpha",), squares=True)
    assert np.array_equal(z["sums"], s) and tuple(z["counts"]) == c == (3000, 0, 0)
    assert info["selected"] == 3000 and info["gas"] == 3000 and info["bins"] == [16, 12] and info["axes"] == ["rho", "u"]
    N, W, mean, disp = binned.finish(s, 1, True)
    assert np.array_equal(z["N"], N) and np.array_equal(z["mean"], mean, equal_nan=True) and np.array_equal(z["disp"], disp, equal_nan=True)
    assert np.array_equal(z["edges_x"], capi.binned_edges(ctx.binned_desc, None, 0)) and z["edges_y"].size == 13
    assert rel_err(W.sum(), g2["m"].sum()) <= 1e-13
    ctx.close()
