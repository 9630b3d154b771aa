"""GPU tests of sph_pairs (include/summersph.h, "pair sums") on the MI355X.  The sums are exact, so the yardstick is equality:
sums, raw limbs, exponents and counts are compared bitwise (np.array_equal) with the numpy restatement (tests/pairs_ref.py)
over sets, bin counts, edge kinds, weights and quantities; then the edge decisions on hand-placed pairs, the geometry of the
cell search, the independence of upload order, grid, repetition, state and form, the exact additivity over phases and clip
boxes, the selection rule, no side effects on a running simulation, and three physical cases whose bounds are derived, not
measured."""
import numpy as np
import pytest

import pairs_ref
from gpu_support import capi, clumped_disc, golden_gas, make_context, over_defaults
from summersph_amd import pairs

pytestmark = pytest.mark.gpu
SPH_ERR_STATE = 5
EPS = 2.0 ** -52


# ---- scaffolding ----------------------------------------------------------------------------------------------------------------
def _pos(gas):
    return np.stack([gas["x"], gas["y"], gas["z"]], axis=1)


def _vel(gas):
    return np.stack([gas["vx"], gas["vy"], gas["vz"]], axis=1)


def _gas(pos, vel=None, m=None, u=None, h=None):
    n = pos.shape[0]
    vel = np.zeros((n, 3)) if vel is None else vel
    g = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": vel[:, 0].copy(), "vy": vel[:, 1].copy(),
         "vz": vel[:, 2].copy(), "u": np.full(n, 0.2) if u is None else u, "m": np.full(n, 1.0 / n) if m is None else m,
         "alpha": np.ones(n)}
    if h is not None:
        g["h"] = h
    return g


def _call(ctx, r_range, bins, **kw):
    """Context.pairs with raw=True as a dict in pairs_ref's form"""
    sums, counts, exps, raw = ctx.pairs(r_range, bins, raw=True, **kw)
    if kw.get("device"):
        return {"sums": sums.cpu().numpy(), "raw": raw.cpu().numpy().view(np.uint64), "exps": exps.cpu().numpy(),
                "counts": tuple(int(v) for v in counts.cpu().tolist())}
    return {"sums": sums, "raw": raw, "exps": exps, "counts": counts}


def _want(capi, ctx, gas, r_range, bins, n_owned=None, **kw):
    """the restatement of the same call, from the uploaded arrays and the library's own edge table"""
    d, tab = capi.pairs_desc(r_range, bins, kw.get("log", False), kw.get("edges"), kw.get("scale_h", False), kw.get("q", ()),
                             kw.get("weight", "one"), kw.get("velocity", False), kw.get("clip"), kw.get("stride", 1), kw.get("phase", 0),
                             0 if kw.get("values") is None else np.atleast_2d(kw["values"]).shape[0])
    edge = capi.pairs_edges(d, tab)
    values = None if kw.get("values") is None else np.atleast_2d(kw["values"])
    q = kw.get("q", ())
    q = [q] if isinstance(q, (str, int, np.integer)) else list(q)
    A = [values[-1 - s] if not isinstance(s, str) and s < 0 else gas[s if isinstance(s, str) else capi.FIELDS[s]] for s in q]
    h = gas["h"] if "h" in gas else float(ctx.params.h)
    return pairs_ref.pairs(_pos(gas), _vel(gas), gas["m"], h, A, edge, n_owned=n_owned, weight_m=kw.get("weight", "one") == "mass",
                           velocity=kw.get("velocity", False), scale_h=kw.get("scale_h", False), clip=kw.get("clip"),
                           stride=kw.get("stride", 1), phase=kw.get("phase", 0))


def _same(a, b):
    assert a["counts"] == b["counts"], (a["counts"], b["counts"])
    assert np.array_equal(a["exps"], b["exps"]), (a["exps"], b["exps"])
    assert a["raw"].shape == b["raw"].shape and np.array_equal(a["raw"], b["raw"])
    assert a["sums"].shape == b["sums"].shape and np.array_equal(a["sums"], b["sums"])


def _check(capi, ctx, gas, r_range, bins, n_owned=None, **kw):
    got = _call(ctx, r_range, bins, **kw)
    _same(got, _want(capi, ctx, gas, r_range, bins, n_owned=n_owned, **kw))
    return got


# ---- bitwise against the restatement ---------------------------------------------------------------------------------------------
def _rows(gas, seed):
    """two caller rows: one smooth, one integer-valued"""
    rng = np.random.default_rng(seed)
    return np.stack([np.hypot(gas["x"], gas["y"]), rng.integers(-4, 5, gas["x"].size).astype(np.float64)])


@pytest.fixture(scope="module", params=["disc3000_eval", "discv3000_eval", "clumped"])
def particle_set(request, capi):
    name = request.param
    if name == "clumped":
        gas, sinks, _, _ = clumped_disc(1500, 3, 200, 21)
    else:
        gas, sinks = golden_gas(name)
    gas = dict(gas)
    variable = "h" in gas
    ctx = make_context(capi, gas, sinks, variable=variable)
    # the binned variable's reach: two smoothing lengths (r / h with variable h), a clump's size in the clumped set
    top = 2.0 if variable else (1.2 if name == "clumped" else 2.0 * float(ctx.params.h))
    yield ctx, gas, top, variable
    ctx.close()


def test_equal_masses_wrap_the_low_limb(capi, particle_set):
    ctx, gas, top, variable = particle_set
    got = _check(capi, ctx, gas, (0.0, top), 1, weight="mass", scale_h=variable)
    assert got["sums"][0, 0] > 16
    if np.all(gas["m"] == gas["m"][0]):
        assert got["raw"][0, 1, 1] > 0                                  # W's high limb: the carry was taken


CASES = {
    "one bin, counts only": dict(bins=1),
    "7 log bins, mass, velocity, u": dict(bins=7, log=True, weight="mass", velocity=True, q=("u",)),
    "64 caller bins, mass, velocity, 4 q": dict(bins=64, caller=True, weight="mass", velocity=True, q=("u", -1, "vx", -2)),
    "64 log bins, a row": dict(bins=64, log=True, q=(-2,)),
    "7 linear bins, mass, 4 q": dict(bins=7, weight="mass", q=("vz", "u", -1, "y")),
    "64 linear bins, velocity": dict(bins=64, velocity=True),
    "1024 bins in chunks": dict(bins=1024, weight="mass", velocity=True, q=("u", -1, "vx", -2)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bitwise_against_the_restatement(capi, particle_set, case):
    ctx, gas, top, variable = particle_set
    kw = dict(CASES[case])
    bins = kw.pop("bins")
    lo = 0.05 * top if kw.get("log") else 0.0
    r_range = (lo, top)
    if kw.pop("caller", False):
        kw["edges"] = np.sort(np.random.default_rng(bins).uniform(0.0, top, bins + 1))
        r_range = None
    if any(not isinstance(s, str) for s in kw.get("q", ())):
        kw["values"] = _rows(gas, 3)
    got = _check(capi, ctx, gas, r_range, bins, scale_h=variable, **kw)
    assert got["sums"][:, 0].sum() > 10000 and got["counts"][2] == 0


def test_fixed_h_scaling_divides_by_the_parameter(capi):
    gas, sinks = golden_gas("disc3000_eval")
    ctx = make_context(capi, gas, sinks)
    got = _check(capi, ctx, gas, (0.1, 2.0), 7, log=True, scale_h=True, velocity=True)
    assert got["sums"][:, 0].sum() > 10000
    ctx.close()


# ---- edge decisions ----------------------------------------------------------------------------------------------------------------
HAND = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 3.0], [5.0, 0.0, 12.0]])     # r = 5, 3, 13 from the first: d2 exact
ONLY_FIRST = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def test_edge_decisions(capi):
    gas = _gas(HAND, vel=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -2.0], [0.0, 0.0, 0.0]]), m=np.array([1.0, 2.0, 4.0, 8.0]))
    ctx = make_context(capi, gas)
    up, down = np.nextafter(5.0, np.inf), np.nextafter(5.0, -np.inf)
    for inner, bins_of_5 in ((5.0, 1), (up, 0), (down, 1)):           # on the edge: the upper bin; an ulp either side
        got = _check(capi, ctx, gas, None, 2, edges=np.array([1.0, inner, 20.0]), clip=ONLY_FIRST, weight="mass", velocity=True)
        assert got["counts"] == (1, 4, 0)
        n = got["sums"][:, 0].tolist()
        assert n == ([1.0, 2.0] if bins_of_5 == 1 else [2.0, 1.0]), (inner, n)       # r = 3 below, r = 13 above, r = 5 decided
    got = _check(capi, ctx, gas, None, 2, edges=np.array([3.0, 5.0, 13.0]), clip=ONLY_FIRST, weight="mass", velocity=True)
    assert got["sums"][:, 0].tolist() == [1.0, 1.0]                    # r on edge[0] is inside, r on edge[n_bins] outside
    assert got["sums"][:, 1].tolist() == [4.0, 2.0] and got["sums"][0, 2] == -8.0 and got["sums"][1, 2] == 2.0 * 0.6
    ctx.close()


def test_a_coincident_pair(capi):
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.5, 2.0, 3.0]])
    gas = _gas(pos, vel=np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0], [1.0, 0.0, 0.0]]))
    ctx = make_context(capi, gas)
    got = _check(capi, ctx, gas, (0.0, 0.25), 1, velocity=True)        # r_lo = 0: counted, u = 0
    assert got["sums"][0].tolist() == [2.0, 2.0, 0.0, 0.0, 0.0, 50.0]
    got = _check(capi, ctx, gas, (1e-300, 0.25), 1, log=True, velocity=True)      # log bins: outside
    assert not got["sums"].any() and not got["raw"].any()
    ctx.close()


# ---- search geometry ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice(capi):
    g = np.arange(3.0)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(4)
    gas = _gas(pos, vel=rng.normal(size=(27, 3)), m=rng.uniform(1.0, 2.0, 27))
    ctx = make_context(capi, gas)
    yield ctx, gas
    ctx.close()


def test_the_centre_sees_all_26_neighbour_cells(capi, lattice):
    ctx, gas = lattice
    top = np.sqrt(3.0) * (1.0 + 1e-3)
    got = _check(capi, ctx, gas, (0.0, top), 3, clip=((0.5, 0.5, 0.5), (1.5, 1.5, 1.5)), weight="mass", velocity=True)
    assert got["counts"] == (1, 27, 0) and got["sums"][:, 0].sum() == 26          # the sources outside the clip box too
    _check(capi, ctx, gas, (0.0, top), 3, weight="mass", velocity=True)


def test_one_cell_and_no_pair(capi, lattice):
    ctx, gas = lattice
    got = _check(capi, ctx, gas, (0.0, 1e3), 5, q=("u",))
    assert got["sums"][:, 0].sum() == 27 * 26                                      # r_hi far beyond the box: every ordered pair
    got = _check(capi, ctx, gas, (0.0, 0.5), 5, weight="mass", velocity=True)
    assert not got["sums"].any() and not got["raw"].any()                          # r_hi below the smallest separation
    assert got["counts"] == (27, 27, 0)


def test_two_far_clusters_enlarge_the_cells(capi):
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.uniform(0.0, 0.02, (300, 3)), 1e4 + rng.uniform(0.0, 0.02, (300, 3))])
    gas = _gas(pos, vel=rng.normal(size=(600, 3)))
    ctx = make_context(capi, gas)
    got = _check(capi, ctx, gas, (0.0, 0.004), 7, velocity=True)       # 1e4 / 0.004 cells per axis > 2^21 - 8
    assert got["sums"][:, 0].sum() > 1000
    got = _check(capi, ctx, gas, (0.001, 0.03), 7, log=True, q=("vx",))            # and without the enlargement
    assert got["sums"][:, 0].sum() > 50000
    ctx.close()


def test_one_h_fifty_times_the_others(capi):
    rng = np.random.default_rng(9)
    n = 500
    h = np.full(n, 0.05)
    h[123] = 2.5
    gas = _gas(rng.uniform(0.0, 1.0, (n, 3)), vel=rng.normal(size=(n, 3)), h=h)
    ctx = make_context(capi, gas, variable=True)
    got = _check(capi, ctx, gas, (0.0, 2.0), 8, scale_h=True, velocity=True, q=("h",))
    assert got["sums"][:, 0].sum() > n - 1 + 500                       # the wide one alone sees every other particle
    ctx.close()


# ---- independence ------------------------------------------------------------------------------------------------------------------
KW = dict(log=True, weight="mass", velocity=True, q=("u", -1))


@pytest.fixture(scope="module")
def disc(capi):
    gas, sinks = golden_gas("disc3000_eval")
    gas = dict(gas)
    ctx = make_context(capi, gas, sinks)
    rows = _rows(gas, 5)[:1]
    first = _call(ctx, (0.25, 5.0), 16, values=rows, **KW)
    yield ctx, gas, sinks, rows, first
    ctx.close()


def test_independent_of_repetition_state_and_form(capi, disc):
    ctx, gas, sinks, rows, first = disc
    _same(_call(ctx, (0.25, 5.0), 16, values=rows, **KW), first)                   # a repeated call
    import torch
    dev = _call(ctx, (0.25, 5.0), 16, values=torch.tensor(rows, device=f"cuda:{ctx.device}"), device=True, **KW)
    _same(dev, first)                                                              # the conversion kernel against the host's
    assert np.max(np.abs(first["raw"][:, 1:, 1].view(np.int64))) > 0               # sums wider than 64 bits were converted
    ctx.density()
    _same(_call(ctx, (0.25, 5.0), 16, values=rows, **KW), first)                   # after sph_density: another slot order
    d, _ = capi.pairs_desc((0.25, 5.0), 16, **{k: v for k, v in KW.items()}, n_rows=1)
    assert np.array_equal(capi.pairs_finish(d, first["exps"], first["raw"]), first["sums"])


def test_independent_of_upload_order_and_grid(capi, disc):
    _, gas, sinks, rows, first = disc
    perm = np.random.default_rng(6).permutation(gas["x"].size)
    shuffled = {k: v[perm] for k, v in gas.items()}
    ctx = make_context(capi, shuffled, sinks, density=True)
    _same(_call(ctx, (0.25, 5.0), 16, values=rows[:, perm], **KW), first)
    ctx.close()
    ctx = make_context(capi, gas, sinks, flags=over_defaults(capi, capi.FLAG_HASHED_GRID, False), density=True)
    assert ctx.grid_info().kind == 1
    _same(_call(ctx, (0.25, 5.0), 16, values=rows, **KW), first)
    ctx.close()


# ---- exact additivity --------------------------------------------------------------------------------------------------------------
def _added(parts):
    raw = parts[0]["raw"]
    for p in parts[1:]:
        assert np.array_equal(p["exps"], parts[0]["exps"])
        raw = pairs.add_raw(raw, p["raw"])
    return raw


def test_phases_and_clip_boxes_add_exactly(capi, disc):
    ctx, gas, sinks, rows, first = disc
    d, _ = capi.pairs_desc((0.25, 5.0), 16, **KW, n_rows=1)
    phases = [_call(ctx, (0.25, 5.0), 16, values=rows, stride=4, phase=p, **KW) for p in range(4)]
    assert sum(p["counts"][0] for p in phases) == first["counts"][0] and all(p["counts"][1] == first["counts"][1] for p in phases)
    raw = _added(phases)
    assert np.array_equal(raw, first["raw"])
    assert np.array_equal(capi.pairs_finish(d, first["exps"], raw), first["sums"])
    xs = np.sort(gas["x"])
    cut = 0.5 * (xs[xs.size // 2 - 1] + xs[xs.size // 2])
    assert not np.any(gas["x"] == cut)
    inf = np.inf
    boxes = [((-inf, -inf, -inf), (cut, inf, inf)), ((cut, -inf, -inf), (inf, inf, inf))]
    halves = [_call(ctx, (0.25, 5.0), 16, values=rows, clip=b, **KW) for b in boxes]
    assert [h["counts"][0] for h in halves] == [int((gas["x"] < cut).sum()), int((gas["x"] > cut).sum())]
    raw = _added(halves)
    assert np.array_equal(raw, first["raw"])
    assert np.array_equal(capi.pairs_finish(d, first["exps"], raw), first["sums"])


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def test_nan_rows_and_ghosts_are_left_out(capi, disc):
    ctx, gas, sinks, rows, first = disc
    bad = rows.copy()
    bad[0, [5, 77, 1500]] = [np.nan, np.inf, -np.inf]
    got = _check(capi, ctx, gas, (0.25, 5.0), 16, values=bad, **KW)
    assert got["counts"] == (first["counts"][0] - 3, first["counts"][1] - 3, 3)
    assert got["sums"][:, 0].sum() < first["sums"][:, 0].sum()
    plain = _check(capi, ctx, gas, (0.25, 5.0), 16, velocity=True)                 # the row is not requested: nobody is dropped
    assert plain["counts"][2] == 0
    n = gas["x"].size
    own = make_context(capi, gas, sinks, n_owned=n - 700)
    got = _check(capi, own, gas, (0.25, 5.0), 16, n_owned=n - 700, values=rows, stride=2, phase=1, **KW)
    assert got["counts"][1] == n - 700 and got["counts"][0] == (n - 700) // 2
    own.close()


# ---- state -------------------------------------------------------------------------------------------------------------------------
def test_a_step_does_not_see_the_call(capi):
    gas, sinks = golden_gas("disc3000_eval")
    a, b = make_context(capi, gas, sinks, density=True), make_context(capi, gas, sinks, density=True)
    stats = a.stats()
    a.pairs((0.25, 5.0), 16, **{k: v for k, v in KW.items() if k != "q"}, q=("rho",))
    after = a.stats()
    for k in ("grid_builds", "nlist_builds", "density_passes", "force_passes"):
        assert getattr(after, k) == getattr(stats, k), k
    assert a.step(1e-2) == b.step(1e-2)
    for f in ("x", "y", "z", "vx", "vy", "vz", "u", "alpha"):
        assert np.array_equal(a.field(f), b.field(f)), f
    a.close(); b.close()


def test_a_stale_derived_field_is_refused(capi):
    gas, sinks = golden_gas("disc3000_eval")
    ctx = make_context(capi, gas, sinks)
    for q in ("rho", "P", "ax"):
        with pytest.raises(capi.SphError) as e:
            ctx.pairs((0.0, 5.0), 4, q=(q,))
        assert e.value.status == SPH_ERR_STATE, q
    ctx.density()
    ctx.pairs((0.0, 5.0), 4, q=("rho", "P"))
    with pytest.raises(capi.SphError) as e:
        ctx.pairs((0.0, 5.0), 4, q=("ax",))
    assert e.value.status == SPH_ERR_STATE
    ctx.close()


# ---- physics with derived bounds -----------------------------------------------------------------------------------------------------
INNER = ((0.25, 0.25, 0.25), (0.75, 0.75, 0.75))


@pytest.fixture(scope="module")
def poisson():
    rng = np.random.default_rng(2024)
    return rng.uniform(0.0, 1.0, (3000, 3))


def test_poisson_counts(capi, poisson):
    """Uniform random points: every shell of a target in the inner half-box lies inside the unit box (r_hi = 0.2 < 0.25), so
    N_b is a sum of n_t n nearly independent indicators of probability V_shell: mean E_b = n_t n V_shell and variance
    <= E_b.  5 sigma; tests/test_pairs_cpu.py's reference gives the same counts for this seed."""
    gas = _gas(poisson)
    ctx = make_context(capi, gas)
    got = _check(capi, ctx, gas, (0.0, 0.2), 8, clip=INNER)
    edge = capi.pairs_edges(ctx.pairs_desc)
    E = got["counts"][0] * 3000 * (4.0 * np.pi / 3.0) * (edge[1:] ** 3 - edge[:-1] ** 3)
    print("N", got["sums"][:, 0], "E", E)
    assert 300 < got["counts"][0] < 450
    assert np.all(np.abs(got["sums"][:, 0] - E) <= 5.0 * np.sqrt(E))
    ctx.close()


def _rotation_bound(omega, R, W):
    """|sum w u| of a bin under v = Omega x r.  In exact arithmetic (Omega x dr) . dr = 0.  In doubles a velocity component
    (two products and a difference) is off by <= 2 eps |Omega| R, a difference dv by <= 5 eps |Omega| R, dx by <= eps / 2 |dx|
    and the three-term dot product adds <= 3 eps |dv| r; with |dv| <= |Omega| r and r <= 2 R that is
    |dot| <= eps |Omega| r (5 sqrt(3) R + sqrt(3) / 2 r + 3 r) < 17 eps |Omega| R r, so |u| < 17 eps |Omega| R before the
    division's own rounding: 32 eps |Omega| R W bounds the bin's sum with room for that and for the half quantum per term."""
    return 32.0 * EPS * float(np.linalg.norm(omega)) * R * W


def test_rigid_rotation_has_no_radial_velocity(capi, poisson):
    pos = poisson[:1500] - 0.5
    omega = np.array([0.3, -1.1, 2.0])
    vel = np.cross(omega, pos)
    rng = np.random.default_rng(5)
    gas = _gas(pos, vel=vel, m=rng.uniform(0.5, 2.0, 1500))
    ctx = make_context(capi, gas)
    got = _check(capi, ctx, gas, (0.0, 0.3), 6, weight="mass", velocity=True)
    R = float(np.max(np.linalg.norm(pos, axis=1)))
    s = got["sums"]
    print("sum w u", s[:, 2], "bound", _rotation_bound(omega, R, s[:, 1]))
    assert np.all(s[:, 0] > 100)
    assert np.all(np.abs(s[:, 2]) <= _rotation_bound(omega, R, s[:, 1]))
    # |dv|^2 = |Omega x dr|^2 <= |Omega|^2 r^2 is all transverse: S2_perp = <|dv|^2> / 2 up to the same rounding
    f = pairs.finish(s, 0, velocity=True)
    assert np.all(f["S2_perp"] > 0.0) and np.all(f["S2_par"] <= (32.0 * EPS * np.linalg.norm(omega) * R) ** 2)
    ctx.close()


def test_uniform_expansion_gives_hubble_flow(capi, poisson):
    pos = poisson[:1500] - 0.5
    H = 0.7
    gas = _gas(pos, vel=H * pos)
    ctx = make_context(capi, gas)
    got = _check(capi, ctx, gas, (0.02, 0.3), 9, log=True, velocity=True)
    edge = capi.pairs_edges(ctx.pairs_desc)
    f = pairs.finish(got["sums"], 0, velocity=True)
    full = f["N"] > 0
    assert full.sum() >= 8
    lo, hi = H * edge[:-1][full], H * edge[1:][full]                   # u = H r for every pair: the mean lies in the bin
    assert np.all(f["u"][full] >= lo * (1.0 - 1e-12)) and np.all(f["u"][full] <= hi * (1.0 + 1e-12))
    ctx.close()


# ---- g(r / h) and the command line ----------------------------------------------------------------------------------------------------
def test_rdf_of_poisson_points_is_one(capi, poisson):
    """rdf on a real context: the targets restated on the host are the call's, and g is N over the expectation that the SPH
    number densities rho_i / m_i of those targets give."""
    gas = _gas(poisson)
    ctx = make_context(capi, gas, h=0.08, density=True)
    sums, counts, exps = ctx.pairs((0.05, 0.2), 4, clip=INNER)
    edge = capi.pairs_edges(ctx.pairs_desc)
    g = pairs.rdf(ctx, sums, edge, False, INNER)
    t = pairs.targets(poisson, 3000, INNER)
    assert t.sum() == counts[0]
    dens = float(np.sum(ctx.field("rho")[t] / gas["m"][t]))
    assert np.allclose(g, sums[:, 0] / (dens * 4.0 * np.pi / 3.0 * (edge[1:] ** 3 - edge[:-1] ** 3)), rtol=1e-14)
    assert np.all(g > 0.0)
    ctx.close()


def test_cli_round_trip(capi, tmp_path, capsys):
    import json
    from summersph_amd import txtio
    from summersph_amd.cli import read_save, uploaded_context
    gas, sinks = golden_gas("disc3000_eval")
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    ns = np.size(sinks["m"])
    srows = np.stack([np.reshape(sinks[k], ns) for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(ns), np.reshape(sinks["m"], ns)], axis=1)
    save, out = tmp_path / "save.txt", tmp_path / "pairs.npz"
    txtio.write_save(str(save), rows, srows)
    assert pairs.main([str(save), "-o", str(out), "--r", "0.05", "2", "--bins", "8", "--log", "--scale-h", "--velocity", "--q", "u",
                       "--stride", "4", "--phase", "1", "--json"]) == 0
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    z = np.load(out)
    g2, s2 = read_save(str(save))                                       # what the tool uploaded
    with uploaded_context(g2, s2) as ctx:
        ctx.density()
        sums, counts, exps, raw = ctx.pairs((0.05, 2.0), 8, log=True, scale_h=True, velocity=True, q=("u",), stride=4, phase=1, raw=True)
        edge = capi.pairs_edges(ctx.pairs_desc)
        g = pairs.rdf(ctx, sums, edge, True, None, 4, 1)
    assert np.array_equal(z["sums"], sums) and np.array_equal(z["raw"], raw) and np.array_equal(z["exps"], exps)
    assert tuple(z["counts"]) == counts and np.array_equal(z["edges"], edge) and np.array_equal(z["g"], g, equal_nan=True)
    assert info["targets"] == counts[0] == (g2.shape[0] + 2) // 4 and info["pairs"] == int(sums[:, 0].sum()) > 1000
    assert z["S2_par"].shape == (8,) and z["dA"].shape == (8, 1) and int(z["desc_target_stride"]) == 4 and list(z["q"]) == ["u"]
    assert np.all(g[sums[:, 0] > 0] > 0.0)
