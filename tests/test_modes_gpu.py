"""GPU tests of sph_modes (include/summersph.h, "mode sums") on the MI355X.  The ring sums are exact and use no library
function, so their yardstick is equality: sums, raw limbs, exponent, ring counts and counts are compared bitwise
(np.array_equal) with the numpy restatement (tests/modes_ref.py).  The spiral sums go through log and sincos and are held
to the derived bound against the longdouble sums.  Then three analytic sets that do not use the restatement, the
independence of upload order, grid, form and slot order, the exact additivity over contexts, every edge of the selection,
the chunked histogram, every refusal, and no side effect on the context."""
import ctypes as C

import numpy as np
import pytest

import modes_ref
from gpu_support import capi, golden_gas, make_context, over_defaults
from summersph_amd import modes

pytestmark = pytest.mark.gpu
SPH_ERR_ARG, SPH_ERR_STATE = 1, 5
RINGS = (10.5, 36.0)


# ---- scaffolding ----------------------------------------------------------------------------------------------------------------
def _pos(gas):
    return np.stack([gas["x"], gas["y"], gas["z"]], axis=1)


def _gas(pos, m, vx=None):
    n = pos.shape[0]
    return {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": np.zeros(n) if vx is None else vx,
            "vy": np.zeros(n), "vz": np.zeros(n), "u": np.full(n, 0.2), "m": np.asarray(m, dtype=np.float64), "alpha": np.ones(n)}


def _call(ctx, r_range, n_r, m_max, **kw):
    """Context.modes with raw=True as a dict in modes_ref's form"""
    ring, spiral, rc, counts, exp, raw = ctx.modes(r_range, n_r, m_max, raw=True, **kw)
    if kw.get("device"):
        host = lambda t: None if t is None else t.cpu().numpy()
        return {"ring": host(ring), "spiral": host(spiral), "raw_ring": host(raw[0]).view(np.uint64),
                "raw_spiral": None if raw[1] is None else host(raw[1]).view(np.uint64), "exp": int(exp.cpu()[0]),
                "ring_counts": host(rc), "counts": tuple(int(v) for v in counts.cpu().tolist())}
    return {"ring": ring, "spiral": spiral, "raw_ring": raw[0], "raw_spiral": raw[1], "exp": exp, "ring_counts": rc, "counts": counts}


def _want(capi, ctx, gas, centre, n_owned=None, **kw):
    """the restatement of the call the context just made, from the uploaded arrays and the library's own tables"""
    d = ctx.modes_desc
    edges, p = capi.modes_tables(d)
    A = None
    if d.n_q:
        A = np.atleast_2d(kw["values"])[-1 - d.q] if d.q < 0 else gas[capi.FIELDS[d.q]]
    return modes_ref.modes(_pos(gas), gas["m"], A, edges=edges, m_max=d.m_max, centre=centre, normal=tuple(d.normal), z_max=d.z_max,
                           weight_m=d.weight == capi.MODES_W_MASS, p=p if d.n_p else None, r_ref=d.r_ref, n_owned=n_owned)


def _same_rings(a, b):
    assert a["counts"] == b["counts"], (a["counts"], b["counts"])
    assert a["exp"] == b["exp"], (a["exp"], b["exp"])
    assert np.array_equal(a["ring_counts"], b["ring_counts"])
    assert a["raw_ring"].shape == b["raw_ring"].shape and np.array_equal(a["raw_ring"], b["raw_ring"])
    assert a["ring"].shape == b["ring"].shape and np.array_equal(a["ring"], b["ring"])


def _same(a, b):
    """two results of the library: everything, the spiral block included"""
    _same_rings(a, b)
    assert (a["spiral"] is None) == (b["spiral"] is None)
    if a["spiral"] is not None:
        assert np.array_equal(a["raw_spiral"], b["raw_spiral"]) and np.array_equal(a["spiral"], b["spiral"])


@pytest.fixture(scope="module")
def disc(capi):
    gas, sinks = golden_gas("disc3000_eval")
    gas = dict(gas)
    ctx = make_context(capi, gas, sinks)
    centre = (float(sinks["x"][0]), float(sinks["y"][0]), float(sinks["z"][0]))
    rng = np.random.default_rng(12)
    rows = np.stack([rng.normal(size=gas["x"].size), gas["vx"]])
    yield ctx, gas, sinks, centre, rows
    ctx.close()


# ---- exact ring sums --------------------------------------------------------------------------------------------------------------
def test_ring_sums_bitwise_against_the_restatement(capi, disc):
    ctx, gas, sinks, centre, rows = disc
    assert hasattr(capi.load(), "sph_modes")
    got = _call(ctx, RINGS, 7, 8, log=True, sink=0)
    _same_rings(got, _want(capi, ctx, gas, centre))
    assert got["spiral"] is None and got["counts"][0] > 2000 and got["counts"][1] > 100 and got["counts"][2:] == (0, 0)
    assert got["ring_counts"].sum() == got["counts"][0] and np.all(got["ring_counts"] > 0)
    assert np.max(np.abs(got["raw_ring"][:, 0, 0, 1].view(np.int64))) > 0        # equal masses: C_0 carried into the high limb


@pytest.mark.parametrize("form", ["field", "row"])
def test_ring_sums_of_a_signed_quantity(capi, disc, form):
    ctx, gas, sinks, centre, rows = disc
    kw = dict(q="vx") if form == "field" else dict(q=capi.modes_row(1), values=rows)
    got = _call(ctx, RINGS, 7, 8, log=True, sink=0, **kw)
    want = _want(capi, ctx, gas, centre, **kw)
    _same_rings(got, want)
    assert np.any(got["raw_ring"][..., 1] == np.uint64(2 ** 64 - 1)) and np.any(got["ring"] < 0.0)      # negative sums: the sign word
    if form == "row":                                                           # the two forms read the same numbers
        _same_rings(got, _call(ctx, RINGS, 7, 8, log=True, sink=0, q="vx"))


# ---- analytic, independent of the restatement -----------------------------------------------------------------------------------------
def test_five_fold_rings_hold_only_m_5(capi):
    """K = 5 equal particles per ring at phi0 + 2 pi j / 5: sum_j exp(i m phi_j) vanishes unless 5 divides m, and is
    K exp(5 i phi0) for m = 5."""
    K, w = 5, 1.0 / 64
    radii, phi0 = (1.5, 2.5, 3.5), (0.1, 0.3, -0.5)
    pos = np.array([[R * np.cos(f0 + 2 * np.pi * j / K), R * np.sin(f0 + 2 * np.pi * j / K), 0.0] for R, f0 in zip(radii, phi0)
                    for j in range(K)])
    gas = _gas(pos, np.full(3 * K, w))
    ctx = make_context(capi, gas)
    got = _call(ctx, (1.0, 4.0), 3, 8)
    assert got["ring_counts"].tolist() == [K, K, K] and got["counts"] == (3 * K, 0, 0, 0)
    for m in (1, 2, 3, 4, 6, 7, 8):
        print(m, np.max(np.abs(got["ring"][:, m])) / (K * w * 2.0 ** -52))
        assert np.all(np.abs(got["ring"][:, m]) <= K * w * (2 * m + 4) * 2.0 ** -52), m
    tol = (2 * 5 + 4) * 2.0 ** -52
    amp = np.hypot(got["ring"][:, 5, 0], got["ring"][:, 5, 1])
    phase = np.arctan2(got["ring"][:, 5, 1], got["ring"][:, 5, 0])
    print(amp / (K * w) - 1.0, phase - 5 * np.array(phi0))
    assert np.all(np.abs(amp - K * w) <= K * w * tol)
    assert np.all(np.abs(phase - 5 * np.array(phi0)) <= tol + 2 * np.spacing(np.abs(phase)))       # |5 phi0| < pi: no wrap
    assert np.array_equal(got["ring"][:, 0, 0], [K * w] * 3) and not got["ring"][:, 0, 1].any()
    ctx.close()


def test_four_against_one_is_minus_three_w_exactly(capi):
    w = 2.0 ** -20
    pos = np.array([[-2.0, 0.0, 0.0], [-2.5, 0.0, 0.1], [-3.0, 0.0, -0.1], [-3.5, 0.0, 0.0], [2.75, 0.0, 0.0]])
    ctx = make_context(capi, _gas(pos, np.full(5, w)))
    got = _call(ctx, (1.0, 4.0), 1, 3)
    assert got["exp"] == -18
    assert got["ring"][0].tolist() == [[5 * w, 0.0], [-3 * w, 0.0], [5 * w, 0.0], [-3 * w, 0.0]]
    assert modes_ref.from_limbs(*got["raw_ring"][0, 1, 0]) == -3 << 60                   # 3 w 2^(62 + 18), negative:
    assert int(got["raw_ring"][0, 1, 0, 1]) == 2 ** 64 - 1                               # the high limb is the sign word
    ctx.close()


def test_a_logarithmic_spiral_peaks_at_its_own_m_and_p(capi):
    """64 particles on phi = -(p* / m*) ln(R / r_ref): m* phi + p* ln(R / r_ref) = 0 for every one of them, so the (m*, p*)
    sum has the modulus sum w.  It is the largest of row m*, and (m*, -p*) is not: the sign convention."""
    ms, ps, r_ref, n = 2, 8.0, 2.0, 64
    rng = np.random.default_rng(3)
    R = np.sort(rng.uniform(1.0, 6.0, n))
    phi = -(ps / ms) * np.log(R / r_ref)
    w = rng.uniform(0.5, 1.5, n)
    pos = np.stack([R * np.cos(phi), R * np.sin(phi), np.zeros(n)], axis=1)
    ctx = make_context(capi, _gas(pos, w))
    got = _call(ctx, (0.5, 7.0), 2, 4, spiral=(-16.0, 16.0, 65), r_ref=r_ref)
    p = capi.modes_tables(ctx.modes_desc)[1]
    ls = int(np.flatnonzero(p == ps)[0])
    amp = np.hypot(got["spiral"][..., 0], got["spiral"][..., 1])
    bound = modes_ref.spiral_bound(w, np.log(R / r_ref), 4, p)
    print("amp - sum w", amp[ms, ls] - w.sum(), "bound", bound[ms, ls])
    assert got["counts"] == (n, 0, 0, 0)
    assert abs(amp[ms, ls] - w.sum()) <= bound[ms, ls]
    assert int(np.argmax(amp[ms])) == ls and amp[ms, int(np.flatnonzero(p == -ps)[0])] < 0.5 * w.sum()
    # its phase is 0, all of it in CS.  The sine sum is first order in the phase errors: the call's own (the bound) and those
    # the set was made with -- phi itself (log, quotient, product: 3/2 ulp of |phi|) and x, y = R cos phi, R sin phi (3/2 ulp
    # each, which moves the angle and ln R by as much): per particle (3 m* (1 + |phi|) + 3 p*) 2^-53
    made = np.sum(w * (3.0 * ms * (1.0 + np.abs(phi)) + 3.0 * ps)) * 2.0 ** -53
    print("SN", got["spiral"][ms, ls, 1], "tolerance", bound[ms, ls] + made)
    assert abs(got["spiral"][ms, ls, 1]) <= bound[ms, ls] + made
    f = modes.finish(got["ring"], got["spiral"], p)
    assert f["p_peak"][ms] == ps and f["pitch"][ms] == np.arctan(ms / ps) and abs(f["spectrum"][ms, ls] - 1.0) < 1e-14
    ctx.close()


# ---- order-freedom ------------------------------------------------------------------------------------------------------------------
def _kw(rows):
    """a signed quantity from row 1, rings and spiral sums"""
    return dict(log=True, sink=0, q=-2, values=rows, spiral=(-8.0, 8.0, 33), r_ref=10.0)


def test_independent_of_upload_order_grid_form_and_slot_order(capi, disc):
    ctx, gas, sinks, centre, rows = disc
    first = _call(ctx, RINGS, 7, 8, **_kw(rows))
    assert first["spiral"].shape == (9, 33, 2) and np.any(first["raw_spiral"][..., 1] == np.uint64(2 ** 64 - 1))
    _same(_call(ctx, RINGS, 7, 8, **_kw(rows)), first)                                   # a repeated call
    import torch
    dev = _call(ctx, RINGS, 7, 8, device=True, **_kw(torch.tensor(rows, device=f"cuda:{ctx.device}")))
    _same(dev, first)                                                                    # the conversion kernel against the host's
    d = ctx.modes_desc
    back = capi.modes_finish(d, first["exp"], (first["raw_ring"], first["raw_spiral"]))
    assert np.array_equal(back[0], first["ring"]) and np.array_equal(back[1], first["spiral"])
    perm = np.random.default_rng(6).permutation(gas["x"].size)
    shuffled = {k: v[perm] for k, v in gas.items()}
    for flags in (0, over_defaults(capi, capi.FLAG_HASHED_GRID, False)):
        other = make_context(capi, shuffled, sinks, flags=flags, density=True)
        assert not flags or other.grid_info().kind == 1
        _same(_call(other, RINGS, 7, 8, **_kw(rows[:, perm])), first)
        other.close()
    # a step re-sorts the slots: the stepped context against a fresh one holding its downloaded state
    moved = make_context(capi, gas, sinks, density=True)
    moved.step(1e-2)
    state, sk = moved.state(), moved.get_sinks()
    a = _call(moved, RINGS, 7, 8, **_kw(rows))
    fresh = make_context(capi, state, sk)
    b = _call(fresh, RINGS, 7, 8, **_kw(rows))
    _same(a, b)
    assert not np.array_equal(a["raw_ring"], first["raw_ring"])                          # the particles did move
    moved.close(); fresh.close()


# ---- additivity -----------------------------------------------------------------------------------------------------------------------
def test_two_contexts_add_exactly(capi, disc):
    ctx, gas, sinks, centre, rows = disc
    n = gas["x"].size
    vals = rows[:1].copy()
    sel = np.flatnonzero((np.hypot(gas["x"], gas["y"]) > 12.0) & (np.hypot(gas["x"], gas["y"]) < 30.0))
    vals[0, sel[0]] = vals[0, sel[-1]] = -7.5                                            # the largest weight, once in either half
    cut = (sel[0] + sel[-1]) // 2 + 1
    kw = dict(log=True, sink=0, q=-1, spiral=(-8.0, 8.0, 33), r_ref=10.0)
    whole = _call(ctx, RINGS, 7, 8, values=vals, **kw)
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        part = make_context(capi, {k: v[lo:hi] for k, v in gas.items()}, sinks)
        parts.append(_call(part, RINGS, 7, 8, values=vals[:, lo:hi], **kw))
        part.close()
    assert parts[0]["exp"] == parts[1]["exp"] == whole["exp"]
    assert np.array_equal(modes.add_raw(parts[0]["raw_ring"], parts[1]["raw_ring"]), whole["raw_ring"])
    assert np.array_equal(modes.add_raw(parts[0]["raw_spiral"], parts[1]["raw_spiral"]), whole["raw_spiral"])
    assert np.array_equal(parts[0]["ring_counts"] + parts[1]["ring_counts"], whole["ring_counts"])
    assert tuple(np.add(parts[0]["counts"], parts[1]["counts"])) == whole["counts"]
    added = (modes.add_raw(parts[0]["raw_ring"], parts[1]["raw_ring"]), modes.add_raw(parts[0]["raw_spiral"], parts[1]["raw_spiral"]))
    back = capi.modes_finish(ctx.modes_desc, whole["exp"], added)
    assert np.array_equal(back[0], whole["ring"]) and np.array_equal(back[1], whole["spiral"])


# ---- the edges of the selection ---------------------------------------------------------------------------------------------------------
def test_selection_edges_and_counts(capi):
    c = np.array([0.5, -0.25, 0.125])                                # the sink's place: every difference below is exact
    rel = np.array([[1.0, 0.0, 0.0],                                 # 0  R == r_min: inside, ring 0
                    [0.0, 3.0, 0.0],                                 # 1  R on an inner edge: the upper ring
                    [-5.0, 0.0, 0.0],                                # 2  R == r_max: outside
                    [2.5, 0.0, 0.75],                                # 3  |z'| == z_max: outside
                    [0.0, -2.5, -0.5],                               # 4  inside, ring 1
                    [1.5, 0.0, 0.0],                                 # 5  a NaN quantity: not usable
                    [0.0, 0.0, 0.0],                                 # 6  R == 0: outside while r_min > 0
                    [np.nan, 1.0, 0.0],                              # 7  a NaN position: not usable
                    [1.5, 0.0, 0.0], [0.0, 3.5, 0.0]])               # 8, 9  ghosts
    m = 2.0 ** -np.arange(10.0)
    vx = np.array([1.0, -2.0, 1.0, 1.0, 3.0, np.nan, 0.5, 1.0, 1.0, 1.0])
    gas = _gas(rel + c, m, vx)
    sinks = {"x": c[:1], "y": c[1:2], "z": c[2:], "vx": np.zeros(1), "vy": np.zeros(1), "vz": np.zeros(1), "m": np.ones(1)}
    ctx = make_context(capi, gas, sinks, n_owned=8)
    kw = dict(sink=0, z_max=0.75, q="vx", spiral=(-1.0, 1.0, 3), r_ref=2.0)
    got = _call(ctx, (1.0, 5.0), 4, 2, **kw)
    _same_rings(got, _want(capi, ctx, gas, tuple(c), n_owned=8))
    assert got["counts"] == (3, 3, 2, 0) and got["ring_counts"].tolist() == [1, 1, 1, 0]
    assert got["ring"][0, :, 0].tolist() == [1.0, 1.0, 1.0] and got["ring"][2, 1].tolist() == [0.0, -1.0]      # w = m vx
    assert got["ring"][1, 0].tolist() == [3.0 / 16, 0.0] and got["ring"][1, 1].tolist() == [0.0, -3.0 / 16]
    # r_min = 0: the particle at the centre enters ring 0 with c = 1, s = 0 for every m, not the spiral sums
    got = _call(ctx, (0.0, 4.0), 4, 2, **kw)
    want = _want(capi, ctx, gas, tuple(c), n_owned=8)
    _same_rings(got, want)
    assert got["counts"] == (4, 2, 2, 1) and got["ring_counts"].tolist() == [1, 1, 1, 1]
    assert got["ring"][0].tolist() == [[0.5 / 64, 0.0]] * 3
    l0 = 1                                                           # p = 0: CS[0] = sum w over the three with R > 0
    assert got["spiral"][0, l0].tolist() == [1.0 - 1.0 + 3.0 / 16, 0.0]
    err = np.abs(got["spiral"] - want["spiral"])
    assert np.all(err <= modes_ref.spiral_bound(want["ws"], want["u"], 2, [-1.0, 0.0, 1.0])[:, :, None])
    # without the quantity nobody is dropped for it; the same set from an explicit centre
    got = _call(ctx, (1.0, 5.0), 4, 2, centre=tuple(c), z_max=0.75)
    _same_rings(got, _want(capi, ctx, gas, tuple(c), n_owned=8))
    assert got["counts"] == (4, 3, 1, 0) and got["ring_counts"].tolist() == [2, 1, 1, 0]
    ctx.close()


# ---- chunking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_r,m_max", [(1024, 8), (1, 0), (161, 8), (162, 8)])
def test_ring_histogram_in_chunks(capi, disc, n_r, m_max):
    """1024 rings of 19 accumulators do not fit the LDS histogram (3072): seven chunks.  161 rings are the largest single
    chunk at m_max = 8 and 162 the smallest two; one ring with m_max = 0 is the smallest call."""
    ctx, gas, sinks, centre, rows = disc
    got = _call(ctx, RINGS, n_r, m_max, sink=0, q=capi.modes_row(0), values=rows)
    _same_rings(got, _want(capi, ctx, gas, centre, values=rows))
    assert got["ring_counts"].sum() == got["counts"][0] > 2000


# ---- spiral sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spiral", [(-32.0, 32.0, 129), (5.0, 9.0, 1), (-3.0, 3.0, 64), (-3.0, 3.0, 65)])
def test_spiral_sums_within_the_bound_of_the_longdouble_sums(capi, disc, spiral):
    """For every (m, l): |delta| <= sum_j |w_j| (2 |p_l u_j| + 2 m + 8) 2^-53: one rounding of theta, one
    ulp of log carried into theta, two ulps of sincos, 2 m roundings of the recurrence and the combination.  129 wavenumbers
    take three wavefronts per block, 64 and 65 are the two sides of a wavefront's edge."""
    ctx, gas, sinks, centre, rows = disc
    got = _call(ctx, RINGS, 7, 8, log=True, sink=0, q=capi.modes_row(1), values=rows, spiral=spiral, r_ref=10.0)
    want = _want(capi, ctx, gas, centre, values=rows)
    _same_rings(got, want)
    p = capi.modes_tables(ctx.modes_desc)[1]
    ring, truth = modes_ref.truth(_pos(gas), want["w"], want["sel"], capi.modes_tables(ctx.modes_desc)[0], 8, p, centre=centre, r_ref=10.0)
    bound = modes_ref.spiral_bound(want["ws"], want["u"], 8, p)
    err = np.abs(got["spiral"].astype(np.longdouble) - truth).max(axis=2).astype(np.float64)
    print("worst spiral error / bound", float(np.max(err / bound)))
    assert err.shape == bound.shape == (9, spiral[2]) and np.all(err <= bound)
    for v, limbs in zip(got["spiral"].reshape(-1)[::7], got["raw_spiral"].reshape(-1, 2)[::7]):
        assert modes_ref.finish_int(modes_ref.from_limbs(*limbs), got["exp"]) == v


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(capi, disc):
    ctx, gas, sinks, centre, rows = disc
    lib, n = capi.load(), gas["x"].size
    good = dict(r_range=(10.5, 36.0), n_r=4, m_max=3, q=capi.modes_row(1), n_rows=2, spiral=(-2.0, 2.0, 5), r_ref=10.0, sink=0)
    n_out = 2 * 4 * (4 + 5)

    def run(d, values=rows, n_out=n_out, null_sums=False):
        sums, raw = np.full(n_out + 8, 7.25), np.full((n_out + 8, 2), 77, dtype=np.uint64)
        ex, rc, cnt = np.full(1, 55, dtype=np.int32), np.full(8, 66, dtype=np.int64), np.full(4, 44, dtype=np.int64)
        st = lib.sph_modes(ctx._h, C.byref(d), None if values is None else values.ctypes.data, None if null_sums else sums.ctypes.data,
                           n_out, raw.ctypes.data, ex.ctypes.data, rc.ctypes.data, cnt.ctypes.data)
        clean = np.all(sums == 7.25) and np.all(raw == 77) and ex[0] == 55 and np.all(rc == 66) and np.all(cnt == 44)
        return st, bool(clean)

    def edit(**fields):
        dd = capi.modes_desc(**good)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(dd, k)[v[0]] = v[1]
            else:
                setattr(dd, k, v)
        return dd

    st, clean = run(edit())
    assert st == 0 and not clean
    bad = {
        "n_r 0": edit(n_r=0), "n_r 1025": edit(n_r=1025), "m_max -1": edit(m_max=-1), "m_max 9": edit(m_max=9), "n_p -1": edit(n_p=-1),
        "n_p 257": edit(n_p=257), "r_min == r_max": edit(r_min=36.0), "r_min < 0": edit(r_min=-0.5), "r_min nan": edit(r_min=np.nan),
        "r_max inf": edit(r_max=np.inf), "log r_min 0": edit(r_min=0.0, flags=capi.MODES_LOG), "coinciding edges": edit(r_max=10.5 + 4e-15),
        "z_max nan": edit(z_max=np.nan), "normal zero": edit(normal=(2, 0.0)), "normal nan": edit(normal=(1, np.nan)),
        "centre nan": edit(sink=-1, centre=(0, np.nan)), "centre_v inf": edit(sink=-1, centre_v=(2, np.inf)), "sink -2": edit(sink=-2),
        "sink 1 of 1": edit(sink=1), "r_ref 0": edit(r_ref=0.0), "r_ref nan": edit(r_ref=np.nan), "p_min nan": edit(p_min=np.nan),
        "p_max inf": edit(p_max=np.inf), "p_min > p_max": edit(p_min=3.0), "n_q 2": edit(n_q=2), "field id": edit(q=19),
        "row id": edit(q=capi.modes_row(2)), "n_rows 17": edit(n_rows=17), "n_rows -1": edit(n_rows=-1), "flags": edit(flags=2),
        "reserved": edit(reserved=(1, 1)), "weight": edit(weight=2),
    }
    for name, dd in bad.items():
        assert run(dd) == (SPH_ERR_ARG, True), name
    assert run(edit(), n_out=n_out - 1) == (SPH_ERR_ARG, True) and run(edit(), n_out=n_out + 1) == (SPH_ERR_ARG, True)
    assert run(edit(), values=None) == (SPH_ERR_ARG, True)                               # values missing with n_rows > 0
    assert run(edit(n_q=0, n_rows=0)) == (SPH_ERR_ARG, True)                             # values given with n_rows == 0
    assert run(edit(), null_sums=True) == (SPH_ERR_ARG, True)
    assert lib.sph_modes(ctx._h, None, None, None, 0, None, None, None, None) == SPH_ERR_ARG
    assert run(edit(n_q=0, n_rows=0), values=None)[0] == 0


def test_a_stale_field_is_refused_and_the_context_is_left_alone(capi):
    gas, sinks = golden_gas("disc3000_eval")
    a, b = make_context(capi, gas, sinks), make_context(capi, gas, sinks, density=True)
    for q in ("rho", "P", "ax"):
        with pytest.raises(capi.SphError) as e:
            a.modes(RINGS, 4, 2, sink=0, q=q)
        assert e.value.status == SPH_ERR_STATE, q
    a.density()
    stats = a.stats()
    a.modes(RINGS, 4, 2, sink=0, q="rho", spiral=(-2.0, 2.0, 5))
    with pytest.raises(capi.SphError) as e:
        a.modes(RINGS, 4, 2, sink=0, q="ax")
    assert e.value.status == SPH_ERR_STATE
    after = a.stats()
    for k in ("grid_builds", "nlist_builds", "density_passes", "force_passes"):
        assert getattr(after, k) == getattr(stats, k), k
    assert a.step(1e-2) == b.step(1e-2)
    for f in ("x", "y", "z", "vx", "vy", "vz", "u", "alpha"):
        assert np.array_equal(a.field(f), b.field(f)), f
    a.close(); b.close()


def test_an_empty_context_and_an_empty_selection(capi, disc):
    ctx, gas, sinks, centre, rows = disc
    got = _call(ctx, (100.0, 200.0), 3, 2, sink=0, spiral=(-1.0, 1.0, 3))
    n = gas["x"].size
    assert got["counts"] == (0, n, 0, 0) and got["exp"] == 0 and not got["ring_counts"].any()
    assert not got["ring"].any() and not got["spiral"].any() and not got["raw_ring"].any() and not got["raw_spiral"].any()
    empty = capi.Context(device=0)
    got = _call(empty, (1.0, 2.0), 3, 2, spiral=(-1.0, 1.0, 3))
    assert got["counts"] == (0, 0, 0, 0) and got["exp"] == 0 and not got["ring"].any() and not got["raw_spiral"].any()
    empty.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip(capi, tmp_path, capsys):
    import json
    from summersph_amd import txtio
    from summersph_amd.cli import read_save, uploaded_context
    gas, sinks = golden_gas("disc3000_eval")
    rows = np.stack([gas[k] for k in "x y z vx vy vz u m alpha".split()], axis=1)
    ns = np.size(sinks["m"])
    srows = np.stack([np.reshape(sinks[k], ns) for k in ("x", "y", "z", "vx", "vy", "vz")] + [np.zeros(ns), np.reshape(sinks["m"], ns)], axis=1)
    save, out = tmp_path / "save.txt", tmp_path / "modes.npz"
    txtio.write_save(str(save), rows, srows)
    assert modes.main([str(save), "-o", str(out), "--rings", "10.5", "36", "7", "--log", "--mmax", "4", "--spiral", "-8", "8", "33",
                       "--rref", "10", "--sink", "0", "--json"]) == 0
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    z = np.load(out)
    g2, s2 = read_save(str(save))                                       # what the tool uploaded
    with uploaded_context(g2, s2) as ctx:
        ring, spiral, rc, counts, exp, raw = ctx.modes(RINGS, 7, 4, log=True, sink=0, spiral=(-8.0, 8.0, 33), r_ref=10.0, raw=True)
        edges, p = capi.modes_tables(ctx.modes_desc)
    assert np.array_equal(z["ring"], ring) and np.array_equal(z["spiral"], spiral) and np.array_equal(z["raw_ring"], raw[0])
    assert np.array_equal(z["raw_spiral"], raw[1]) and int(z["exp"]) == exp and np.array_equal(z["ring_counts"], rc)
    assert tuple(z["counts"]) == counts and np.array_equal(z["edges"], edges) and np.array_equal(z["p"], p)
    f = modes.finish(ring, spiral, p)
    assert np.array_equal(z["A"], f["A"]) and np.array_equal(z["spectrum"], f["spectrum"]) and z["pitch"].shape == (5,)
    assert info["selected"] == counts[0] > 2000 and info["n_p"] == 33 and 1 <= info["m_peak"] <= 4 and int(z["desc_n_r"]) == 7
