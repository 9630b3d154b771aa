"""What capi.Context's fourteen analysis methods hand to the C ABI, and what the command-line parsers accept: pinned
without a library or a GPU.

A Context is made without __init__ around a recording stub of the library: every symbol is a callable that records
(name, args), returns 0 (sph_count: N, sph_stream: 0) and writes fixed values through the int64 count pointers, so the
return paths run.  The host form of every method is checked argument by argument -- the symbol, every integer, the
address (or None) of every pointer against the arrays the method returns -- with the shapes, dtypes and types of what
comes back and the descriptor left on the context.  Every ValueError of the marshalling is pinned with its text; those
of the device forms that are raised before anything touches a GPU are pinned too.  The second half pins parse_clip,
parse_fields, parse_vec and read_save in every module that exports them.
"""
import ctypes as C

import numpy as np
import pytest

from summersph_amd import capi

N, M = 7, 5
HANDLE = 0x5150
# symbol -> ((argument index, values written through it), ...): the int64 count outputs
COUNT_OUT = {
    "sph_groups": ((6, [3]),), "sph_peaks": ((6, [3, 9, 11]),), "sph_gradients": ((6, [6]), (7, [1])),
    "sph_sample": ((10, [4, 1]),), "sph_trace": ((12, [1, 2, 0, 1, 1]),), "sph_gravity_at": ((9, [2, 1]),),
    "sph_bound": ((9, [5, 0, 1, 0]),), "sph_binned": ((6, [6, 1, 0]),),
}
QUIET = ("sph_count", "sph_stream", "sph_ctx_destroy")


def addr(p):
    """the address a pointer argument carries: None, an int, a c_void_p, a ctypes object or byref() of one"""
    if p is None or isinstance(p, int):
        return p
    if isinstance(p, C.c_void_p):
        return p.value
    if hasattr(p, "_obj"):
        return C.addressof(p._obj)
    return C.addressof(p)


class StubLib:
    def __init__(self):
        self.calls = []
        self.peek = {}          # symbol -> {argument index: doubles to copy at call time}
        self.peeked = {}

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "sph_count":
                return N
            if name == "sph_energy":                                # finite sums for energy_total
                (C.c_double * capi.ENERGY_NSUM).from_address(addr(args[2]))[:] = [1.0] * capi.ENERGY_NSUM
            for k, vals in COUNT_OUT.get(name, ()):
                (C.c_int64 * len(vals)).from_address(addr(args[k]))[:] = vals
            for k, cnt in self.peek.get(name, {}).items():
                if args[k] is not None:
                    self.peeked[k] = np.array((C.c_double * cnt).from_address(addr(args[k]))[:])
            return 0
        return fn

    def one(self, name):
        """the arguments of the only call that is not bookkeeping; it must be `name`"""
        calls = [c for c in self.calls if c[0] not in QUIET]
        assert [c[0] for c in calls] == [name]
        return calls[0][1]


@pytest.fixture
def ctx():
    c = capi.Context.__new__(capi.Context)
    c.device = 0
    c.params = capi.Params()
    c._h = C.c_void_p(HANDLE)
    c.lib = StubLib()
    return c


def is_f64(a, shape):
    return isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == tuple(shape) and a.flags["C_CONTIGUOUS"]


def three_points():
    rng = np.random.default_rng(5)
    return [np.ascontiguousarray(rng.random(M)) for _ in range(3)]


# ---- the host forms ----------------------------------------------------------------------------------------------------
def test_render_density(ctx):
    out = ctx.render_density((2, 3, 4), bounds=((0, 0, 0), (1, 2, 3)))
    a = ctx.lib.one("sph_render_density")
    assert addr(a[0]) == HANDLE and len(a) == 4
    assert is_f64(out, (2, 3, 4)) and addr(a[2]) == out.ctypes.data and a[3] == 24
    d = a[1]._obj
    assert isinstance(d, capi.RenderDesc) and tuple(d.n) == (2, 3, 4) and d.axis == -1 and d.flags == 0
    lo, hi = ctx.render_bounds
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [1, 2, 3]
    ctx.lib.calls.clear()
    out = ctx.render_density(4, axis="y", spacing=True)
    a = ctx.lib.one("sph_render_density")
    assert is_f64(out, (4, 4)) and a[3] == 16 and a[1]._obj.axis == 1
    assert a[1]._obj.flags == capi.RENDER_AUTO_BOUNDS | capi.RENDER_SPACING


def test_render_field(ctx):
    out = ctx.render_field("u", (2, 3, 4), axis=2, normalise=True)
    a = ctx.lib.one("sph_render_field")
    assert addr(a[0]) == HANDLE and len(a) == 6
    d = a[1]._obj
    assert isinstance(d, capi.RenderFieldDesc) and d.field == capi.FIELDS.index("u") and d.normalise == 1 and d.weight == 0
    assert is_f64(out, (2, 3)) and a[2] is None and addr(a[3]) == out.ctypes.data and a[4] is None and a[5] == 6
    assert len(ctx.render_bounds) == 2
    ctx.lib.calls.clear()
    vals = np.arange(N, dtype=np.float64)
    res = ctx.render_field(vals, 3, weight="volume", weight_out=True)
    a = ctx.lib.one("sph_render_field")
    assert isinstance(res, tuple) and is_f64(res[0], (3, 3, 3)) and is_f64(res[1], (3, 3, 3))
    assert a[1]._obj.field == capi.RENDER_FIELD_VALUES and a[1]._obj.weight == capi.RENDER_WEIGHT_VOLUME
    assert addr(a[2]) == vals.ctypes.data and addr(a[3]) == res[0].ctypes.data and addr(a[4]) == res[1].ctypes.data
    assert a[5] == 27


def test_profile(ctx):
    table, sums = ctx.profile(1.0, 5.0, 4, n_phi=2, log=True, normal="auto")
    a = ctx.lib.one("sph_profile")
    assert addr(a[0]) == HANDLE and len(a) == 5 and a[4] == 8
    assert addr(a[1]) == C.addressof(ctx.profile_desc) and isinstance(ctx.profile_desc, capi.ProfileDesc)
    assert ctx.profile_desc.flags == capi.PROFILE_LOG | capi.PROFILE_AUTO_NORMAL and ctx.profile_desc.sink == -1
    assert is_f64(sums, (8, capi.PROFILE_NSUM)) and addr(a[2]) == sums.ctypes.data
    assert table.shape == (8,) and table.dtype.names == tuple(capi.PROFILE_COLUMNS) and addr(a[3]) == table.ctypes.data
    ctx.lib.calls.clear()
    table, sums = ctx.profile(1.0, 5.0, 4, sink=1, sums_only=True)
    a = ctx.lib.one("sph_profile")
    assert table is None and a[3] is None and is_f64(sums, (4, capi.PROFILE_NSUM)) and ctx.profile_desc.sink == 1


def test_energy(ctx):
    out = ctx.energy(src_offset=3)
    a = ctx.lib.one("sph_energy")
    assert addr(a[0]) == HANDLE and len(a) == 5 and a[1] == 3 and a[3] is None and a[4] == N
    assert is_f64(out["sums"], (capi.ENERGY_NSUM,)) and addr(a[2]) == out["sums"].ctypes.data and "phi" not in out
    assert set(capi.ENERGY_SUMS) | {"E", "P", "L", "com", "sums"} == set(out) and out["E"] == 6.0 and out["M"] == 1.0
    ctx.lib.calls.clear()
    out = ctx.energy(phi=True)
    a = ctx.lib.one("sph_energy")
    assert a[1] == 0 and is_f64(out["phi"], (N,)) and addr(a[3]) == out["phi"].ctypes.data


@pytest.mark.parametrize("which", ["groups", "peaks"])
def test_groups_and_peaks(ctx, which):
    ncol = capi.GROUPS_NCOL if which == "groups" else capi.PEAKS_NCOL
    cols = capi.GROUPS_COLUMNS if which == "groups" else capi.PEAKS_COLUMNS
    call = getattr(ctx, which)

    def returned(res):
        if which == "groups":
            assert len(res) == 3
        else:
            assert len(res) == 4 and res[3] == (3, 9, 11) and all(type(v) is int for v in res[3])
        assert res[2] == 3 and type(res[2]) is int
        return res[0], res[1]

    lab, tab = returned(call(0.5, rho_min=2.0, min_members=4, link_h=True, clip=((0, 0, 0), (1, 1, 1))))
    a = ctx.lib.one("sph_" + which)
    d = getattr(ctx, which + "_desc")
    assert addr(a[0]) == HANDLE and len(a) == 7 and addr(a[1]) == C.addressof(d)
    assert d.link == 0.5 and d.rho_min == 2.0 and d.min_members == 4 and d.flags == 1 and list(d.clip_hi) == [1, 1, 1]
    assert isinstance(lab, np.ndarray) and lab.dtype == np.int32 and lab.shape == (N,) and addr(a[2]) == lab.ctypes.data
    assert a[3] == N and a[5] == N and addr(a[6]) is not None
    assert tab.shape == (3,) and tab.dtype.names == tuple(cols) and addr(a[4]) == tab.ctypes.data      # min(3, N) rows
    ctx.lib.calls.clear()
    lab, tab = returned(call(0.5, max_groups=2, labels=False))
    a = ctx.lib.one("sph_" + which)
    assert lab is None and a[2] is None and a[5] == 2 and tab.shape == (2,) and tab.itemsize == 8 * ncol
    ctx.lib.calls.clear()
    lab, tab = returned(call(0.5, max_groups=0))
    a = ctx.lib.one("sph_" + which)
    assert tab is None and a[4] is None and a[5] == 0 and lab.shape == (N,)


def test_gradients(ctx):
    g, rho, counts = ctx.gradients()
    a = ctx.lib.one("sph_gradients")
    d = ctx.gradients_desc
    assert addr(a[0]) == HANDLE and len(a) == 8 and addr(a[1]) == C.addressof(d)
    assert d.n_fields == 3 and list(d.fields)[:3] == [3, 4, 5] and d.flags == capi.GRAD_CORRECTED and d.h == 0.0
    assert a[2] is None and is_f64(g, (3, 3, N)) and addr(a[3]) == g.ctypes.data and a[4] == 9 * N
    assert rho is None and a[5] is None and counts == (6, 1) and all(type(v) is int for v in counts)
    ctx.lib.calls.clear()
    ctx.lib.peek["sph_gradients"] = {2: 2 * N}
    vals = np.arange(N, dtype=np.float64)
    g, rho, counts = ctx.gradients(fields=(capi.GRAD_VALUES, "rho"), values=vals, corrected=False, h=0.7, rho=True)
    a = ctx.lib.one("sph_gradients")
    assert is_f64(g, (2, 3, N)) and a[4] == 6 * N and is_f64(rho, (N,)) and addr(a[5]) == rho.ctypes.data
    assert ctx.gradients_desc.flags == 0 and ctx.gradients_desc.h == 0.7
    assert ctx.lib.peeked[2].tolist() == vals.tolist() + [0.0] * N          # the row no field reads is zero-padded
    ctx.lib.calls.clear()
    two = np.arange(2.0 * N).reshape(2, N)
    ctx.gradients(fields=(capi.GRAD_VALUES, capi.GRAD_VALUES), values=two)
    assert addr(ctx.lib.one("sph_gradients")[2]) == two.ctypes.data


def test_sample(ctx):
    p = three_points()
    out = ctx.sample(p, fields=("rho", "u"), normalise=True, h=0.3)
    a = ctx.lib.one("sph_sample")
    d = ctx.sample_desc
    assert addr(a[0]) == HANDLE and len(a) == 11 and addr(a[1]) == C.addressof(d) and a[2] == M
    assert d.n_fields == 2 and d.flags == capi.SAMPLE_NORMALISE and d.h == 0.3 and d.weight == capi.RENDER_WEIGHT_MASS
    assert [addr(a[k]) for k in (3, 4, 5)] == [t.ctypes.data for t in p]
    assert a[6] is None and is_f64(out, (2, M)) and addr(a[7]) == out.ctypes.data and a[8] == 2 * M and a[9] is None
    assert addr(a[10]) is not None
    ctx.lib.calls.clear()
    pts = np.arange(3.0 * M).reshape(M, 3)
    ctx.lib.peek["sph_sample"] = {3: M, 4: M, 5: M, 6: N}
    vals = np.arange(N, dtype=np.float64)
    res = ctx.sample(pts, fields=(capi.SAMPLE_VALUES,), values=vals, weight="volume", weight_out=True, counts=True)
    a = ctx.lib.one("sph_sample")
    assert [ctx.lib.peeked[3 + k].tolist() for k in range(3)] == [pts[:, k].tolist() for k in range(3)]
    assert ctx.lib.peeked[6].tolist() == vals.tolist() and ctx.sample_desc.weight == capi.RENDER_WEIGHT_VOLUME
    assert isinstance(res, tuple) and len(res) == 3 and is_f64(res[0], (1, M)) and is_f64(res[1], (M,)) and res[2] == (4, 1)
    assert addr(a[7]) == res[0].ctypes.data and addr(a[9]) == res[1].ctypes.data and a[8] == M
    ctx.lib.calls.clear()
    res = ctx.sample(pts, fields=("u",), counts=True)
    assert isinstance(res, tuple) and len(res) == 2 and is_f64(res[0], (1, M)) and res[1] == (4, 1)
    assert ctx.lib.one("sph_sample")[9] is None
    ctx.lib.calls.clear()
    w = ctx.sample(pts, fields=())                                   # the weight alone
    a = ctx.lib.one("sph_sample")
    assert is_f64(w, (M,)) and a[7] is None and a[8] == 0 and addr(a[9]) == w.ctypes.data and ctx.sample_desc.n_fields == 0
    ctx.lib.calls.clear()
    res = ctx.sample(pts, fields=(), weight_out=True, counts=True)
    assert len(res) == 3 and is_f64(res[0], (0, M)) and is_f64(res[1], (M,)) and res[2] == (4, 1)


def test_trace(ctx):
    p = three_points()
    res = ctx.trace(p, 4, 0.1, stride=2)
    a = ctx.lib.one("sph_trace")
    d = ctx.trace_desc
    assert addr(a[0]) == HANDLE and len(a) == 13 and addr(a[1]) == C.addressof(d) and a[2] == M
    assert d.n_steps == 4 and d.stride == 2 and d.ds == 0.1 and d.carry == capi.TRACE_NONE and d.flags == 0
    assert [addr(a[k]) for k in (3, 4, 5)] == [t.ctypes.data for t in p] and a[6] is None
    path, status, done = res
    assert is_f64(path, (3, 3, M)) and addr(a[7]) == path.ctypes.data and a[8] == 9 * M and a[9] is None
    for k, t in ((10, status), (11, done)):
        assert isinstance(t, np.ndarray) and t.dtype == np.int32 and t.shape == (M,) and addr(a[k]) == t.ctypes.data
    assert addr(a[12]) is not None
    ctx.lib.calls.clear()
    ctx.lib.peek["sph_trace"] = {6: 4 * N}
    vals = np.arange(2.0 * N).reshape(2, N)
    res = ctx.trace(np.zeros((M, 3)), 4, -0.1, fields=("vx", capi.TRACE_VALUES, "vz"), values=vals, carry=capi.TRACE_VALUES,
                    arclength=True, normal=(0, 0, 1), counts=True)
    a = ctx.lib.one("sph_trace")
    assert len(res) == 5 and is_f64(res[0], (5, 3, M)) and is_f64(res[3], (5, M)) and addr(a[9]) == res[3].ctypes.data
    assert res[4] == (1, 2, 0, 1, 1) and all(type(v) is int for v in res[4]) and a[8] == 15 * M
    assert ctx.trace_desc.flags == capi.TRACE_ARCLENGTH | capi.TRACE_PLANAR
    assert ctx.lib.peeked[6].tolist() == vals.reshape(-1).tolist() + [0.0] * (2 * N)      # carry reads row 3: four rows


def test_cube(ctx):
    out = ctx.cube((2, 3), ((-1, -1), (1, 1)), 0.0, 0.5, 4, per_velocity=True)
    a = ctx.lib.one("sph_cube")
    d = ctx.cube_desc
    assert addr(a[0]) == HANDLE and len(a) == 5 and addr(a[1]) == C.addressof(d)
    assert (d.n_u, d.n_v, d.n_chan, d.flags) == (2, 3, 4, capi.CUBE_PER_VELOCITY) and d.dv == 0.5
    assert a[2] is None and is_f64(out, (4, 2, 3)) and addr(a[3]) == out.ctypes.data and a[4] == 24
    ctx.lib.calls.clear()
    vals = np.arange(N, dtype=np.float64)
    out = ctx.cube(2, ((-1, -1), (1, 1)), 0.0, 0.5, 0, values=vals)
    a = ctx.lib.one("sph_cube")
    assert addr(a[2]) == vals.ctypes.data and is_f64(out, (0, 2, 2)) and a[4] == 0


def test_force_terms(ctx):
    out = ctx.force_terms(skip_gas_gravity=True)
    a = ctx.lib.one("sph_force_terms")
    assert addr(a[0]) == HANDLE and len(a) == 4 and isinstance(a[1]._obj, capi.ForceTermsDesc)
    assert a[1]._obj.flags == capi.TERMS_SKIP_GAS_GRAVITY
    assert is_f64(out, (capi.TERMS_NROW, N)) and addr(a[2]) == out.ctypes.data and a[3] == capi.TERMS_NROW * N
    ctx.lib.calls.clear()
    ctx.force_terms(refresh=True)
    assert [c[0] for c in ctx.lib.calls if c[0] not in QUIET] == ["sph_density", "sph_force_terms"]
    assert ctx.lib.calls[-1][1][1]._obj.flags == 0


def test_binned(ctx):
    sums, counts = ctx.binned("x", 8, ranges=(0.0, 1.0), q=("u", "vx"), squares=True)
    a = ctx.lib.one("sph_binned")
    d = ctx.binned_desc
    assert addr(a[0]) == HANDLE and len(a) == 7 and addr(a[1]) == C.addressof(d)
    assert (d.n_axes, d.n_q, d.n_rows, d.n[0], d.n[1]) == (1, 2, 0, 8, 1) and d.weight == capi.BINNED_W_MASS
    assert d.flags == capi.BINNED_SQUARES | capi.BINNED_SKIP_NAN
    assert a[2] is None and a[3] is None and is_f64(sums, (8, 1, 6)) and addr(a[4]) == sums.ctypes.data and a[5] == 48
    assert counts == (6, 1, 0) and all(type(v) is int for v in counts)
    ctx.lib.calls.clear()
    ctx.lib.peek["sph_binned"] = {3: 4 + 3}
    vals = np.arange(2.0 * N).reshape(2, N)
    ex, ey = np.linspace(0, 1, 4), np.array([1.0, 2.0, 4.0])
    sums, counts = ctx.binned((capi.binned_row(0), "y"), (3, 2), edges=(ex, ey), q=capi.binned_row(1), weight="one", values=vals,
                              skip_nan=False)
    a = ctx.lib.one("sph_binned")
    assert ctx.binned_desc.n_rows == 2 and ctx.binned_desc.flags == capi.BINNED_EDGES0 | capi.BINNED_EDGES1
    assert addr(a[2]) == vals.ctypes.data and ctx.lib.peeked[3].tolist() == ex.tolist() + ey.tolist()
    assert is_f64(sums, (3, 2, 3)) and a[5] == 18
    ctx.lib.calls.clear()
    one = np.arange(N, dtype=np.float64)
    ctx.binned(capi.binned_row(0), 2, ranges=(0, 1), values=one)
    assert ctx.binned_desc.n_rows == 1 and addr(ctx.lib.one("sph_binned")[2]) == one.ctypes.data


def test_gravity_at(ctx):
    p = three_points()
    res = ctx.gravity_at(p, h=0.2, sinks=False)
    a = ctx.lib.one("sph_gravity_at")
    d = ctx.gravity_at_desc
    assert addr(a[0]) == HANDLE and len(a) == 10 and addr(a[1]) == C.addressof(d) and a[2] == M
    assert d.h == 0.2 and d.flags == capi.GRAVAT_GAS and d.soft2 == capi.GRAVAT_REF_SOFT2
    assert [addr(a[k]) for k in (3, 4, 5)] == [t.ctypes.data for t in p] and a[6] is None and a[8] == 4 * M
    phi, acc = res
    assert phi.shape == (M,) and acc.shape == (3, M) and phi.dtype == acc.dtype == np.float64
    assert addr(a[7]) == phi.ctypes.data and acc.ctypes.data == phi.ctypes.data + 8 * M and addr(a[9]) is not None
    ctx.lib.calls.clear()
    ph = np.full(M, 0.1)
    phi, acc, cn = ctx.gravity_at(np.zeros((M, 3)), ph=ph, split=True, counts=True)
    a = ctx.lib.one("sph_gravity_at")
    assert addr(a[6]) == ph.ctypes.data and a[8] == 8 * M and cn == (2, 1) and all(type(v) is int for v in cn)
    assert phi.shape == (2, M) and acc.shape == (2, 3, M) and addr(a[7]) == phi.ctypes.data
    assert ctx.gravity_at_desc.flags == capi.GRAVAT_GAS | capi.GRAVAT_SINKS | capi.GRAVAT_SPLIT


def test_bound(ctx):
    labels = np.array([0, 0, 1, -1, 1, 0, 2], dtype=np.int32)
    bl, e, phi, tab, counts = ctx.bound(labels, 3, thermal=True, max_rounds=5, min_members=2)
    a = ctx.lib.one("sph_bound")
    d = ctx.bound_desc
    assert addr(a[0]) == HANDLE and len(a) == 10 and addr(a[1]) == C.addressof(d)
    assert (d.flags, d.max_rounds, d.min_members, d.max_members) == (capi.BOUND_THERMAL, 5, 2, 2**31 - 1)
    assert addr(a[2]) == labels.ctypes.data and a[3] == N and a[4] == 3 and a[7] == 2 * N
    assert isinstance(bl, np.ndarray) and bl.dtype == np.int32 and bl.shape == (N,) and addr(a[5]) == bl.ctypes.data
    assert e.shape == phi.shape == (N,) and addr(a[6]) == e.ctypes.data and phi.ctypes.data == e.ctypes.data + 8 * N
    assert tab.shape == (3,) and tab.dtype.names == tuple(capi.BOUND_COLUMNS) and addr(a[8]) == tab.ctypes.data
    assert counts == (5, 0, 1, 0) and all(type(v) is int for v in counts)
    ctx.lib.calls.clear()
    ctx.bound(labels.astype(np.int64), 0)
    a = ctx.lib.one("sph_bound")
    assert a[3] == N and a[4] == 0 and addr(a[2]) != labels.ctypes.data


# ---- the marshalling's ValueErrors -------------------------------------------------------------------------------------
def raises(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text
    return True


def test_point_errors(ctx):
    bad = np.zeros((M, 2))
    short = [np.zeros(M), np.zeros(M), np.zeros(M - 1)]
    assert raises("sample: points must be an (M, 3) array or three arrays", ctx.sample, bad)
    assert raises("sample: the three point arrays differ in length", ctx.sample, short)
    assert raises("trace: seeds must be an (M, 3) array or three arrays", ctx.trace, bad, 4, 0.1)
    assert raises("trace: the three seed arrays differ in length", ctx.trace, short, 4, 0.1)
    assert raises("gravity_at: points must be an (M, 3) array or three arrays", ctx.gravity_at, np.zeros(M))
    assert raises("gravity_at: the three point arrays differ in length", ctx.gravity_at, short)
    assert raises(f"gravity_at: ph has 3 values for {M} points", ctx.gravity_at, np.zeros((M, 3)), ph=np.zeros(3))
    assert not [c for c in ctx.lib.calls if c[0] not in QUIET]


def test_values_errors(ctx):
    pts, rows = np.zeros((M, 3)), np.zeros((2, 3))
    assert raises(f"gradients: values rows of 3 for {N} particles", ctx.gradients, fields=(capi.GRAD_VALUES,), values=rows)
    assert raises(f"sample: values rows of 3 for {N} particles", ctx.sample, pts, fields=(capi.SAMPLE_VALUES,), values=rows)
    assert raises(f"trace: values rows of 3 for {N} particles", ctx.trace, pts, 4, 0.1, fields=(capi.TRACE_VALUES, "vy", "vz"),
                  values=np.zeros(3))
    assert raises(f"binned: values rows of 3 for {N} particles", ctx.binned, capi.binned_row(0), 2, ranges=(0, 1), values=rows)
    assert raises(f"cube: 3 values for {N} particles", ctx.cube, 2, ((0, 0), (1, 1)), 0.0, 1.0, 2, values=np.zeros(3))
    assert raises(f"render_field: 3 values for {N} particles", ctx.render_field, np.zeros(3), 4)
    assert raises("render_field: a numpy values array renders with device=False", ctx.render_field, np.zeros(N), 4, device=True)
    assert raises("trace: n_steps >= 1 and stride >= 1 dividing n_steps", ctx.trace, pts, 4, 0.1, stride=3)
    assert raises("trace: n_steps >= 1 and stride >= 1 dividing n_steps", ctx.trace, pts, 0, 0.1)
    assert not [c for c in ctx.lib.calls if c[0] not in QUIET]


def test_device_form_errors_raised_before_the_gpu(ctx):
    """the device forms refuse host arrays before they allocate anything"""
    import torch
    pts = np.zeros((M, 3))
    gpu = "on the context's GPU"
    assert raises(f"sample: device points must be an (M, 3) or three contiguous float64 tensors {gpu}", ctx.sample, pts, device=True)
    assert raises(f"trace: device seeds must be an (M, 3) or three contiguous float64 tensors {gpu}", ctx.trace, pts, 4, 0.1,
                  device=True)
    assert raises(f"gravity_at: device points (and ph) must be contiguous float64 tensors {gpu}", ctx.gravity_at, pts, device=True)
    assert raises(f"gradients: device values must be a contiguous float64 tensor {gpu}", ctx.gradients,
                  fields=(capi.GRAD_VALUES,), values=np.zeros(N), device=True)
    assert raises(f"binned: device values must be a contiguous float64 tensor {gpu}", ctx.binned, capi.binned_row(0), 2,
                  ranges=(0, 1), values=np.zeros(N), device=True)
    assert raises(f"cube: device values must be a contiguous float64 tensor of sph_count() {gpu}", ctx.cube, 2, ((0, 0), (1, 1)),
                  0.0, 1.0, 2, values=np.zeros(N), device=True)
    assert raises(f"bound: device labels must be a contiguous int32 tensor of sph_count values {gpu}", ctx.bound,
                  np.zeros(N, dtype=np.int32), 1, device=True)
    assert raises(f"render_field: values must be float64 numpy or a contiguous float64 tensor {gpu}", ctx.render_field,
                  torch.zeros(N, dtype=torch.float64), 4)
    assert not [c for c in ctx.lib.calls if c[0] not in QUIET]


# ---- the command-line parsers and the save-file readers ---------------------------------------------------------------
def clip_error(spec):
    return f"--clip wants x0,y0,z0,x1,y1,z1 with x0 <= x1 ..., not {spec!r}"


@pytest.mark.parametrize("module", ["groups", "gradients", "sample", "trace", "peaks"])
def test_parse_clip(module):
    import importlib
    parse_clip = importlib.import_module("summersph_amd." + module).parse_clip
    assert parse_clip("0,1,2,3,4,5") == ((0.0, 1.0, 2.0), (3.0, 4.0, 5.0))
    assert parse_clip("-inf,0,0,inf,0,1e3") == ((-np.inf, 0.0, 0.0), (np.inf, 0.0, 1000.0))
    for spec in ("0,0,0,1,1", "0,0,0,1,1,nan", "0,0,2,1,1,1", "0,0,0,1,1,1,1"):
        assert raises(clip_error(spec), parse_clip, spec)
    with pytest.raises(ValueError):
        parse_clip("a,0,0,1,1,1")


def fields_error(count, spec, variable=False):
    allowed = [f for f in capi.FIELDS if variable or f not in ("h", "omega")]
    return f"--fields wants {count} comma-separated names of {allowed}, not {spec!r}"


def test_parse_fields():
    from summersph_amd import gradients, sample, trace
    assert gradients.parse_fields("vx,vy,vz") == ["vx", "vy", "vz"]
    assert gradients.parse_fields("rho") == ["rho"] and gradients.parse_fields("h,omega,u,m", True) == ["h", "omega", "u", "m"]
    for spec in ("", "x,y,z,u,m", "h", "vx,,vy", "nope"):
        assert raises(fields_error("1 .. 4", spec), gradients.parse_fields, spec)
    assert raises(fields_error("1 .. 4", "nope", True), gradients.parse_fields, "nope", True)
    assert sample.parse_fields("") == [] and sample.parse_fields("rho,,u,") == ["rho", "u"]
    assert sample.parse_fields("x,y,z,h", True) == ["x", "y", "z", "h"]
    for spec in ("x,y,z,u,m", "omega", "nope"):
        assert raises(fields_error("0 .. 4", spec), sample.parse_fields, spec)
    assert trace.parse_fields("vx,vy,vz") == ["vx", "vy", "vz"] and trace.parse_fields("ax,,ay,az") == ["ax", "ay", "az"]
    assert trace.parse_fields("x,y,h", True) == ["x", "y", "h"]
    for spec in ("", "vx,vy", "vx,vy,vz,u", "vx,vy,h", "vx,vy,nope"):
        assert raises(fields_error("three", spec), trace.parse_fields, spec)


@pytest.mark.parametrize("module", ["sample", "trace", "gravity"])
def test_parse_vec(module):
    import importlib
    parse_vec = importlib.import_module("summersph_amd." + module).parse_vec
    assert parse_vec("1,2.5,-3e2") == (1.0, 2.5, -300.0) and parse_vec("0,0,1", "--normal") == (0.0, 0.0, 1.0)
    assert raises("a vector wants three finite numbers x,y,z, not '1,2'", parse_vec, "1,2")
    assert raises("--centre wants three finite numbers x,y,z, not '1,2,inf'", parse_vec, "1,2,inf", "--centre")
    assert raises("--line wants three finite numbers x,y,z, not '1,2,nan'", parse_vec, "1,2,nan", what="--line")


def test_cube_keeps_its_own_lax_parsers():
    from summersph_amd import cube
    assert cube.parse_vec("1,2,3") == (1.0, 2.0, 3.0) and cube.parse_vec("1,inf", 2) == (1.0, np.inf)
    assert raises("'1,2': 3 comma-separated numbers", cube.parse_vec, "1,2")
    assert cube.parse_clip("0,0,2,1,1,1") == ((0.0, 0.0, 2.0), (1.0, 1.0, 1.0))        # lo > hi passes
    assert np.isnan(cube.parse_clip("0,0,0,1,1,nan")[1][2])
    assert raises("'0,0,0,1,1': 6 comma-separated numbers", cube.parse_clip, "0,0,0,1,1")


def test_read_save(tmp_path):
    from summersph_amd import profile, render
    gas = "1 2 3 4 5 6 7 8.5D-1 9"
    sink = "1 2 3 4 5 6 7 8"
    path = tmp_path / "save.txt"
    path.write_text(f"header line\n{gas}\n{sink}\n")
    g, s = profile.read_save(str(path))
    assert g.shape == (1, 9) and g.dtype == np.float64 and g[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 0.85, 9]
    assert s.shape == (1, 8) and s[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert raises(f"{path}: a record of 9 values", profile.read_save, str(path), variable=True)
    path.write_text(f"header line\n{gas} 10\n{sink}\n\n")
    g, s = profile.read_save(str(path), True)
    assert g.shape == (1, 10) and g[0, 9] == 10.0 and s.shape == (1, 8)
    assert raises(f"{path}: a record of 10 values", profile.read_save, str(path))
    # render's reader skips what it does not know, counts it, and reads no Fortran exponents
    g, s, skipped = render.read_save(str(path))
    assert g.shape == (0, 9) and s.shape == (1, 8) and skipped == 1
    path.write_text(f"header line\n{gas.replace('D', 'E')}\n{sink}\n")
    g, s, skipped = render.read_save(str(path))
    assert g.shape == (1, 9) and g[0, 7] == 0.85 and s.shape == (1, 8) and skipped == 0
    import importlib
    for module in ("groups", "gradients", "peaks"):                   # the modules that re-export the strict reader
        assert importlib.import_module("summersph_amd." + module).read_save is profile.read_save
