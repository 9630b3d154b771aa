"""What capi.Context.modes hands to the C ABI, pinned without a library or a GPU: a Context is made without __init__ around
a recording stub of the library (every symbol records (name, args), returns 0, sph_count: N, and writes fixed values through
the count, exponent and ring-count pointers, so the return paths run).  The host form is checked argument by argument
against the arrays the method returns; every ValueError of the marshalling is pinned with its text, those of the device form
that are raised before anything touches a GPU too."""
import ctypes as C

import numpy as np
import pytest

from summersph_amd import capi

N = 7
HANDLE = 0x5150
COUNTS = [5, 1, 1, 2]


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

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "sph_count":
                return N
            if name == "sph_modes":
                C.c_int32.from_address(addr(args[6])).value = -17
                n_r = args[1]._obj.n_r
                (C.c_int64 * n_r).from_address(addr(args[7]))[:] = list(range(n_r))
                (C.c_int64 * 4).from_address(addr(args[8]))[:] = COUNTS
            return 0
        return fn

    def one(self):
        calls = [c for c in self.calls if c[0] not in ("sph_count", "sph_stream", "sph_ctx_destroy")]
        assert [c[0] for c in calls] == ["sph_modes"]
        return calls[0][1]


@pytest.fixture
def ctx():
    c = capi.Context.__new__(capi.Context)
    c.device = 0
    c.params = capi.Params()
    c._h = C.c_void_p(HANDLE)
    c.lib = StubLib()
    return c


def base_of(a):
    """the array a view was cut from"""
    while a.base is not None:
        a = a.base
    return a


def test_rings_only(ctx):
    ring, spiral, rc, counts, exp = ctx.modes((10.0, 200.0), 40, 8, log=True, sink=0)
    a = ctx.lib.one()
    assert len(a) == 9 and addr(a[0]) == HANDLE and a[2] is None and a[4] == 2 * 9 * 40 and a[5] is None
    d = ctx.modes_desc
    assert addr(a[1]) == C.addressof(d) and isinstance(d, capi.ModesDesc)
    assert (d.r_min, d.r_max, d.n_r, d.m_max, d.n_p, d.sink, d.flags) == (10.0, 200.0, 40, 8, 0, 0, capi.MODES_LOG)
    assert (d.weight, d.n_q, d.n_rows, d.z_max) == (capi.MODES_W_MASS, 0, 0, np.inf) and tuple(d.normal) == (0.0, 0.0, 1.0)
    assert tuple(d.reserved) == (0, 0, 0)
    assert spiral is None and ring.shape == (40, 9, 2) and ring.dtype == np.float64 and addr(a[3]) == base_of(ring).ctypes.data
    assert base_of(ring).shape == (720,)
    assert rc.dtype == np.int64 and rc.tolist() == list(range(40)) and addr(a[7]) == rc.ctypes.data
    assert counts == tuple(COUNTS) and exp == -17 and isinstance(exp, int)


def test_spiral_quantity_and_raw(ctx):
    vals = np.arange(2.0 * N).reshape(2, N)
    res = ctx.modes((0.0, 5.0), 3, 2, z_max=1.5, centre=(1, 2, 3), centre_v=(4, 5, 6), normal=(0, 1, 1), weight="one",
                    q=capi.modes_row(1), values=vals, spiral=(-4.0, 4.0, 5), r_ref=2.5, raw=True)
    ring, spiral, rc, counts, exp, raw = res
    a = ctx.lib.one()
    d = ctx.modes_desc
    assert (d.n_r, d.m_max, d.n_p, d.sink, d.flags, d.weight, d.n_q, d.q, d.n_rows) == (3, 2, 5, -1, 0, capi.MODES_W_ONE, 1, -2, 2)
    assert (d.p_min, d.p_max, d.r_ref, d.z_max) == (-4.0, 4.0, 2.5, 1.5)
    assert tuple(d.centre) == (1.0, 2.0, 3.0) and tuple(d.centre_v) == (4.0, 5.0, 6.0) and tuple(d.normal) == (0.0, 1.0, 1.0)
    assert addr(a[2]) == vals.ctypes.data and a[4] == 2 * 3 * (3 + 5) == 48
    flat = base_of(ring)
    assert flat.shape == (48,) and base_of(spiral) is flat and addr(a[3]) == flat.ctypes.data
    assert ring.shape == (3, 3, 2) and spiral.shape == (3, 5, 2)
    assert spiral.ctypes.data == flat.ctypes.data + 18 * 8         # the spiral block follows the ring block
    rring, rspiral = raw
    rflat = base_of(rring)
    assert rflat.dtype == np.uint64 and rflat.shape == (48, 2) and addr(a[5]) == rflat.ctypes.data
    assert rring.shape == (3, 3, 2, 2) and rspiral.shape == (3, 5, 2, 2) and base_of(rspiral) is rflat
    assert rc.shape == (3,) and counts == tuple(COUNTS)
    # a field name as the quantity, one row given as 1-D
    ctx.lib.calls.clear()
    ctx.modes((0.0, 5.0), 1, 0, q="vx", spiral=(0.0, 0.0, 1))
    assert (ctx.modes_desc.n_q, ctx.modes_desc.q, ctx.modes_desc.n_rows) == (1, capi.FIELDS.index("vx"), 0)
    ctx.lib.calls.clear()
    one = np.arange(float(N))
    ctx.modes((0.0, 5.0), 1, 0, q=capi.modes_row(0), values=one)
    assert ctx.modes_desc.n_rows == 1 and addr(ctx.lib.one()[2]) == one.ctypes.data
    # rows as plain lists: converted, not refused
    ctx.lib.calls.clear()
    ctx.modes((0.0, 5.0), 1, 0, q=capi.modes_row(1), values=[[0.0] * N, list(range(N))])
    assert ctx.modes_desc.n_rows == 2 and addr(ctx.lib.one()[2])


def test_error_texts(ctx):
    with pytest.raises(ValueError, match="modes: give centre / centre_v or sink, not both"):
        ctx.modes((0.0, 5.0), 3, 2, sink=0, centre=(0, 0, 0))
    with pytest.raises(ValueError, match="modes: give centre / centre_v or sink, not both"):
        ctx.modes((0.0, 5.0), 3, 2, sink=1, centre_v=(0, 0, 0))
    with pytest.raises(ValueError, match="modes: values rows of 6 for 7 particles"):
        ctx.modes((0.0, 5.0), 3, 2, q=capi.modes_row(0), values=np.zeros((1, N - 1)))
    with pytest.raises(KeyError):
        ctx.modes((0.0, 5.0), 3, 2, weight="volume")
    with pytest.raises(ValueError, match="is not in list"):
        ctx.modes((0.0, 5.0), 3, 2, q="nothing")
    assert not [c for c in ctx.lib.calls if c[0] == "sph_modes"]     # nothing reached the library


def test_device_form_refuses_host_values(ctx):
    import torch  # noqa: F401  (the device form needs it; a missing torch is an error, not a skip)
    with pytest.raises(ValueError, match="modes: device values must be a contiguous float64 tensor on the context's GPU"):
        ctx.modes((0.0, 5.0), 3, 2, q=capi.modes_row(0), values=np.zeros((1, N)), device=True)
    with pytest.raises(ValueError, match="modes: device values must be a contiguous float64 tensor on the context's GPU"):
        ctx.modes((0.0, 5.0), 3, 2, q=capi.modes_row(0), values=[[0.0] * N], device=True)
    assert not [c for c in ctx.lib.calls if c[0].startswith("sph_modes")]
