"""The device forms of the fourteen analysis calls on a caller's stream: the context runs on a torch side stream
(sph_set_stream), so Context's ordering takes the arm in which torch's current stream waits for the context's stream
instead of synchronising the device.  Every case calls the device form, consumes the outputs at once on torch's current
stream (clone, then the copy to the host) and compares with the host form of the same call.

The comparison is the one each call's own GPU test makes between its two forms, and every one of them is exact
(np.array_equal, equal_nan where non-targets are NaN): test_render_gpu, test_render_field_gpu, test_profile_gpu,
test_energy_gpu, test_groups_gpu, test_peaks_gpu, test_gradients_gpu, test_sample_gpu, test_trace_gpu, test_cube_gpu,
test_force_terms_gpu, test_binned_gpu, test_gravity_at_gpu and test_bound_gpu.  The arguments are the smallest
meaningful ones: 64 points, an 8 x 8 image, 4 channels, 8 bins, 4 steps, on a fixed-h disc of 2000 particles.
"""
import numpy as np
import pytest

from summersph_amd import ic

pytestmark = pytest.mark.gpu
M = 64


@pytest.fixture(scope="module")
def world():
    import torch
    from summersph_amd import capi
    capi.load()
    gas, sinks = ic.split_rows(ic.keplerian_disc(2000, seed=9))
    ctx = capi.Context(device=0)
    ctx.upload(gas)
    ctx.set_sinks(sinks)
    ctx.density()
    ctx.forces()
    ctx.synchronize()
    stream = torch.cuda.Stream(device=0)                # kept alive by the fixture
    ctx.set_stream(stream.cuda_stream)
    assert ctx.stream() == stream.cuda_stream != 0
    pts = np.ascontiguousarray(np.stack([gas["x"], gas["y"], gas["z"]], axis=1)[:M])      # inside the gas
    R = np.hypot(gas["x"], gas["y"])
    w = {"ctx": ctx, "capi": capi, "torch": torch, "gas": gas, "pts": pts, "r_max": float(R.max()),
         "values": np.ascontiguousarray(np.stack([gas["vx"] * 2.0, R]))}
    yield w
    ctx.close()


def _dev(w, a):
    return w["torch"].from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rows(w, tab, n, device):
    """the first min(n, 50) rows of a groups or peaks table as plain float64: the rows the device form wrote"""
    if device:
        return tab[:min(n, 50)]
    return np.ascontiguousarray(tab).view(np.float64).reshape(-1, tab.itemsize // 8)


def _tuple(w, cnt):
    """peaks and binned leave their counts on the device"""
    return tuple(int(v) for v in (cnt.clone().cpu().tolist() if isinstance(cnt, w["torch"].Tensor) else cnt))


def _render_density(w, device):
    return [w["ctx"].render_density(8, axis="z", device=device)]


def _render_field(w, device):
    v = w["values"][0].copy()
    return list(w["ctx"].render_field(_dev(w, v) if device else v, 8, axis="z", normalise=True, weight_out=True, device=device))


def _profile(w, device):
    res = w["ctx"].profile(10.0, w["r_max"], 8, sink=0, device=device)
    return [res if device else res[1]]


def _energy(w, device):
    e = w["ctx"].energy(phi=True, device=device)
    return [e["sums"], e["phi"]]


def _groups(w, device):
    lab, tab, ng = w["ctx"].groups(1.0, link_h=True, max_groups=50, device=device)
    return [lab, _rows(w, tab, ng, device), ng]


def _peaks(w, device):
    lab, tab, ng, cnt = w["ctx"].peaks(1.0, link_h=True, max_groups=50, device=device)
    return [lab, _rows(w, tab, ng, device), ng, _tuple(w, cnt)]


def _gradients(w, device):
    v = w["values"]
    g, rho, cnt = w["ctx"].gradients(fields=("vx", w["capi"].GRAD_VALUES), values=_dev(w, v) if device else v, rho=True,
                                     device=device)
    return [g, rho, cnt]


def _sample(w, device):
    p, v = w["pts"], w["values"]
    out, den, cnt = w["ctx"].sample(_dev(w, p) if device else p, fields=(w["capi"].SAMPLE_VALUES, "rho"),
                                    values=_dev(w, v) if device else v, weight_out=True, counts=True, device=device)
    return [out, den, cnt]


def _trace(w, device):
    p = w["pts"]
    return list(w["ctx"].trace(_dev(w, p) if device else p, 4, 0.5, carry="u", stride=2, counts=True, device=device))


def _cube(w, device):
    r = w["r_max"]
    return [w["ctx"].cube(8, ((-r, -r), (r, r)), -0.3, 0.2, 4, rot=None, sigma_floor=0.1, device=device)]


def _force_terms(w, device):
    return [w["ctx"].force_terms(device=device)]


def _binned(w, device):
    v, r = w["values"], w["r_max"]
    sums, cnt = w["ctx"].binned(w["capi"].binned_row(1), 8, ranges=(10.0, r), q=("vy", w["capi"].binned_row(0)),
                                values=_dev(w, v) if device else v, squares=True, device=device)
    return [sums, _tuple(w, cnt)]


def _gravity_at(w, device):
    p = [np.ascontiguousarray(w["pts"][:, k]) for k in range(3)]
    ph = np.full(M, 1.5)
    phi, acc, cnt = w["ctx"].gravity_at([_dev(w, t) for t in p] if device else p, ph=_dev(w, ph) if device else ph, split=True,
                                        counts=True, device=device)
    return [phi, acc, cnt]


def _bound(w, device):
    lab, _, ng = w["ctx"].groups(1.0, link_h=True)
    res = w["ctx"].bound(_dev(w, lab) if device else lab, ng, max_rounds=2, device=device)
    tab = res[3] if device else np.ascontiguousarray(res[3]).view(np.float64).reshape(-1, w["capi"].BOUND_NCOL)
    return [res[0], res[1], res[2], tab, res[4]]


CASES = {"render_density": _render_density, "render_field": _render_field, "profile": _profile, "energy": _energy,
         "groups": _groups, "peaks": _peaks, "gradients": _gradients, "sample": _sample, "trace": _trace, "cube": _cube,
         "force_terms": _force_terms, "binned": _binned, "gravity_at": _gravity_at, "bound": _bound}


def _consume(w, x):
    """a device output, used at once on torch's current stream: clone it, then copy the clone to the host"""
    return x.clone().cpu().numpy() if isinstance(x, w["torch"].Tensor) else x


@pytest.mark.parametrize("name", list(CASES))
def test_device_form_on_a_callers_stream(world, name):
    w = world
    assert w["ctx"].stream() != 0
    dev = [_consume(w, x) for x in CASES[name](w, True)]            # consumed before anything else waits for the GPU
    host = [_consume(w, x) for x in CASES[name](w, False)]
    assert len(dev) == len(host)
    seen = False
    for k, (d, h) in enumerate(zip(dev, host)):
        if isinstance(h, np.ndarray):
            assert isinstance(d, np.ndarray) and d.dtype == h.dtype and d.shape == h.shape, (name, k)
            assert np.array_equal(d, h, equal_nan=True), (name, k)
            if h.dtype.kind == "f" and np.any(np.isfinite(h) & (h != 0)):
                seen = True
        else:
            assert d == h, (name, k, d, h)
    assert seen, f"{name}: no finite non-zero value was compared"
