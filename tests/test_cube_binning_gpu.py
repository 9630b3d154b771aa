"""GPU tests of sph_cube (include/summersph.h, "spectral cubes") on image grids that stress its binning
(tests/image_sets.py; tests/test_image_sets_cpu.py asserts the path every case takes): ten and thirteen interval batches
per tile, the MAX_CELLS clamp, the cell-halving loop, exact chunk counts of the LDS staging and a flat image axis, with a
rotated frame, signed values, sigma_floor > 0 and 33 channels (a second channel chunk of one channel).

EVERY voxel is compared with the extended-precision reference (tests/image_ref.py) against its node's term scale:
    |got - ref| <= TOL S_g,   S_g = sum |y0_j| F(0) over the footprints covering the node,   TOL = 1e-12
(a term y0_j F(p) w_k has F <= F(0) and a channel weight w_k <= 1 whose absolute error is about an ulp of 1; at most 2000
terms are added in sequence).  Nodes with no particle within 2 h (1 + 1e-12) must be exactly 0.0 in every channel."""
import numpy as np
import pytest

from gpu_support import capi
import image_ref
import image_sets as S

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _run(ctx, c, a):
    return ctx.cube(c["n"], (c["lo"], c["hi"]), c["v0"], c["dv"], c["n_chan"], rot=c["rot"], centre=c["centre"], v_ref=c["v_ref"],
                    sigma_floor=c["sigma_floor"], values=a, h=c["h"])


@pytest.mark.parametrize("name", S.CUBE_CASES)
def test_cube_every_voxel(capi, name):
    c = S.cube_case(name)
    g = c["gas"]
    pos = np.stack([g["x"], g["y"], g["z"]], axis=1)
    vel = np.stack([g["vx"], g["vy"], g["vz"]], axis=1)
    a = S.field_values(pos.shape[0])
    gu, gv = S.node_coords(c["lo"][0], c["hi"][0], c["n"][0]), S.node_coords(c["lo"][1], c["hi"][1], c["n"][1])
    ref, s, near = image_ref.cube(pos, vel, g["m"], c["h"], a, gu, gv, c["v0"], c["dv"], c["n_chan"], c["rot"], c["centre"], c["v_ref"],
                                  c["sigma_floor"])
    ctx = capi.Context(device=0)
    ctx.upload(g)
    got = _run(ctx, c, a)
    assert got.shape == ref.shape == (c["n_chan"],) + c["n"]
    err = np.abs(got.astype(image_ref.LD) - ref)
    sb = np.broadcast_to(s, ref.shape)
    reached = np.asarray(sb > 0)
    ratio = float(np.max(err[reached] / sb[reached]))
    print(f"    cube: {name}: worst |got - ref| / S = {ratio:.2e} over {int(reached.sum())} of {got.size} voxels")
    assert np.all(err <= TOL * sb), (name, ratio)
    assert np.all(got[:, ~near] == 0.0)
    assert (got < 0).any() and (got > 0).any() and np.abs(got[32]).max() > 0
    assert np.array_equal(got, _run(ctx, c, a))                                # two calls are bitwise equal
    flat = c.get("flat")
    if flat is not None:                                                       # the nodes of the flat axis coincide
        for k in range(c["n"][flat]):
            assert np.array_equal(np.take(got, k, axis=1 + flat), np.take(got, 0, axis=1 + flat))
    ctx.close()
