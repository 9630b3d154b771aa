"""CPU tests of tests/image_sets.py: every case takes, by the restatement of the host sizing (image_sets.render_sizing /
cube_sizing, which follow summersph_amd/csrc/render.hip and cube.hip), the path it is named for, so that
tests/test_render_binning_gpu.py and tests/test_cube_binning_gpu.py cannot silently cease to cover these paths; the
reference-compared cases of tests/test_render_gpu.py never run a second interval batch (the gap these cases close); and the
float64 brute force agrees with the extended-precision reference within a tenth of the GPU tests' tolerance, so that the
tolerance is not tight for the reference alone."""
import numpy as np
import pytest

import cube_ref
import image_ref
import image_sets as S
import render_field_ref
import render_ref
import test_render_gpu as existing
from summersph_amd import ic

TOL = 1e-12
MAX_PARTICLES, MAX_TERMS = 4000, 2000


def _sizing(name, axis=None, bricks=True):
    c = S.render_case(name)
    return c, S.render_sizing(S.case_pos(c), S.case_h(c), c["lo"], c["hi"], c["n"], axis, c["clip"], bricks=bricks)


def _frame(c):
    g = c["gas"]
    pos = np.stack([g["x"], g["y"], g["z"]], axis=1)
    vel = np.stack([g["vx"], g["vy"], g["vz"]], axis=1)
    P, V = cube_ref.project(c["rot"], pos, vel, c["centre"], c["v_ref"])
    return pos, vel, P, V


def _cube_sizing(name):
    c = S.cube_case(name)
    _, _, P, _ = _frame(c)
    return c, S.cube_sizing(P[:, :2], c["h"], c["lo"], c["hi"], c["n"])


# ---- the paths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coarse", "offset"])
def test_coarse_runs_many_batches_with_records_where_the_loop_can_lose_them(name):
    c, z = _sizing(name)
    assert z["enlargements"] == 0 and z["edge"] == 2.0 * c["h"]
    b = z["bricks"][0]                                           # tile (0, 0), segment 0
    L, B = b["lens"], b["batch_records"]
    assert b["n_int"] == 4221 and B.size == 66 and b["n_int"] % S.GT == 61
    nz = np.flatnonzero(B > 0)
    assert nz.size >= 20
    inner_empty = [i for i in range(nz[0], nz[-1]) if B[i] == 0]
    assert inner_empty, "no batch without records between two with records"
    if name == "offset":
        return
    # the planted records: intervals 0, 63, 64 and the ragged last batch hold records that contribute to a node
    assert L[0] >= 1 and L[63] >= 1 and L[64] >= 2 and B[-1] >= 1
    planted = S._coarse_planted(S.COARSE["lo"], S.COARSE["hi"], S.COARSE["n"], S.COARSE["h"])
    assert np.array_equal(S.case_pos(c)[:planted.shape[0]], planted)
    _, _, g = S.render_nodes(c)
    cnt = image_ref.render_terms(planted, c["h"], g)
    org, inv = z["lo"] - z["reach"], 1.0 / z["edge"]
    cells = np.stack([S.cell_1d(org[a], inv, z["dim"][a], planted[:, a]) for a in range(3)], axis=1)
    n1c = b["cells"][1][1] - b["cells"][0][1] + 1
    r = (cells[:, 0] - b["cells"][0][0]) * n1c + (cells[:, 1] - b["cells"][0][1])
    reaches = np.array([image_ref.render_terms(planted[k:k + 1], c["h"], g)[:8, :8, :8].sum() > 0 for k in range(planted.shape[0])])
    assert cnt.sum() >= planted.shape[0] and reaches.all()      # each planted particle is within 2h of a node of the brick
    for want in (0, 63, 64):
        assert want in r[reaches], want
    assert (r[reaches] >= (B.size - 1) * S.GT).any()             # one in the last batch
    assert len(set(r[reaches] // S.GT)) >= 8                     # and in many batches between


def test_cells_clamped_enlarges_the_edge():
    c, z = _sizing("cells_clamped")
    assert z["enlargements"] == 3 and z["edge"] > 2.0 * c["h"] * 1.99 and z["dim"] == (352, 352, 352)
    assert z["ncells"] <= S.RENDER_MAX_CELLS < 2 * z["ncells"]
    assert max(b["n_int"] for b in z["bricks"]) > 20000
    pos, lo, hi = S.case_pos(c), c["lo"], c["hi"]
    for a in range(3):                                           # within reach outside all six faces
        assert (pos[:, a] < lo[a]).any() and (pos[:, a] > hi[a]).any()
    out = np.where(pos < lo, -1, np.where(pos > hi, 1, 0))
    corners = {tuple(v) for v in out if np.all(v != 0)}
    assert len(corners) == 8                                     # and the eight corners
    assert z["nsel"] == pos.shape[0]


@pytest.mark.parametrize("k", S.CHUNK_COUNTS)
def test_chunk_counts_are_exact(k):
    c, z = _sizing(f"chunk_counts_{k}")
    assert len(z["bricks"]) == 1 and z["nsel"] == k
    b = z["bricks"][0]
    assert int(b["batch_records"].sum()) == k and b["n_int"] <= S.GT
    chunks = -(-k // S.RENDER_CH)
    assert chunks == {255: 1, 256: 1, 257: 2, 513: 3}[k]
    if k == 513:                                                 # one interval alone spans three chunks; r = 0 at a node
        assert b["lens"].max() == 513
        _, _, g = S.render_nodes(c)
        assert all((g[a] == 0.0).any() for a in range(3)) and np.all(S.case_pos(c)[:513] == 0.0)


def test_h_decades_spans_the_decades_and_its_special_particles():
    c, z = _sizing("h_decades")
    h, pos = c["gas"]["h"], S.case_pos(c)
    assert h.min() < 2e-3 and h.max() == 8.0 and z["h_max"] == 8.0
    _, _, g = S.render_nodes(c)
    kinds = np.array(c["kinds"])
    for k, kind in enumerate(kinds):
        cnt = image_ref.render_terms(pos[k:k + 1], h[k:k + 1], g)
        assert cnt.sum() == (0 if kind == "mid" else 1), (k, kind)
        if kind == "on":
            assert all((g[a] == pos[k, a]).any() for a in range(3))
        if kind == "ulp":
            assert np.any([not (g[a] == pos[k, a]).any() for a in range(3)])
    big = np.flatnonzero((h == 8.0) & np.any((pos < c["lo"]) | (pos > c["hi"]), axis=1))
    reach = [image_ref.render_terms(pos[k:k + 1], h[k:k + 1], g).sum() for k in big]
    assert sum(r > 0 for r in reach) >= 5 and min(reach) == 0     # they reach into the box; one does not


def test_flat_axes_are_flat():
    c, z = _sizing("flat_z")
    lo, hi, g = S.render_nodes(c)
    assert c["lo"] is None and lo[2] == hi[2] and g[2].size == 5 and np.all(g[2] == lo[2])
    c, z = _sizing("flat_x")
    assert c["lo"][0] == c["hi"][0] and c["n"][0] == 9 and z["nsel"] > 0


def test_long_axis_exceeds_the_grid_cap():
    c, z = _sizing("long_axis", bricks=False)
    assert z["nseg"] == 65537 > S.YSEGS_MAX == z["ysegs"]
    _, _, g = S.render_nodes(c)
    cnt = image_ref.render_terms(S.case_pos(c), c["h"], g)[:, 0, 0]
    seg = np.flatnonzero(cnt) // S.KW
    assert (seg >= S.YSEGS_MAX).any() and (seg < 2).any()        # the second trips of blocks 0 and 1, and their first
    assert (cnt == 0).sum() > cnt.size // 2


def test_nothing_reaches():
    c, z = _sizing("nothing_far")
    assert S.select(S.case_pos(c), c["clip"]).sum() == 500 and z["nsel"] == 0
    c, z = _sizing("nothing_clipped")
    assert S.select(S.case_pos(c), c["clip"]).sum() == 0 and c["lo"] is not None


def test_cube_paths():
    c, z = _cube_sizing("cube_coarse")
    assert z["enlargements"] == 0 and z["halvings"] == 0 and z["edge"] == 2 * c["h"]
    t = z["tiles"][0]
    assert t["n_int"] == 586 and t["batch_records"].size == 10 and (t["batch_records"] > 0).sum() >= 8
    c, z = _cube_sizing("cube_clamped")
    assert z["enlargements"] == 1 and z["halvings"] == 0 and z["edge"] > 2 * c["h"] * 1.4
    assert z["ncells"] <= S.CUBE_MAX_CELLS < 2 * z["ncells"]
    assert all(t["n_int"] == 806 and t["batch_records"].size == 13 for t in z["tiles"][:1])
    c, z = _cube_sizing("cube_halved")
    assert z["enlargements"] == 0 and z["halvings"] == 2 and z["edge"] == 0.5 * c["h"]
    for k in S.CUBE_CHUNKS:
        c, z = _cube_sizing(f"cube_chunks_{k}")
        assert len(z["tiles"]) == 1 and int(z["tiles"][0]["batch_records"].sum()) == k == z["nsel"]
        assert -(-k // S.CUBE_CH) == {127: 1, 128: 1, 129: 2, 257: 3}[k]
    c, z = _cube_sizing("cube_flat")
    assert c["lo"][0] == c["hi"][0] and c["n"][0] == 5 and z["nsel"] > 0
    # a second channel chunk of one channel, and records that straddle the boundary
    assert c["n_chan"] == 33 and c["sigma_floor"] > 0
    _, _, _, V = _frame(c)
    k = (V - c["v0"]) / c["dv"]
    reach = cube_ref.XCUT * c["sigma_floor"] / c["dv"]
    assert np.mean((k - reach < 31) & (k + reach > 32.5)) > 0.5
    r = c["rot"]
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(r) - 1) < 1e-15 and np.all(np.abs(r) > 0.05)


# ---- the gap: the reference-compared cases of test_render_gpu.py stay within one batch ---------------------------------
def _max_n_int(pos, h, lo, hi, n):
    return max(b["n_int"] for b in S.render_sizing(pos, h, lo, hi, n)["bricks"])


def test_existing_brute_force_cases_never_run_a_second_batch():
    h = 1.25
    sets = {"sod": (ic.sod_column(), np.array([-20.0, -2.0, -2.0]), np.array([30.0, 2.5, 2.0]), (41, 9, 7), 24),
            "disc3000": (ic.keplerian_disc(3000, seed=41), np.array([-20.0, -15.0, -3.0]), np.array([25.0, 20.0, 3.5]), (29, 23, 11), 49),
            "clustered": (existing._clustered(), np.array([-18.0, -16.0, -14.0]), np.array([17.0, 15.0, 16.0]), (21, 19, 17), 64)}
    for name, (rows, lo, hi, n, want) in sets.items():
        gas, _ = ic.split_rows(existing._edge_set(rows, h, lo, hi))
        got = _max_n_int(existing.positions(gas), h, lo, hi, n)
        assert got == want <= S.GT, (name, got)
    # per-particle h (test_per_particle_h_variable_context): n_int depends on the largest h alone; the disc's h is at least
    # its midplane value and at most h_max_length = 10
    lo, hi, n = np.array([-30.0, -25.0, -6.0]), np.array([28.0, 30.0, 5.0]), (25, 27, 9)
    worst = max(_max_n_int(np.zeros((1, 3)), hm, lo, hi, n) for hm in np.linspace(ic.H_REF, 10.0, 200))
    assert worst <= 42 <= S.GT, worst


# ---- sizes, and the reference against itself ----------------------------------------------------------------------------
def _within(f64, ext, s, what):
    err = np.abs(f64.astype(image_ref.LD) - ext)
    bad = err > 0.1 * TOL * s
    worst = float(np.max(np.where(s > 0, err / np.where(s > 0, s, 1), 0)))
    print(f"    {what}: float64 against extended precision, worst |diff| / S = {worst:.2e}")
    assert not bad.any(), (what, worst)
    assert np.all(f64[np.asarray(s == 0)] == 0.0)


@pytest.mark.parametrize("name", S.RENDER_CASES)
def test_render_reference_agrees_with_extended_precision(name):
    c = S.render_case(name)
    pos, m, h = S.case_pos(c), c["gas"]["m"], S.case_h(c)
    assert pos.shape[0] <= MAX_PARTICLES
    sel = S.select(pos, c["clip"])
    lo, hi, g = S.render_nodes(c) if sel.any() else (c["lo"], c["hi"], [S.node_coords(c["lo"][a], c["hi"][a], c["n"][a]) for a in range(3)])
    assert image_ref.render_terms(pos, h, g, sel).max() <= MAX_TERMS
    a = S.field_values(pos.shape[0])
    num, den, s_num, s_den, near = image_ref.render(pos, m, a, h, g, sel)
    X, Y, Z = np.meshgrid(*g, indexing="ij")
    nodes = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    hs = np.broadcast_to(np.asarray(h, dtype=np.float64), m.shape)[sel]
    if sel.any():
        fnum, fden = render_field_ref.brute(nodes, pos[sel], m[sel], a[sel], hs, chunk=256)
        dens = render_ref.brute(nodes, pos[sel], m[sel], hs, chunk=256)
    else:
        fnum = fden = dens = np.zeros(nodes.shape[0])
    _within(fnum.reshape(c["n"]), num, s_num, name + " num")
    _within(fden.reshape(c["n"]), den, s_den, name + " den")
    _within(dens.reshape(c["n"]), den, s_den, name + " density")
    assert np.all(np.asarray(s_den)[~near] == 0)
    if name.startswith("nothing"):
        assert not near.any() and np.all(num == 0)
    else:
        assert near.any()


@pytest.mark.parametrize("name", S.CUBE_CASES)
def test_cube_reference_agrees_with_extended_precision(name):
    c = S.cube_case(name)
    pos, vel, P, V = _frame(c)
    assert pos.shape[0] <= MAX_PARTICLES
    gu, gv = S.node_coords(c["lo"][0], c["hi"][0], c["n"][0]), S.node_coords(c["lo"][1], c["hi"][1], c["n"][1])
    terms = [(np.hypot(u - P[:, 0], gv[:, None] - P[None, :, 1]) <= 2 * c["h"]).sum(axis=1).max() for u in gu]
    assert max(terms) <= MAX_TERMS
    a = S.field_values(pos.shape[0])
    m = c["gas"]["m"]
    vox, s, near = image_ref.cube(pos, vel, m, c["h"], a, gu, gv, c["v0"], c["dv"], c["n_chan"], c["rot"], c["centre"], c["v_ref"],
                                  c["sigma_floor"])
    f64 = cube_ref.cube(pos, vel, m, c["h"], c["n"], (c["lo"], c["hi"]), c["v0"], c["dv"], c["n_chan"], rot=c["rot"], centre=c["centre"],
                        v_ref=c["v_ref"], sigma_floor=c["sigma_floor"], values=a)
    _within(f64, vox, np.broadcast_to(s, vox.shape), name)
    assert near.any() and np.abs(vox).max() > 0
    assert np.abs(vox[32]).max() > 0 and np.abs(vox[31]).max() > 0          # both channel chunks hold signal
