"""GPU tests of sph_profile on the sets of tests/profile_sets.py (validated on the CPU by tests/test_profile_sets_cpu.py):
particles exactly on ring, sector, z-cut and shell edges and on their representable neighbours, a million rings, bins whose
populations straddle the piece (1024) and wavefront (64) sizes of the sorted reduction up to the second round of
profile_final (more than 64 pieces), ghosts, the centre itself, and both branches of the frame rule.  The exact sets are
compared with np.array_equal: membership through the bitmask sum m alpha, and all 20 sums against the restatement reduced
in the library's own shape (profile_ref.piece_sum).  The last tests hold the header's "a numpy restatement reproduces it"
to the bit on generic discs."""
import numpy as np
import pytest

from gpu_support import capi, make_context
import profile_ref
import profile_sets as S
import test_profile_gpu as existing

pytestmark = pytest.mark.gpu
SPH_ERR_STATE = 5


def _context(capi, gas, sinks=None, **kw):
    return make_context(capi, gas, sinks, **S.PARAMS, **kw)


def _table_cols(capi, t):
    return np.stack([t[c] for c in capi.PROFILE_COLUMNS], axis=1)


def _finish(ctx, kw, sums, normal=(0, 0, 1)):
    p = ctx.params
    return profile_ref.finish(sums, kw["r_min"], kw["r_max"], kw["n_r"], kw.get("n_phi", 1), kw.get("log", False), normal,
                              p.gamma, p.gamma_m1, p.G)


def _same_bits(got, want):
    """all 20 sums, naming the first column and bin that differ"""
    if not np.array_equal(got, want):
        b, s = np.argwhere(got != want)[0]
        raise AssertionError(f"sum {s} of bin {b}: {got[b, s]!r} != {want[b, s]!r}; columns that differ: "
                             f"{sorted(set(np.argwhere(got != want)[:, 1].tolist()))}")


# ---- (a) ring edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(S.RING_CASES))
def test_ring_edges(capi, case):
    for gas, _, kw, note in S.ring_edge_sets(case):
        ctx = _context(capi, gas)
        t, s = ctx.profile(**kw)
        # the library's table is the restatement's, to the bit (both are the host's arithmetic and pow)
        e = note["edges"]
        assert np.array_equal(t["R_lo"], e[:-1]) and np.array_equal(t["R_hi"], e[1:])
        want, b = S.reference(gas, kw)
        assert np.array_equal(s[:, 0], want[:, 0])                        # counts
        assert np.array_equal(s[:, 12], want[:, 12])                      # members: sum m alpha is their bitmask
        _same_bits(s, want)
        ctx.close()


# ---- (b) a million rings ----------------------------------------------------------------------------------------------
def test_million_rings(capi):
    gas, _, kw, note = S.million_rings()
    ctx = _context(capi, gas)
    t, s = ctx.profile(**kw)
    assert t is None and s.shape == (S.MILLION, capi.PROFILE_NSUM)
    want, b = S.reference(gas, {k: v for k, v in kw.items() if k != "sums_only"}, only_bins=note["occupied"])
    occ = note["occupied"]
    assert np.array_equal(s[occ, 0], want[occ, 0]) and np.array_equal(s[occ, 12], want[occ, 12])
    empty = np.ones(S.MILLION, bool); empty[occ] = False
    assert not s[empty].any()                                             # every other bin exactly zero
    _same_bits(s, want)
    ctx.close()


# ---- (c) sectors, the axes and the centre -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_phi", S.SECTOR_NPHI)
def test_sectors_axes_and_centre(capi, n_phi):
    for cm in (0.0, 4.0):
        gas, _, kw, note = S.sectors(n_phi, cm)
        ctx = _context(capi, gas)
        t, s = ctx.profile(**kw)
        want, b = S.reference(gas, kw)
        if note["expected"] is not None:
            assert list(b) == note["expected"]
        mask = np.zeros(n_phi)
        for i, bi in enumerate(b):
            mask[bi] += 2.0 ** i
        assert np.array_equal(s[:, 0], want[:, 0])
        assert np.array_equal(s[:, 12], mask), (s[:, 12], mask)           # who sits in which sector
        assert np.all(np.isfinite(s))
        _same_bits(s, want)
        ctx.close()
    # the centre particle alone: selected (r_min == 0), finite, no radial or azimuthal velocity, no eccentricity
    one = {k: v[5:] for k, v in gas.items()}
    ctx = _context(capi, one)
    _, s = ctx.profile(**dict(kw, n_phi=1))
    assert s[0, 0] == 1 and np.all(np.isfinite(s)) and not s[0, [2, 5, 6, 8, 9, 14, 15, 16, 17, 18, 19]].any()
    assert s[0, 7] == one["vz"][0] and s[0, 10] == one["vz"][0] ** 2
    ctx.close()


# ---- (d) the z cut ----------------------------------------------------------------------------------------------------
def test_z_cut(capi):
    ctx = _context(capi, S.z_cut(S.Z_CUT)[0])
    cols = {c: i for i, c in enumerate(capi.PROFILE_COLUMNS)}
    for z_max in S.Z_CALLS:
        gas, _, kw, note = S.z_cut(z_max)
        t, s = ctx.profile(**kw)
        want, b = S.reference(gas, kw)
        assert s[0, 0] == len(note["members"]) and s[0, 12] == sum(2.0 ** i for i in note["members"])
        _same_bits(s, want)
        if z_max <= 0:                                                    # nothing selected
            assert not s.any()
            tt = _table_cols(capi, t)
            with np.errstate(all="ignore"):
                assert np.array_equal(np.isnan(tt), np.isnan(_finish(ctx, kw, want)))
            assert t["N"][0] == 0 and t["M"][0] == 0 and t["Sigma"][0] == 0
            assert tt[0, cols["R_lo"]] == 0.0 and tt[0, cols["R_hi"]] == 10.0
            for c in ("R_mean", "z_mean", "H", "vphi_mean", "u_mean", "Omega", "kappa", "Q", "j", "tilt", "ecc", "peri"):
                assert np.isnan(t[c][0]), c
        if z_max == np.inf:
            assert s[0, 4] == np.inf and not np.isnan(s).any()           # m z' z' of z' = 1e300
    ctx.close()


# ---- (e) the piece shapes ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def piece_refs():
    """the exact sums of the flat set and the layered set's in the library's shape, once"""
    out = {}
    for layered in (False, True):
        for n_phi in (1, 4):
            gas, _, kw, note = S.piece_shapes(n_phi, layered)
            out[layered, n_phi] = S.reference(gas, kw, shape="pieces", n_owned=note["n_owned"])[0]
            if layered:
                k0 = dict(kw, centre=(kw["centre"][0], kw["centre"][1], 0.0))
                out[layered, n_phi, "no_mass"] = S.reference(gas, k0, shape="sequential", n_owned=note["n_owned"])[0]
    return out


def _cmp_piece_table(capi, ctx, kw, t, sums):
    """the finished table at test_profile_gpu.TOL with the restatement's NaN pattern: empty rings, and kappa NaN for their neighbours"""
    with np.errstate(all="ignore"):
        ref = _finish(ctx, kw, sums)
    existing._cmp_table(capi, t, ref)
    empty = sums[:, 0] == 0
    assert np.array_equal(np.isnan(t["R_mean"]), empty) and np.array_equal(t["N"] == 0, empty)
    assert np.array_equal(t["M"] == 0, empty) and np.array_equal(t["Sigma"] == 0, empty)
    pops = np.array(S.POPULATIONS)
    beside = pops == 0                                                    # an empty ring, or one whose kappa needs it
    beside[1:-1] |= (pops[:-2] == 0) | (pops[2:] == 0)
    beside[0] |= pops[1] == 0; beside[-1] |= pops[-2] == 0
    assert beside.sum() == 12 and np.all(np.isnan(t["kappa"][np.repeat(beside, kw["n_phi"])]))


@pytest.mark.parametrize("n_phi", [1, 4])
def test_piece_shapes_exact(capi, piece_refs, n_phi):
    """the set with z = 0: every sum exact in any order, so np.array_equal whatever the shape -- host and device form"""
    gas, _, kw, note = S.piece_shapes(n_phi)
    want = piece_refs[False, n_phi]
    assert tuple(want.reshape(20, n_phi, -1)[:, :, 0].sum(axis=1)) == S.POPULATIONS
    ctx = _context(capi, gas, n_owned=note["n_owned"])
    t, s = ctx.profile(**kw)
    assert s[:, 0].sum() == note["n_owned"]                               # no ghost counted
    _same_bits(s, want)
    _cmp_piece_table(capi, ctx, kw, t, want)
    d = ctx.profile(**kw, device=True)
    _same_bits(d.cpu().numpy(), want)
    ctx.close()


@pytest.mark.parametrize("n_phi", [1, 4])
def test_piece_shapes_in_every_slot_order(capi, piece_refs, n_phi):
    """the same particles with a z that a density pass can take (profile_sets.piece_shapes): upload order, cell-sorted slots of
    the dense and of the hashed grid.  Central mass 0: exact in any order.  Central mass 4: the e sums are no dyadic rationals
    any more; all 20 equal the restatement reduced in the library's shape, in every slot order."""
    gas, _, kw, note = S.piece_shapes(n_phi, layered=True)
    k0 = dict(kw, centre=(kw["centre"][0], kw["centre"][1], 0.0))
    exact, shaped = piece_refs[True, n_phi, "no_mass"], piece_refs[True, n_phi]
    assert np.array_equal(shaped[:, :17], exact[:, :17]) and not exact[:, 17:].any()
    a = _context(capi, gas, n_owned=note["n_owned"])
    b = _context(capi, gas, n_owned=note["n_owned"], flags=capi.FLAG_HASHED_GRID)
    for ctx, sort in ((a, False), (a, True), (b, True)):
        if sort:
            ctx.density()                                                 # cell-sorted slots
        t, s = ctx.profile(**k0)
        _same_bits(s, exact)
        _cmp_piece_table(capi, ctx, k0, t, exact)
        _same_bits(ctx.profile(**k0, device=True).cpu().numpy(), exact)
        _, s4 = ctx.profile(**kw)
        _same_bits(s4, shaped)                                            # e sums included: the reduction's shape
    assert a.grid_info().kind == 0 and b.grid_info().kind == 1
    a.close(); b.close()


# ---- (f) the AUTO_NORMAL shell ----------------------------------------------------------------------------------------
def test_auto_normal_shell_edges(capi):
    gas = S.auto_shell()[0]
    ctx = _context(capi, gas)
    for which, device in (("shell", False), ("shell", True), ("above_2", False), ("through_8", False)):
        _, _, kw, note = S.auto_shell(which)
        s = ctx.profile(**kw, device=True).cpu().numpy() if device else ctx.profile(**kw)[1]
        n = np.array(ctx.profile_desc.normal[:])
        want_n = profile_ref.axes(note["L"])[0]
        assert np.max(np.abs(n - want_n)) <= 4 * np.finfo(float).eps, (which, n)
        if which == "shell":
            assert np.max(np.abs(n - S.SHELL_NORMAL)) <= 4 * np.finfo(float).eps
        # the rings of the call, in the frame of the shell's L
        want, b = S.reference(gas, kw, normal=note["L"])
        assert np.array_equal(s[:, 0], want[:, 0]) and np.array_equal(s[:, 12], want[:, 12])
        _same_bits(s, want)
    kw = S.auto_shell("only_8")[2]                                       # |r'| = 8 is outside [6, 8): no angular momentum
    with pytest.raises(capi.SphError) as e:
        ctx.profile(**kw)
    assert e.value.status == SPH_ERR_STATE
    ctx.profile(**S.auto_shell("shell")[2])                              # still usable
    ctx.close()


# ---- (g) both branches of the frame rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("normal", S.FRAME_NORMALS)
def test_frame_branches(capi, normal):
    gas, sinks, kw, note = S.frame_branch(normal)
    ctx = make_context(capi, gas, sinks)
    t, s = ctx.profile(**kw)
    r0, r1, nr, nphi, log = S.FRAME_CASE
    rs, rt = existing._ref(capi, ctx, gas, sinks, r0, r1, nr, nphi, log, normal=normal)
    assert s[:, 0].sum() > 5000
    existing._cmp_sums(s, rs)
    existing._cmp_table(capi, t, rt)
    nn, e1, e2 = profile_ref.axes(normal)
    assert np.array_equal(np.array(ctx.profile_desc.normal[:]), nn)
    ctx.close()


# ---- the restatement, to the bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,n_r,n_phi", [(20000, 5, 1, 1), (20000, 5, 16, 4), (70000, 7, 1, 1)])
def test_generic_disc_bitwise_in_the_reduction_shape(capi, n, seed, n_r, n_phi):
    """Per-particle arithmetic in the header's order and the reduction in the header's shape: all 20 sums of a generic disc
    equal the restatement's bits.  70 000 particles in one ring are 69 pieces: the second round of profile_final."""
    gas, sinks = existing._disc(n, seed)
    case = (10.0, 60.0, n_r, n_phi, False)
    if n > 60000:
        case = (0.0, 1.001 * float(np.max(np.hypot(gas["x"], gas["y"]))), n_r, n_phi, False)
    gas = existing._drop_edges(gas, [case])
    ctx = make_context(capi, gas, sinks)
    _, s = ctx.profile(case[0], case[1], n_r, n_phi, sink=0, sums_only=True)
    p = ctx.params
    c, cv = [sinks[k][0] for k in "xyz"], [sinks[k][0] for k in ("vx", "vy", "vz")]
    want, b = profile_ref.profile_sums(gas, p.h, p.G, case[0], case[1], n_r, n_phi, False, np.inf, c, cv, sinks["m"][0],
                                       shape="pieces")
    if n > 60000:
        assert want[0, 0] > 64 * profile_ref.PIECE
    assert np.array_equal(s[:, 0], want[:, 0])
    _same_bits(s, want)
    ctx.close()
