"""CPU tests of the friends-of-friends groups (sph_groups): the ABI mirrors (ctypes, Fortran) against the C header, the
register budget of the groups kernels, the numpy restatement against scipy's connected components and a brute-force
pair search, its order rule, and the command line's parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import groups_ref

FIELDS = ["link", "rho_min", "clip_lo", "clip_hi", "min_members", "flags", "reserved"]


def test_groups_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_groups_desc", FIELDS, ['printf("consts %d %d\\n", SPH_GROUPS_LINK_H, SPH_GROUPS_NCOL);'])
    assert int(got["size"]) == ctypes.sizeof(capi.GroupsDesc) == 80
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.GroupsDesc, f).offset, f
    assert got["consts"] == f"{capi.GROUPS_LINK_H} {capi.GROUPS_NCOL}" == "1 21"
    assert capi.GROUPS_COLUMNS == groups_ref.COLUMNS and len(capi.GROUPS_COLUMNS) == capi.GROUPS_NCOL
    assert "sph_groups" in capi.SYMBOLS and "sph_groups_dev" in capi.SYMBOLS
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_GROUPS_LINK_H = 1, SPH_GROUPS_NCOL = 21", binding)
    d = capi.groups_desc(0.5, rho_min=2.0, min_members=3, link_h=True, clip=((0, 1, 2), (3, 4, 5)))
    assert (d.link, d.rho_min, d.min_members, d.flags, d.reserved) == (0.5, 2.0, 3, 1, 0)
    assert list(d.clip_lo) == [0, 1, 2] and list(d.clip_hi) == [3, 4, 5]
    d = capi.groups_desc(1.0)
    assert d.rho_min == -np.inf and list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "groups_caller", """program groups_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_groups_desc) :: d
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable, target :: labels(:)
  real(c_double), allocatable, target :: table(:, :)
  integer(c_int64_t) :: ng
  integer(c_int) :: st
  ctx = c_null_ptr
  d%link = 0.5_c_double
  d%rho_min = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%min_members = 2_c_int64_t
  d%flags = SPH_GROUPS_LINK_H
  d%reserved = 0
  if (c_sizeof(d) /= 80) stop 1
  allocate(labels(10), table(SPH_GROUPS_NCOL, 4))
  st = sph_groups(ctx, d, c_loc(labels), 10_c_int64_t, c_loc(table), 4_c_int64_t, ng)
  st = sph_groups_dev(ctx, d, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, c_null_ptr)
  print *, st, ng
end program groups_caller
""")


@needs_hipcc
def test_groups_kernels_fit_the_register_budget():
    k = resource_usage("groups.hip", containing("groups_"))
    for name in ("groups_select", "groups_box", "groups_keys", "groups_gather", "groups_tails", "groups_link", "groups_jump",
                 "groups_count", "groups_root_keys", "groups_number", "groups_members", "groups_starts"):
        assert sum(name in n for n in k) == 1, name
    assert sum("groups_pieces" in n for n in k) == 2 and sum("groups_final" in n for n in k) == 2
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)


def _brute_pairs(pos, link):
    d = pos[:, None, :] - pos[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    i, j = np.nonzero(np.triu(d2 < link * link, 1))
    return np.stack([i, j], axis=1)


def test_pair_search_matches_brute_force():
    rng = np.random.default_rng(3)
    for n, link in ((1500, 0.08), (1500, 0.3), (800, 5.0)):
        pos = rng.uniform(0, 1, (n, 3)) * [1.0, 2.0, 0.5]
        got = groups_ref.link_pairs(pos, np.zeros(n), link)
        want = _brute_pairs(pos, link)
        assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    # variable b = link * max(h_i, h_j)
    pos = rng.uniform(0, 1, (1200, 3))
    h = rng.uniform(0.02, 0.1, 1200)
    got = groups_ref.link_pairs(pos, h, 0.8, link_h=True)
    d = pos[:, None, :] - pos[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    b = 0.8 * np.maximum(h[:, None], h[None, :])
    i, j = np.nonzero(np.triu(d2 < b * b, 1))
    assert np.array_equal(got[np.lexsort(got.T[::-1])], np.stack([i, j], axis=1))


def test_restatement_matches_scipy_connected_components():
    sp = pytest.importorskip("scipy.sparse")
    cg = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(5)
    for n, link in ((5000, 0.05), (5000, 0.07), (3000, 0.2)):
        pos = rng.uniform(0, 1, (n, 3))
        pairs = groups_ref.link_pairs(pos, np.zeros(n), link)
        root = groups_ref.components(n, pairs)
        g = sp.coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
        nc, lab = cg.connected_components(g, directed=False)
        assert np.unique(root).size == nc
        # the same partition: root and scipy's label determine each other
        assert np.unique(np.stack([root, lab], axis=1), axis=0).shape[0] == nc
        assert np.all(root <= np.arange(n)) and np.all(root[root] == root)


def test_restatement_numbering_and_table():
    rng = np.random.default_rng(7)
    n = 4000
    pos = rng.uniform(0, 1, (n, 3))
    f = {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "vx": rng.normal(size=n), "vy": rng.normal(size=n),
         "vz": rng.normal(size=n), "u": rng.uniform(size=n), "m": rng.uniform(0.5, 1.5, n), "rho": rng.uniform(size=n)}
    lab, t, ng = groups_ref.groups(f, n - 100, 0.06, min_members=2, rho_min=0.05)
    assert np.all(lab[n - 100:] == -1) and np.all(lab[f["rho"] < 0.05] == -1)
    assert np.all(np.diff(t[:, 0]) <= 0)                                  # N descending
    tie = t[1:, 0] == t[:-1, 0]
    assert np.all(t[1:, 20][tie] > t[:-1, 20][tie])                       # then the smallest id
    for g in range(ng):
        mem = np.nonzero(lab == g)[0]
        m = f["m"][mem]
        assert t[g, 0] == mem.size >= 2 and t[g, 20] == mem[0]
        M = m.sum()
        assert abs(t[g, 1] - M) <= 1e-13 * M
        R = np.array([np.sum(m * f[k][mem]) for k in "xyz"]) / M
        assert np.max(np.abs(t[g, 2:5] - R)) <= 1e-13
        j = mem[np.argmax(f["rho"][mem])]
        assert t[g, 15] == f["rho"][j] and t[g, 19] == j and t[g, 16] == f["x"][j]
        dr = pos[mem] - R
        assert abs(t[g, 9] - np.sqrt(np.max(np.sum(dr * dr, axis=1)))) <= 1e-14


def test_shaped_sums_follow_the_wavefront_order():
    rng = np.random.default_rng(9)
    v = rng.normal(size=(5000, 1)) * 10.0 ** rng.integers(-8, 8, (5000, 1))
    glen = np.array([1, 63, 64, 65, 1024, 1025, 2800 - 2242, 2242 - 0])
    glen[-1] = 5000 - glen[:-1].sum()
    gs = np.cumsum(glen) - glen
    got = groups_ref.shaped_sums(v, gs, glen)[:, 0]

    def wave(vals):
        lanes = np.zeros(64)
        for p, x in enumerate(vals):
            lanes[p % 64] = lanes[p % 64] + x
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[idx ^ o]
        return lanes[0]

    for g in range(len(glen)):
        seg = v[gs[g]:gs[g] + glen[g], 0]
        pieces = [wave(seg[k:k + 1024]) for k in range(0, len(seg), 1024)]
        assert got[g] == wave(pieces), g


def test_cli_parses_clip_and_refuses_bad_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, groups
    assert groups.parse_clip("0,1,2,3,4,5") == ((0.0, 1.0, 2.0), (3.0, 4.0, 5.0))
    assert groups.parse_clip("-inf,0,0,inf,1,1") == ((-np.inf, 0.0, 0.0), (np.inf, 1.0, 1.0))
    for bad in ("1,2,3", "0,0,0,1,1,nan", "2,0,0,1,1,1", "a,b,c,d,e,f", ""):
        with pytest.raises(ValueError):
            groups.parse_clip(bad)

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    monkeypatch.setattr(groups, "read_save", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the save file was read")))
    base = ["missing.txt", "-o", str(tmp_path / "o.npz")]
    for extra in (["--link", "0"], ["--link", "-1"], ["--link", "inf"], ["--link", "nan"], ["--link", "1", "--min-members", "0"],
                  ["--link", "1", "--clip", "0,0,0,1,1"], ["--link", "1", "--rho-min", "nan"], ["--link", "1", "--top", "-1"], []):
        with pytest.raises(SystemExit) as e:
            groups.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
