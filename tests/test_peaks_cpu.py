"""CPU tests of the density-peak clumps (sph_peaks): the ABI mirrors (ctypes, Fortran) against the C header, the register
budget of the peaks kernels, the numpy restatement's merge against a naive merge without a union-find, its two limits
(contrast = inf: friends-of-friends; contrast = 1: the raw basins), the disc-with-blobs set that friends-of-friends
cannot separate, and the command line's parsing."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_support import CSRC, c_layout, containing, fortran_links, needs_fc, needs_hipcc, resource_usage
from conftest import ROOT
import groups_ref
import peaks_ref

FIELDS = ["link", "rho_min", "peak_min", "contrast", "clip_lo", "clip_hi", "min_members", "flags", "reserved"]


def test_peaks_desc_layout_matches_header(tmp_path):
    from summersph_amd import capi
    got = c_layout(tmp_path, "sph_peaks_desc", FIELDS,
                   ['printf("consts %d %d %d\\n", SPH_PEAKS_LINK_H, SPH_PEAKS_NCOL, SPH_PEAKS_NCOUNT);'])
    assert int(got["size"]) == ctypes.sizeof(capi.PeaksDesc) == 96
    assert [f for f, _ in capi.PeaksDesc._fields_] == FIELDS
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.PeaksDesc, f).offset, f
    assert got["consts"] == f"{capi.PEAKS_LINK_H} {capi.PEAKS_NCOL} {capi.PEAKS_NCOUNT}" == "1 23 3"
    assert capi.PEAKS_COLUMNS == peaks_ref.COLUMNS and len(capi.PEAKS_COLUMNS) == capi.PEAKS_NCOL
    assert capi.PEAKS_COLUMNS[:capi.GROUPS_NCOL] == capi.GROUPS_COLUMNS and len(capi.PEAKS_COUNTS) == capi.PEAKS_NCOUNT
    assert "sph_peaks" in capi.SYMBOLS and "sph_peaks_dev" in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "summersph.h")).read()
    assert "} sph_peaks_desc;                    /* 96 bytes */" in header
    binding = open(os.path.join(ROOT, "summersph_amd", "host", "sph_hip_binding.f90")).read()
    assert re.search(r"SPH_PEAKS_LINK_H = 1, SPH_PEAKS_NCOL = 23, SPH_PEAKS_NCOUNT = 3", binding)
    d = capi.peaks_desc(0.5, contrast=3.0, rho_min=2.0, peak_min=4.0, min_members=3, link_h=True, clip=((0, 1, 2), (3, 4, 5)))
    assert (d.link, d.contrast, d.rho_min, d.peak_min, d.min_members, d.flags, d.reserved) == (0.5, 3.0, 2.0, 4.0, 3, 1, 0)
    assert list(d.clip_lo) == [0, 1, 2] and list(d.clip_hi) == [3, 4, 5]
    d = capi.peaks_desc(1.0)
    assert d.contrast == 2.0 and d.rho_min == -np.inf and d.peak_min == -np.inf
    assert list(d.clip_lo) == [-np.inf] * 3 and list(d.clip_hi) == [np.inf] * 3


@needs_fc
def test_fortran_binding_compiles_and_links(tmp_path):
    fortran_links(tmp_path, "peaks_caller", """program peaks_caller
  use, intrinsic :: iso_c_binding
  use, intrinsic :: ieee_arithmetic
  use sph_hip_binding
  implicit none
  type(sph_peaks_desc) :: d
  type(c_ptr) :: ctx
  integer(c_int32_t), allocatable, target :: labels(:)
  real(c_double), allocatable, target :: table(:, :)
  integer(c_int64_t) :: counts(SPH_PEAKS_NCOUNT)
  integer(c_int) :: st
  ctx = c_null_ptr
  d%link = 0.5_c_double
  d%rho_min = ieee_value(1.0_c_double, ieee_negative_inf)
  d%peak_min = ieee_value(1.0_c_double, ieee_negative_inf)
  d%contrast = 2.0_c_double
  d%clip_lo = ieee_value(1.0_c_double, ieee_negative_inf)
  d%clip_hi = ieee_value(1.0_c_double, ieee_positive_inf)
  d%min_members = 2_c_int64_t
  d%flags = SPH_PEAKS_LINK_H
  d%reserved = 0
  if (c_sizeof(d) /= 96) stop 1
  allocate(labels(10), table(SPH_PEAKS_NCOL, 4))
  st = sph_peaks(ctx, d, c_loc(labels), 10_c_int64_t, c_loc(table), 4_c_int64_t, counts)
  st = sph_peaks_dev(ctx, d, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, c_null_ptr)
  print *, st, counts
end program peaks_caller
""")


@needs_hipcc
def test_peaks_kernels_fit_the_register_budget():
    k = resource_usage("peaks.hip", containing("peaks_"))
    for name in ("peaks_gather", "peaks_slots", "peaks_hop", "peaks_jump", "peaks_flags", "peaks_compact", "peaks_edge_keys",
                 "peaks_edge_idx", "peaks_scatter", "peaks_assign", "peaks_minid", "peaks_root", "peaks_table"):
        assert sum(name in n for n in k) == 1, name
    assert sum("peaks_edgesILi" in n for n in k) == 2
    for name, r in k.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, (name, r)
        assert 0 < r.get("VGPRs", 999) <= 128, (name, r)
    # no kernel of this feature lives in groups.hip, whose kernels test_groups_cpu.py counts by name
    assert "peaks_" not in open(os.path.join(CSRC, "groups.hip")).read()


def _random_set(seed, n):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 1, (n, 3))
    return {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "vx": rng.normal(size=n), "vy": rng.normal(size=n),
            "vz": rng.normal(size=n), "u": rng.uniform(size=n), "m": rng.uniform(0.5, 1.5, n),
            # a few exact ties and plateaus in rho
            "rho": np.round(rng.uniform(0.1, 1.0, n), 2 if seed % 2 else 12)}


def _naive_merge(ea, eb, es, rho, rank, contrast):
    """the definition without a union-find: take the highest remaining edge (the list is sorted), relabel by arrays"""
    peaks = np.unique(np.concatenate([ea, eb]))
    comp = {int(p): int(p) for p in peaks}                # component label: any member; top kept beside it
    top = {int(p): int(p) for p in peaks}
    remaining = list(range(len(ea)))
    while remaining:
        e = remaining.pop(0)
        A, B = comp[int(ea[e])], comp[int(eb[e])]
        if A == B:
            continue
        if rank[top[A]] < rank[top[B]]:
            A, B = B, A
        with np.errstate(invalid="ignore"):
            ok = rho[top[B]] < np.float64(contrast) * es[e]
        if ok:
            for p in comp:
                if comp[p] == B:
                    comp[p] = A
    return {p: top[comp[p]] for p in comp}


@pytest.mark.parametrize("seed, n, link", [(1, 5000, 0.05), (2, 4000, 0.07), (3, 3000, 0.1)])
def test_merge_matches_a_naive_merge(seed, n, link):
    f = _random_set(seed, n)
    for contrast in (1.0, 1.3, 2.0, 10.0, np.inf):
        a = peaks_ref.peaks(f, n, link, contrast=contrast, min_members=1)
        b = peaks_ref.peaks(f, n, link, contrast=contrast, min_members=1, merger=_naive_merge)
        assert a[2] == b[2] and a[3] == b[3] and a[3][2] > 50
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)
    # the edges are sorted by S descending, then key ascending, and S never exceeds the lower peak
    d = peaks_ref.peaks(f, n, link, detail=True)[4]
    assert np.all(np.diff(d["es"]) <= 0)
    tie = np.diff(d["es"]) == 0
    assert np.all(np.diff(d["ekey"])[tie] > 0)
    assert np.all(d["es"] <= np.minimum(d["rho"][d["ea"]], d["rho"][d["eb"]]))


def test_contrast_inf_is_friends_of_friends():
    for seed, n, link in ((4, 5000, 0.05), (5, 3000, 0.08)):
        f = _random_set(seed, n)
        for kw in ({}, {"min_members": 3, "rho_min": 0.3}):
            lab, t, ng, cnt = peaks_ref.peaks(f, n - 50, link, contrast=np.inf, **kw)
            gl, gt, gn = groups_ref.groups(f, n - 50, link, **kw)
            assert ng == gn == cnt[0] and np.array_equal(lab, gl)
            assert np.array_equal(t[:, :21], gt, equal_nan=True)
            # nothing is left to merge with: every component's S_out is 0; the raw peaks add up
            assert np.all(t[:, 21] == 0)
            if not kw:
                assert t[:, 22].sum() == cnt[1]


def test_contrast_one_gives_the_raw_basins():
    f = _random_set(6, 5000)
    lab, t, ng, cnt, d = peaks_ref.peaks(f, 5000, 0.06, contrast=1.0, detail=True)
    assert ng == cnt[1] and np.all(t[:, 22] == 1)
    assert np.array_equal(np.sort(t[:, 19].astype(np.int64)), np.sort(d["ids"][d["peak"] == np.arange(len(d["ids"]))]))
    # every id_dense is a local maximum of the order: no neighbour is above it
    rank, pairs = d["rank"], d["pairs"]
    tops = t[:, 19].astype(np.int64)
    for side, other in ((0, 1), (1, 0)):
        hit = np.isin(pairs[:, side], tops)
        assert np.all(rank[pairs[hit, side]] > rank[pairs[hit, other]])
    # the invariant of columns 15 and 19, and chains ascend
    assert np.array_equal(t[:, 15], f["rho"][tops])
    assert np.all(rank[d["next"]] >= rank)


def _disc_with_blobs():
    from summersph_amd import ic
    gas, _ = ic.split_rows(ic.keplerian_disc(20000, seed=5))
    rng = np.random.default_rng(6)
    r = np.hypot(gas["x"], gas["y"])
    rmax = float(np.max(r))
    blobs = []
    for j in range(3):
        ang = 2 * np.pi * j / 3
        rc = 15.0 + (rmax - 25.0) * (j + 0.5) / 3
        u = rng.uniform(0, 0.95, 1200)
        rr = 0.2 / np.sqrt(u ** (-2.0 / 3.0) - 1.0)       # Plummer, a = 0.2, truncated at 0.8
        rr = rr[rr < 0.8][:400]
        d = rng.normal(size=(rr.size, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        blobs.append(np.array([rc * np.cos(ang), rc * np.sin(ang), 0.0]) + d * rr[:, None])
    bl = np.concatenate(blobs)
    n0 = gas["x"].size
    pos = np.concatenate([np.stack([gas["x"], gas["y"], gas["z"]], axis=1), bl])
    n = len(pos)
    m = np.full(n, gas["m"][0])
    f = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": np.zeros(n), "vy": np.zeros(n),
         "vz": np.zeros(n), "u": np.ones(n), "m": m, "rho": peaks_ref.kernel_rho(pos, m, 2.5)}
    return f, n0, [len(b) for b in blobs]


def test_blobs_in_a_disc_are_separated_where_fof_percolates():
    pytest.importorskip("scipy.spatial")
    f, n0, sizes = _disc_with_blobs()
    n = len(f["x"])
    gl, gt, gn = groups_ref.groups(f, n, 2.5)
    off, fof = n0, []
    for s in sizes:
        fof.append(np.unique(gl[off:off + s]))
        off += s
    assert all(len(g) == 1 for g in fof) and len({int(g[0]) for g in fof}) == 1       # one component holds all three
    assert gt[int(fof[0][0]), 0] > 0.9 * n
    lab, t, ng, cnt = peaks_ref.peaks(f, n, 2.5, contrast=1.2)
    off, own = n0, []
    for s in sizes:
        vals, c = np.unique(lab[off:off + s], return_counts=True)
        assert c.max() > 0.9 * s                          # the blob sits in one group ...
        own.append(int(vals[np.argmax(c)]))
        off += s
    assert len(set(own)) == 3 and min(own) >= 0           # ... and the three groups differ
    assert sorted(own) == [0, 1, 2]                       # they are the three largest


def test_cli_refuses_bad_arguments(tmp_path, monkeypatch):
    from summersph_amd import capi, groups, peaks
    assert peaks.parse_clip is groups.parse_clip

    def no_context(*a, **k):
        raise AssertionError("a context was made")
    monkeypatch.setattr(capi, "Context", no_context)
    monkeypatch.setattr(peaks, "read_save", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the save file was read")))
    base = ["missing.txt", "-o", str(tmp_path / "o.npz")]
    for extra in (["--link", "0"], ["--link", "-1"], ["--link", "inf"], ["--link", "nan"], ["--link", "1", "--min-members", "0"],
                  ["--link", "1", "--clip", "0,0,0,1,1"], ["--link", "1", "--rho-min", "nan"], ["--link", "1", "--top", "-1"],
                  ["--link", "1", "--contrast", "0.5"], ["--link", "1", "--contrast", "nan"], ["--link", "1", "--peak-min", "nan"],
                  ["--link", "1", "--unbind", "3"], ["--link", "1", "--bound", "--max-members", "0"], []):
        with pytest.raises(SystemExit) as e:
            peaks.main(base + extra)
        assert e.value.code == 2, extra
    assert not (tmp_path / "o.npz").exists()
    # good arguments get as far as the save file
    with pytest.raises(AssertionError, match="the save file was read"):
        peaks.main(base + ["--link", "1", "--link-h", "--contrast", "inf", "--peak-min", "3", "--min-members", "20"])
