"""numpy restatement of sph_groups (include/summersph.h, "friends-of-friends groups"): the selection, a vectorised
cell-grid pair search with the exact link predicate, a union-find, the numbering, and both reduction passes in the
device's fixed shape.  Needs numpy only."""
import numpy as np

NCOL = 21
COLUMNS = ["N", "M", "x", "y", "z", "vx", "vy", "vz", "r_rms", "r_max", "Sx", "Sy", "Sz", "K_int", "U", "rho_max",
           "x_dense", "y_dense", "z_dense", "id_dense", "id_min"]
PIECE = 1024
WAVE = 64
AXIS_MASK = (1 << 21) - 1
AXIS_CELLS = float((1 << 21) - 8)
PAIR_CHUNK = 1 << 22          # candidate pairs per vectorised step


def select(x, y, z, rho, n_owned, rho_min=-np.inf, clip=None):
    """bool mask over the particles in download order: owned, rho >= rho_min, strictly inside the clip box"""
    n = len(x)
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    with np.errstate(invalid="ignore"):
        s = np.arange(n) < n_owned
        s &= rho >= rho_min
        for a, p in enumerate((x, y, z)):
            s &= (lo[a] < p) & (p < hi[a])
    return s


def _linked(pi, pj, hi, hj, link, link_h):
    dx = pi[:, 0] - pj[:, 0]
    dy = pi[:, 1] - pj[:, 1]
    dz = pi[:, 2] - pj[:, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    if link_h:
        b = link * np.maximum(hi, hj)
        return d2 < b * b
    return d2 < link * link


def link_pairs(pos, h, link, link_h=False):
    """every linked pair (i < j, indices into pos) of the particles pos (n, 3), by a cell grid of edge >= the largest b"""
    n = len(pos)
    if n < 2:
        return np.zeros((0, 2), dtype=np.int64)
    bmax = link * float(np.max(h)) if link_h else link
    e = bmax * (1.0 + 1e-6)
    lo = pos.min(axis=0)
    ext = pos.max(axis=0) - lo
    for a in range(3):
        if ext[a] / e > AXIS_CELLS:
            e = (ext[a] / AXIS_CELLS) * (1.0 + 1e-6)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.clip(np.nan_to_num(np.floor((pos - lo) * (1.0 / e)), nan=0.0), 0, AXIS_MASK).astype(np.int64)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    ukey, ustart, ucount = np.unique(sk, return_index=True, return_counts=True)
    uc = np.stack([ukey >> 42, (ukey >> 21) & AXIS_MASK, ukey & AXIS_MASK], axis=1)
    sp = pos[order]
    shs = h[order] if link_h else None
    out = []
    for o in range(13, 27):
        off = np.array([o // 9 - 1, (o // 3) % 3 - 1, o % 3 - 1])
        nc = uc + off
        ok = np.all((nc >= 0) & (nc <= AXIS_MASK), axis=1)
        nk = (nc[:, 0] << 42) | (nc[:, 1] << 21) | nc[:, 2]
        idx = np.searchsorted(ukey, nk)
        idx_c = np.minimum(idx, len(ukey) - 1)
        ok &= (idx < len(ukey)) & (ukey[idx_c] == nk)
        a_cells = np.nonzero(ok)[0]
        b_cells = idx_c[a_cells]
        sa, na = ustart[a_cells], ucount[a_cells]
        sb, nb = ustart[b_cells], ucount[b_cells]
        sizes = na * nb
        k0 = 0
        csum = np.cumsum(sizes)
        while k0 < len(a_cells):
            base = csum[k0 - 1] if k0 > 0 else 0
            k1 = max(int(np.searchsorted(csum, base + PAIR_CHUNK, side="right")), k0 + 1)
            sz = sizes[k0:k1]
            tot = int(sz.sum())
            if tot:
                cp = np.repeat(np.arange(k0, k1), sz)
                local = np.arange(tot) - np.repeat(np.cumsum(sz) - sz, sz)
                ia = sa[cp] + local // nb[cp]
                ib = sb[cp] + local % nb[cp]
                if o == 13:
                    keep = ia < ib
                    ia, ib = ia[keep], ib[keep]
                m = _linked(sp[ia], sp[ib], shs[ia] if link_h else None, shs[ib] if link_h else None, link, link_h)
                out.append(np.stack([order[ia[m]], order[ib[m]]], axis=1))
            k0 = k1
    if not out:
        return np.zeros((0, 2), dtype=np.int64)
    p = np.concatenate(out)
    return np.sort(p, axis=1)


def components(n, pairs):
    """root (the smallest index) of every node's component, hooking the larger root under the smaller, then jumping"""
    parent = np.arange(n, dtype=np.int64)
    i, j = pairs[:, 0], pairs[:, 1]
    while len(i):
        ri, rj = parent[i], parent[j]
        live = ri != rj
        i, j, ri, rj = i[live], j[live], ri[live], rj[live]
        if not len(i):
            break
        np.minimum.at(parent, np.maximum(ri, rj), np.minimum(ri, rj))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def _wave(acc):
    """the xor butterfly over the 64 lanes (axis 1 of (S, 64, nq)): lane l adds lane l ^ o for o = 32 .. 1 -> lane 0"""
    s, _, nq = acc.shape
    for o in (32, 16, 8, 4, 2, 1):
        v = acc.reshape(s, WAVE // (2 * o), 2, o, nq)
        acc = (v + v[:, :, ::-1]).reshape(s, WAVE, nq)
    return acc[:, 0, :]


SEG_CHUNK = 1 << 14           # segments per vectorised step


def _shaped(vals, starts, lens):
    """one wavefront per segment: lane l adds vals[start + l + 64 j] for j = 0, 1, ... in turn, then the butterfly"""
    nq = vals.shape[1]
    out = np.zeros((len(starts), nq))
    nj = (lens + WAVE - 1) // WAVE
    for J in np.unique(nj):
        if J == 0:
            continue
        allsel = np.nonzero(nj == J)[0]
        rel = (np.arange(J)[:, None] * WAVE + np.arange(WAVE)[None, :])[None]       # (1, J, 64)
        for c0 in range(0, len(allsel), SEG_CHUNK):
            sel = allsel[c0:c0 + SEG_CHUNK]
            valid = rel < lens[sel][:, None, None]
            pos = np.where(valid, starts[sel][:, None, None] + rel, 0)
            a = np.where(valid[..., None], vals[pos], 0.0)                             # (S, J, 64, nq)
            acc = np.zeros((len(sel), WAVE, nq))
            for j in range(J):
                acc = acc + a[:, j]
            out[sel] = _wave(acc)
    return out


def shaped_sums(vals, gstart, glen):
    """the device's order rule: each group's run of vals (sorted by id) in pieces of 1024 from its start, a wavefront per
    piece, then one wavefront over the pieces"""
    npc = (glen + PIECE - 1) // PIECE
    pg = np.repeat(np.arange(len(gstart)), npc)
    pk = np.arange(int(npc.sum())) - np.repeat(np.cumsum(npc) - npc, npc)
    ps = gstart[pg] + pk * PIECE
    pl = np.minimum(PIECE, glen[pg] - pk * PIECE)
    part = _shaped(vals, ps, pl)
    return _shaped(part, np.cumsum(npc) - npc, npc)


def groups(f, n_owned, link, rho_min=-np.inf, min_members=1, link_h=False, clip=None, h=None):
    """f: dict of download-order arrays x y z vx vy vz u m rho (and h for link_h unless h is given as a number).
    Returns (labels int32, table (n_groups, NCOL), n_groups)."""
    x, y, z = f["x"], f["y"], f["z"]
    n = len(x)
    sel = select(x, y, z, f["rho"], n_owned, rho_min, clip)
    ids = np.nonzero(sel)[0]
    labels = np.full(n, -1, dtype=np.int32)
    if len(ids) == 0:
        return labels, np.zeros((0, NCOL)), 0
    pos = np.stack([x[ids], y[ids], z[ids]], axis=1)
    hh = None
    if link_h:
        hh = np.full(len(ids), float(h)) if np.isscalar(h) else np.asarray(f["h"] if h is None else h)[ids]
        if not np.all((hh > 0) & np.isfinite(hh)):
            raise ValueError("bad h")
    pairs = link_pairs(pos, hh if link_h else np.zeros(len(ids)), link, link_h)
    root = components(len(ids), pairs)                 # local indices; ids ascend, so the smallest local = smallest id
    cnt = np.bincount(root, minlength=len(ids))
    roots = np.nonzero((root == np.arange(len(ids))) & (cnt >= min_members))[0]
    order = np.lexsort((ids[roots], -cnt[roots]))
    roots = roots[order]
    ng = len(roots)
    gnum = np.full(len(ids), -1, dtype=np.int64)
    gnum[roots] = np.arange(ng)
    g_of = gnum[root]
    labels[ids] = g_of.astype(np.int32)
    keep = g_of >= 0
    mem = ids[keep]
    mg = g_of[keep]
    o = np.lexsort((mem, mg))
    mem, mg = mem[o], mg[o]
    glen = np.bincount(mg, minlength=ng).astype(np.int64)
    gstart = np.cumsum(glen) - glen
    m = f["m"][mem]
    q1 = np.stack([m, m * x[mem], m * y[mem], m * z[mem], m * f["vx"][mem], m * f["vy"][mem], m * f["vz"][mem],
                   m * f["u"][mem]], axis=1)
    s1 = shaped_sums(q1, gstart, glen)
    M = s1[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        R = s1[:, 1:4] / M[:, None]
        V = s1[:, 4:7] / M[:, None]
    Rm, Vm = R[mg], V[mg]
    dr = np.stack([x[mem], y[mem], z[mem]], axis=1) - Rm
    dv = np.stack([f["vx"][mem], f["vy"][mem], f["vz"][mem]], axis=1) - Vm
    d2 = (dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2]
    q2 = np.stack([m * d2,
                   m * (dr[:, 1] * dv[:, 2] - dr[:, 2] * dv[:, 1]),
                   m * (dr[:, 2] * dv[:, 0] - dr[:, 0] * dv[:, 2]),
                   m * (dr[:, 0] * dv[:, 1] - dr[:, 1] * dv[:, 0]),
                   (0.5 * m) * ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])], axis=1)
    s2 = shaped_sums(q2, gstart, glen)
    t = np.zeros((ng, NCOL))
    t[:, 0] = glen
    t[:, 1] = M
    t[:, 2:5] = R
    t[:, 5:8] = V
    with np.errstate(invalid="ignore", divide="ignore"):
        t[:, 8] = np.sqrt(s2[:, 0] / M)
    t[:, 9] = np.maximum.reduceat(np.sqrt(d2), gstart)
    t[:, 10:13] = s2[:, 1:4]
    t[:, 13] = s2[:, 4]
    t[:, 14] = s1[:, 7]
    rho = f["rho"][mem]
    t[:, 15] = np.maximum.reduceat(rho, gstart)
    # the densest member, the smallest id on ties: members run in id order, so the first maximum of each run
    is_max = rho == t[mg, 15]
    first = np.full(ng, -1, dtype=np.int64)
    cand = np.nonzero(is_max)[0][::-1]
    first[mg[cand]] = cand
    dense = mem[first]
    t[:, 16], t[:, 17], t[:, 18] = x[dense], y[dense], z[dense]
    t[:, 19] = dense
    t[:, 20] = mem[gstart]
    return labels, t, ng
