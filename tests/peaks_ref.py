"""numpy restatement of sph_peaks (include/summersph.h, "density-peak clumps"): sph_groups' selection and neighbour
relation (groups_ref.select, link_pairs), the order, the hop, the saddles, the sequential merge, dropping, numbering and
the table in the device's fixed shape (groups_ref.shaped_sums).  Written from the definition, not from the GPU code.
kernel_rho (a plain cubic-spline density sum over a cKDTree) serves the tests that have no context to ask for rho."""
import numpy as np

import groups_ref

NCOL = 23
COLUMNS = groups_ref.COLUMNS + ["S_out", "n_peaks"]


def kernel_rho(pos, m, h):
    """rho_i = sum_j m_j W(|r_i - r_j|, h), cubic spline of support 2 h, self term included"""
    from scipy.spatial import cKDTree
    tree = cKDTree(pos)
    pr = tree.query_pairs(2.0 * h, output_type="ndarray")
    q = np.linalg.norm(pos[pr[:, 0]] - pos[pr[:, 1]], axis=1) / h
    w = np.where(q < 1.0, 1.0 - 1.5 * q * q + 0.75 * q ** 3, 0.25 * (2.0 - q) ** 3) / (np.pi * h ** 3)
    rho = m / (np.pi * h ** 3)
    rho = rho + np.bincount(pr[:, 0], weights=m[pr[:, 1]] * w, minlength=len(pos))
    return rho + np.bincount(pr[:, 1], weights=m[pr[:, 0]] * w, minlength=len(pos))


def ranks(rho):
    """rank[i] of the strict total order: a above b iff rho_a > rho_b, or rho_a == rho_b and a < b.  -> (rank, order)"""
    n = len(rho)
    order = np.lexsort((-np.arange(n), rho))              # ascending: the last is the highest
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return rank, order


def hop(rank, order, pairs):
    """next[i]: the highest of i and its neighbours"""
    best = rank.copy()
    np.maximum.at(best, pairs[:, 0], rank[pairs[:, 1]])
    np.maximum.at(best, pairs[:, 1], rank[pairs[:, 0]])
    return order[best]


def chain_lengths(nxt, order):
    """hops from every particle to its peak"""
    depth = np.zeros(len(nxt), dtype=np.int64)
    for i in order[::-1]:                                 # from the highest down: next[i] is done before i
        if nxt[i] != i:
            depth[i] = depth[nxt[i]] + 1
    return depth


def chain_ends(nxt):
    peak = nxt.copy()
    while True:
        pp = peak[peak]
        if np.array_equal(pp, peak):
            return peak
        peak = pp


def saddles(peak, rho, pairs, ids):
    """distinct peak-peak edges: (a, b) local indices with a < b, key = id_a << 32 | id_b, S = max over the pairs of
    min(rho_i, rho_j); sorted by S descending, then key ascending"""
    pi, pj = peak[pairs[:, 0]], peak[pairs[:, 1]]
    cross = pi != pj
    a, b = np.minimum(pi[cross], pj[cross]), np.maximum(pi[cross], pj[cross])
    s = np.minimum(rho[pairs[cross, 0]], rho[pairs[cross, 1]])
    key = (ids[a].astype(np.int64) << 32) | ids[b].astype(np.int64)
    o = np.lexsort((s, key))
    key, s, a, b = key[o], s[o], a[o], b[o]
    last = np.ones(len(key), dtype=bool)
    last[:-1] = key[1:] != key[:-1]                       # the largest s of every key
    key, s, a, b = key[last], s[last], a[last], b[last]
    o = np.lexsort((key, -s))
    return a[o], b[o], key[o], s[o]


def merge(ea, eb, es, rho, rank, contrast):
    """the sequential merge over the sorted edges -> {peak: top} for every peak with an edge"""
    parent, top = {}, {}
    for p in np.unique(np.concatenate([ea, eb])):
        parent[int(p)] = int(p)
        top[int(p)] = int(p)

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    with np.errstate(invalid="ignore"):
        lim = np.float64(contrast) * es                   # rounded once
    for e in range(len(ea)):
        A, B = find(int(ea[e])), find(int(eb[e]))
        if A == B:
            continue
        if rank[top[A]] < rank[top[B]]:
            A, B = B, A
        if rho[top[B]] < lim[e]:
            parent[B] = A
    return {p: top[find(p)] for p in parent}


def table21(f, mem, mg, ng):
    """sph_groups' 21 columns of the members mem (sorted by (group, id)) of groups mg: groups_ref's arithmetic and shape"""
    x, y, z = f["x"], f["y"], f["z"]
    glen = np.bincount(mg, minlength=ng).astype(np.int64)
    gstart = np.cumsum(glen) - glen
    m = f["m"][mem]
    q1 = np.stack([m, m * x[mem], m * y[mem], m * z[mem], m * f["vx"][mem], m * f["vy"][mem], m * f["vz"][mem],
                   m * f["u"][mem]], axis=1)
    s1 = groups_ref.shaped_sums(q1, gstart, glen)
    M = s1[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        R = s1[:, 1:4] / M[:, None]
        V = s1[:, 4:7] / M[:, None]
    dr = np.stack([x[mem], y[mem], z[mem]], axis=1) - R[mg]
    dv = np.stack([f["vx"][mem], f["vy"][mem], f["vz"][mem]], axis=1) - V[mg]
    d2 = (dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2]
    q2 = np.stack([m * d2,
                   m * (dr[:, 1] * dv[:, 2] - dr[:, 2] * dv[:, 1]),
                   m * (dr[:, 2] * dv[:, 0] - dr[:, 0] * dv[:, 2]),
                   m * (dr[:, 0] * dv[:, 1] - dr[:, 1] * dv[:, 0]),
                   (0.5 * m) * ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])], axis=1)
    s2 = groups_ref.shaped_sums(q2, gstart, glen)
    t = np.zeros((ng, NCOL))
    if ng == 0:
        return t
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
    is_max = rho == t[mg, 15]
    first = np.full(ng, -1, dtype=np.int64)
    cand = np.nonzero(is_max)[0][::-1]
    first[mg[cand]] = cand                                # members run in id order: the first maximum of each run
    dense = mem[first]
    t[:, 16], t[:, 17], t[:, 18] = x[dense], y[dense], z[dense]
    t[:, 19] = dense
    t[:, 20] = mem[gstart]
    return t


def peaks(f, n_owned, link, contrast=2.0, rho_min=-np.inf, peak_min=-np.inf, min_members=1, link_h=False, clip=None,
          h=None, merger=merge, detail=False):
    """f: dict of download-order arrays x y z vx vy vz u m rho (and h for link_h unless h is given as a number).
    Returns (labels int32, table (n_groups, NCOL), n_groups, (n_groups, n_raw_peaks, n_edges)); detail=True adds a dict
    with ids, next, peak (local indices), the edges and the top of every selected particle."""
    x, y, z = f["x"], f["y"], f["z"]
    n = len(x)
    sel = groups_ref.select(x, y, z, f["rho"], n_owned, rho_min, clip) & np.isfinite(f["rho"])
    ids = np.nonzero(sel)[0]
    labels = np.full(n, -1, dtype=np.int32)
    if len(ids) == 0:
        out = (labels, np.zeros((0, NCOL)), 0, (0, 0, 0))
        return out + ({},) if detail else out
    pos = np.stack([x[ids], y[ids], z[ids]], axis=1)
    hh = np.zeros(len(ids))
    if link_h:
        hh = np.full(len(ids), float(h)) if np.isscalar(h) else np.asarray(f["h"] if h is None else h)[ids]
        if not np.all((hh > 0) & np.isfinite(hh)):
            raise ValueError("bad h")
    pairs = groups_ref.link_pairs(pos, hh, link, link_h)
    rho = f["rho"][ids]
    rank, order = ranks(rho)
    nxt = hop(rank, order, pairs)
    peak = chain_ends(nxt)
    raw = np.nonzero(peak == np.arange(len(ids)))[0]
    ea, eb, ekey, es = saddles(peak, rho, pairs, ids)
    tmap = merger(ea, eb, es, rho, rank, contrast)
    top_of_peak = np.arange(len(ids))
    for p, t in tmap.items():
        top_of_peak[p] = t
    top = top_of_peak[peak]                               # every selected particle's component, named by its top
    s_out = np.zeros(len(ids))
    diff = top_of_peak[ea] != top_of_peak[eb]
    np.maximum.at(s_out, top_of_peak[ea[diff]], es[diff])
    np.maximum.at(s_out, top_of_peak[eb[diff]], es[diff])
    n_pk = np.bincount(top_of_peak[raw], minlength=len(ids))
    alive = ~(rho[top] < peak_min)
    cnt = np.bincount(top[alive], minlength=len(ids))
    first = np.full(len(ids), len(ids), dtype=np.int64)
    np.minimum.at(first, top[alive], np.nonzero(alive)[0])           # local indices ascend with the ids
    tops = np.nonzero(cnt >= max(min_members, 1))[0]
    tops = tops[np.lexsort((ids[first[tops]], -cnt[tops]))]
    ng = len(tops)
    gnum = np.full(len(ids), -1, dtype=np.int64)
    gnum[tops] = np.arange(ng)
    g_of = np.where(alive, gnum[top], -1)
    labels[ids] = g_of.astype(np.int32)
    keep = g_of >= 0
    mem, mg = ids[keep], g_of[keep]
    o = np.lexsort((mem, mg))
    t = table21(f, mem[o], mg[o], ng)
    t[:, 21] = s_out[tops]
    t[:, 22] = n_pk[tops]
    out = (labels, t, ng, (ng, len(raw), len(ea)))
    if detail:
        return out + ({"ids": ids, "next": nxt, "peak": peak, "order": order, "rank": rank, "rho": rho, "pairs": pairs,
                       "ea": ea, "eb": eb, "ekey": ekey, "es": es, "top": top, "tops": tops, "top_of_peak": top_of_peak},)
    return out
