"""The numpy restatement the sph_track tests compare with: pack()'s renumbering replayed on id arrays, the tracker's log
and fates replayed from per-step downloads of a twin context, and the lookup of particles by their (unique) mass bits."""
import numpy as np

NHEAD, NCOL = 4, 10
COLUMNS = "x y z vx vy vz u rho h alpha".split()
ALIVE, ACCRETED, CULLED = 0, 1, 2


def bits(a):
    """the bit patterns: NaN compares equal to NaN, 0.0 differs from -0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """a log against its restatement: NaN where and only where the other is NaN (the log's fill is the all-ones NaN, numpy's
    the quiet one), every other entry bit for bit"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a[ok]), bits(b[ok]))


def replay_pack(ids, keep):
    """pack() on ids: the survivors are renumbered by rank, new = cumsum(keep) - 1 where kept; a removed id becomes -1 and
    -1 (gone before) stays.  Returns (the new ids, the mask of the ids removed by this pack)."""
    ids = np.asarray(ids, dtype=np.int64)
    keep = np.asarray(keep).astype(bool)
    new = np.cumsum(keep) - 1
    alive = ids >= 0
    kept = np.zeros(ids.shape, bool)
    kept[alive] = keep[ids[alive]]
    out = np.full(ids.shape, -1, dtype=np.int64)
    out[kept] = new[ids[kept]]
    return out, alive & ~kept


def index_by_mass(m_now, m_named):
    """where each named mass sits in m_now (-1: nowhere); the masses are unique bit patterns"""
    where = {int(b): i for i, b in enumerate(bits(m_now))}
    assert len(where) == len(m_now), "the masses are not unique"
    return np.array([where.get(int(b), -1) for b in bits(m_named)], dtype=np.int64)


def keep_of(m_before, m_after):
    """the keep flags of a pack from the masses before and after it"""
    return np.isin(bits(m_before), bits(m_after))


def body_row(fields, idx):
    """one row of the body, (NCOL, K): fields[name][idx[k]] where idx[k] >= 0, NaN elsewhere; a missing or None field is
    NaN throughout (rho where it is not current)"""
    idx = np.asarray(idx, dtype=np.int64)
    out = np.full((NCOL, idx.size), np.nan)
    live = idx >= 0
    for c, name in enumerate(COLUMNS):
        v = fields.get(name)
        if v is None:
            continue
        v = np.broadcast_to(np.asarray(v, dtype=np.float64), np.shape(fields["x"]))
        out[c, live] = v[idx[live]]
    return out
