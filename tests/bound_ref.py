"""numpy restatement of sph_bound (include/summersph.h, "binding energies and unbinding of clumps"): one evaluation of a
member set (the group's own softened potential by the chunked direct sum of energy_ref, the members' energies in the
set's frame, the set's sums), the round rule with its statuses, the table, the labels and the counts.

The restatement asserts its own precondition: in every evaluation of every group each member's |e_i| exceeds MARGIN times
k_i + f u_i + |Phi_i|, so that no removal hangs on rounding.  A member with Phi_i == 0 exactly (a set of one, or only
massless companions) is exempt: its e_i = k_i + f u_i is a sum of non-negative terms, never < 0 whatever the rounding."""
import numpy as np

import energy_ref

NCOL = 24
MARGIN = 1e-9
COLUMNS = ["N0", "M0", "K0", "U0", "W0", "E0", "virial0", "N", "M", "x", "y", "z", "vx", "vy", "vz", "K", "U", "W", "E",
           "n_bound", "rounds", "status", "id_most_bound", "e_most_bound"]
EXACT = ("N0", "N", "n_bound", "rounds", "status", "id_most_bound")
SOFT2 = energy_ref.SOFT2


def members(f, labels, n_owned, n_groups):
    """ascending original ids of every group's members: owned, finite position, 0 <= label < n_groups"""
    x, y, z = (np.asarray(f[k], dtype=np.float64) for k in "xyz")
    lab = np.asarray(labels)
    ok = (np.arange(lab.size) < n_owned) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (lab >= 0) & (lab < n_groups)
    ids = np.nonzero(ok)[0]
    order = np.argsort(lab[ids], kind="stable")
    ids, gl = ids[order], lab[ids][order]
    start = np.searchsorted(gl, np.arange(n_groups + 1))
    return [ids[start[g]:start[g + 1]] for g in range(n_groups)]


def evaluate(f, S, h, G, soft2=SOFT2, thermal=False):
    """one evaluation of the member set S (ids, ascending): dict of M, V, phi, k, e, the sums and their scales (the sums of
    the terms' absolute values)"""
    m = np.asarray(f["m"], dtype=np.float64)[S]
    pos = np.stack([np.asarray(f[k], dtype=np.float64)[S] for k in "xyz"], axis=1)
    vel = np.stack([np.asarray(f[k], dtype=np.float64)[S] for k in ("vx", "vy", "vz")], axis=1)
    u = np.asarray(f["u"], dtype=np.float64)[S]
    hh = np.full(S.size, float(h)) if np.isscalar(h) else np.asarray(h, dtype=np.float64)[S]
    with np.errstate(invalid="ignore", divide="ignore"):
        M = m.sum()
        V = (m[:, None] * vel).sum(axis=0) / M
        phi = energy_ref.self_potential(pos[:, 0], pos[:, 1], pos[:, 2], m, hh, G, soft2=soft2)
        dv = vel - V
        k = 0.5 * ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
        fu = u if thermal else np.zeros_like(u)
        e = (k + fu) + phi
        mr = (m[:, None] * pos).sum(axis=0)
        out = {"M": M, "V": V, "phi": phi, "k": k, "e": e, "e_scale": k + fu + np.abs(phi),
               "K": np.sum(m * k), "U": np.sum(m * u), "W": np.sum(0.5 * m * phi), "R": mr / M,
               "sM": np.sum(np.abs(m)), "sK": np.sum(np.abs(m * k)), "sU": np.sum(np.abs(m * u)),
               "sW": np.sum(np.abs(0.5 * m * phi)), "sR": np.abs(m[:, None] * pos).sum(axis=0) / M,
               "sV": np.abs(m[:, None] * vel).sum(axis=0) / M}
    return out


def bound(f, labels, n_owned, n_groups, G, h, soft2=SOFT2, thermal=False, max_rounds=0, min_members=1,
          max_members=2**31 - 1, check_margin=True):
    """f: dict of download-order arrays x y z vx vy vz u m; h: one number or the per-particle array.
    Returns (bound_labels int32, e, phi, table (n_groups, NCOL), counts[4], info) -- info: "scale" (n_groups, NCOL), what a
    relative tolerance of a table entry is relative to (0 for the exact columns); "e_scale" per particle; "margin", the
    smallest |e| / (k + f u + |Phi|) met; "evaluations" per group."""
    n = np.asarray(f["x"]).size
    fl = 1.0 if thermal else 0.0
    bl = np.full(n, -1, dtype=np.int32)
    e_out = np.full(n, np.nan)
    phi_out = np.full(n, np.nan)
    e_scale = np.full(n, np.nan)
    table = np.full((n_groups, NCOL), np.nan)
    scale = np.zeros((n_groups, NCOL))
    counts = [0, 0, 0, 0]
    margin = np.inf
    evaluations = np.zeros(n_groups, dtype=np.int64)
    for g, mem in enumerate(members(f, labels, n_owned, n_groups)):
        row, sc = table[g], scale[g]
        n0 = mem.size
        counts[0] += n0
        row[0] = n0
        if n0 > max_members:
            row[21] = 3
            counts[1] += 1
            continue
        if n0 < min_members:
            row[[7, 8, 19, 20]] = 0.0
            row[21], row[22] = 2, -1
            counts[2] += 1
            continue
        S, R = mem, 0
        while True:
            ev = evaluate(f, S, h, G, soft2, thermal)
            evaluations[g] += 1
            e = ev["e"]
            e_out[S], phi_out[S], e_scale[S] = e, ev["phi"], ev["e_scale"]
            if check_margin:
                decided = ev["phi"] != 0.0
                with np.errstate(invalid="ignore", divide="ignore"):
                    mg = np.abs(e[decided]) / ev["e_scale"][decided]
                assert np.all(mg > MARGIN), (g, R, float(np.min(mg)))
                margin = min(margin, float(np.min(mg, initial=np.inf)))
            KU, sKU = ev["K"] + fl * ev["U"], ev["sK"] + fl * ev["sU"]
            if R == 0:
                row[1:7] = [ev["M"], ev["K"], ev["U"], ev["W"], KU + ev["W"], KU / abs(ev["W"]) if ev["W"] != 0 else np.nan]
                if ev["W"] == 0 and not np.isnan(KU):
                    row[6] = np.inf if KU > 0 else np.nan
                # K + f U and W are sums of terms of one sign: each to 1e-12 of itself, their ratio to twice that
                sc[1:7] = [ev["sM"], ev["sK"], ev["sU"], ev["sW"], sKU + ev["sW"], 2.5 * abs(row[6])]
            neg = e < 0.0
            nneg = int(neg.sum())
            st = 0 if nneg == S.size else (1 if R >= max_rounds else (2 if nneg < min_members else -1))
            if st == -1:
                S, R = S[neg], R + 1
                continue
            row[20], row[21] = R, st
            if st == 2:
                row[[7, 8, 19]] = 0.0
                row[22] = -1
                sc[7:] = 0.0
                counts[2] += 1
            else:
                row[7], row[8] = S.size, ev["M"]
                row[9:12], row[12:15] = ev["R"], ev["V"]
                row[15:19] = [ev["K"], ev["U"], ev["W"], KU + ev["W"]]
                sc[8] = ev["sM"]
                sc[9:12], sc[12:15] = ev["sR"], ev["sV"]
                sc[15:19] = [ev["sK"], ev["sU"], ev["sW"], sKU + ev["sW"]]
                row[19] = nneg
                if np.any(~np.isnan(e)):
                    j = int(np.nanargmin(e))                 # the first of equal minima: the smallest id
                    row[22], row[23], sc[23] = S[j], e[j], ev["e_scale"][j]
                else:
                    row[22] = -1
                bl[S[neg]] = g
                counts[3] += st == 1
            break
    info = {"scale": scale, "e_scale": e_scale, "margin": margin, "evaluations": evaluations}
    return bl, e_out, phi_out, table, counts, info


# ---- the GPU test set: Gaussian blobs far apart, one group each ----------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000)
KINDS = ("cold", "cold", "cold", "hot", "halo", "cold", "hot", "halo", "cold", "halo", "hot", "halo")
N_GHOST = 200
COINCIDENT_GROUP, MASSLESS_GROUP = 5, 6


def blob_set(G, seed=11):
    """(gas, sinks, labels, n_owned, n_groups): len(SIZES) blobs of total mass 0.01 each -- cold (bound as they are), hot
    (every member unbound) and halo (a cold core in a halo whose speeds straddle the escape speed: several rounds) --
    shuffled over the ids; two coincident members in one cold blob, a massless member in a hot one; particles with label
    -1, -7 and labels >= n_groups; N_GHOST trailing particles that carry valid labels and are to be declared ghosts; h per
    particle for a variable-h context; one sink."""
    rng = np.random.default_rng(seed)
    ng = len(SIZES)
    pos, vel, lab, mass = [], [], [], []

    def unit(k):
        d = rng.normal(size=(k, 3))
        return d / np.linalg.norm(d, axis=1)[:, None]
    for g, (N, kind) in enumerate(zip(SIZES, KINDS)):
        centre = np.array([60.0 * (g % 4), 60.0 * (g // 4), 5.0 * g])
        v0 = np.sqrt(G * 0.01)
        p = rng.normal(0, 1.0, (N, 3))
        v = rng.normal(0, 0.1 * v0, (N, 3))
        if kind == "hot":
            v = rng.normal(0, 3.0 * v0, (N, 3))
        elif kind == "halo":
            nh = N // 2
            p[:nh] = rng.normal(0, 3.0, (nh, 3))
            v[:nh] = unit(nh) * (rng.uniform(0.0, 1.6, nh) * v0)[:, None]
        if N == 2:
            p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
        pos.append(p + centre)
        vel.append(v + rng.normal(0, 2.0, 3))
        lab.append(np.full(N, g))
        mass.append(np.full(N, 0.01 / N))
    pos[COINCIDENT_GROUP][1] = pos[COINCIDENT_GROUP][0]
    mass[MASSLESS_GROUP][3] = 0.0
    # particles in no group: labels -1, -7, n_groups, 99 and 2^31 - 1, placed inside the blobs
    k = 250
    pos.append(np.concatenate(pos[:ng])[rng.integers(0, sum(SIZES), k)] + rng.normal(0, 0.5, (k, 3)))
    vel.append(rng.normal(0, 1.0, (k, 3)))
    lab.append(rng.choice([-1, -7, ng, 99, 2**31 - 1], k))
    mass.append(np.full(k, 1e-4))
    pos, vel, lab, mass = np.concatenate(pos), np.concatenate(vel), np.concatenate(lab), np.concatenate(mass)
    perm = rng.permutation(pos.shape[0])
    pos, vel, lab, mass = pos[perm], vel[perm], lab[perm], mass[perm]
    # ghosts: copies of owned members with their labels
    src = rng.integers(0, pos.shape[0], N_GHOST)
    pos = np.concatenate([pos, pos[src] + rng.normal(0, 0.2, (N_GHOST, 3))])
    vel, lab, mass = np.concatenate([vel, vel[src]]), np.concatenate([lab, lab[src]]), np.concatenate([mass, mass[src]])
    n = pos.shape[0]
    gas = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "vx": vel[:, 0].copy(), "vy": vel[:, 1].copy(),
           "vz": vel[:, 2].copy(), "u": rng.uniform(0.001, 0.002, n), "m": mass, "alpha": np.ones(n),
           "h": rng.uniform(0.15, 0.5, n)}
    sinks = {"x": np.array([30.0]), "y": np.array([30.0]), "z": np.array([0.0]), "vx": np.zeros(1), "vy": np.zeros(1),
             "vz": np.zeros(1), "m": np.array([1.0])}
    return gas, sinks, lab.astype(np.int32), n - N_GHOST, ng
