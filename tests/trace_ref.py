"""numpy restatement of sph_trace's contract (include/summersph.h, "field lines of an SPH-interpolated vector field").

trace_with(sampler, ...) is the contract's step, frame, options and stops in float64 numpy, written in the header's order
(numpy never fuses a multiply into an add); the field comes from `sampler(points) -> (w (K, n), den (n,))`, w being the
NORMALISED values (0 where den == 0), row 3 the carry.  trace(...) plugs in sample_ref.sample; brute_sampler(...) is an
O(N M) sampler that uses neither sample_ref nor a KD-tree; the GPU tests plug in Context.sample and so pin the arithmetic
of the walk kernel bit for bit."""
import numpy as np

import sample_ref

DONE, LEFT_GAS, LEFT_BOX, STAGNANT, NONFINITE = range(5)
RUNNING = -1


def unit_normal(normal):
    """normal / sqrt((nx nx + ny ny) + nz nz): the host's normalisation"""
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    return n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])


def velocity(q, w, omega, centre, normal, arclength):
    """(v (n, 3), ok (n,)) of the stage points q (n, 3) with the sampled w (n, 3): frame, PLANAR, ARCLENGTH in the header's
    order; ok is False where ARCLENGTH finds sp == 0 or a non-finite sp"""
    t = q - centre
    f = np.stack([omega[1] * t[:, 2] - omega[2] * t[:, 1], omega[2] * t[:, 0] - omega[0] * t[:, 2],
                  omega[0] * t[:, 1] - omega[1] * t[:, 0]], axis=1)
    v = w - f
    if normal is not None:
        d = (v[:, 0] * normal[0] + v[:, 1] * normal[1]) + v[:, 2] * normal[2]
        v = v - d[:, None] * normal[None, :]
    ok = np.ones(q.shape[0], dtype=bool)
    if arclength:
        with np.errstate(all="ignore"):
            sp = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            ok = (sp > 0.0) & np.isfinite(sp)
            v = v / sp[:, None]
    return v, ok


def trace_with(sampler, seeds, n_steps, ds, arclength=False, omega=None, centre=(0.0, 0.0, 0.0), normal=None, box=None, stride=1,
               carry=False, dens=None):
    """(path (n_rec + 1, 3, M), status (M,) int32, n_done (M,) int32[, carry (n_rec + 1, M)]).  dens: a list that receives the
    den of every stage evaluation of every line (one array per call of the sampler that a step used)."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    M = seeds.shape[0]
    assert n_steps >= 1 and stride >= 1 and n_steps % stride == 0 and ds != 0.0 and np.isfinite(ds)
    n_rec = n_steps // stride
    ds = np.float64(ds)
    hs, s6 = 0.5 * ds, ds / 6.0
    omega = np.zeros(3) if omega is None else np.asarray(omega, dtype=np.float64)
    centre = np.asarray(centre, dtype=np.float64)
    nrm = None if normal is None else unit_normal(normal)
    lo, hi = (np.full(3, -np.inf), np.full(3, np.inf)) if box is None else (np.asarray(box[0], float), np.asarray(box[1], float))
    path = np.full((n_rec + 1, 3, M), np.nan)
    car = np.full((n_rec + 1, M), np.nan)
    status = np.full(M, RUNNING, dtype=np.int32)
    done = np.zeros(M, dtype=np.int32)
    p = seeds.copy()
    fin = np.isfinite(seeds).all(axis=1)
    status[~fin] = NONFINITE
    path[0][:, fin] = p[fin].T
    for s in range(n_steps + 1):
        act = np.nonzero(status == RUNNING)[0]
        if act.size == 0:
            break
        rec_here = s % stride == 0
        with np.errstate(invalid="ignore"):
            inside = ((p[act] > lo) & (p[act] < hi)).all(axis=1)
        last = ~inside | (s == n_steps)
        end_code = np.where(inside, DONE, LEFT_BOX).astype(np.int32)
        if not (carry and rec_here):
            status[act[last]] = end_code[last]
            act, end_code, last = act[~last], end_code[~last], last[~last]
            if act.size == 0:
                continue
        w, den = sampler(p[act])
        if carry and rec_here:
            car[s // stride, act] = w[3]
        status[act[last]] = end_code[last]
        keep = ~last
        act, w, den = act[keep], w[:, keep], den[keep]
        n = act.size
        if n == 0:
            continue
        alive = np.ones(n, dtype=bool)
        A, B, q = np.zeros((n, 3)), np.zeros((n, 3)), p[act].copy()
        for stg in range(4):
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                break
            if stg > 0:
                w, den = sampler(q[idx])
            if dens is not None:
                dens.append(np.array(den))
            gas = den != 0.0
            status[act[idx[~gas]]] = LEFT_GAS
            alive[idx[~gas]] = False
            idx = idx[gas]
            v, ok = velocity(q[idx], w[:3, gas].T, omega, centre, nrm, arclength)
            status[act[idx[~ok]]] = STAGNANT
            alive[idx[~ok]] = False
            idx, v = idx[ok], v[ok]
            if stg == 0:
                A[idx] = v
            elif stg == 1:
                A[idx] = A[idx] + 2.0 * v
            elif stg == 2:
                B[idx] = 2.0 * v
            else:
                B[idx] = B[idx] + v
            if stg < 3:
                q[idx] = p[act[idx]] + (ds if stg == 2 else hs) * v
        idx = np.nonzero(alive)[0]
        g = act[idx]
        with np.errstate(all="ignore"):
            p[g] = p[g] + s6 * (A[idx] + B[idx])
        done[g] += 1
        if (s + 1) % stride == 0:
            path[(s + 1) // stride][:, g] = p[g].T
    assert not np.any(status == RUNNING)
    return (path, status, done, car) if carry else (path, status, done)


def ref_sampler(pos, m, h, A, rho=None, n_owned=None, clip=None):
    """sample_ref.sample(..., normalise=True) as a sampler; A: 3 rows, or 4 with a carry"""
    def f(q):
        out, den, _ = sample_ref.sample(q, pos, m, h, A, rho, n_owned, clip, normalise=True)
        return out, den
    return f


def brute_sampler(pos, m, h, A, rho=None):
    """the O(N M) form: every pair's distance, the cubic spline written out, no selection (all particles are sources)"""
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (pos.shape[0],))
    ws = (m if rho is None else m / rho) / (np.pi * h ** 3)

    def f(q):
        r = np.sqrt(((q[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)) / h[None, :]
        wn = np.where(r <= 1.0, 1.0 - 1.5 * r ** 2 + 0.75 * r ** 3, np.where(r <= 2.0, 0.25 * (2.0 - r) ** 3, 0.0))
        den = (ws[None, :] * wn).sum(axis=1)
        num = np.stack([(ws[None, :] * A[k][None, :] * wn).sum(axis=1) for k in range(A.shape[0])])
        out = np.zeros_like(num)
        nz = den != 0.0
        out[:, nz] = num[:, nz] / den[nz]
        return out, den
    return f


def trace(seeds, pos, m, h, A, n_steps, ds, rho=None, n_owned=None, clip=None, **kw):
    """the restatement over sample_ref: A (3, N) the vector's rows, or (4, N) with carry=True"""
    return trace_with(ref_sampler(pos, m, h, np.asarray(A, dtype=np.float64), rho, n_owned, clip), seeds, n_steps, ds, **kw)


def parity_seeds(pos, h, gen_seed, n=256, n_far=16):
    """the parity tests' seed set: n particle positions + N(0, 0.3 h) (h: one number or the particles' own), the first n_far
    scaled x 3 to start outside the gas"""
    rng = np.random.default_rng(gen_seed)
    pick = rng.choice(pos.shape[0], n, replace=False)
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (pos.shape[0],))[pick]
    s = pos[pick] + rng.normal(size=(n, 3)) * (0.3 * hh)[:, None]
    s[:n_far] *= 3.0
    return s


# the parity cases of tests/test_trace_cpu.py (the seed set is decisive) and tests/test_trace_gpu.py (parity): golden set,
# desc.h (None: the particles' own), ARCLENGTH, ds (a length with ARCLENGTH, else a time), the seed generator's seed
PARITY_STEPS = 16
PARITY_CASES = [
    ("disc3000_eval", 2.7, True, 0.5, 2), ("disc3000_eval", 2.7, False, 2.0, 2),
    ("disc3000_eval", 5.4, True, 0.5, 2), ("disc3000_eval", 5.4, False, 2.0, 2),
    ("discv3000_eval", None, True, 0.5, 1), ("discv3000_eval", None, False, 2.0, 1),
]


def parity_case(gas, h, arclength, ds, gen_seed, dens=None):
    """(seeds, restatement's result) of a parity case on the gas dict of a golden set's initial conditions"""
    pos = np.stack([gas["x"], gas["y"], gas["z"]], axis=1)
    hh = gas["h"] if h is None else h
    seeds = parity_seeds(pos, hh, gen_seed)
    A = np.stack([gas["vx"], gas["vy"], gas["vz"]])
    return seeds, trace(seeds, pos, gas["m"], hh, A, PARITY_STEPS, ds, arclength=arclength, dens=dens)
