"""The two table knots of a pair visit are fetched by two 8-byte LDS reads instead of one paired read (pair_common.hpp
table_knots_at, in every kernel that keeps its table in LDS).  That changes no operation: the whole-tile kernels must still give, bit for bit where the order of
the sums is the same, what the direct-gather kernels, the table-free variants and the paired-read A/B build give -- checked
where the table is read at its ENDS: pairs at r = 0 (knot 0), r = h and r = 2h exactly (knot nq, whose second read is the
padding entry tab[nq + 1]) and idle lanes (the far-away sentinel record: knot nq as well).

Every run is a fresh child process: the switches are read once per process (SPH_TILE_MIN_GROUPS_D=0 lets density_wt serve a
set with fewer groups than CUs; SPH_TILE_TABLE, SUMMERSPH_LIB)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = "rho P c ax ay az du dalpha".split()
BITWISE = ("rho", "P", "c")
READ2_LIB = os.path.join(ROOT, "summersph_amd", "libsummersph_hip_read2.so")      # profiles/knot_reads_ab.sh

H = 2.5
NX = 128


def lattice_sheet():
    """128 x 128 x 1 particles at spacing h/2 = 1.25 (exact in binary) plus a copy of 64 of them at identical positions: pairs
    with r = 0, r = h (offset (2, 0)) and r^2 == (2h)^2 == 25.0 exactly (offset (4, 0)); equal masses"""
    ix, iy = np.meshgrid(np.arange(NX, dtype=np.float64), np.arange(NX, dtype=np.float64), indexing="ij")
    x, y = (1.25 * ix).ravel(), (1.25 * iy).ravel()
    dup = np.arange(64) * 241 + 1000                   # 64 lattice sites spread over the sheet
    x, y = np.concatenate([x, x[dup]]), np.concatenate([y, y[dup]])
    n = x.size
    rng = np.random.default_rng(41)
    gas = {k: np.zeros(n) for k in "x y z vx vy vz u m alpha".split()}
    gas["x"], gas["y"] = x, y
    gas["vx"], gas["vy"], gas["vz"] = (rng.normal(0.0, 0.05, n) for _ in range(3))      # viscosity switches on
    gas["u"][:] = 0.25; gas["m"][:] = 1e-4; gas["alpha"][:] = 0.3
    sinks = {k: np.zeros(0) for k in "x y z vx vy vz m".split()}
    return gas, sinks


def twins(gas):
    """the particles that share their position with another one"""
    key = gas["x"] * (4.0 * NX) + gas["y"]                   # exact: multiples of 1.25 below 2^20
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return cnt[inv] > 1


CHILD = (
    "import sys, numpy as np\n"
    f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
    "from summersph_amd import capi, ic\n"
    "import test_knot_reads_gpu as T\n"
    "kind, flags, steps, variable, path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]\n"
    "gas, sinks = T.lattice_sheet() if kind == 'lattice' else T.stirred_disc(20_000, bool(variable))\n"
    "ctx = capi.Context(device=0, variable=bool(variable), flags=flags | (capi.FLAG_VARIABLE_H if variable else 0))\n"
    "ctx.upload(gas); ctx.set_sinks(sinks)\n"
    "if steps:\n"
    "    ctx.run(steps, 1e-2, 0.0)\n"
    "    out = {f: ctx.field(f) for f in 'x y z vx vy vz u alpha'.split()}\n"
    "else:\n"
    "    ctx.density(); ctx.forces()\n"
    "    out = {f: ctx.field(f) for f in T.FIELDS}\n"
    "st = ctx.stats()\n"
    "np.savez(path, fit_d=st.tile_fit_pct, fit_f=st.tile_fit_pct_forces, **out)\n"
)


def stirred_disc(n, variable, seed=202):
    """as stirred_disc of test_whole_tile_gpu.py; variable: the variable-h disc (it carries h)"""
    from summersph_amd import ic
    rows = ic.keplerian_disc_var(n, seed=seed) if variable else ic.keplerian_disc(n, seed=seed, nngb=85.0)
    gas, sinks = ic.split_rows(rows)
    rng = np.random.default_rng(3)
    gas["vx"] = gas["vx"] + rng.normal(0.0, 0.05, n)
    gas["alpha"] = np.full(n, 0.3)
    return gas, sinks


def run_child(tmp, tag, kind, flags=0, steps=0, variable=False, env=None):
    path = os.path.join(str(tmp), tag + ".npz")
    subprocess.run([sys.executable, "-c", CHILD, kind, str(flags), str(steps), str(int(variable)), path], check=True,
                   env={**os.environ, "SPH_TILE_MIN_GROUPS_D": "0", **(env or {})}, timeout=300)
    return dict(np.load(path))


def same(a, b, f, tol=1e-14):
    if f in BITWISE:
        return np.array_equal(a, b)
    return float(np.max(np.abs(a - b))) <= tol * float(np.max(np.abs(b)))


NO_WHOLE_TILE = 128      # capi.FLAG_NO_WHOLE_TILE (the package is not imported before the children have run)


@pytest.fixture(scope="module")
def lattice(tmp_path_factory):
    """the lattice sheet through the whole-tile kernels, the direct-gather kernels, the table-free tile kernels and (if it was
    built) the paired-read library; the CPU oracle on the same particles -- each computed once"""
    from oracle import orc
    tmp = tmp_path_factory.mktemp("knots")
    out = {"tile": run_child(tmp, "tile", "lattice"),
           "gather": run_child(tmp, "gather", "lattice", flags=NO_WHOLE_TILE),
           "regs": run_child(tmp, "regs", "lattice", env={"SPH_TILE_TABLE": "regs"})}
    if os.path.exists(READ2_LIB):
        out["read2"] = run_child(tmp, "read2", "lattice", env={"SUMMERSPH_LIB": READ2_LIB})
    gas, sinks = lattice_sheet()
    o = orc.Oracle(gas, sinks, h=H, nthreads=orc.max_threads())
    o.evaluate()
    out["oracle"] = {f: getattr(o, f) for f in FIELDS}
    out["gas"] = gas
    return out


def test_lattice_has_the_pairs_at_the_tables_ends(lattice):
    gas = lattice["gas"]
    x, y = gas["x"], gas["y"]
    i = 5 * NX + 7
    r2 = (x - x[i]) ** 2 + (y - y[i]) ** 2
    assert np.count_nonzero(r2 == 25.0) == 4 and np.count_nonzero(r2 == 6.25) == 4      # r = 2h and r = h, exactly
    i = 1000                                                   # a duplicated site
    assert np.count_nonzero((x == x[i]) & (y == y[i])) == 2    # r = 0
    # the oracle, like the reference, divides by r = 0: the rates of the 2 x 64 coincident particles are NaN there (the kernels add
    # zeros; test_parity_gpu.py treats its coincident pair the same way) -- everything else it gives is finite
    others = ~twins(gas)
    assert np.count_nonzero(~others) == 128
    for f in FIELDS:
        v = lattice["oracle"][f]
        assert np.all(np.isfinite(v if f in ("rho", "P", "c") else v[others])), f


def test_tile_kernels_equal_the_gather_kernels_at_the_tables_ends(lattice):
    a, b = lattice["tile"], lattice["gather"]
    assert a["fit_d"] >= 90 and a["fit_f"] >= 90 and b["fit_d"] == -1      # density_wt and forces_q really served the sheet
    for f in FIELDS:
        assert same(a[f], b[f], f), f


def test_lattice_agrees_with_the_oracle(lattice):
    from conftest import rel_err
    others = ~twins(lattice["gas"])
    for tag in ("tile", "gather", "regs"):
        for f in FIELDS:
            got, want = lattice[tag][f], lattice["oracle"][f]
            assert np.all(np.isfinite(got)), (tag, f)
            if f in ("rho", "P", "c"):                       # a coincident partner counts with W(0) in the density
                assert rel_err(got, want) <= 1e-13, (tag, f)
            else:                                            # rates: the oracle has NaN for the coincident particles
                assert rel_err(got[others], want[others]) <= 1e-13, (tag, f)


def test_table_free_equals_table(lattice):
    assert lattice["regs"]["fit_d"] >= 90
    for f in FIELDS:
        assert np.array_equal(lattice["regs"][f], lattice["tile"][f]), f


def test_paired_read_build_is_bitwise_the_product(lattice):
    if "read2" not in lattice:
        pytest.skip("the paired-read A/B library is not built (profiles/knot_reads_ab.sh)")
    for f in FIELDS:
        assert np.array_equal(lattice["read2"][f], lattice["tile"][f]), f


@pytest.mark.parametrize("variable", [False, True], ids=["fixed_h", "variable_h"])
def test_stirred_disc_three_steps(tmp_path, variable):
    """20 000 particles, three steps: the tile kernels against the gather path to 1e-12 (variable h has gather kernels only: the
    same kernels with the new read), and the same bits from a second context"""
    a = run_child(tmp_path, "a", "disc", steps=3, variable=variable)
    b = run_child(tmp_path, "b", "disc", flags=NO_WHOLE_TILE, steps=3, variable=variable)
    a2 = run_child(tmp_path, "a2", "disc", steps=3, variable=variable)
    if not variable:
        assert a["fit_d"] >= 90 and a["fit_f"] >= 90
    for f in "x y z vx vy vz u alpha".split():
        assert float(np.max(np.abs(a[f] - b[f]))) <= 1e-12 * float(np.max(np.abs(b[f]))), f
        assert np.array_equal(a[f], a2[f]), f
