"""GPU tests of the per-step time series (sph_history): the rows of sph_run against the trajectory fixtures, the run with a
history against its twin without one, every row against the numpy restatement (tests/history_ref.py) of a twin context
advanced step by step -- the exact gas sums bitwise --, the independence of the upload order and the grid kind, adversarial
sets through sph_history_record, and the bookkeeping."""
import math

import numpy as np
import pytest

from conftest import load_golden
from gpu_support import capi, golden_gas, make_context, var_params
import history_ref

pytestmark = pytest.mark.gpu

STATE = "x y z vx vy vz u m alpha".split()
SPH_ERR_ARG, SPH_ERR_STATE = 1, 5


def bits(a):
    """the bit patterns: NaN compares equal to NaN, 0.0 differs from -0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def random_gas(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    g = {k: rng.normal(size=n) * (spread if k in "xyz" else 1.0) for k in "x y z vx vy vz".split()}
    g["u"] = rng.uniform(0.1, 1.0, n)
    g["m"] = rng.uniform(0.5, 2.0, n) * 1e-4
    g["alpha"] = np.full(n, 0.1)
    return g


def sinks_of(*rows):
    """a sink dict of (x, y, z, vx, vy, vz, m) rows"""
    a = np.array(rows, dtype=np.float64).reshape(-1, 7)
    return {k: a[:, i].copy() for i, k in enumerate("x y z vx vy vz m".split())}


def recorded_row(capi, gas, sinks, max_sinks=None, density=False, rho=None, **kw):
    """one sph_history_record row of a fresh context, with what the restatement needs: (row, sph_energy's sums, rho)"""
    ctx = make_context(capi, gas, sinks, density=density, **kw)
    if rho is not None:
        ctx.upload_field("rho", rho)
    ctx.history_begin(1, max_sinks=max_sinks)
    ctx.history_record()
    h = ctx.history()
    assert h["rows"].shape == (1, capi.history_width(ctx.history_desc.max_sinks)) and h["dropped"] == 0
    e = ctx.energy()["sums"]
    r = ctx.field("rho") if density else None
    ctx.close()
    return h["rows"][0], e, r


def check_row_against_restatement(row, gas, sinks, e_sums, rho, max_sinks):
    ref = history_ref.row(gas, sinks, rho, max_sinks=max_sinks, sink_part=e_sums[15:])
    assert same_bits(row[4:7], ref[4:7])                              # n, ns, N
    for i in list(range(7, 19)) + [20]:
        assert bits(row[i]) == bits(ref[i]), (i, row[i], ref[i])      # the exact sums
    assert row[19] == 0.0                                             # W_self: not taken
    assert same_bits(row[21:34], e_sums[15:])                         # the sink part: sph_energy's bits
    assert np.array_equal(row[34:40], ref[34:40], equal_nan=True), (row[34:40], ref[34:40])
    assert same_bits(row[40:], ref[40:])


# ---- 1. the fixtures -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variable", [("disc3000_traj", False), ("discv3000_traj", True)])
def test_run_records_the_fixture_trajectory(capi, name, variable):
    g = load_golden(name)
    gas, sinks = golden_gas(name)
    ctx = make_context(capi, gas, sinks, variable=variable, **(var_params(g) if variable else {}))
    ctx.history_begin(8)
    dt, t = ctx.run(5, 1e-2, 0.0)
    h = ctx.history()
    ctx.close()
    assert h["step"].tolist() == [1, 2, 3, 4, 5] and h["dropped"] == 0
    assert h["dt_next"].tolist() == list(g["sph_dt_seq"][1:]) and h["dt_next"][-1] == dt
    assert h["n"].tolist() == [int(v) for v in g["sph_n_seq"][1:]] and h["N"].tolist() == h["n"].tolist()
    assert h["t"][-1] == g["sph_t_end"][0] == t
    clock = np.cumsum(np.concatenate([[0.0], g["sph_dt_seq"][:5]]))[1:]      # t advances by the dt each step ran with
    assert h["t"].tolist() == clock.tolist()
    assert np.all(h["ns"] == 1) and np.all(h["rho_max"] > 0.0) and np.all(h["v_max"] > 0.0)


@pytest.mark.parametrize("name,saved", [("acc2000_traj", (1, 2, 3)), ("bin2000_traj", (1, 3))])
def test_accreting_run_records_counts_and_sinks(capi, name, saved):
    g = load_golden(name)
    gas, sinks = golden_gas(name)
    ctx = make_context(capi, gas, sinks, flags=capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL)
    ctx.history_begin(4)                                              # the per-sink columns of the sinks in place
    ctx.run(3, 1e-2, 0.0)
    h = ctx.history()
    ctx.close()
    ns = len(sinks["m"])
    assert h["n"].tolist() == [int(v) for v in g["full_n_seq"][1:]]
    assert h["dt_next"].tolist() == list(g["full_dt_seq"][1:]) and h["t"][-1] == g["full_t_end"][0]
    assert h["sinks"].shape == (3, ns, 7) and np.all(h["ns"] == ns)
    for k in saved:                                                   # test_gravity_gpu.py's tolerances
        p, s = f"full_s{k}_", h["sinks"][k - 1]
        assert np.max(np.abs(s[:, 6] - g[p + "sm"])) <= 1e-15 and np.max(np.abs(s[:, 0] - g[p + "sx"])) <= 1e-12
        assert np.max(np.abs(s[:, 4] - g[p + "svy"])) <= 1e-12
        assert same_bits(h["Ms"][k - 1], np.sum(s[:, 6]) if ns == 1 else s[0, 6] + s[1, 6])


# ---- 2. no behaviour change ----------------------------------------------------------------------------------------------------------
def test_history_changes_nothing_of_the_run(capi):
    gas, sinks = golden_gas("acc2000_traj")
    out = []
    for on in (True, False):
        ctx = make_context(capi, gas, sinks, flags=capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL)
        if on:
            ctx.history_begin(2)                                      # fills up after two steps: the third is dropped
        dt, t = ctx.run(3, 1e-2, 0.0)
        st = ctx.stats()
        counters = {f: (list(getattr(st, f)) if f == "grid_dim" else getattr(st, f)) for f, _ in st._fields_ if f != "device_bytes"}
        out.append((dt, t, {f: ctx.field(f) for f in STATE + ["rho", "ax", "du"]}, ctx.get_sinks(), counters, st.device_bytes))
        ctx.close()
    a, b = out
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4], (a[4], b[4])
    for f in a[2]:
        assert same_bits(a[2][f], b[2][f]), f
    for k in a[3]:
        assert same_bits(a[3][k], b[3][k]), k
    assert a[5] > b[5]                                                # the log and the partials are counted


def test_history_adds_no_host_synchronisation(capi):
    gas, sinks = golden_gas("disc3000_traj")
    syncs = []
    for on in (True, False):
        ctx = make_context(capi, gas, sinks)
        dt, t = ctx.run(4, 1e-2, 0.0)                                 # into the steady state
        if on:
            ctx.history_begin(8)
        before = ctx.stats().host_syncs
        ctx.run(8, dt, t)
        syncs.append(ctx.stats().host_syncs - before)
        if on:
            assert ctx.history_info()["rows"] == 8
        ctx.close()
    assert syncs[0] == syncs[1], syncs


# ---- 3. every row against the restatement of a twin context ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,steps,variable,full", [("disc3000_traj", 5, False, False), ("discv3000_traj", 3, True, False),
                                                      ("acc2000_traj", 3, False, True), ("bin2000_traj", 3, False, True)])
def test_rows_are_exact_per_step(capi, name, steps, variable, full):
    g = load_golden(name)
    gas, sinks = golden_gas(name)
    kw = dict(variable=variable, **(var_params(g) if variable else {}))
    if full:
        kw["flags"] = capi.FLAG_SELF_GRAVITY | capi.FLAG_ACCRETE_CULL
    ctx = make_context(capi, gas, sinks, **kw)
    ctx.history_begin(steps)
    ctx.run(steps, 1e-2, 0.0)
    h = ctx.history()
    ctx.close()
    twin = make_context(capi, gas, sinks, **kw)
    G = float(twin.params.G)
    ms = len(sinks["m"])
    dt, t = 1e-2, 0.0
    for k in range(steps):
        dt, t = twin.step(dt, t)
        row = h["rows"][k]
        now = {f: twin.field(f) for f in STATE}
        snk = twin.get_sinks()
        rho = twin.field("rho")
        e = twin.energy()["sums"]
        assert row[0] == k + 1 and row[1] == t and row[2] == dt and row[4] == twin.n and row[5] == len(snk["m"])
        ref = history_ref.row(now, snk, rho, max_sinks=ms, G=G, sink_part=e[15:])
        for i in list(range(6, 19)) + [20]:
            assert bits(row[i]) == bits(ref[i]), (k, i, row[i], ref[i])
        assert row[19] == 0.0
        assert same_bits(row[21:34], e[15:]), k
        i0 = int(np.argmax(rho))
        assert row[34] == np.max(rho) and row[35] == i0 and row[36:39].tolist() == [now["x"][i0], now["y"][i0], now["z"][i0]]
        assert row[39] == math.sqrt(np.max((now["vx"] * now["vx"] + now["vy"] * now["vy"]) + now["vz"] * now["vz"]))
        assert same_bits(row[40:], ref[40:])
        # against sph_energy's fp64 tree sums: the grid rounding is <= N 2^(e - 63), the tree adds a few dozen roundings
        terms = history_ref.gas_terms(now, snk, G)
        for s, tm in terms.items():
            err, bound = abs(row[6 + s] - e[s]), 2.0 ** -46 * float(np.sum(np.abs(tm)))
            assert err <= bound, (k + 1, s, row[6 + s], e[s], err, bound)
    twin.close()


# ---- 4. independence of the order and the grid -----------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_order_or_the_grid(capi):
    gas, sinks = golden_gas("disc3000_traj")
    n = len(gas["x"])
    rng = np.random.default_rng(5)
    perms = [np.arange(n), np.arange(n)[::-1].copy(), rng.permutation(n)]
    first = make_context(capi, gas, sinks, density=True)
    rho0 = first.field("rho")                                         # every context gets these densities, particle by particle
    first.close()
    rows = []
    for perm in perms:
        for flags in (0, capi.FLAG_HASHED_GRID, capi.FLAG_NO_WHOLE_TILE):
            mine = {k: np.asarray(v)[perm] for k, v in gas.items()}
            row, _, _ = recorded_row(capi, mine, sinks, density=True, rho=rho0[perm], flags=flags)
            assert perm[int(row[35])] == int(np.argmax(rho0)), flags      # densest maps through the permutation
            rows.append(np.delete(row, 35))
    for r in rows[1:]:
        assert same_bits(r, rows[0])
    assert rows[0][34] == np.max(rho0)


# ---- 5. adversarial sets through sph_history_record ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 255, 256, 257, 513, 1023, 1024, 1025, 2049, 63 * 256, 64 * 256, 64 * 256 + 1,
                               1024 * 256 + 1])
def test_sizes_around_the_wavefront_the_block_and_the_grid(capi, n):
    """The two passes run blocks of 256 and the two final kernels one block of 1024: B - 1, B, B + 1 and 2 B + 1 of both, the
    wavefront's 64, the sets whose 63, 64 and 65 partials end on and beside a full wavefront of the final kernels' lanes,
    and one beyond 1024 blocks of 256, where the passes stride"""
    gas = random_gas(n, 100 + n % 97)
    sinks = sinks_of((0.5, -0.25, 0.125, 0.0, 0.01, 0.0, 1.0))
    row, e, _ = recorded_row(capi, gas, sinks, max_sinks=2)
    check_row_against_restatement(row, gas, sinks, e, None, 2)
    assert row[0] == 0 and row[4] == n and np.all(np.isnan(row[34:39])) and np.all(np.isnan(row[47:]))
    if n == 0:
        assert np.all(row[6:21] == 0.0) and row[39] == 0.0 and row[21] == 1.0


def test_a_smaller_set_after_a_larger_one_reads_no_stale_partial(capi):
    """the partial buffers keep the larger set's 79 blocks of values when the smaller set writes 2: a final kernel that read
    past its block count would show in the second row"""
    sinks = sinks_of((0.5, -0.25, 0.125, 0.0, 0.01, 0.0, 1.0))
    large, small = random_gas(20000, 31), random_gas(500, 32)
    small["m"] = small["m"] * 1e-3                                    # every maximum below the larger set's
    ctx = make_context(capi, large, sinks)
    ctx.history_begin(4)
    ctx.history_record()
    e_large = ctx.energy()["sums"]
    ctx.upload(small)
    ctx.history_record()
    e_small = ctx.energy()["sums"]
    ctx.upload(large)                                                 # and back: the row of the first again, bit for bit
    ctx.history_record()
    rows = ctx.history()["rows"]
    ctx.close()
    check_row_against_restatement(rows[0], large, sinks, e_large, None, 1)
    check_row_against_restatement(rows[1], small, sinks, e_small, None, 1)
    assert same_bits(rows[2], rows[0]) and rows[1][4] == 500 and rows[1][7] < 1e-3 * rows[0][7]


def test_masses_over_forty_decades(capi):
    gas = random_gas(700, 1)
    gas["m"] = 10.0 ** np.random.default_rng(2).uniform(-20.0, 20.0, 700)
    sinks = sinks_of((0.5, -0.25, 0.125, 0.0, 0.01, 0.0, 1.0))
    row, e, _ = recorded_row(capi, gas, sinks)
    check_row_against_restatement(row, gas, sinks, e, None, 1)
    assert row[7] >= np.max(gas["m"])


def test_mirrored_set_sums_to_exact_zero(capi):
    half = random_gas(300, 3)
    gas = {k: np.concatenate([half[k], -half[k]]) if k in "x y z vx vy vz".split() else np.tile(half[k], 2) for k in half}
    order = np.random.default_rng(4).permutation(600)
    gas = {k: v[order] for k, v in gas.items()}
    row, e, _ = recorded_row(capi, gas, None, max_sinks=0)
    check_row_against_restatement(row, gas, None, e, None, 0)
    assert same_bits(row[8:14], np.zeros(6)) and row[17] > 0.0        # sum m r and sum m v: +0.0, bit for bit


def test_gas_at_rest(capi):
    gas = random_gas(300, 6)
    for k in ("vx", "vy", "vz"):
        gas[k] = np.zeros(300)
    row, e, _ = recorded_row(capi, gas, None, max_sinks=0)
    check_row_against_restatement(row, gas, None, e, None, 0)
    assert same_bits(row[11:18], np.zeros(7)) and same_bits(row[39], 0.0)      # p, L, K and v_max: +0.0


def test_one_nan_velocity_marks_only_its_sums(capi):
    gas = random_gas(400, 7)
    sinks = sinks_of((0.5, -0.25, 0.125, 0.0, 0.01, 0.0, 1.0))
    clean, e, _ = recorded_row(capi, gas, sinks)
    bad = {k: v.copy() for k, v in gas.items()}
    bad["vx"][123] = np.nan
    row, e_bad, _ = recorded_row(capi, bad, sinks)
    nan_at = [6 + 5, 6 + 9, 6 + 10, 6 + 11, 39]                       # m vx, L_y and L_z (vx enters both), K, v_max
    assert all(np.isnan(row[i]) for i in nan_at)
    same = [i for i in range(4, 34) if i not in nan_at]
    assert same_bits(row[same], clean[same])                          # M, m r, m vy, m vz, L_x, U, W_gs, the sink part
    check_row_against_restatement(row, bad, sinks, e_bad, None, 1)


def test_tied_densities_go_to_the_lower_index(capi):
    gas, sinks = golden_gas("disc3000_traj")
    rho = np.linspace(1.0, 2.0, len(gas["x"]))
    rho[[2100, 40, 1700]] = 7.0                                       # three at the maximum
    rho[5] = np.nan                                                   # passed over
    row, e, back = recorded_row(capi, gas, sinks, density=True, rho=rho)
    assert same_bits(back, rho)
    assert row[34] == 7.0 and row[35] == 40 and row[36:39].tolist() == [gas["x"][40], gas["y"][40], gas["z"][40]]
    check_row_against_restatement(row, gas, sinks, e, rho, 1)


@pytest.mark.parametrize("max_sinks", [0, 1, 2, 3, 64])
def test_massless_sink_and_sink_columns(capi, max_sinks):
    gas = random_gas(200, 9)
    sinks = sinks_of((0.5, -0.25, 0.125, 0.0, 0.3, 0.0, 0.75), (3.0, 1.0, -2.0, 0.1, 0.0, -0.2, 0.0))      # the second: mass 0
    row, e, _ = recorded_row(capi, gas, sinks, max_sinks=max_sinks)
    assert row.size == 40 + 7 * max_sinks and row[5] == 2 and row[21] == 2.0 and row[22] == 0.75 and row[33] == 0.0
    check_row_against_restatement(row, gas, sinks, e, None, max_sinks)
    want = np.full((max_sinks, 7), np.nan)
    for s in range(min(2, max_sinks)):
        want[s] = [sinks[k][s] for k in "x y z vx vy vz m".split()]
    assert same_bits(row[40:], want.reshape(-1))
    one = {k: v[:1] for k, v in sinks.items()}
    alone, _, _ = recorded_row(capi, gas, one, max_sinks=0)
    assert same_bits(alone[20], row[20])                              # W_gs: the massless sink adds nothing


# ---- 6. the bookkeeping ----------------------------------------------------------------------------------------------------------------
def test_capacity_every_begin_end_and_read(capi):
    import torch
    gas, sinks = golden_gas("disc3000_traj")
    ctx = make_context(capi, gas, sinks)
    for call in (ctx.history_record, ctx.history_end, ctx.history_info, ctx.history):
        with pytest.raises(capi.SphError) as err:                     # nothing begun
            call()
        assert err.value.status == SPH_ERR_STATE
    for bad in ((0, 1, 0, 0), (4, 0, 0, 0), (4, 1, -1, 0), (4, 1, 65, 0), (4, 1, 0, 1)):
        d = capi.HistoryDesc(*bad)
        assert ctx.lib.sph_history_begin(ctx._h, d) == SPH_ERR_ARG, bad
    assert ctx.lib.sph_history_begin(ctx._h, None) == SPH_ERR_ARG
    ctx.history_begin(3)
    dt, t = ctx.run(5, 1e-2, 0.0)                                     # capacity 3 over 5 steps
    assert ctx.history_info() == {"rows": 3, "dropped": 2, "steps": 5, "width": 47}
    h = ctx.history()
    assert h["step"].tolist() == [1, 2, 3] and h["dropped"] == 2
    # reads: ranges, the device form, an empty read
    assert same_bits(ctx.history(1, 2)["rows"], h["rows"][1:]) and ctx.history(3)["rows"].shape == (0, 47)
    dev = ctx.history(device=True)
    assert isinstance(dev["rows"], torch.Tensor) and same_bits(dev["rows"].cpu().numpy(), h["rows"])
    assert same_bits(dev["E"], h["E"])
    out = np.zeros(4 * 47)
    for first, count in ((-1, 1), (0, 4), (4, 0), (2, 2), (0, -1)):
        assert ctx.lib.sph_history_read(ctx._h, first, count, out.ctypes.data) == SPH_ERR_ARG, (first, count)
    assert ctx.lib.sph_history_read(ctx._h, 0, 1, None) == SPH_ERR_ARG and np.all(out == 0.0)
    ctx.history_begin(8, every=2)                                     # a second begin: rows, steps and dropped start again
    assert ctx.history_info() == {"rows": 0, "dropped": 0, "steps": 0, "width": 47}
    dt, t = ctx.run(5, dt, t)
    assert ctx.history()["step"].tolist() == [2, 4]
    ctx.history_record()                                              # the current number, not advanced
    assert ctx.history()["step"].tolist() == [2, 4, 5] and ctx.history_info()["steps"] == 5
    last = ctx.history(2)["rows"][0]
    assert last[1] == t and last[2] == dt and last[4] == ctx.n
    small = {k: np.asarray(v)[:500] for k, v in gas.items()}
    ctx.upload(small)                                                 # a new set: the history and its numbers stay
    ctx.history_record()
    ctx.run(1, dt, t)
    h = ctx.history()
    assert h["step"].tolist() == [2, 4, 5, 5, 6] and h["n"].tolist() == [3000, 3000, 3000, 500, 500]
    assert np.isnan(h["rho_max"][3]) and h["rho_max"][4] > 0.0        # no density of the new set yet / after its step
    bytes_on = ctx.stats().device_bytes
    ctx.history_end()
    assert ctx.stats().device_bytes < bytes_on                        # the log and the partials are given back
    ctx.run(2, dt, t)                                                 # steps record nothing again
    with pytest.raises(capi.SphError) as err:
        ctx.history_info()
    assert err.value.status == SPH_ERR_STATE
    ctx.close()


# ---- 7. the Fortran host's history file ------------------------------------------------------------------------------------------------
def test_fortran_host_writes_the_history_file(tmp_path):
    """SPH_HISTORY_FILE switches the file on; the run itself (its dt lines) is what it is without"""
    import os
    import subprocess
    from conftest import ROOT
    from summersph_amd import txtio
    host = os.path.join(ROOT, "summersph_amd", "host", "run_sph_hip")
    if not os.path.exists(host):
        subprocess.run(["make", "-C", os.path.dirname(host)], check=True, stdout=subprocess.DEVNULL)
    g = load_golden("acc2000_traj")
    icf, hist = tmp_path / "ic.txt", tmp_path / "hist.txt"
    txtio.write_ic(str(icf), g["ic"])
    runs = []
    for env in (dict(os.environ, SPH_HISTORY_FILE=str(hist)), {k: v for k, v in os.environ.items() if k != "SPH_HISTORY_FILE"}):
        r = subprocess.run([host, str(icf), "3"], capture_output=True, text=True, cwd=tmp_path, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        runs.append([l for l in r.stdout.splitlines() if l.startswith("dt ")])
    assert runs[0] == runs[1] and len(runs[0]) == 4
    lines = hist.read_text().splitlines()
    assert lines[0].split() == "# sph_history rows 3 dropped 0 steps 3 width 47".split()
    rows = np.array([[float(v) for v in l.split()] for l in lines[1:]])
    assert rows.shape == (3, 47) and rows[:, 0].tolist() == [1.0, 2.0, 3.0]
    assert rows[:, 2].tolist() == list(g["full_dt_seq"][1:]) and rows[:, 4].tolist() == list(g["full_n_seq"][1:])
    assert abs(rows[2, 46] - g["full_s3_sm"][0]) <= 1e-15
    assert sorted(os.listdir(tmp_path)) == ["hist.txt", "ic.txt"]     # no other output file appears


# ---- 8. the command line end to end ------------------------------------------------------------------------------------------------------
def test_cli_runs_a_save_file(tmp_path, capsys):
    import json
    from summersph_amd import history
    g = load_golden("acc2000_traj")
    save = tmp_path / "save.txt"
    with open(save, "w") as f:                                        # a save file: gas records of 9 values, sinks of 8
        f.write("x y z vx vy vz u m alpha\n")
        for r in g["ic"]:
            f.write(" ".join(f"{v:.17e}" for v in (r if r[6] == 0.0 else list(r) + [0.0])) + "\n")
    out = tmp_path / "hist.npz"
    assert history.main([str(save), "--steps", "3", "--self-gravity", "--accrete", "-o", str(out), "--json"]) == 0
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s["rows"] == 4 and s["dropped"] == 0 and len(s["first"]) == len(s["last"]) == 47 and set(s["drift"]) == {"E", "P", "L"}
    assert s["first"][0] == 0 and s["first"][4] == 2000 and s["last"][0] == 3 and s["last"][4] == g["full_n_seq"][3]
    z = np.load(out)
    assert z["rows"].shape == (4, 47) and z["step"].tolist() == [0, 1, 2, 3] and z["sinks"].shape == (4, 1, 7)
    assert z["dt_next"][1:].tolist() == list(g["full_dt_seq"][1:]) and z["n"].tolist() == [int(v) for v in g["full_n_seq"]]
    assert z["t_end"] == g["full_t_end"][0] and z["rho_max"][0] > 0.0 and int(z["desc_capacity"]) == 4 and int(z["desc_every"]) == 1
    assert s["last"] == z["rows"][3].tolist() and np.all(np.isfinite(z["E"]))
