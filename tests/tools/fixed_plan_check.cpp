// fixed_plan_check.cpp -- the fixed-h step's host decisions (csrc/fixed_plan.hpp) and the parsers of the A/B switches
// (csrc/switches.hpp) at the edges where they can go wrong, against expected values written out here
// (tests/test_fixed_plan_cpu.py builds this with -fsanitize=address,undefined and runs it; no HIP, no GPU).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../summersph_amd/csrc/fixed_plan.hpp"
#include "../../summersph_amd/csrc/switches.hpp"

using namespace sph;

static int failures = 0, checks = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        checks++;                                                                          \
        if (!(cond)) { failures++; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

struct Rep {
    int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Rep &set(ListReportWord w, int32_t x) { v[w] = x; return *this; }
};
static Rep list_rep(int32_t longest, int32_t need) { return Rep().set(REP_LONGEST, longest).set(REP_NEED, need); }

static bool is(const ListVerdict &v, ListKind k, int32_t cap = 0) { return v.kind == k && v.new_cap == cap; }

static void check_judge_list() {
    const auto PREV = ListReportAge::PREVIOUS_BUILD, OWN = ListReportAge::OWN_BUILD, DRAIN = ListReportAge::DRAIN;
    // the list's length against a capacity of 96: three quarters are 72
    for (auto age : {PREV, OWN}) {
        CHECK(is(judge_list(list_rep(72, 0).v, 96, age), ListKind::FITS));             // 4 * 72 == 3 * 96
        CHECK(is(judge_list(list_rep(73, 0).v, 96, age), ListKind::REGROW, 120));      // 73 + 36 + 8 = 117 -> 120
        CHECK(is(judge_list(list_rep(96, 0).v, 96, age), ListKind::REGROW, 152));      // 96 + 48 + 8 = 152
        CHECK(is(judge_list(list_rep(0, 0).v, 96, age), ListKind::FITS));
    }
    CHECK(is(judge_list(list_rep(97, 0).v, 96, PREV), ListKind::LIST_OVERFLOWED));
    CHECK(is(judge_list(list_rep(97, 0).v, 96, OWN), ListKind::REGROW, 160));          // 97 + 48 + 8 = 153 -> 160
    CHECK(is(judge_list(list_rep(96, 0).v, 96, DRAIN), ListKind::FITS));               // a drain regrows nothing
    CHECK(is(judge_list(list_rep(97, 0).v, 96, DRAIN), ListKind::LIST_OVERFLOWED));
    CHECK(is(judge_list(list_rep(97, 0).v, 96, DRAIN, false), ListKind::LIST_OVERFLOWED));
    // the tile need against the 16-bit entries
    for (auto age : {PREV, OWN, DRAIN}) CHECK(is(judge_list(list_rep(10, 32767).v, 96, age), ListKind::FITS));
    for (auto age : {PREV, OWN}) CHECK(is(judge_list(list_rep(10, 32768).v, 96, age), ListKind::LEAVE_TILED));
    CHECK(is(judge_list(list_rep(10, 32768).v, 96, DRAIN), ListKind::FITS));
    CHECK(is(judge_list(list_rep(10, 65535).v, 96, PREV), ListKind::LEAVE_TILED));
    CHECK(is(judge_list(list_rep(10, 65535).v, 96, DRAIN), ListKind::FITS));
    CHECK(is(judge_list(list_rep(10, 65536).v, 96, PREV), ListKind::OUTGREW_16BIT));
    CHECK(is(judge_list(list_rep(10, 65536).v, 96, OWN), ListKind::LEAVE_TILED));
    CHECK(is(judge_list(list_rep(10, 65536).v, 96, DRAIN), ListKind::OUTGREW_16BIT));
    CHECK(is(judge_list(list_rep(10, 65536).v, 96, DRAIN, true), ListKind::OUTGREW_16BIT));
    CHECK(is(judge_list(list_rep(10, 65536).v, 96, DRAIN, false), ListKind::FITS));    // an untiled list has 32-bit entries
    CHECK(is(judge_list(list_rep(10, 0x7fffffff).v, 96, OWN), ListKind::LEAVE_TILED)); // no 32-bit overflow in 2 * need
    // precedence: overflow, outgrown, leave, regrow
    CHECK(is(judge_list(list_rep(97, 65536).v, 96, PREV), ListKind::LIST_OVERFLOWED));
    CHECK(is(judge_list(list_rep(97, 65536).v, 96, DRAIN), ListKind::LIST_OVERFLOWED));
    CHECK(is(judge_list(list_rep(97, 32768).v, 96, PREV), ListKind::LIST_OVERFLOWED));
    CHECK(is(judge_list(list_rep(96, 32768).v, 96, PREV), ListKind::LEAVE_TILED));     // leaving beats regrowing
    CHECK(is(judge_list(list_rep(97, 32768).v, 96, OWN), ListKind::LEAVE_TILED));
    CHECK(is(judge_list(list_rep(73, 65535).v, 96, OWN), ListKind::LEAVE_TILED));
    // only the two words named count
    Rep noise = list_rep(72, 32767);
    for (auto w : {REP_MISFIT_D, REP_MISFIT_F, REP_MISFIT_D_FREE, REP_MISFIT_F_FREE, REP_MISFIT_H, REP_MISFIT_H_FREE}) noise.set(w, 1 << 30);
    for (auto age : {PREV, OWN, DRAIN}) CHECK(is(judge_list(noise.v, 96, age), ListKind::FITS));
}

// a particle count, its groups of density_wt (1024), of forces_q (256; twice as many half groups), and the largest misfit
// counts that still pass the nine-in-ten rule for the three (misfits * 10 <= groups)
struct Size { int64_t n; int d, f, lim_d, lim_f, lim_h; };
static const Size SIZES[] = {{1, 1, 1, 0, 0, 0},    {255, 1, 1, 0, 0, 0},  {256, 1, 1, 0, 0, 0},  {257, 1, 2, 0, 0, 0},
                             {1023, 1, 4, 0, 0, 0}, {1024, 1, 4, 0, 0, 0}, {1025, 2, 5, 0, 0, 1}, {10240, 10, 40, 1, 4, 8}};

static void check_choose_tiles() {
    for (const Size &s : SIZES) {
        const int64_t n = s.n;
        {   // nothing misfits
            const TileChoice t = choose_tiles(Rep().v, n, false, 0);
            CHECK(t.ok && t.ok_f && !t.big && !t.big_f && !t.half_f && t.fit_pct == 100 && t.fit_pct_f == 100);
        }
        // ---- density: the table variant while it fits, table-free only where it misfits and table-free fits
        for (int below = 0; below <= (s.lim_d > 0 ? 1 : 0); below++) {
            const TileChoice t = choose_tiles(Rep().set(REP_MISFIT_D, s.lim_d - below).set(REP_MISFIT_D_FREE, s.lim_d + 1).v, n, false, 0);
            CHECK(t.ok && !t.big);
        }
        {
            TileChoice t = choose_tiles(Rep().set(REP_MISFIT_D, s.lim_d + 1).set(REP_MISFIT_D_FREE, s.lim_d).v, n, false, 0);
            CHECK(t.ok && t.big);
            t = choose_tiles(Rep().set(REP_MISFIT_D, s.lim_d + 1).set(REP_MISFIT_D_FREE, s.lim_d + 1).v, n, false, 0);
            CHECK(!t.ok && !t.big);
            CHECK(t.ok_f && !t.big_f && !t.half_f && t.fit_pct_f == 100);              // the forces side is its own
            // forced table-free: big, and ok follows the table-free count
            t = choose_tiles(Rep().set(REP_MISFIT_D_FREE, s.lim_d).v, n, true, 0);
            CHECK(t.ok && t.big && t.ok_f && t.big_f && !t.half_f);
            t = choose_tiles(Rep().set(REP_MISFIT_D_FREE, s.lim_d + 1).v, n, true, 0);
            CHECK(!t.ok && t.big);
            t = choose_tiles(Rep().set(REP_MISFIT_D, s.lim_d + 1).set(REP_MISFIT_D_FREE, s.lim_d).v, n, true, 0);
            CHECK(t.ok && t.big);
        }
        // ---- forces, full groups
        for (int below = 0; below <= (s.lim_f > 0 ? 1 : 0); below++) {
            const TileChoice t = choose_tiles(Rep().set(REP_MISFIT_F, s.lim_f - below).set(REP_MISFIT_F_FREE, s.lim_f + 1).set(REP_MISFIT_H, 0).v, n, false, 0);
            CHECK(t.ok_f && !t.big_f && !t.half_f);
        }
        {
            TileChoice t = choose_tiles(Rep().set(REP_MISFIT_F, s.lim_f + 1).set(REP_MISFIT_F_FREE, s.lim_f).v, n, false, 0);
            CHECK(t.ok_f && t.big_f && !t.half_f);                                     // a full-group variant fits: no half groups
            CHECK(t.ok && !t.big && t.fit_pct == 100);
            t = choose_tiles(Rep().set(REP_MISFIT_F_FREE, s.lim_f + 1).v, n, true, 0);
            CHECK(!t.ok_f && t.big_f && !t.half_f);                                    // forced table-free: ok_f follows its count
        }
        // ---- forces, half groups: only when both full-group variants misfit and a half-group variant fits
        const Rep full_misfit = Rep().set(REP_MISFIT_F, s.lim_f + 1).set(REP_MISFIT_F_FREE, s.lim_f + 1);
        for (int below = 0; below <= (s.lim_h > 0 ? 1 : 0); below++) {
            const TileChoice t = choose_tiles(Rep(full_misfit).set(REP_MISFIT_H, s.lim_h - below).set(REP_MISFIT_H_FREE, s.lim_h + 1).v, n, false, 0);
            CHECK(t.half_f && t.ok_f && !t.big_f);
        }
        {
            TileChoice t = choose_tiles(Rep(full_misfit).set(REP_MISFIT_H, s.lim_h + 1).set(REP_MISFIT_H_FREE, s.lim_h).v, n, false, 0);
            CHECK(t.half_f && t.ok_f && t.big_f);
            t = choose_tiles(Rep(full_misfit).set(REP_MISFIT_H, s.lim_h + 1).set(REP_MISFIT_H_FREE, s.lim_h + 1).v, n, false, 0);
            CHECK(!t.half_f && !t.ok_f && !t.big_f);                                   // nothing fits: the gather kernel
            t = choose_tiles(Rep(full_misfit).set(REP_MISFIT_H, s.lim_h).v, n, true, 0);
            CHECK(t.half_f && t.ok_f && t.big_f);                                      // forced table-free inside the half-group branch
            t = choose_tiles(Rep(full_misfit).set(REP_MISFIT_H, s.lim_h).set(REP_MISFIT_H_FREE, s.lim_h + 1).v, n, true, 0);
            CHECK(t.half_f && !t.ok_f && t.big_f);
            // forced half groups, whatever the full groups do
            t = choose_tiles(Rep().v, n, false, 1);
            CHECK(t.half_f && t.ok_f && !t.big_f && t.fit_pct_f == 100 && t.ok && !t.big);
            t = choose_tiles(Rep().set(REP_MISFIT_H, s.lim_h + 1).set(REP_MISFIT_H_FREE, s.lim_h).v, n, false, -1);
            CHECK(t.half_f && t.ok_f && t.big_f);
            t = choose_tiles(Rep().set(REP_MISFIT_H, s.lim_h + 1).set(REP_MISFIT_H_FREE, s.lim_h + 1).v, n, false, 1);
            CHECK(t.half_f && !t.ok_f && t.big_f);
        }
    }
    // the percentages, floor arithmetic; each from the count of the variant chosen
    TileChoice t = choose_tiles(Rep().set(REP_MISFIT_D, 1).set(REP_MISFIT_F, 4).v, 10240, false, 0);
    CHECK(t.fit_pct == 90 && t.fit_pct_f == 90);
    t = choose_tiles(Rep().set(REP_MISFIT_D, 2).set(REP_MISFIT_D_FREE, 2).set(REP_MISFIT_F, 5).set(REP_MISFIT_F_FREE, 5).set(REP_MISFIT_H, 9).set(REP_MISFIT_H_FREE, 9).v, 10240, false, 0);
    CHECK(!t.ok && t.fit_pct == 80 && !t.ok_f && !t.half_f && t.fit_pct_f == 88);      // 100 - floor(500 / 40)
    t = choose_tiles(Rep().set(REP_MISFIT_D, 3).set(REP_MISFIT_D_FREE, 1).set(REP_MISFIT_F, 7).set(REP_MISFIT_F_FREE, 3).v, 10240, false, 0);
    CHECK(t.big && t.fit_pct == 90 && t.big_f && t.fit_pct_f == 93);                   // 100 - floor(300 / 40)
    t = choose_tiles(Rep().set(REP_MISFIT_F, 5).set(REP_MISFIT_F_FREE, 5).set(REP_MISFIT_H, 7).set(REP_MISFIT_H_FREE, 1).v, 10240, false, 0);
    CHECK(t.half_f && !t.big_f && t.fit_pct_f == 92);                                  // 100 - floor(700 / 80)
    t = choose_tiles(Rep().set(REP_MISFIT_F, 5).set(REP_MISFIT_F_FREE, 5).set(REP_MISFIT_H, 9).set(REP_MISFIT_H_FREE, 1).v, 10240, false, 0);
    CHECK(t.half_f && t.big_f && t.fit_pct_f == 99);                                   // 100 - floor(100 / 80)
    t = choose_tiles(Rep().set(REP_MISFIT_D, 1).set(REP_MISFIT_D_FREE, 1).set(REP_MISFIT_F, 1).set(REP_MISFIT_F_FREE, 1).set(REP_MISFIT_H, 2).set(REP_MISFIT_H_FREE, 2).v, 1, false, 0);
    CHECK(!t.ok && t.fit_pct == 0 && !t.ok_f && t.fit_pct_f == 0);
    t = choose_tiles(Rep().set(REP_MISFIT_D, 1).set(REP_MISFIT_D_FREE, 1).set(REP_MISFIT_F, 2).v, 1025, false, 0);
    CHECK(t.fit_pct == 50 && t.fit_pct_f == 100 && t.big_f);                           // 2 density groups, 5 force groups: the table-free count is 0
    t = choose_tiles(Rep().set(REP_MISFIT_D, 0x7fffffff).set(REP_MISFIT_D_FREE, 0x7fffffff).v, 10240, false, 0);
    CHECK(!t.ok && !t.big && t.ok_f);                                                  // 64-bit products: no overflow in misfits * 10
}

static void check_use_tile_kernel() {
    TileChoice t;
    t.ok = t.ok_f = true;
    // density_wt: groups of 1024, from one group per CU (threshold 100 hundredths)
    CHECK(!use_tile_kernel(t, true, false, 261120, 256, 100, 0));      // 255 groups
    CHECK(use_tile_kernel(t, true, false, 261121, 256, 100, 0));       // 256 groups
    CHECK(use_tile_kernel(t, true, false, 262144, 256, 100, 0));       // still 256
    CHECK(!use_tile_kernel(t, true, false, 195584, 256, 75, 0));       // 191 groups against 0.75 * 256 = 192
    CHECK(use_tile_kernel(t, true, false, 195585, 256, 75, 0));        // 192 groups
    CHECK(!use_tile_kernel(t, true, false, 7168, 8, 100, 0));          // 8 CUs: 7 groups
    CHECK(use_tile_kernel(t, true, false, 7169, 8, 100, 0));           // 8 groups
    // forces_q: groups of 256, its own threshold
    CHECK(!use_tile_kernel(t, true, true, 65280, 256, 0, 100));        // 255 groups
    CHECK(use_tile_kernel(t, true, true, 65281, 256, 0, 100));         // 256 groups
    CHECK(!use_tile_kernel(t, true, true, 1792, 8, 0, 100));           // 7 groups
    CHECK(use_tile_kernel(t, true, true, 1793, 8, 0, 100));            // 8 groups
    CHECK(use_tile_kernel(t, true, true, 1, 256, 100, 0));             // the default: forces_q at every size
    CHECK(!use_tile_kernel(t, true, false, 1, 256, 100, 0));
    for (int64_t n : {(int64_t)1, (int64_t)255, (int64_t)1025, (int64_t)3000000000ll})
        for (int forces = 0; forces < 2; forces++) {
            CHECK(use_tile_kernel(t, true, forces, n, 256, 0, 0));     // threshold 0: always, where ok
            CHECK(!use_tile_kernel(t, false, forces, n, 256, 0, 0));   // whole_tile off
            CHECK(!use_tile_kernel(TileChoice{}, true, forces, n, 256, 0, 0));
        }
    TileChoice d_only, f_only;
    d_only.ok = true; f_only.ok_f = true;
    CHECK(use_tile_kernel(d_only, true, false, 5000, 8, 0, 0) && !use_tile_kernel(d_only, true, true, 5000, 8, 0, 0));
    CHECK(!use_tile_kernel(f_only, true, false, 5000, 8, 0, 0) && use_tile_kernel(f_only, true, true, 5000, 8, 0, 0));
}

static void check_riders() {
    const StepConditions plain{false, false, false, 20000, 20000, 0, 20000, 1};
    CHECK(riders_allowed(plain, false));
    CHECK(!riders_allowed(plain, true));                                // SPH_NO_SINK_RIDE
    StepConditions s = plain; s.variable = true; CHECK(!riders_allowed(s, false));
    s = plain; s.gravity = true; CHECK(!riders_allowed(s, false));
    s = plain; s.accrete_cull = true; CHECK(!riders_allowed(s, false));
    s = plain; s.n_slots = 20001; CHECK(!riders_allowed(s, false));
    s = plain; s.n_slots = 19999; CHECK(!riders_allowed(s, false));
    s = plain; s.dead_below = 1; CHECK(!riders_allowed(s, false));
    s = plain; s.n_owned = 19999; CHECK(!riders_allowed(s, false));     // one ghost
    s = plain; s.nranks = 2; CHECK(!riders_allowed(s, false));
    s = plain; s.nranks = 0; CHECK(!riders_allowed(s, false));
    s = plain; s.n = s.n_slots = s.n_owned = 0; CHECK(riders_allowed(s, false));
    // sink_accel_final rides where partials rode, forces_q runs, and on full groups
    TileChoice t;
    CHECK(ride_final(4, true, t));
    CHECK(!ride_final(0, true, t) && !ride_final(-1, true, t) && !ride_final(4, false, t));
    t.half_f = true;
    CHECK(!ride_final(4, true, t));
}

static void check_parsers() {
    const char *V = "SPH_FIXED_PLAN_CHECK_VAR";
    unsetenv(V);
    CHECK(!env_present(V) && env_int_or(V, 100) == 100 && env_int_or(V, 0) == 0 && env_int(V, 1, 0, 13) == 1 && env_flag(V, 1) == 1 &&
          env_flag(V, 0) == 0 && !env_equals(V, "regs"));
    setenv(V, "", 1);
    CHECK(env_present(V) && env_int_or(V, 100) == 0 && env_int(V, 1, 0, 13) == 1 && env_flag(V, 1) == 1 && !env_equals(V, "regs") && env_equals(V, ""));
    setenv(V, "0", 1);
    CHECK(env_present(V) && env_int_or(V, 100) == 0 && env_int(V, 1, 0, 13) == 0 && env_flag(V, 1) == 0);
    setenv(V, "1", 1);
    CHECK(env_present(V) && env_int_or(V, 100) == 1 && env_int(V, 0, 0, 13) == 1 && env_flag(V, 0) == 1);
    setenv(V, "64", 1);
    CHECK(env_int_or(V, 0) == 64 && env_int(V, 1, 0, 13) == 13 && env_flag(V, 0) == 1);       // above the range
    setenv(V, "13", 1);
    CHECK(env_int(V, 1, 0, 13) == 13);
    setenv(V, "7", 1);
    CHECK(env_int(V, 1, 0, 13) == 7);
    setenv(V, "-3", 1);
    CHECK(env_int_or(V, 100) == -3 && env_int(V, 1, 0, 13) == 0 && env_flag(V, 0) == 1);      // below the range; a flag is "not zero"
    setenv(V, "abc", 1);
    CHECK(env_present(V) && env_int_or(V, 100) == 0 && env_int(V, 5, 0, 13) == 0 && env_flag(V, 1) == 0);
    setenv(V, "regs", 1);
    CHECK(env_equals(V, "regs"));
    for (const char *miss : {"reg", "regs ", " regs", "Regs", "regss"}) {
        setenv(V, miss, 1);
        CHECK(!env_equals(V, "regs"));
    }
    unsetenv(V);
    // the switch structs read the names they say, with their defaults
    for (const char *name : {"SPH_SAMPLE_LEVEL_WIDTH", "SPH_SAMPLE_POINT_SORT", "SPH_GRAVAT_POINT_SORT", "SPH_SYNC_EVERY_BUILD"}) unsetenv(name);
    CHECK(SampleSwitches().level_width == 1 && SampleSwitches().point_sort && GravityAtSwitches().point_sort && !ContextSwitches().sync_every_build);
    setenv("SPH_SAMPLE_LEVEL_WIDTH", "99", 1); setenv("SPH_SAMPLE_POINT_SORT", "0", 1); setenv("SPH_GRAVAT_POINT_SORT", "0", 1);
    setenv("SPH_SYNC_EVERY_BUILD", "0", 1);
    CHECK(SampleSwitches().level_width == 13 && !SampleSwitches().point_sort && !GravityAtSwitches().point_sort && ContextSwitches().sync_every_build);
    setenv("SPH_SAMPLE_LEVEL_WIDTH", "", 1); setenv("SPH_SAMPLE_POINT_SORT", "", 1); setenv("SPH_GRAVAT_POINT_SORT", "", 1);
    CHECK(SampleSwitches().level_width == 1 && SampleSwitches().point_sort && GravityAtSwitches().point_sort);
    // the once-per-process switches: read at the first call of switches(), and never again
    setenv("SPH_TILE_MIN_GROUPS_D", "0", 1); setenv("SPH_TILE_TABLE", "regs", 1); setenv("SPH_NO_RIDERS", "", 1); unsetenv("SPH_TILE_MIN_GROUPS_F");
    unsetenv("SPH_GRAV_WAVE"); unsetenv("SPH_NO_SINK_RIDE"); setenv("SPH_FRAMES_SPLAT", "plain ", 1);
    const Switches &sw = switches();
    CHECK(sw.tile_min_groups_d == 0 && sw.tile_min_groups_f == 0 && sw.tile_table_regs && sw.no_riders && !sw.no_sink_ride && sw.grav_wave == 1 &&
          !sw.frames_splat_plain);
    setenv("SPH_TILE_MIN_GROUPS_D", "50", 1); unsetenv("SPH_NO_RIDERS"); setenv("SPH_GRAV_WAVE", "0", 1);
    CHECK(&switches() == &sw && switches().tile_min_groups_d == 0 && switches().no_riders && switches().grav_wave == 1);
    CHECK(Switches().tile_min_groups_d == 50 && !Switches().no_riders && Switches().grav_wave == 0);      // (a fresh read sees the change)
}

int main() {
    static_assert(WT_BS == 1024 && FQ_T == 256 && FQ_HALF == 128 && LIST16_MAX_NEED == 65536, "the group sizes and the entries' reach");
    static_assert(REP_LONGEST == 0 && REP_MISFIT_D == 1 && REP_MISFIT_F == 2 && REP_NEED == 3 && REP_MISFIT_D_FREE == 4 &&
                  REP_MISFIT_F_FREE == 5 && REP_MISFIT_H == 6 && REP_MISFIT_H_FREE == 7 && REP_WORDS == 8, "plan_reduce_kernel's report");
    check_judge_list();
    check_choose_tiles();
    check_use_tile_kernel();
    check_riders();
    check_parsers();
    std::printf("checks %d, failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
