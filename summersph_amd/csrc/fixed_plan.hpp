// fixed_plan.hpp -- what a fixed-h step decides on the host: which kernels run, and what a neighbour-list report means.
// Plain C++ (no HIP, no sph_ctx): the callers (tiled.hip, api.hip) read the context, call these and act on the answer, and
// tests/test_fixed_plan_cpu.py compiles this header alone to check every rule at its edges.  DESIGN.md, "The fixed-h step's
// plan and the A/B switches".  The measurements behind the thresholds stand next to the callers.
#pragma once
#include <algorithm>
#include <cstdint>

namespace sph {

constexpr int WT_BS = 1024;          // density_wt: threads (= targets) per workgroup, one workgroup per CU
constexpr int FQ_T = 256;            // forces_q: targets per group (four lanes each) ...
constexpr int FQ_HALF = 128;         // ... and per half group (eight lanes each)
static_assert(2 * FQ_HALF == FQ_T && WT_BS == 4 * FQ_T, "plan_reduce_kernel: a density group is four force groups, eight half groups");
// the three intervals of a group must stay below this many records together: what a 16-bit list entry can address
// (tile_common.hpp)
constexpr int LIST16_MAX_NEED = 65536;

// the eight words of ListReport::v (sph_internal.hpp), written by plan_reduce_kernel (tiled.hip)
enum ListReportWord {
    REP_LONGEST = 0,       // longest list
    REP_MISFIT_D,          // groups of density_wt whose tile does not fit beside the kernel table
    REP_MISFIT_F,          // groups of forces_q, the same
    REP_NEED,              // largest tile need of a force group (records)
    REP_MISFIT_D_FREE,     // density groups that do not fit the table-free (bigger) tile
    REP_MISFIT_F_FREE,     // force groups, the same
    REP_MISFIT_H,          // half groups of forces_q that do not fit beside the table
    REP_MISFIT_H_FREE,     // half groups, table-free
    REP_WORDS
};

// ---- the tile verdict of a list build ----------------------------------------------------------------------------------------
struct TileChoice {
    bool ok = false, ok_f = false;        // the workgroups' intervals fit the tile (density / forces geometry)
    bool half_f = false;                  // forces_q on half groups: half the tile need of a group of 256
    bool big = false, big_f = false;      // only the table-free tile (the kernel table's knots recomputed, 40 KB more for the tile)
    int32_t fit_pct = -1, fit_pct_f = -1; // percentage of workgroups that fit (-1: kernels off)
};

// The whole-tile kernels pay a prologue and run their fall-back loop at one workgroup per CU: they are used when (nearly)
// every workgroup's intervals fit the tile -- nine in ten; thin discs and sheets, thick domains keep pairs.hip -- with the
// kernel table beside the tile; where that fails but the table-free tile holds the intervals (dense neighbourhoods) the
// table-free variant runs (force_table_free: always).  Forces: groups of 256 with the table (1.0), table-free (x1.1 on the
// bench disc), half groups -- every record staged more often -- with the table, table-free; the first whose tiles fit
// (force_half: half groups whatever fits).
inline TileChoice choose_tiles(const int32_t rep[REP_WORDS], int64_t n, bool force_table_free, int force_half) {
    const unsigned d_blocks = (unsigned)((n + WT_BS - 1) / WT_BS), f_blocks = (unsigned)((n + FQ_T - 1) / FQ_T);
    auto fits = [](int32_t misfits, int64_t groups) { return (int64_t)misfits * 10 <= groups; };
    auto pct = [](int32_t misfits, int64_t groups) { return (int32_t)(100 - (100 * (int64_t)misfits) / std::max<int64_t>(groups, 1)); };
    const bool ok_d = fits(rep[REP_MISFIT_D], d_blocks), ok_db = fits(rep[REP_MISFIT_D_FREE], d_blocks);
    const bool ok_f = fits(rep[REP_MISFIT_F], f_blocks), ok_fb = fits(rep[REP_MISFIT_F_FREE], f_blocks);
    const bool ok_h = fits(rep[REP_MISFIT_H], 2 * (int64_t)f_blocks), ok_hb = fits(rep[REP_MISFIT_H_FREE], 2 * (int64_t)f_blocks);
    TileChoice t;
    t.big = force_table_free || (!ok_d && ok_db);
    t.ok = t.big ? ok_db : ok_d;
    t.fit_pct = pct(rep[t.big ? REP_MISFIT_D_FREE : REP_MISFIT_D], d_blocks);
    t.half_f = force_half != 0 || (!ok_f && !ok_fb && (ok_h || ok_hb));
    if (t.half_f) {
        t.big_f = force_table_free || !ok_h;
        t.ok_f = t.big_f ? ok_hb : ok_h;
        t.fit_pct_f = pct(rep[t.big_f ? REP_MISFIT_H_FREE : REP_MISFIT_H], 2 * (int64_t)f_blocks);
    } else {
        t.big_f = force_table_free || (!ok_f && ok_fb);
        t.ok_f = t.big_f ? ok_fb : ok_f;
        t.fit_pct_f = pct(rep[t.big_f ? REP_MISFIT_F_FREE : REP_MISFIT_F], f_blocks);
    }
    return t;
}

// Does the tile kernel run at this size?  The kernels are persistent, one workgroup per CU: below min_groups_d / _f
// hundredths of a group per CU the gather kernel of pairs.hip runs (api.hip has the measurements).
inline bool use_tile_kernel(const TileChoice &t, bool whole_tile, bool forces, int64_t n, int num_cus, int min_groups_d, int min_groups_f) {
    if (!whole_tile || !(forces ? t.ok_f : t.ok)) return false;
    const int per = forces ? FQ_T : WT_BS;
    const int64_t groups = (n + per - 1) / per;
    return 100 * groups >= (int64_t)(forces ? min_groups_f : min_groups_d) * num_cus;
}

// ---- what a list report means ------------------------------------------------------------------------------------------------
// The steady state reads the report of the PREVIOUS build instead of waiting for this one's.  The list keeps a third of
// headroom, so a list that overflows within one step is an error reported one build late, not a silent truncation; the same
// for the 16-bit entries: the context leaves the tiled path when a group's intervals reach HALF of what an entry can address.
enum class ListReportAge {
    PREVIOUS_BUILD,        // nlist_build_tiled, steady state: the list and the entries it describes are already in use
    OWN_BUILD,             // nlist_build_tiled after waiting for its own report: nothing has read the list yet
    DRAIN                  // drain_reports: the last build's report, after the results were computed from its list
};
enum class ListKind { FITS, REGROW, LEAVE_TILED, LIST_OVERFLOWED, OUTGREW_16BIT };
struct ListVerdict {
    ListKind kind;
    int32_t new_cap;       // REGROW: the list's new capacity, a multiple of 8 (rows of eight 16-bit entries); 0 otherwise
};
// In this order: a list longer than the capacity was truncated, entries of a need >= LIST16_MAX_NEED were (both are errors
// where the list was already read, and only there); a need of half that leaves the tiled path; a list longer than three
// quarters of the capacity regrows to one and a half times its length.  A drain changes nothing, it only reports the two
// errors -- the second for a tiled context alone (an untiled list has 32-bit entries).
inline ListVerdict judge_list(const int32_t rep[REP_WORDS], int32_t nl_cap, ListReportAge age, bool tiled = true) {
    const int32_t r = rep[REP_LONGEST], need = rep[REP_NEED];
    if (age != ListReportAge::OWN_BUILD) {
        if (r > nl_cap) return {ListKind::LIST_OVERFLOWED, 0};
        if (tiled && need >= LIST16_MAX_NEED) return {ListKind::OUTGREW_16BIT, 0};
        if (age == ListReportAge::DRAIN) return {ListKind::FITS, 0};
    }
    if (2 * (int64_t)need >= LIST16_MAX_NEED) return {ListKind::LEAVE_TILED, 0};
    if (4 * (int64_t)r > 3 * (int64_t)nl_cap) return {ListKind::REGROW, ((r + r / 2 + 8) + 7) & ~7};
    return {ListKind::FITS, 0};
}

// ---- riders: the sinks' sums in the tails of density_wt / forces_q (rider_common.hpp) ------------------------------------------
// what of the context the step's riders depend on
struct StepConditions {
    bool variable, gravity, accrete_cull;     // variable h, self-gravity, SPH_FLAG_ACCRETE_CULL
    int64_t n, n_slots, dead_below, n_owned;  // slots != n or dead_below != 0: a ghost swap is pending; n_owned != n: ghosts
    int32_t nranks;
};
// only the plain fixed-h step asks for sink_accel_partial / _final to ride (no_sink_ride: the A/B switch SPH_NO_SINK_RIDE)
inline bool riders_allowed(const StepConditions &s, bool no_sink_ride) {
    return !(no_sink_ride || s.variable || s.gravity || s.accrete_cull || s.n_slots != s.n || s.dead_below != 0 || s.n_owned != s.n ||
             s.nranks != 1);
}
// does sink_accel_final ride on forces_q?  rode: the blocks of sink_accel_partial that rode on the density pass before;
// tile_f: forces_q runs (use_tile_kernel); the half-group variants of forces_q take no rider
inline bool ride_final(int32_t rode, bool tile_f, const TileChoice &t) { return rode > 0 && tile_f && !t.half_f; }

}  // namespace sph
