// ctx_state.hpp -- the call-order state of a context: what is valid, what is pending, and what every event does to it.
// Plain C++ (no HIP): sph_ctx inherits CtxState (sph_internal.hpp), and tests/test_ctx_state_cpu.py compiles this header
// alone to walk the transitions.
//
// The rule for the rest of the library: a flag is assigned `true` where the code has just computed what the flag promises,
// and `false` only through one of the transitions below, which are named after what happened.  The flags that are an
// algorithm's own bookkeeping (keys_early, inv_valid, ring_*, bbox_exact) are also written by that algorithm (grid.hip,
// tiled.hip); what an EVENT does to them stands here.  DESIGN.md, "The context's state", lists every call site.
#pragma once
#include "../../include/summersph.h"

namespace sph {

struct CtxState {
    // ---- the evaluation chain: each needs the ones above it (order <- grid <- rho <- eos; rates stand on their own) ----
    bool order_valid = false;        // sorted order, drec, bbox, orig / inv match the current positions              (do_density: grid build)
    bool grid_valid = false;         // ... and the cell table and the neighbour list match positions, masses and h    (do_density)
    bool rho_valid = false;          // rho (omega) matches positions, masses and h                                    (do_density)
    bool eos_valid = false;          // P, c and the force records match rho, u, alpha, v                              (do_density, sph_refresh_eos)
    bool rates_valid = false;        // the rates are those of a whole force evaluation in the current slot order      (do_forces, part 2)
    bool derived_kept = false;       // a pack compacted rho .. dalpha with the state: downloads only                  (accretion pack)
    // ---- octree, gravity, variable h --------------------------------------------------------------------------------
    bool tree_valid = false;         // the gravity tree is that of the current sources and sorted order               (do_forces, sph_force_terms)
    bool grav_valid = false;         // g_cache holds the self-gravity term of the current positions, masses, h, tree  (do_forces)
    bool gx_keys_valid = false;      // g_keys_alt / g_vals_alt hold the sorted path keys of gx_src                    (global_keys_sorted)
    bool path_keys_valid = false;    // mkeys_alt / mvals_alt hold the sorted path keys of the current grid build      (leaf build, accretion)
    bool leaf_valid = false;         // the leaf cells match the current sorted order and (external) octree            (do_density)
    bool h_refresh_ok = false;       // the only thing newer than the grid is h                                        (sph_update_h, an upload of h)
    bool h_new_is_build = false;     // h_new holds the lengths the list in place was built with                       (sph_update_h's swap)
    bool list_has_margin = false;    // the list in place carries the margin shell calc_smoothing reads                (varh_nlist_build)
    // ---- the split force evaluation -----------------------------------------------------------------------------------
    bool wave_class_valid = false;   // wave_class sorts the waves by the boundary boxes in place                      (sph_forces_part 1)
    bool interior_done = false;      // part 1 ran on the force records in place, part 2 may follow                    (sph_forces_part 1)
    // ---- the fixed-h build's bookkeeping ------------------------------------------------------------------------------
    bool keys_early = false;         // keys, histogram, box partials of the current positions are in the key buffers  (grid_prepare_early)
    bool inv_valid = true;           // inv matches orig; false: the last reorder skipped it, ensure_inv rebuilds it    (reorder, iota)
    bool ring_bbox_valid = false;    // the other bounding-box report is the previous build's                           (grid_rebuild)
    bool ring_nl_valid = false;      // the other list report is the previous build's                                   (nlist_build_tiled)
    bool nl_overflowed = false;      // a list overflow was reported: every evaluation is refused until sph_upload     (drain_reports, tiled build)
    bool bbox_exact = true;          // c->bbox is the exact box of the last build, not the previous one widened        (grid_rebuild, do_accrete)
    // ---- numbering and the multi-GPU pack -----------------------------------------------------------------------------
    bool numbers_set = false;        // number[] holds the caller's particle numbers by original id                    (sph_set_numbers_dev)
    bool acc_marked = false;         // keep[] and the mask hold the marks of sph_accrete_mark_dev                      (sph_accrete_mark_dev)

    // ---- events: what happened -> what no longer holds ------------------------------------------------------------------
    void evaluation_stale() { grid_valid = rho_valid = eos_valid = rates_valid = false; }      // (shared by the events below)
    // sph_upload: the slots hold a new set in the caller's order; the one-build-late reports describe the old one
    void particle_set_replaced() {
        evaluation_stale();
        order_valid = tree_valid = derived_kept = ring_bbox_valid = ring_nl_valid = nl_overflowed = false;
        h_new_is_build = h_refresh_ok = numbers_set = keys_early = false;
    }
    // a pack left the survivors in the caller's order (both accretion packs); keep_derived: rho .. dalpha went with them
    void slots_repacked(bool keep_derived) {
        evaluation_stale();
        order_valid = tree_valid = h_refresh_ok = path_keys_valid = numbers_set = false;
        derived_kept = keep_derived;
    }
    // sph_replace_ghosts_dev: new ghosts behind the slots, the old ones dead until the next grid build
    void ghosts_replaced() { evaluation_stale(); order_valid = tree_valid = keys_early = false; }
    // sph_set_owned: the lists and the reductions tell targets from neighbours-only particles by it
    void owned_count_changed() { evaluation_stale(); h_refresh_ok = keys_early = false; }
    void positions_moved() { grid_valid = rho_valid = eos_valid = order_valid = false; }       // drift: all that was sorted or summed over x
    void velocities_kicked() { eos_valid = false; }                                            // kick: P, c, the force records carry v (and u)
    // sph_update_h: reaches, neighbour sets and rho depend on h, nothing else does (do_density's short path); the
    // softening length of the self-gravity term is the particle's own h
    void h_updated() { grid_valid = rho_valid = eos_valid = grav_valid = false; }
    // sph_upload_field*, sph_scatter_field(s)_dev: what an overwritten field invalidates
    void field_written(int field) {
        if (field <= SPH_F_Z || field == SPH_F_M || field == SPH_F_H) {
            h_refresh_ok = field == SPH_F_H && (grid_valid || h_refresh_ok);     // only h is newer than the grid
            grid_valid = rho_valid = false;
        }
        if (field == SPH_F_H) h_new_is_build = false;    // h_new no longer pairs with the new h: the next list is built, not re-flagged
        // a new configuration: the one-build-late reports (list overflow, bounding box, non-finite flag) describe the old one,
        // so the next build waits for its own read-backs instead of trusting them
        if (field <= SPH_F_Z || field == SPH_F_M) ring_nl_valid = ring_bbox_valid = false;
        if (field <= SPH_F_Z) order_valid = keys_early = false;     // the keys of launch_kick_drift_keys too
        if (field <= SPH_F_ALPHA || field == SPH_F_RHO || field == SPH_F_H || field == SPH_F_OMEGA) eos_valid = false;
        derived_kept = grav_valid = false;
    }
    void sinks_changed() { rates_valid = false; }       // set, created, accreted onto or culled: the rates hold the old sinks' pull
    // sph_set_gravity_sources_dev: another shared octree; under variable h the leaf boxes come from it
    void gravity_sources_changed(bool variable) {
        gx_keys_valid = tree_valid = grav_valid = leaf_valid = rates_valid = false;
        if (variable) grid_valid = rho_valid = eos_valid = false;
    }
    // sph_set_numbers_dev: under variable h the numbers break ties in the neighbour lists
    void numbers_changed(bool variable) { if (variable) grid_valid = rho_valid = eos_valid = false; }
    void wave_classes_stale() { wave_class_valid = false; }      // new boundary boxes, or a list build used wave_class as scratch
    // do_density, in its order: the growth of h against h_new was taken (or a build overwrites the list h_new pairs with) ...
    void h_growth_taken() { h_new_is_build = false; }
    // ... the short path refreshed prec, reaches and cell maxima for the new h: nothing summed with the old h stands ...
    void h_records_refreshed() { rates_valid = rho_valid = eos_valid = false; }
    // ... grid and list in place are those of the current h, or are rebuilt now ...
    void h_refresh_settled() { h_refresh_ok = false; }
    // ... grid_rebuild re-sorted the slots: whatever was computed in, or keyed to, the old order
    void grid_rebuilt() {
        derived_kept = grav_valid = path_keys_valid = tree_valid = leaf_valid = false;
        rates_valid = rho_valid = eos_valid = wave_class_valid = interior_done = false;
    }
    // sph_forces_part: after part 1 the rates hold half an evaluation; part 2 completes it
    void forces_part_done(int part) { (part == 1 ? rates_valid : interior_done) = false; }
    void list_reflagged() { list_has_margin = false; }           // varh.hip: the margin rows may be overwritten
    // drain_reports found the last build's list truncated: results are incomplete, evaluations refused until sph_upload
    void list_overflow_reported() { evaluation_stale(); ring_nl_valid = false; nl_overflowed = true; }
    // ---- buffers that changed hands ----------------------------------------------------------------------------------------
    void early_keys_dropped() { keys_early = false; }            // the key buffers became the packs' scratch, or their pass failed
    void marks_applied() { acc_marked = false; }                 // sph_accrete_apply_dev consumed the marks
    void tree_arrays_freed() { gx_keys_valid = false; }          // gravity_free
    // sph_energy / sph_gravity_at built a tree over staged records into the context's tree arrays (gravity.hip) ...
    void tree_arrays_taken() { tree_valid = grav_valid = gx_keys_valid = false; }
    void tree_rebuilt_for_analysis() { grav_valid = false; }     // ... or rebuilt the external sources' tree: the cache was the old tree's
    void arrays_freed() { grav_valid = h_new_is_build = list_has_margin = false; }      // a larger upload: cache, h_new and list are gone
};

// May sph_download_field (and every call that reads a field by name) hand out `field`?
//   x .. alpha           always
//   h                    variable h
//   omega                variable h, and rho's rule
//   rho                  rho_valid or rates_valid
//   P, c                 eos_valid or rates_valid
//   ax .. dalpha         rates_valid
//   derived_kept         every derived field (omega: variable h): a pack compacted them along with the state; the survivors
//                        keep the values of the last evaluation, as the reference's pack leaves them ([F]:481,554)
// The derived arrays are in the current slot order as long as no re-sort happened since they were written (a re-sort clears
// rates_valid).
inline bool field_ready(const CtxState &s, bool variable, int field) {
    if (field <= SPH_F_ALPHA) return true;
    if (field == SPH_F_H) return variable;
    if (s.derived_kept) return field != SPH_F_OMEGA || variable;
    if (field == SPH_F_OMEGA) return variable && (s.rho_valid || s.rates_valid);
    if (field == SPH_F_RHO) return s.rho_valid || s.rates_valid;
    if (field == SPH_F_P || field == SPH_F_C) return s.eos_valid || s.rates_valid;
    return s.rates_valid;
}

}  // namespace sph
