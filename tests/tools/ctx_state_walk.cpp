// ctx_state_walk.cpp -- walks the call-order state machine of csrc/ctx_state.hpp (tests/test_ctx_state_cpu.py builds this
// with -fsanitize=address,undefined and runs it; no HIP, no GPU).
//
// Every state that any sequence of steps can reach from a fresh context is visited (breadth first, to a fixed point or to
// the depth given on the command line), for fixed / variable h with and without self-gravity.  A step is one of the header's
// transitions as an entry point applies it (with that entry point's own guard, where it has one), or an "establish" step: the
// flag writes of do_density, do_forces, do_forces_part, sph_refresh_eos and of the early-keys grant of sph_step, restated
// here from api.hip / grid.hip / tiled.hip / varh.hip.  After every step the invariants below must hold, and field_ready
// must agree with the table in its comment, restated here independently.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../summersph_amd/csrc/ctx_state.hpp"

using sph::CtxState;

struct Cfg { bool variable, gravity; };
struct State {
    CtxState s;
    bool rebuilt_since_part1 = false;      // model only: a grid build ran after the last sph_forces_part(1)
};

static const std::vector<bool CtxState::*> FLAGS = {
    &CtxState::order_valid, &CtxState::grid_valid, &CtxState::rho_valid, &CtxState::eos_valid, &CtxState::rates_valid,
    &CtxState::derived_kept, &CtxState::tree_valid, &CtxState::grav_valid, &CtxState::gx_keys_valid, &CtxState::path_keys_valid,
    &CtxState::leaf_valid, &CtxState::h_refresh_ok, &CtxState::h_new_is_build, &CtxState::list_has_margin,
    &CtxState::wave_class_valid, &CtxState::interior_done, &CtxState::keys_early, &CtxState::inv_valid,
    &CtxState::ring_bbox_valid, &CtxState::ring_nl_valid, &CtxState::nl_overflowed, &CtxState::bbox_exact,
    &CtxState::numbers_set, &CtxState::acc_marked};

static unsigned pack(const State &st) {
    unsigned k = st.rebuilt_since_part1 ? 1u : 0u;
    for (auto f : FLAGS) k = (k << 1) | (st.s.*f ? 1u : 0u);
    return k;
}

// ---- establish steps (the `true` assignments live outside the header, so they are restated) ---------------------------
// do_density; mode 0: the plain outcome; 1: the variable-h short path takes the unfused re-flag / build; 2: the tiled
// build finds the previous build's list overflowed (tiled.hip)
static bool density(State &st, const Cfg &c, int mode) {
    CtxState &s = st.s;
    if (s.nl_overflowed) return false;
    if (!s.grid_valid && c.variable && s.h_refresh_ok && s.order_valid && s.leaf_valid) {
        s.h_growth_taken();
        s.h_records_refreshed();
        if (s.list_has_margin && mode != 1) {          // varh_reflag_density
            s.list_reflagged();
            s.grid_valid = true; s.h_refresh_settled();
            s.rho_valid = s.eos_valid = true;
            return true;
        }
        if (s.list_has_margin) s.list_reflagged();     // varh_nlist_reflag
        else s.list_has_margin = true;                 // varh_nlist_build
        s.grid_valid = true;
    }
    s.h_refresh_settled();
    if (!s.grid_valid) {
        s.h_growth_taken();
        s.keys_early = false; s.ring_bbox_valid = true;      // grid_rebuild
        st.rebuilt_since_part1 = true;
        s.order_valid = true;
        s.grid_rebuilt();
        if (c.variable) {
            s.path_keys_valid = true; s.leaf_valid = true;   // varh_leaf_build (own octree)
            s.list_has_margin = true;                        // varh_nlist_build
        } else {
            if (mode == 2 && s.ring_nl_valid) { s.nl_overflowed = true; return false; }
            s.ring_nl_valid = true;                          // nlist_build_tiled
        }
        s.grid_valid = true;
    }
    s.rho_valid = s.eos_valid = true;
    return true;
}
static bool forces(State &st, const Cfg &c) {
    CtxState &s = st.s;
    if (!s.eos_valid || !s.grid_valid) return false;
    if (c.gravity) s.tree_valid = s.grav_valid = true;       // SPH_FLAG_REUSE_GRAVITY
    s.rates_valid = true;
    return true;
}
static bool forces_part(State &st, const Cfg &c, int part) {
    CtxState &s = st.s;
    if (c.variable || c.gravity || !s.eos_valid || !s.grid_valid) return false;
    if (part == 1) {
        s.wave_class_valid = true; s.interior_done = true;
        st.rebuilt_since_part1 = false;
        s.forces_part_done(1);
        return true;
    }
    if (!s.interior_done) return false;
    s.forces_part_done(2);
    s.rates_valid = true;
    return true;
}

struct Step { const char *name; bool (*run)(State &, const Cfg &); };
#define STEP(name, body) {name, [](State &st, const Cfg &c) -> bool { CtxState &s = st.s; (void)s; (void)c; body; return true; }}
static const std::vector<Step> STEPS = {
    // establish
    {"density", [](State &st, const Cfg &c) { return density(st, c, 0); }},
    {"density (unfused refresh)", [](State &st, const Cfg &c) { return density(st, c, 1); }},
    {"density (overflow found in the build)", [](State &st, const Cfg &c) { return density(st, c, 2); }},
    {"forces", [](State &st, const Cfg &c) { return forces(st, c); }},
    {"forces_part 1", [](State &st, const Cfg &c) { return forces_part(st, c, 1); }},
    {"forces_part 2", [](State &st, const Cfg &c) { return forces_part(st, c, 2); }},
    STEP("refresh_eos", if (!s.grid_valid || !s.rho_valid) return false; s.eos_valid = true),
    STEP("kick + drift with early keys (sph_step)",
         if (!s.rates_valid || c.variable || c.gravity || !s.ring_bbox_valid) return false; s.keys_early = true; s.positions_moved()),
    // transitions, as their entry points apply them
    STEP("upload", s.inv_valid = true; s.particle_set_replaced()),
    STEP("upload (larger)", s.arrays_freed(); s.tree_arrays_freed(); s.inv_valid = true; s.particle_set_replaced()),
    STEP("accrete_and_cull (some leave)", if (!s.order_valid) return false; s.bbox_exact = true; s.early_keys_dropped();
         s.path_keys_valid = true; s.inv_valid = true; s.slots_repacked(s.rates_valid)),
    STEP("accrete_and_cull (a sink leaves, all stay)", if (!s.order_valid) return false; s.bbox_exact = true; s.early_keys_dropped();
         s.path_keys_valid = true; s.sinks_changed()),
    STEP("accrete_mark_dev", s.gx_keys_valid = true; s.acc_marked = true),
    STEP("accrete_apply_dev", if (!s.acc_marked) return false; s.marks_applied(); s.early_keys_dropped(); s.inv_valid = true;
         s.slots_repacked(s.derived_kept)),
    STEP("replace_ghosts_dev", s.ghosts_replaced()),
    STEP("set_owned", s.owned_count_changed()),
    STEP("drift", s.positions_moved()),
    STEP("kick", if (!s.rates_valid) return false; s.velocities_kicked()),
    STEP("kick_drift_devdt", if (!s.rates_valid) return false; s.positions_moved()),
    STEP("update_h", if (!c.variable || !s.grid_valid || !s.rho_valid) return false; s.h_updated(); s.h_refresh_ok = s.h_new_is_build = true),
    STEP("write x", s.field_written(SPH_F_X)),
    STEP("write vx", s.field_written(SPH_F_VX)),
    STEP("write m", s.field_written(SPH_F_M)),
    STEP("write rho", s.field_written(SPH_F_RHO)),
    STEP("write ax", s.field_written(SPH_F_AX)),
    STEP("write h", if (!c.variable) return false; s.field_written(SPH_F_H)),
    STEP("write omega", if (!c.variable) return false; s.field_written(SPH_F_OMEGA)),
    STEP("set_sinks", s.sinks_changed()),
    STEP("set_gravity_sources_dev", if (!c.variable && !c.gravity) return false; s.gravity_sources_changed(c.variable)),
    STEP("set_numbers_dev", s.numbers_set = true; s.numbers_changed(c.variable)),
    STEP("set_boundary_boxes", s.wave_classes_stale()),
    STEP("a download finds the list overflowed", if (!s.ring_nl_valid) return false; s.list_overflow_reported()),
    STEP("sph_energy (own tree)", s.tree_arrays_taken()),
    STEP("sph_energy (external tree)", if (s.tree_valid) return false; s.tree_rebuilt_for_analysis()),
    STEP("sph_force_terms builds the tree", if (!c.gravity || !s.eos_valid || !s.grid_valid) return false; s.tree_valid = true),
};

// the invariants; n > 0 throughout.  Two candidates of the issue are NOT obeyed as first stated and are checked in the form
// that holds ("The context's state", says which transitions break the plain form and why that is harmless):
//   interior_done => eos_valid && grid_valid      broken by every transition that clears grid or eos without a rebuild
//   grav_valid => tree_valid                      broken by upload, both packs and replace_ghosts (they clear tree_valid only)
static const char *violated(const State &st) {
    const CtxState &s = st.s;
    if (s.eos_valid && !s.rho_valid) return "eos_valid => rho_valid";
    if (s.rho_valid && !s.grid_valid) return "rho_valid => grid_valid";
    if (s.grid_valid && !s.order_valid) return "grid_valid => order_valid";
    if (s.h_refresh_ok && s.grid_valid) return "h_refresh_ok => !grid_valid";
    if (s.keys_early && s.order_valid) return "keys_early => !order_valid";
    if (s.interior_done && s.grid_valid && st.rebuilt_since_part1) return "interior_done && grid_valid => no grid build since part 1";
    if (s.grav_valid && s.grid_valid && !s.tree_valid) return "grav_valid && grid_valid => tree_valid";
    if (s.nl_overflowed && (s.grid_valid || s.rho_valid || s.eos_valid || s.rates_valid)) return "nl_overflowed => no evaluation stands";
    return nullptr;
}

// field_ready's table, from its comment
static bool ready_table(const CtxState &s, bool variable, int f) {
    const bool rho = s.rho_valid || s.rates_valid;
    switch (f) {
        case SPH_F_H: return variable;
        case SPH_F_OMEGA: return variable && (s.derived_kept || rho);
        case SPH_F_RHO: return s.derived_kept || rho;
        case SPH_F_P: case SPH_F_C: return s.derived_kept || s.eos_valid || s.rates_valid;
        case SPH_F_AX: case SPH_F_AY: case SPH_F_AZ: case SPH_F_DU: case SPH_F_DALPHA: return s.derived_kept || s.rates_valid;
        default: return true;      // x .. alpha
    }
}

int main(int argc, char **argv) {
    const int max_depth = argc > 1 ? atoi(argv[1]) : 1 << 30;
    size_t total = 0, plain6 = 0, plain7 = 0;
    for (int v = 0; v < 4; v++) {
        const Cfg cfg{(v & 1) != 0, (v & 2) != 0};
        std::set<unsigned> seen;
        std::deque<std::pair<State, int>> todo;
        std::vector<std::pair<unsigned, std::string>> how;      // (state, last step) for the report of a violation
        todo.push_back({State{}, 0});
        seen.insert(pack(State{}));
        while (!todo.empty()) {
            const auto [st, depth] = todo.front();
            todo.pop_front();
            if (depth >= max_depth) continue;
            for (const Step &step : STEPS) {
                State nx = st;
                if (!step.run(nx, cfg)) continue;
                if (const char *bad = violated(nx)) {
                    std::printf("variable %d gravity %d: \"%s\" broken by step \"%s\" at depth %d\n", cfg.variable, cfg.gravity, bad, step.name, depth + 1);
                    return 1;
                }
                for (int f = 0; f < SPH_F_COUNT; f++)
                    if (sph::field_ready(nx.s, cfg.variable, f) != ready_table(nx.s, cfg.variable, f)) {
                        std::printf("field_ready disagrees with its table: field %d, variable %d, after \"%s\"\n", f, cfg.variable, step.name);
                        return 1;
                    }
                plain6 += nx.s.interior_done && !(nx.s.eos_valid && nx.s.grid_valid);
                plain7 += nx.s.grav_valid && !nx.s.tree_valid;
                if (seen.insert(pack(nx)).second) todo.push_back({nx, depth + 1});
            }
        }
        total += seen.size();
    }
    std::printf("states %zu, steps into the plain interior_done rule's violation %zu, the plain grav_valid rule's %zu\n", total, plain6, plain7);
    return 0;
}
