// switches.hpp -- the A/B switches of libsummersph_hip.so: environment variables that choose between two forms of the same
// computation, for measurements and for the tests that compare the forms.  This is the only file of the library that reads
// the environment (halo.hip, a separate library, keeps its SPH_HALO_REPLICATED).  Plain C++ (no HIP);
// tests/test_fixed_plan_cpu.py checks the parsers.  DESIGN.md, "The fixed-h step's plan and the A/B switches", has the table
// with the effects at length.
//
// WHEN a switch is read is part of what it means, and is the struct it stands in: once per process (at the first use of
// any of them: a test or script that flips one starts a fresh process), once per context, or at every call.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace sph {

// ---- the parsers --------------------------------------------------------------------------------------------------------------
// presence: set to anything -- "0" and the empty string included -- means on
inline bool env_present(const char *name) { return std::getenv(name) != nullptr; }
// integer with a default: unset gives the default, anything else atoi (so "abc" and "" give 0)
inline int env_int_or(const char *name, int fallback) {
    const char *v = std::getenv(name);
    return v ? std::atoi(v) : fallback;
}
// clamped integer and flag of the per-call switches: the empty string counts as unset
inline int env_int(const char *name, int fallback, int lo, int hi) {
    const char *v = std::getenv(name);
    if (!v || !*v) return fallback;
    return std::min(std::max(std::atoi(v), lo), hi);
}
inline int env_flag(const char *name, int fallback) {
    const char *v = std::getenv(name);
    if (!v || !*v) return fallback;
    return std::atoi(v) != 0;
}
// string equality: exactly `value`, nothing around it
inline bool env_equals(const char *name, const char *value) {
    const char *v = std::getenv(name);
    return v && std::strcmp(v, value) == 0;
}

// ---- read once per process, at the first use of any of them (switches()) -----------------------------------------------------------
// name: what it does [who uses it]
struct Switches {
    // the fixed-h step (api.hip, tiled.hip, pairs.hip, grid.hip)
    int tile_min_groups_d = env_int_or("SPH_TILE_MIN_GROUPS_D", 100);  // density_wt runs from this many hundredths of a group per CU [test_step_riders_gpu, test_whole_tile_gpu, test_knot_reads_gpu, tests/tools/small_n_ab.sh]
    int tile_min_groups_f = env_int_or("SPH_TILE_MIN_GROUPS_F", 0);    // forces_q, the same [tests/tools/small_n_ab.sh]
    bool tile_table_regs = env_equals("SPH_TILE_TABLE", "regs");       // always the table-free tile kernels [test_whole_tile_gpu, test_knot_reads_gpu]
    int forces_half_groups = env_int_or("SPH_FORCES_HALF_GROUPS", 0);  // non-zero: forces_q on half groups whatever fits [test_whole_tile_gpu]
    int gather_block = env_int_or("SPH_GATHER_BLOCK", 0);              // 64: gather kernels in workgroups of 64 threads [tests/tools/small_n_ab.sh]
    bool no_sink_ride = env_present("SPH_NO_SINK_RIDE");               // the step does not ask for the sinks' sums to ride [test_step_riders_gpu]
    bool no_riders = env_present("SPH_NO_RIDERS");                     // the launchers carry no rider workgroup whatever they are asked [test_step_riders_gpu]
    bool no_drift_keys = env_present("SPH_NO_DRIFT_KEYS");             // kick + drift leaves no keys for the next grid build [test_step_fusion_gpu, test_steady_state_adversarial_gpu]
    bool no_box_ride = env_present("SPH_NO_BOX_RIDE");                 // the box of the early partials by a launch of its own [test_step_fusion_gpu]
    bool no_rank_reorder = env_present("SPH_NO_RANK_REORDER");         // the rank within a cell by a launch of its own [test_step_fusion_gpu]
    bool no_lazy_inv = env_present("SPH_NO_LAZY_INV");                 // every reorder stores inv [test_step_fusion_gpu]
    bool sort_radix = env_present("SPH_SORT_RADIX");                   // radix sort of the cell keys instead of the counting sort [test_whole_tile_gpu]
    // variable h (api.hip, varh.hip)
    bool no_h_refresh = env_present("SPH_NO_H_REFRESH");               // a new h rebuilds the grid instead of taking the short path [tests/tools/var_step_probe.py]
    bool no_fused_reflag = env_present("SPH_NO_FUSED_REFLAG");         // re-flag pass and density pass as two kernels [none; DESIGN section 4 has the A/B figures]
    bool no_reflag = env_present("SPH_NO_REFLAG");                     // always build the list, no re-flag margin (as SPH_FLAG_NO_REFLAG) [none; the tests use the flag]
    // self-gravity (gravity.hip)
    int grav_wave = env_int_or("SPH_GRAV_WAVE", 1);                    // 0: the per-lane walk, 2: the wave walk printing its visit counts [test_octree_adversarial_gpu, profiles/README.md]
    // analysis calls (frames.hip, peaks.hip)
    bool frames_splat_plain = env_equals("SPH_FRAMES_SPLAT", "plain"); // every pair of the splat straight to the global limbs [profiles/frames_time.py]
    bool peaks_timing = env_present("SPH_PEAKS_TIMING");               // one line of timings per sph_peaks call on stderr [profiles/peaks_time.py]
};
// thread-safe: the in-process halo transport runs one rank per thread
inline const Switches &switches() {
    static const Switches s;
    return s;
}

// ---- read once per context, by sph_create --------------------------------------------------------------------------------------------
struct ContextSwitches {
    bool sync_every_build = env_present("SPH_SYNC_EVERY_BUILD");       // wait for every read-back of the build path: no one-build-late reports [test_parity_gpu, test_list16_edges_gpu, test_steady_state_adversarial_gpu]
};

// ---- read at every call (profiles/sample_time.py and gravity_at_time.py flip them inside one process) --------------------------------
struct SampleSwitches {      // sample_build, sample_run
    int level_width = env_int("SPH_SAMPLE_LEVEL_WIDTH", 1, 0, 13);     // 2^width quarter octaves of h per level [test_sample_adversarial_gpu, profiles/sample_time.py]
    bool point_sort = env_int("SPH_SAMPLE_POINT_SORT", 1, 0, 1) != 0;  // 0: the points are walked in the caller's order [profiles/sample_time.py]
};
struct GravityAtSwitches {   // gravity_at_run
    bool point_sort = env_flag("SPH_GRAVAT_POINT_SORT", 1) != 0;       // 0: the points are walked in the caller's order [profiles/gravity_at_time.py]
};

}  // namespace sph
