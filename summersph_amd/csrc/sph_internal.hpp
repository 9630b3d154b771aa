// sph_internal.hpp -- context layout and kernel-launcher declarations shared by the
// translation units of libsummersph_hip.so.  gfx950 (MI355X) only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/summersph.h"
#include "ctx_state.hpp"
#include "fixed_plan.hpp"
#include "switches.hpp"

namespace sph {

// W / dW table length in doubles (one entry of zero padding behind the knot at q = 2, see table_lerp in pair_common.hpp) and its LDS footprint
constexpr int TAB_LEN(int nq) { return nq + 2; }
constexpr int TAB_LDS(int nq) { return (nq + 3) & ~1; }

constexpr int WAVE = 64;           // CDNA wavefront
constexpr int FREC = 12;           // doubles per force gather record
constexpr int MAX_SINKS = 64;      // sinks handled by the in-kernel loops
constexpr int MAX_SEL_BOXES = 64;  // boxes per sph_select_boxes call (multi-GPU ghost selection)
struct FieldPtrs9 { double *p[9]; };

// Uniform cell grid over the particles' bounding box.  Axes are permuted so that
// axis s[0] (the one with the fewest cells) varies fastest in the cell key: for a disc
// that is z, which keeps the three key-contiguous cells of a neighbour row short and the
// nine rows of a 27-cell stencil close together in the sorted particle order.
struct GridDesc {
    double org[3];      // bbox minimum, natural x,y,z order
    double inv_edge;    // 1 / cell edge, edge = 2h (1 + 1e-6)
    int32_t dim[3];     // cells along x,y,z
    int32_t s[3];       // axis permutation: s[0] fastest ... s[2] slowest
    int64_t ncells;
};

// Hashed cell table (grid.hip; domains whose box is too sparse for a dense table).  The same GridDesc, but the cell of
// (c2, c1, c0) (permuted axes, c2 slowest) is the 64-bit key c2 << sh2 | c1 << sh1 | c0 with bit widths >= log2 of each
// dimension: key order is the dense row-major order, so the sorted particle order is the dense one.  The occupied cells
// are compacted into ukey[0..m) / ustart[0..m] (ustart[m] = live particles) and hashed (open addressing, linear probing):
// every occupied key k maps to {its index, ustart}, and k + 1 to {index + 1, ustart[index + 1]} (the end of a cell run).
// A lookup answers what the dense table answers -- the lower bound of the key in the sorted order -- and falls back to a
// binary search over ukey for the keys the table does not hold.
constexpr int HASH_AXIS_BITS = 21;            // cells per axis of a hashed grid: at most 2^21 (three axes fit 63 bits)
struct HashEnt { uint64_t key; int32_t idx, start; };      // empty: key = ~0
struct HashView {
    const HashEnt *tab;
    const uint64_t *ukey;      // occupied cell keys, ascending
    const int32_t *ustart;     // first sorted slot of each, [m] = live particles
    const int32_t *m;          // occupied cells (device)
    uint64_t mask;             // table entries - 1 (a power of two)
    int32_t sh1, sh2;          // bit offsets of c1 and c2 in a key
};
// where a 64-bit cell key starts probing (this table and the analysis calls' cell_table.hpp)
__device__ __forceinline__ uint64_t hash_mix(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

// Constants every pair kernel needs; passed by value as a kernel argument (SGPRs).
struct PairConst {
    double h;            // smoothing length
    double inv_h;        // 1 / h
    double inv_dq;       // nq / 2 exactly (dq = 2 / nq, [F]:58): scalar registers for the kernels, not vector ones computed per thread
    double dq;           // 2/nq
    double wnorm;        // kernel_pi * h^3        (W  is DIVIDED by this, [F]:125)
    double inv_dwnorm;   // 1 / (kernel_pi * h^4)  (dW is divided by kernel_pi h^4, [F]:126: once, in the epilogue)
    double visc_eps_h2;  // (0.01f * h) * h        ([F]:373)
    double alpha_floor, alpha_decay, G, gamma, gamma_m1;
    double rcut2;        // (2h)^2 (1 + 1e-12): filter only, the evaluation re-tests q <= 2
    int32_t nq;
    int32_t ns;          // sinks
    int32_t grav;        // 1: ax, ay, az already hold the self-gravity term ([F]:825), continue from there
    // variable-h path
    double kernel_pi, eta, h_tol, h_max_length, h_min_length, h_iter_cap, dt_scale;
};

struct TimingSlot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    int64_t launches = 0;
};

// The pinned host block of the build and step paths (c->pin, zeroed at creation): one member per use, so that no two uses
// can share a word.  Every member is the target of an asynchronous copy, the source of one, or is written by a kernel
// through its address (pinned memory is mapped into the device's address space); a report keeps the element layout of
// the kernel that writes it.  (The analysis calls have their own 32 doubles, rnd_pinned.)
struct DtWords { double dt, t, cand; };                      // the layout of d_dt
struct HStats { double h_max, h_sum, growth, shrink; };      // h_stats_final
struct BoxReport { double box[6]; int32_t nonfinite; };      // bbox_final: min xyz, max xyz, then the flag as an int at double 6
struct ListReport { int32_t v[REP_WORDS]; };                 // plan_reduce_kernel (tiled.hip); the words: ListReportWord, fixed_plan.hpp
struct AccWords { int32_t pos_last, keep_last, ns; };        // the packs: scan and mark of the last particle, sinks after the cull
struct PinnedSlots {
    int32_t wave_max;                              // max_to_host: the longest list of the untiled builds
    DtWords dt_in, dt_out;                         // sph_set_dt's source, sph_get_dt's target
    double dt_cand;                                // sph_dt_candidate
    HStats h_stats;                                // varh_h_stats
    double owned_box[6];                           // owned_bbox
    int64_t sel_counts[MAX_SEL_BOXES];             // sph_select_boxes*
    double bnd_boxes[6 * MAX_SEL_BOXES];           // sph_set_boundary_boxes' staging
    BoxReport bbox[2];                             // the bounding-box reports of the last two builds (ring_bbox)
    ListReport nl[2];                              // the list reports of the last two tiled builds (ring_nl)
    double trim[7];                                // grid_rebuild's trim moments
    AccWords acc;                                  // the accretion packs' read-back
};
struct History;                                              // the per-step time series (history.hip); null: none begun
struct Track;                                                // the tracked particles' log (track.hip); null: none begun
struct Frames;                                               // the movie's log (frames.hip); null: none begun
struct Dust;                                                 // the tracer grains (dust.hip); null: none begun
static_assert(offsetof(BoxReport, nonfinite) == 6 * sizeof(double) && sizeof(BoxReport) % 8 == 0, "bbox_final's layout");
static_assert(sizeof(DtWords) == 3 * sizeof(double) && sizeof(HStats) == 4 * sizeof(double), "copied as arrays of doubles");
#define SPH_PIN_ALIGNED(m, a) static_assert(offsetof(PinnedSlots, m) % (a) == 0, #m " is misaligned for its writer")
SPH_PIN_ALIGNED(wave_max, 4); SPH_PIN_ALIGNED(dt_in, 8); SPH_PIN_ALIGNED(dt_out, 8); SPH_PIN_ALIGNED(dt_cand, 8);
SPH_PIN_ALIGNED(h_stats, 8); SPH_PIN_ALIGNED(owned_box, 8); SPH_PIN_ALIGNED(sel_counts, 8); SPH_PIN_ALIGNED(bnd_boxes, 8);
SPH_PIN_ALIGNED(bbox, 8); SPH_PIN_ALIGNED(nl, 4); SPH_PIN_ALIGNED(trim, 8); SPH_PIN_ALIGNED(acc, 4);
#undef SPH_PIN_ALIGNED

}  // namespace sph

struct sph_ctx : sph::CtxState {
    sph_params p;
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    std::string err;

    int64_t n = 0;        // particles held (owned + ghosts)
    int64_t n_owned = 0;  // original ids [0, n_owned) are this GPU's particles; [n_owned, n) are ghost
                          // copies of other GPUs' particles: neighbours only, never targets
    int64_t cap = 0;      // allocated particle slots
    int64_t reserve = 0;  // minimum capacity requested by sph_reserve (room for ghost swaps)
    // multi-GPU ghost swap (domain.hip): between sph_replace_ghosts_dev and the next grid build the arrays hold
    // n_slots > n entries; slots below dead_below whose original id is >= n_owned are the replaced ghosts
    int64_t n_slots = 0, dead_below = 0;
    int64_t *sel_ids = nullptr; size_t sel_cap = 0;      // box selection results, nbox x n_owned
    int64_t *sel_count = nullptr;
    void *sel_tmp = nullptr; size_t sel_tmp_bytes = 0;
    int32_t sel_boxes = 0; int64_t sel_counts[64] = {};  // last sph_select_boxes
    int64_t sel_stride = 0;                              // ids of box b start at sel_ids + b * sel_stride (n_owned at select time)
    // split force evaluation (sph_forces_part): waves near the other GPUs' boxes wait for the ghost fields
    int32_t *wave_class = nullptr; double *bnd_boxes = nullptr; int32_t n_bnd_boxes = 0;
    bool own_stream = true;                              // false: the caller's stream (sph_set_stream), *_dev calls do not synchronise

    // cell-sorted struct-of-arrays state + derived + rates (SPH_F_* order)
    double *f[SPH_F_COUNT] = {};
    double *f_alt[10] = {};          // ping-pong targets for the state fields on reorder (9, +h when variable)
    int32_t *orig = nullptr, *orig_alt = nullptr;   // sorted slot -> original index
    int32_t *inv = nullptr;                         // original index -> sorted slot
    double *scratch = nullptr;       // n doubles (un-permute on download)

    // gather records (array-of-structs: one particle = one or few cache lines)
    double *drec = nullptr;          // 4 doubles: x y z m
    double *frec = nullptr;          // FREC doubles: x y z m | vx vy vz rho/2 | c/2 alpha/2 P/rho^2 h (pair_common.hpp)

    // variable-h path ("SUMMER_SPH - Variable.f90"): extra gather records and the octree leaf boxes
    bool variable = false;
    bool tiled = true;               // fixed-h: LDS-staged neighbour-list build (tiled.hip) unless SPH_FLAG_NO_LDS_TILES
    bool whole_tile = false;         // fixed-h: density/forces read the neighbours' {x,y,z,m} from one LDS tile per workgroup (tiled.hip)
    sph::TileChoice tile;            // ... and which of them the last list build's report allows (fixed_plan.hpp: choose_tiles)
    bool packed_list = true;         // list layout: 4-packed (tiled build) or wave-strided dwords (nlist_kernel)
    double *prec = nullptr;          // 4 doubles: x y z h        (neighbour-list build)
    double *lrec = nullptr;          // 4 doubles: leaf centre x y z, reach = 2h + leaf_edge/2 (<0: unresolved)
    uint64_t *mkeys = nullptr, *mkeys_alt = nullptr;   // octree path keys (3 bits per level, 21 levels)
    uint32_t *mvals = nullptr, *mvals_alt = nullptr;
    void *msort_tmp = nullptr; size_t msort_tmp_bytes = 0;
    double *cell_hmax = nullptr;     // per cell: largest h of its particles
    double *h_new = nullptr;         // scratch for calc_smoothing
    double *leaf_half = nullptr;     // half edge of every slot's leaf cell (reach = 2 h + this)
    double h_max_glob = 0.0, h_mean = 0.0;
    double root_box[4] = {0, 0, 0, 0};   // octree root centre + edge ([V]:1007-1012)

    // Barnes-Hut gas self-gravity (gravity.hip): binary radix tree over the octree path keys
    bool gravity = false;
    double *g_cache[3] = {nullptr, nullptr, nullptr};   // SPH_FLAG_REUSE_GRAVITY: the self-gravity term of the last walk (sorted order)
                                                        // (grav_valid: still that of the current positions, masses, h, tree and order)
    int32_t *g_left = nullptr, *g_right = nullptr, *g_parent = nullptr, *g_leaf_parent = nullptr, *g_prefix = nullptr;
    int32_t *g_flag = nullptr, *g_slot = nullptr, *g_lvl = nullptr, *g_rope = nullptr, *g_leaf_rope = nullptr;
    double *g_sum = nullptr, *g_leafA = nullptr;     // 4 doubles per node / leaf
    int32_t *g_leaf_of = nullptr;                    // cell-sorted slot -> leaf index
    double *g_wrec = nullptr;                        // 64-byte walk records, 2 cap of them (gravity.hip WalkRec)
    double *g_seg = nullptr;                         // segment tree of leaf moments: 4 doubles x (cap + 64)
    int32_t *g_walkB = nullptr, *g_leafB = nullptr;  // int4 per node, int2 per leaf: packed walk pointers
    double *grav_tab = nullptr;                      // softening table, [F]:81-101
    uint64_t *g_keys = nullptr, *g_keys_alt = nullptr; uint32_t *g_vals = nullptr, *g_vals_alt = nullptr;
    void *g_sort_tmp = nullptr; size_t g_sort_tmp_bytes = 0;
    int64_t g_cap = 0;                               // leaves the tree arrays hold
    // external gravity sources (multi-GPU: the particles of every GPU), caller-owned {x,y,z,m} records + their bounding box
    const double *gx_src = nullptr; int64_t gx_n = 0; double gx_box[6] = {0, 0, 0, 0, 0, 0};
    int32_t *number = nullptr;                       // variable h: the reference's particle numbers by original id (numbers_set)

    // grid
    sph::GridDesc grid{};
    double bbox[6] = {0, 0, 0, 0, 0, 0};   // min xyz, max xyz at the last grid build
    uint32_t *keys = nullptr, *keys_alt = nullptr, *vals = nullptr, *vals_alt = nullptr;
    void *sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
    int32_t *cell_start = nullptr; int64_t cell_cap = 0;
    int32_t *cell_fill = nullptr;    // counting sort of the grid build: per-cell cursor (inside the cell_start allocation, behind the table)
    double *bbox_part = nullptr;     // per-block partial min/max
    // fixed-h steps (sph_run / sph_step): the opening kick + drift also wrote the cell keys, the histogram and the box
    // partials of the new positions for the grid grid_early (grid.hip: grid_prepare_early; keys_early); the next grid build takes them
    sph::GridDesc grid_early{};
    int early_blocks = 0;            // ... and the number of box partials it left behind the classic ones in bbox_part
    sph::PinnedSlots *pin = nullptr; // pinned host memory: staging and read-back slots of the build and step paths
    int32_t *d_flags = nullptr;      // [0] nonfinite, [1] nlist max count
    // Read-backs one build stale (no host wait on the step that is being enqueued): the fixed-h path sizes its grid from
    // the bounding box of the PREVIOUS build plus one cell (a particle outside the box is clamped into a boundary cell and
    // still finds every neighbour: the box is a matter of speed, not of correctness) and checks the list overflow of the
    // previous build.  Two pinned slots (pin->bbox, pin->nl) and two events each, used alternately; ring_*_valid: the other
    // slot holds the previous build's report.  A reported overflow (nl_overflowed) means the state may carry a kick from
    // truncated sums: every evaluation is refused until sph_upload.
    hipEvent_t ev_bbox[2] = {nullptr, nullptr}, ev_nl[2] = {nullptr, nullptr};
    int ring_bbox = 0, ring_nl = 0;
    bool no_stale = false;           // SPH_SYNC_EVERY_BUILD: wait for every read-back (A/B switch, switches.hpp)
    int64_t host_syncs = 0;          // stream synchronisations inside the build path (statistics)
    // hashed cell table (grid.hip): used instead of cell_start when the current grid is hashed
    bool hashed = false;             // the current grid build is hashed
    bool hash_sticky = false;        // a build had to go hashed: later ones skip the dense attempt while the box stays sparse
    sph::HashView hv{};
    int64_t hash_cap = 0;            // particles the hashed buffers hold
    uint64_t *hkeys = nullptr, *hkeys_alt = nullptr;    // 64-bit cell keys and the sorted copy
    uint64_t *ukey = nullptr; int32_t *ustart = nullptr, *uidx = nullptr, *d_m = nullptr;
    sph::HashEnt *htab = nullptr; int64_t htab_len = 0;
    void *hash_tmp = nullptr; size_t hash_tmp_bytes = 0;
    int64_t hash_bytes = 0;          // device bytes of the buffers above
    double index_cells = 0.0;        // cells the current grid indexes (dim product; hashed: most of them empty)
    int64_t hmax_cap = 0;            // entries cell_hmax holds

    // neighbour list: slot k of particle i (wave w = i/64, lane = i%64) lives at
    // nlist[(w*nl_cap + k)*64 + lane]  -> a wave reads 64 consecutive ints per k
    int32_t *nlist = nullptr; int32_t nl_cap = 0; int64_t nl_waves_cap = 0;
    int32_t *ncount = nullptr; int32_t *wave_max = nullptr;
    int32_t *plan_h = nullptr;                      // ... and of every half group (128 targets) of forces_q
    int32_t *plan_d = nullptr, *plan_f = nullptr;   // whole-tile kernels: the tile intervals of every workgroup (density / forces geometry), per list build
    int32_t *deal = nullptr;                        // forces_q: order of the targets within their workgroup (by list length)
    int32_t *ntail = nullptr;        // variable h: entries of the margin shell, stored from the end of the lane's column
    // variable h, re-flag pass (varh.hip): the growth of h the list in place was built to survive, the growth measured
    double vl_grow = 1.0, h_growth = 0.0, h_shrink = 0.0;    // h_shrink: largest h_build / h_now
    int64_t nlist_reflags = 0;
    int32_t nl_max = 0; double nl_mean = 0.0;

    // kernel tables on the device
    double *w_tab = nullptr, *dw_tab = nullptr;
    double *w_pair = nullptr, *dw_pair = nullptr;    // pair-packed copies: entry k = {t[k], t[k+1]} (16-B aligned)

    // sinks on the device: 10 arrays of MAX_SINKS doubles: x y z vx vy vz m ax ay az
    int32_t ns = 0;
    double *sink = nullptr;
    double *sink_radius = nullptr;   // MAX_SINKS accretion radii
    double *sink_part = nullptr;     // per-block partial sums for the sink accelerations
    int32_t sink_blocks = 0;

    // time step on the device: [0] dt, [1] t, [2] dt candidate
    double *d_dt = nullptr;
    double *dt_part = nullptr; int32_t dt_blocks = 0;

    // Riders of the persistent pair kernels on the plain fixed-h step (rider_common.hpp, DESIGN section 4 "Round 6"): their arguments
    void *d_dens_riders = nullptr, *d_force_riders = nullptr;   // DensRiders / ForceRiders on the device
    std::vector<unsigned char> dens_riders_host, force_riders_host;   // ... and what they hold (rewritten only on a change)

    // (what is valid and what is pending: the flags of sph::CtxState, ctx_state.hpp)

    // statistics and timing
    int64_t grid_builds = 0, nlist_builds = 0, density_passes = 0, force_passes = 0;
    int64_t device_bytes = 0;
    std::unordered_map<void *, size_t> allocs;   // every device allocation of this context
    int32_t rank = 0, nranks = 1;   // multi-GPU: only rank 0 adds the sink-sink pair terms before the all-reduce
    unsigned timing = 0;             // bit k: kernel group k is bracketed by HIP events
    int timing_stride = 1;           // ... every timing_stride-th launch of it (sph_timing_stride)
    int64_t timing_seen[32] = {};    // launches of group k since timing was switched on
    sph::TimingSlot tslot[SPH_K_COUNT];

    // the analysis calls (render, profile, energy, groups, gradients, sample, trace): private scratch, never the grid / list buffers above
    void *rnd_buf = nullptr; size_t rnd_bytes = 0;
    double *rnd_small = nullptr;     // per-block statistics, their result and the selection cursor
    double *rnd_pinned = nullptr;    // pinned read-back slots
    // sph_profile and sph_binned (profile.hip, binned.hip): the edge table's pinned staging copy and the event of its last upload
    double *prf_edge = nullptr; size_t prf_edge_cap = 0;
    hipEvent_t prf_evt = nullptr;
    // sph_history (history.hip): the log, its partial buffers and the host-side row / step / dropped counts
    sph::History *hist = nullptr;
    // sph_track (track.hip): the log, the membership bitmap with its prefix and tags, the fates and the host-side counts
    sph::Track *track = nullptr;
    // sph_dust (dust.hip): the grains' state, stored sample, log and fates and the host-side counts
    sph::Dust *dust = nullptr;
    // sph_frames (frames.hip): the log, the limb image, the partials, the device words and the host-side step count
    sph::Frames *frames = nullptr;
};

// Host scaffolding of every launcher that has the context as `c` and returns a status.
// SPH_HIP: a failing HIP call goes into c->err, as its own text and HIP's, and returns SPH_ERR_HIP.
#define SPH_HIP(expr)                                                       \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) {                                             \
            c->err = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            return SPH_ERR_HIP;                                             \
        }                                                                   \
    } while (0)

// SPH_TRY: a status other than SPH_OK is returned as it is (whoever produced it has set c->err)
#define SPH_TRY(expr)                  \
    do {                               \
        int _s = (expr);               \
        if (_s != SPH_OK) return _s;   \
    } while (0)

namespace sph {

inline int arg_error(sph_ctx *c, const char *who, const char *what) {
    c->err = std::string(who) + ": " + what;
    return SPH_ERR_ARG;
}

inline size_t align_up(size_t b) { return (b + 255) & ~(size_t)255; }

// blocks of `per` items over n items, at least one (an empty launch is an error)
inline unsigned blocks(int64_t n, int per) { return (unsigned)std::max<int64_t>((n + per - 1) / per, 1); }

// A call's buffers inside one scratch allocation.  The call writes its layout once, as a function that take()s every
// buffer in order, and runs it twice: on a null base for the size, then on the allocation.  A buffer's element type and
// count are stated where its pointer is made, every buffer starts 256-byte aligned, and a count of 0 takes no room.
struct Carve {
    char *base = nullptr;
    size_t bytes = 0;
    template <class T>
    T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += align_up(count * sizeof(T));
        return p;
    }
};

// device memory owned by the context (tracked so that sph_stats.device_bytes is exact)
int ctx_alloc_bytes(sph_ctx *c, void **p, size_t bytes, const char *what);
void ctx_free_ptr(sph_ctx *c, void *p);
template <class T>
inline int ctx_alloc(sph_ctx *c, T **p, size_t count, const char *what) {
    return ctx_alloc_bytes(c, reinterpret_cast<void **>(p), (count ? count : 1) * sizeof(T), what);
}
template <class T>
inline void ctx_free(sph_ctx *c, T *&p) {
    ctx_free_ptr(c, p);
    p = nullptr;
}

// The neighbour list's allocation, for every build that (re)sizes it: frees the list in place and allocates nl_cap entries a
// lane -- 16-bit ones on the tiled path (tile_common.hpp), 32-bit ones otherwise.  On failure the context holds no list.
inline int list_alloc(sph_ctx *c, int32_t new_cap) {
    ctx_free(c, c->nlist);
    c->nl_cap = new_cap;
    if (ctx_alloc(c, &c->nlist, (size_t)c->nl_waves_cap * c->nl_cap * (c->tiled ? 32 : 64), "neighbour list") != SPH_OK) { c->nl_cap = 0; return SPH_ERR_NOMEM; }
    return SPH_OK;
}

// all launchers enqueue on ctx->stream and return a hipError_t (no synchronisation unless noted)
hipError_t grid_sort_tmp_bytes(int64_t n, size_t *bytes);
// builds sorted order + cell table from the current positions.  Synchronises once (bbox read-back).
int grid_rebuild(sph_ctx *c);
void grid_hash_free(sph_ctx *c);
int64_t grid_occupied_cells(const sph_ctx *c);   // hashed: reads the occupied-cell count back (synchronises); dense: ncells
// builds the neighbour list; synchronises once (overflow check), grows the list if needed
int nlist_build(sph_ctx *c);
hipError_t launch_density(sph_ctx *c, const PairConst &pc);
hipError_t launch_eos_only(sph_ctx *c, const PairConst &pc, bool ghosts_only = false);
hipError_t launch_forces(sph_ctx *c, const PairConst &pc, int part = 0);
hipError_t launch_classify_waves(sph_ctx *c);
hipError_t launch_sink_accel(sph_ctx *c, const PairConst &pc, int from = 0);
int sink_accel_blocks(const sph_ctx *c);
hipError_t launch_kick(sph_ctx *c, double dt, bool dt_from_device);
hipError_t launch_drift(sph_ctx *c, double dt, bool dt_from_device);
hipError_t launch_next_dt(sph_ctx *c, bool advance_t);
hipError_t launch_unpermute(sph_ctx *c, const double *src_sorted, double *dst_original);
hipError_t launch_iota(sph_ctx *c, int32_t *p, int64_t n);
hipError_t launch_fill(sph_ctx *c, double *p, double v, int64_t n);
hipError_t launch_scatter_field(sph_ctx *c, double *field, int64_t first, int64_t count, const double *vals);
hipError_t launch_gather_fields(sph_ctx *c, int nf, const int *fields, const int64_t *ids, int64_t count, double *out);
hipError_t launch_gather_selected(sph_ctx *c, int nf, const int *fields, int box, int64_t capacity, double *out);
hipError_t launch_scatter_fields(sph_ctx *c, int nf, const int *fields, int64_t first, int64_t count, const double *vals);
hipError_t launch_dt_partial_only(sph_ctx *c);
hipError_t launch_kick_drift(sph_ctx *c);
// the same pass + cell keys, histogram and box partials of the new positions (grid.hip); needs grid_prepare_early, which
// sets c->keys_early where the next build is the plain dense counting-sort build over the previous build's box
int grid_prepare_early(sph_ctx *c);
hipError_t launch_kick_drift_keys(sph_ctx *c);
hipError_t ensure_inv(sph_ctx *c);               // inv of the current sorted order (a kernel only if the last reorder skipped it)
constexpr int EARLY_MAX_BLOCKS = 4096;           // box partials of launch_kick_drift_keys
constexpr size_t BBOX_PART_CLASSIC = (size_t)1024 * 8 + 64;      // doubles of bbox_part the classic build and owned_bbox use
hipError_t launch_kick_next_dt(sph_ctx *c, bool advance_t);   // closing kick + get_next_timestep in one pass      // kick + drift with the device dt in one pass (sph_step / sph_run)
hipError_t launch_kick_dt_candidate(sph_ctx *c, bool with_sinks = true);
hipError_t launch_kick_sinks(sph_ctx *c);
// multi-GPU building blocks (domain.hip, grid.hip)
int owned_bbox(sph_ctx *c, double *d_out6, double *h_out6);      // h_out6 != nullptr: synchronises
int domain_select_boxes(sph_ctx *c, int nbox, const double *boxes, int64_t *counts);
int domain_select_boxes_enqueue(sph_ctx *c, int nbox, const double *boxes);     // the same without waiting: counts to pinned memory
void domain_selected_counts(sph_ctx *c, int nbox, int64_t *counts);                // ... read after the caller's own synchronisation
int domain_replace_ghosts(sph_ctx *c, int64_t count, const double *d_vals);
hipError_t launch_pack_partials(sph_ctx *c, double *d_out, bool predict_box);
hipError_t launch_set_numbers(sph_ctx *c, int64_t first, int64_t count, const int64_t *d_numbers);
hipError_t launch_apply_partials(sph_ctx *c, const double *d_all, int nranks, int stride, bool apply_dt);
// LDS-tiled fixed-h kernels (tiled.hip; default)
int nlist_build_tiled(sph_ctx *c);
constexpr int WT_TILE_RECORDS = 3712;     // whole-tile kernels: {x,y,z,m} records per LDS tile (116 KB; + the kernel table <= 160 KB)
// ride_sink: the launch may carry sink_accel_partial as riders; *rode = the blocks it did carry (0: none).  rode > 0 for the
// forces: that many partials are there, and forces_q<., 4, .> carries sink_accel_final as a rider
hipError_t launch_density_wt(sph_ctx *c, const PairConst &pc, bool ride_sink = false, int32_t *rode = nullptr);
hipError_t launch_forces_wt(sph_ctx *c, const PairConst &pc, int part, int32_t rode = 0);
double forces_lane_efficiency(const std::vector<int32_t> &cnt);   // list entries / lane-trips of the forces kernel in use (host, statistics)
// self-gravity (gravity.hip)
hipError_t grav_sort_tmp_bytes(int64_t n, size_t *bytes);
int gravity_tree_build(sph_ctx *c);
int global_keys_sorted(sph_ctx *c);      // sorted path keys of the external source set -> c->g_keys_alt / g_vals_alt
void gravity_free(sph_ctx *c);
hipError_t launch_gravity(sph_ctx *c, double *ax = nullptr, double *ay = nullptr, double *az = nullptr);   // null: SPH_F_AX..AZ
// sph_energy (gravity.hip): the tree over caller-order {x,y,z,m} records and their box, built into the context's tree
// arrays (clears tree_valid, grav_valid, gx_keys_valid), and the potential walk over the tree in place
int gravity_tree_build_records(sph_ctx *c, const double *rec, int64_t n, const double box[6]);
hipError_t launch_potential(sph_ctx *c, int64_t n_src, int64_t src_off, double *phi);
// sph_gravity_at (gravity.hip): the walk over the tree in place with the caller's points as targets -> out[c * m + p], c < 4
hipError_t launch_field_points(sph_ctx *c, int64_t n_src, int64_t m, const double *px, const double *py, const double *pz,
                               const double *ph, double h_one, double soft2, const uint32_t *pidx, double *out);
// accretion + boundary cull (accrete.hip)
int accrete_and_cull(sph_ctx *c, int64_t *removed, int32_t *d_keep_out = nullptr);
int sink_creation(sph_ctx *c, int32_t *created);
int sink_candidate(sph_ctx *c, double *d_cand);    // multi-GPU halves of sink_creation
int sink_add_checked(sph_ctx *c, const double *d_cand, int32_t *created);
int sinks_cull(sph_ctx *c);                         // [V] check_bounds for the sinks    // [V] check_sink_creation; may add one sink (c->ns grows)
int accrete_mark_ext(sph_ctx *c, int64_t src_off, double *d_partials);       // multi-GPU: marks + per-rank sink sums
int accrete_apply_ext(sph_ctx *c, const double *d_all, int nranks, int stride, int32_t *d_keep_out, int64_t *removed);
// variable-h path (varh.hip)
hipError_t varh_sort_tmp_bytes(int64_t n, size_t *bytes);
int varh_h_stats(sph_ctx *c, bool with_growth = false);   // h_max_glob, h_mean (+ h_growth against c->h_new): one read-back
bool varh_can_reflag(const sph_ctx *c);
int varh_nlist_reflag(sph_ctx *c);
int varh_reflag_density(sph_ctx *c, const PairConst &pc);   // the re-flag pass and the density pass in one walk over the list
int varh_leaf_build(sph_ctx *c);       // leaf boxes of all particles for the current positions + h
int varh_nlist_build(sph_ctx *c);
int varh_refresh_h(sph_ctx *c);        // only h changed: prec, reaches and per-cell max h from the new h
hipError_t launch_density_v(sph_ctx *c, const PairConst &pc);
hipError_t launch_eos_only_v(sph_ctx *c, const PairConst &pc);
hipError_t launch_forces_v(sph_ctx *c, const PairConst &pc);
hipError_t launch_update_h(sph_ctx *c, const PairConst &pc);   // leaves the local candidate (min * dt_scale) in d_dt[2]
PairConst make_pair_const(const sph_ctx *c);
// density rendering (render.hip): out is host memory (host_out) or device memory; two read-backs (+ the host copy)
int render_density(sph_ctx *c, sph_render_desc *d, double *out, int64_t out_len, bool host_out);
// field rendering (render.hip): host (values, out and wout host memory) or device form
int render_field(sph_ctx *c, sph_render_field_desc *d, const double *values, double *out, double *wout, int64_t out_len,
                 bool host);
void render_free(sph_ctx *c);
// what the analysis calls share (render.hip; freed by render_free): their scratch, which grows and never shrinks, and the
// 32 pinned doubles of their read-backs, allocated at the first call that needs them
int analysis_scratch(sph_ctx *c, size_t bytes, char **out);
int analysis_pinned(sph_ctx *c);
// The small host tables of sph_profile, sph_binned, sph_pairs and sph_modes (edges, wavenumbers) travel to the device in the
// stream's order from one pinned staging copy of the context (freed by profile_free).  table_staging returns it with room
// for `count` doubles, after the host has waited for the copy's last upload (c->prf_evt): the one host wait of the device
// forms, which ends when the previous call's table copy has run.  The caller fills it, enqueues the copy and records
// c->prf_evt on the stream.
inline int table_staging(sph_ctx *c, size_t count, double **out) {
    if (!c->prf_evt) SPH_HIP(hipEventCreateWithFlags(&c->prf_evt, hipEventDisableTiming));
    SPH_HIP(hipEventSynchronize(c->prf_evt));
    if (count > c->prf_edge_cap) {
        if (c->prf_edge) SPH_HIP(hipHostFree(c->prf_edge));
        c->prf_edge = nullptr; c->prf_edge_cap = 0;
        SPH_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->prf_edge), count * sizeof(double), hipHostMallocDefault));
        c->prf_edge_cap = count;
    }
    *out = c->prf_edge;
    return SPH_OK;
}
// What sph_binned, sph_pairs and sph_modes share around the caller's values block: n_rows <= MAX_ROWS rows of c->n doubles by
// original id.  A source is an SPH_F_* id (>= 0) or -1 - row.
constexpr int MAX_ROWS = 16;
inline bool source_ok(int32_t id, int32_t n_rows) { return id >= 0 ? id < SPH_F_COUNT : -1 - (int64_t)id < n_rows; }
// the host forms' device copies of the rows that rows_used names (bit k: row k), in the stream's order
inline hipError_t upload_rows(double *dst, const double *src, int n_rows, uint32_t rows_used, size_t n, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_rows && e == hipSuccess; k++)
        if (rows_used >> k & 1u) e = hipMemcpyAsync(dst + k * n, src + k * n, n * sizeof(double), hipMemcpyHostToDevice, st);
    return e;
}
// zeroes n elements of an output: host memory (host form) or device memory in the stream's order; null: nothing to do
template <class T>
inline hipError_t zero_output(T *p, size_t n, bool host, hipStream_t st) {
    if (!p) return hipSuccess;
    if (!host) return hipMemsetAsync(p, 0, n * sizeof(T), st);
    std::memset(p, 0, n * sizeof(T));
    return hipSuccess;
}
// disc profiles (profile.hip): host form (sums and / or table host memory, one read-back) or device form (sums only)
int profile_sums(sph_ctx *c, sph_profile_desc *d, double *sums, double *table, int64_t n_bins, bool host);
void profile_free(sph_ctx *c);
// conserved totals and the gravitational potential (energy.hip): host form (sums / phi host memory, one read-back) or
// device form
int energy_sums(sph_ctx *c, int64_t src_offset, double *sums, double *phi, int64_t n_phi, bool host);
// the staged source records of sph_energy and sph_gravity_at (energy.hip): the owned gas in the caller's order + their box
int stage_blocks(int64_t n_owned);
int stage_sources(sph_ctx *c, double *rec, double *box_part, double bb[6]);
// friends-of-friends groups (groups.hip): host form (labels / table / count host memory, one synchronisation) or device
// form
int groups_run(sph_ctx *c, const sph_groups_desc *d, int32_t *labels, int64_t n_labels, double *table, int64_t max_groups,
               int64_t *n_groups, bool host);
// sph_groups' front end (selection, box, cell keys, sort, records and hashed cell table) and its tail (members per root,
// numbering, member sort, labels, the two table reductions) as host functions, shared with sph_peaks (peaks.hip), which
// puts its own partition between them.  Between the two, parent[id] is the root of every selected owned id (a root is
// the smallest id of its set and its own parent) and -1 for every other; cnt[] is 0 and gnum[] -1.
struct Ent;                                // cell_table.hpp
struct GroupsSel {                         // the selection and the link, by value to the kernels
    double rho_min, rho_cap, clip_lo[3], clip_hi[3];     // rho_min <= rho <= rho_cap (+INFINITY: sph_groups' rule)
    double link, fixed_h;                  // fixed_h: h of every particle when hf is null
    const double *hf;                      // SPH_F_H (variable h) or null
    int32_t link_h;
};
struct GroupsInfo {                        // on the device, written by groups_box (and n_groups by groups_number)
    double lo[3];
    double inv_e;                          // 1 / cell edge
    int64_t n_sel;                         // selected particles (0 when bad)
    int64_t n_groups;                      // -1: a selected particle has a bad h under LINK_H
    int32_t bad;
};
struct GroupsWork {                        // sizes (groups_sizes) and the buffers inside the call's scratch (groups_take)
    int64_t ns, no, gb, rows, n_pieces, tl;
    int nb;
    size_t sort_bytes;
    uint64_t *keys, *keys_alt;             // after groups_front: keys_alt / vals_alt = the sorted cell keys and their slots
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    double4 *rec;                          // {x, y, z, h} in sorted order
    int32_t *sid;                          // original id in sorted order
    Ent *tab;                              // tl entries
    GroupsInfo *info;
    int32_t *parent, *cnt, *gnum, *start;
    double *box_part, *part, *gstat;
};
void groups_sizes(const sph_ctx *c, int64_t min_members, int64_t max_groups, GroupsWork &w);   // max_groups: 0 without a table
void groups_take(GroupsWork &w, Carve &cv);
int groups_front(sph_ctx *c, const GroupsSel &s, GroupsWork &w);
// d_table: w.rows rows of SPH_GROUPS_NCOL doubles (device memory) or null with w.rows == 0; d_labels: c->n int32 or null
int groups_tail(sph_ctx *c, GroupsWork &w, int64_t min_members, int32_t *d_labels, double *d_table);
// density-peak clumps (peaks.hip): host form (labels / table / counts[3] host memory) or device form; both wait for the
// stream (the merge runs on the host)
int peaks_run(sph_ctx *c, const sph_peaks_desc *d, int32_t *labels, int64_t n_labels, double *table, int64_t max_groups,
              int64_t *counts, bool host);
// SPH gradients (gradients.hip): host form (values / out / rho host memory, counts[2] host, one synchronisation) or device
// form (counts[2] device memory or null)
int gradients_run(sph_ctx *c, const sph_gradients_desc *d, const double *values, double *out, int64_t n_out, double *rho_out,
                  int64_t *counts, bool host);
// SPH interpolation at arbitrary points (sample.hip): host form (points / values / out / weight host memory, counts[2] host,
// one synchronisation) or device form (counts[2] device memory or null)
int sample_run(sph_ctx *c, const sph_sample_desc *d, int64_t n_points, const double *px, const double *py, const double *pz,
               const double *values, double *out, int64_t n_out, double *weight, int64_t *counts, bool host);
// field lines of an SPH-interpolated vector field (trace.hip, over sample.hip's structure: sample_common.hpp): host form
// (seeds / values / path / carry / status / n_done host memory, counts[5] host, one synchronisation) or device form
// (counts[5] device memory or null)
int trace_run(sph_ctx *c, const sph_trace_desc *d, int64_t n_seeds, const double *sx, const double *sy, const double *sz,
              const double *values, double *path, int64_t n_path, double *carry_out, int32_t *status, int32_t *n_done,
              int64_t *counts, bool host);
// potential and acceleration at arbitrary points (gravity_at.hip): host form (points / ph / out host memory, counts[2]
// host) or device form (counts[2] device memory or null)
int gravity_at_run(sph_ctx *c, const sph_gravity_at_desc *d, int64_t n_points, const double *px, const double *py,
                   const double *pz, const double *ph, double *out, int64_t n_out, int64_t *counts, bool host);
// binding energies and unbinding of groups (bound.hip): host form (labels in, every output and counts[4] host memory) or
// device form (all device memory, no synchronisation)
int bound_run(sph_ctx *c, const sph_bound_desc *d, const int32_t *labels, int64_t n_labels, int64_t n_groups,
              int32_t *bound_labels, double *out, int64_t n_out, double *table, int64_t *counts, bool host);
// position-position-velocity cubes (cube.hip): host form (values / out host memory, two read-backs + the copy out) or device
// form
int cube_run(sph_ctx *c, const sph_cube_desc *d, const double *values, double *out, int64_t out_len, bool host);
// emission-absorption images (transfer.hip): host form (source / kappa / out host memory, two read-backs + the copy out) or
// device form
int transfer_run(sph_ctx *c, const sph_transfer_desc *d, const double *source, const double *kappa, double *out,
                 int64_t out_len, bool host);
// the rates of sph_forces split by term (terms.hip): host form (out host memory, one synchronisation) or device form
int force_terms_run(sph_ctx *c, const sph_force_terms_desc *d, double *out, int64_t n_out, bool host);
// binned sums (binned.hip): host form (values / sums / counts[3] host memory, one read-back) or device form (counts[3] device
// memory or null); edges is host memory in both
int binned_run(sph_ctx *c, const sph_binned_desc *d, const double *values, const double *edges, double *sums, int64_t n_sums,
               int64_t *counts, bool host);
// pair-separation sums (pair_stats.hip): host form (values / sums / raw / exps / counts[3] host memory, one read-back) or
// device form (raw, exps, counts device memory or null); edges is host memory in both
int pairs_run(sph_ctx *c, const sph_pairs_desc *d, const double *values, const double *edges, double *sums, int64_t n_out,
              uint64_t *raw, int32_t *exps, int64_t *counts, bool host);
// azimuthal and logarithmic-spiral mode sums (modes.hip): host form (values / sums / raw / exp / ring_counts / counts[4] host
// memory, one read-back) or device form (raw, exp, ring_counts, counts device memory or null)
int modes_run(sph_ctx *c, const sph_modes_desc *d, const double *values, double *sums, int64_t n_out, uint64_t *raw, int32_t *exp,
              int64_t *ring_counts, int64_t *counts, bool host);

// the per-step time series (history.hip).  history_step is the step's hook (a no-op without a history); history_read only
// enqueues the copy (the host form's caller synchronises)
int history_begin(sph_ctx *c, const sph_history_desc *d);
int history_end(sph_ctx *c);
void history_free(sph_ctx *c);
int history_record(sph_ctx *c);
int history_step(sph_ctx *c);
int history_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *steps, int32_t *width);
int history_read(sph_ctx *c, int64_t first, int64_t count, double *out, bool host);

// trajectories and fates of chosen particles (track.hip).  track_step is the step's hook and track_packed the accretion
// pack's (keep / pos by caller id, accmask by sorted slot; before any of them is reused); both are no-ops without a tracker
// or with a closed one.  track_close: the particle set was replaced, the ids mean nothing any more.  track_read and
// track_fates only enqueue the copies (the host forms' callers synchronise)
int track_begin(sph_ctx *c, const sph_track_desc *d, int64_t n_ids, const int64_t *ids, bool host);
int track_end(sph_ctx *c);
void track_free(sph_ctx *c);
void track_close(sph_ctx *c);
int track_record(sph_ctx *c);
int track_step(sph_ctx *c);
int track_packed(sph_ctx *c, const int32_t *keep, const int32_t *pos, const unsigned long long *accmask);
int track_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *steps, int64_t *n_tracked, int64_t *n_live, int32_t *closed);
int track_read(sph_ctx *c, int64_t first, int64_t count, double *head, double *body, bool host);
int track_fates(sph_ctx *c, int32_t *fates, bool host);

// drag-coupled tracer grains (dust.hip).  dust_step is the step's hook (called where c->dust is set; a no-op on closed
// dust); arrays: x y z vx vy vz par.  dust_close: ghosts or several ranks, no further advance.  dust_read, dust_state and
// dust_fates only enqueue the copies (the host forms' callers synchronise)
int dust_begin(sph_ctx *c, const sph_dust_desc *d, int64_t n, const double *const *arrays, bool host);
int dust_end(sph_ctx *c);
void dust_free(sph_ctx *c);
void dust_close(sph_ctx *c);
int dust_advance(sph_ctx *c);
int dust_step(sph_ctx *c);
int dust_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *advances, int64_t *n_grains, int64_t *n_live);
int dust_read(sph_ctx *c, int64_t first, int64_t count, double *head, double *body, bool host);
int dust_state(sph_ctx *c, double *const *arrays, bool host);
int dust_fates(sph_ctx *c, int32_t *fates, bool host);

// the movie of a run (frames.hip).  frames_step is the step's hook (called where c->frames is set); frames_read and frame_run
// only enqueue the copies (the host forms' callers synchronise); frames_info reads the device's counts and synchronises
int frames_begin(sph_ctx *c, const sph_frames_desc *d);
int frames_end(sph_ctx *c);
void frames_free(sph_ctx *c);
int frames_record(sph_ctx *c);
int frames_step(sph_ctx *c);
int frames_rewind(sph_ctx *c);
int frames_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *steps);
int frames_read(sph_ctx *c, int64_t first, int64_t count, double *head, double *planes, bool host);
int frame_run(sph_ctx *c, const sph_frames_desc *d, double *head, double *planes, int64_t out_len, bool host);

}  // namespace sph
