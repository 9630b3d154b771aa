/* summersph.h -- C ABI of the MI355X-native SPH core (libsummersph_hip.so).
 *
 * Drop-in boundary for the hot path of graves-andrew-02/SUMMERSPH: the calls `simulate`
 * makes between tree allocation and the second `kick` (reference file
 * SUMMER_SPH.f90, "[F]", lines 886-916).  The reference has no FFI; its de-facto interface
 * is the set of module procedures listed beside each entry point below.  A Fortran
 * maintainer binds these with `bind(C)` interfaces (summersph_amd/host/sph_hip_binding.f90,
 * INTEGRATION.md).
 *
 * Conventions
 *   - every entry point returns an int status (SPH_OK == 0); nothing aborts or prints.
 *     sph_strerror() / sph_last_error() give text.
 *   - caller-owned HOST arrays of double, contiguous, length n (struct-of-arrays); the
 *     opaque context owns all device memory.  *_dev variants take DEVICE pointers instead
 *     (inputs already resident in HBM).
 *   - one context per GPU, one host thread per context (not re-entrant per context).
 *   - particle order: whatever order the caller uploaded ("original order").  Internally
 *     particles live cell-sorted; every download un-permutes.
 *   - there is NO CPU fallback: without a HIP device sph_ctx_create fails with
 *     SPH_ERR_NO_DEVICE.
 */
#ifndef SUMMERSPH_H
#define SUMMERSPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_ABI_VERSION 1

typedef struct sph_ctx sph_ctx;

enum sph_status {
    SPH_OK = 0,
    SPH_ERR_ARG = 1,          /* null pointer, negative size, bad field id ...            */
    SPH_ERR_NO_DEVICE = 2,    /* no HIP device / device index out of range                */
    SPH_ERR_HIP = 3,          /* a HIP runtime call failed (text in sph_last_error)       */
    SPH_ERR_NOMEM = 4,        /* device or host allocation failed                         */
    SPH_ERR_STATE = 5,        /* call order violated (e.g. forces before density).  Also the fixed-h list overflow: a
                                 build reads the PREVIOUS build's reports, so a neighbour list that outgrows its
                                 third of headroom between two builds is reported one build late -- by the next
                                 sph_density / sph_step / sph_run, or at the end of the call that returns (every
                                 call that waits for the stream: sph_step, sph_run, sph_download_field, sph_get_stats)
                                 -- never as truncated sums handed out.  The sums of that build were incomplete and
                                 the context cannot tell what was integrated from them, so from then on
                                 sph_density, sph_forces, sph_step and sph_run return SPH_ERR_STATE and the derived
                                 fields are stale, until sph_upload brings a new particle set (sph_upload_field
                                 does not lift the refusal, whichever fields it rewrites)                  */
    SPH_ERR_GRID = 6,         /* no cell grid possible: a non-finite box, or one axis needs more than 2^21
                                 cells of edge 2h (2 <h>) even after the 6-sigma trim (a hashed grid holds
                                 any box up to that; a dense one up to 2^31 cells)        */
    SPH_ERR_NONFINITE = 7     /* NaN/Inf in particle positions at grid build               */
};

/* Runtime parameters.  Defaults (sph_params_default) are the reference's compile-time
 * constants of SUMMER_SPH.f90, with REAL(4)-rounded literals reproduced bit for bit. */
typedef struct sph_params {
    double h;            /* smoothing length; [F]:11 smoothing = 2.5                      */
    double gamma;        /* 1.4    ([F]:466)                                              */
    double gamma_m1;     /* 0.4    ([F]:465 writes the literal 0.4_dp, not gamma-1)       */
    int32_t nq;          /* 5000   ([F]:8) kernel-table intervals on q in [0,2]           */
    int32_t flags;       /* SPH_FLAG_*                                                    */
    double kernel_pi;    /* 3.14159265359 ([F]:125-126)                                   */
    double visc_eps;     /* (double)0.01f  ([F]:373)                                      */
    double alpha_floor;  /* 0.1    ([F]:317)                                              */
    double alpha_decay;  /* (double)0.15f ([F]:317)                                       */
    double G;            /* (double)39.47841760435743f ([F]:7)                            */
    double dt_scale;     /* 0.25   ([F]:851)                                              */
    double dt_max;       /* (double)0.1f    ([F]:855)                                     */
    double dt_min;       /* (double)0.0001f ([F]:857)                                     */
    double bounding_size;/* 1500   ([F]:11), used by sph_cull_bounds                      */
    /* variable-h path only ("SUMMER_SPH - Variable.f90", "[V]"; flags & SPH_FLAG_VARIABLE_H)  */
    double eta;          /* h = eta (m/rho)^(1/3) target of calc_smoothing ([V]:527)          */
    double h_tol;        /* convergence_criteria of calc_smoothing ([V]:529)                  */
    double h_max_length; /* max_length ([V]:528)                                              */
    double h_min_length; /* (double)0.01f ([V]:528)                                           */
    double h_iter_cap;   /* 10.0 ([V]:529)                                                    */
    /* Barnes-Hut gas self-gravity (flags & SPH_FLAG_SELF_GRAVITY)                              */
    double theta;        /* 0.5: opening angle, hard coded at the call site [F]:825 / [V]:1029 */
} sph_params;

/* flags */
#define SPH_FLAG_VARIABLE_H 2   /* per-particle smoothing length, grad-h terms and the leaf-box
                                   neighbour rule of the reference's variable-h variant [V]:
                                   kernel normalised with h_i and REAL(4) pi, nq = 2500, Omega,
                                   h update after every step.  Upload h with sph_upload_field. */
#define SPH_FLAG_SELF_GRAVITY 16 /* find_forces WITH the Barnes-Hut gas self-gravity term (particle_gravforces,
                                   [F]:249-290, 825): sph_forces then equals find_forces as it is (several GPUs:
                                   sph_set_gravity_sources_dev) */
#define SPH_FLAG_ACCRETE_CULL 32 /* sph_step / sph_run also do the end-of-step sink accretion and boundary cull
                                   of simulate() ([F]:919-920): the particle count may shrink (sph_count) */
#define SPH_FLAG_SINK_CREATION 64 /* variable h: sph_step / sph_run also run check_sink_creation ([V]:549-597, 1155): the
                                    number of sinks may grow by one per step (sph_sink_count)                  */
#define SPH_FLAG_NO_LDS_TILES 4  /* fixed-h path: build the neighbour list with per-lane gathers (pairs.hip)
                                   instead of LDS-staged tiles (tiled.hip); A/B measurements        */
/* flag bit 8 (round 1: SPH_FLAG_LDS_TILE_EVAL, chunk-staged density/forces kernels) was measured slower in every
   configuration and is gone; the bit is ignored */
#define SPH_FLAG_NO_WHOLE_TILE 128 /* fixed-h path: density/forces with the memory gathers of pairs.hip only, never the
                                   whole-tile kernels of tiled.hip (bitwise the same results); A/B measurements */
#define SPH_FLAG_REUSE_GRAVITY 256 /* self-gravity: keep the Barnes-Hut term of the last walk and copy it instead of
                                    walking again while positions, masses, h and the tree are unchanged -- the case of
                                    the start-of-step evaluation, which sees the positions of the previous step's
                                    last evaluation (bitwise the same accelerations); OFF by default: the reference
                                    walks its tree in both evaluations ([F]:898,910) and the headline numbers do too */
#define SPH_FLAG_NO_REFLAG 512   /* variable h: build the neighbour list anew also when only h changed since the last build
                                    (start of a step, after calc_smoothing); by default that list is derived in place from the
                                    list of the old lengths (varh.hip nlist_v_reflag: the same neighbour sets, entries in a
                                    different order); A/B measurements                                */
#define SPH_FLAG_HASHED_GRID 1024 /* always index the cell grid with the hashed table (64-bit cell keys, a hash table over
                                    the occupied cells) instead of the dense one; bitwise the same results.  Without it the
                                    hashed table is used where the dense one cannot be built: fixed h, a box of 2^31 cells
                                    or more after the trim; variable h, more than 2^27 cells (far-apart particle groups);
                                    sph_grid_info tells which one the last build used                     */
#define SPH_FLAG_REUSE_DENSITY 1 /* skip the density pass when positions and masses did not
                                    change since the last one (bitwise the same rho); OFF by
                                    default: the reference recomputes it, [F]:896,908 */

/* field ids for sph_download_field / sph_field_dev */
enum sph_field {
    SPH_F_X = 0, SPH_F_Y, SPH_F_Z, SPH_F_VX, SPH_F_VY, SPH_F_VZ, SPH_F_U, SPH_F_M, SPH_F_ALPHA,
    SPH_F_RHO, SPH_F_P, SPH_F_C, SPH_F_AX, SPH_F_AY, SPH_F_AZ, SPH_F_DU, SPH_F_DALPHA,
    SPH_F_H,        /* smoothing length (state, variable-h path; [V]:24 s_length)             */
    SPH_F_OMEGA,    /* grad-h factor (derived, variable-h path; [V]:25 omega)                  */
    SPH_F_COUNT
};

/* kernels whose device time is recorded when timing is on */
enum sph_kernel_id {
    SPH_K_GRID = 0,    /* bbox + keys + sort + cell table + reorder                        */
    SPH_K_NLIST,       /* neighbour-list build                                            */
    SPH_K_DENSITY,     /* density + EOS                                                   */
    SPH_K_FORCES,      /* sink gravity + SPH pair forces + alpha rate                     */
    SPH_K_SINKACC,     /* acceleration of the sinks                                       */
    SPH_K_KICK, SPH_K_DRIFT, SPH_K_DT,
    SPH_K_LEAF,        /* variable-h: octree leaf boxes (Morton keys, sort, depth)             */
    SPH_K_UPDATE_H,    /* variable-h: calc_smoothing                                          */
    SPH_K_GRAVITY,     /* self-gravity: octree keys, radix tree, node sums, tree walk          */
    SPH_K_GRAV_WALK,   /* self-gravity: the tree walk alone (inside SPH_K_GRAVITY)             */
    SPH_K_REFLAG,      /* variable-h: the list of the new h derived from the list in place (nlist_v_reflag);
                          SPH_K_NLIST then counts list BUILDS only                              */
    SPH_K_COUNT
};

typedef struct sph_stats {
    int64_t n;              /* gas particles                                              */
    int64_t n_cells;        /* cells of the current grid (hashed grid: the occupied ones)  */
    int32_t grid_dim[3];    /* cells along x, y, z (hashed grid: of the index)            */
    int32_t nlist_capacity; /* neighbour slots per particle currently allocated           */
    int32_t nlist_max;      /* largest neighbour count found at the last build            */
    int32_t tile_fit_pct;   /* fixed h: workgroups (%) whose neighbour intervals fit the LDS tile of the
                               whole-tile pair kernels at the last build; those kernels run when >= 90;
                               -1: kernels off (flags, variable h)                        */
    double  nlist_mean;     /* mean neighbour count (pairs inside 2h, self excluded)      */
    int64_t grid_builds, nlist_builds, density_passes, force_passes;
    int64_t device_bytes;   /* HBM held by the context                                    */
    double  nlist_wave_mean;/* mean over wavefronts of the longest list in the wave = trips the pair kernels run */
    int32_t tile_fit_pct_forces; /* as tile_fit_pct, for the forces kernel's workgroup size and tile record            */
    int32_t host_syncs;     /* stream synchronisations inside grid / list builds since the context was created: a
                               steady-state fixed-h step adds none (read-backs are taken one build late)       */
    double  lane_efficiency_forces; /* fixed h: list entries / lane-trips of the forces kernel in use (1 = no idle lanes):
                                       forces_q deals targets by list length, so this is not nlist_mean / nlist_wave_mean */
    int64_t nlist_reflags;  /* variable h: list builds replaced by the re-flag pass (same positions, new h: the list of the
                               new lengths derived from the list in place, entry for entry what a build would write) */
} sph_stats;

/* ---- life cycle: replaces init_kernel_table ([F]:55-79) and the tree (de)allocation
 *      in simulate ([F]:894,901,905,928) ------------------------------------------------ */
int sph_params_default(sph_params *p);
/* defaults of the variable-h variant: SPH_FLAG_VARIABLE_H, nq 2500, REAL(4) pi, gamma_m1 =
 * gamma - 1.0, eta 1.2, h_tol 1e-3, h_max_length 10 (the reference ships no parameters.txt) */
int sph_params_default_variable(sph_params *p);
int sph_ctx_create(const sph_params *p, int device, sph_ctx **out);
int sph_ctx_destroy(sph_ctx *ctx);
const char *sph_strerror(int status);
const char *sph_last_error(const sph_ctx *ctx);
int sph_abi_version(void);
/* the parameters the context was created with */
int sph_get_params(const sph_ctx *ctx, sph_params *out);

/* ---- state hand-over: replaces packing from `type(particle)` / `type(sink)` ([F]:14-37).
 *      alpha may be NULL (-> 0, as the reader initialises it, [F]:681). ------------------ */
int sph_upload(sph_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
               const double *vx, const double *vy, const double *vz,
               const double *u, const double *m, const double *alpha);
int sph_upload_dev(sph_ctx *ctx, int64_t n, const double *d_x, const double *d_y, const double *d_z,
                   const double *d_vx, const double *d_vy, const double *d_vz,
                   const double *d_u, const double *d_m, const double *d_alpha);
int sph_set_sinks(sph_ctx *ctx, int32_t ns, const double *sx, const double *sy, const double *sz,
                  const double *svx, const double *svy, const double *svz, const double *sm);
/* any output pointer may be NULL */
int sph_get_sinks(sph_ctx *ctx, int32_t ns, double *sx, double *sy, double *sz,
                  double *svx, double *svy, double *svz, double *sm,
                  double *sax, double *say, double *saz);
/* accretion radii of the sinks ([F]:694: 3.5, [V]:830: 5.0 for file sinks, 0 for the dummy sink); the
 * defaults set by sph_set_sinks are 3.5 (fixed h) / 5.0 (variable h) */
int sph_set_sink_radii(sph_ctx *ctx, int32_t ns, const double *radius);
int sph_get_sink_radii(sph_ctx *ctx, int32_t ns, double *radius);
int64_t sph_count(const sph_ctx *ctx);
int32_t sph_sink_count(const sph_ctx *ctx);
/* check_sink_creation of the variable-h reference ([V]:549-597) on the sorted order of the last sph_density: the first
 * particle (caller's order) with m (eta/h)^3 > 0.5 either lies within radius + 2h of a sink (nothing happens) or a
 * sink of mass 1e-11 and radius 2h is created at its position; *created = 0/1 */
int sph_check_sink_creation(sph_ctx *ctx, int32_t *created);
/* the two halves of it for several GPUs: the first candidate among the owned particles as a record of SPH_SINK_CAND
 * doubles {particle number or +inf, x, y, z, vx, vy, vz, h, 0} in device memory; the caller all-gathers the records,
 * picks the lowest number and hands that record to every context, which applies the distance test and the creation */
#define SPH_SINK_CAND 9
int sph_sink_candidate_dev(sph_ctx *ctx, double *d_cand);
int sph_add_sink_checked_dev(sph_ctx *ctx, const double *d_cand, int32_t *created);
/* one field in the caller's particle order, host or device source (e.g. SPH_F_H after sph_upload) */
int sph_upload_field(sph_ctx *ctx, int field, const double *host, int64_t n);
int sph_upload_field_dev(sph_ctx *ctx, int field, const double *d_vals, int64_t n);

/* ---- the hot path ------------------------------------------------------------------- */
/* create_tree + get_density + get_pressure_and_sound_speed   ([F]:894-897, 398-468)      */
int sph_density(sph_ctx *ctx);
/* find_forces ([F]:818-829): zero_rates, [particle_gravforces when SPH_FLAG_SELF_GRAVITY],
 * sink_gravforces, get_SPH   ([F]:249-290, 559-591, 295-395)                             */
int sph_forces(sph_ctx *ctx);
/* kick ([F]:742-759) and drift ([F]:762-776), gas and sinks                              */
int sph_kick(sph_ctx *ctx, double dt);
int sph_drift(sph_ctx *ctx, double dt);
/* get_next_timestep ([F]:831-860): in/out dt                                             */
int sph_next_dt(sph_ctx *ctx, double *dt);
/* initiate_sink_accretion (only if a sink has mass, [F]:919) + check_bounds ([F]:920) on the current
 * positions: removes accreted / escaped particles on the device, merges accreted mass and momentum
 * into the sinks.  Survivors keep their relative order: the caller's numbering becomes the rank among
 * survivors, as after the reference's pack().  Needs the grid of the current positions (call it after
 * sph_density / sph_forces / sph_kick, before the next sph_drift).                               */
int sph_accrete_and_cull(sph_ctx *ctx, int64_t *n_removed);
/* the same, and which particles stayed: d_keep (device, one int32 per particle held BEFORE the call, the caller's order;
 * 1 = survivor) -- for a caller that keeps per-particle data of its own beside the context (the global numbers of
 * libsummersph_halo.so) and has to pack() it the same way ([F]:481,554)                                          */
int sph_accrete_and_cull_keep(sph_ctx *ctx, int32_t *d_keep, int64_t *n_removed);
/* variable-h only: calc_smoothing ([V]:515-546) on the neighbour structure of the last evaluation */
int sph_update_h(sph_ctx *ctx);
/* one iteration of simulate's loop body, [F]:889-916 (variable-h: [V]:1120-1152 incl. the h update): density, forces, kick, drift,
 * density, forces, kick, t += dt, next dt.  Identical to the unfused call sequence.      */
int sph_step(sph_ctx *ctx, double *dt, double *t);
/* nsteps iterations without returning to the host in between (dt stays on the device)    */
int sph_run(sph_ctx *ctx, int32_t nsteps, double *dt, double *t);

/* ---- read-back, original particle order ---------------------------------------------- */
int sph_download_field(sph_ctx *ctx, int field, double *host, int64_t n);
int sph_download_field_dev(sph_ctx *ctx, int field, double *d_out, int64_t n);
int sph_download_state(sph_ctx *ctx, int64_t n, double *x, double *y, double *z,
                       double *vx, double *vy, double *vz, double *u, double *m, double *alpha);

/* ---- multi-GPU building blocks (one context per GPU; orchestration: summersph_amd/dist.py) --
 * A context may hold GHOST particles: copies of other GPUs' particles that lie within 2h of
 * this GPU's domain.  Upload owned particles first and ghosts after them, then declare how
 * many are owned: original ids [n_owned, n) are ghosts.  Ghosts act as neighbours in the
 * density and force sums but are never targets (no rho, rates, dt candidate or sink pull is
 * computed for them); their rho comes from their owner through sph_scatter_field_dev.      */
int sph_set_owned(sph_ctx *ctx, int64_t n_owned);
int sph_set_rank(sph_ctx *ctx, int32_t rank, int32_t nranks);
/* field[slot of original id first+k] = d_vals[k], k in [0,count): refreshes ghost rho after the
 * owners' density pass, or ghost v, u, alpha after a kick.                                 */
int sph_scatter_field_dev(sph_ctx *ctx, int field, int64_t first, int64_t count, const double *d_vals);
/* several fields at once (one kernel, one synchronisation):
 * gather : d_out[f*count + k] = field fields[f] of the particle with original id d_ids[k]
 *          (d_ids == NULL: ids 0..count-1, e.g. all owned particles)
 * scatter: field fields[f] of original id first+k = d_vals[f*count + k]                      */
int sph_gather_fields_dev(sph_ctx *ctx, int32_t nf, const int32_t *fields, int64_t count,
                          const int64_t *d_ids, double *d_out);
int sph_scatter_fields_dev(sph_ctx *ctx, int32_t nf, const int32_t *fields, int64_t first, int64_t count,
                           const double *d_vals);
/* ---- the same exchange kept on the device (no re-upload, no host reductions) ----------------
 * sph_set_stream      run the context on the caller's HIP stream (e.g. torch's current stream; NULL =
 *                     the default stream): calls that take device pointers then stop synchronising
 *                     and are ordered with the caller's own work on that stream.
 * sph_reserve         minimum slot capacity of the next sph_upload (room for ghosts).
 * sph_owned_bbox      min xyz, max xyz of the owned particles at their current positions, to the host
 *                     (lo_hi, synchronises) and/or to device memory (d_lo_hi).
 * sph_select_boxes    for each of nbox boxes {lo xyz, hi xyz}: the owned particles inside, ascending
 *                     original id; counts to the host; ids fetched with sph_selected_ids_dev.
 * sph_select_boxes_async  the same selection without the wait: the counts stay on the device (and travel to pinned memory
 *                     behind the selection); sph_gather_selected_dev packs a selection whose size only the device knows:
 *                     d_out[0] = count, d_out[1] = 0, then d_out[2 + f*count + k] -- if count <= capacity, else the header
 *                     alone; sph_selected_counts hands the counts over once the caller has synchronised with whatever
 *                     followed the selection on the context's stream (it does not wait itself).
 * sph_replace_ghosts_dev  drop the current ghosts and append `count` new ones (d_state[f*count + k],
 *                     f = x y z vx vy vz u m alpha); owned particles stay where they are, the next
 *                     sph_density re-sorts everything.  SPH_ERR_NOMEM if the slots do not suffice.
 * sph_set_dt / sph_get_dt, sph_kick_devdt / sph_drift_devdt: dt and t held on the device
 *                     (sph_run's mechanism), so that a step needs no host round trip for them.
 * sph_kick_drift_devdt / sph_kick_dt_candidate_dev: the same pairs of calls fused into one pass over the state each
 *                     (kick + drift; closing kick + local dt candidate), bitwise the separate calls.
 *                     sph_kick_dt_candidate_gas_dev + sph_kick_sinks_devdt split the latter into its gas and its sink part, so
 *                     that the gas is kicked while the sinks' accelerations still travel through the rank reduction.
 * sph_dt_candidate_dev    local dt candidate ([F]:845-851 over owned particles) kept on the device.
 * sph_pack_partials_dev   d_out[0..3*64) = this GPU's partial sink accelerations (ax[64] ay[64]
 *                     az[64]), d_out[192] = its dt candidate, d_out[193..199) = the bounding box its owned particles
 *                     will have after the coming kick + drift (union over the three dt values the dt rule can
 *                     produce; NaN when the rates are stale): SPH_PARTIALS doubles, to be
 *                     all-gathered by the caller.
 *                     sph_pack_partials_ex_dev(.., predict_box = 0) leaves the box out (NaN): it costs a pass over the
 *                     particles and only a reduction that is followed by a drift has a reader for it.
 * sph_apply_partials_dev  sink accelerations = sum over the nranks gathered blocks (rank order);
 *                     apply_dt != 0: t += dt, then [F]:855-858 with the minimum candidate.
 * sph_set_boundary_boxes / sph_forces_part: forces in two launches so that the exchange of ghost fields overlaps
 *                     the bulk of the work.  boxes = the other GPUs' bounding boxes {lo xyz, hi xyz} (every ghost lies
 *                     inside them).  part 1: sink gravity + every wavefront whose 64 particles are all farther than
 *                     2h from all boxes (they cannot have a ghost neighbour); part 2 (after the ghost fields arrived
 *                     and sph_refresh_eos ran): the remaining wavefronts.  Together identical to sph_forces.
 *                     Fixed-h contexts without self-gravity.
 * sph_set_gravity_sources_dev  self-gravity from a particle set other than the context's own: n_src records
 *                     {x, y, z, m} in device memory (caller-owned, must stay valid until replaced) and their bounding
 *                     box {min xyz, max xyz} (host).  The Barnes-Hut tree is then built over these sources -- with
 *                     every GPU's particles all-gathered into them it is the SAME tree on every GPU as the single
 *                     tree of the undecomposed run -- and walked for the context's owned particles.  n_src = 0: back
 *                     to the context's own particles.
 * sph_accrete_mark_dev / sph_accrete_apply_dev  sink accretion + boundary cull ([F]:471-556) when the octree is that of
 *                     all GPUs' particles (after sph_forces with sph_set_gravity_sources_dev; src_offset = position
 *                     of this GPU's owned particles, in the caller's order, inside the source set).  mark: decides for
 *                     the owned particles and writes this GPU's sums per sink (m, m x, m y, m z, m vx, m vy, m vz:
 *                     SPH_ACC_PARTIALS doubles) to d_partials; the caller all-gathers them.  apply: sink update from the
 *                     sums of all ranks (rank order), then the context keeps only the surviving OWNED particles, in
 *                     the caller's order (ghosts are dropped); d_keep (optional) receives keep[0..n_owned_before).
 * sph_set_numbers_dev  variable h: the reference's particle numbers (the rank in the input file) of original ids
 *                     [first, first + count).  The force pair {a, b} is evaluated iff the walk of the HIGHER-numbered
 *                     partner reaches the other's leaf ([V]:383), so on several GPUs the numbers must be the global
 *                     ones, for owned particles and ghosts alike.  Without this call: the context's own numbering.
 *                     With SPH_FLAG_VARIABLE_H sph_replace_ghosts_dev takes 10 rows (.. alpha, h) and
 *                     sph_set_gravity_sources_dev also supplies the octree the leaf boxes are taken from.            */
#define SPH_PARTIALS 199
int sph_set_numbers_dev(sph_ctx *ctx, int64_t first, int64_t count, const int64_t *d_numbers);
#define SPH_ACC_PARTIALS 448
int sph_accrete_mark_dev(sph_ctx *ctx, int64_t src_offset, double *d_partials);
int sph_accrete_apply_dev(sph_ctx *ctx, const double *d_all, int32_t nranks, int32_t stride, int32_t *d_keep, int64_t *n_removed);
int sph_set_gravity_sources_dev(sph_ctx *ctx, int64_t n_src, const double *d_xyzm, const double *lo_hi);
int sph_set_boundary_boxes(sph_ctx *ctx, int32_t nbox, const double *boxes);
int sph_forces_part(sph_ctx *ctx, int32_t part);
int sph_set_stream(sph_ctx *ctx, void *hip_stream);
int sph_reserve(sph_ctx *ctx, int64_t n_slots);
int sph_owned_bbox(sph_ctx *ctx, double *lo_hi, double *d_lo_hi);
int sph_select_boxes(sph_ctx *ctx, int32_t nbox, const double *boxes, int64_t *counts);
int sph_selected_ids_dev(sph_ctx *ctx, int32_t box, int64_t count, int64_t *d_ids);
int sph_select_boxes_async(sph_ctx *ctx, int32_t nbox, const double *boxes);
int sph_selected_counts(sph_ctx *ctx, int32_t nbox, int64_t *counts);
int sph_gather_selected_dev(sph_ctx *ctx, int32_t box, int32_t nf, const int32_t *fields, int64_t capacity, double *d_out);
int sph_replace_ghosts_dev(sph_ctx *ctx, int64_t count, const double *d_state);
int sph_set_dt(sph_ctx *ctx, double dt, double t);
int sph_get_dt(sph_ctx *ctx, double *dt, double *t);
int sph_kick_devdt(sph_ctx *ctx);
int sph_drift_devdt(sph_ctx *ctx);
int sph_dt_candidate_dev(sph_ctx *ctx);
int sph_kick_drift_devdt(sph_ctx *ctx);
int sph_kick_dt_candidate_dev(sph_ctx *ctx);
int sph_kick_dt_candidate_gas_dev(sph_ctx *ctx);
int sph_kick_sinks_devdt(sph_ctx *ctx);
int sph_pack_partials_dev(sph_ctx *ctx, double *d_out);
int sph_pack_partials_ex_dev(sph_ctx *ctx, double *d_out, int32_t predict_box);
int sph_apply_partials_dev(sph_ctx *ctx, const double *d_all, int32_t nranks, int32_t stride, int32_t apply_dt);
/* P, c and the force gather records of ALL slots from the current rho, u, alpha, v          */
int sph_refresh_eos(sph_ctx *ctx);
/* the same for the ghost slots only (the owned particles' records are written by sph_density itself) */
int sph_refresh_eos_ghosts(sph_ctx *ctx);
/* the local part of get_next_timestep ([F]:845-851): min over OWNED particles * dt_scale;
 * the caller min-reduces over ranks and applies [F]:855-858                                */
int sph_dt_candidate(sph_ctx *ctx, double *candidate);
/* overwrite the sink accelerations (after summing the per-GPU partial sums over ranks)     */
int sph_set_sink_accel(sph_ctx *ctx, int32_t ns, const double *sax, const double *say, const double *saz);

/* ---- density rendering: replaces the grid loop and the projection of the reference's imaging script
 *      (Density_Image.py: KD-tree ball query per node of a 120^3 grid, m W(r, h) summed, grid summed along z) --------
 * For a node g and the selected particles j:  D(g) = sum_j m_j W(|g - r_j|, h_j),  W(r, h) = sigma (1 - 1.5 q^2 + 0.75 q^3)
 * for q <= 1, sigma 0.25 (2 - q)^3 for 1 < q <= 2, 0 beyond; q = r / h, sigma = 1 / (pi h^3) with the DOUBLE-precision pi.
 * This is the script's analytic kernel, not the simulation's REAL(4)-pi table: a rendered density is not the rho field.
 *   selection   the context's owned gas particles (ghosts excluded as sph_owned_bbox excludes them; sinks are never
 *               rendered) with clip_lo < x < clip_hi on every axis (strict; -INFINITY / +INFINITY: no clip)
 *   h           > 0: one h for every particle (the script's 1.25); 0: each particle's own h (SPH_F_H on a variable-h
 *               context, params.h on a fixed-h one)
 *   nodes       node i on axis a is lo[a] + i (hi[a] - lo[a]) / (n[a] - 1), the last one exactly hi[a] (np.linspace);
 *               n[a] == 1: the single node lo[a].  SPH_RENDER_AUTO_BOUNDS: lo / hi = min / max of the selected
 *               particles (the script's default), written back into the descriptor
 *   output      axis = -1: the n0 n1 n2 grid in C order [i][j][k] (x slowest, meshgrid(indexing='ij')); axis 0, 1, 2: the
 *               column sums along that axis, the two other axes in order.  A column sum adds the 3-D mode's node values
 *               in increasing node index (bitwise the sequential sum of the 3-D output).  SPH_RENDER_SPACING multiplies
 *               the sums by that axis's node spacing (hi - lo) / (n - 1): a column density
 *   flat axes   lo[a] == hi[a] with n[a] > 1 (SPH_RENDER_AUTO_BOUNDS over a coplanar selection gives it) is valid: the n[a]
 *               nodes of that axis coincide, the 3-D output repeats one plane, a column sum along the axis adds it n[a]
 *               times, and the node spacing is 0: with SPH_RENDER_SPACING that column image is all zeros
 *   order       every node adds its terms in the (cell, particle id) order of the render's own binning, which depends
 *               only on the node box, n, h and the clip: results are bitwise reproducible, independent of the context's
 *               sorted order and of axis / flags
 *   cost        two stream synchronisations (selection statistics, window size) + the output copy of the host form; no
 *               state, statistic (other than device_bytes: the render's scratch) or flag of the context changes
 * SPH_ERR_ARG: null pointer, n < 1, out_len != the output's size, lo > hi, h < 0, axis out of range, SPH_RENDER_SPACING
 * without a projection axis of n > 1, reserved != 0, SPH_RENDER_AUTO_BOUNDS over an empty selection.  SPH_ERR_NOMEM:
 * the scratch does not fit.  sph_render_density_dev leaves the result in device memory (ordered on the context's stream). */
#define SPH_RENDER_AUTO_BOUNDS 1
#define SPH_RENDER_SPACING 2
typedef struct sph_render_desc {
    double  lo[3], hi[3];           /* node box (written back with SPH_RENDER_AUTO_BOUNDS)          */
    double  clip_lo[3], clip_hi[3]; /* strict particle clip box; -INFINITY / +INFINITY = none        */
    double  h;                      /* > 0: one h for all; 0: each particle's own h                  */
    int32_t n[3];                   /* nodes per axis, each >= 1                                     */
    int32_t axis;                   /* -1: 3-D grid; 0, 1, 2: column sums along that axis            */
    int32_t flags;                  /* SPH_RENDER_AUTO_BOUNDS | SPH_RENDER_SPACING                   */
    int32_t reserved;               /* must be 0                                                     */
} sph_render_desc;
int sph_render_density(sph_ctx *ctx, sph_render_desc *d, double *host_out, int64_t out_len);
int sph_render_density_dev(sph_ctx *ctx, sph_render_desc *d, double *d_out, int64_t out_len);

/* ---- field rendering: any per-particle quantity A on the density render's nodes (temperature, moment-1 velocity,
 *      alpha maps ...) -----------------------------------------------------------------------------------------------
 * The same selection, nodes, kernel, h rule and summation order as sph_render_density (base: exactly its descriptor,
 * auto bounds written back).  With s_j = 1 / (pi h_j^3) as there, for a node g:
 *   ws_j = m_j s_j            SPH_RENDER_WEIGHT_MASS   (bitwise the density render's term weight)
 *        = (m_j / rho_j) s_j  SPH_RENDER_WEIGHT_VOLUME (rho_j: the context's SPH_F_RHO)
 *   wa_j = ws_j A_j,   num(g) = sum_j wa_j Wn(q),   den(g) = sum_j ws_j Wn(q)   (Wn = W / s_j, the same skip test)
 *   output      normalise 0: num (3-D) or col_num * scale (projection; scale = the node spacing with SPH_RENDER_SPACING,
 *               else 1) -- MASS: sum m A W (e.g. momentum density); VOLUME: the SPH interpolant sum (m / rho) A W.
 *               normalise 1: num / den (3-D) or col_num / col_den (projection, no scale), exactly 0.0 where the
 *               denominator is 0.0 -- MASS + projection: the density-weighted line-of-sight mean (a temperature or
 *               moment-1 map); VOLUME: the Shepard-normalised interpolant.
 *               Column sums add the node values in increasing index, as the density render does.
 *   weight      optional (NULL = none): den (3-D) or col_den * scale.  Summing images and weights of separate contexts
 *               or ranks and dividing gives the normalised image of the union.
 *   field       an SPH_F_* id, read from the context (SPH_ERR_STATE where sph_download_field would refuse it as stale),
 *               or SPH_RENDER_FIELD_VALUES with values: sph_count(ctx) doubles in sph_download_field's order (upload
 *               order; after a cull, the survivors' order) -- host memory for sph_render_field, device memory for _dev.
 *               Only the selected (owned) particles' entries are read.
 *   VOLUME reads the rho that sph_download_field(SPH_F_RHO) would return: SPH_ERR_STATE exactly when that call would be.
 *   cost        as sph_render_density (two read-backs + the output copies), plus the copy of values in the host form; no
 *               state, statistic (other than device_bytes) or flag of the context changes.
 * SPH_ERR_ARG: everything sph_render_density rejects, a field id out of range, values NULL with SPH_RENDER_FIELD_VALUES
 * or non-NULL with a field id, weight not MASS / VOLUME, normalise not 0 / 1, reserved != 0. */
#define SPH_RENDER_FIELD_VALUES (-1)
#define SPH_RENDER_WEIGHT_MASS 0
#define SPH_RENDER_WEIGHT_VOLUME 1
typedef struct sph_render_field_desc {
    sph_render_desc base;           /* as for sph_render_density; base.reserved must be 0            */
    int32_t field;                  /* SPH_F_* or SPH_RENDER_FIELD_VALUES                            */
    int32_t weight;                 /* SPH_RENDER_WEIGHT_MASS / SPH_RENDER_WEIGHT_VOLUME             */
    int32_t normalise;              /* 0: num; 1: num / den                                          */
    int32_t reserved;               /* must be 0                                                     */
} sph_render_field_desc;            /* 144 bytes */
int sph_render_field(sph_ctx *ctx, sph_render_field_desc *d, const double *values, double *host_out, double *host_weight,
                     int64_t out_len);
int sph_render_field_dev(sph_ctx *ctx, sph_render_field_desc *d, const double *d_values, double *d_out, double *d_weight,
                         int64_t out_len);

/* ---- disc profiles: binned, mass-weighted moments of the owned gas particles in rings (and ring sectors) about a
 *      centre, in the frame of a disc normal (surface density, rotation, epicyclic frequency, scale height, Toomre Q,
 *      radial drift and accretion rate, tilt, twist and eccentricity of each ring) ----------------------------------------
 * Frame    n^ = normal / |normal|; a = x^ if |n^_x| <= 0.9 else y^; e1 = (a - (a.n^) n^) / |a - (a.n^) n^|; e2 = n^ x e1
 *          (n^ = z^ gives the lab axes).  Centre c and velocity v_c: centre / centre_v, or sink `sink`'s position and
 *          velocity on the device (then central_mass is that sink's mass).  Per particle, in this order, with no fused
 *          multiply-adds (a.b = (a0 b0 + a1 b1) + a2 b2):  r' = r - c, v' = v - v_c, X = r'.e1, Y = r'.e2, z' = r'.n^,
 *          R = sqrt(X X + Y Y), v1 = v'.e1, v2 = v'.e2, v_z = v'.n^, v_R = (X v1 + Y v2) / R, v_phi = (X v2 - Y v1) / R
 *          (both 0 where R == 0), phi = atan2(Y, X) with +pi taken as -pi.
 * Select   the owned gas particles (ghosts and sinks excluded, as the renders select) with r_min <= R < r_max and
 *          |z'| < z_max (strict; INFINITY: no cut).
 * Bins     ring edges computed once on the host: edge[k] = r_min + (k (r_max - r_min)) / n_r, or with SPH_PROFILE_LOG
 *          r_min pow(r_max / r_min, k / n_r); edge[n_r] = r_max exactly.  Ring k: edge[k] <= R < edge[k + 1] against that
 *          table.  Sector j: -pi + (2 pi j) / n_phi <= phi < -pi + (2 pi (j + 1)) / n_phi.  Bin b = k n_phi + j.
 * Sums     sums[b * SPH_PROFILE_NSUM + s], s = 0..19:  N (count as a double), M = sum m, then sum m q for q =
 *          R, z', z' z', v_R, v_phi, v_z, v_R v_R, v_phi v_phi, v_z v_z, u, alpha, h (params.h; SPH_F_H with variable h),
 *          l_x, l_y, l_z, e_x, e_y, e_z  (each term m * q).  Lab components: l = r' x v' =
 *          (r'y v'z - r'z v'y, r'z v'x - r'x v'z, r'x v'y - r'y v'x) and e = w / (G M_c) - r' / |r'| with w = v' x l (the
 *          same component form), |r'| = sqrt((r'x r'x + r'y r'y) + r'z r'z), r' / |r'| = 0 where |r'| == 0, G = params.G,
 *          M_c = central_mass; e = 0 where G M_c <= 0.  The sums are additive: those of two contexts or ranks add up to
 *          the sums of the union.
 * Order    the selected particles are sorted by (bin, original id); every bin's sums are reduced in a fixed shape that
 *          depends only on that sorted sequence (pieces of 1024 sorted positions, each added by a 64-lane wavefront, then
 *          the pieces by another): the sums are bitwise reproducible, independent of the context's sorted order, of the
 *          dense or hashed grid and of repeated calls.  No float atomics.
 * AUTO_NORMAL  normal = sum m (r' x v') over the owned gas in the shell r_min <= |r'| < r_max (no z cut), by the same
 *          sorted reduction and one read-back; SPH_ERR_STATE if it is zero.  The normalised normal used is written back in
 *          every case.
 * Table    sph_profile_finish (pure host code: no context, no device), table[b * SPH_PROFILE_NCOL + col] with
 *          mean(q) = (sum m q) / M and disp(q) = sqrt(v) for v = mean(q q) - mean(q)^2 >= 0, else 0:
 *           0 R_lo = edge[k]            1 R_hi = edge[k + 1]           2 R_mean = mean(R)           3 N
 *           4 M                         5 Sigma = M / area, area = (pi (R_hi R_hi - R_lo R_lo)) / n_phi
 *           6 z_mean = mean(z')         7 H = disp(z')                 8 vR_mean    9 vphi_mean    10 vz_mean
 *          11 sigma_R = disp(v_R)      12 sigma_phi = disp(v_phi)     13 sigma_z = disp(v_z)      14 u_mean
 *          15 c_s = sqrt((gamma gamma_m1) u_mean) (params; the reference's EOS)                    16 alpha_mean
 *          17 h_mean                   18 Omega = vphi_mean / R_mean
 *          19 kappa = sqrt(kappa2) over the ring-combined sums (sectors added in j order): R_k = mean(R), W_k = mean(v_phi)
 *             / R_k, f_k = ((R_k R_k)(R_k R_k))(W_k W_k), kappa2_k = ((f_b - f_a) / (R_b - R_a)) / ((R_k R_k) R_k) with
 *             (a, b) = (k - 1, k + 1) inside, (0, 1) and (n_r - 2, n_r - 1) at the ends; NaN with one ring or kappa2 < 0
 *          20 Q = (c_s kappa) / ((pi G) Sigma) (the sector's own Sigma and c_s)
 *          21 Mdot = -(((2 pi) R_mean) Sigma) vR_mean
 *          22 j = |L| / M, L = (sum m l), |L| = sqrt((Lx Lx + Ly Ly) + Lz Lz)
 *          23 tilt = atan2(sqrt(a1 a1 + a2 a2), a3) = the angle between L^ and n^, with L^ = L / |L|, a1 = L^.e1, a2 = L^.e2,
 *             a3 = L^.n^ (acos(a3) would lose accuracy for small tilts)      24 twist = atan2(a2, a1)
 *          25 ecc = |E| / M, E = (sum m e)        26 peri = atan2(E.e2, E.e1) (NaN where M == 0): periapsis longitude
 *          27 phi_lo = -pi + (2 pi j) / n_phi    28 phi_hi = -pi + (2 pi (j + 1)) / n_phi
 *          A quantity whose denominator is zero is NaN (0 / 0 in empty bins, a ring's missing neighbour for kappa); N, M and
 *          Sigma of an empty bin are 0.  The edges are recomputed from the descriptor (normal: the written-back one).
 * cost     host form: one read-back of the sums (plus one for AUTO_NORMAL); device form: sums only, ordered on the
 *          context's stream, no synchronisation (AUTO_NORMAL: one).  No state, statistic (other than device_bytes: the
 *          render's scratch), flag, grid, list or dt of the context changes.
 * SPH_ERR_ARG: null pointers, both outputs null, n_bins != n_r n_phi, n_r < 1, n_phi < 1, n_r n_phi > 2^20, r_min < 0,
 * r_min >= r_max, a non-finite r_min / r_max, LOG with r_min == 0, a zero or non-finite normal (without AUTO_NORMAL), a
 * non-finite centre (sink < 0), NaN z_max, sink < -1 or >= sph_sink_count, unknown flags, reserved != 0, rings so narrow
 * that two edges coincide.  SPH_ERR_NOMEM: the scratch does not fit. */
#define SPH_PROFILE_LOG          1   /* logarithmic ring edges (r_min > 0)                                    */
#define SPH_PROFILE_AUTO_NORMAL  2   /* normal = total angular momentum of the shell about the centre          */
#define SPH_PROFILE_NSUM  20         /* raw sums per bin                                                        */
#define SPH_PROFILE_NCOL  29         /* derived columns per bin                                                 */
typedef struct sph_profile_desc {
    double  centre[3], centre_v[3];  /* frame origin and velocity (ignored when sink >= 0)                      */
    double  central_mass;            /* for the eccentricity vector; <= 0: no eccentricity (zeros)              */
    double  normal[3];               /* disc normal, any length > 0; written back normalised                   */
    double  r_min, r_max;            /* ring range [r_min, r_max)                                               */
    double  z_max;                   /* strict |z'| < z_max; INFINITY = none                                    */
    int32_t n_r, n_phi;              /* rings >= 1, sectors per ring >= 1, n_r n_phi <= 2^20                    */
    int32_t sink;                    /* >= 0: centre, centre_v and central_mass are that sink's state; -1: none */
    int32_t flags;                   /* SPH_PROFILE_LOG | SPH_PROFILE_AUTO_NORMAL                               */
    int32_t reserved[2];             /* must be 0                                                               */
} sph_profile_desc;                  /* 128 bytes */
/* either output may be NULL, not both; table needs no sums output (they are read back in any case) */
int sph_profile(sph_ctx *ctx, sph_profile_desc *d, double *host_sums, double *host_table, int64_t n_bins);
int sph_profile_dev(sph_ctx *ctx, sph_profile_desc *d, double *d_sums, int64_t n_bins);
int sph_profile_finish(const sph_profile_desc *d, const sph_params *p, const double *sums, double *table, int64_t n_bins);

/* ---- conserved totals and the gravitational potential: energy, momentum and angular momentum of the gas and the
 *      sinks, with the Barnes-Hut gas self-potential and the sink potentials, and the potential of every particle -------
 * Particles the state as sph_download_field returns it, in every state of the context (after an upload, a drift, an
 *          sph_step with SPH_FLAG_ACCRETE_CULL, a cull).  Targets: the owned gas (original ids < n_owned), never ghosts;
 *          sinks: the context's sink arrays.  h_i = SPH_F_H with variable h, else params.h.  G = params.G.
 * Phi_sink,i = -sum_s G M_s / |r_i - R_s| in sink order, unsoftened as the sink accelerations are ([F]:559-591), with
 *          |d| = sqrt((dx dx + dy dy) + dz dz) and each term (G M_s) / |d|; massless sinks add 0.
 * Phi_self,i  0 without SPH_FLAG_SELF_GRAVITY (the energy of the equations the context integrates).  With it: the
 *          Barnes-Hut walk of the force (same acceptance test, theta, soft2 = 0.001 * 2.5 and target h) over the tree of the
 *          sources; an accepted node or leaf of mass m_j adds (G m_j / h_i) phi(q), s = sqrt(d.d + soft2), q = s / h_i, where
 *          phi is the potential of the cubic-spline softening whose mass fraction is the reference's grav_table polynomial
 *          ([F]:81-101), q^2 phi'(q) = that polynomial:
 *            q < 1:      phi = (2/3) q^2 - (3/10) q^4 + (1/10) q^5 - 7/5
 *            1 <= q < 2: phi = (4/3) q^2 - q^3 + (3/10) q^4 - (1/30) q^5 - 8/5 + 1 / (15 q)
 *            q >= 2:     phi = -1 / q
 *          evaluated analytically (the force interpolates its table; the two differ by O(dq^2)).  The target's own source is
 *          excluded by identity, not by distance: two distinct coincident particles see each other.  As in the force walk,
 *          a node smaller than theta sqrt(soft2) that contains the target can be accepted, its monopole then including the
 *          target.  With variable h, Phi_self,i uses h_i (as the force): W_self is a diagnostic, not an exact pair sum.
 * Sources  without sph_set_gravity_sources_dev: the owned gas records {x, y, z, m} in the caller's order and their exact
 *          bounding box; src_offset is ignored.  With external sources: those records and box, the tree sph_forces builds;
 *          the particle of original id k is source src_offset + k (its own source, for the exclusion).  Phi_self,i is a
 *          function of the source records in order, their box and the target's own record only: a single context and a
 *          set of contexts fed the same records and box through sph_set_gravity_sources_dev give bitwise the same values.
 * Sums     sums[0..SPH_ENERGY_NSUM), per gas particle terms in this order, without fused multiply-adds:
 *           0 N (count as a double)    1 M = sum m             2-4 sum m r            5-7 sum m v
 *           8-10 sum m (r x v) = m (y vz - z vy, z vx - x vz, x vy - y vx) about the origin
 *          11 K = sum (0.5 m) ((vx vx + vy vy) + vz vz)     12 U = sum m u
 *          13 W_self = sum (0.5 m) Phi_self,i               14 W_gs = sum m Phi_sink,i
 *          additive over contexts and ranks.  The sink part, on rank 0 only (sph_set_rank; 0 elsewhere), so that the whole
 *          array adds over ranks: 15 number of sinks  16 M_s  17-19 sum M R  20-22 sum M V  23-25 sum M (R x V)
 *          26 K_s = sum (0.5 M) V.V  27 W_ss = -sum_{s<t} (G (M_s M_t)) / |R_s - R_t| (pairs with M_s M_t == 0 add 0).
 *          Derived (capi.energy_total): E = K + U + W_self + W_gs + K_s + W_ss, P = [5-7] + [20-22], L = [8-10] + [23-25].
 * Order    the gas terms are reduced in the caller's particle order in a fixed shape: pieces of 1024 ids, each added by
 *          one 64-lane wavefront (lanes strided, then a xor butterfly), then the pieces by one wavefront.  Bitwise
 *          reproducible over calls, sorted orders, dense or hashed grids, and whether forces were just evaluated.  No
 *          float atomics.
 * phi      (optional) Phi_self,i + Phi_sink,i: n_phi == sph_count doubles in sph_download_field order, 0 for ghosts
 *          (e.g. the values of sph_render_field with SPH_RENDER_FIELD_VALUES).
 * cost     host form: one read-back (one more for the root box with self-gravity and no external sources); device form:
 *          ordered on the context's stream, synchronising only for that root box.  No state, field, statistic (other than
 *          device_bytes), dt, grid or list changes; a run that calls sph_energy after every step is bitwise the run
 *          without it.  With self-gravity and no external sources the tree is built into the context's tree arrays, so the
 *          next sph_forces builds its own tree again (one more tree build, the same results).
 * SPH_ERR_ARG: both outputs null, n_phi != sph_count with phi given, src_offset outside [0, n_src - n_owned] with external
 * sources.  An empty context returns zeros (and the sink part). */
#define SPH_ENERGY_NSUM 28
int sph_energy(sph_ctx *ctx, int64_t src_offset, double *host_sums, double *host_phi, int64_t n_phi);
int sph_energy_dev(sph_ctx *ctx, int64_t src_offset, double *d_sums, double *d_phi, int64_t n_phi);

/* ---- friends-of-friends groups: the clumps of the owned gas (which particles form them, how many there are, their
 *      mass, size, spin and bulk motion) -------------------------------------------------------------------------------
 * Select   the owned gas (original ids < n_owned; ghosts and sinks excluded, as the renders select) with rho >= rho_min
 *          (-INFINITY: every particle whose rho is not NaN) and clip_lo < x < clip_hi on every axis (strict; -INFINITY /
 *          +INFINITY: no cut; a non-finite position is never selected).  rho is the value sph_download_field(SPH_F_RHO)
 *          would return: SPH_ERR_STATE exactly when that call would refuse it.  One context's owned particles only: groups
 *          that cross ranks (dist.py, the native multi-GPU loop) are not joined.
 * Link     selected i and j are linked iff d2 < b * b, d2 = (dx dx + dy dy) + dz dz with dx = x_i - x_j (each product
 *          and sum rounded on its own, no fused multiply-adds).  b = link; with SPH_GROUPS_LINK_H b = link * max(h_i, h_j)
 *          (rounded once), h = SPH_F_H with variable h, else params.h.
 * Groups   the connected components of the links with >= min_members members; smaller components are dropped.  They
 *          are numbered 0 .. n_groups - 1 by N descending, ties by the smallest original id ascending: the partition is
 *          unique, so the numbering depends only on the positions, the selection and the descriptor.
 * Labels   (optional) int32 per particle in sph_download_field order, n_labels == sph_count: the group number, -1 for
 *          unselected particles, particles of dropped components and ghosts.
 * Table    (optional) table[g * SPH_GROUPS_NCOL + col] for the first min(n_groups, max_groups) groups; *n_groups
 *          receives the full count in every case.  Per member, in this order, without fused multiply-adds:
 *          first pass  m, m x, m y, m z, m vx, m vy, m vz, m u;
 *          second pass dr = r - R, dv = v - V, d2 = (dr_x dr_x + dr_y dr_y) + dr_z dr_z, m d2,
 *                      m (dr_y dv_z - dr_z dv_y), m (dr_z dv_x - dr_x dv_z), m (dr_x dv_y - dr_y dv_x),
 *                      (0.5 m) ((dv_x dv_x + dv_y dv_y) + dv_z dv_z), sqrt(d2) (max), rho (max).
 *           0 N (count, as a double)     1 M = sum m                  2-4 R = (sum m r) / M (each axis)
 *           5-7 V = (sum m v) / M        8 r_rms = sqrt((sum m d2) / M)            9 r_max = max sqrt(d2)
 *          10-12 spin S = sum m (dr x dv)                        13 K_int = sum (0.5 m) |dv|^2
 *          14 U = sum m u                15 rho_max                   16-18 position of the densest member
 *          19 original id of the densest member (the smallest id on ties)           20 smallest original id
 *          (M == 0: R, V and r_rms are NaN.)
 * Order    each group's members are sorted by original id and its sums reduced in a fixed shape: pieces of 1024 sorted
 *          positions counted from the group's start, each added by one 64-lane wavefront (lane l: positions l, l + 64,
 *          ... in turn, then a xor butterfly over the lanes), then the pieces by one wavefront in the same shape.  First
 *          pass N, M, sum m r, sum m v, sum m u; R and V from it on the device; second pass the moments about R and V.
 *          max and argmax are order-free.  No float atomics.  Labels and table are bitwise the same over repeated calls,
 *          over the context's sorted order and over dense or hashed grids.
 * cost     host form: one synchronisation, which copies out the count, the table rows and the labels.  Device form
 *          (labels, table and the int64 count in device memory): ordered on the context's stream, no synchronisation; a
 *          selected h <= 0 or non-finite under LINK_H then shows as *d_n_groups == -1 with every label -1.  No state,
 *          field, statistic (other than device_bytes: the render's scratch), flag, grid, list or dt of the context
 *          changes; a run that calls sph_groups after every step is bitwise the run without it.
 * SPH_ERR_ARG: null descriptor or count pointer, link <= 0 or non-finite, NaN rho_min or clip, min_members < 1, labels
 * given with n_labels != sph_count, max_groups < 0, a table with max_groups == 0, unknown flags, reserved != 0.
 * SPH_ERR_STATE: stale rho; under LINK_H params.h <= 0 (fixed h) or, host form, a selected h <= 0 or non-finite.  An empty
 * selection gives 0 groups. */
#define SPH_GROUPS_LINK_H  1         /* b = link * max(h_i, h_j)                                                 */
#define SPH_GROUPS_NCOL    21        /* table columns per group                                                  */
typedef struct sph_groups_desc {
    double  link;                    /* linking length (LINK_H: in units of h), finite, > 0                      */
    double  rho_min;                 /* rho >= rho_min; -INFINITY: no cut                                        */
    double  clip_lo[3], clip_hi[3];  /* strict particle clip box; -INFINITY / +INFINITY = none                   */
    int64_t min_members;             /* >= 1                                                                     */
    int32_t flags;                   /* SPH_GROUPS_LINK_H                                                        */
    int32_t reserved;                /* must be 0                                                                */
} sph_groups_desc;                   /* 80 bytes */
int sph_groups(sph_ctx *ctx, const sph_groups_desc *d, int32_t *host_labels, int64_t n_labels, double *host_table,
               int64_t max_groups, int64_t *n_groups);
int sph_groups_dev(sph_ctx *ctx, const sph_groups_desc *d, int32_t *d_labels, int64_t n_labels, double *d_table,
                   int64_t max_groups, int64_t *d_n_groups);

/* ---- density-peak clumps: the basins of the density field of the owned gas, merged across high saddles (a HOP /
 *      watershed finder: where friends-of-friends percolates through a disc, this separates a fragment from its arm) ------
 * Select   as sph_groups: the owned gas with rho >= rho_min strictly inside the clip box, finite positions; rho is what
 *          sph_download_field(SPH_F_RHO) returns (SPH_ERR_STATE when stale).  A non-finite rho is never selected.
 * Neighbours  selected i and j are neighbours iff sph_groups would link them: d2 < b * b, d2 = (dx dx + dy dy) + dz dz,
 *          no fused multiply-adds, b = link or, with SPH_PEAKS_LINK_H, link * max(h_i, h_j) (rounded once).  Symmetric.
 * Order    a is above b iff rho_a > rho_b, or rho_a == rho_b and id_a < id_b (original ids): a strict total order, so
 *          plateaus and ties need no special case.
 * Hop      next[i] = the highest of i and its neighbours; next[i] == i: a raw peak.  peak[i] = the end of i's chain
 *          (chains strictly ascend, so they end).  The particles of one peak are its basin.
 * Saddles  every neighbour pair (i, j) with peak[i] != peak[j] has the saddle value s = min(rho_i, rho_j); the edge
 *          {a, b} between two raw peaks carries S(a, b) = the maximum of s over all such pairs.
 * Merge    components start as single raw peaks; a component's top is its highest peak.  Edges are taken by S descending,
 *          ties by the key (min id << 32 | max id) ascending.  For an edge whose ends lie in different components A and
 *          B, top(A) above top(B): B joins A iff rho(top(B)) < contrast * S (the product rounded once).  contrast = 1
 *          never merges (S <= rho(top(B)) always): the raw basins.  contrast = +INFINITY merges every edge: the
 *          friends-of-friends components, labels and columns 0 .. 20 bitwise what sph_groups gives for the same link.
 * Drop, number  components whose top has rho < peak_min (-INFINITY: none) and components with fewer than min_members
 *          members are dropped; the rest are numbered by N descending, then the smallest original id ascending.
 * Labels   as sph_groups: int32 per particle in sph_download_field order, -1 for unselected, dropped and ghosts.
 * Table    table[g * SPH_PEAKS_NCOL + col]: columns 0 .. 20 are sph_groups' columns with the same per-member
 *          arithmetic, order rule and reduction shape; 21 S_out = the largest S over the edges whose ends lie in different
 *          final components (before dropping), 0 if there is none; 22 the number of raw peaks in the component.  Column 19
 *          (id of the densest member) is the component's top and column 15 its rho.
 * Counts   int64 counts[SPH_PEAKS_NCOUNT] = {n_groups, raw peaks of the selection, distinct peak-peak edges}.
 * Order    every decision is a comparison, S is an integer maximum over bit patterns and the table follows sph_groups'
 *          order rule: labels, counts and table are bitwise the same over repeated calls, over the context's sorted order
 *          and over dense or hashed grids.  No float atomics.
 * cost     the merge is a sequential union-find over the edge list (about n / 10 edges and n / 10 raw peaks in a disc),
 *          run on the host.  Both forms therefore wait for the stream three times: for the number of neighbour pairs
 *          that cross basins and of raw peaks (12 bytes; the pair buffer is sized from the first, the scratch grows
 *          and the pass starts again when it does not fit, so nothing is ever truncated), for the number of distinct
 *          edges (8 bytes), and for the sorted edge list and the peaks' rho (16 bytes per edge, 8 per peak), after
 *          which the top and S_out of every peak are uploaded (12 bytes per peak).  The host form copies counts, table
 *          rows and labels out in one more wait.  The device form (labels, table, counts in device memory) cannot
 *          promise zero synchronisations as sph_groups_dev does; a selected h <= 0 or non-finite under LINK_H shows
 *          there as counts[0] == -1 with every label -1.  No state, field, statistic (other than device_bytes: the
 *          render's scratch), flag, grid, list or dt of the context changes; a run that calls sph_peaks after every step
 *          is bitwise the run without it.
 * SPH_ERR_ARG: as sph_groups (null descriptor or counts, link <= 0 or non-finite, NaN rho_min or clip, min_members < 1,
 * labels with n_labels != sph_count, max_groups < 0, a table with max_groups == 0, unknown flags, reserved != 0), and
 * contrast < 1 or NaN, NaN peak_min.  SPH_ERR_STATE: as sph_groups.  An empty selection gives 0 groups. */
#define SPH_PEAKS_LINK_H   1         /* b = link * max(h_i, h_j)                                                 */
#define SPH_PEAKS_NCOL     23        /* table columns per group                                                  */
#define SPH_PEAKS_NCOUNT   3         /* n_groups, raw peaks, edges                                               */
typedef struct sph_peaks_desc {
    double  link;                    /* neighbour radius (LINK_H: in units of h), finite, > 0                    */
    double  rho_min;                 /* rho >= rho_min; -INFINITY: no cut                                        */
    double  peak_min;                /* components whose top has rho < peak_min are dropped; -INFINITY: none     */
    double  contrast;                /* >= 1; 1: raw basins, +INFINITY: friends-of-friends                       */
    double  clip_lo[3], clip_hi[3];  /* strict particle clip box; -INFINITY / +INFINITY = none                   */
    int64_t min_members;             /* >= 1                                                                     */
    int32_t flags;                   /* SPH_PEAKS_LINK_H                                                         */
    int32_t reserved;                /* must be 0                                                                */
} sph_peaks_desc;                    /* 96 bytes */
int sph_peaks(sph_ctx *ctx, const sph_peaks_desc *d, int32_t *host_labels, int64_t n_labels, double *host_table,
              int64_t max_groups, int64_t *counts);
int sph_peaks_dev(sph_ctx *ctx, const sph_peaks_desc *d, int32_t *d_labels, int64_t n_labels, double *d_table,
                  int64_t max_groups, int64_t *d_counts);

/* ---- SPH gradients: the gradient of up to four per-particle fields at every owned gas particle (vorticity, divergence,
 *      gradients of rho, u, P or any caller's array), in the standard difference form or the matrix-corrected form -------
 * Kernel   the renders' analytic cubic spline with the DOUBLE-precision pi (not the simulation's REAL(4)-pi table):
 *          W(r, h) = sigma w(q), q = r / h, sigma = 1 / (pi h^3), w = 1 - 1.5 q^2 + 0.75 q^3 (q <= 1), 0.25 (2 - q)^3
 *          (1 < q <= 2), 0 beyond; F(r, h) = -W'(r) / r = (sigma / h^2) f(q), f = 3 - 2.25 q (q <= 1), 0.75 (2 - q)^2 / q
 *          (1 < q <= 2), 0 beyond (finite at q = 0).
 * h        every target i gathers with its own h_i: desc.h when desc.h > 0, else each particle's own h (SPH_F_H on a
 *          variable-h context, params.h on a fixed-h one) -- the renders' h rule.
 * Targets  the owned gas (original ids < n_owned) with finite positions strictly inside clip_lo < x < clip_hi on every axis
 *          (-INFINITY / +INFINITY: no clip).
 * Sources  every gas slot with a finite position, owned AND ghost, no clip; sinks are neither.  A rank whose ghost layer
 *          covers 2 h of its targets gets the rows of the union to rounding.
 * Sums     for target i and every source j with d2 <= 4 h_i^2 (d2 = (dx dx + dy dy) + dz dz, x_ij = x_i - x_j):
 *          rho~_i = sum_j m_j W(r_ij, h_i) (j = i included: the SPH density of this kernel's gather),
 *          C_i = sum_j m_j F x_ij x_ij^T (symmetric, 6 sums), b_i^(k) = sum_j m_j F (A_i^(k) - A_j^(k)) x_ij per field k;
 *          j = i and coincident particles (d2 == 0) add nothing to C or b.  No fused multiply-adds.
 * Forms    standard (default): grad A_i = b_i / rho~_i (Monaghan's difference form).  SPH_GRAD_CORRECTED: grad A_i =
 *          adj(C_i) b_i / det C_i, exact for linear A on any particle set.  A target is singular in the corrected form when
 *          !(det C_i > 1e-6 (tr C_i / 3)^3) (fewer than three non-coplanar neighbours: an isolated particle, a planar set):
 *          its gradients are NaN, its rho~ is written, and it is counted.
 * Fields   fields[k], k < n_fields <= SPH_GRAD_MAX_FIELDS, all in one neighbour walk (velocity: three fields in one call):
 *          an SPH_F_* id, read as sph_download_field reads it (SPH_ERR_STATE exactly when that call would refuse the field
 *          as stale), or SPH_GRAD_VALUES: row k of values, values[k * n + id], n = sph_count, in sph_download_field order
 *          with ghosts -- host memory for sph_gradients, device memory for _dev.
 * Output   out[(3 k + a) n + id], a = x, y, z, n_out == 3 n_fields sph_count: every gradient component is a contiguous row
 *          in download order (render values for sph_render_field).  Rows of non-targets are NaN.  rho_out (optional,
 *          sph_count doubles, download order): rho~, NaN for non-targets.
 * Counts   host form: optional *n_targets and *n_singular; device form: optional int64 d_counts[2] (targets, singular).
 * Order    every target adds its sources over its stencil cells in increasing cell key and within a cell in increasing
 *          original id.  The cell edge E is a function of the source set and desc.h only (2 h (1 + 1e-6) with one h; with
 *          per-particle h, 2 h_ref (1 + 1e-6), h_ref the upper edge of the quarter octave holding the median source h), so a
 *          target's row depends only on the sources and the target: bitwise the same over repeated calls, the context's
 *          slot order (a fresh upload, or after sph_density re-sorts), dense or SPH_FLAG_HASHED_GRID grids, any clip box
 *          that contains the target, and an owned / ghost split of the same upload (sph_set_owned).  No float atomics.
 * cost     host form: one synchronisation, then the copies out.  Device form: ordered on the context's stream, no
 *          synchronisation; a bad target h shows as d_counts[0] == -1 with NaN rows.  No state, field, statistic (other than
 *          device_bytes: the render's scratch), flag, grid, list or dt of the context changes; a run that calls
 *          sph_gradients after every step is bitwise the run without it.
 * SPH_ERR_ARG: null descriptor or output, n_fields outside 1 .. SPH_GRAD_MAX_FIELDS, a bad field id, values missing while
 * a field is SPH_GRAD_VALUES or given while none is, n_out != 3 n_fields sph_count, h < 0 or NaN, a NaN clip, unknown
 * flags, reserved != 0.  SPH_ERR_STATE: a stale field; params.h <= 0 on a fixed-h context with desc.h == 0; host form, a
 * target h <= 0 or non-finite.  An empty target set gives 0 targets and all-NaN output. */
#define SPH_GRAD_CORRECTED   1       /* adj(C) b / det C                                                         */
#define SPH_GRAD_MAX_FIELDS  4
#define SPH_GRAD_VALUES    (-1)      /* fields[k]: row k of values                                               */
typedef struct sph_gradients_desc {
    double  clip_lo[3], clip_hi[3];        /* strict target clip box; -INFINITY / +INFINITY = none */
    double  h;                             /* > 0: one h for every target; 0: each particle's own h */
    int32_t fields[SPH_GRAD_MAX_FIELDS];   /* SPH_F_* or SPH_GRAD_VALUES (row k of values)          */
    int32_t n_fields;                      /* 1 .. SPH_GRAD_MAX_FIELDS                              */
    int32_t flags;                         /* SPH_GRAD_CORRECTED                                    */
    int32_t reserved[2];                   /* must be 0                                             */
} sph_gradients_desc;                      /* 88 bytes */
int sph_gradients(sph_ctx *ctx, const sph_gradients_desc *d, const double *values, double *host_out, int64_t n_out,
                  double *host_rho, int64_t *n_targets, int64_t *n_singular);
int sph_gradients_dev(sph_ctx *ctx, const sph_gradients_desc *d, const double *d_values, double *d_out, int64_t n_out,
                      double *d_rho, int64_t *d_counts);

/* ---- SPH interpolation at arbitrary points: density, any field, or the caller's values at points that move independently
 *      of the gas (an unwrapped (R, phi) map, an (R, z) cut, an inclined plane, a probe line, tracers) -------------------
 * Sources  exactly the renders' selection: the context's owned gas particles (original ids < n_owned; ghosts and sinks
 *          never) with a finite position strictly inside clip_lo < x < clip_hi on every axis (-INFINITY / +INFINITY: no
 *          clip).  Partial results of ranks or contexts therefore add: summing num and den over ranks and dividing gives
 *          the union's normalised value, as sph_render_field documents for images.
 * h        the renders' rule: desc.h when desc.h > 0, else each particle's own h (SPH_F_H on a variable-h context, params.h
 *          on a fixed-h one).  The points have no h: this is the scatter form, every source spreads with its own h_j.
 * Sums     the renders' kernel, weights and term arithmetic, without fused multiply-adds: s_j = 1 / (pi h_j^3) with the
 *          DOUBLE-precision pi, ws_j = m_j s_j (SPH_RENDER_WEIGHT_MASS) or (m_j / rho_j) s_j (SPH_RENDER_WEIGHT_VOLUME; rho
 *          as sph_download_field(SPH_F_RHO) returns it, SPH_ERR_STATE exactly when that call would refuse),
 *          q = sqrt((dx dx + dy dy) + dz dz) * (1 / h_j) with dx = p_x - x_j, Wn = 1 - 1.5 q^2 + 0.75 q^3 (q <= 1),
 *          0.25 (2 - q)^3 (1 < q <= 2); den(p) = sum ws_j Wn, num_k(p) = sum (ws_j A_j^(k)) Wn.  A source contributes iff
 *          q <= 2.  A point farther than 2 h_j from every source gets den, num and the normalised value exactly 0.0.
 * Fields   fields[k], k < n_fields <= SPH_SAMPLE_MAX_FIELDS, all in one walk: an SPH_F_* id read as sph_download_field
 *          reads it (SPH_ERR_STATE when stale), or SPH_SAMPLE_VALUES: row k of values, values[k * n + id], n = sph_count,
 *          in sph_download_field order -- host memory for sph_sample, device memory for _dev.  Only the sources' entries
 *          are read.
 * Points   three arrays of n_points doubles (struct of arrays, as sph_upload), host memory for sph_sample, device memory
 *          for _dev.  0 <= n_points <= 2^31 - 1; n_points == 0 succeeds and writes no row (counts, if given: 0, 0).  A
 *          point with a non-finite coordinate gets NaN in every output row and is counted.
 * Output   out[k * n_points + p] = num_k(p), or with SPH_SAMPLE_NORMALISE num_k(p) / den(p) (exactly 0.0 where den == 0.0);
 *          n_out == n_fields * n_points.  weight (optional unless n_fields == 0): den(p), n_points doubles; with the MASS
 *          weight and n_fields == 0 this is the SPH density at the points.  counts (optional, 2 x int64): the points with
 *          den != 0, the points with a non-finite coordinate.
 * Order    the search structure is a function of the source set and the descriptor only, never of the points.  The
 *          sources are binned by LEVELS of h: with one h there is one level; with per-particle h a level is an aligned
 *          group of 2^g quarter octaves of h (half octaves, g = 1, unless more than 64 such groups are occupied: g then
 *          grows until at most 64 are), level l with upper edge H_l in cells of edge 2 H_l (1 + 1e-6) over the source box
 *          (enlarged where an axis would need more than 2^19 - 8 cells).  Every point adds its sources level by level in
 *          ascending h, within a level over the <= 27 cells around it in ascending cell key (x slowest), within a cell in
 *          ascending original id.  A point's values are therefore bitwise the same over repeated calls, any order or
 *          subset of the points (one point alone included), the context's slot order (a fresh upload, or after
 *          sph_density re-sorts), dense or SPH_FLAG_HASHED_GRID grids, and the host and device forms.  No float atomics.
 * cost     host form: the copies in, one synchronisation, the copies out.  Device form: ordered on the context's stream,
 *          no synchronisation; a source with h <= 0 or a non-finite h shows as d_counts[0] == -1 and NaN outputs (host
 *          form: SPH_ERR_STATE).  No state, field, statistic (other than device_bytes: the render's scratch), flag, grid,
 *          list or dt of the context changes; a run that samples after every step is bitwise the run without it.
 * SPH_ERR_ARG: null descriptor, null point arrays with n_points > 0, n_points out of range, n_fields outside 0 ..
 * SPH_SAMPLE_MAX_FIELDS, a bad field id, values missing while a field is SPH_SAMPLE_VALUES or given while none is,
 * n_out != n_fields n_points, null out with n_fields > 0, null weight with n_fields == 0, weight not MASS / VOLUME, unknown
 * flags, reserved != 0, h < 0 or NaN, a NaN clip; nothing is written then.  SPH_ERR_STATE: a stale field or rho; params.h <= 0
 * on a fixed-h context with desc.h == 0; host form, a source h <= 0 or non-finite.  SPH_ERR_NOMEM: the scratch does not fit.
 * An empty source set gives all-zero outputs, not an error. */
#define SPH_SAMPLE_NORMALISE   1        /* out = num / den (0 where den == 0)                                        */
#define SPH_SAMPLE_MAX_FIELDS  4
#define SPH_SAMPLE_VALUES    (-1)       /* fields[k]: row k of values                                                */
typedef struct sph_sample_desc {
    double  clip_lo[3], clip_hi[3];          /* strict SOURCE clip box; -INFINITY / +INFINITY = none              */
    double  h;                               /* > 0: one h for every source; 0: each particle's own h             */
    int32_t fields[SPH_SAMPLE_MAX_FIELDS];   /* SPH_F_* or SPH_SAMPLE_VALUES (row k of values)                    */
    int32_t n_fields;                        /* 0 .. SPH_SAMPLE_MAX_FIELDS; 0: the weight alone (weight required) */
    int32_t weight;                          /* SPH_RENDER_WEIGHT_MASS / SPH_RENDER_WEIGHT_VOLUME                 */
    int32_t flags;                           /* SPH_SAMPLE_NORMALISE                                              */
    int32_t reserved;                        /* must be 0                                                         */
} sph_sample_desc;                           /* 88 bytes */
int sph_sample(sph_ctx *ctx, const sph_sample_desc *d, int64_t n_points, const double *px, const double *py, const double *pz,
               const double *values, double *host_out, int64_t n_out, double *host_weight, int64_t *counts);
int sph_sample_dev(sph_ctx *ctx, const sph_sample_desc *d, int64_t n_points, const double *d_px, const double *d_py,
                   const double *d_pz, const double *d_values, double *d_out, int64_t n_out, double *d_weight, int64_t *d_counts);

/* ---- field lines of an SPH-interpolated vector field: streamlines of the gas velocity (in the inertial frame or one that
 *      rotates with a sink), of g, of the vorticity, ... -- n_seeds lines of n_steps classical RK4 steps each through the
 *      FROZEN field, in one kernel after one build of sph_sample's search structure ---------------------------------------
 * Field    at a point q, w_k(q) (k = 0, 1, 2) is exactly what sph_sample returns there with SPH_SAMPLE_NORMALISE for
 *          fields[k] with this descriptor's weight, h and clip: num_k(q) / den(q) in sph_sample's order rule (level, cell
 *          key, original id), same kernel, same arithmetic; 0.0 where den == 0.  fields[k] is an SPH_F_* id or
 *          SPH_TRACE_VALUES: row k of values, values[k * n + id] (n = sph_count, sph_download_field order; host memory for
 *          sph_trace, device memory for _dev).  Then, without fused multiply-adds and in this order:
 *            t = q - centre;  f = (om_y t_z - om_z t_y, om_z t_x - om_x t_z, om_x t_y - om_y t_x);  v = w - f;
 *            SPH_TRACE_PLANAR:     d = (v_x n_x + v_y n_y) + v_z n_z;  v_a = v_a - d n_a, with n = normal / |normal| and
 *                                  |normal| = sqrt((n_x n_x + n_y n_y) + n_z n_z), formed once on the host;
 *            SPH_TRACE_ARCLENGTH:  sp = sqrt((v_x v_x + v_y v_y) + v_z v_z);  v_a = v_a / sp.
 * Step     hs = 0.5 * ds and s6 = ds / 6.0, formed once on the host.  k1 = v(p), k2 = v(p + hs k1), k3 = v(p + hs k2),
 *          k4 = v(p + ds k3), p' = p + s6 ((k1 + 2 k2) + (2 k3 + k4)), per component, every product rounded before it is
 *          added.  ds is a time, or with SPH_TRACE_ARCLENGTH a length; ds < 0 traces upstream.
 * Stops    status per seed.  SPH_TRACE_NONFINITE: the seed has a non-finite coordinate; all its rows are NaN, row 0 included,
 *          n_done = 0.  SPH_TRACE_LEFT_BOX: a vertex is not strictly inside box_lo < p < box_hi on every axis (so a vertex
 *          that became non-finite also ends here); the seed itself: n_done = 0; a new vertex: it is recorded if its index is
 *          a multiple of stride, then the line stops.  SPH_TRACE_LEFT_GAS: den == 0 at one of the four stage points (no
 *          source reaches it); the step is not taken and the line ends at its last vertex.  SPH_TRACE_STAGNANT
 *          (SPH_TRACE_ARCLENGTH only): sp == 0 or not finite at a stage, in the same way.  SPH_TRACE_DONE: n_steps taken.
 *          n_done: the steps completed.  An empty source set makes every finite seed inside the box SPH_TRACE_LEFT_GAS.
 * Output   n_rec = n_steps / stride; path[(r * 3 + a) * n_seeds + p] is coordinate a of vertex r * stride of line p, r = 0 ..
 *          n_rec; row 0 is the seed; rows after the line's last vertex are NaN.  n_path == 3 (n_rec + 1) n_seeds.
 *          carry_out[r * n_seeds + p] (iff carry != SPH_TRACE_NONE): sph_sample's normalised value of the field `carry`
 *          (an SPH_F_* id, or SPH_TRACE_VALUES: row 3 of values) at every recorded vertex, 0.0 where den == 0; NaN in the rows
 *          path has NaN in.  counts (optional, 5 x int64): the seeds per status code.
 * Order    a line depends on the sources, the descriptor and its own seed only: bitwise the same over repeated calls, any
 *          order or subset of the seeds (one seed alone included), the context's slot order, dense or SPH_FLAG_HASHED_GRID
 *          grids, and the host and device forms.  The seeds are sorted by cell for the work distribution only.  No float
 *          atomics.
 * cost     sph_sample's: the host form has one synchronisation, the device form none (ordered on the context's stream); a
 *          source with h <= 0 or a non-finite h shows as d_counts[0] == -1 (the other four 0) with NaN paths, status
 *          SPH_TRACE_NONFINITE and n_done 0 in the device form, as SPH_ERR_STATE in the host form.  No state of the
 *          context changes (device_bytes may grow: the analysis scratch).
 * SPH_ERR_ARG, nothing written: null descriptor; null seed arrays with n_seeds > 0; n_seeds outside 0 .. 2^31 - 1; ds zero
 * or non-finite; n_steps outside 1 .. 65535; stride < 1 or not dividing n_steps; a bad field or carry id; values given with no
 * SPH_TRACE_VALUES id or missing while one is used; n_path != 3 (n_rec + 1) n_seeds; null path, status or n_done; carry_out
 * present without a carry or missing with one; unknown flags; reserved != 0; SPH_TRACE_PLANAR with a zero or non-finite
 * normal; a non-finite omega or centre; a NaN in either box; h < 0 or NaN; a bad weight.  SPH_ERR_STATE, SPH_ERR_NOMEM: as
 * sph_sample.  n_seeds == 0 succeeds (counts, if given: zeros). */
#define SPH_TRACE_ARCLENGTH  1   /* step along v / |v| by ds (a length) instead of along v by ds (a time) */
#define SPH_TRACE_PLANAR     2   /* remove v's component along desc.normal before it is used              */
#define SPH_TRACE_VALUES   (-1)  /* fields[k] / carry: row k (carry: row 3) of values, values[k * n + id]  */
#define SPH_TRACE_NONE     (-2)  /* carry: nothing carried                                                */
enum { SPH_TRACE_DONE = 0, SPH_TRACE_LEFT_GAS = 1, SPH_TRACE_LEFT_BOX = 2, SPH_TRACE_STAGNANT = 3, SPH_TRACE_NONFINITE = 4 };
typedef struct sph_trace_desc {
    double  clip_lo[3], clip_hi[3];   /* SOURCE clip box, sph_sample's                                   */
    double  h;                        /* sph_sample's h rule                                             */
    double  box_lo[3], box_hi[3];     /* tracers stop outside lo < p < hi; -/+INFINITY: none             */
    double  ds;                       /* finite, != 0; < 0 traces upstream                               */
    double  omega[3], centre[3];      /* frame: v - omega x (p - centre); zeros: the inertial frame      */
    double  normal[3];                /* SPH_TRACE_PLANAR: any non-zero vector (normalised on the host)  */
    int32_t fields[3];                /* the vector's components: SPH_F_* or SPH_TRACE_VALUES            */
    int32_t carry;                    /* a scalar sampled at every recorded vertex, or SPH_TRACE_NONE    */
    int32_t weight;                   /* SPH_RENDER_WEIGHT_MASS / _VOLUME                                */
    int32_t n_steps;                  /* 1 .. 65535                                                      */
    int32_t stride;                   /* >= 1, divides n_steps: every stride-th vertex is recorded       */
    int32_t flags;                    /* SPH_TRACE_ARCLENGTH | SPH_TRACE_PLANAR                          */
    int32_t reserved[2];              /* must be 0                                                       */
} sph_trace_desc;                     /* 224 bytes */
int sph_trace(sph_ctx *ctx, const sph_trace_desc *d, int64_t n_seeds, const double *sx, const double *sy, const double *sz,
              const double *values, double *host_path, int64_t n_path, double *host_carry, int32_t *host_status,
              int32_t *host_n_done, int64_t *counts);
int sph_trace_dev(sph_ctx *ctx, const sph_trace_desc *d, int64_t n_seeds, const double *d_sx, const double *d_sy,
                  const double *d_sz, const double *d_values, double *d_path, int64_t n_path, double *d_carry, int32_t *d_status,
                  int32_t *d_n_done, int64_t *d_counts);

/* ---- gravitational potential and acceleration at arbitrary points: the Barnes-Hut field of the gas and the field of the
 *      sinks where no particle is (a rotation curve, a potential map, torque maps, the tidal field at a candidate sink
 *      position, tracers) ------------------------------------------------------------------------------------------------
 * Sources  sph_energy's rule.  Without sph_set_gravity_sources_dev: the owned gas records {x, y, z, m} in the caller's order
 *          and their exact bounding box, in every state of the context (after an upload, a drift, a cull); ghosts never.
 *          With external sources: those records and box, the tree sph_forces builds.  The gas part is computed whether or
 *          not SPH_FLAG_SELF_GRAVITY is set.  theta = params.theta, G = params.G.  The fields of contexts with disjoint
 *          source sets add (up to the Barnes-Hut approximation); with external sources every rank holds the whole field.
 * Points   three arrays of n_points doubles, and optionally ph, n_points softening lengths -- host memory for
 *          sph_gravity_at, device memory for _dev.  h_p = ph[p], else desc.h when desc.h > 0, else params.h (fixed-h
 *          contexts only).  A point may lie anywhere, far outside the source box included.  Points are not sources: nothing
 *          is excluded, and a point placed on particle i sees particle i.
 * Gas      (SPH_GRAVAT_GAS) the walk of the force over the tree of the sources.  For an accepted node or leaf of mass m at c,
 *          with d = p - c: d2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, soft2))), the force walk's softened squared distance
 *          and its acceptance test on it; s = sqrt(d2), q = s / h_p;
 *            q < 2:   Phi += (G m / h_p) phi(q),   a -= ((G m / h_p^3) gamma(q)) d
 *            q >= 2:  Phi -= (G m) (1 / s),        a -= ((G m) (1 / s)^3) d
 *          phi is sph_energy's softening potential and gamma(q) = M(q) / q^3 the force's mass-fraction polynomial
 *          ([F]:81-101) divided by q^3 analytically (q phi'(q) = gamma(q) q^2):
 *            q < 1:      gamma = 4/3 - (6/5) q^2 + (1/2) q^3
 *            1 <= q < 2: gamma = 8/3 - 3 q + (6/5) q^2 - (1/6) q^3 - 1 / (15 q^3)
 *          Both are finite at s = 0: a point exactly on a source with soft2 = 0 gets -1.4 G m / h_p and no pull from it.
 *          The force interpolates its table of M(q) linearly; this call is analytic (they differ by O(dq^2) inside 2 h).
 * Sinks    (SPH_GRAVAT_SINKS) in sink order, unsoftened as sink_gravforces ([F]:559-591), without fused multiply-adds:
 *          d = p - R_s, |d| = sqrt((dx dx + dy dy) + dz dz), Phi -= (G M_s) / |d|, a -= ((G M_s) / ((|d| |d|) |d|)) d.  A
 *          massless sink adds 0.  A point on a massive sink gets Phi = -INFINITY and a = NaN; that is not an error.
 * Output   out[c * n_points + p], c = 0 Phi, 1..3 a, of the sum of the selected parts (gas + sinks, in that order, as
 *          sph_energy's phi); n_out == 4 n_points.  With SPH_GRAVAT_SPLIT (needs both parts) rows 0-3 are the gas and rows
 *          4-7 the sinks; n_out == 8 n_points.  counts (optional, 2 x int64): the points with a non-finite coordinate, the
 *          points whose softening length is <= 0 or non-finite; both kinds get NaN in every row.  n_points == 0 succeeds
 *          and writes no row.  An empty source set gives zeros for the gas part.
 * Order    a point's rows are a function of the source records in order with their box, the sinks, and the point's own
 *          {x, y, z, h} only: every lane of the walk adds exactly its own walk's contributions in its own walk's order,
 *          and the per-lane arithmetic does not depend on the other lanes.  The rows are bitwise the same over repeated
 *          calls, any order or subset of the points (one point alone included), the context's slot order, dense or
 *          SPH_FLAG_HASHED_GRID grids, the host and device forms, and a single context versus a context fed the same records
 *          and box through sph_set_gravity_sources_dev.  (The points are walked in the order of their 63-bit path keys in
 *          the tree's root box; that is a matter of speed only.)  No float atomics.
 * cost     sph_energy's.  Without external sources the tree is built into the context's tree arrays at every call (one
 *          read-back for the root box), so the next sph_forces builds its own tree again, with the same results; with
 *          external sources the tree in place is used, or built.  Host form: the copies in, that read-back, the copies out;
 *          a bad softening length is SPH_ERR_STATE (the rows are written).  Device form: ordered on the context's stream.
 *          No state, field, statistic (other than device_bytes), dt, grid or list changes; a run that calls it between the
 *          steps is bitwise the run without it.
 * SPH_ERR_ARG: null descriptor, null point arrays with n_points > 0, n_points outside 0 .. 2^31 - 1, n_out != 4 (8 with
 * SPLIT) n_points, null out with n_points > 0, no part selected, SPLIT without both parts, unknown flags, reserved != 0, h < 0
 * or NaN, soft2 < 0 or NaN, h == 0 without ph on a variable-h context; nothing is written then.  SPH_ERR_STATE: params.h <= 0
 * with h == 0 and no ph on a fixed-h context; host form, a point's softening length <= 0 or non-finite.  SPH_ERR_NOMEM: the
 * scratch does not fit. */
#define SPH_GRAVAT_GAS    1   /* the Barnes-Hut field of the gas sources                       */
#define SPH_GRAVAT_SINKS  2   /* the sinks' field, unsoftened as sink_gravforces ([F]:559-591) */
#define SPH_GRAVAT_SPLIT  4   /* 8 output rows: gas (phi, ax, ay, az), then sinks; needs both parts */
typedef struct sph_gravity_at_desc {
    double  h;            /* > 0: softening length of every point; 0: params.h (fixed-h contexts only); unused with ph */
    double  soft2;        /* >= 0, added to d.d as the force walk does; 0.001 * 2.5 is the force's value */
    int32_t flags;        /* SPH_GRAVAT_*; at least one of GAS, SINKS */
    int32_t reserved[3];  /* must be 0 */
} sph_gravity_at_desc;    /* 32 bytes */
int sph_gravity_at(sph_ctx *ctx, const sph_gravity_at_desc *d, int64_t n_points, const double *px, const double *py,
                   const double *pz, const double *ph, double *host_out, int64_t n_out, int64_t *counts);
int sph_gravity_at_dev(sph_ctx *ctx, const sph_gravity_at_desc *d, int64_t n_points, const double *d_px, const double *d_py,
                       const double *d_pz, const double *d_ph, double *d_out, int64_t n_out, int64_t *d_counts);

/* ---- binding energies and unbinding of clumps: is a group gravitationally bound, and which of its members form the
 *      bound core -- the group's OWN softened potential by a direct pair sum, the members' energies in the group's frame,
 *      and the iterated removal of the unbound members ------------------------------------------------------------------
 * labels   one int32 per particle in sph_download_field order, n_labels == sph_count: what sph_groups writes, or any
 *          partition of the caller's (the call does not depend on friends-of-friends).  Host memory for sph_bound, device
 *          memory for _dev.
 * Members  of group g, 0 <= g < n_groups: the owned gas particles (original id < n_owned) with a finite position and
 *          label g.  Every other label value means "in no group".  Ghosts and sinks are never members.  One context's
 *          owned particles only, as sph_groups.
 * h        the renders' rule: desc.h when desc.h > 0, else each particle's own h (SPH_F_H on a variable-h context,
 *          params.h on a fixed-h one).  G = params.G.  f = 1 with SPH_BOUND_THERMAL, else 0.
 * One evaluation of a member set S of group g, without fused multiply-adds:
 *          M = sum m, V = (sum m v) / M per axis.
 *          Phi_i = sum_{j in S, j != i} ((G m_j) (1 / h_i)) phi(q), d = r_i - r_j, d2 = ((dx dx + dy dy) + dz dz) + soft2,
 *          s = d2 rs with rs = 1 / sqrt(d2) to rounding (s = 0 where d2 == 0), q = s (1 / h_i); phi is sph_energy's
 *          softening potential, evaluated analytically in Horner form, its 1 / q taken as h_i rs.  j != i is decided by
 *          identity, never by distance: two distinct coincident members see each other, and phi(0) = -1.4 is finite.
 *          d2 must not overflow.
 *          k_i = 0.5 ((dvx dvx + dvy dvy) + dvz dvz), dv = v_i - V;  e_i = (k_i + u_i) + Phi_i (THERMAL) or k_i + Phi_i.
 *          The set's sums: K = sum (0.5 m) |dv|^2, U = sum m u, W = sum (0.5 m) Phi, sum m r.
 * Rounds   S_0 is the group, S_{r+1} = { i in S_r : e_i < 0 } (a NaN e_i is not < 0).  S_0, S_1, ... are evaluated, and
 *          the group stops after the evaluation of S_R with the first of these that holds:
 *          status 0  S_{R+1} == S_R: converged;
 *          status 1  R == max_rounds: no further removal is allowed (max_rounds == 0 evaluates once and removes nothing);
 *          status 2  |S_{R+1}| < min_members: dissolved.  Also N_0 < min_members (empty groups included): R = 0 and
 *                    nothing is evaluated.
 *          A group with N_0 > max_members is status 3: never evaluated, its row is NaN apart from N_0 and the status, its
 *          labels are -1, and it is counted.  Every evaluation is complete: Phi is recomputed over the current set, never
 *          decremented, so a value depends on the set alone, not on the path to it.
 * Order    a group's members are taken in ascending original id.  Phi_i is one accumulation chain over the members of
 *          S_0 in that order, in which a removed member and i itself add nothing.  The set sums run over the sorted
 *          positions of S_0 (a removed member adds nothing) in the fixed shape of sph_groups: pieces of 1024 sorted
 *          positions counted from the group's start, each added by one 64-lane wavefront (lane l: positions l, l + 64, ...
 *          in turn, then a xor butterfly over the lanes), then the pieces by one wavefront in the same shape.  The minimum
 *          and its member are order-free.  No float atomics.  A group's row and its members' outputs are a function of
 *          that group's id-sorted member records and the descriptor only: bitwise the same over repeated calls, the
 *          context's slot order, dense or hashed grids, the host and device forms, and whatever other groups the labels
 *          hold.  Removed members are masked (zero-mass sources), not compacted away.
 * Outputs  all optional, at least one given.
 *          bound_labels[id] (sph_count int32): g if the member is in the last evaluated set of g, e_i < 0 and g ended with
 *          status 0 or 1; else -1 (a dissolved group has no bound member).
 *          out[0 * n + id] = e_i, out[1 * n + id] = Phi_i, n = sph_count, n_out == 2 n: from the last evaluation that
 *          included the member, so a removed member keeps the e_i >= 0 that removed it; NaN for non-members and for the
 *          members of groups that were never evaluated.
 *          table[g * SPH_BOUND_NCOL + c], n_groups rows:
 *           0 N_0   1 M_0   2 K_0   3 U_0   4 W_0   5 E_0 = (K_0 + f U_0) + W_0   6 (K_0 + f U_0) / |W_0|       (of S_0)
 *           7 N_R   8 M_R   9-11 R_R = (sum m r) / M   12-14 V_R   15 K_R   16 U_R   17 W_R   18 E_R   (of the last set)
 *          19 members of S_R with e < 0      20 R      21 status
 *          22 original id of the most bound member of S_R (the smallest e, the smallest id on ties; -1 if none)  23 its e
 *          Dissolved groups: columns 7, 8 and 19 are 0, 9-18 and 23 NaN, 22 is -1; 0-6 stay those of S_0 where S_0 was
 *          evaluated (NaN apart from N_0 where it was not).
 *          counts[4] (int64): members, groups skipped over the cap, groups dissolved, groups stopped at max_rounds.
 * cost     sum over rounds and groups of N_0 N_r pair terms (a removed member is still streamed as a source, but no
 *          longer a target; where the removed members lie scattered over the 64-lane target tiles, N_0^2 a round), so
 *          max_members is a cost decision.  Device form: ordered on the context's stream, never
 *          synchronises; min(max_rounds, min(n_owned, max_members) - 1) + 1 rounds of six launches are enqueued, whose
 *          grids n_groups and the slot count bound from the host; the per-round work list is built on the device and the
 *          launches of a round in which no group is active leave at once.  Host form: reads one "groups still active"
 *          count per round and stops enqueueing at 0, then one synchronisation for the copies out.  A member with h <= 0
 *          or a non-finite h (per-particle h only): device form d_counts[0] == -1, every row NaN, every label -1; host form
 *          SPH_ERR_STATE.  The scratch is the render's.  No state, field, statistic (other than device_bytes), flag, grid,
 *          list or dt of the context changes; a run that calls sph_bound after every step is bitwise the run without it.
 *          Works in every state of the context (after an upload, a step, a cull); rho is not needed.
 * SPH_ERR_ARG: null descriptor or labels, no output, n_labels != sph_count, n_out != 2 sph_count with out given, n_groups
 * outside 0 .. 2^31 - 1, min_members < 1, max_members < 1, max_rounds < 0, h < 0 or NaN, soft2 < 0 or NaN, unknown flags,
 * reserved != 0; nothing is written then.  SPH_ERR_STATE: params.h <= 0 with h == 0 on a fixed-h context; host form, a
 * member with h <= 0 or a non-finite h.  SPH_ERR_NOMEM: the scratch does not fit.  n_groups == 0, an empty context or all
 * labels -1 succeed with zero members. */
#define SPH_BOUND_THERMAL  1     /* e_i includes u_i */
#define SPH_BOUND_NCOL    24     /* table columns per group */
typedef struct sph_bound_desc {
    double  h;            /* > 0: one softening length for every member; 0: each particle's own h (SPH_F_H / params.h) */
    double  soft2;        /* >= 0, added to d.d; 0.001 * 2.5 is the force's value */
    int64_t min_members;  /* >= 1: a set that falls below it dissolves */
    int64_t max_members;  /* >= 1: groups with more initial members are skipped (cost cap) */
    int32_t max_rounds;   /* >= 0: removals allowed; 0 = evaluate once, remove nothing */
    int32_t flags;        /* SPH_BOUND_THERMAL */
    int32_t reserved[2];  /* must be 0 */
} sph_bound_desc;         /* 48 bytes */
int sph_bound(sph_ctx *ctx, const sph_bound_desc *d, const int32_t *labels, int64_t n_labels, int64_t n_groups,
              int32_t *bound_labels, double *host_out, int64_t n_out, double *host_table, int64_t *counts);
int sph_bound_dev(sph_ctx *ctx, const sph_bound_desc *d, const int32_t *d_labels, int64_t n_labels, int64_t n_groups,
                  int32_t *d_bound_labels, double *d_out, int64_t n_out, double *d_table, int64_t *d_counts);

/* ---- spectral cubes: the optically thin position-position-velocity cube of the owned gas seen along any direction
 *      (channel maps, position-velocity diagrams, line profiles; moments with summersph_amd/cube.py) ------------------
 * Frame    rot[9], row-major: the rows are the image axes u^, v^ and the line of sight w^ (orthonormal and right-handed
 *          within 1e-12, else SPH_ERR_ARG).  P_j = rot (r_j - centre), every row evaluated in the fixed order
 *          ((a0 dx + a1 dy) + a2 dz) with no fused multiply-adds; V_j = w^ . (v_j - v_ref) in the same order.  w^ points
 *          away from the observer: V > 0 is receding.
 * Select   as sph_render_density: the owned gas particles (ghosts and sinks never) with clip_lo < r < clip_hi on every
 *          axis of the SIMULATION frame (strict; -INFINITY / +INFINITY: no clip).  h > 0: one h for every particle; 0:
 *          each particle's own h (SPH_F_H on a variable-h context, params.h on a fixed-h one).
 * Nodes    node i on image axis a is lo[a] + i (hi[a] - lo[a]) / (n - 1), the last one exactly hi[a] (np.linspace);
 *          n == 1: the single node lo[a].  Nodes are point-sampled, as in the renders.
 * Footprint  the renders' cubic spline integrated along the line of sight analytically:
 *          Y_j(b) = m_j A_j F(b / h_j) / (pi h_j^2), pi in double precision; A_j = values[id] (sph_count doubles in
 *          sph_download_field's order; host memory for sph_cube, device memory for _dev) or 1 without values.
 *          With p = b / h, r(t) = sqrt(p^2 + t^2), L(t) = p^2 ln(t + r) (0 at p == 0):
 *            I1 = (t r + L) / 2,  I2 = p^2 t + t^3 / 3,  I3 = t r^3 / 4 + 3 p^2 t r / 8 + 3 p^2 L / 8
 *            G_in(t) = t - 1.5 I2 + 0.75 I3,  G_out(t) = 2 t - 3 I1 + 1.5 I2 - 0.25 I3,  t1 = sqrt(1 - p^2), t2 = sqrt(4 - p^2)
 *            F = 2 [G_in(t1) - G_in(0) + G_out(t2) - G_out(t1)]  (p < 1),  2 [G_out(t2) - G_out(0)]  (1 <= p < 2),  0  (p >= 2)
 *          F(0) = 1.5 and the integral of F 2 p dp is 1: a particle's footprint integrates to its m A.
 * Line     sigma_j = sqrt((sigma_scale c_j)^2 + sigma_floor^2), c_j the context's SPH_F_C (SPH_ERR_STATE exactly when
 *          sph_download_field(SPH_F_C) would refuse, unless sigma_scale == 0).  Channel edges e_k = (k - 0.5) dv + v0,
 *          k = 0 .. n_chan: channel k is centred on v0 + k dv.  With x = (e - V_j) / sigma_j:
 *          cdf(x) = erf(x / sqrt 2) / 2 for |x| < 8.5 and exactly -1/2, +1/2 beyond (the truncation is part of the
 *          definition: a particle's far channels get an exact +0.0 and are skipped).  sigma_j == 0: the particle goes into
 *          the one channel with e_k <= V_j < e_{k+1}.
 * Output   voxel[k][iu][iv] = sum_j Y_j(|node - P_j,uv|) (cdf_j(e_{k+1}) - cdf_j(e_k)), doubles in C order, n_chan n_u n_v
 *          of them; SPH_CUBE_PER_VELOCITY divides by dv.  sph_cube copies it to host memory; sph_cube_dev leaves it in
 *          device memory, ordered on the context's stream.
 * Order    every voxel adds its terms in the (image-plane cell, particle id) order of the pass's own binning, which
 *          depends only on the descriptor and the selected particles' h range: a repeated call, the host and the device
 *          form are bitwise equal, and the result does not depend on the context's sorted order.
 * Cost     two stream synchronisations (selection statistics, window size) + the copies of the host form.  No state,
 *          statistic (other than device_bytes: the analysis scratch) or flag of the context changes.
 * SPH_ERR_ARG: null descriptor or output, n_u, n_v or n_chan < 1, out_len != n_chan n_u n_v, lo > hi or non-finite, h < 0
 * or non-finite, a NaN clip, a non-finite centre, v_ref or v0, dv <= 0 or non-finite, a negative or non-finite sigma_scale
 * or sigma_floor, a bad rot, unknown flags, reserved != 0.  SPH_ERR_STATE: a stale c with sigma_scale > 0; a selected h <= 0
 * or non-finite.  SPH_ERR_NOMEM: the scratch does not fit. */
#define SPH_CUBE_PER_VELOCITY 1
typedef struct sph_cube_desc {
    double  rot[9];                 /* rows u^, v^, w^ (row-major)                                   */
    double  centre[3], v_ref[3];    /* origin of the image plane, velocity of the reference frame    */
    double  lo[2], hi[2];           /* node box on the image axes u, v                               */
    double  clip_lo[3], clip_hi[3]; /* strict particle clip box (simulation axes); -/+INFINITY = none */
    double  h;                      /* > 0: one h for all; 0: each particle's own h                  */
    double  v0, dv;                 /* centre of channel 0, channel width (> 0)                      */
    double  sigma_scale, sigma_floor; /* sigma_j = sqrt((sigma_scale c_j)^2 + sigma_floor^2), both >= 0 */
    int32_t n_u, n_v;               /* image nodes per axis, each >= 1                               */
    int32_t n_chan;                 /* channels, >= 1                                                */
    int32_t flags;                  /* SPH_CUBE_PER_VELOCITY                                         */
    int64_t reserved;               /* must be 0                                                     */
} sph_cube_desc;                    /* 264 bytes */
int sph_cube(sph_ctx *ctx, const sph_cube_desc *d, const double *values, double *host_out, int64_t out_len);
int sph_cube_dev(sph_ctx *ctx, const sph_cube_desc *d, const double *d_values, double *d_out, int64_t out_len);

/* ---- emission-absorption images: what an observer sees of the owned gas when it is not optically thin -- intensity,
 *      optical depth, transmission and the depth of the tau = tau_surface surface (summersph_amd/transfer.py) -----------
 * Frame, Select, Nodes  exactly sph_cube's: rot[9] with rows u^, v^, w^ (orthonormal and right-handed within 1e-12, else
 *          SPH_ERR_ARG), w^ pointing away from the observer; P_j = rot (r_j - centre), every row evaluated as
 *          ((a0 dx + a1 dy) + a2 dz) with no fused multiply-adds; the owned gas particles with clip_lo < r < clip_hi on
 *          every axis of the SIMULATION frame (strict); h > 0: one h for every particle, 0: each particle's own; node i on
 *          image axis a is lo[a] + i (hi[a] - lo[a]) / (n - 1), the last one exactly hi[a] (np.linspace), n == 1: the
 *          single node lo[a].  The depth of a particle is D_j = P_j,w.
 * Inputs   the opacity kappa_j = kappa_scale K_j and the source function S_j.  K and S each come from the place their
 *          selector (kappa, source) names: an SPH_F_* field of the context (SPH_ERR_STATE exactly where sph_download_field
 *          would refuse it as stale), SPH_TRANSFER_VALUES (the caller's array of sph_count doubles in sph_download_field's
 *          order; host memory for sph_transfer, device memory for _dev) or SPH_TRANSFER_ONE (the constant 1).  A pointer
 *          must be non-NULL exactly when its selector is SPH_TRANSFER_VALUES.  A selected K_j that is negative or
 *          non-finite, or a selected non-finite S_j, gives SPH_ERR_ARG (found in the statistics pass, before anything is
 *          written).  S_j may have either sign.
 * Slab     for node g, b = |g - P_j,uv| and p = b / h_j: dtau_j = y0_j F(p), y0_j = m_j kappa_j / (pi h_j^2), pi in double
 *          precision, F the line-integrated spline of sph_cube ("Footprint" above): F(0) = 1.5, F = 0 for p >= 2.
 * Order    the selected particles are taken in ascending (D_j, id), nearest the observer first; equal depths are ordered by
 *          id (a flat sheet seen face-on); the order is total over the doubles, -0.0 and +0.0 compare equal and fall to
 *          the id.
 * Compositing  per node start with tau = 0, T = 1, I = 0, surf = NaN and the node running.  For each particle in order
 *          while the node runs, a particle with p >= 2 being skipped, with no fused multiply-adds:
 *            a = -expm1(-dtau)
 *            I <- I + (S_j T) a
 *            T <- T - T a
 *            tau <- tau + dtau
 *            if surf is NaN and tau >= tau_surface: surf <- D_j
 *            if tau >= tau_max: the node stops (deeper particles add nothing)
 *          tau_max = +INFINITY never stops a node.  The stop is part of the definition, as the 8.5 sigma truncation is of
 *          sph_cube's; it is what lets the pass leave an opaque tile early.
 * Output   four planes of n_u n_v doubles in C order [plane][iu][iv], out_len == 4 n_u n_v: 0: I + T background; 1: tau
 *          as accumulated until the node stopped; 2: T; 3: surf, NaN where tau never reached tau_surface.  sph_transfer
 *          copies them to host memory; sph_transfer_dev leaves them in device memory, ordered on the context's stream.
 * Reproducibility  the result depends only on the descriptor, the selected particles and their ids: a repeated call, the
 *          host and the device form, and the same state in a context with another sorted order are bitwise equal.
 * Cost     two stream synchronisations (selection statistics, list sizes) + the copies of the host form.  Every particle
 *          is entered into the list of each tile of 8 x 8 nodes that holds a node within 2 h_j (1 + 1e-6) of P_j,uv on both
 *          axes; the lists hold sum_j (tiles touched) entries of 8 bytes (twice, for the sort).  SPH_ERR_NOMEM when the
 *          scratch does not fit or that count reaches 2^31: the bad case is a large fixed h over a tiny image extent, where
 *          every particle touches every tile.  No state, statistic (other than device_bytes: the analysis scratch) or flag
 *          of the context changes.  One context: compositing across contexts is only valid for depth-disjoint sets.
 * SPH_ERR_ARG: null descriptor or output, n_u or n_v < 1, out_len != 4 n_u n_v, lo > hi or non-finite, h < 0 or
 * non-finite, a NaN clip, a non-finite centre, kappa_scale < 0 or non-finite, tau_surface <= 0 or NaN, tau_max <= 0 or NaN,
 * a non-finite background, a bad rot, a selector that is neither a field id nor SPH_TRANSFER_VALUES / _ONE, a pointer given
 * without SPH_TRANSFER_VALUES or missing with it, flags != 0, reserved != 0, a bad selected K or S (above).  SPH_ERR_STATE:
 * a stale field named by source or kappa; a selected h <= 0 or non-finite.  SPH_ERR_NOMEM: see Cost. */
#define SPH_TRANSFER_VALUES (-1)    /* K or S from the caller's array */
#define SPH_TRANSFER_ONE (-2)       /* K or S = 1                     */
typedef struct sph_transfer_desc {
    double  rot[9];                 /* rows u^, v^, w^ (row-major)                                   */
    double  centre[3];              /* origin of the image plane                                     */
    double  lo[2], hi[2];           /* node box on the image axes u, v                               */
    double  clip_lo[3], clip_hi[3]; /* strict particle clip box (simulation axes); -/+INFINITY = none */
    double  h;                      /* > 0: one h for all; 0: each particle's own h                  */
    double  kappa_scale;            /* kappa_j = kappa_scale K_j; >= 0, finite                       */
    double  tau_surface;            /* plane 3 is the depth at which tau reaches it; > 0             */
    double  tau_max;                /* a node stops at tau >= tau_max; > 0, may be +INFINITY         */
    double  background;             /* intensity behind the gas; finite                              */
    int32_t n_u, n_v;               /* image nodes per axis, each >= 1                               */
    int32_t source, kappa;          /* where S and K come from: SPH_F_*, SPH_TRANSFER_VALUES, _ONE   */
    int32_t flags;                  /* must be 0                                                     */
    int32_t reserved;               /* must be 0                                                     */
} sph_transfer_desc;                /* 240 bytes */
int sph_transfer(sph_ctx *ctx, const sph_transfer_desc *d, const double *source, const double *kappa, double *host_out,
                 int64_t out_len);
int sph_transfer_dev(sph_ctx *ctx, const sph_transfer_desc *d, const double *d_source, const double *d_kappa, double *d_out,
                     int64_t out_len);

/* ---- the rates of sph_forces split by physical term: which term moves angular momentum at a radius (torque by term per
 *      ring), where the artificial viscosity heats the gas (a shock-heating map through sph_render_field), how large the
 *      numerical dissipation is beside the PdV work ----------------------------------------------------------------------
 * Definition  the acceleration, du/dt and dalpha/dt that sph_forces would write now, with every sum taken apart where the
 *          force pass folds terms together: the pair accumulator m_j ((P_i/rho_i^2 + P_j/rho_j^2) + Pi_ij) of [F]:381-383
 *          ([V]:413-416), the factor (P_i/rho_i^2 + Pi_ij/2) of [F]:387 ([V]:419-421), the start value of the acceleration
 *          (self-gravity, then the sinks) and the two addends of the alpha rate.  Every quantity is read from the context's
 *          force records exactly as sph_forces would read them; the state required is that of sph_forces (the grid, the list
 *          and the density current, the EOS valid), else SPH_ERR_STATE "call sph_density first" -- after sph_step call
 *          sph_density first, the closing kick made the records stale.
 * Targets  the owned gas (original ids < n_owned).  The rows of ghosts are NaN.
 * Sources  whatever the target's neighbour list holds, ghosts included; the sinks; the gravity sources of sph_forces (the
 *          context's own particles, or the external set of sph_set_gravity_sources_dev).
 * Rows     out[row * n + id], n = sph_count, n_out == SPH_TERMS_NROW * n, id in sph_download_field's order: every row is a
 *          contiguous array that sph_render_field accepts as values.  g: the normalised kernel gradient the force pass uses
 *          for the pair, v_ij = v_i - v_j, Pi_ij: the force pass's visc (vdotr = min(v.r, 0), visc_eps, the halved records
 *          and the reciprocal helpers of the force pass).
 *            0-2   a_P   pressure gradient      fixed h -sum m_j (P_i/rho_i^2 + P_j/rho_j^2) g         [F]:381-383
 *                                               variable h -sum m_j (C_i g_i + C_j g_j), C = P/(Omega rho^2)   [V]:413-416
 *            3-5   a_V   artificial viscosity   fixed h -sum m_j Pi_ij g                               [F]:373-383
 *                                               variable h -sum m_j Pi_ij (g_i + g_j)/2                [V]:405-416
 *            6-8   a_S   sink gravity on the gas: the force pass's sink loop ([F]:567-576, [V]:691-), started from 0
 *            9-11  a_G   gas self-gravity: with SPH_FLAG_SELF_GRAVITY the Barnes-Hut term sph_forces starts its sums from
 *                        ([F]:825) -- the same tree, walk and acceptance test, written here and not to SPH_F_AX..AZ; +0.0
 *                        without self-gravity; NaN with SPH_TERMS_SKIP_GAS_GRAVITY (no tree is built or walked)
 *            12    du_P  PdV work               sum m_j (v_ij . g) P_i/rho_i^2 (variable h: C_i)       [F]:387, [V]:419-421
 *            13    du_V  viscous heating        sum m_j (v_ij . g) Pi_ij/2: every pair term is >= 0    [F]:387, [V]:419-421
 *            14    alpha source                 max(sum m_j (v_ij . g) / rho_i, 0)                     [F]:316-318,390, [V]:346,427
 *            15    alpha decay                  alpha_decay (alpha_floor - alpha_i) c_i / h_i          [F]:316-318, [V]:346
 *          Rows 0-11 summed per axis are SPH_F_AX..AZ, rows 12 + 13 SPH_F_DU and rows 14 + 15 SPH_F_DALPHA of sph_forces, to
 *          rounding.  A coincident pair (r == 0) and a pair beyond the support add exact zeros, as in the force pass; the
 *          table normalisation 1 / (pi h^4) is applied once at the end ([F]:126).  a_P and a_V are pairwise antisymmetric
 *          at fixed h: without ghosts sum m a and sum m r x a of either vanish to rounding, and so do sum m (v . a_P + du_P)
 *          and sum m (v . a_V + du_V).
 * Order    a target's sums run over its neighbour list in list order, so they depend on the context's sorted order and its
 *          list layout: repeated calls, the host and device forms, and calls before and after an intervening sph_forces agree
 *          bitwise; different contexts (another slot order, flags that change the list) agree to rounding only -- unlike the
 *          (cell, id)-ordered analysis calls above.  No float atomics.
 * cost     one gather pass over the lists (the memory traffic of the gather force kernel; a 128-byte record per slot) and a
 *          pass that turns the records into rows, plus the tree walk when rows 9-11 are asked for; with self-gravity and no
 *          valid tree in place the tree sph_forces would build is built and KEPT (the next sph_forces uses it: the same tree,
 *          bit for bit).  Scratch (16 n doubles, + 3 n with the walk) from the analysis calls' shared buffer.  Host form: one
 *          synchronisation, then the copy is complete; device form: ordered on the
 *          context's stream, no synchronisation (but one when the scratch has to grow).  No field (SPH_F_AX..DALPHA
 *          included, bitwise), list, grid, flag, dt, validity of a field or statistic (other than device_bytes) changes;
 *          force_passes does not move; a run that calls sph_density and this between the steps is bitwise the run that calls
 *          sph_density alone.
 * SPH_ERR_ARG: null descriptor, n_out != SPH_TERMS_NROW * sph_count, null output with n > 0, unknown flags, reserved != 0;
 * nothing is written then.  n == 0 succeeds and writes nothing.  SPH_ERR_STATE: see Definition.  SPH_ERR_NOMEM: the scratch
 * does not fit. */
#define SPH_TERMS_NROW 16
#define SPH_TERMS_SKIP_GAS_GRAVITY 1   /* do not walk the tree: rows 9..11 are NaN */
typedef struct sph_force_terms_desc {
    int32_t flags;        /* SPH_TERMS_* */
    int32_t reserved[3];  /* must be 0 */
} sph_force_terms_desc;   /* 16 bytes */
int sph_force_terms(sph_ctx *ctx, const sph_force_terms_desc *d, double *host_out, int64_t n_out);
int sph_force_terms_dev(sph_ctx *ctx, const sph_force_terms_desc *d, double *d_out, int64_t n_out);

/* ---- binned sums: the count, the sum of a weight and the sums of the weight times up to eight quantities (and their
 *      squares) of the owned gas over one or two binned axes -- phase diagrams (rho x u), distribution functions, the mean
 *      of any quantity against any other, ring sums of the rows sph_gradients and sph_force_terms write.  The generic form
 *      of sph_profile's reduction: the same order rule, the same bitwise reproducibility ------------------------------------
 * Sources  an axis or a quantity is an SPH_F_* id, read as sph_download_field reads it (SPH_ERR_STATE exactly when that call
 *          would refuse the field as stale), or SPH_BINNED_ROW(k): row k of values, values[k * n + id], n = sph_count, id in
 *          sph_download_field's order (ghosts included) -- the layout sph_gradients_dev, sph_force_terms_dev and
 *          sph_energy_dev's phi write, so those outputs pass straight in.  values is host memory in the host form and device
 *          memory in the device form; it is NULL if and only if n_rows == 0.  Only the rows some source names are read.
 * Edges    one table per axis, computed once on the host: edge[k] = lo + (k (hi - lo)) / n, or with SPH_BINNED_LOGa
 *          lo pow(hi / lo, k / n); edge[n] = hi exactly (sph_profile's ring edges).  With SPH_BINNED_EDGESa the table is the
 *          caller's: n[a] + 1 strictly increasing finite doubles in edges (host memory in both forms; the tables of the axes
 *          that have one, axis 0's first), lo / hi of that axis ignored.  sph_binned_edges returns the table the call will
 *          use (pure host code: no context, no device) and refuses what the call refuses of the descriptor and the tables.
 *          Bin along axis a: edge[k] <= value < edge[k + 1] against that table, never by a formula alone.  Bin b =
 *          k0 n[1] + k1.
 * Select   the owned gas particles (ghosts and sinks excluded, as the renders and sph_profile select) whose every axis
 *          value lies in [edge[0], edge[n]) (a NaN is outside).  With SPH_BINNED_SKIP_NAN a particle inside the range with
 *          a NaN among its quantities is dropped (the rows of sph_gradients and sph_force_terms are NaN at non-targets);
 *          without it the NaN is summed and poisons its bin.
 * Weight   w = 1 (SPH_BINNED_W_ONE), m (SPH_BINNED_W_MASS) or m / rho (SPH_BINNED_W_VOLUME; rho as
 *          sph_download_field(SPH_F_RHO) returns it, SPH_ERR_STATE exactly when that call would refuse).
 * Sums     sums[b * nsum + s], nsum = 2 + n_q (1 + squares), n_sums == n[0] n[1] nsum:  s = 0 N (the count as a double),
 *          s = 1 sum w, s = 2 + k sum w * A_k, and with SPH_BINNED_SQUARES s = 2 + n_q + k sum w * (A_k * A_k); every term in
 *          exactly that parenthesisation, no fused multiply-adds.  The sums are additive: those of two contexts or ranks add
 *          up to the sums of the union.
 * Counts   counts[3] (may be NULL; device memory in the device form): selected, owned gas outside the range, owned gas
 *          inside the range dropped by SPH_BINNED_SKIP_NAN.  Exact (integers); they add up to the owned gas.
 * Order    sph_profile's: the selected particles are sorted by (bin, original id); every bin's run is cut into pieces of
 *          1024 sorted positions from its own start, each added by a 64-lane wavefront (lane l: positions l, l + 64, ..., then
 *          a xor butterfly), then the pieces by another in the same shape.  The sums are bitwise reproducible, independent
 *          of the context's sorted order, of the dense or hashed grid, of the host or device form and of repeated calls; a
 *          ring-binned sum with weight m of SPH_F_U is bitwise sph_profile's sum 11 where both select the same particles.
 *          No float atomics.
 * cost     host form: one read-back (sums and counts); device form: ordered on the context's stream, no synchronisation
 *          (but one when the scratch has to grow).  The scratch is the analysis calls' shared buffer.  No state, field,
 *          statistic (other than device_bytes), flag, grid, list or dt of the context changes.
 * SPH_ERR_ARG: null descriptor or output, n_axes not 1 or 2, n[a] < 1, n[1] != 1 with one axis, n[0] n[1] > 2^20, n_sums
 * != n[0] n[1] nsum, n_q outside 0 .. SPH_BINNED_MAX_Q, a source that is neither an SPH_F_* id nor a row below n_rows, n_rows
 * outside 0 .. 16, values NULL with n_rows > 0 or given with n_rows == 0, edges NULL with SPH_BINNED_EDGESa or given without, a
 * caller's table that is not strictly increasing or not finite, a non-finite lo or hi, lo >= hi, LOG with lo <= 0, LOG and
 * EDGES on one axis, a flag of axis 1 with one axis, bins so narrow that two computed edges coincide, an unknown weight,
 * unknown flags, reserved != 0; nothing is written then.  SPH_ERR_STATE: a stale field.  SPH_ERR_NOMEM: the scratch does
 * not fit.  An empty context or an empty selection gives zero sums. */
#define SPH_BINNED_MAX_Q     8
#define SPH_BINNED_ROW(k)    (-1 - (k))   /* a source: row k of values, k < n_rows <= 16 */
#define SPH_BINNED_W_ONE     0            /* w = 1 */
#define SPH_BINNED_W_MASS    1            /* w = m */
#define SPH_BINNED_W_VOLUME  2            /* w = m / rho */
#define SPH_BINNED_LOG0      1            /* axis 0: logarithmic edges (lo > 0) */
#define SPH_BINNED_LOG1      2
#define SPH_BINNED_EDGES0    4            /* axis 0: the caller's edge table */
#define SPH_BINNED_EDGES1    8
#define SPH_BINNED_SQUARES   16           /* also sum w A A per quantity */
#define SPH_BINNED_SKIP_NAN  32           /* drop a particle if any of its quantities is NaN */
typedef struct sph_binned_desc {
    double  lo[2], hi[2];           /* axis range [lo, hi); ignored with SPH_BINNED_EDGESa             */
    int32_t axis[2];                /* source of each axis: SPH_F_* or SPH_BINNED_ROW(k)                */
    int32_t n[2];                   /* bins per axis >= 1; n[1] == 1 with one axis; n[0] n[1] <= 2^20   */
    int32_t n_axes;                 /* 1 or 2                                                           */
    int32_t n_q;                    /* quantities, 0 .. SPH_BINNED_MAX_Q                                */
    int32_t q[SPH_BINNED_MAX_Q];    /* their sources                                                    */
    int32_t weight;                 /* SPH_BINNED_W_*                                                   */
    int32_t n_rows;                 /* rows of values, 0 .. 16                                          */
    int32_t flags;                  /* SPH_BINNED_LOG* | EDGES* | SQUARES | SKIP_NAN                    */
    int32_t reserved[3];            /* must be 0                                                        */
} sph_binned_desc;                  /* 112 bytes */
int sph_binned(sph_ctx *ctx, const sph_binned_desc *d, const double *values, const double *edges, double *host_sums,
               int64_t n_sums, int64_t *counts);
int sph_binned_dev(sph_ctx *ctx, const sph_binned_desc *d, const double *d_values, const double *edges, double *d_sums,
                   int64_t n_sums, int64_t *d_counts);
int sph_binned_edges(const sph_binned_desc *d, const double *edges, int32_t axis, double *out);

/* ---- pair sums: per bin of the separation r (or of r / h_i), the count of the ordered pairs (i, j), j != i, of the owned gas
 *      and exact sums over them -- the pair distribution g(r / h) (the pairing instability, particle noise), the mean pairwise
 *      radial velocity, the second- and third-order structure functions of the velocity and the variogram of any scalar ----
 * Sources  j: the owned gas (ghosts and sinks excluded) that is usable: finite x, y, z and finite every requested quantity --
 *          the A_k, m with SPH_PAIRS_W_MASS, vx vy vz with SPH_PAIRS_VELOCITY, h (also > 0) with SPH_PAIRS_SCALE_H.  An owned
 *          gas particle that is not usable is neither source nor target and is counted in counts[2].
 * Targets  i: the sources strictly inside the clip box (clip_lo < r < clip_hi on every axis, the renders' rule; -inf / +inf
 *          for no clip) whose original id (sph_download_field's order) has id % target_stride == target_phase.  Sources
 *          outside the clip box still act as sources.  The phases 0 .. stride - 1 partition the targets: a single phase is an
 *          unbiased sample at 1 / stride of the cost.
 * A_k      up to SPH_PAIRS_MAX_Q quantities, each an SPH_F_* id, read as sph_download_field reads it (SPH_ERR_STATE exactly
 *          when that call would refuse the field as stale), or SPH_PAIRS_ROW(k): row k of values, values[k * n + id], n =
 *          sph_count -- sph_binned's sources.  values is host memory in the host form and device memory in the device form;
 *          NULL if and only if n_rows == 0.
 * Pair     dx = x_j - x_i (dy, dz alike), d2 = (dx * dx + dy * dy) + dz * dz, r = sqrt(d2); the binned variable is r, or with
 *          SPH_PAIRS_SCALE_H r / h_i (an IEEE division; h_i the target's h, params.h on the fixed-h path).  No fused
 *          multiply-adds anywhere.  The pair is selected when the variable lies in [edge[0], edge[n_bins]); its bin b has
 *          edge[b] <= variable < edge[b + 1] against the table, never by a formula alone.
 * Edges    sph_binned's: edge[k] = lo + (k (hi - lo)) / n_bins, or with SPH_PAIRS_LOG lo pow(hi / lo, k / n_bins);
 *          edge[n_bins] = hi exactly.  With SPH_PAIRS_EDGES the table is the caller's: n_bins + 1 strictly increasing finite
 *          doubles in edges (host memory in both forms), lo / hi ignored.  sph_pairs_edges returns the table the call will
 *          use (pure host code: no context, no device) and refuses what the call refuses of the descriptor and the table.
 * Weight   w = w_i * w_j with w_p = 1 (SPH_PAIRS_W_ONE) or m_p (SPH_PAIRS_W_MASS).
 * Sums     sums[b * nsum + s], nsum = 2 + 2 n_q + (4 with SPH_PAIRS_VELOCITY), n_out == n_bins nsum:
 *            s = 0                N, the count
 *            s = 1                sum w
 *            s = 2 + k            sum w * dA_k,           dA_k = A_k(j) - A_k(i)
 *            s = 2 + n_q + k      sum w * (dA_k * dA_k)
 *          and with SPH_PAIRS_VELOCITY, s0 = 2 + 2 n_q, dv = v_j - v_i per component,
 *          u = ((dvx * dx + dvy * dy) + dvz * dz) / r, u = 0 where r == 0, u2 = u * u:
 *            s = s0               sum w * u
 *            s = s0 + 1           sum w * u2
 *            s = s0 + 2           sum w * (u2 * u)
 *            s = s0 + 3           sum w * ((dvx * dvx + dvy * dvy) + dvz * dvz)
 * Exact    every float sum is accumulated exactly in 128-bit fixed point.  A first pass takes order-free maxima over the
 *          sources: w_max = max |w_p|, A_k,max = max |A_k|, v_max = the largest |v| component.  With W2 = w_max * w_max,
 *          D_k = 2 * A_k,max and V = 4 * v_max the bounds B_s are ("Bounds"):
 *            s = 1  W2;   s = 2 + k  W2 * D_k;   s = 2 + n_q + k  W2 * (D_k * D_k);
 *            s = s0  W2 * V;   s = s0 + 1  W2 * (V * V);   s = s0 + 2  W2 * ((V * V) * V);   s = s0 + 3  W2 * (V * V)
 *          (|u| <= sqrt(3) * 2 v_max < V, |dv|^2 <= 12 v_max^2 < V * V; rounding is monotone, so no term exceeds its bound).
 *          e_s is the binary exponent with B_s < 2^e_s: the exponent frexp returns (0 for B_s = 0); e_0 = 62.  A term is
 *          formed in double as written above, multiplied by 2^(62 - e_s) (exact), rounded half-even to a 64-bit integer (its
 *          magnitude is < 2^62) and added into a 128-bit two's-complement integer: an error of at most half a quantum
 *          2^(e_s - 62) per term, none from the addition; B_s = 0 gives the sum 0.  N is a plain 64-bit count.  A bin's
 *          accumulator overflows only beyond 2^65 terms.  The bounds must be finite.
 *          raw[2 (b * nsum + s)] is the low and raw[2 (b * nsum + s) + 1] the high 64-bit limb, exps[s] = e_s; sums[..] is
 *          limb value * 2^(e_s - 62), correctly rounded (once).  Raw results with equal exps add exactly as 128-bit integers
 *          (phases, clip boxes, ranks); sph_pairs_finish(d, exps, raw, sums) turns limbs into the same doubles (pure host
 *          code; it reads n_bins, n_q and flags of the descriptor).
 * Counts   counts[3] (may be NULL; device memory in the device form): targets, sources, owned gas not usable.  sources +
 *          not usable = the owned gas.
 * Order    none: integer addition is associative.  sums, raw, exps and counts are bitwise independent of the context's
 *          sorted order, of the dense or hashed grid, of the launch shape, of the host or device form and of repeated calls.
 *          No float atomics.
 * Search   groups' hashed cell table at cell edge r_max (1 + 1e-6), r_max = edge[n_bins] (times the targets' largest h with
 *          SPH_PAIRS_SCALE_H), enlarged on the device where an axis would need more than 2^21 - 8 cells; the cost is that of
 *          the 27 cells around every target.
 * cost     host form: one read-back (limbs, exponents, counts; raw and exps may be NULL); device form: ordered on the
 *          context's stream, no synchronisation (but one when the scratch has to grow); d_raw, d_exps, d_counts may be NULL.
 *          The scratch is the analysis calls' shared buffer.  No state, field, statistic (other than device_bytes), flag,
 *          grid, list or dt of the context changes.
 * SPH_ERR_ARG: null descriptor or output, n_bins outside 1 .. SPH_PAIRS_MAX_BINS, n_out != n_bins nsum, n_q outside 0 ..
 * SPH_PAIRS_MAX_Q, a source that is neither an SPH_F_* id nor a row below n_rows, n_rows outside 0 .. 16, values NULL with
 * n_rows > 0 or given with n_rows == 0, edges NULL with SPH_PAIRS_EDGES or given without, a caller's table that is not strictly
 * increasing or not finite, a non-finite lo or hi, lo >= hi, LOG with lo <= 0, LOG with EDGES, computed edges that coincide,
 * target_stride < 1, target_phase outside 0 .. target_stride - 1, a NaN in the clip box, an unknown weight, unknown flags,
 * reserved != 0; nothing is written then.  SPH_ERR_STATE: a stale field.  SPH_ERR_NOMEM: the scratch does not fit.  An empty
 * context or an empty selection gives zero sums. */
#define SPH_PAIRS_MAX_Q      4
#define SPH_PAIRS_MAX_BINS   1024
#define SPH_PAIRS_ROW(k)     (-1 - (k))   /* a quantity: row k of values, k < n_rows <= 16 */
#define SPH_PAIRS_W_ONE      0            /* w_p = 1 */
#define SPH_PAIRS_W_MASS     1            /* w_p = m_p */
#define SPH_PAIRS_LOG        1            /* logarithmic edges (lo > 0) */
#define SPH_PAIRS_EDGES      2            /* the caller's edge table */
#define SPH_PAIRS_SCALE_H    4            /* bin r / h_i instead of r */
#define SPH_PAIRS_VELOCITY   8            /* also the four velocity sums */
typedef struct sph_pairs_desc {
    double  lo, hi;                 /* range [lo, hi) of the binned variable; ignored with SPH_PAIRS_EDGES */
    double  clip_lo[3], clip_hi[3]; /* the targets' strict clip box; -inf / +inf: none                     */
    int32_t n_bins;                 /* 1 .. SPH_PAIRS_MAX_BINS                                             */
    int32_t n_q;                    /* quantities, 0 .. SPH_PAIRS_MAX_Q                                    */
    int32_t q[SPH_PAIRS_MAX_Q];     /* their sources: SPH_F_* or SPH_PAIRS_ROW(k)                          */
    int32_t weight;                 /* SPH_PAIRS_W_*                                                       */
    int32_t n_rows;                 /* rows of values, 0 .. 16                                             */
    int32_t flags;                  /* SPH_PAIRS_LOG | EDGES | SCALE_H | VELOCITY                          */
    int32_t target_stride;          /* >= 1                                                                */
    int32_t target_phase;           /* 0 .. target_stride - 1                                              */
    int32_t reserved[3];            /* must be 0                                                           */
} sph_pairs_desc;                   /* 120 bytes */
int sph_pairs(sph_ctx *ctx, const sph_pairs_desc *d, const double *values, const double *edges, double *host_sums, int64_t n_out,
              uint64_t *host_raw, int32_t *exps, int64_t *counts);
int sph_pairs_dev(sph_ctx *ctx, const sph_pairs_desc *d, const double *d_values, const double *edges, double *d_sums,
                  int64_t n_out, uint64_t *d_raw, int32_t *d_exps, int64_t *d_counts);
int sph_pairs_edges(const sph_pairs_desc *d, const double *edges, double *out);
int sph_pairs_finish(const sph_pairs_desc *d, const int32_t *exps, const uint64_t *raw, double *sums);

/* ---- mode sums: the azimuthal Fourier sums C_m, S_m of a weight per ring, m = 0 .. m_max, and the logarithmic-spiral sums
 *      over (m, p) of the whole annulus -- which spiral modes a disc carries, how strong they are (A_m(R) = |C_m + i S_m| /
 *      C_0) and how tightly wound (the peak of |A(m, p)| gives the arm number m and the pitch angle tan i = m / p) ----------
 * Frame    sph_profile's, by the same code: n^ = normal / |normal| and e1, e2 as there; centre c: centre (centre_v is
 *          checked and otherwise unused), or sink `sink`'s position on the device.  Per particle r' = r - c, X = r'.e1,
 *          Y = r'.e2, z' = r'.n^ (a.b = (a0 b0 + a1 b1) + a2 b2), R = sqrt(X X + Y Y).  There is no AUTO_NORMAL: pass the
 *          normal sph_profile wrote back.  No fused multiply-adds anywhere.
 * Select   the owned gas particles (ghosts and sinks excluded) with r_min <= R < r_max and |z'| < z_max (strict;
 *          INFINITY: no cut).  A selected particle is usable when base and A (below) are both finite; an owned gas particle
 *          whose x, y or z is not finite counts as selected and not usable.  What is not usable is dropped and counted.
 * Weight   w = base * A: base = 1 (SPH_MODES_W_ONE) or m_j (SPH_MODES_W_MASS); A = 1 (n_q == 0; then w = base) or one
 *          quantity (n_q == 1): q is an SPH_F_* id, read as sph_download_field reads it (SPH_ERR_STATE exactly when that
 *          call would refuse the field as stale), or SPH_MODES_ROW(k): row k of values, values[k * n + id], n = sph_count
 *          -- sph_binned's sources.  values is host memory in the host form and device memory in the device form; NULL if
 *          and only if n_rows == 0.  Only the row q names is read.
 * Angle    c = X / R, s = Y / R (c = 1, s = 0 where R == 0); no trigonometric function.  The powers (c + i s)^m by the
 *          recurrence c_0 = 1, s_0 = 0, c_{m+1} = c_m * c - s_m * s, s_{m+1} = s_m * c + c_m * s: each product and each sum
 *          rounded separately.
 * Rings    sph_profile's edges, computed once on the host: edge[k] = r_min + (k (r_max - r_min)) / n_r, or with
 *          SPH_MODES_LOG r_min pow(r_max / r_min, k / n_r); edge[n_r] = r_max exactly.  Ring k: edge[k] <= R < edge[k + 1]
 *          against that table.  For ring k and m = 0 .. m_max:  C[k][m] = sum w * c_m,  S[k][m] = sum w * s_m;
 *          ring_counts[k] = the usable selected particles of ring k.
 * Spiral   with n_p > 0: p[l] = p_min + (l (p_max - p_min)) / (n_p - 1) (p[0] = p_min when n_p == 1), computed once on the
 *          host; per particle u = log(R / r_ref), and per l: theta = p[l] * u, (cp, sp) = (cos theta, sin theta) (the device
 *          library's sincos).  For every m, l:  CS[m][l] = sum w * (c_m * cp - s_m * sp),  SN[m][l] = sum w * (s_m * cp +
 *          c_m * sp) -- the cosine and sine sums of m phi + p ln(R / r_ref).  A selected particle with R == 0 enters the ring
 *          sums but not these, and is counted in counts[3].
 * Tables   sph_modes_tables returns the two tables the call will use (pure host code: no context, no device; edges_out n_r +
 *          1, p_out n_p doubles, either may be NULL) and refuses what the call refuses of the descriptor.
 * Exact    every sum is accumulated exactly in 128-bit fixed point (sph_pairs' scheme).  A first pass takes the order-free
 *          maximum W_max = max |w| over the usable selected particles.  One bound for all sums: B = 2 * W_max (|c_m|, |s_m|
 *          and |c_m cp - s_m sp| are <= 1 + O(m eps) < 2; rounding is monotone, so no term exceeds B); e is the binary
 *          exponent with B < 2^e: the exponent frexp returns (0 for B = 0).  A term is formed in double as written above,
 *          multiplied by 2^(62 - e) (exact), rounded half-even to a 64-bit integer (its magnitude is < 2^62) and added into
 *          a 128-bit two's-complement integer: an error of at most half a quantum 2^(e - 62) per term, none from the
 *          addition.  An accumulator overflows only beyond 2^65 terms.  B must be finite.
 * Outputs  sums[n_out], n_out == 2 (m_max + 1) (n_r + n_p): the ring block, ((k (m_max + 1)) + m) 2 + {0: C, 1: S}, then
 *          the spiral block at 2 n_r (m_max + 1) + ((m n_p) + l) 2 + {0: CS, 1: SN}; every double is limb value * 2^(e -
 *          62), correctly rounded (once).  raw: the same layout with two uint64 limbs each, raw[2 g] the low and raw[2 g +
 *          1] the high one.  exp: e, one int32.  ring_counts: n_r int64.  counts[4]: selected and usable, owned gas outside
 *          the selection, owned gas selected but not usable, usable selected with R == 0 (part of the first); the first
 *          three add up to the owned gas.  raw, exp, ring_counts and counts may be NULL (device memory in the device form).
 *          Raw results with equal e add exactly as 128-bit integers (ranks, clip pieces); sph_modes_finish(d, exp, raw,
 *          sums) turns limbs into the same doubles (pure host code; it reads n_r, m_max and n_p of the descriptor).
 * Order    none: integer addition is associative.  sums, raw, exp, ring_counts and counts are bitwise independent of the
 *          context's sorted order, of the dense or hashed grid, of the launch shape, of the host or device form and of
 *          repeated calls.  No float atomics.
 * cost     host form: one read-back (limbs, ring counts, exponent, counts); device form: ordered on the context's stream, no
 *          synchronisation of the stream (but one when the scratch has to grow).  Both forms first wait, on the host, for
 *          the event of the last upload of the context's pinned table copy (the edges and p of the previous sph_modes,
 *          sph_pairs, sph_binned or sph_profile call) before they rewrite it: a device-form call that follows another waits until the
 *          stream has run the earlier call's table copy and all that was queued before it, not that call's kernels.  The scratch is the analysis calls' shared buffer.  No
 *          state, field, statistic (other than device_bytes), flag, grid, list or dt of the context changes.
 * SPH_ERR_ARG: null descriptor or output, n_r outside 1 .. SPH_MODES_MAX_RINGS, m_max outside 0 .. SPH_MODES_MAX_M, n_p
 * outside 0 .. SPH_MODES_MAX_P, n_out != 2 (m_max + 1) (n_r + n_p), r_min < 0, r_min >= r_max, a non-finite r_min / r_max, LOG
 * with r_min == 0, rings so narrow that two edges coincide, NaN z_max, a zero or non-finite normal, a non-finite centre or
 * centre_v (sink < 0), sink < -1 or >= sph_sink_count, with n_p > 0: r_ref <= 0 or not finite, a non-finite p_min or p_max,
 * p_min > p_max; n_q outside 0 .. 1, a source that is neither an SPH_F_* id nor a row below n_rows, n_rows outside 0 .. 16,
 * values NULL with n_rows > 0 or given with n_rows == 0, an unknown weight, unknown flags, reserved != 0; nothing is written
 * then.  SPH_ERR_STATE: a stale field.  SPH_ERR_NOMEM: the scratch does not fit.  An empty context or an empty selection
 * gives zero sums and e = 0. */
#define SPH_MODES_MAX_M      8
#define SPH_MODES_MAX_RINGS  1024
#define SPH_MODES_MAX_P      256
#define SPH_MODES_ROW(k)     (-1 - (k))   /* the quantity: row k of values, k < n_rows <= 16 */
#define SPH_MODES_W_ONE      0            /* base = 1 */
#define SPH_MODES_W_MASS     1            /* base = m */
#define SPH_MODES_LOG        1            /* logarithmic ring edges (r_min > 0) */
typedef struct sph_modes_desc {
    double  centre[3], centre_v[3]; /* frame origin and its velocity (ignored when sink >= 0)                  */
    double  normal[3];              /* disc normal, any length > 0                                             */
    double  r_min, r_max;           /* ring range [r_min, r_max)                                               */
    double  z_max;                  /* strict |z'| < z_max; INFINITY = none                                    */
    double  p_min, p_max;           /* the spiral wavenumbers' range (n_p > 0)                                 */
    double  r_ref;                  /* u = log(R / r_ref), > 0 (n_p > 0)                                       */
    int32_t n_r;                    /* rings, 1 .. SPH_MODES_MAX_RINGS                                         */
    int32_t m_max;                  /* 0 .. SPH_MODES_MAX_M                                                    */
    int32_t n_p;                    /* spiral wavenumbers, 0 (no spiral sums) .. SPH_MODES_MAX_P               */
    int32_t sink;                   /* >= 0: the centre is that sink's position; -1: none                      */
    int32_t weight;                 /* SPH_MODES_W_*                                                           */
    int32_t n_q;                    /* 0: A = 1; 1: A = the quantity q                                         */
    int32_t q;                      /* its source: SPH_F_* or SPH_MODES_ROW(k)                                 */
    int32_t n_rows;                 /* rows of values, 0 .. 16                                                 */
    int32_t flags;                  /* SPH_MODES_LOG                                                           */
    int32_t reserved[3];            /* must be 0                                                               */
} sph_modes_desc;                   /* 168 bytes */
int sph_modes(sph_ctx *ctx, const sph_modes_desc *d, const double *values, double *host_sums, int64_t n_out, uint64_t *host_raw,
              int32_t *exp, int64_t *ring_counts, int64_t *counts);
int sph_modes_dev(sph_ctx *ctx, const sph_modes_desc *d, const double *d_values, double *d_sums, int64_t n_out, uint64_t *d_raw,
                  int32_t *d_exp, int64_t *d_ring_counts, int64_t *d_counts);
int sph_modes_tables(const sph_modes_desc *d, double *edges_out, double *p_out);
int sph_modes_finish(const sph_modes_desc *d, const int32_t *exp, const uint64_t *raw, double *sums);

/* ---- history: a per-step time series recorded on the device (the dt every step chose, the accreted counts, the sinks'
 *      orbits and masses, the peak density, the conserved totals) ---------------------------------------------------------
 * A device-resident log of `capacity` rows of doubles.  Between sph_history_begin and sph_history_end every step of
 * sph_step / sph_run whose running number is a multiple of `every` appends one row, at the very end of the step (after the
 * h update, sink creation and accretion / cull): the row describes what sph_download_state would return after that step.
 * The rows are written by kernels on the context's stream; a recorded step adds no stream synchronisation and no host
 * read-back.  The row index, the step number and the dropped count are kept on the host.  A full log drops further rows
 * and counts them (no wrap-around).  Without a history the step is exactly what it is without this section: no kernel, no
 * argument and no allocation differ.  The native multi-rank loop (summersph_halo.h) does not record.
 * Step     steps are counted since sph_history_begin, the unrecorded ones included.  sph_history_record appends a row for
 *          the state as it is now without advancing the number: the t = 0 row, or a row after explicit sph_density /
 *          sph_forces / sph_kick / sph_drift calls; sph_upload keeps the history and its numbers.
 * Row      width = SPH_HISTORY_NHEAD + 7 max_sinks doubles:
 *           0      the step number
 *           1-3    the device's time words after the step: t, the next dt, the dt candidate
 *           4, 5   owned gas particles (original ids < n_owned), sinks
 *           6-33   sph_energy's sums[0..28), same indices, same per-term arithmetic in the same order, no fused
 *                  multiply-adds: capi.energy_total(row[6:34]) works.  Entry 6 + 13 (W_self) is 0: the history walks no
 *                  tree; take sph_energy at snapshots for it.
 *           34     rho_max over the owned gas (NaN densities are passed over); NaN where the context's density is not
 *                  current (sph_download_field would refuse rho, e.g. sph_history_record after a drift) or no gas is held
 *           35-38  the densest particle: its index in sph_download_field order, and x, y, z; ties go to the lowest index;
 *                  NaN where 34 is
 *           39     max |v| = sqrt(max((vx vx + vy vy) + vz vz)); 0 without gas, NaN where a velocity is NaN
 *           40 + 7 s ..  sink s < min(ns, max_sinks): x, y, z, vx, vy, vz, m; NaN for s >= ns
 * Exact    the gas sums 1 .. 12 and 14 (row 7 .. 18 and 20) are exact sums of sph_energy's fp64 terms: with B = max |term|
 *          of a sum and e the exponent with B < 2^e (0 for B = 0), every term is rounded half-even to a multiple of
 *          2^(e - 62), the integers are added in 128 bits and the total is rounded to a double once (sph_pairs' arithmetic).
 *          The result is defined by these rules alone: it does not depend on the sorted order, the grid kind, the block
 *          count or the launch, and it differs from the real sum by at most N 2^(e - 63) plus the final rounding.  A sum
 *          with a non-finite term is NaN; the other sums are unaffected.  N (row 6) is a plain count.
 *          Rows 4 and 6 (n and N) are the host's owned count (sph_set_owned; sph_count without ghosts), not a count of the
 *          slots the passes ran over: the passes take the slots whose original id is in [0, n_owned), which are exactly
 *          that many between steps.
 * Sinks    row 21 .. 33: sph_energy's sink part, the same arithmetic bit for bit, on rank 0 only (sph_set_rank).
 * read     sph_history_read copies rows [first, first + count) to the host: it synchronises the stream and then reports
 *          what sph_get_dt reports (a list overflow or a non-finite position of the last build).  sph_history_read_dev
 *          copies to device memory in the stream's order without waiting.  The host form's wait is not counted in
 *          sph_stats.host_syncs, which counts the waits inside the build path only (sph_get_dt's and the downloads' are
 *          not counted either).  sph_history_info: the rows held, the rows
 *          dropped, the steps counted and the row width (null outputs are skipped).
 * cost     four launches per recorded row: two coalesced passes over the sorted state and two single blocks.  The log
 *          and about 0.4 MB of partials are counted in device_bytes from begin to end.
 * SPH_ERR_STATE: record, info, read or end without begin.  SPH_ERR_ARG: a null descriptor, capacity < 1, every < 1, max_sinks
 * outside 0 .. 64, flags != 0, a null output of a read of count > 0 rows, first or count outside [0, rows]. */
typedef struct sph_history_desc {
    int32_t capacity;   /* rows the log holds (>= 1)                                           */
    int32_t every;      /* record the steps whose running number is a multiple of this (>= 1)  */
    int32_t max_sinks;  /* per-sink columns kept per row (0 .. 64)                             */
    int32_t flags;      /* 0; reserved                                                         */
} sph_history_desc;     /* 16 bytes */
#define SPH_HISTORY_NHEAD 40                    /* row width = NHEAD + 7 * max_sinks doubles   */
int sph_history_begin(sph_ctx *ctx, const sph_history_desc *d);   /* allocate, rows = 0, step number = 0; a second begin replaces the first */
int sph_history_end(sph_ctx *ctx);                                /* free; steps record nothing again */
int sph_history_record(sph_ctx *ctx);
int sph_history_info(sph_ctx *ctx, int64_t *rows, int64_t *dropped, int64_t *steps, int32_t *width);
int sph_history_read(sph_ctx *ctx, int64_t first, int64_t count, double *host_out);
int sph_history_read_dev(sph_ctx *ctx, int64_t first, int64_t count, double *d_out);

/* ---- track: trajectories and fates of chosen particles, recorded on the device (where the gas of a fragment came from, the
 *      thermal history of gas that passes a shock, which particles a sink swallowed and when) --------------------------------
 * A tracking set is n_ids caller-order ids (indices of sph_download_* at the time of sph_track_begin).  Each id names one
 * particle for the lifetime of the tracker, whatever happens to the numbering afterwards: the sorted order changes at every
 * grid build, and the caller's numbering at every accretion or cull (the survivors are renumbered by rank).  Between
 * sph_track_begin and sph_track_end every step of sph_step / sph_run whose running number is a multiple of `every` appends
 * one row at the very end of the step, beside sph_history's row and independent of it: one launch on the context's stream,
 * no stream synchronisation, no host read-back; the live count stays on the device.  A full log drops further rows and counts
 * them.  Without a tracker the step and the accretion pack are exactly what they are without this section: no kernel, no
 * argument, no allocation and no synchronisation differ.
 * Row      head: SPH_TRACK_NHEAD doubles: the step number (steps are counted since begin, the unrecorded ones included),
 *          t (the device's time word, as sph_history's column 1), the owned gas count, the tracked particles still alive.
 *          body: SPH_TRACK_NCOL values per tracked particle, x y z vx vy vz u rho h alpha, laid out [column][k] with k the
 *          index into the ids as given at begin: body is (rows, SPH_TRACK_NCOL, n_ids) in C order, sph_trace's path shape,
 *          and one quantity of all tracked particles is contiguous.  A value is bit for bit what sph_download_state /
 *          sph_download_field would return for that particle at that moment; rho is NaN where sph_download_field would
 *          refuse SPH_F_RHO (sph_history's rule), h is the context's smoothing length with fixed h.
 *          A particle that has been removed is NaN in every later row (the log is filled with NaN once, at begin).
 * Fates    four int32 per tracked particle, {fate, step, sink, current_id}: fate 0 alive, 1 accreted, 2 culled (outside the
 *          bound); step the tracker's count of completed steps at the moment of removal, so that the particle is finite
 *          only in rows whose step number is <= it; sink the index of the sink whose sums took its mass (the lowest
 *          index where the accretion marked it for several, which all take it), -1 unless accreted; current_id its index
 *          in today's caller order (sph_download_* at that index is this particle), -1 once it is gone.  A particle both
 *          marked by a sink and outside the bound counts as accreted.
 * record   sph_track_record appends a row of the state as it is now without advancing the step number (the t = 0 row, or a
 *          row after an explicit sph_accrete_and_cull).
 * Scope    one rank, no ghosts: begin returns SPH_ERR_STATE where nranks > 1 or n_owned != n.  sph_upload, sph_upload_dev,
 *          sph_set_owned, sph_replace_ghosts_dev, sph_set_rank with nranks > 1 and sph_accrete_apply_dev *close* the
 *          tracker: the ids mean nothing in a new state, and a silently wrong trajectory is worse than a short one.  A
 *          closed tracker records nothing more (steps go on and are not counted; sph_track_record returns SPH_ERR_STATE);
 *          its rows and fates stay readable until sph_track_end.  sph_upload_field keeps the numbering and the tracker.
 * read     sph_track_read copies rows [first, first + count) to the host, the heads to head (count x SPH_TRACK_NHEAD) and
 *          the bodies to body (count x SPH_TRACK_NCOL x n_ids); either pointer may be null.  It synchronises the stream and
 *          then reports what sph_get_dt reports.  sph_track_fates copies 4 n_ids int32 and synchronises.  The _dev forms
 *          copy to device memory in the stream's order without waiting.  sph_track_begin_dev takes the ids from device
 *          memory; both forms of begin check the ids on the host and may wait for the stream.  sph_track_info: the rows held
 *          and dropped, the steps counted, n_ids, the live count and whether the tracker is closed (null outputs are
 *          skipped); asking for n_live reads the device's count and synchronises.  None of these waits is counted in
 *          sph_stats.host_syncs.
 * cost     one launch per recorded row: a pass over the sorted order's 4-byte ids with a bit test, ten gathers per hit.  A
 *          pack that removed particles adds five small launches (the fates, and the bitmap, prefix and tags rebuilt); a pack
 *          that removed nobody adds none.  The log (capacity x (4 + 10 n_ids) doubles), n / 8 bytes of bitmap, n / 16 of
 *          prefix and 20 n_ids bytes are counted in device_bytes from begin to end.
 * SPH_ERR_STATE: record, info, read, fates or end without begin; begin with several ranks or ghosts; record on a closed
 * tracker.  SPH_ERR_ARG: a null descriptor, capacity < 1, every < 1, flags != 0, n_ids < 1, null ids, an id outside [0, n),
 * an id given twice, first or count outside [0, rows], a null fates output.  SPH_ERR_NOMEM: the log does not fit. */
typedef struct sph_track_desc {
    int64_t capacity;   /* rows the log holds (>= 1)                                           */
    int32_t every;      /* record the steps whose running number is a multiple of this (>= 1)  */
    int32_t flags;      /* 0; reserved                                                         */
} sph_track_desc;       /* 16 bytes */
#define SPH_TRACK_NHEAD 4                       /* step, t, owned gas count, tracked particles alive */
#define SPH_TRACK_NCOL 10                       /* x y z vx vy vz u rho h alpha                      */
int sph_track_begin(sph_ctx *ctx, const sph_track_desc *d, int64_t n_ids, const int64_t *ids);   /* a second begin replaces the first */
int sph_track_begin_dev(sph_ctx *ctx, const sph_track_desc *d, int64_t n_ids, const int64_t *d_ids);
int sph_track_end(sph_ctx *ctx);
int sph_track_record(sph_ctx *ctx);
int sph_track_info(sph_ctx *ctx, int64_t *rows, int64_t *dropped, int64_t *steps, int64_t *n_tracked, int64_t *n_live,
                   int32_t *closed);
int sph_track_read(sph_ctx *ctx, int64_t first, int64_t count, double *host_head, double *host_body);
int sph_track_read_dev(sph_ctx *ctx, int64_t first, int64_t count, double *d_head, double *d_body);
int sph_track_fates(sph_ctx *ctx, int32_t *host_fates);
int sph_track_fates_dev(sph_ctx *ctx, int32_t *d_fates);

/* ---- dust: drag-coupled tracer grains advanced with the run (where a mm grain goes, compared with a micron grain: into the
 *      arms and clumps, onto a sink, out of the disc) ----------------------------------------------------------------------
 * A dust set is M massless test grains on the device, each with a position, a velocity and one drag parameter par.  The
 * grains feel the sinks' gravity and the drag of the SPH-interpolated gas and act on nothing: the gas run with grains is
 * bitwise the gas run without them.  Between sph_dust_begin and sph_dust_end every step of sph_step / sph_run whose running
 * number (counted since begin) is a multiple of `every` advances all live grains from their own clock t_d to the gas clock
 * t (the device's time word), at the very end of the step, after sph_history's, sph_track's and sph_frames' rows: a few
 * launches on the context's stream, no stream synchronisation, no host read-back.  Without dust the step is exactly what it
 * is without this section: no kernel, no argument, no allocation and no synchronisation differ.
 * Scheme   kick-drift-kick with exact drag and one gas evaluation per advance.  Each grain keeps the sample S = (a[3], vg[3],
 *          r) of the end of its last advance: the sinks' acceleration, the gas velocity and the drag rate r = 1 / t_s at
 *          the grain.  With D = t - t_d an advance does, in this order and without fused multiply-adds:
 *          1 half kick with the stored S: tau = D / 2, k = r tau; where k > 0: e = -expm1(-k) and
 *            v <- (v + (vg - v) e) + a (tau (e / k)), the exact solution of dv/dt = a - r (v - vg) with a, vg and r frozen
 *            (finite however stiff the drag; k -> infinity gives the terminal velocity vg + a / r); where r == 0:
 *            v <- v + a tau.
 *          2 drift: x <- x + v D.
 *          3 fates, with SPH_DUST_REMOVE only: the sinks in sink order, the first with |x - R_s| < radius_s (Euclidean,
 *            sph_set_sink_radii's radii) takes the grain, fate 1; otherwise any |x_k| > params.bounding_size is fate 2.
 *            With or without the flag a non-finite x or v is fate 3.  A grain with a fate stops here.
 *          4 the gas at the new x in the state the step just left: sph_sample's sums den, num[0..3] over the owned gas,
 *            mass-weighted, fields vx vy vz u, no clip box, desc.h = 0.  rho = den, vg = num[0..2] / den, u = num[3] / den,
 *            c = sqrt((gamma gamma_m1) u).  Where den == 0: r = 0 and vg = 0 (and u = 0).  Otherwise
 *            SPH_DUST_EPSTEIN: r = ((rho c) cE) / (rho_grain par) with par the grain size and cE = sqrt(8 / pi) in double;
 *            SPH_DUST_FIXED_TS: r = 1 / par with par the stopping time.
 *            The sinks' a in sink order with sph_gravity_at's arithmetic (its "Sinks" paragraph), unsoftened.
 *          5 the second half kick, step 1's formula with the new S.  A grain whose v or a is not finite now (a grain
 *            placed exactly on a massive sink), and every grain if a gas particle has a bad h (sph_sample would return
 *            NaN), is fate 3.
 *          6 S is stored, t_d = t, and the row is appended if this advance is one to record.
 *          Where D <= 0 or D is not finite (after a sph_set_dt that moved t back) only steps 4 to 6 run, without the kick:
 *          nothing moves.  sph_dust_begin does that once (advance number 0, no row), so that S exists before the first
 *          step; it may wait for the stream.
 * Order    one lane per grain adds its sources in sph_sample's documented order.  The grains are walked in the order of
 *          their cells, which is a matter of speed only: a grain's result depends on the gas, the sinks, its own x, v,
 *          par, S and D alone, not on the other grains, M, the walk order, the gas's sorted order or the kind of cell grid.
 * Row      head: SPH_DUST_NHEAD doubles: the advance number (advances are counted since begin, from 1, the explicit ones
 *          included), t, the D of this advance, the grains alive after it.  body: SPH_DUST_NCOL values per grain, x y z vx
 *          vy vz rho_g u_g vgx vgy vgz rate, laid out [column][p]: body is (rows, SPH_DUST_NCOL, M) in C order, sph_track's
 *          shape.  rho_g, u_g and vg are bitwise what sph_sample returns at (x, y, z) with fields vx vy vz u, normalised,
 *          and its weight output.  A grain with a fate is NaN in the row of that advance and in every later row (the log is
 *          filled with NaN once, at begin).  A step-driven advance appends a row where the count of step-driven advances is a
 *          multiple of record_every; sph_dust_advance always appends one.  A full log drops further rows and counts them.
 * Fates    three int32 per grain, {fate, advance, sink}: fate 0 alive, 1 accreted, 2 culled, 3 non-finite; the number of the
 *          advance that removed it; the sink that took it (-1 unless accreted).
 * advance  sph_dust_advance advances to the clock now, outside a step, and appends a row; the first call after begin (D = 0)
 *          is the t = 0 row.
 * Scope    one rank, no ghosts: begin returns SPH_ERR_STATE where nranks > 1 or n_owned != n.  The gas's self-gravity does
 *          not act on the grains.  Grains are not gas ids: sph_upload keeps them, they are sampled against the new gas.
 *          sph_set_owned, sph_replace_ghosts_dev and sph_set_rank with nranks > 1 *close* the dust: no further advance
 *          (sph_dust_advance returns SPH_ERR_STATE); rows, state and fates stay readable until sph_dust_end.
 * read     sph_dust_read copies rows [first, first + count) to the host, the heads to head (count x SPH_DUST_NHEAD) and the
 *          bodies to body (count x SPH_DUST_NCOL x M); either pointer may be null.  sph_dust_state copies the seven arrays
 *          x y z vx vy vz par as they are now (a removed grain keeps its last values), so that grains can be saved and begun
 *          again; sph_dust_fates copies 3 M int32.  The host forms synchronise the stream; the _dev forms copy to device
 *          memory in the stream's order without waiting.  sph_dust_begin_dev takes the arrays from device memory; both forms
 *          of begin check par on the host.  sph_dust_info: the rows held and dropped, the advances counted, M and the live
 *          count (null outputs are skipped); asking for n_live reads the device's count and synchronises.  None of these
 *          waits is counted in sph_stats.host_syncs.
 * cost     an advance is one sample_build over the gas, a launch over the grains, a radix sort of M pairs, the walk and a
 *          one-lane launch.  The log (capacity x (4 + 12 M) doubles), 16 M doubles of state and sample and 12 M bytes of fates
 *          are counted in device_bytes from begin to end; the advance works in the analysis scratch and keeps nothing there.
 * SPH_ERR_STATE: advance, info, read, state, fates or end without begin; begin with several ranks or ghosts; advance on closed
 * dust.  SPH_ERR_ARG: a null descriptor, M < 1, null arrays, capacity < 0, every < 1, record_every < 1, an unknown law or
 * flags, a par <= 0 or not finite, rho_grain <= 0 or not finite with SPH_DUST_EPSTEIN, first or count outside [0, rows], a
 * null output.  SPH_ERR_NOMEM: the log does not fit. */
typedef struct sph_dust_desc {
    int64_t capacity;      /* rows the log holds (>= 0; 0: no log, state and fates only)                       */
    int32_t every;         /* advance at the steps whose running number is a multiple of this (>= 1)           */
    int32_t record_every;  /* append a row at every record_every-th advance (>= 1)                             */
    int32_t law;           /* SPH_DUST_EPSTEIN | SPH_DUST_FIXED_TS                                             */
    int32_t flags;         /* SPH_DUST_REMOVE                                                                  */
    double  rho_grain;     /* > 0 with EPSTEIN (mass / length^3 in code units); unused otherwise               */
} sph_dust_desc;           /* 32 bytes */
#define SPH_DUST_EPSTEIN 0
#define SPH_DUST_FIXED_TS 1
#define SPH_DUST_REMOVE 1
#define SPH_DUST_NHEAD 4   /* advance number, t, D of this advance, grains alive */
#define SPH_DUST_NCOL 12   /* x y z vx vy vz rho_g u_g vgx vgy vgz rate */
int sph_dust_begin(sph_ctx *ctx, const sph_dust_desc *d, int64_t m, const double *x, const double *y, const double *z,
                   const double *vx, const double *vy, const double *vz, const double *par);   /* a second begin replaces the first */
int sph_dust_begin_dev(sph_ctx *ctx, const sph_dust_desc *d, int64_t m, const double *d_x, const double *d_y, const double *d_z,
                       const double *d_vx, const double *d_vy, const double *d_vz, const double *d_par);
int sph_dust_end(sph_ctx *ctx);
int sph_dust_advance(sph_ctx *ctx);
int sph_dust_info(sph_ctx *ctx, int64_t *rows, int64_t *dropped, int64_t *advances, int64_t *n_grains, int64_t *n_live);
int sph_dust_read(sph_ctx *ctx, int64_t first, int64_t count, double *host_head, double *host_body);
int sph_dust_read_dev(sph_ctx *ctx, int64_t first, int64_t count, double *d_head, double *d_body);
int sph_dust_state(sph_ctx *ctx, double *x, double *y, double *z, double *vx, double *vy, double *vz, double *par);
int sph_dust_state_dev(sph_ctx *ctx, double *d_x, double *d_y, double *d_z, double *d_vx, double *d_vy, double *d_vz, double *d_par);
int sph_dust_fates(sph_ctx *ctx, int32_t *host_fates);
int sph_dust_fates_dev(sph_ctx *ctx, int32_t *d_fates);

/* ---- frames: a device-resident movie of a run -- line-of-sight-integrated maps of the owned gas appended from the end of
 *      the step, and the same map as a one-shot call (summersph_amd/frames.py) ------------------------------------------
 * Between sph_frames_begin and sph_frames_end the steps of sph_step / sph_run append frames to a log of `capacity` rows, at
 * the very end of the step, after sph_history's and sph_track's rows and independent of them.  The frame's kernels run on
 * the context's stream; a recorded step adds no stream synchronisation and no host read-back.  Without frames begun the
 * step is exactly what it is without this section: no kernel, no argument and no allocation differ.  The recorder only
 * reads the state and names no particle: it survives accretion, culls and a new upload.  One context (several ranks'
 * frames are not combined here).
 * Frame, Select, Nodes  exactly sph_cube's: rot[9] with rows u^, v^, w^ (orthonormal and right-handed within 1e-12, else
 *          SPH_ERR_ARG); P_j = rot (r_j - C), every row evaluated as ((a0 dx + a1 dy) + a2 dz) with no fused multiply-adds;
 *          the owned gas particles with clip_lo < r < clip_hi on every axis of the SIMULATION frame (strict); h > 0: one h
 *          for every particle, 0: each particle's own; node i on image axis a is lo[a] + i (hi[a] - lo[a]) / (n - 1), the
 *          last one exactly hi[a] (np.linspace), n == 1: the single node lo[a]; nodes are point-sampled.
 * Centre   C = centre, or with centre_sink >= 0 centre[a] + the position of that sink at the time of the frame, read on the
 *          device.  A sink index >= the current sink count: every plane of that frame is NaN and the head's status is
 *          SPH_FRAMES_SINK_GONE.
 * Planes   plane 0 is the column density, planes 1 .. nq (nq <= SPH_FRAMES_MAX_FIELDS) the same sum weighted by the context's
 *          field fields[k - 1] (an SPH_F_* id).  The term of particle j at node g, with p = sqrt(du du + dv dv) / h_j, du and
 *          dv the node's coordinates minus P_j,u and P_j,v, is (y0_j A_j) F(p) for p < 2 and nothing otherwise:
 *          y0_j = m_j / (pi (h_j h_j)), pi in double precision (sph_transfer's y0 with kappa = 1); A_j = 1 for plane 0 and
 *          the field's value otherwise; F the line-integrated spline of sph_cube ("Footprint" above), F <= F(0) = 1.5.  No
 *          fused multiply-adds.  A field that sph_download_field would refuse at that moment makes its plane NaN for that
 *          frame and leaves the others alone (sph_history's rule for rho).
 * Sum      per plane, B = max |y0_j A_j| over the SELECTED particles (whether or not they reach a node) and e the exponent
 *          with 1.5 B < 2^e (0 for B = 0).  Every term is rounded half-even to a multiple of 2^(e - 62), the integers are
 *          added in 128 bits and each node is rounded to a double once (sph_pairs' arithmetic).  A selected particle whose
 *          1.5 y0 A is not finite makes that plane of that frame NaN.  A frame is therefore a function of the descriptor
 *          and the selected particles' values alone: bitwise the same for any slot order, upload order, grid kind, launch
 *          shape, binning and repetition, and it differs from the real-number sum of the fp64 terms by at most
 *          (terms on that node) 2^(e - 63) plus the final rounding.
 * Head     SPH_FRAMES_NHEAD doubles per frame: 0 the step number (steps are counted since begin, the unrecorded ones
 *          included; sph_frame: the count of the log that is begun, else 0); 1 t, the device's time word; 2 the owned gas
 *          count; 3 the selected count; 4-6 C; 7-10 the planes' exponents e (NaN for a plane that is unused or NaN);
 *          11 the status (SPH_FRAMES_OK, SPH_FRAMES_SINK_GONE); 12-15 zero.
 * Log      planes: capacity x (1 + nq) x n_u x n_v doubles in C order [row][plane][iu][iv]; heads: capacity x 16.  A full
 *          log drops further frames and counts them.  sph_frames_rewind sets the row count to 0 and keeps the allocation,
 *          the step number, the cadence counter and the dropped count: a long movie is drained between sph_run chunks.
 * Cadence  every >= 1 with dt_frame == 0: the steps whose running number is a multiple of `every`, decided on the host as
 *          sph_history does.  dt_frame > 0 with every == 0: uniform in simulation time, the reference's save rule, decided
 *          on the device, where t lives during sph_run: with t0 the context's t at begin and k starting at 1, a step that
 *          ends at time t records a frame iff t >= t0 + k dt_frame (product, then sum, in double), and afterwards
 *          k = floor((t - t0) / dt_frame) + 1 -- at most one frame per step, missed thresholds are skipped.  In this mode
 *          the frame's launches are enqueued every step and return at once when no frame is due.  The due decision, the row
 *          index and the dropped count are device words in both modes; sph_frames_info is the only call that reads them
 *          back (it synchronises; null outputs are skipped, and asking for steps alone does not wait).
 * record   sph_frames_record appends a frame of the state as it is now, whatever the cadence, without advancing the step
 *          number or the cadence counter.
 * read     sph_frames_read copies rows [first, first + count) to the host (either pointer may be null): it reads the row
 *          count, synchronises and reports what sph_get_dt reports.  sph_frames_read_dev copies to device memory in the
 *          stream's order without waiting; it cannot know the row count, so its range is checked against the capacity.
 * One-shot sph_frame / sph_frame_dev: the frame of the state as it is now into head (16 doubles) and planes (out_len ==
 *          (1 + nq) n_u n_v doubles), by the same kernels on the analysis scratch; capacity, every and dt_frame are not
 *          read.  sph_frame_dev makes no stream synchronisation and no read-back; sph_frame synchronises once, for its
 *          copies.  Neither of them touches a log that is begun.
 * cost     five launches per frame: two passes over the sorted state, the clear and the conversion of the image, one
 *          block.  The log, 32 (1 + nq) n_u n_v bytes of limbs and about 50 kB are counted in device_bytes from begin to end.
 * SPH_ERR_ARG: a null descriptor or output, reserved != 0, n_u or n_v < 1, nq outside 0 .. 3, an unknown field id, h < 0 or
 * non-finite, lo > hi or non-finite, a NaN clip, a non-finite centre, a bad rot, centre_sink >= 64, capacity < 1, neither
 * cadence or both (every < 0 and a negative or non-finite dt_frame included), out_len != (1 + nq) n_u n_v, first or count
 * outside the rows.  SPH_ERR_STATE: record, rewind, info, read or end without begin.  SPH_ERR_NOMEM: (1 + nq) n_u n_v above
 * 2^28, or the log does not fit. */
#define SPH_FRAMES_MAX_FIELDS 3
#define SPH_FRAMES_NHEAD 16
#define SPH_FRAMES_OK 0
#define SPH_FRAMES_SINK_GONE 1
typedef struct sph_frames_desc {
    double  rot[9];                 /* rows u^, v^, w^ (row-major)                                   */
    double  centre[3];              /* origin of the image plane (added to the sink's position)      */
    double  lo[2], hi[2];           /* node box on the image axes u, v                               */
    double  clip_lo[3], clip_hi[3]; /* strict particle clip box (simulation axes); -/+INFINITY = none */
    double  h;                      /* > 0: one h for all; 0: each particle's own h                  */
    double  dt_frame;               /* > 0: a frame every dt_frame of simulation time; 0: `every`    */
    int64_t capacity;               /* frames the log holds (>= 1)                                   */
    int32_t n_u, n_v;               /* image nodes per axis, each >= 1                               */
    int32_t every;                  /* >= 1: every every-th step; 0 with dt_frame > 0                */
    int32_t centre_sink;            /* >= 0: the frame follows this sink; < 0: none                  */
    int32_t nq;                     /* weighted planes, 0 .. 3                                       */
    int32_t fields[SPH_FRAMES_MAX_FIELDS]; /* their SPH_F_* ids                                      */
    int64_t reserved;               /* must be 0                                                     */
} sph_frames_desc;                  /* 240 bytes */
int sph_frames_begin(sph_ctx *ctx, const sph_frames_desc *d);     /* allocate, rows = 0, step number = 0, t0 = t; a second begin replaces the first */
int sph_frames_end(sph_ctx *ctx);
int sph_frames_record(sph_ctx *ctx);
int sph_frames_rewind(sph_ctx *ctx);
int sph_frames_info(sph_ctx *ctx, int64_t *rows, int64_t *dropped, int64_t *steps);
int sph_frames_read(sph_ctx *ctx, int64_t first, int64_t count, double *host_head, double *host_planes);
int sph_frames_read_dev(sph_ctx *ctx, int64_t first, int64_t count, double *d_head, double *d_planes);
int sph_frame(sph_ctx *ctx, const sph_frames_desc *d, double *host_head, double *host_planes, int64_t out_len);
int sph_frame_dev(sph_ctx *ctx, const sph_frames_desc *d, double *d_head, double *d_planes, int64_t out_len);

/* ---- diagnostics / measurement -------------------------------------------------------- */
int sph_get_stats(sph_ctx *ctx, sph_stats *out);
/* the cell grid of the last build: dense (one table entry per cell of the box) or hashed (SPH_FLAG_HASHED_GRID, or a box too
 * sparse for the dense table: the occupied cells in a hash table).  Reads the occupied-cell count back (synchronises).   */
typedef struct sph_grid_info {
    int32_t kind;             /* 0 dense, 1 hashed, -1 no grid built yet                                  */
    int32_t dim[3];           /* cells along x, y, z                                                      */
    int64_t occupied_cells;   /* cells holding particles (dense: every cell of the table)                 */
    int64_t table_entries;    /* dense: cells + 1; hashed: hash table slots (a power of two >= 4 capacity) */
    double  index_cells;      /* dim[0] dim[1] dim[2]: the cells the keys address                         */
    int64_t bytes;            /* device bytes of the cell table (hashed: keys, sort, cells, table)         */
} sph_grid_info;
int sph_get_grid_info(const sph_ctx *ctx, sph_grid_info *out);
/* bounding box of the particle positions at the last grid build (= the current positions
 * after sph_density / sph_step): lo[3], hi[3].  Serves check_bounds ([F]:471-482) without a
 * download.                                                                              */
int sph_get_bbox(sph_ctx *ctx, double *lo, double *hi);
/* HIP events around kernel groups: on = 0 none, 1 every group, else a mask with bit (k + 1) set for sph_kernel_id k (timing
 * one group costs two event records per launch of that group; timing all of them ~4 % of a fixed-h step)                */
int sph_timing_enable(sph_ctx *ctx, int on);
/* bracket only every stride-th launch of a timed group (default 1): an event pair costs the stream ~14 us, so a run that is
 * itself being timed samples its dominant kernel instead of bracketing every launch; sph_timing_get then returns the
 * bracketed launches and their total                                                                                      */
int sph_timing_stride(sph_ctx *ctx, int stride);
int sph_timing_reset(sph_ctx *ctx);
int sph_timing_get(sph_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
int sph_synchronize(sph_ctx *ctx);
/* the HIP stream all kernels of this context are launched on (hipStream_t as void*)      */
void *sph_stream(sph_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* SUMMERSPH_H */
