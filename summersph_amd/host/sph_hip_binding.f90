! sph_hip_binding.f90 -- ISO_C_BINDING view of include/summersph.h (libsummersph_hip.so).
!
! This is the stub a maintainer of the reference adds to call the MI355X core from
! Fortran: one `bind(C)` interface per C entry point, plus the parameter struct.  Each
! interface names the reference procedure it stands in for (file SUMMER_SPH.f90).
module sph_hip_binding
  use, intrinsic :: iso_c_binding
  implicit none
  private
  public :: sph_params, sph_stats
  public :: sph_params_default, sph_ctx_create, sph_ctx_destroy, sph_strerror, sph_last_error, sph_abi_version, sph_get_params
  public :: sph_upload, sph_set_sinks, sph_get_sinks, sph_count
  public :: sph_density, sph_forces, sph_kick, sph_drift, sph_next_dt, sph_step, sph_run
  public :: sph_download_field, sph_download_state, sph_get_stats, sph_get_bbox, sph_synchronize
  public :: SPH_OK, SPH_F_X, SPH_F_Y, SPH_F_Z, SPH_F_VX, SPH_F_VY, SPH_F_VZ, SPH_F_U, SPH_F_M, SPH_F_ALPHA
  public :: SPH_F_RHO, SPH_F_P, SPH_F_C, SPH_F_AX, SPH_F_AY, SPH_F_AZ, SPH_F_DU, SPH_F_DALPHA
  public :: sph_set_sink_radii, sph_accrete_and_cull, sph_upload_field, sph_update_h, sph_params_default_variable
  public :: SPH_F_H, SPH_F_OMEGA
  public :: SPH_FLAG_REUSE_DENSITY, SPH_FLAG_VARIABLE_H, SPH_FLAG_SELF_GRAVITY, SPH_FLAG_ACCRETE_CULL
  public :: SPH_FLAG_SINK_CREATION, sph_sink_count, sph_get_sink_radii
  ! cell grid: the hashed table (far-apart particle groups) and what the last build used
  public :: SPH_FLAG_HASHED_GRID, sph_grid_info, sph_get_grid_info
  ! multi-GPU building blocks (device pointers as type(c_ptr), e.g. from hipMalloc or an MPI library's GPU buffers)
  public :: sph_set_owned, sph_set_rank, sph_reserve, sph_owned_bbox, sph_select_boxes, sph_selected_ids_dev
  public :: sph_select_boxes_async, sph_selected_counts, sph_gather_selected_dev
  public :: sph_replace_ghosts_dev, sph_gather_fields_dev, sph_scatter_fields_dev, sph_refresh_eos_ghosts
  public :: sph_set_boundary_boxes, sph_forces_part, sph_set_dt, sph_get_dt, sph_kick_devdt, sph_drift_devdt
  public :: sph_kick_drift_devdt, sph_kick_dt_candidate_dev, sph_kick_dt_candidate_gas_dev, sph_kick_sinks_devdt
  public :: sph_dt_candidate_dev, sph_pack_partials_dev, sph_pack_partials_ex_dev, sph_apply_partials_dev, sph_set_gravity_sources_dev
  public :: SPH_PARTIALS
  ! density rendering (Density_Image.py's grid loop and projection)
  public :: sph_render_desc, sph_render_density, sph_render_density_dev, SPH_RENDER_AUTO_BOUNDS, SPH_RENDER_SPACING
  ! field rendering (any per-particle quantity: temperature, moment-1 velocity, alpha maps ...)
  public :: sph_render_field_desc, sph_render_field, sph_render_field_dev
  public :: SPH_RENDER_FIELD_VALUES, SPH_RENDER_WEIGHT_MASS, SPH_RENDER_WEIGHT_VOLUME
  ! disc profiles (binned mass-weighted moments in rings about a centre, and their derived table)
  public :: sph_profile_desc, sph_profile, sph_profile_dev, sph_profile_finish
  public :: SPH_PROFILE_LOG, SPH_PROFILE_AUTO_NORMAL, SPH_PROFILE_NSUM, SPH_PROFILE_NCOL
  ! conserved totals and the gravitational potential (energy, momentum, angular momentum; phi per particle)
  public :: sph_energy, sph_energy_dev, SPH_ENERGY_NSUM
  ! friends-of-friends groups (clumps of the owned gas: labels per particle and a table per group)
  public :: sph_groups_desc, sph_groups, sph_groups_dev, SPH_GROUPS_LINK_H, SPH_GROUPS_NCOL
  ! density-peak clumps (basins of the density field merged across high saddles: labels, a table per clump, counts)
  public :: sph_peaks_desc, sph_peaks, sph_peaks_dev, SPH_PEAKS_LINK_H, SPH_PEAKS_NCOL, SPH_PEAKS_NCOUNT
  ! SPH gradients (standard or matrix-corrected) of up to four fields at the owned gas
  public :: sph_gradients_desc, sph_gradients, sph_gradients_dev, SPH_GRAD_CORRECTED, SPH_GRAD_MAX_FIELDS, SPH_GRAD_VALUES
  ! SPH interpolation at arbitrary points (density, fields or the caller's values where the caller wants them)
  public :: sph_sample_desc, sph_sample, sph_sample_dev, SPH_SAMPLE_NORMALISE, SPH_SAMPLE_MAX_FIELDS, SPH_SAMPLE_VALUES
  ! field lines of an SPH-interpolated vector field (streamlines of the velocity, in a rotating frame if wanted)
  public :: sph_trace_desc, sph_trace, sph_trace_dev, SPH_TRACE_ARCLENGTH, SPH_TRACE_PLANAR, SPH_TRACE_VALUES, SPH_TRACE_NONE
  public :: SPH_TRACE_DONE, SPH_TRACE_LEFT_GAS, SPH_TRACE_LEFT_BOX, SPH_TRACE_STAGNANT, SPH_TRACE_NONFINITE
  ! gravitational potential and acceleration at arbitrary points (the gas' Barnes-Hut field and the sinks' field)
  public :: sph_gravity_at_desc, sph_gravity_at, sph_gravity_at_dev, SPH_GRAVAT_GAS, SPH_GRAVAT_SINKS, SPH_GRAVAT_SPLIT
  ! binding energies and unbinding of groups (each group's own potential, the members' energies, the bound core)
  public :: sph_bound_desc, sph_bound, sph_bound_dev, SPH_BOUND_THERMAL, SPH_BOUND_NCOL
  ! spectral cubes (the optically thin position-position-velocity cube of the owned gas seen along any direction)
  public :: sph_cube_desc, sph_cube, sph_cube_dev, SPH_CUBE_PER_VELOCITY
  ! emission-absorption images (intensity, optical depth, transmission and the tau surface of the gas seen along any direction)
  public :: sph_transfer_desc, sph_transfer, sph_transfer_dev, SPH_TRANSFER_VALUES, SPH_TRANSFER_ONE
  ! the rates of sph_forces split by physical term (pressure, viscosity, sink gravity, self-gravity, PdV, heating, alpha)
  public :: sph_force_terms_desc, sph_force_terms, sph_force_terms_dev, SPH_TERMS_NROW, SPH_TERMS_SKIP_GAS_GRAVITY
  ! binned sums (weighted 1-D and 2-D sums of any fields or caller rows; the generic form of sph_profile's reduction)
  public :: sph_binned_desc, sph_binned, sph_binned_dev, sph_binned_edges, SPH_BINNED_MAX_Q
  public :: SPH_BINNED_W_ONE, SPH_BINNED_W_MASS, SPH_BINNED_W_VOLUME, SPH_BINNED_LOG0, SPH_BINNED_LOG1
  public :: SPH_BINNED_EDGES0, SPH_BINNED_EDGES1, SPH_BINNED_SQUARES, SPH_BINNED_SKIP_NAN
  ! pair sums (pair-separation histograms and structure functions, accumulated exactly in 128-bit fixed point)
  public :: sph_pairs_desc, sph_pairs, sph_pairs_dev, sph_pairs_edges, sph_pairs_finish, SPH_PAIRS_MAX_Q, SPH_PAIRS_MAX_BINS
  public :: sph_modes_desc, sph_modes, sph_modes_dev, sph_modes_tables, sph_modes_finish, SPH_MODES_MAX_M, SPH_MODES_MAX_RINGS
  public :: SPH_MODES_MAX_P, SPH_MODES_W_ONE, SPH_MODES_W_MASS, SPH_MODES_LOG
  public :: sph_history_desc, sph_history_begin, sph_history_end, sph_history_record, sph_history_info, sph_history_read
  public :: sph_history_read_dev, SPH_HISTORY_NHEAD, sph_history_begin_env, sph_history_write
  ! trajectories and fates of chosen particles
  public :: sph_track_desc, sph_track_begin, sph_track_begin_dev, sph_track_end, sph_track_record, sph_track_info, sph_track_read
  public :: sph_track_read_dev, sph_track_fates, sph_track_fates_dev, SPH_TRACK_NHEAD, SPH_TRACK_NCOL, sph_track_begin_env
  public :: sph_track_write
  public :: sph_dust_desc, sph_dust_begin, sph_dust_begin_dev, sph_dust_end, sph_dust_advance, sph_dust_info, sph_dust_read
  public :: sph_dust_read_dev, sph_dust_state, sph_dust_state_dev, sph_dust_fates, sph_dust_fates_dev
  public :: SPH_DUST_NHEAD, SPH_DUST_NCOL, SPH_DUST_EPSTEIN, SPH_DUST_FIXED_TS, SPH_DUST_REMOVE
  ! the movie of a run: line-of-sight-integrated maps of the owned gas appended on the device, and the one-shot frame
  public :: sph_frames_desc, sph_frames_begin, sph_frames_end, sph_frames_record, sph_frames_rewind, sph_frames_info
  public :: sph_frames_read, sph_frames_read_dev, sph_frame, sph_frame_dev, SPH_FRAMES_NHEAD, SPH_FRAMES_MAX_FIELDS
  public :: SPH_FRAMES_OK, SPH_FRAMES_SINK_GONE, sph_frames_begin_env, sph_frames_write
  public :: SPH_PAIRS_W_ONE, SPH_PAIRS_W_MASS, SPH_PAIRS_LOG, SPH_PAIRS_CALLER_EDGES, SPH_PAIRS_SCALE_H, SPH_PAIRS_VELOCITY
  public :: c_message

  integer(c_int), parameter :: SPH_OK = 0
  integer(c_int), parameter :: SPH_F_X = 0, SPH_F_Y = 1, SPH_F_Z = 2, SPH_F_VX = 3, SPH_F_VY = 4, SPH_F_VZ = 5
  integer(c_int), parameter :: SPH_F_U = 6, SPH_F_M = 7, SPH_F_ALPHA = 8, SPH_F_RHO = 9, SPH_F_P = 10, SPH_F_C = 11
  integer(c_int), parameter :: SPH_F_AX = 12, SPH_F_AY = 13, SPH_F_AZ = 14, SPH_F_DU = 15, SPH_F_DALPHA = 16

  integer(c_int), parameter :: SPH_F_H = 17, SPH_F_OMEGA = 18
  integer(c_int32_t), parameter :: SPH_FLAG_REUSE_DENSITY = 1, SPH_FLAG_VARIABLE_H = 2, SPH_FLAG_SELF_GRAVITY = 16
  integer(c_int32_t), parameter :: SPH_FLAG_ACCRETE_CULL = 32, SPH_FLAG_SINK_CREATION = 64
  integer(c_int32_t), parameter :: SPH_FLAG_HASHED_GRID = 1024
  integer(c_int32_t), parameter :: SPH_PARTIALS = 199
  integer(c_int32_t), parameter :: SPH_RENDER_AUTO_BOUNDS = 1, SPH_RENDER_SPACING = 2
  integer(c_int32_t), parameter :: SPH_RENDER_FIELD_VALUES = -1, SPH_RENDER_WEIGHT_MASS = 0, SPH_RENDER_WEIGHT_VOLUME = 1
  integer(c_int32_t), parameter :: SPH_PROFILE_LOG = 1, SPH_PROFILE_AUTO_NORMAL = 2, SPH_PROFILE_NSUM = 20, SPH_PROFILE_NCOL = 29
  integer(c_int32_t), parameter :: SPH_ENERGY_NSUM = 28
  integer(c_int32_t), parameter :: SPH_GROUPS_LINK_H = 1, SPH_GROUPS_NCOL = 21
  integer(c_int32_t), parameter :: SPH_PEAKS_LINK_H = 1, SPH_PEAKS_NCOL = 23, SPH_PEAKS_NCOUNT = 3

  type, bind(C) :: sph_params
    real(c_double) :: h, gamma, gamma_m1
    integer(c_int32_t) :: nq, flags
    real(c_double) :: kernel_pi, visc_eps, alpha_floor, alpha_decay, G, dt_scale, dt_max, dt_min, bounding_size
    real(c_double) :: eta, h_tol, h_max_length, h_min_length, h_iter_cap     ! variable-h path only
    real(c_double) :: theta                                                   ! self-gravity opening angle
  end type sph_params

  type, bind(C) :: sph_grid_info
    integer(c_int32_t) :: kind              ! 0 dense, 1 hashed, -1 no grid built yet
    integer(c_int32_t) :: dim(3)
    integer(c_int64_t) :: occupied_cells, table_entries
    real(c_double) :: index_cells
    integer(c_int64_t) :: bytes
  end type sph_grid_info

  type, bind(C) :: sph_stats
    integer(c_int64_t) :: n, n_cells
    integer(c_int32_t) :: grid_dim(3)
    integer(c_int32_t) :: nlist_capacity, nlist_max, tile_fit_pct
    real(c_double) :: nlist_mean
    integer(c_int64_t) :: grid_builds, nlist_builds, density_passes, force_passes, device_bytes
    real(c_double) :: nlist_wave_mean
    integer(c_int32_t) :: tile_fit_pct_forces, host_syncs
    real(c_double) :: lane_efficiency_forces
    integer(c_int64_t) :: nlist_reflags
  end type sph_stats

  ! node box, strict clip box (-huge / +huge or IEEE infinities: none), h (0: each particle's own), nodes per axis,
  ! axis (-1: the 3-D grid, 0/1/2: column sums along x/y/z), flags, reserved (0).  The 3-D output is C order, x slowest:
  ! a Fortran array out(n(3), n(2), n(1)); column sums along z are out(n(2), n(1)).
  type, bind(C) :: sph_render_desc
    real(c_double) :: lo(3), hi(3), clip_lo(3), clip_hi(3)
    real(c_double) :: h
    integer(c_int32_t) :: n(3)
    integer(c_int32_t) :: axis, flags, reserved
  end type sph_render_desc

  ! base: as for sph_render_density; field: SPH_F_* or SPH_RENDER_FIELD_VALUES; weight: SPH_RENDER_WEIGHT_MASS / _VOLUME;
  ! normalise: 0 (num) / 1 (num / den); reserved: 0.  144 bytes.
  type, bind(C) :: sph_render_field_desc
    type(sph_render_desc) :: base
    integer(c_int32_t) :: field, weight, normalise, reserved
  end type sph_render_field_desc

  ! centre / centre_v / central_mass (ignored with sink >= 0), normal (written back normalised), rings [r_min, r_max),
  ! strict |z'| < z_max (IEEE +infinity: none), n_r rings x n_phi sectors, sink (-1: none), flags, reserved (0).
  ! sums(SPH_PROFILE_NSUM, n_bins) and table(SPH_PROFILE_NCOL, n_bins), bin = ring * n_phi + sector.  128 bytes.
  type, bind(C) :: sph_profile_desc
    real(c_double) :: centre(3), centre_v(3)
    real(c_double) :: central_mass
    real(c_double) :: normal(3)
    real(c_double) :: r_min, r_max, z_max
    integer(c_int32_t) :: n_r, n_phi, sink, flags
    integer(c_int32_t) :: reserved(2)
  end type sph_profile_desc

  ! linking length (LINK_H: in units of max(h_i, h_j)), rho >= rho_min (IEEE -infinity: none), strict clip box
  ! (+-infinity: none), min_members >= 1, flags, reserved (0).  table(SPH_GROUPS_NCOL, max_groups).  80 bytes.
  type, bind(C) :: sph_groups_desc
    real(c_double) :: link, rho_min
    real(c_double) :: clip_lo(3), clip_hi(3)
    integer(c_int64_t) :: min_members
    integer(c_int32_t) :: flags, reserved
  end type sph_groups_desc

  ! neighbour radius (LINK_H: in units of max(h_i, h_j)), rho >= rho_min, components whose top has rho < peak_min are
  ! dropped (IEEE -infinity: none), contrast >= 1 (1: raw basins, +infinity: friends-of-friends), strict clip box,
  ! min_members >= 1, flags, reserved (0).  table(SPH_PEAKS_NCOL, max_groups), counts(SPH_PEAKS_NCOUNT).  96 bytes.
  type, bind(C) :: sph_peaks_desc
    real(c_double) :: link, rho_min, peak_min, contrast
    real(c_double) :: clip_lo(3), clip_hi(3)
    integer(c_int64_t) :: min_members
    integer(c_int32_t) :: flags, reserved
  end type sph_peaks_desc

  ! sph_gradients: strict target clip box (+-infinity: none), h (> 0: one h for all; 0: each particle's own), fields
  ! (SPH_F_* or SPH_GRAD_VALUES: row k of values), n_fields 1 .. 4, flags (SPH_GRAD_CORRECTED), reserved (0).  out holds
  ! out(id, a, k) in Fortran order: (sph_count, 3, n_fields).  88 bytes.
  integer(c_int32_t), parameter :: SPH_GRAD_CORRECTED = 1, SPH_GRAD_MAX_FIELDS = 4, SPH_GRAD_VALUES = -1
  type, bind(C) :: sph_gradients_desc
    real(c_double) :: clip_lo(3), clip_hi(3)
    real(c_double) :: h
    integer(c_int32_t) :: fields(SPH_GRAD_MAX_FIELDS)
    integer(c_int32_t) :: n_fields, flags
    integer(c_int32_t) :: reserved(2)
  end type sph_gradients_desc

  ! sph_sample: strict SOURCE clip box (+-infinity: none), h (> 0: one h for all; 0: each particle's own), fields (SPH_F_*
  ! or SPH_SAMPLE_VALUES: row k of values), n_fields 0 .. 4 (0: the weight alone), weight (SPH_RENDER_WEIGHT_MASS /
  ! _VOLUME), flags (SPH_SAMPLE_NORMALISE), reserved (0).  out holds out(p, k) in Fortran order: (n_points, n_fields).
  ! 88 bytes.
  integer(c_int32_t), parameter :: SPH_SAMPLE_NORMALISE = 1, SPH_SAMPLE_MAX_FIELDS = 4, SPH_SAMPLE_VALUES = -1
  type, bind(C) :: sph_sample_desc
    real(c_double) :: clip_lo(3), clip_hi(3)
    real(c_double) :: h
    integer(c_int32_t) :: fields(SPH_SAMPLE_MAX_FIELDS)
    integer(c_int32_t) :: n_fields, weight, flags, reserved
  end type sph_sample_desc

  ! sph_trace: sph_sample's SOURCE clip box and h, the tracers' box (+-infinity: none), the step ds (finite, /= 0), the frame
  ! v - omega x (p - centre), the SPH_TRACE_PLANAR normal, the three component ids and the carry id (SPH_F_*,
  ! SPH_TRACE_VALUES: row k, the carry row 4, of values; carry: SPH_TRACE_NONE), weight, n_steps 1 .. 65535, stride (divides
  ! n_steps), flags, reserved (0).  path holds path(p, a, r) in Fortran order: (n_seeds, 3, n_steps / stride + 1).  224 bytes.
  integer(c_int32_t), parameter :: SPH_TRACE_ARCLENGTH = 1, SPH_TRACE_PLANAR = 2, SPH_TRACE_VALUES = -1, SPH_TRACE_NONE = -2
  integer(c_int32_t), parameter :: SPH_TRACE_DONE = 0, SPH_TRACE_LEFT_GAS = 1, SPH_TRACE_LEFT_BOX = 2, SPH_TRACE_STAGNANT = 3, &
                                   SPH_TRACE_NONFINITE = 4
  type, bind(C) :: sph_trace_desc
    real(c_double) :: clip_lo(3), clip_hi(3)
    real(c_double) :: h
    real(c_double) :: box_lo(3), box_hi(3)
    real(c_double) :: ds
    real(c_double) :: omega(3), centre(3), normal(3)
    integer(c_int32_t) :: fields(3)
    integer(c_int32_t) :: carry, weight, n_steps, stride, flags
    integer(c_int32_t) :: reserved(2)
  end type sph_trace_desc

  ! sph_gravity_at: h (> 0: the softening length of every point; 0: params.h, fixed-h contexts only; unused with ph), soft2
  ! (>= 0, added to d.d; 0.0025 is the force's value), flags (SPH_GRAVAT_GAS, _SINKS, _SPLIT), reserved (0).  out holds
  ! out(p, c) in Fortran order: (n_points, 4) -- c = 1 Phi, 2..4 a -- or (n_points, 8) with SPLIT (the gas, then the sinks).
  ! 32 bytes.
  integer(c_int32_t), parameter :: SPH_GRAVAT_GAS = 1, SPH_GRAVAT_SINKS = 2, SPH_GRAVAT_SPLIT = 4
  type, bind(C) :: sph_gravity_at_desc
    real(c_double) :: h, soft2
    integer(c_int32_t) :: flags
    integer(c_int32_t) :: reserved(3)
  end type sph_gravity_at_desc

  ! sph_bound: h (> 0: one softening length for every member; 0: each particle's own h), soft2 (>= 0, added to d.d; 0.0025
  ! is the force's value), min_members (>= 1: a set that falls below it dissolves), max_members (>= 1: larger groups are
  ! skipped), max_rounds (>= 0 removals; 0: evaluate once), flags (SPH_BOUND_THERMAL), reserved (0).  out holds out(id, c) in
  ! Fortran order: (sph_count, 2) -- c = 1 e, 2 Phi; table(SPH_BOUND_NCOL, n_groups); counts(4).  48 bytes.
  integer(c_int32_t), parameter :: SPH_BOUND_THERMAL = 1, SPH_BOUND_NCOL = 24
  type, bind(C) :: sph_bound_desc
    real(c_double) :: h, soft2
    integer(c_int64_t) :: min_members, max_members
    integer(c_int32_t) :: max_rounds, flags
    integer(c_int32_t) :: reserved(2)
  end type sph_bound_desc

  ! sph_cube: rot (row-major in C: rot(1:3) = u^, rot(4:6) = v^, rot(7:9) = w^, the line of sight, away from the observer),
  ! centre, v_ref, image node box lo / hi (u, v), strict clip box (simulation axes; +-infinity: none), h (> 0: one h for all;
  ! 0: each particle's own), v0 (centre of channel 0), dv (channel width, > 0), sigma_scale, sigma_floor (sigma_j =
  ! sqrt((sigma_scale c_j)^2 + sigma_floor^2)), n_u, n_v, n_chan, flags (SPH_CUBE_PER_VELOCITY), reserved (0).  out holds
  ! out(iv, iu, k) in Fortran order: (n_v, n_u, n_chan).  264 bytes.
  integer(c_int32_t), parameter :: SPH_CUBE_PER_VELOCITY = 1
  type, bind(C) :: sph_cube_desc
    real(c_double) :: rot(9)
    real(c_double) :: centre(3), v_ref(3)
    real(c_double) :: lo(2), hi(2)
    real(c_double) :: clip_lo(3), clip_hi(3)
    real(c_double) :: h
    real(c_double) :: v0, dv
    real(c_double) :: sigma_scale, sigma_floor
    integer(c_int32_t) :: n_u, n_v, n_chan, flags
    integer(c_int64_t) :: reserved
  end type sph_cube_desc

  ! sph_transfer: rot, centre, image node box, strict clip box and h as sph_cube's; kappa_scale (kappa_j = kappa_scale K_j),
  ! tau_surface (> 0), tau_max (> 0, may be +infinity), background, n_u, n_v, source and kappa (where S and K come from: a
  ! field id, SPH_TRANSFER_VALUES or SPH_TRANSFER_ONE), flags (0), reserved (0).  out holds out(iv, iu, plane) in Fortran
  ! order: (n_v, n_u, 4), planes I + T background, tau, T, depth of the tau_surface surface.  240 bytes.
  integer(c_int32_t), parameter :: SPH_TRANSFER_VALUES = -1
  integer(c_int32_t), parameter :: SPH_TRANSFER_ONE = -2
  type, bind(C) :: sph_transfer_desc
    real(c_double) :: rot(9)
    real(c_double) :: centre(3)
    real(c_double) :: lo(2), hi(2)
    real(c_double) :: clip_lo(3), clip_hi(3)
    real(c_double) :: h
    real(c_double) :: kappa_scale, tau_surface, tau_max, background
    integer(c_int32_t) :: n_u, n_v, source, kappa
    integer(c_int32_t) :: flags, reserved
  end type sph_transfer_desc

  ! sph_force_terms: flags (SPH_TERMS_SKIP_GAS_GRAVITY: rows 9-11 are NaN, no tree walk), reserved (0).  out holds
  ! out(id, row) in Fortran order: (sph_count, SPH_TERMS_NROW), rows a_P(3) a_V(3) a_S(3) a_G(3) du_P du_V and the source and
  ! decay parts of dalpha/dt.  16 bytes.
  integer(c_int32_t), parameter :: SPH_TERMS_NROW = 16, SPH_TERMS_SKIP_GAS_GRAVITY = 1
  type, bind(C) :: sph_force_terms_desc
    integer(c_int32_t) :: flags
    integer(c_int32_t) :: reserved(3)
  end type sph_force_terms_desc

  ! sph_binned: a source (axis, q) is an SPH_F_* id or -1 - k: row k of values (C: SPH_BINNED_ROW(k)), values(id, row) in
  ! Fortran order: (sph_count, n_rows).  sums(s, k1, k0) in Fortran order: (nsum, n(2), n(1)), nsum = 2 + n_q (1 + squares).
  ! 112 bytes.
  integer(c_int32_t), parameter :: SPH_BINNED_MAX_Q = 8
  integer(c_int32_t), parameter :: SPH_BINNED_W_ONE = 0, SPH_BINNED_W_MASS = 1, SPH_BINNED_W_VOLUME = 2
  integer(c_int32_t), parameter :: SPH_BINNED_LOG0 = 1, SPH_BINNED_LOG1 = 2, SPH_BINNED_EDGES0 = 4, SPH_BINNED_EDGES1 = 8
  integer(c_int32_t), parameter :: SPH_BINNED_SQUARES = 16, SPH_BINNED_SKIP_NAN = 32
  type, bind(C) :: sph_binned_desc
    real(c_double) :: lo(2), hi(2)
    integer(c_int32_t) :: axis(2)
    integer(c_int32_t) :: n(2)
    integer(c_int32_t) :: n_axes, n_q
    integer(c_int32_t) :: q(SPH_BINNED_MAX_Q)
    integer(c_int32_t) :: weight, n_rows, flags
    integer(c_int32_t) :: reserved(3)
  end type sph_binned_desc

  ! sph_pairs: a quantity q is an SPH_F_* id or -1 - k: row k of values (C: SPH_PAIRS_ROW(k)), values(id, row) in Fortran
  ! order: (sph_count, n_rows).  sums(s, b) in Fortran order: (nsum, n_bins), nsum = 2 + 2 n_q + (4 with VELOCITY); raw(limb,
  ! s, b): (2, nsum, n_bins) 64-bit limbs, low first; exps(nsum).  120 bytes.
  integer(c_int32_t), parameter :: SPH_PAIRS_MAX_Q = 4, SPH_PAIRS_MAX_BINS = 1024
  integer(c_int32_t), parameter :: SPH_PAIRS_W_ONE = 0, SPH_PAIRS_W_MASS = 1
  ! SPH_PAIRS_CALLER_EDGES is C's SPH_PAIRS_EDGES: Fortran names ignore case, and sph_pairs_edges is the function
  integer(c_int32_t), parameter :: SPH_PAIRS_LOG = 1, SPH_PAIRS_CALLER_EDGES = 2, SPH_PAIRS_SCALE_H = 4, SPH_PAIRS_VELOCITY = 8
  type, bind(C) :: sph_pairs_desc
    real(c_double) :: lo, hi
    real(c_double) :: clip_lo(3), clip_hi(3)
    integer(c_int32_t) :: n_bins, n_q
    integer(c_int32_t) :: q(SPH_PAIRS_MAX_Q)
    integer(c_int32_t) :: weight, n_rows, flags
    integer(c_int32_t) :: target_stride, target_phase
    integer(c_int32_t) :: reserved(3)
  end type sph_pairs_desc

  ! sph_modes: q is an SPH_F_* id or -1 - k: row k of values (C: SPH_MODES_ROW(k)), values(id, row) in Fortran order.  The
  ! output is flat, n_out = 2 (m_max + 1) (n_r + n_p): the ring block as ring(2, m_max + 1, n_r) in Fortran order (C, S), then
  ! the spiral block as spiral(2, n_p, m_max + 1) (CS, SN); raw the same with a leading axis of 2 limbs, low first.  168 bytes.
  integer(c_int32_t), parameter :: SPH_MODES_MAX_M = 8, SPH_MODES_MAX_RINGS = 1024, SPH_MODES_MAX_P = 256
  integer(c_int32_t), parameter :: SPH_MODES_W_ONE = 0, SPH_MODES_W_MASS = 1, SPH_MODES_LOG = 1
  type, bind(C) :: sph_modes_desc
    real(c_double) :: centre(3), centre_v(3)
    real(c_double) :: normal(3)
    real(c_double) :: r_min, r_max, z_max
    real(c_double) :: p_min, p_max, r_ref
    integer(c_int32_t) :: n_r, m_max, n_p, sink
    integer(c_int32_t) :: weight, n_q, q, n_rows
    integer(c_int32_t) :: flags
    integer(c_int32_t) :: reserved(3)
  end type sph_modes_desc

  ! sph_history: a row is SPH_HISTORY_NHEAD + 7 max_sinks doubles; rows(width, count) in Fortran order.  16 bytes.
  integer(c_int32_t), parameter :: SPH_HISTORY_NHEAD = 40
  type, bind(C) :: sph_history_desc
    integer(c_int32_t) :: capacity, every, max_sinks, flags
  end type sph_history_desc

  ! sph_track: a row is a head of SPH_TRACK_NHEAD doubles and a body of SPH_TRACK_NCOL values per tracked particle,
  ! body(n_ids, SPH_TRACK_NCOL, count) in Fortran order; fates(4, n_ids).  16 bytes.
  integer(c_int32_t), parameter :: SPH_TRACK_NHEAD = 4, SPH_TRACK_NCOL = 10
  type, bind(C) :: sph_track_desc
    integer(c_int64_t) :: capacity
    integer(c_int32_t) :: every, flags
  end type sph_track_desc

  ! sph_dust: a row is a head of SPH_DUST_NHEAD doubles and a body of SPH_DUST_NCOL values per grain, body(m, SPH_DUST_NCOL,
  ! count) in Fortran order; fates(3, m).  32 bytes.
  integer(c_int32_t), parameter :: SPH_DUST_NHEAD = 4, SPH_DUST_NCOL = 12
  integer(c_int32_t), parameter :: SPH_DUST_EPSTEIN = 0, SPH_DUST_FIXED_TS = 1, SPH_DUST_REMOVE = 1
  type, bind(C) :: sph_dust_desc
    integer(c_int64_t) :: capacity
    integer(c_int32_t) :: every, record_every, law, flags
    real(c_double) :: rho_grain
  end type sph_dust_desc

  ! sph_frames: a frame is a head of SPH_FRAMES_NHEAD doubles and 1 + nq planes, planes(n_v, n_u, 1 + nq, count) in Fortran
  ! order; rot(9) holds the rows u^, v^, w^ one after the other.  240 bytes.
  integer(c_int32_t), parameter :: SPH_FRAMES_NHEAD = 16, SPH_FRAMES_MAX_FIELDS = 3
  integer(c_int32_t), parameter :: SPH_FRAMES_OK = 0, SPH_FRAMES_SINK_GONE = 1
  type, bind(C) :: sph_frames_desc
    real(c_double) :: rot(9)
    real(c_double) :: centre(3)
    real(c_double) :: lo(2), hi(2)
    real(c_double) :: clip_lo(3), clip_hi(3)
    real(c_double) :: h, dt_frame
    integer(c_int64_t) :: capacity
    integer(c_int32_t) :: n_u, n_v
    integer(c_int32_t) :: every, centre_sink, nq
    integer(c_int32_t) :: fields(SPH_FRAMES_MAX_FIELDS)
    integer(c_int64_t) :: reserved
  end type sph_frames_desc

  interface
    integer(c_int) function sph_abi_version() bind(C, name='sph_abi_version')
      import :: c_int
    end function

    integer(c_int) function sph_get_params(ctx, p) bind(C, name='sph_get_params')
      import :: c_int, c_ptr, sph_params
      type(c_ptr), value :: ctx
      type(sph_params), intent(out) :: p
    end function

    integer(c_int) function sph_params_default(p) bind(C, name='sph_params_default')
      import :: c_int, sph_params
      type(sph_params), intent(out) :: p
    end function

    ! stands in for init_kernel_table (:55-79) and the per-step tree allocation (:894,905)
    integer(c_int) function sph_ctx_create(p, device, ctx) bind(C, name='sph_ctx_create')
      import :: c_int, c_ptr, sph_params
      type(sph_params), intent(in) :: p
      integer(c_int), value :: device
      type(c_ptr), intent(out) :: ctx
    end function

    integer(c_int) function sph_ctx_destroy(ctx) bind(C, name='sph_ctx_destroy')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    type(c_ptr) function sph_strerror(status) bind(C, name='sph_strerror')
      import :: c_int, c_ptr
      integer(c_int), value :: status
    end function

    type(c_ptr) function sph_last_error(ctx) bind(C, name='sph_last_error')
      import :: c_ptr
      type(c_ptr), value :: ctx
    end function

    ! hand-over of `type(particle) :: bodies(:)` as struct-of-arrays (:14-27)
    integer(c_int) function sph_upload(ctx, n, x, y, z, vx, vy, vz, u, m, alpha) bind(C, name='sph_upload')
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n
      real(c_double), intent(in) :: x(*), y(*), z(*), vx(*), vy(*), vz(*), u(*), m(*), alpha(*)
    end function

    ! hand-over of `type(sink) :: sinks(:)` (:30-37)
    integer(c_int) function sph_set_sinks(ctx, ns, sx, sy, sz, svx, svy, svz, sm) bind(C, name='sph_set_sinks')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: ns
      real(c_double), intent(in) :: sx(*), sy(*), sz(*), svx(*), svy(*), svz(*), sm(*)
    end function

    integer(c_int) function sph_get_sinks(ctx, ns, sx, sy, sz, svx, svy, svz, sm, sax, say, saz) &
        bind(C, name='sph_get_sinks')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: ns
      real(c_double), intent(out) :: sx(*), sy(*), sz(*), svx(*), svy(*), svz(*), sm(*), sax(*), say(*), saz(*)
    end function

    integer(c_int) function sph_params_default_variable(p) bind(C, name='sph_params_default_variable')
      import :: c_int, sph_params
      type(sph_params), intent(out) :: p
    end function

    ! sink%radius (:694)
    integer(c_int) function sph_set_sink_radii(ctx, ns, radius) bind(C, name='sph_set_sink_radii')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: ns
      real(c_double), intent(in) :: radius(*)
    end function

    ! initiate_sink_accretion + check_bounds (:919-920)
    integer(c_int) function sph_accrete_and_cull(ctx, n_removed) bind(C, name='sph_accrete_and_cull')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx
      integer(c_int64_t), intent(out) :: n_removed
    end function

    ! one field in the caller's particle order (e.g. the smoothing lengths of the variable-h variant)
    integer(c_int) function sph_upload_field(ctx, field, host, n) bind(C, name='sph_upload_field')
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int), value :: field
      real(c_double), intent(in) :: host(*)
      integer(c_int64_t), value :: n
    end function

    ! calc_smoothing of the variable-h variant
    integer(c_int) function sph_update_h(ctx) bind(C, name='sph_update_h')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    integer(c_int64_t) function sph_count(ctx) bind(C, name='sph_count')
      import :: c_int64_t, c_ptr
      type(c_ptr), value :: ctx
    end function

    ! number of sinks (check_sink_creation of the variable-h variant may add one per step)
    integer(c_int32_t) function sph_sink_count(ctx) bind(C, name='sph_sink_count')
      import :: c_int32_t, c_ptr
      type(c_ptr), value :: ctx
    end function

    integer(c_int) function sph_get_sink_radii(ctx, ns, radius) bind(C, name='sph_get_sink_radii')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: ns
      real(c_double), intent(out) :: radius(*)
    end function

    ! create_tree + get_density + get_pressure_and_sound_speed (:894-897)
    integer(c_int) function sph_density(ctx) bind(C, name='sph_density')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    ! find_forces (:818-829) without the Barnes-Hut gas self-gravity term
    integer(c_int) function sph_forces(ctx) bind(C, name='sph_forces')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    ! kick (:742-759)
    integer(c_int) function sph_kick(ctx, dt) bind(C, name='sph_kick')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), value :: dt
    end function

    ! drift (:762-776)
    integer(c_int) function sph_drift(ctx, dt) bind(C, name='sph_drift')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), value :: dt
    end function

    ! get_next_timestep (:831-860)
    integer(c_int) function sph_next_dt(ctx, dt) bind(C, name='sph_next_dt')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), intent(inout) :: dt
    end function

    ! one iteration of simulate's loop body (:889-916)
    integer(c_int) function sph_step(ctx, dt, t) bind(C, name='sph_step')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), intent(inout) :: dt, t
    end function

    integer(c_int) function sph_run(ctx, nsteps, dt, t) bind(C, name='sph_run')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nsteps
      real(c_double), intent(inout) :: dt, t
    end function

    integer(c_int) function sph_download_field(ctx, field, host, n) bind(C, name='sph_download_field')
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int), value :: field
      real(c_double), intent(out) :: host(*)
      integer(c_int64_t), value :: n
    end function

    integer(c_int) function sph_download_state(ctx, n, x, y, z, vx, vy, vz, u, m, alpha) &
        bind(C, name='sph_download_state')
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n
      real(c_double), intent(out) :: x(*), y(*), z(*), vx(*), vy(*), vz(*), u(*), m(*), alpha(*)
    end function

    integer(c_int) function sph_get_stats(ctx, st) bind(C, name='sph_get_stats')
      import :: c_int, c_ptr, sph_stats
      type(c_ptr), value :: ctx
      type(sph_stats), intent(out) :: st
    end function

    ! the cell grid of the last build (dense or hashed); reads the occupied-cell count back
    integer(c_int) function sph_get_grid_info(ctx, gi) bind(C, name='sph_get_grid_info')
      import :: c_int, c_ptr, sph_grid_info
      type(c_ptr), value :: ctx
      type(sph_grid_info), intent(out) :: gi
    end function

    ! bounding box of the current positions: what check_bounds (:471-482) needs
    integer(c_int) function sph_get_bbox(ctx, lo, hi) bind(C, name='sph_get_bbox')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), intent(out) :: lo(3), hi(3)
    end function

    integer(c_int) function sph_synchronize(ctx) bind(C, name='sph_synchronize')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    ! ---- one context per GPU: owned particles + ghost copies, exchanged by the caller (MPI, RCCL, ...) -------------
    integer(c_int) function sph_set_owned(ctx, n_owned) bind(C, name='sph_set_owned')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n_owned
    end function
    integer(c_int) function sph_set_rank(ctx, rank, nranks) bind(C, name='sph_set_rank')
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: rank, nranks
    end function
    integer(c_int) function sph_reserve(ctx, n_slots) bind(C, name='sph_reserve')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx
      integer(c_int64_t), value :: n_slots
    end function
    integer(c_int) function sph_owned_bbox(ctx, lo_hi, d_lo_hi) bind(C, name='sph_owned_bbox')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx, d_lo_hi
      real(c_double), intent(out) :: lo_hi(6)
    end function
    integer(c_int) function sph_select_boxes(ctx, nbox, boxes, counts) bind(C, name='sph_select_boxes')
      import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nbox
      real(c_double), intent(in) :: boxes(6, *)
      integer(c_int64_t), intent(out) :: counts(*)
    end function
    integer(c_int) function sph_selected_ids_dev(ctx, box, count, d_ids) bind(C, name='sph_selected_ids_dev')
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_ids
      integer(c_int32_t), value :: box
      integer(c_int64_t), value :: count
    end function
    integer(c_int) function sph_select_boxes_async(ctx, nbox, boxes) bind(C, name='sph_select_boxes_async')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nbox
      real(c_double), intent(in) :: boxes(*)
    end function
    integer(c_int) function sph_selected_counts(ctx, nbox, counts) bind(C, name='sph_selected_counts')
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nbox
      integer(c_int64_t), intent(out) :: counts(*)
    end function
    integer(c_int) function sph_gather_selected_dev(ctx, box, nf, fields, capacity, d_out) bind(C, name='sph_gather_selected_dev')
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_out
      integer(c_int32_t), value :: box, nf
      integer(c_int32_t), intent(in) :: fields(*)
      integer(c_int64_t), value :: capacity
    end function
    integer(c_int) function sph_replace_ghosts_dev(ctx, count, d_state) bind(C, name='sph_replace_ghosts_dev')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_state
      integer(c_int64_t), value :: count
    end function
    integer(c_int) function sph_gather_fields_dev(ctx, nf, fields, count, d_ids, d_out) bind(C, name='sph_gather_fields_dev')
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_ids, d_out
      integer(c_int32_t), value :: nf
      integer(c_int32_t), intent(in) :: fields(*)
      integer(c_int64_t), value :: count
    end function
    integer(c_int) function sph_scatter_fields_dev(ctx, nf, fields, first, count, d_vals) bind(C, name='sph_scatter_fields_dev')
      import :: c_int, c_int32_t, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_vals
      integer(c_int32_t), value :: nf
      integer(c_int32_t), intent(in) :: fields(*)
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_refresh_eos_ghosts(ctx) bind(C, name='sph_refresh_eos_ghosts')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_set_boundary_boxes(ctx, nbox, boxes) bind(C, name='sph_set_boundary_boxes')
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: nbox
      real(c_double), intent(in) :: boxes(6, *)
    end function
    integer(c_int) function sph_forces_part(ctx, part) bind(C, name='sph_forces_part')
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: ctx
      integer(c_int32_t), value :: part
    end function
    integer(c_int) function sph_set_dt(ctx, dt, t) bind(C, name='sph_set_dt')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), value :: dt, t
    end function
    integer(c_int) function sph_get_dt(ctx, dt, t) bind(C, name='sph_get_dt')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: ctx
      real(c_double), intent(out) :: dt, t
    end function
    integer(c_int) function sph_kick_devdt(ctx) bind(C, name='sph_kick_devdt')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_kick_drift_devdt(ctx) bind(C, name='sph_kick_drift_devdt')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    integer(c_int) function sph_kick_dt_candidate_gas_dev(ctx) bind(C, name='sph_kick_dt_candidate_gas_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    integer(c_int) function sph_kick_sinks_devdt(ctx) bind(C, name='sph_kick_sinks_devdt')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    integer(c_int) function sph_kick_dt_candidate_dev(ctx) bind(C, name='sph_kick_dt_candidate_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function

    integer(c_int) function sph_drift_devdt(ctx) bind(C, name='sph_drift_devdt')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_dt_candidate_dev(ctx) bind(C, name='sph_dt_candidate_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_pack_partials_ex_dev(ctx, d_out, predict_box) bind(C, name='sph_pack_partials_ex_dev')
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: ctx, d_out
      integer(c_int32_t), value :: predict_box
    end function

    integer(c_int) function sph_pack_partials_dev(ctx, d_out) bind(C, name='sph_pack_partials_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, d_out
    end function
    integer(c_int) function sph_apply_partials_dev(ctx, d_all, nranks, stride, apply_dt) bind(C, name='sph_apply_partials_dev')
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: ctx, d_all
      integer(c_int32_t), value :: nranks, stride, apply_dt
    end function
    integer(c_int) function sph_set_gravity_sources_dev(ctx, n_src, d_xyzm, lo_hi) bind(C, name='sph_set_gravity_sources_dev')
      import :: c_int, c_int64_t, c_ptr, c_double
      type(c_ptr), value :: ctx, d_xyzm
      integer(c_int64_t), value :: n_src
      real(c_double), intent(in) :: lo_hi(6)
    end function

    ! ---- density rendering: the grid loop and the projection of Density_Image.py (KD-tree ball query per node,
    ! m W(r, h) with the analytic cubic spline, sum along z); d%lo / d%hi written back with SPH_RENDER_AUTO_BOUNDS
    integer(c_int) function sph_render_density(ctx, d, host_out, out_len) bind(C, name='sph_render_density')
      import :: c_int, c_int64_t, c_ptr, c_double, sph_render_desc
      type(c_ptr), value :: ctx
      type(sph_render_desc), intent(inout) :: d
      real(c_double), intent(out) :: host_out(*)
      integer(c_int64_t), value :: out_len
    end function
    integer(c_int) function sph_render_density_dev(ctx, d, d_out, out_len) bind(C, name='sph_render_density_dev')
      import :: c_int, c_int64_t, c_ptr, sph_render_desc
      type(c_ptr), value :: ctx, d_out
      type(sph_render_desc), intent(inout) :: d
      integer(c_int64_t), value :: out_len
    end function

    ! ---- field rendering: sum ws A W (and sum ws W) on the density render's nodes, ws = m sigma or (m / rho) sigma;
    ! values (sph_count doubles in the upload order, with field = SPH_RENDER_FIELD_VALUES) and host_weight are
    ! c_loc(...) or c_null_ptr
    integer(c_int) function sph_render_field(ctx, d, values, host_out, host_weight, out_len) bind(C, name='sph_render_field')
      import :: c_int, c_int64_t, c_ptr, c_double, sph_render_field_desc
      type(c_ptr), value :: ctx, values, host_weight
      type(sph_render_field_desc), intent(inout) :: d
      real(c_double), intent(out) :: host_out(*)
      integer(c_int64_t), value :: out_len
    end function
    integer(c_int) function sph_render_field_dev(ctx, d, d_values, d_out, d_weight, out_len) &
        bind(C, name='sph_render_field_dev')
      import :: c_int, c_int64_t, c_ptr, sph_render_field_desc
      type(c_ptr), value :: ctx, d_values, d_out, d_weight
      type(sph_render_field_desc), intent(inout) :: d
      integer(c_int64_t), value :: out_len
    end function

    ! ---- disc profiles: host_sums / host_table are c_loc(...) or c_null_ptr (not both); sph_profile_finish is host code
    integer(c_int) function sph_profile(ctx, d, host_sums, host_table, n_bins) bind(C, name='sph_profile')
      import :: c_int, c_int64_t, c_ptr, sph_profile_desc
      type(c_ptr), value :: ctx, host_sums, host_table
      type(sph_profile_desc), intent(inout) :: d
      integer(c_int64_t), value :: n_bins
    end function
    integer(c_int) function sph_profile_dev(ctx, d, d_sums, n_bins) bind(C, name='sph_profile_dev')
      import :: c_int, c_int64_t, c_ptr, sph_profile_desc
      type(c_ptr), value :: ctx, d_sums
      type(sph_profile_desc), intent(inout) :: d
      integer(c_int64_t), value :: n_bins
    end function
    integer(c_int) function sph_profile_finish(d, p, sums, table, n_bins) bind(C, name='sph_profile_finish')
      import :: c_int, c_int64_t, c_double, sph_profile_desc, sph_params
      type(sph_profile_desc), intent(in) :: d
      type(sph_params), intent(in) :: p
      real(c_double), intent(in) :: sums(*)
      real(c_double), intent(out) :: table(*)
      integer(c_int64_t), value :: n_bins
    end function

    ! ---- conserved totals and the potential: host_sums (SPH_ENERGY_NSUM doubles) / host_phi (sph_count doubles, the
    !      download order) are c_loc(...) or c_null_ptr (not both); src_offset: this rank's first source (external sources)
    integer(c_int) function sph_energy(ctx, src_offset, host_sums, host_phi, n_phi) bind(C, name='sph_energy')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, host_sums, host_phi
      integer(c_int64_t), value :: src_offset, n_phi
    end function
    integer(c_int) function sph_energy_dev(ctx, src_offset, d_sums, d_phi, n_phi) bind(C, name='sph_energy_dev')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_sums, d_phi
      integer(c_int64_t), value :: src_offset, n_phi
    end function

    ! ---- friends-of-friends groups: host_labels (int32, sph_count of them, the download order) / host_table
    !      (SPH_GROUPS_NCOL doubles per group, max_groups groups) are c_loc(...) or c_null_ptr; n_groups: the full count
    integer(c_int) function sph_groups(ctx, d, host_labels, n_labels, host_table, max_groups, n_groups) &
        bind(C, name='sph_groups')
      import :: c_int, c_int64_t, c_ptr, sph_groups_desc
      type(c_ptr), value :: ctx, host_labels, host_table
      type(sph_groups_desc), intent(in) :: d
      integer(c_int64_t), value :: n_labels, max_groups
      integer(c_int64_t), intent(out) :: n_groups
    end function
    integer(c_int) function sph_groups_dev(ctx, d, d_labels, n_labels, d_table, max_groups, d_n_groups) &
        bind(C, name='sph_groups_dev')
      import :: c_int, c_int64_t, c_ptr, sph_groups_desc
      type(c_ptr), value :: ctx, d_labels, d_table, d_n_groups
      type(sph_groups_desc), intent(in) :: d
      integer(c_int64_t), value :: n_labels, max_groups
    end function
    ! ---- density-peak clumps: as sph_groups, with counts (SPH_PEAKS_NCOUNT int64: groups, raw peaks, edges) in place
    !      of the count and SPH_PEAKS_NCOL doubles per table row
    integer(c_int) function sph_peaks(ctx, d, host_labels, n_labels, host_table, max_groups, counts) &
        bind(C, name='sph_peaks')
      import :: c_int, c_int64_t, c_ptr, sph_peaks_desc
      type(c_ptr), value :: ctx, host_labels, host_table
      type(sph_peaks_desc), intent(in) :: d
      integer(c_int64_t), value :: n_labels, max_groups
      integer(c_int64_t), intent(out) :: counts(*)
    end function
    integer(c_int) function sph_peaks_dev(ctx, d, d_labels, n_labels, d_table, max_groups, d_counts) &
        bind(C, name='sph_peaks_dev')
      import :: c_int, c_int64_t, c_ptr, sph_peaks_desc
      type(c_ptr), value :: ctx, d_labels, d_table, d_counts
      type(sph_peaks_desc), intent(in) :: d
      integer(c_int64_t), value :: n_labels, max_groups
    end function
    ! ---- SPH gradients: values (n_fields rows of sph_count doubles, download order, or c_null_ptr), host_out
    !      (3 n_fields sph_count doubles), host_rho (sph_count doubles or c_null_ptr); n_targets, n_singular: the counts
    integer(c_int) function sph_gradients(ctx, d, values, host_out, n_out, host_rho, n_targets, n_singular) &
        bind(C, name='sph_gradients')
      import :: c_int, c_int64_t, c_ptr, sph_gradients_desc
      type(c_ptr), value :: ctx, values, host_out, host_rho
      type(sph_gradients_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
      integer(c_int64_t), intent(out) :: n_targets, n_singular
    end function
    integer(c_int) function sph_gradients_dev(ctx, d, d_values, d_out, n_out, d_rho, d_counts) &
        bind(C, name='sph_gradients_dev')
      import :: c_int, c_int64_t, c_ptr, sph_gradients_desc
      type(c_ptr), value :: ctx, d_values, d_out, d_rho, d_counts
      type(sph_gradients_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    ! ---- SPH interpolation at points: px, py, pz (n_points doubles each), values (n_fields rows of sph_count doubles,
    !      download order, or c_null_ptr), host_out (n_fields n_points doubles or c_null_ptr with n_fields == 0), host_weight
    !      (n_points doubles, or c_null_ptr unless n_fields == 0), counts (2 x int64: reached, non-finite; or c_null_ptr)
    integer(c_int) function sph_sample(ctx, d, n_points, px, py, pz, values, host_out, n_out, host_weight, counts) &
        bind(C, name='sph_sample')
      import :: c_int, c_int64_t, c_ptr, sph_sample_desc
      type(c_ptr), value :: ctx, px, py, pz, values, host_out, host_weight, counts
      type(sph_sample_desc), intent(in) :: d
      integer(c_int64_t), value :: n_points, n_out
    end function
    integer(c_int) function sph_sample_dev(ctx, d, n_points, d_px, d_py, d_pz, d_values, d_out, n_out, d_weight, d_counts) &
        bind(C, name='sph_sample_dev')
      import :: c_int, c_int64_t, c_ptr, sph_sample_desc
      type(c_ptr), value :: ctx, d_px, d_py, d_pz, d_values, d_out, d_weight, d_counts
      type(sph_sample_desc), intent(in) :: d
      integer(c_int64_t), value :: n_points, n_out
    end function
    ! ---- field lines: sx, sy, sz (n_seeds doubles each), values (rows of sph_count doubles, download order, or c_null_ptr),
    !      host_path (3 (n_rec + 1) n_seeds doubles), host_carry ((n_rec + 1) n_seeds doubles, or c_null_ptr without a carry),
    !      host_status and host_n_done (n_seeds int32 each), counts (5 x int64: the seeds per status code; or c_null_ptr)
    integer(c_int) function sph_trace(ctx, d, n_seeds, sx, sy, sz, values, host_path, n_path, host_carry, host_status, &
                                      host_n_done, counts) bind(C, name='sph_trace')
      import :: c_int, c_int64_t, c_ptr, sph_trace_desc
      type(c_ptr), value :: ctx, sx, sy, sz, values, host_path, host_carry, host_status, host_n_done, counts
      type(sph_trace_desc), intent(in) :: d
      integer(c_int64_t), value :: n_seeds, n_path
    end function
    integer(c_int) function sph_trace_dev(ctx, d, n_seeds, d_sx, d_sy, d_sz, d_values, d_path, n_path, d_carry, d_status, &
                                          d_n_done, d_counts) bind(C, name='sph_trace_dev')
      import :: c_int, c_int64_t, c_ptr, sph_trace_desc
      type(c_ptr), value :: ctx, d_sx, d_sy, d_sz, d_values, d_path, d_carry, d_status, d_n_done, d_counts
      type(sph_trace_desc), intent(in) :: d
      integer(c_int64_t), value :: n_seeds, n_path
    end function
    ! ---- potential and acceleration at points: px, py, pz (n_points doubles each), ph (n_points softening lengths or
    !      c_null_ptr), host_out (4 n_points doubles, 8 n_points with SPH_GRAVAT_SPLIT), counts (2 x int64: points with a
    !      non-finite coordinate, points with a bad softening length; or c_null_ptr)
    integer(c_int) function sph_gravity_at(ctx, d, n_points, px, py, pz, ph, host_out, n_out, counts) &
        bind(C, name='sph_gravity_at')
      import :: c_int, c_int64_t, c_ptr, sph_gravity_at_desc
      type(c_ptr), value :: ctx, px, py, pz, ph, host_out, counts
      type(sph_gravity_at_desc), intent(in) :: d
      integer(c_int64_t), value :: n_points, n_out
    end function
    integer(c_int) function sph_gravity_at_dev(ctx, d, n_points, d_px, d_py, d_pz, d_ph, d_out, n_out, d_counts) &
        bind(C, name='sph_gravity_at_dev')
      import :: c_int, c_int64_t, c_ptr, sph_gravity_at_desc
      type(c_ptr), value :: ctx, d_px, d_py, d_pz, d_ph, d_out, d_counts
      type(sph_gravity_at_desc), intent(in) :: d
      integer(c_int64_t), value :: n_points, n_out
    end function
    ! ---- binding energies and unbinding of groups: labels (sph_count int32: the group of every particle, e.g. what
    !      sph_groups wrote), bound_labels (sph_count int32), host_out (2 sph_count doubles: e, then Phi), host_table
    !      (SPH_BOUND_NCOL doubles per group), counts (4 x int64: members, groups skipped, dissolved, stopped at
    !      max_rounds); every output is c_loc(...) or c_null_ptr, at least one given
    integer(c_int) function sph_bound(ctx, d, labels, n_labels, n_groups, bound_labels, host_out, n_out, host_table, counts) &
        bind(C, name='sph_bound')
      import :: c_int, c_int64_t, c_ptr, sph_bound_desc
      type(c_ptr), value :: ctx, labels, bound_labels, host_out, host_table, counts
      type(sph_bound_desc), intent(in) :: d
      integer(c_int64_t), value :: n_labels, n_groups, n_out
    end function
    integer(c_int) function sph_bound_dev(ctx, d, d_labels, n_labels, n_groups, d_bound_labels, d_out, n_out, d_table, &
                                          d_counts) bind(C, name='sph_bound_dev')
      import :: c_int, c_int64_t, c_ptr, sph_bound_desc
      type(c_ptr), value :: ctx, d_labels, d_bound_labels, d_out, d_table, d_counts
      type(sph_bound_desc), intent(in) :: d
      integer(c_int64_t), value :: n_labels, n_groups, n_out
    end function
    ! ---- spectral cubes: values (sph_count doubles in the download order, or c_null_ptr: A = 1), host_out (n_chan n_u n_v
    !      doubles, C order [k][iu][iv]), out_len = n_chan n_u n_v
    integer(c_int) function sph_cube(ctx, d, values, host_out, out_len) bind(C, name='sph_cube')
      import :: c_int, c_int64_t, c_ptr, sph_cube_desc
      type(c_ptr), value :: ctx, values, host_out
      type(sph_cube_desc), intent(in) :: d
      integer(c_int64_t), value :: out_len
    end function
    integer(c_int) function sph_cube_dev(ctx, d, d_values, d_out, out_len) bind(C, name='sph_cube_dev')
      import :: c_int, c_int64_t, c_ptr, sph_cube_desc
      type(c_ptr), value :: ctx, d_values, d_out
      type(sph_cube_desc), intent(in) :: d
      integer(c_int64_t), value :: out_len
    end function
    ! ---- emission-absorption images: source, kappa (sph_count doubles in the download order with SPH_TRANSFER_VALUES, else
    !      c_null_ptr), host_out (4 n_u n_v doubles, C order [plane][iu][iv]), out_len = 4 n_u n_v
    integer(c_int) function sph_transfer(ctx, d, source, kappa, host_out, out_len) bind(C, name='sph_transfer')
      import :: c_int, c_int64_t, c_ptr, sph_transfer_desc
      type(c_ptr), value :: ctx, source, kappa, host_out
      type(sph_transfer_desc), intent(in) :: d
      integer(c_int64_t), value :: out_len
    end function
    integer(c_int) function sph_transfer_dev(ctx, d, d_source, d_kappa, d_out, out_len) bind(C, name='sph_transfer_dev')
      import :: c_int, c_int64_t, c_ptr, sph_transfer_desc
      type(c_ptr), value :: ctx, d_source, d_kappa, d_out
      type(sph_transfer_desc), intent(in) :: d
      integer(c_int64_t), value :: out_len
    end function
    ! ---- the rates split by term: host_out / d_out (SPH_TERMS_NROW sph_count doubles, C order [row][id]), n_out = their number;
    !      the state sph_forces needs (after sph_step: call sph_density first)
    integer(c_int) function sph_force_terms(ctx, d, host_out, n_out) bind(C, name='sph_force_terms')
      import :: c_int, c_int64_t, c_ptr, sph_force_terms_desc
      type(c_ptr), value :: ctx, host_out
      type(sph_force_terms_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    integer(c_int) function sph_force_terms_dev(ctx, d, d_out, n_out) bind(C, name='sph_force_terms_dev')
      import :: c_int, c_int64_t, c_ptr, sph_force_terms_desc
      type(c_ptr), value :: ctx, d_out
      type(sph_force_terms_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    ! ---- binned sums: values / d_values (n_rows sph_count doubles or c_null_ptr), edges (host memory in both forms, or
    !      c_null_ptr), sums (n_sums doubles), counts (3 int64 or c_null_ptr: selected, outside, dropped as NaN)
    integer(c_int) function sph_binned(ctx, d, values, edges, host_sums, n_sums, counts) bind(C, name='sph_binned')
      import :: c_int, c_int64_t, c_ptr, sph_binned_desc
      type(c_ptr), value :: ctx, values, edges, host_sums, counts
      type(sph_binned_desc), intent(in) :: d
      integer(c_int64_t), value :: n_sums
    end function
    integer(c_int) function sph_binned_dev(ctx, d, d_values, edges, d_sums, n_sums, d_counts) bind(C, name='sph_binned_dev')
      import :: c_int, c_int64_t, c_ptr, sph_binned_desc
      type(c_ptr), value :: ctx, d_values, edges, d_sums, d_counts
      type(sph_binned_desc), intent(in) :: d
      integer(c_int64_t), value :: n_sums
    end function
    ! the edge table the call uses for an axis (0 or 1): out holds n(axis + 1) + 1 doubles; host only, no context
    integer(c_int) function sph_binned_edges(d, edges, axis, out) bind(C, name='sph_binned_edges')
      import :: c_int, c_int32_t, c_double, c_ptr, sph_binned_desc
      type(sph_binned_desc), intent(in) :: d
      type(c_ptr), value :: edges
      integer(c_int32_t), value :: axis
      real(c_double), intent(out) :: out(*)
    end function
    ! ---- pair sums: values / d_values (n_rows sph_count doubles or c_null_ptr), edges (host memory in both forms, or
    !      c_null_ptr), sums (n_out doubles), raw (2 n_out 64-bit limbs or c_null_ptr), exps (nsum int32 or c_null_ptr),
    !      counts (3 int64 or c_null_ptr: targets, sources, not usable)
    integer(c_int) function sph_pairs(ctx, d, values, edges, host_sums, n_out, host_raw, exps, counts) bind(C, name='sph_pairs')
      import :: c_int, c_int64_t, c_ptr, sph_pairs_desc
      type(c_ptr), value :: ctx, values, edges, host_sums, host_raw, exps, counts
      type(sph_pairs_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    integer(c_int) function sph_pairs_dev(ctx, d, d_values, edges, d_sums, n_out, d_raw, d_exps, d_counts) &
        bind(C, name='sph_pairs_dev')
      import :: c_int, c_int64_t, c_ptr, sph_pairs_desc
      type(c_ptr), value :: ctx, d_values, edges, d_sums, d_raw, d_exps, d_counts
      type(sph_pairs_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    ! the edge table the call uses: out holds n_bins + 1 doubles; host only, no context
    integer(c_int) function sph_pairs_edges(d, edges, out) bind(C, name='sph_pairs_edges')
      import :: c_int, c_double, c_ptr, sph_pairs_desc
      type(sph_pairs_desc), intent(in) :: d
      type(c_ptr), value :: edges
      real(c_double), intent(out) :: out(*)
    end function
    ! raw limbs (2, nsum, n_bins) and their exponents -> the correctly rounded doubles (nsum, n_bins); host only, no context
    integer(c_int) function sph_pairs_finish(d, exps, raw, sums) bind(C, name='sph_pairs_finish')
      import :: c_int, c_int32_t, c_int64_t, c_double, sph_pairs_desc
      type(sph_pairs_desc), intent(in) :: d
      integer(c_int32_t), intent(in) :: exps(*)
      integer(c_int64_t), intent(in) :: raw(*)
      real(c_double), intent(out) :: sums(*)
    end function
    ! ---- mode sums: values, host_sums, host_raw, exp, ring_counts and counts are c_loc(...) (c_null_ptr where the header
    !      allows NULL); the _dev form takes device memory
    integer(c_int) function sph_modes(ctx, d, values, host_sums, n_out, host_raw, exp, ring_counts, counts) bind(C, name='sph_modes')
      import :: c_int, c_int64_t, c_ptr, sph_modes_desc
      type(c_ptr), value :: ctx, values, host_sums, host_raw, exp, ring_counts, counts
      type(sph_modes_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    integer(c_int) function sph_modes_dev(ctx, d, d_values, d_sums, n_out, d_raw, d_exp, d_ring_counts, d_counts) &
        bind(C, name='sph_modes_dev')
      import :: c_int, c_int64_t, c_ptr, sph_modes_desc
      type(c_ptr), value :: ctx, d_values, d_sums, d_raw, d_exp, d_ring_counts, d_counts
      type(sph_modes_desc), intent(in) :: d
      integer(c_int64_t), value :: n_out
    end function
    ! the tables the call uses: edges_out holds n_r + 1 doubles, p_out n_p (at least 1); host only, no context
    integer(c_int) function sph_modes_tables(d, edges_out, p_out) bind(C, name='sph_modes_tables')
      import :: c_int, c_double, sph_modes_desc
      type(sph_modes_desc), intent(in) :: d
      real(c_double), intent(out) :: edges_out(*), p_out(*)
    end function
    ! raw limbs (2, n_out) and their exponent -> the correctly rounded doubles (n_out); host only, no context
    integer(c_int) function sph_modes_finish(d, exp, raw, sums) bind(C, name='sph_modes_finish')
      import :: c_int, c_int32_t, c_int64_t, c_double, sph_modes_desc
      type(sph_modes_desc), intent(in) :: d
      integer(c_int32_t), intent(in) :: exp
      integer(c_int64_t), intent(in) :: raw(*)
      real(c_double), intent(out) :: sums(*)
    end function
    ! ---- the per-step time series: begin / end / record; info's outputs and read's host_out (count rows of the width info
    !      returns) are c_loc(...) (info's may be c_null_ptr); d_out is device memory
    integer(c_int) function sph_history_begin(ctx, d) bind(C, name='sph_history_begin')
      import :: c_int, c_ptr, sph_history_desc
      type(c_ptr), value :: ctx
      type(sph_history_desc), intent(in) :: d
    end function
    integer(c_int) function sph_history_end(ctx) bind(C, name='sph_history_end')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_history_record(ctx) bind(C, name='sph_history_record')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_history_info(ctx, rows, dropped, steps, width) bind(C, name='sph_history_info')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, rows, dropped, steps, width
    end function
    integer(c_int) function sph_history_read(ctx, first, count, host_out) bind(C, name='sph_history_read')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, host_out
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_history_read_dev(ctx, first, count, d_out) bind(C, name='sph_history_read_dev')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_out
      integer(c_int64_t), value :: first, count
    end function
    ! ---- tracked particles: ids are 0-based indices in the upload order; info's outputs, read's head and body and the fates
    !      are c_loc(...) (info's and either of read's may be c_null_ptr); the d_ arguments are device memory
    integer(c_int) function sph_track_begin(ctx, d, n_ids, ids) bind(C, name='sph_track_begin')
      import :: c_int, c_int64_t, c_ptr, sph_track_desc
      type(c_ptr), value :: ctx
      type(sph_track_desc), intent(in) :: d
      integer(c_int64_t), value :: n_ids
      integer(c_int64_t), intent(in) :: ids(*)
    end function
    integer(c_int) function sph_track_begin_dev(ctx, d, n_ids, d_ids) bind(C, name='sph_track_begin_dev')
      import :: c_int, c_int64_t, c_ptr, sph_track_desc
      type(c_ptr), value :: ctx, d_ids
      type(sph_track_desc), intent(in) :: d
      integer(c_int64_t), value :: n_ids
    end function
    integer(c_int) function sph_track_end(ctx) bind(C, name='sph_track_end')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_track_record(ctx) bind(C, name='sph_track_record')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_track_info(ctx, rows, dropped, steps, n_tracked, n_live, closed) bind(C, name='sph_track_info')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, rows, dropped, steps, n_tracked, n_live, closed
    end function
    integer(c_int) function sph_track_read(ctx, first, count, host_head, host_body) bind(C, name='sph_track_read')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, host_head, host_body
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_track_read_dev(ctx, first, count, d_head, d_body) bind(C, name='sph_track_read_dev')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_head, d_body
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_track_fates(ctx, host_fates) bind(C, name='sph_track_fates')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, host_fates
    end function
    integer(c_int) function sph_track_fates_dev(ctx, d_fates) bind(C, name='sph_track_fates_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, d_fates
    end function
    ! ---- tracer grains: begin's seven arrays of m are x y z vx vy vz par; info's outputs, read's head and body, state's arrays
    !      and the fates are c_loc(...) (info's and either of read's may be c_null_ptr); the d_ arguments are device memory
    integer(c_int) function sph_dust_begin(ctx, d, m, x, y, z, vx, vy, vz, par) bind(C, name='sph_dust_begin')
      import :: c_int, c_int64_t, c_double, c_ptr, sph_dust_desc
      type(c_ptr), value :: ctx
      type(sph_dust_desc), intent(in) :: d
      integer(c_int64_t), value :: m
      real(c_double), intent(in) :: x(*), y(*), z(*), vx(*), vy(*), vz(*), par(*)
    end function
    integer(c_int) function sph_dust_begin_dev(ctx, d, m, d_x, d_y, d_z, d_vx, d_vy, d_vz, d_par) bind(C, name='sph_dust_begin_dev')
      import :: c_int, c_int64_t, c_ptr, sph_dust_desc
      type(c_ptr), value :: ctx, d_x, d_y, d_z, d_vx, d_vy, d_vz, d_par
      type(sph_dust_desc), intent(in) :: d
      integer(c_int64_t), value :: m
    end function
    integer(c_int) function sph_dust_end(ctx) bind(C, name='sph_dust_end')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_dust_advance(ctx) bind(C, name='sph_dust_advance')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_dust_info(ctx, rows, dropped, advances, n_grains, n_live) bind(C, name='sph_dust_info')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, rows, dropped, advances, n_grains, n_live
    end function
    integer(c_int) function sph_dust_read(ctx, first, count, host_head, host_body) bind(C, name='sph_dust_read')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, host_head, host_body
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_dust_read_dev(ctx, first, count, d_head, d_body) bind(C, name='sph_dust_read_dev')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_head, d_body
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_dust_state(ctx, x, y, z, vx, vy, vz, par) bind(C, name='sph_dust_state')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, x, y, z, vx, vy, vz, par
    end function
    integer(c_int) function sph_dust_state_dev(ctx, d_x, d_y, d_z, d_vx, d_vy, d_vz, d_par) bind(C, name='sph_dust_state_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, d_x, d_y, d_z, d_vx, d_vy, d_vz, d_par
    end function
    integer(c_int) function sph_dust_fates(ctx, host_fates) bind(C, name='sph_dust_fates')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, host_fates
    end function
    integer(c_int) function sph_dust_fates_dev(ctx, d_fates) bind(C, name='sph_dust_fates_dev')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, d_fates
    end function
    ! ---- frames: info's outputs and read's head and planes are c_loc(...) (any of them may be c_null_ptr); the d_ arguments
    !      are device memory
    integer(c_int) function sph_frames_begin(ctx, d) bind(C, name='sph_frames_begin')
      import :: c_int, c_ptr, sph_frames_desc
      type(c_ptr), value :: ctx
      type(sph_frames_desc), intent(in) :: d
    end function
    integer(c_int) function sph_frames_end(ctx) bind(C, name='sph_frames_end')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_frames_record(ctx) bind(C, name='sph_frames_record')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_frames_rewind(ctx) bind(C, name='sph_frames_rewind')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx
    end function
    integer(c_int) function sph_frames_info(ctx, rows, dropped, steps) bind(C, name='sph_frames_info')
      import :: c_int, c_ptr
      type(c_ptr), value :: ctx, rows, dropped, steps
    end function
    integer(c_int) function sph_frames_read(ctx, first, count, host_head, host_planes) bind(C, name='sph_frames_read')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, host_head, host_planes
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_frames_read_dev(ctx, first, count, d_head, d_planes) bind(C, name='sph_frames_read_dev')
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: ctx, d_head, d_planes
      integer(c_int64_t), value :: first, count
    end function
    integer(c_int) function sph_frame(ctx, d, host_head, host_planes, out_len) bind(C, name='sph_frame')
      import :: c_int, c_int64_t, c_ptr, sph_frames_desc
      type(c_ptr), value :: ctx, host_head, host_planes
      type(sph_frames_desc), intent(in) :: d
      integer(c_int64_t), value :: out_len
    end function
    integer(c_int) function sph_frame_dev(ctx, d, d_head, d_planes, out_len) bind(C, name='sph_frame_dev')
      import :: c_int, c_int64_t, c_ptr, sph_frames_desc
      type(c_ptr), value :: ctx, d_head, d_planes
      type(sph_frames_desc), intent(in) :: d
      integer(c_int64_t), value :: out_len
    end function
  end interface

contains

  ! copies a NUL-terminated C string into a Fortran string
  function c_message(cp) result(s)
    type(c_ptr), intent(in) :: cp
    character(len=:), allocatable :: s
    character(kind=c_char), pointer :: chars(:)
    integer :: k
    s = ''
    if (.not. c_associated(cp)) return
    call c_f_pointer(cp, chars, [4096])
    do k = 1, 4096
      if (chars(k) == c_null_char) exit
      s = s // chars(k)
    end do
  end function c_message

  ! The hosts' optional history file: where the environment variable SPH_HISTORY_FILE names a file, begins a history of
  ! max_rows rows (every step, the per-sink columns of n_sinks sinks) and returns the name in path; on = .false. and no
  ! call otherwise, so that a run without the variable is exactly the run it was.  The hosts pass max_rows = the step limit,
  ! at most 100000 (a run without a step limit holds 100000 rows, 38 MB with one sink): the rows of later steps are dropped
  ! and counted in the file's '#' line.  A name that does not fit path is refused (status 1, SPH_ERR_ARG), not cut short.
  integer(c_int) function sph_history_begin_env(ctx, max_rows, n_sinks, path, on) result(st)
    type(c_ptr), intent(in) :: ctx
    integer, intent(in) :: max_rows, n_sinks
    character(len=*), intent(out) :: path
    logical, intent(out) :: on
    type(sph_history_desc) :: d
    integer :: stat
    st = SPH_OK
    call get_environment_variable('SPH_HISTORY_FILE', path, status=stat)
    on = stat == 0 .and. len_trim(path) > 0
    if (stat == -1) st = 1_c_int
    if (.not. on) return
    d%capacity = int(max(1, max_rows), c_int32_t)
    d%every = 1_c_int32_t
    d%max_sinks = int(max(0, min(n_sinks, 64)), c_int32_t)
    d%flags = 0_c_int32_t
    st = sph_history_begin(ctx, d)
  end function sph_history_begin_env

  ! writes the rows recorded so far as text, one line per row (a '#' line with the counts first), and ends the history
  integer(c_int) function sph_history_write(ctx, path) result(st)
    type(c_ptr), intent(in) :: ctx
    character(len=*), intent(in) :: path
    integer(c_int64_t), target :: rows, dropped, steps
    integer(c_int32_t), target :: width
    real(c_double), allocatable, target :: buf(:, :)
    integer :: u, k
    st = sph_history_info(ctx, c_loc(rows), c_loc(dropped), c_loc(steps), c_loc(width))
    if (st /= SPH_OK) return
    allocate(buf(width, max(rows, 1_c_int64_t)))
    st = sph_history_read(ctx, 0_c_int64_t, rows, c_loc(buf))
    if (st /= SPH_OK) return                             ! nothing is written and the history stays begun
    open(newunit=u, file=trim(path), status='replace', action='write')
    write(u, '(A,I0,A,I0,A,I0,A,I0)') '# sph_history rows ', rows, ' dropped ', dropped, ' steps ', steps, ' width ', width
    do k = 1, int(rows)
      write(u, '(*(ES25.17E3,1X))') buf(:, k)
    end do
    close(u)
    st = sph_history_end(ctx)
  end function sph_history_write

  ! The hosts' optional trajectory file: where the environment variable SPH_TRACK_FILE names a file, begins a tracker of every
  ! SPH_TRACK_STRIDE-th of the n particles (default 100; 0-based ids 0, stride, 2 stride ...) with max_rows rows, records the
  ! state as it is and returns the name in path; on = .false. and no call otherwise, so that a run without the variable is
  ! exactly the run it was.  The hosts pass max_rows = the step limit + 1; the log holds at most 1000000 / the tracked count
  ! + 1 rows (80 MB of row-particles), later rows are dropped and counted in the file's first line.
  integer(c_int) function sph_track_begin_env(ctx, n, max_rows, path, on) result(st)
    type(c_ptr), intent(in) :: ctx
    integer, intent(in) :: n, max_rows
    character(len=*), intent(out) :: path
    logical, intent(out) :: on
    type(sph_track_desc) :: d
    integer(c_int64_t), allocatable :: ids(:)
    character(len=32) :: word
    integer :: stat, stride, k, nk, ios
    st = SPH_OK
    call get_environment_variable('SPH_TRACK_FILE', path, status=stat)
    on = stat == 0 .and. len_trim(path) > 0 .and. n > 0
    if (stat == -1) st = 1_c_int
    if (.not. on) return
    stride = 100
    call get_environment_variable('SPH_TRACK_STRIDE', word, status=stat)
    if (stat == 0 .and. len_trim(word) > 0) then
      read(word, *, iostat=ios) stride
      if (ios /= 0 .or. stride < 1) then
        st = 1_c_int
        return
      end if
    end if
    nk = (n + stride - 1) / stride
    allocate(ids(nk))
    do k = 1, nk
      ids(k) = int(k - 1, c_int64_t) * int(stride, c_int64_t)
    end do
    d%capacity = int(max(1, min(max_rows, 1000000 / nk + 1)), c_int64_t)
    d%every = 1_c_int32_t
    d%flags = 0_c_int32_t
    st = sph_track_begin(ctx, d, int(nk, c_int64_t), ids)
    if (st == SPH_OK) st = sph_track_record(ctx)
  end function sph_track_begin_env

  ! writes the rows recorded so far as text: a '#' line with the counts, one line per row and tracked particle (the row's
  ! step and t, the tracked index k from 0, then x y z vx vy vz u rho h alpha), a '# fates' line and one line per tracked
  ! particle (k, fate, step, sink, current id); ends the tracker
  integer(c_int) function sph_track_write(ctx, path) result(st)
    type(c_ptr), intent(in) :: ctx
    character(len=*), intent(in) :: path
    integer(c_int64_t), target :: rows, dropped, steps, nk, live
    integer(c_int32_t), target :: closed
    real(c_double), allocatable, target :: head(:, :), body(:, :, :)
    integer(c_int32_t), allocatable, target :: fates(:, :)
    integer :: u, r, k
    st = sph_track_info(ctx, c_loc(rows), c_loc(dropped), c_loc(steps), c_loc(nk), c_loc(live), c_loc(closed))
    if (st /= SPH_OK) return
    allocate(head(SPH_TRACK_NHEAD, max(rows, 1_c_int64_t)), body(nk, SPH_TRACK_NCOL, max(rows, 1_c_int64_t)), fates(4, nk))
    st = sph_track_read(ctx, 0_c_int64_t, rows, c_loc(head), c_loc(body))
    if (st == SPH_OK) st = sph_track_fates(ctx, c_loc(fates))
    if (st /= SPH_OK) return                             ! nothing is written and the tracker stays begun
    open(newunit=u, file=trim(path), status='replace', action='write')
    write(u, '(A,I0,A,I0,A,I0,A,I0,A,I0,A,I0)') '# sph_track rows ', rows, ' dropped ', dropped, ' steps ', steps, &
      ' tracked ', nk, ' live ', live, ' closed ', closed
    do r = 1, int(rows)
      do k = 1, int(nk)
        write(u, '(I0,1X,ES25.17E3,1X,I0,10(1X,ES25.17E3))') int(head(1, r), c_int64_t), head(2, r), k - 1, body(k, :, r)
      end do
    end do
    write(u, '(A)') '# fates: k fate step sink current_id'
    do k = 1, int(nk)
      write(u, '(I0,4(1X,I0))') k - 1, fates(:, k)
    end do
    close(u)
    st = sph_track_end(ctx)
  end function sph_track_write

  ! The hosts' optional movie file: where the environment variable SPH_FRAMES_FILE names a file, begins a log of face-on
  ! column-density maps (looking down z) over the node box lo .. hi -- the hosts pass the initial bounding box of the gas in x
  ! and y -- on SPH_FRAMES_SIZE x SPH_FRAMES_SIZE nodes (default 256), a frame every SPH_FRAMES_DT of simulation time or,
  ! without that variable, every SPH_FRAMES_EVERY-th step (default 10), and returns the name in path; on = .false. and no
  ! call otherwise, so that a run without the variable is exactly the run it was.  The log holds max_rows frames, at most
  ! 2^27 doubles (1 GB): later frames are dropped and counted in the file's header.  nodes: the image size chosen.
  integer(c_int) function sph_frames_begin_env(ctx, lo, hi, max_rows, path, on, nodes) result(st)
    type(c_ptr), intent(in) :: ctx
    real(c_double), intent(in) :: lo(2), hi(2)
    integer, intent(in) :: max_rows
    character(len=*), intent(out) :: path
    logical, intent(out) :: on
    integer, intent(out) :: nodes                         ! the image is nodes x nodes (sph_frames_write wants it)
    type(sph_frames_desc) :: d
    character(len=64) :: word
    integer :: stat, ios, n, every
    real(c_double) :: dtf
    st = SPH_OK
    call get_environment_variable('SPH_FRAMES_FILE', path, status=stat)
    on = stat == 0 .and. len_trim(path) > 0
    if (stat == -1) st = 1_c_int
    nodes = 0
    if (.not. on) return
    n = 256
    every = 10
    dtf = 0.0_c_double
    call get_environment_variable('SPH_FRAMES_SIZE', word, status=stat)
    if (stat == 0 .and. len_trim(word) > 0) then
      read(word, *, iostat=ios) n
      if (ios /= 0 .or. n < 1 .or. n > 8192) st = 1_c_int
    end if
    call get_environment_variable('SPH_FRAMES_EVERY', word, status=stat)
    if (stat == 0 .and. len_trim(word) > 0) then
      read(word, *, iostat=ios) every
      if (ios /= 0 .or. every < 1) st = 1_c_int
    end if
    call get_environment_variable('SPH_FRAMES_DT', word, status=stat)
    if (stat == 0 .and. len_trim(word) > 0) then
      read(word, *, iostat=ios) dtf
      if (ios /= 0 .or. .not. dtf > 0.0_c_double) st = 1_c_int
      every = 0
    end if
    if (st /= SPH_OK) return
    nodes = n
    d%rot = [1.0_c_double, 0.0_c_double, 0.0_c_double, 0.0_c_double, 1.0_c_double, 0.0_c_double, 0.0_c_double, 0.0_c_double, &
             1.0_c_double]
    d%centre = 0.0_c_double
    d%lo = lo
    d%hi = hi
    d%clip_lo = -huge(1.0_c_double)
    d%clip_hi = huge(1.0_c_double)
    d%h = 0.0_c_double
    d%dt_frame = dtf
    d%capacity = int(max(1, min(max_rows, 2**27 / (n * n))), c_int64_t)
    d%n_u = int(n, c_int32_t)
    d%n_v = int(n, c_int32_t)
    d%every = int(every, c_int32_t)
    d%centre_sink = -1_c_int32_t
    d%nq = 0_c_int32_t
    d%fields = 0_c_int32_t
    d%reserved = 0_c_int64_t
    st = sph_frames_begin(ctx, d)
  end function sph_frames_begin_env

  ! writes the frames recorded so far as one unformatted stream -- four int64 (rows, dropped, steps, n: the image is n x n,
  ! one plane), then the heads (16 doubles per frame), then the planes (n n doubles per frame, [row][iu][iv] as C has
  ! them) -- and ends the log
  integer(c_int) function sph_frames_write(ctx, path, n) result(st)
    type(c_ptr), intent(in) :: ctx
    character(len=*), intent(in) :: path
    integer, intent(in) :: n
    integer(c_int64_t), target :: rows, dropped, steps
    real(c_double), allocatable, target :: head(:, :), planes(:, :, :)
    integer :: u
    st = sph_frames_info(ctx, c_loc(rows), c_loc(dropped), c_loc(steps))
    if (st /= SPH_OK) return
    allocate(head(SPH_FRAMES_NHEAD, max(rows, 1_c_int64_t)), planes(n, n, max(rows, 1_c_int64_t)))
    st = sph_frames_read(ctx, 0_c_int64_t, rows, c_loc(head), c_loc(planes))
    if (st /= SPH_OK) return                             ! nothing is written and the log stays begun
    open(newunit=u, file=trim(path), status='replace', action='write', access='stream', form='unformatted')
    write(u) rows, dropped, steps, int(n, c_int64_t)
    write(u) head(:, 1:rows)
    write(u) planes(:, :, 1:rows)
    close(u)
    st = sph_frames_end(ctx)
  end function sph_frames_write
end module sph_hip_binding
