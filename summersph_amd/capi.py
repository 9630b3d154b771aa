"""ctypes binding of the C ABI (include/summersph.h) for the Python harness (tests, bench).

This is plumbing only: every call goes straight to libsummersph_hip.so.  There is no fallback;
if the library is missing or no GPU is present the constructors raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libsummersph_hip.so")
LIB_PATH = os.environ.get("SUMMERSPH_LIB", LIB_PATH)      # A/B builds of the same ABI (profiles/)
_D = C.POINTER(C.c_double)

FIELDS = ["x", "y", "z", "vx", "vy", "vz", "u", "m", "alpha", "rho", "P", "c", "ax", "ay", "az", "du", "dalpha", "h", "omega"]
KERNELS = ["grid", "nlist", "density", "forces", "sinkacc", "kick", "drift", "dt", "leaf", "update_h", "gravity", "grav_walk", "reflag"]
FLAG_REUSE_DENSITY = 1
FLAG_VARIABLE_H = 2
FLAG_NO_LDS_TILES = 4
FLAG_SELF_GRAVITY = 16
FLAG_ACCRETE_CULL = 32
FLAG_SINK_CREATION = 64
FLAG_NO_WHOLE_TILE = 128
FLAG_REUSE_GRAVITY = 256
FLAG_NO_REFLAG = 512
FLAG_HASHED_GRID = 1024

# every symbol include/summersph.h declares (tests check that the library exports them all)
SYMBOLS = [
    "sph_set_sink_radii", "sph_accrete_and_cull", "sph_accrete_and_cull_keep",
    "sph_params_default", "sph_params_default_variable", "sph_upload_field", "sph_upload_field_dev", "sph_update_h",
    "sph_ctx_create", "sph_ctx_destroy", "sph_strerror", "sph_last_error", "sph_abi_version", "sph_get_params",
    "sph_upload", "sph_upload_dev", "sph_set_sinks", "sph_get_sinks", "sph_count", "sph_sink_count", "sph_check_sink_creation", "sph_get_sink_radii", "sph_sink_candidate_dev", "sph_add_sink_checked_dev",
    "sph_density", "sph_forces", "sph_kick", "sph_drift", "sph_next_dt", "sph_step", "sph_run",
    "sph_download_field", "sph_download_field_dev", "sph_download_state",
    "sph_gather_fields_dev", "sph_scatter_fields_dev",
    "sph_set_owned", "sph_set_rank", "sph_scatter_field_dev", "sph_refresh_eos", "sph_refresh_eos_ghosts", "sph_dt_candidate", "sph_set_sink_accel",
    "sph_set_stream", "sph_reserve", "sph_owned_bbox", "sph_select_boxes", "sph_selected_ids_dev", "sph_select_boxes_async", "sph_selected_counts", "sph_gather_selected_dev", "sph_replace_ghosts_dev",
    "sph_set_dt", "sph_get_dt", "sph_kick_devdt", "sph_drift_devdt", "sph_dt_candidate_dev", "sph_kick_drift_devdt", "sph_kick_dt_candidate_dev", "sph_kick_dt_candidate_gas_dev", "sph_kick_sinks_devdt", "sph_pack_partials_dev", "sph_pack_partials_ex_dev",
    "sph_apply_partials_dev", "sph_set_boundary_boxes", "sph_forces_part", "sph_set_gravity_sources_dev", "sph_accrete_mark_dev", "sph_accrete_apply_dev", "sph_set_numbers_dev",
    "sph_get_stats", "sph_get_grid_info", "sph_get_bbox", "sph_timing_enable", "sph_timing_stride", "sph_timing_reset", "sph_timing_get", "sph_synchronize", "sph_stream",
    "sph_render_density", "sph_render_density_dev", "sph_render_field", "sph_render_field_dev",
    "sph_profile", "sph_profile_dev", "sph_profile_finish",
    "sph_energy", "sph_energy_dev",
    "sph_groups", "sph_groups_dev",
    "sph_peaks", "sph_peaks_dev",
    "sph_gradients", "sph_gradients_dev",
    "sph_sample", "sph_sample_dev",
    "sph_trace", "sph_trace_dev",
    "sph_gravity_at", "sph_gravity_at_dev",
    "sph_bound", "sph_bound_dev",
    "sph_cube", "sph_cube_dev",
    "sph_transfer", "sph_transfer_dev",
    "sph_force_terms", "sph_force_terms_dev",
    "sph_binned", "sph_binned_dev", "sph_binned_edges",
    "sph_pairs", "sph_pairs_dev", "sph_pairs_edges", "sph_pairs_finish",
    "sph_modes", "sph_modes_dev", "sph_modes_tables", "sph_modes_finish",
    "sph_history_begin", "sph_history_end", "sph_history_record", "sph_history_info", "sph_history_read", "sph_history_read_dev",
    "sph_track_begin", "sph_track_begin_dev", "sph_track_end", "sph_track_record", "sph_track_info", "sph_track_read",
    "sph_track_read_dev", "sph_track_fates", "sph_track_fates_dev",
    "sph_frames_begin", "sph_frames_end", "sph_frames_record", "sph_frames_rewind", "sph_frames_info", "sph_frames_read",
    "sph_frames_read_dev", "sph_frame", "sph_frame_dev",
    "sph_dust_begin", "sph_dust_begin_dev", "sph_dust_end", "sph_dust_advance", "sph_dust_info", "sph_dust_read",
    "sph_dust_read_dev", "sph_dust_state", "sph_dust_state_dev", "sph_dust_fates", "sph_dust_fates_dev",
]
RENDER_AUTO_BOUNDS = 1
RENDER_SPACING = 2
RENDER_FIELD_VALUES = -1
RENDER_WEIGHT_MASS = 0
RENDER_WEIGHT_VOLUME = 1
PROFILE_LOG = 1
PROFILE_AUTO_NORMAL = 2
PROFILE_NSUM = 20
PROFILE_NCOL = 29
# sph_profile_finish's columns (include/summersph.h, "Table") and the raw sums' order ("Sums")
PROFILE_COLUMNS = ["R_lo", "R_hi", "R_mean", "N", "M", "Sigma", "z_mean", "H", "vR_mean", "vphi_mean", "vz_mean", "sigma_R",
                   "sigma_phi", "sigma_z", "u_mean", "c_s", "alpha_mean", "h_mean", "Omega", "kappa", "Q", "Mdot", "j", "tilt",
                   "twist", "ecc", "peri", "phi_lo", "phi_hi"]
ENERGY_NSUM = 28
# sph_energy's sums (include/summersph.h, "Sums"): the gas part (additive over contexts and ranks), then the sink part
# (rank 0 only)
ENERGY_SUMS = ["N", "M", "mx", "my", "mz", "px", "py", "pz", "lx", "ly", "lz", "K", "U", "W_self", "W_gs",
               "Ns", "Ms", "Mx_s", "My_s", "Mz_s", "Px_s", "Py_s", "Pz_s", "Lx_s", "Ly_s", "Lz_s", "K_s", "W_ss"]
HISTORY_NHEAD = 40
HISTORY_MAX_SINKS = 64
# a row of sph_history (include/summersph.h, "Row"): the head's HISTORY_NHEAD columns, then 7 per kept sink
HISTORY_SINK_COLUMNS = ["x", "y", "z", "vx", "vy", "vz", "m"]
HISTORY_COLUMNS = (["step", "t", "dt_next", "dt_cand", "n", "ns"] + ENERGY_SUMS +
                   ["rho_max", "densest", "densest_x", "densest_y", "densest_z", "v_max"])
TRACK_NHEAD = 4
TRACK_NCOL = 10
# a row of sph_track (include/summersph.h, "Row"): the head's columns, the per-particle columns of the body, the fates' entries
TRACK_HEAD = ["step", "t", "n", "n_live"]
TRACK_COLUMNS = ["x", "y", "z", "vx", "vy", "vz", "u", "rho", "h", "alpha"]
TRACK_FATES = ["fate", "step", "sink", "current_id"]
TRACK_ALIVE, TRACK_ACCRETED, TRACK_CULLED = 0, 1, 2
DUST_NHEAD = 4
DUST_NCOL = 12
# a row of sph_dust (include/summersph.h, "Row"): the head's columns, the per-grain columns of the body, the fates' entries
DUST_HEAD = ["advance", "t", "delta", "n_live"]
DUST_COLUMNS = ["x", "y", "z", "vx", "vy", "vz", "rho_g", "u_g", "vgx", "vgy", "vgz", "rate"]
DUST_FATES = ["fate", "advance", "sink"]
DUST_STATE = ["x", "y", "z", "vx", "vy", "vz", "par"]
DUST_ALIVE, DUST_ACCRETED, DUST_CULLED, DUST_NONFINITE = 0, 1, 2, 3
DUST_EPSTEIN, DUST_FIXED_TS = 0, 1
DUST_LAWS = {"epstein": DUST_EPSTEIN, "fixed_ts": DUST_FIXED_TS}
DUST_REMOVE = 1
FRAMES_NHEAD = 16
FRAMES_MAX_FIELDS = 3
FRAMES_MAX_SINKS = 64
FRAMES_OK, FRAMES_SINK_GONE = 0, 1
GROUPS_LINK_H = 1
GROUPS_NCOL = 21
# sph_groups' table columns (include/summersph.h, "Table")
GROUPS_COLUMNS = ["N", "M", "x", "y", "z", "vx", "vy", "vz", "r_rms", "r_max", "Sx", "Sy", "Sz", "K_int", "U", "rho_max",
                  "x_dense", "y_dense", "z_dense", "id_dense", "id_min"]
PEAKS_LINK_H = 1
PEAKS_NCOL = 23
PEAKS_NCOUNT = 3
# sph_peaks' table columns (include/summersph.h, "Table"): sph_groups' columns, the highest saddle towards another
# component and the raw peaks merged into this one; and its counts
PEAKS_COLUMNS = GROUPS_COLUMNS + ["S_out", "n_peaks"]
PEAKS_COUNTS = ["n_groups", "n_raw_peaks", "n_edges"]
GRAD_CORRECTED = 1
GRAD_MAX_FIELDS = 4
GRAD_VALUES = -1
SAMPLE_NORMALISE = 1
SAMPLE_MAX_FIELDS = 4
SAMPLE_VALUES = -1
TRACE_ARCLENGTH = 1
TRACE_PLANAR = 2
TRACE_VALUES = -1
TRACE_NONE = -2
# sph_trace's status codes (include/summersph.h, "Stops")
TRACE_DONE, TRACE_LEFT_GAS, TRACE_LEFT_BOX, TRACE_STAGNANT, TRACE_NONFINITE = range(5)
TRACE_STATUS = ["done", "left_gas", "left_box", "stagnant", "nonfinite"]
GRAVAT_GAS = 1
GRAVAT_SINKS = 2
GRAVAT_SPLIT = 4
GRAVAT_REF_SOFT2 = 0.001 * 2.5      # the force walk's softening term (0.001_dp * smoothing)
CUBE_PER_VELOCITY = 1
CUBE_CHUNK = 32               # channels per workgroup of cube_gather (csrc/cube.hip, CUBE_CHUNK): more run in several chunks
TRANSFER_VALUES = -1
TRANSFER_ONE = -2
# sph_transfer's planes (include/summersph.h, "Output")
TRANSFER_PLANES = ["intensity", "tau", "transmission", "surface"]
TERMS_NROW = 16
TERMS_SKIP_GAS_GRAVITY = 1
# sph_force_terms' rows (include/summersph.h, "Rows"): pressure gradient, artificial viscosity, sink gravity, gas
# self-gravity, PdV work, viscous heating, the two addends of the alpha rate
TERM_ROWS = ["aP_x", "aP_y", "aP_z", "aV_x", "aV_y", "aV_z", "aS_x", "aS_y", "aS_z", "aG_x", "aG_y", "aG_z",
             "du_P", "du_V", "dalpha_source", "dalpha_decay"]
BINNED_MAX_Q = 8
BINNED_MAX_ROWS = 16
BINNED_W_ONE, BINNED_W_MASS, BINNED_W_VOLUME = 0, 1, 2
BINNED_WEIGHTS = {"one": BINNED_W_ONE, "mass": BINNED_W_MASS, "volume": BINNED_W_VOLUME}
BINNED_LOG0, BINNED_LOG1, BINNED_EDGES0, BINNED_EDGES1, BINNED_SQUARES, BINNED_SKIP_NAN = 1, 2, 4, 8, 16, 32
PAIRS_MAX_Q = 4
PAIRS_MAX_BINS = 1024
PAIRS_W_ONE, PAIRS_W_MASS = 0, 1
PAIRS_WEIGHTS = {"one": PAIRS_W_ONE, "mass": PAIRS_W_MASS}
PAIRS_LOG, PAIRS_EDGES, PAIRS_SCALE_H, PAIRS_VELOCITY = 1, 2, 4, 8
MODES_MAX_M = 8
MODES_MAX_RINGS = 1024
MODES_MAX_P = 256
MODES_W_ONE, MODES_W_MASS = 0, 1
MODES_WEIGHTS = {"one": MODES_W_ONE, "mass": MODES_W_MASS}
MODES_LOG = 1
# sph_modes' counts (include/summersph.h, "Outputs")
MODES_COUNTS = ["selected", "outside", "not_usable", "at_centre"]
BOUND_THERMAL = 1
BOUND_NCOL = 24
# sph_bound's table columns (include/summersph.h, "Outputs"): S_0's, the last evaluated set's, the outcome
BOUND_COLUMNS = ["N0", "M0", "K0", "U0", "W0", "E0", "virial0", "N", "M", "x", "y", "z", "vx", "vy", "vz", "K", "U", "W", "E",
                 "n_bound", "rounds", "status", "id_most_bound", "e_most_bound"]
BOUND_STATUS = ["converged", "max_rounds", "dissolved", "skipped"]
BOUND_COUNTS = ["members", "skipped", "dissolved", "max_rounds"]
PROFILE_SUMS = ["N", "M", "mR", "mz", "mzz", "mvR", "mvphi", "mvz", "mvRvR", "mvphivphi", "mvzvz", "mu", "malpha", "mh",
                "mlx", "mly", "mlz", "mex", "mey", "mez"]


class Params(C.Structure):
    _fields_ = [("h", C.c_double), ("gamma", C.c_double), ("gamma_m1", C.c_double), ("nq", C.c_int32),
                ("flags", C.c_int32), ("kernel_pi", C.c_double), ("visc_eps", C.c_double),
                ("alpha_floor", C.c_double), ("alpha_decay", C.c_double), ("G", C.c_double),
                ("dt_scale", C.c_double), ("dt_max", C.c_double), ("dt_min", C.c_double),
                ("bounding_size", C.c_double), ("eta", C.c_double), ("h_tol", C.c_double),
                ("h_max_length", C.c_double), ("h_min_length", C.c_double), ("h_iter_cap", C.c_double),
                ("theta", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_cells", C.c_int64), ("grid_dim", C.c_int32 * 3),
                ("nlist_capacity", C.c_int32), ("nlist_max", C.c_int32), ("tile_fit_pct", C.c_int32), ("nlist_mean", C.c_double),
                ("grid_builds", C.c_int64), ("nlist_builds", C.c_int64), ("density_passes", C.c_int64),
                ("force_passes", C.c_int64), ("device_bytes", C.c_int64), ("nlist_wave_mean", C.c_double),
                ("tile_fit_pct_forces", C.c_int32), ("host_syncs", C.c_int32), ("lane_efficiency_forces", C.c_double), ("nlist_reflags", C.c_int64)]


class GridInfo(C.Structure):
    """sph_grid_info (include/summersph.h): kind 0 dense / 1 hashed / -1 none, cells per axis, occupied cells, table
    entries, indexed cells (dim product) and the table's device bytes"""
    _fields_ = [("kind", C.c_int32), ("dim", C.c_int32 * 3), ("occupied_cells", C.c_int64), ("table_entries", C.c_int64),
                ("index_cells", C.c_double), ("bytes", C.c_int64)]


class RenderDesc(C.Structure):
    """sph_render_desc (include/summersph.h): node box, strict clip box, h, nodes per axis, output axis, flags"""
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3),
                ("h", C.c_double), ("n", C.c_int32 * 3), ("axis", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class RenderFieldDesc(C.Structure):
    """sph_render_field_desc (include/summersph.h): the density render's descriptor, field id (or RENDER_FIELD_VALUES),
    weight (RENDER_WEIGHT_MASS / _VOLUME), normalise (0 / 1), reserved"""
    _fields_ = [("base", RenderDesc), ("field", C.c_int32), ("weight", C.c_int32), ("normalise", C.c_int32),
                ("reserved", C.c_int32)]


class ProfileDesc(C.Structure):
    """sph_profile_desc (include/summersph.h): centre and its velocity, central mass, normal (written back normalised),
    ring range, z cut, rings, sectors, sink (-1: none), flags (PROFILE_LOG | PROFILE_AUTO_NORMAL), reserved"""
    _fields_ = [("centre", C.c_double * 3), ("centre_v", C.c_double * 3), ("central_mass", C.c_double),
                ("normal", C.c_double * 3), ("r_min", C.c_double), ("r_max", C.c_double), ("z_max", C.c_double),
                ("n_r", C.c_int32), ("n_phi", C.c_int32), ("sink", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class GroupsDesc(C.Structure):
    """sph_groups_desc (include/summersph.h): linking length, rho cut, strict clip box, min_members, flags
    (GROUPS_LINK_H), reserved"""
    _fields_ = [("link", C.c_double), ("rho_min", C.c_double), ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3),
                ("min_members", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32)]


def groups_desc(link, rho_min=-np.inf, min_members=1, link_h=False, clip=None) -> GroupsDesc:
    """The descriptor of Context.groups' arguments (see there)."""
    d = GroupsDesc()
    d.link, d.rho_min, d.min_members = float(link), float(rho_min), int(min_members)
    d.flags = GROUPS_LINK_H if link_h else 0
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    d.clip_lo[:] = [float(v) for v in lo]
    d.clip_hi[:] = [float(v) for v in hi]
    return d


def groups_table(table: np.ndarray) -> np.ndarray:
    """(n, GROUPS_NCOL) float64 -> a structured array of n records with the GROUPS_COLUMNS names"""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, GROUPS_NCOL)
    return t.view([(c, np.float64) for c in GROUPS_COLUMNS]).reshape(-1)


class PeaksDesc(C.Structure):
    """sph_peaks_desc (include/summersph.h): neighbour radius, rho cut, peak cut, contrast, strict clip box, min_members,
    flags (PEAKS_LINK_H), reserved"""
    _fields_ = [("link", C.c_double), ("rho_min", C.c_double), ("peak_min", C.c_double), ("contrast", C.c_double),
                ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("min_members", C.c_int64), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


def peaks_desc(link, contrast=2.0, rho_min=-np.inf, peak_min=-np.inf, min_members=1, link_h=False, clip=None) -> PeaksDesc:
    """The descriptor of Context.peaks' arguments (see there)."""
    d = PeaksDesc()
    d.link, d.rho_min, d.peak_min, d.contrast = float(link), float(rho_min), float(peak_min), float(contrast)
    d.min_members = int(min_members)
    d.flags = PEAKS_LINK_H if link_h else 0
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    d.clip_lo[:] = [float(v) for v in lo]
    d.clip_hi[:] = [float(v) for v in hi]
    return d


def peaks_table(table: np.ndarray) -> np.ndarray:
    """(n, PEAKS_NCOL) float64 -> a structured array of n records with the PEAKS_COLUMNS names"""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, PEAKS_NCOL)
    return t.view([(c, np.float64) for c in PEAKS_COLUMNS]).reshape(-1)


class GradientsDesc(C.Structure):
    """sph_gradients_desc (include/summersph.h): strict target clip box, h (0: each particle's own), field ids (SPH_F_* or
    GRAD_VALUES), n_fields, flags (GRAD_CORRECTED), reserved"""
    _fields_ = [("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("h", C.c_double),
                ("fields", C.c_int32 * GRAD_MAX_FIELDS), ("n_fields", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 2)]


def gradients_desc(fields=("vx", "vy", "vz"), corrected=True, h=None, clip=None) -> GradientsDesc:
    """The descriptor of Context.gradients' arguments (fields: SPH_F_* names or ids, or GRAD_VALUES; see there)."""
    fields = list(fields)
    if not 1 <= len(fields) <= GRAD_MAX_FIELDS:
        raise ValueError(f"gradients: 1 .. {GRAD_MAX_FIELDS} fields, not {len(fields)}")
    d = GradientsDesc()
    d.fields[:] = [FIELDS.index(f) if isinstance(f, str) else int(f) for f in fields] + [0] * (GRAD_MAX_FIELDS - len(fields))
    d.n_fields = len(fields)
    d.flags = GRAD_CORRECTED if corrected else 0
    d.h = 0.0 if h is None else float(h)
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    d.clip_lo[:] = [float(v) for v in lo]
    d.clip_hi[:] = [float(v) for v in hi]
    return d


class SampleDesc(C.Structure):
    """sph_sample_desc (include/summersph.h): strict source clip box, h (0: each particle's own), field ids (SPH_F_* or
    SAMPLE_VALUES), n_fields (0: the weight alone), weight (RENDER_WEIGHT_MASS / _VOLUME), flags (SAMPLE_NORMALISE), reserved"""
    _fields_ = [("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("h", C.c_double),
                ("fields", C.c_int32 * SAMPLE_MAX_FIELDS), ("n_fields", C.c_int32), ("weight", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


def sample_desc(fields=(), weight="mass", normalise=False, h=None, clip=None) -> SampleDesc:
    """The descriptor of Context.sample's arguments (fields: SPH_F_* names or ids, or SAMPLE_VALUES; see there)."""
    fields = list(fields)
    if len(fields) > SAMPLE_MAX_FIELDS:
        raise ValueError(f"sample: 0 .. {SAMPLE_MAX_FIELDS} fields, not {len(fields)}")
    d = SampleDesc()
    d.fields[:] = [FIELDS.index(f) if isinstance(f, str) else int(f) for f in fields] + [0] * (SAMPLE_MAX_FIELDS - len(fields))
    d.n_fields = len(fields)
    d.weight = {"mass": RENDER_WEIGHT_MASS, "volume": RENDER_WEIGHT_VOLUME}[weight] if isinstance(weight, str) else int(weight)
    d.flags = SAMPLE_NORMALISE if normalise else 0
    d.h = 0.0 if h is None else float(h)
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    d.clip_lo[:] = [float(v) for v in lo]
    d.clip_hi[:] = [float(v) for v in hi]
    return d


class TraceDesc(C.Structure):
    """sph_trace_desc (include/summersph.h): sph_sample's source clip box and h, the tracers' box, the step ds, the frame
    (omega, centre), the PLANAR normal, the three component ids and the carry id (SPH_F_*, TRACE_VALUES; carry: TRACE_NONE),
    weight, n_steps, stride, flags (TRACE_ARCLENGTH | TRACE_PLANAR), reserved"""
    _fields_ = [("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("h", C.c_double),
                ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3), ("ds", C.c_double),
                ("omega", C.c_double * 3), ("centre", C.c_double * 3), ("normal", C.c_double * 3),
                ("fields", C.c_int32 * 3), ("carry", C.c_int32), ("weight", C.c_int32), ("n_steps", C.c_int32),
                ("stride", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


def trace_desc(n_steps, ds, fields=("vx", "vy", "vz"), carry=None, arclength=False, omega=None, centre=(0.0, 0.0, 0.0),
               normal=None, box=None, stride=1, weight="mass", h=None, clip=None) -> TraceDesc:
    """The descriptor of Context.trace's arguments (see there)."""
    fields = list(fields)
    if len(fields) != 3:
        raise ValueError(f"trace: three component fields, not {len(fields)}")

    def fid(f):
        return FIELDS.index(f) if isinstance(f, str) else int(f)
    d = TraceDesc()
    d.fields[:] = [fid(f) for f in fields]
    d.carry = TRACE_NONE if carry is None else fid(carry)
    d.weight = {"mass": RENDER_WEIGHT_MASS, "volume": RENDER_WEIGHT_VOLUME}[weight] if isinstance(weight, str) else int(weight)
    d.n_steps, d.stride, d.ds = int(n_steps), int(stride), float(ds)
    d.flags = (TRACE_ARCLENGTH if arclength else 0) | (TRACE_PLANAR if normal is not None else 0)
    d.h = 0.0 if h is None else float(h)
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    d.clip_lo[:] = [float(v) for v in lo]
    d.clip_hi[:] = [float(v) for v in hi]
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if box is None else box
    d.box_lo[:] = [float(v) for v in lo]
    d.box_hi[:] = [float(v) for v in hi]
    d.omega[:] = [0.0] * 3 if omega is None else [float(v) for v in omega]
    d.centre[:] = [float(v) for v in centre]
    d.normal[:] = [0.0] * 3 if normal is None else [float(v) for v in normal]
    return d


class GravityAtDesc(C.Structure):
    """sph_gravity_at_desc (include/summersph.h): h (0: params.h; unused with ph), soft2, flags (GRAVAT_*), reserved"""
    _fields_ = [("h", C.c_double), ("soft2", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


def gravity_at_desc(h=None, soft2=GRAVAT_REF_SOFT2, gas=True, sinks=True, split=False) -> GravityAtDesc:
    """The descriptor of Context.gravity_at's arguments."""
    d = GravityAtDesc()
    d.h = 0.0 if h is None else float(h)
    d.soft2 = float(soft2)
    d.flags = (GRAVAT_GAS if gas else 0) | (GRAVAT_SINKS if sinks else 0) | (GRAVAT_SPLIT if split else 0)
    return d


class BoundDesc(C.Structure):
    """sph_bound_desc (include/summersph.h): h (0: each particle's own), soft2, min_members, max_members (cost cap),
    max_rounds (0: evaluate once), flags (BOUND_THERMAL), reserved"""
    _fields_ = [("h", C.c_double), ("soft2", C.c_double), ("min_members", C.c_int64), ("max_members", C.c_int64),
                ("max_rounds", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class ForceTermsDesc(C.Structure):
    """sph_force_terms_desc (include/summersph.h): flags (TERMS_*), reserved"""
    _fields_ = [("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class BinnedDesc(C.Structure):
    _fields_ = [("lo", C.c_double * 2), ("hi", C.c_double * 2), ("axis", C.c_int32 * 2), ("n", C.c_int32 * 2),
                ("n_axes", C.c_int32), ("n_q", C.c_int32), ("q", C.c_int32 * BINNED_MAX_Q), ("weight", C.c_int32),
                ("n_rows", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


def binned_row(k: int) -> int:
    """the source id of row k of values (SPH_BINNED_ROW)"""
    return -1 - int(k)


def _binned_source(s) -> int:
    """a source: a field name, an SPH_F_* id, or a negative id from binned_row(k)"""
    return FIELDS.index(s) if isinstance(s, str) else int(s)


def binned_desc(axes, bins, ranges=None, edges=None, log=(), q=(), weight="mass", n_rows=0, squares=False, skip_nan=True):
    """(BinnedDesc, edge table or None) of a sph_binned call (include/summersph.h).  axes: one source or a sequence of one or
    two; bins: an int or one per axis; ranges: (lo, hi) per axis (or one pair with one axis), None for an axis that has
    edges; edges: None, or per axis None or its n + 1 edges (one axis: the array itself); log: the axes (0, 1) with
    logarithmic edges."""
    if isinstance(axes, (str, int, np.integer)):
        axes = (axes,)
    na = len(axes)
    if na not in (1, 2):
        raise ValueError("binned: one or two axes")
    bins = (int(bins),) * na if isinstance(bins, (int, np.integer)) else tuple(int(b) for b in bins)
    if len(bins) != na:
        raise ValueError("binned: one bin count per axis")
    if edges is None:
        edges = (None,) * na
    elif na == 1 and not (isinstance(edges, (tuple, list)) and len(edges) == 1 and (edges[0] is None or np.ndim(edges[0]) == 1)):
        edges = (edges,)
    if ranges is None:
        ranges = (None,) * na
    elif na == 1 and np.ndim(ranges) == 1 and len(ranges) == 2 and ranges[0] is not None and np.ndim(ranges[0]) == 0:
        ranges = (ranges,)
    if len(edges) != na or len(ranges) != na:
        raise ValueError("binned: ranges and edges go by axis")
    q = (q,) if isinstance(q, (str, int, np.integer)) else tuple(q)
    if len(q) > BINNED_MAX_Q:
        raise ValueError(f"binned: at most {BINNED_MAX_Q} quantities")
    d = BinnedDesc()
    d.n_axes, d.n_q, d.n_rows = na, len(q), int(n_rows)
    d.n[0], d.n[1] = bins[0], bins[1] if na == 2 else 1
    d.weight = BINNED_WEIGHTS[weight] if isinstance(weight, str) else int(weight)
    flags = (BINNED_SQUARES if squares else 0) | (BINNED_SKIP_NAN if skip_nan else 0)
    tables = []
    for a in range(na):
        d.axis[a] = _binned_source(axes[a])
        if edges[a] is not None:
            e = np.ascontiguousarray(edges[a], dtype=np.float64)
            if e.shape != (bins[a] + 1,):
                raise ValueError(f"binned: axis {a} wants {bins[a] + 1} edges")
            tables.append(e)
            flags |= BINNED_EDGES0 << a
        else:
            if ranges[a] is None:
                raise ValueError(f"binned: axis {a} needs a range or edges")
            d.lo[a], d.hi[a] = float(ranges[a][0]), float(ranges[a][1])
        if a in tuple(log):
            flags |= BINNED_LOG0 << a
    for k, s in enumerate(q):
        d.q[k] = _binned_source(s)
    d.flags = flags
    return d, (np.concatenate(tables) if tables else None)


def binned_nsum(n_q: int, squares: bool) -> int:
    return 2 + int(n_q) * (2 if squares else 1)


def binned_edges(desc: BinnedDesc, edges=None, axis: int = 0) -> np.ndarray:
    """the edge table sph_binned uses for an axis of the descriptor (pure host code: no context, no device)"""
    if not 0 <= int(axis) < 2:
        raise SphError(1, "axis out of range")
    out = np.empty(max(int(desc.n[int(axis)]), 0) + 1, dtype=np.float64)
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    st = load().sph_binned_edges(C.byref(desc), None if e is None else e.ctypes.data, int(axis), out.ctypes.data)
    if st != 0:
        raise SphError(st, load().sph_strerror(st).decode())
    return out


class PairsDesc(C.Structure):
    """sph_pairs_desc (include/summersph.h)"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3),
                ("n_bins", C.c_int32), ("n_q", C.c_int32), ("q", C.c_int32 * PAIRS_MAX_Q), ("weight", C.c_int32),
                ("n_rows", C.c_int32), ("flags", C.c_int32), ("target_stride", C.c_int32), ("target_phase", C.c_int32),
                ("reserved", C.c_int32 * 3)]


def pairs_row(k: int) -> int:
    """the source id of row k of values (SPH_PAIRS_ROW)"""
    return -1 - int(k)


def pairs_nsum(n_q: int, velocity: bool) -> int:
    return 2 + 2 * int(n_q) + (4 if velocity else 0)


def pairs_desc(r_range, bins, log=False, edges=None, scale_h=False, q=(), weight="one", velocity=False, clip=None, stride=1,
               phase=0, n_rows=0):
    """(PairsDesc, edge table or None) of a sph_pairs call (include/summersph.h).  r_range: (lo, hi) of the binned variable,
    None with edges (bins + 1 values); q: up to PAIRS_MAX_Q field names, SPH_F_* ids or pairs_row(k); clip: None or
    ((x0, y0, z0), (x1, y1, z1)), the targets' strict box."""
    q = (q,) if isinstance(q, (str, int, np.integer)) else tuple(q)
    if len(q) > PAIRS_MAX_Q:
        raise ValueError(f"pairs: at most {PAIRS_MAX_Q} quantities")
    d = PairsDesc()
    d.n_bins, d.n_q, d.n_rows = int(bins), len(q), int(n_rows)
    d.weight = PAIRS_WEIGHTS[weight] if isinstance(weight, str) else int(weight)
    d.target_stride, d.target_phase = int(stride), int(phase)
    flags = (PAIRS_LOG if log else 0) | (PAIRS_SCALE_H if scale_h else 0) | (PAIRS_VELOCITY if velocity else 0)
    tab = None
    if edges is not None:
        tab = np.ascontiguousarray(edges, dtype=np.float64)
        if tab.shape != (int(bins) + 1,):
            raise ValueError(f"pairs: {int(bins)} bins want {int(bins) + 1} edges")
        flags |= PAIRS_EDGES
    else:
        if r_range is None:
            raise ValueError("pairs: a range or edges")
        d.lo, d.hi = float(r_range[0]), float(r_range[1])
    lo, hi = ((-np.inf,) * 3, (np.inf,) * 3) if clip is None else clip
    d.clip_lo[:] = [float(v) for v in lo]
    d.clip_hi[:] = [float(v) for v in hi]
    for k, s in enumerate(q):
        d.q[k] = _binned_source(s)
    d.flags = flags
    return d, tab


def pairs_edges(desc: PairsDesc, edges=None) -> np.ndarray:
    """the edge table sph_pairs uses (pure host code: no context, no device)"""
    out = np.empty(min(max(int(desc.n_bins), 0), PAIRS_MAX_BINS) + 1, dtype=np.float64)
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    st = load().sph_pairs_edges(C.byref(desc), None if e is None else e.ctypes.data, out.ctypes.data)
    if st != 0:
        raise SphError(st, load().sph_strerror(st).decode() + " -- sph_pairs_edges")
    return out


def pairs_finish(desc: PairsDesc, exps, raw) -> np.ndarray:
    """sph_pairs_finish: raw limbs (n_bins, nsum, 2) uint64 -- e.g. those of several calls added with pairs.add_raw -- and
    their exponents -> the (n_bins, nsum) doubles, correctly rounded.  Host code only: no context, no device."""
    nsum = pairs_nsum(desc.n_q, bool(desc.flags & PAIRS_VELOCITY))
    r = np.ascontiguousarray(raw, dtype=np.uint64).reshape(int(desc.n_bins), nsum, 2)
    e = np.ascontiguousarray(exps, dtype=np.int32).reshape(nsum)
    out = np.empty((int(desc.n_bins), nsum))
    st = load().sph_pairs_finish(C.byref(desc), e.ctypes.data, r.ctypes.data, out.ctypes.data)
    if st != 0:
        raise SphError(st, load().sph_strerror(st).decode() + " -- sph_pairs_finish")
    return out


class ModesDesc(C.Structure):
    """sph_modes_desc (include/summersph.h)"""
    _fields_ = [("centre", C.c_double * 3), ("centre_v", C.c_double * 3), ("normal", C.c_double * 3), ("r_min", C.c_double),
                ("r_max", C.c_double), ("z_max", C.c_double), ("p_min", C.c_double), ("p_max", C.c_double), ("r_ref", C.c_double),
                ("n_r", C.c_int32), ("m_max", C.c_int32), ("n_p", C.c_int32), ("sink", C.c_int32), ("weight", C.c_int32),
                ("n_q", C.c_int32), ("q", C.c_int32), ("n_rows", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


def modes_row(k: int) -> int:
    """the source id of row k of values (SPH_MODES_ROW)"""
    return -1 - int(k)


def modes_desc(r_range, n_r, m_max, log=False, z_max=np.inf, centre=None, centre_v=None, sink=None, normal=(0.0, 0.0, 1.0),
               weight="mass", q=None, spiral=None, r_ref=1.0, n_rows=0) -> ModesDesc:
    """The descriptor of a sph_modes call (include/summersph.h).  r_range: (r_min, r_max); centre / centre_v: three numbers
    each (default 0), or sink: the index of the sink the frame is centred on; q: None (A = 1), a field name, an SPH_F_* id
    or modes_row(k); spiral: None or (p_min, p_max, n_p)."""
    d = ModesDesc()
    d.r_min, d.r_max, d.z_max = float(r_range[0]), float(r_range[1]), float(z_max)
    d.n_r, d.m_max, d.n_rows = int(n_r), int(m_max), int(n_rows)
    d.flags = MODES_LOG if log else 0
    d.weight = MODES_WEIGHTS[weight] if isinstance(weight, str) else int(weight)
    if sink is not None:
        if centre is not None or centre_v is not None:
            raise ValueError("modes: give centre / centre_v or sink, not both")
        d.sink = int(sink)
    else:
        d.sink = -1
        if centre is not None:
            d.centre[:] = [float(v) for v in centre]
        if centre_v is not None:
            d.centre_v[:] = [float(v) for v in centre_v]
    d.normal[:] = [float(v) for v in normal]
    if q is not None:
        d.n_q, d.q = 1, _binned_source(q)
    if spiral is not None:
        p_min, p_max, n_p = spiral
        d.p_min, d.p_max, d.n_p, d.r_ref = float(p_min), float(p_max), int(n_p), float(r_ref)
    return d


def _modes_sizes(desc: ModesDesc):
    """(n_r, m_max + 1, n_p) of a descriptor, clamped to what an array can be made for"""
    return (min(max(int(desc.n_r), 0), MODES_MAX_RINGS), min(max(int(desc.m_max), -1), MODES_MAX_M) + 1,
            min(max(int(desc.n_p), 0), MODES_MAX_P))


def modes_split(desc: ModesDesc, flat):
    """the flat output of sph_modes (sums, or raw with a last axis of 2 limbs) as (ring[n_r, m_max + 1, 2(, 2)],
    spiral[m_max + 1, n_p, 2(, 2)] or None): views, numpy or torch"""
    n_r, m1, n_p = _modes_sizes(desc)
    tail = tuple(flat.shape[1:])
    ring = flat[:n_r * m1 * 2].reshape((n_r, m1, 2) + tail)
    spiral = flat[n_r * m1 * 2:].reshape((m1, n_p, 2) + tail) if n_p > 0 else None
    return ring, spiral


def modes_tables(desc: ModesDesc):
    """(ring edges (n_r + 1,), p table (n_p,)) as sph_modes uses them (pure host code: no context, no device)"""
    n_r, _, n_p = _modes_sizes(desc)
    edges, p = np.empty(n_r + 1), np.empty(n_p)
    st = load().sph_modes_tables(C.byref(desc), edges.ctypes.data, p.ctypes.data)
    if st != 0:
        raise SphError(st, load().sph_strerror(st).decode() + " -- sph_modes_tables")
    return edges, p


def modes_finish(desc: ModesDesc, exp, raw):
    """sph_modes_finish: raw limbs -- the flat (n_out, 2) uint64 block, or the (ring, spiral) pair Context.modes returns,
    e.g. those of several calls added with modes.add_raw -- and their exponent -> (ring[n_r, m_max + 1, 2],
    spiral[m_max + 1, n_p, 2] or None) doubles, correctly rounded.  Host code only: no context, no device."""
    n_r, m1, n_p = _modes_sizes(desc)
    n_out = 2 * m1 * (n_r + n_p)
    if isinstance(raw, (tuple, list)):
        raw = np.concatenate([np.asarray(r).reshape(-1, 2) for r in raw if r is not None])
    r = np.asarray(raw)
    r = np.ascontiguousarray(r.view(np.uint64) if r.dtype == np.int64 else r, dtype=np.uint64).reshape(n_out, 2)
    e = np.array([int(np.asarray(exp).reshape(-1)[0])], dtype=np.int32)
    out = np.empty(n_out)
    st = load().sph_modes_finish(C.byref(desc), e.ctypes.data, r.ctypes.data, out.ctypes.data)
    if st != 0:
        raise SphError(st, load().sph_strerror(st).decode() + " -- sph_modes_finish")
    return modes_split(desc, out)


class HistoryDesc(C.Structure):
    """sph_history_desc (include/summersph.h)"""
    _fields_ = [("capacity", C.c_int32), ("every", C.c_int32), ("max_sinks", C.c_int32), ("flags", C.c_int32)]


def history_desc(capacity, every=1, max_sinks=0) -> HistoryDesc:
    """The HistoryDesc of a sph_history_begin call: capacity rows, every every-th step, max_sinks per-sink column groups."""
    capacity, every, max_sinks = int(capacity), int(every), int(max_sinks)
    if not 1 <= capacity < 2**31:
        raise ValueError("history: capacity must be 1 .. 2^31 - 1")
    if not 1 <= every < 2**31:
        raise ValueError("history: every must be 1 .. 2^31 - 1")
    if not 0 <= max_sinks <= HISTORY_MAX_SINKS:
        raise ValueError(f"history: max_sinks must be 0 .. {HISTORY_MAX_SINKS}")
    d = HistoryDesc()
    d.capacity, d.every, d.max_sinks, d.flags = capacity, every, max_sinks, 0
    return d


def history_width(max_sinks: int) -> int:
    return HISTORY_NHEAD + 7 * int(max_sinks)


def history_columns(rows, dropped=0) -> dict:
    """Raw history rows (R, HISTORY_NHEAD + 7 max_sinks) -> the dict Context.history returns: the head's columns by name
    (step, n, ns and densest as int64; densest is -1 where the row has none), the energy_total keys per row (E without
    W_self, P, L and com as (R, 3)), densest_pos (R, 3), sinks (R, max_sinks, 7), dropped and "rows", the raw array."""
    r = np.asarray(rows, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] < HISTORY_NHEAD or (r.shape[1] - HISTORY_NHEAD) % 7:
        raise ValueError("history: rows must be (R, HISTORY_NHEAD + 7 max_sinks)")
    out = {k: r[:, i] for i, k in enumerate(HISTORY_COLUMNS)}
    for k in ("step", "n", "ns"):
        out[k] = out[k].astype(np.int64)
    out["densest"] = np.where(np.isnan(out["densest"]), -1.0, out["densest"]).astype(np.int64)
    out["densest_pos"] = np.stack([out.pop("densest_x"), out.pop("densest_y"), out.pop("densest_z")], axis=1)
    s = r[:, 6:6 + ENERGY_NSUM]
    out["E"] = ((((s[:, 11] + s[:, 12]) + s[:, 13]) + s[:, 14]) + s[:, 26]) + s[:, 27]
    out["P"] = s[:, 5:8] + s[:, 20:23]
    out["L"] = s[:, 8:11] + s[:, 23:26]
    mt = s[:, 1] + s[:, 16]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["com"] = np.where((mt > 0)[:, None], (s[:, 2:5] + s[:, 17:20]) / mt[:, None], 0.0)
    out["sinks"] = r[:, HISTORY_NHEAD:].reshape(r.shape[0], (r.shape[1] - HISTORY_NHEAD) // 7, 7)
    out["dropped"] = int(dropped)
    out["rows"] = r
    return out


class FramesDesc(C.Structure):
    """sph_frames_desc (include/summersph.h): rot (rows u^, v^, w^), centre, image node box, strict clip box, h, dt_frame,
    capacity, image nodes, every, centre_sink, nq, fields, reserved"""
    _fields_ = [("rot", C.c_double * 9), ("centre", C.c_double * 3), ("lo", C.c_double * 2), ("hi", C.c_double * 2),
                ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("h", C.c_double), ("dt_frame", C.c_double),
                ("capacity", C.c_int64), ("n_u", C.c_int32), ("n_v", C.c_int32), ("every", C.c_int32),
                ("centre_sink", C.c_int32), ("nq", C.c_int32), ("fields", C.c_int32 * 3), ("reserved", C.c_int64)]


def frames_desc(shape, bounds, capacity=1, every=1, dt_frame=None, rot=None, centre=None, centre_sink=None, fields=(), h=None,
                clip=None) -> FramesDesc:
    """The descriptor of Context.frames_begin's and Context.frame's arguments (see there).  dt_frame given and every left at
    1: the cadence is dt_frame's (every = 0 in the descriptor); both given: both are passed on, which the library refuses."""
    n = (int(shape),) * 2 if np.isscalar(shape) else tuple(int(v) for v in shape)
    if len(n) != 2:
        raise ValueError("shape: one node count or (n_u, n_v)")
    fields = (fields,) if isinstance(fields, (str, int, np.integer)) else tuple(fields)
    if len(fields) > FRAMES_MAX_FIELDS:
        raise ValueError(f"frames: at most {FRAMES_MAX_FIELDS} fields")
    d = FramesDesc()
    d.rot[:] = np.asarray(np.eye(3) if rot is None else rot, dtype=np.float64).reshape(9).tolist()
    d.centre[:] = [float(v) for v in ((0.0, 0.0, 0.0) if centre is None else centre)]
    b = np.asarray(bounds, dtype=np.float64).reshape(2, 2)
    d.lo[:] = b[0].tolist(); d.hi[:] = b[1].tolist()
    cb = np.array([[-np.inf] * 3, [np.inf] * 3]) if clip is None else np.asarray(clip, dtype=np.float64).reshape(2, 3)
    d.clip_lo[:] = cb[0].tolist(); d.clip_hi[:] = cb[1].tolist()
    d.h = 0.0 if h is None else float(h)
    d.dt_frame = 0.0 if dt_frame is None else float(dt_frame)
    d.capacity = int(capacity)
    d.n_u, d.n_v = n
    d.every = 0 if (dt_frame is not None and int(every) == 1) else int(every)
    d.centre_sink = -1 if centre_sink is None else int(centre_sink)
    d.nq = len(fields)
    for k, f in enumerate(fields):
        d.fields[k] = FIELDS.index(f) if isinstance(f, str) else int(f)
    return d


def frames_columns(head, planes, dropped=0) -> dict:
    """Raw frames, head (R, FRAMES_NHEAD) and planes (R, 1 + nq, n_u, n_v), -> the dict Context.frames returns: step, n,
    n_sel and status as int64 (R,), t (R,), centre (R, 3), exp (R, 4; NaN where a plane is unused or NaN), planes, head and
    dropped."""
    hd = np.asarray(head, dtype=np.float64)
    if hd.ndim != 2 or hd.shape[1] != FRAMES_NHEAD:
        raise ValueError("frames: head must be (R, FRAMES_NHEAD)")
    return {"step": hd[:, 0].astype(np.int64), "t": hd[:, 1], "n": hd[:, 2].astype(np.int64), "n_sel": hd[:, 3].astype(np.int64),
            "centre": hd[:, 4:7], "exp": hd[:, 7:11], "status": hd[:, 11].astype(np.int64), "planes": planes, "head": hd,
            "dropped": int(dropped)}


class TrackDesc(C.Structure):
    """sph_track_desc (include/summersph.h)"""
    _fields_ = [("capacity", C.c_int64), ("every", C.c_int32), ("flags", C.c_int32)]


def track_desc(capacity, every=1) -> TrackDesc:
    """The TrackDesc of a sph_track_begin call: capacity rows, every every-th step."""
    capacity, every = int(capacity), int(every)
    if not 1 <= capacity < 2**63:
        raise ValueError("track: capacity must be 1 .. 2^63 - 1")
    if not 1 <= every < 2**31:
        raise ValueError("track: every must be 1 .. 2^31 - 1")
    d = TrackDesc()
    d.capacity, d.every, d.flags = capacity, every, 0
    return d


def track_ids(ids) -> np.ndarray:
    """The ids of a tracking set as a contiguous 1-D int64 array (at least one; integers only)"""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("track: ids must be a 1-D array of at least one integer")
    return np.ascontiguousarray(a, dtype=np.int64)


def track_columns(head, body, dropped=0) -> dict:
    """Raw tracker rows, head (R, TRACK_NHEAD) and body (R, TRACK_NCOL, K), -> the dict Context.track returns: step, n and
    n_live as int64 (R,), t (R,), one (R, K) view per name of TRACK_COLUMNS, body, head and dropped."""
    hd, bd = np.asarray(head, dtype=np.float64), np.asarray(body, dtype=np.float64)
    if hd.ndim != 2 or hd.shape[1] != TRACK_NHEAD or bd.ndim != 3 or bd.shape[1] != TRACK_NCOL or bd.shape[0] != hd.shape[0]:
        raise ValueError("track: head must be (R, TRACK_NHEAD) and body (R, TRACK_NCOL, K)")
    out = {k: hd[:, i] for i, k in enumerate(TRACK_HEAD)}
    for k in ("step", "n", "n_live"):
        out[k] = out[k].astype(np.int64)
    for i, k in enumerate(TRACK_COLUMNS):
        out[k] = bd[:, i, :]
    out["body"], out["head"], out["dropped"] = bd, hd, int(dropped)
    return out


def track_fates_columns(fates) -> dict:
    """Raw fates (K, 4) int32 -> {"fate", "step", "sink", "current_id"}: four (K,) arrays"""
    f = np.asarray(fates, dtype=np.int32)
    if f.ndim != 2 or f.shape[1] != len(TRACK_FATES):
        raise ValueError("track: fates must be (K, 4)")
    return {k: f[:, i] for i, k in enumerate(TRACK_FATES)}


class DustDesc(C.Structure):
    """sph_dust_desc (include/summersph.h)"""
    _fields_ = [("capacity", C.c_int64), ("every", C.c_int32), ("record_every", C.c_int32), ("law", C.c_int32),
                ("flags", C.c_int32), ("rho_grain", C.c_double)]


def dust_desc(law="epstein", rho_grain=None, capacity=0, every=1, record_every=1, remove=False) -> DustDesc:
    """The DustDesc of a sph_dust_begin call.  law: "epstein" (par is the grain size, rho_grain the grains' material
    density in code units) or "fixed_ts" (par is the stopping time); remove: SPH_DUST_REMOVE."""
    if law not in DUST_LAWS:
        raise ValueError(f"dust: law must be one of {sorted(DUST_LAWS)}")
    if law == "epstein" and rho_grain is None:
        raise ValueError("dust: the epstein law needs rho_grain")
    d = DustDesc()
    d.capacity, d.every, d.record_every = int(capacity), int(every), int(record_every)
    d.law, d.flags = DUST_LAWS[law], DUST_REMOVE if remove else 0
    d.rho_grain = 0.0 if rho_grain is None else float(rho_grain)
    return d


def dust_columns(head, body, dropped=0) -> dict:
    """Raw dust rows, head (R, DUST_NHEAD) and body (R, DUST_NCOL, M), -> the dict Context.dust returns: advance and n_live
    as int64 (R,), t and delta (R,), one (R, M) view per name of DUST_COLUMNS, body, head and dropped."""
    hd, bd = np.asarray(head, dtype=np.float64), np.asarray(body, dtype=np.float64)
    if hd.ndim != 2 or hd.shape[1] != DUST_NHEAD or bd.ndim != 3 or bd.shape[1] != DUST_NCOL or bd.shape[0] != hd.shape[0]:
        raise ValueError("dust: head must be (R, DUST_NHEAD) and body (R, DUST_NCOL, M)")
    out = {k: hd[:, i] for i, k in enumerate(DUST_HEAD)}
    for k in ("advance", "n_live"):
        out[k] = out[k].astype(np.int64)
    for i, k in enumerate(DUST_COLUMNS):
        out[k] = bd[:, i, :]
    out["body"], out["head"], out["dropped"] = bd, hd, int(dropped)
    return out


def bound_desc(h=None, soft2=GRAVAT_REF_SOFT2, thermal=False, max_rounds=0, min_members=1, max_members=2**31 - 1) -> BoundDesc:
    """The descriptor of Context.bound's arguments (see there)."""
    d = BoundDesc()
    d.h = 0.0 if h is None else float(h)
    d.soft2 = float(soft2)
    d.min_members, d.max_members, d.max_rounds = int(min_members), int(max_members), int(max_rounds)
    d.flags = BOUND_THERMAL if thermal else 0
    return d


class CubeDesc(C.Structure):
    """sph_cube_desc (include/summersph.h): rot (rows u^, v^, w^), centre, v_ref, image node box, strict clip box, h, channel 0's
    centre and the channel width, sigma_scale, sigma_floor, image nodes, channels, flags (CUBE_PER_VELOCITY), reserved"""
    _fields_ = [("rot", C.c_double * 9), ("centre", C.c_double * 3), ("v_ref", C.c_double * 3), ("lo", C.c_double * 2),
                ("hi", C.c_double * 2), ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("h", C.c_double),
                ("v0", C.c_double), ("dv", C.c_double), ("sigma_scale", C.c_double), ("sigma_floor", C.c_double),
                ("n_u", C.c_int32), ("n_v", C.c_int32), ("n_chan", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int64)]


def cube_desc(shape, bounds, v0, dv, n_chan, rot=None, centre=(0.0, 0.0, 0.0), v_ref=(0.0, 0.0, 0.0), sigma_scale=0.0,
              sigma_floor=0.0, h=None, clip=None, per_velocity=False) -> CubeDesc:
    """The descriptor of Context.cube's arguments (see there)."""
    n = (int(shape),) * 2 if np.isscalar(shape) else tuple(int(v) for v in shape)
    if len(n) != 2:
        raise ValueError("shape: one node count or (n_u, n_v)")
    d = CubeDesc()
    d.rot[:] = np.asarray(np.eye(3) if rot is None else rot, dtype=np.float64).reshape(9).tolist()
    d.centre[:] = [float(v) for v in centre]
    d.v_ref[:] = [float(v) for v in v_ref]
    b = np.asarray(bounds, dtype=np.float64).reshape(2, 2)
    d.lo[:] = b[0].tolist(); d.hi[:] = b[1].tolist()
    cb = np.array([[-np.inf] * 3, [np.inf] * 3]) if clip is None else np.asarray(clip, dtype=np.float64).reshape(2, 3)
    d.clip_lo[:] = cb[0].tolist(); d.clip_hi[:] = cb[1].tolist()
    d.h = 0.0 if h is None else float(h)
    d.v0, d.dv, d.n_chan = float(v0), float(dv), int(n_chan)
    d.sigma_scale, d.sigma_floor = float(sigma_scale), float(sigma_floor)
    d.n_u, d.n_v = n
    d.flags = CUBE_PER_VELOCITY if per_velocity else 0
    return d


class TransferDesc(C.Structure):
    """sph_transfer_desc (include/summersph.h): rot (rows u^, v^, w^), centre, image node box, strict clip box, h, kappa_scale,
    tau_surface, tau_max, background, image nodes, the selectors of S and K (a field id, TRANSFER_VALUES, TRANSFER_ONE),
    flags, reserved"""
    _fields_ = [("rot", C.c_double * 9), ("centre", C.c_double * 3), ("lo", C.c_double * 2), ("hi", C.c_double * 2),
                ("clip_lo", C.c_double * 3), ("clip_hi", C.c_double * 3), ("h", C.c_double), ("kappa_scale", C.c_double),
                ("tau_surface", C.c_double), ("tau_max", C.c_double), ("background", C.c_double), ("n_u", C.c_int32),
                ("n_v", C.c_int32), ("source", C.c_int32), ("kappa", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


def _transfer_selector(v) -> int:
    """None: the constant 1; a field name or id; anything else: the caller's array"""
    if v is None:
        return TRANSFER_ONE
    if isinstance(v, str):
        return FIELDS.index(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return TRANSFER_VALUES


def transfer_desc(shape, bounds, rot=None, centre=(0.0, 0.0, 0.0), source="u", kappa=None, kappa_scale=1.0, tau_surface=1.0,
                  tau_max=np.inf, background=0.0, h=None, clip=None) -> TransferDesc:
    """The descriptor of Context.transfer's arguments (see there); source and kappa arrays only set their selectors."""
    n = (int(shape),) * 2 if np.isscalar(shape) else tuple(int(v) for v in shape)
    if len(n) != 2:
        raise ValueError("shape: one node count or (n_u, n_v)")
    d = TransferDesc()
    d.rot[:] = np.asarray(np.eye(3) if rot is None else rot, dtype=np.float64).reshape(9).tolist()
    d.centre[:] = [float(v) for v in centre]
    b = np.asarray(bounds, dtype=np.float64).reshape(2, 2)
    d.lo[:] = b[0].tolist(); d.hi[:] = b[1].tolist()
    cb = np.array([[-np.inf] * 3, [np.inf] * 3]) if clip is None else np.asarray(clip, dtype=np.float64).reshape(2, 3)
    d.clip_lo[:] = cb[0].tolist(); d.clip_hi[:] = cb[1].tolist()
    d.h = 0.0 if h is None else float(h)
    d.kappa_scale, d.tau_surface, d.tau_max, d.background = float(kappa_scale), float(tau_surface), float(tau_max), float(background)
    d.n_u, d.n_v = n
    d.source, d.kappa = _transfer_selector(source), _transfer_selector(kappa)
    return d


def bound_table(table: np.ndarray) -> np.ndarray:
    """(n, BOUND_NCOL) float64 -> a structured array of n records with the BOUND_COLUMNS names"""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, BOUND_NCOL)
    return t.view([(c, np.float64) for c in BOUND_COLUMNS]).reshape(-1)


def velocity_derivatives(grad):
    """(3, 3, n) gradients of vx, vy, vz (Context.gradients with fields ('vx', 'vy', 'vz')): grad[k, a] = d v_k / d x_a ->
    dict divv = div v, curl = (3, n) curl v, curl_mag = |curl v|.  numpy or torch, as given."""
    g = grad
    divv = (g[0, 0] + g[1, 1]) + g[2, 2]
    cx = g[2, 1] - g[1, 2]
    cy = g[0, 2] - g[2, 0]
    cz = g[1, 0] - g[0, 1]
    if isinstance(g, np.ndarray):
        curl = np.stack([cx, cy, cz])
        mag = np.sqrt((cx * cx + cy * cy) + cz * cz)
    else:
        import torch
        curl = torch.stack([cx, cy, cz])
        mag = torch.sqrt((cx * cx + cy * cy) + cz * cz)
    return {"divv": divv, "curl": curl, "curl_mag": mag}


def profile_desc(r_min, r_max, n_r, n_phi=1, log=False, centre=None, sink=None, normal=(0.0, 0.0, 1.0),
                 z_max=np.inf) -> ProfileDesc:
    """The descriptor of Context.profile's arguments (see there)."""
    d = ProfileDesc()
    d.r_min, d.r_max, d.z_max = float(r_min), float(r_max), float(z_max)
    d.n_r, d.n_phi = int(n_r), int(n_phi)
    d.flags = PROFILE_LOG if log else 0
    if sink is not None:
        if centre is not None:
            raise ValueError("profile: give centre or sink, not both")
        d.sink = int(sink)
    else:
        d.sink = -1
        if centre is not None:
            xyz, vxyz, mass = centre
            d.centre[:] = [float(v) for v in xyz]
            d.centre_v[:] = [float(v) for v in vxyz]
            d.central_mass = float(mass)
    if isinstance(normal, str):
        if normal != "auto":
            raise ValueError("profile: normal must be three numbers or 'auto'")
        d.flags |= PROFILE_AUTO_NORMAL
    else:
        d.normal[:] = [float(v) for v in normal]
    return d


def profile_table(table: np.ndarray) -> np.ndarray:
    """(n_bins, PROFILE_NCOL) float64 -> a structured array of n_bins records with the PROFILE_COLUMNS names"""
    t = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, PROFILE_NCOL)
    return t.view([(c, np.float64) for c in PROFILE_COLUMNS]).reshape(-1)


def profile_finish(desc: ProfileDesc, params: Params, sums) -> np.ndarray:
    """sph_profile_finish: raw sums (n_bins, PROFILE_NSUM) -- e.g. the sums of several contexts or ranks added up -> the
    derived table as a structured array (PROFILE_COLUMNS).  Host code only: no context, no device."""
    s = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1, PROFILE_NSUM)
    out = np.empty((s.shape[0], PROFILE_NCOL))
    st = load().sph_profile_finish(C.byref(desc), C.byref(params), s.ctypes.data, out.ctypes.data, s.shape[0])
    if st != 0:
        raise SphError(st, load().sph_strerror(st).decode() + " -- sph_profile_finish")
    return profile_table(out)


def energy_total(sums) -> dict:
    """sph_energy's sums (ENERGY_NSUM values, e.g. those of several contexts or ranks added up) -> a dict of the named
    sums (ENERGY_SUMS) and the derived totals: E = K + U + W_self + W_gs + K_s + W_ss, P and L (gas + sinks, numpy arrays
    of 3) and com, the centre of mass of gas and sinks (zeros without mass)."""
    s = np.asarray(sums, dtype=np.float64).reshape(ENERGY_NSUM)
    d = {k: float(v) for k, v in zip(ENERGY_SUMS, s)}
    d["E"] = float(s[11] + s[12] + s[13] + s[14] + s[26] + s[27])
    d["P"] = s[5:8] + s[20:23]
    d["L"] = s[8:11] + s[23:26]
    mt = s[1] + s[16]
    d["com"] = (s[2:5] + s[17:20]) / mt if mt > 0 else np.zeros(3)
    return d


class SphError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"summersph status {status}: {text}")
        self.status = status


_lib = None


def load():
    """Loads libsummersph_hip.so (built by __graft_entry__.build() / make -C summersph_amd/csrc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same SONAME,
    # libamdhip64.so.7, as /opt/rocm's).  Importing torch first makes the dynamic loader bind
    # our library to that already-loaded runtime, so torch tensors (device memory, RCCL via
    # torch.distributed) and this library share one set of devices and streams.
    try:
        import torch  # noqa: F401
    except Exception:  # torch absent: the system runtime in /opt/rocm/lib is used
        pass
    lib = C.CDLL(LIB_PATH)
    lib.sph_strerror.restype = C.c_char_p
    lib.sph_last_error.restype = C.c_char_p
    lib.sph_last_error.argtypes = [C.c_void_p]
    lib.sph_count.restype = C.c_int64
    lib.sph_count.argtypes = [C.c_void_p]
    lib.sph_sink_count.restype = C.c_int32
    lib.sph_sink_count.argtypes = [C.c_void_p]
    lib.sph_check_sink_creation.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.sph_get_sink_radii.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sph_sink_candidate_dev.argtypes = [C.c_void_p, C.c_void_p]
    lib.sph_add_sink_checked_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.sph_stream.restype = C.c_void_p
    lib.sph_stream.argtypes = [C.c_void_p]
    lib.sph_ctx_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
    lib.sph_ctx_destroy.argtypes = [C.c_void_p]
    lib.sph_upload.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 9
    lib.sph_upload_dev.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 9
    lib.sph_set_sinks.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    lib.sph_get_sinks.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 10
    for f in ("sph_density", "sph_forces", "sph_synchronize", "sph_timing_reset"):
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.sph_kick.argtypes = [C.c_void_p, C.c_double]
    lib.sph_drift.argtypes = [C.c_void_p, C.c_double]
    lib.sph_next_dt.argtypes = [C.c_void_p, _D]
    lib.sph_step.argtypes = [C.c_void_p, _D, _D]
    lib.sph_run.argtypes = [C.c_void_p, C.c_int32, _D, _D]
    lib.sph_download_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.sph_download_field_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.sph_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    lib.sph_get_bbox.argtypes = [C.c_void_p, _D, _D]
    lib.sph_get_grid_info.argtypes = [C.c_void_p, C.POINTER(GridInfo)]
    lib.sph_upload_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.sph_upload_field_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.sph_update_h.argtypes = [C.c_void_p]
    lib.sph_set_sink_radii.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sph_accrete_and_cull.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.sph_set_owned.argtypes = [C.c_void_p, C.c_int64]
    lib.sph_set_rank.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.sph_scatter_field_dev.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    lib.sph_gather_fields_dev.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_void_p, C.c_void_p]
    lib.sph_scatter_fields_dev.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.c_void_p]
    lib.sph_refresh_eos.argtypes = [C.c_void_p]
    lib.sph_refresh_eos_ghosts.argtypes = [C.c_void_p]
    lib.sph_dt_candidate.argtypes = [C.c_void_p, _D]
    lib.sph_set_sink_accel.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sph_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.sph_reserve.argtypes = [C.c_void_p, C.c_int64]
    lib.sph_owned_bbox.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sph_select_boxes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.sph_selected_ids_dev.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
    lib.sph_replace_ghosts_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.sph_set_dt.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.sph_get_dt.argtypes = [C.c_void_p, _D, _D]
    for f in ("sph_kick_devdt", "sph_drift_devdt", "sph_dt_candidate_dev", "sph_kick_drift_devdt", "sph_kick_dt_candidate_dev",
              "sph_kick_dt_candidate_gas_dev", "sph_kick_sinks_devdt"):
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.sph_pack_partials_dev.argtypes = [C.c_void_p, C.c_void_p]
    lib.sph_pack_partials_ex_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.sph_select_boxes_async.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sph_selected_counts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sph_gather_selected_dev.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sph_apply_partials_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.sph_set_boundary_boxes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.sph_forces_part.argtypes = [C.c_void_p, C.c_int32]
    lib.sph_set_gravity_sources_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.sph_accrete_mark_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.sph_set_numbers_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.sph_accrete_apply_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]
    lib.sph_timing_enable.argtypes = [C.c_void_p, C.c_int]
    lib.sph_timing_stride.argtypes = [C.c_void_p, C.c_int]
    lib.sph_timing_get.argtypes = [C.c_void_p, C.c_int, _D, C.POINTER(C.c_int64)]
    lib.sph_render_density.argtypes = [C.c_void_p, C.POINTER(RenderDesc), C.c_void_p, C.c_int64]
    lib.sph_render_density_dev.argtypes = [C.c_void_p, C.POINTER(RenderDesc), C.c_void_p, C.c_int64]
    lib.sph_render_field.argtypes = [C.c_void_p, C.POINTER(RenderFieldDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sph_render_field_dev.argtypes = [C.c_void_p, C.POINTER(RenderFieldDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sph_profile.argtypes = [C.c_void_p, C.POINTER(ProfileDesc), C.c_void_p, C.c_void_p, C.c_int64]
    lib.sph_profile_dev.argtypes = [C.c_void_p, C.POINTER(ProfileDesc), C.c_void_p, C.c_int64]
    lib.sph_profile_finish.argtypes = [C.POINTER(ProfileDesc), C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_int64]
    lib.sph_energy.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sph_energy_dev.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    for fn in (lib.sph_groups, lib.sph_groups_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(GroupsDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    for fn in (lib.sph_peaks, lib.sph_peaks_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(PeaksDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sph_gradients.argtypes = [C.c_void_p, C.POINTER(GradientsDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    for fn in (lib.sph_sample, lib.sph_sample_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(SampleDesc), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_int64, C.c_void_p, C.c_void_p]
    for fn in (lib.sph_trace, lib.sph_trace_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(TraceDesc), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sph_gradients_dev.argtypes = [C.c_void_p, C.POINTER(GradientsDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p]
    for fn in (lib.sph_gravity_at, lib.sph_gravity_at_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(GravityAtDesc), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_int64, C.c_void_p]
    for fn in (lib.sph_bound, lib.sph_bound_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(BoundDesc), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                       C.c_void_p, C.c_void_p]
    for fn in (lib.sph_cube, lib.sph_cube_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(CubeDesc), C.c_void_p, C.c_void_p, C.c_int64]
    for fn in (lib.sph_transfer, lib.sph_transfer_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(TransferDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    for fn in (lib.sph_force_terms, lib.sph_force_terms_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(ForceTermsDesc), C.c_void_p, C.c_int64]
    for fn in (lib.sph_binned, lib.sph_binned_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(BinnedDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sph_binned_edges.argtypes = [C.POINTER(BinnedDesc), C.c_void_p, C.c_int32, C.c_void_p]
    for fn in (lib.sph_pairs, lib.sph_pairs_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(PairsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                       C.c_void_p]
    lib.sph_pairs_edges.argtypes = [C.POINTER(PairsDesc), C.c_void_p, C.c_void_p]
    lib.sph_pairs_finish.argtypes = [C.POINTER(PairsDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    for fn in (lib.sph_modes, lib.sph_modes_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(ModesDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_void_p]
    lib.sph_modes_tables.argtypes = [C.POINTER(ModesDesc), C.c_void_p, C.c_void_p]
    lib.sph_modes_finish.argtypes = [C.POINTER(ModesDesc), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sph_history_begin.argtypes = [C.c_void_p, C.POINTER(HistoryDesc)]
    lib.sph_history_end.argtypes = [C.c_void_p]
    lib.sph_history_record.argtypes = [C.c_void_p]
    lib.sph_history_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int32)]
    for fn in (lib.sph_history_read, lib.sph_history_read_dev):
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    for fn in (lib.sph_track_begin, lib.sph_track_begin_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(TrackDesc), C.c_int64, C.c_void_p]
    lib.sph_track_end.argtypes = [C.c_void_p]
    lib.sph_track_record.argtypes = [C.c_void_p]
    lib.sph_track_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 5 + [C.POINTER(C.c_int32)]
    for fn in (lib.sph_track_read, lib.sph_track_read_dev):
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    for fn in (lib.sph_track_fates, lib.sph_track_fates_dev):
        fn.argtypes = [C.c_void_p, C.c_void_p]
    for fn in (lib.sph_dust_begin, lib.sph_dust_begin_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(DustDesc), C.c_int64] + [C.c_void_p] * 7
    lib.sph_dust_end.argtypes = [C.c_void_p]
    lib.sph_dust_advance.argtypes = [C.c_void_p]
    lib.sph_dust_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 5
    for fn in (lib.sph_dust_read, lib.sph_dust_read_dev):
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    for fn in (lib.sph_dust_state, lib.sph_dust_state_dev):
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 7
    for fn in (lib.sph_dust_fates, lib.sph_dust_fates_dev):
        fn.argtypes = [C.c_void_p, C.c_void_p]
    lib.sph_frames_begin.argtypes = [C.c_void_p, C.POINTER(FramesDesc)]
    for fn in (lib.sph_frames_end, lib.sph_frames_record, lib.sph_frames_rewind):
        fn.argtypes = [C.c_void_p]
    lib.sph_frames_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
    for fn in (lib.sph_frames_read, lib.sph_frames_read_dev):
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    for fn in (lib.sph_frame, lib.sph_frame_dev):
        fn.argtypes = [C.c_void_p, C.POINTER(FramesDesc), C.c_void_p, C.c_void_p, C.c_int64]
    _lib = lib
    return lib


def default_params(variable: bool = False) -> Params:
    p = Params()
    if variable:
        load().sph_params_default_variable(C.byref(p))
    else:
        load().sph_params_default(C.byref(p))
    return p


def _hp(a):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


# ---- the marshalling of the analysis calls -----------------------------------------------------------------------------
# Every analysis call has a host form (numpy in and out, sph_X) and a device form (torch tensors on the context's GPU,
# sph_X_dev) with the same argument list.  A Context method is written once against a form object: it allocates the
# outputs, turns arrays into pointer arguments, holds the int64 counts and runs the call.
def _on_gpu(t, device: int, dtype=np.float64) -> bool:
    """t is a torch tensor of the dtype on GPU `device`"""
    import torch
    return isinstance(t, torch.Tensor) and t.dtype == getattr(torch, np.dtype(dtype).name) and t.device == torch.device("cuda", device)


class _HostForm:
    device = False

    def __init__(self, ctx):
        self.ctx = ctx

    def empty(self, shape, dtype=np.float64):
        return np.empty(shape, dtype=dtype)

    @staticmethod
    def ptr(a):
        return None if a is None else a.ctypes.data

    @staticmethod
    def counts(k: int):
        return np.zeros(k, dtype=np.int64)

    @staticmethod
    def host(a):
        return a

    def read(self, cnt) -> tuple:
        return tuple(int(v) for v in self.host(cnt))

    def call(self, name: str, *args):
        self.ctx._ck(getattr(self.ctx.lib, name)(self.ctx._h, *args))


class _DeviceForm(_HostForm):
    device = True

    def __init__(self, ctx):
        import torch
        self.ctx, self.torch, self.dev = ctx, torch, torch.device("cuda", ctx.device)

    def owns(self, t, dtype=np.float64) -> bool:
        return _on_gpu(t, self.ctx.device, dtype)

    def empty(self, shape, dtype=np.float64):
        return self.torch.empty(shape, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.dev)

    @staticmethod
    def ptr(a):
        return None if a is None else C.c_void_p(a.data_ptr())

    def counts(self, k: int):
        return self.empty(k, np.int64)

    @staticmethod
    def host(a):
        return a.cpu().numpy()

    def call(self, name: str, *args):
        """sph_X_dev ordered against torch: the call runs on the context's stream, not torch's"""
        cuda, ctx = self.torch.cuda, self.ctx
        cuda.current_stream(self.dev).synchronize()               # the blocks may still be in use by torch's queued work
        ctx._ck(getattr(ctx.lib, name + "_dev")(ctx._h, *args))
        st = ctx.stream()                                         # torch's later work on the outputs waits for the call
        if st:
            cuda.current_stream(self.dev).wait_stream(cuda.ExternalStream(st, device=self.dev))
        else:
            cuda.synchronize(self.dev)


def _points(who, points, form, extra=None, noun="point"):
    """The rule "points as an (M, 3) array or three arrays of M": ([x, y, z, *extra], M).  extra: the optional per-point
    arrays by name (an absent one stays None).  The host form converts to contiguous float64 numpy; the device form takes
    contiguous float64 tensors on the context's GPU as they are (an (M, 3) tensor is split into three)."""
    three = isinstance(points, (tuple, list)) and len(points) == 3
    more = list((extra or {}).items())
    if form.device:
        if three:
            p = list(points)
        elif form.owns(points) and points.ndim == 2 and points.shape[1] == 3:
            p = [points[:, a].contiguous() for a in range(3)]
        else:
            p = [None]
        given = p + [t for _, t in more if t is not None]
        if not all(form.owns(t) and t.ndim == 1 and t.is_contiguous() and t.numel() == p[0].numel() for t in given):
            what = f"(and {', '.join(extra)}) must be" if extra else "must be an (M, 3) or three"
            raise ValueError(f"{who}: device {noun}s {what} contiguous float64 tensors on the context's GPU")
        return p + [t for _, t in more], p[0].numel()
    if three:
        p = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in points]
    else:
        a = np.asarray(points, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{who}: {noun}s must be an (M, 3) array or three arrays")
        p = [np.ascontiguousarray(a[:, k]) for k in range(3)]
    m = p[0].size
    if p[1].size != m or p[2].size != m:
        raise ValueError(f"{who}: the three {noun} arrays differ in length")
    for name, t in more:
        if t is not None:
            t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
            if t.size != m:
                raise ValueError(f"{who}: {name} has {t.size} values for {m} points")
        p.append(t)
    return p, m


def _values_rows(who, values, rows, n, form, exact=False):
    """The multi-row rule: values is None or an (n_rows, n) array in the upload order of which the call reads `rows` rows.
    The host form takes 1-D input as one row and zero-pads the rows nothing reads (row k belongs to field k); the device
    form takes a contiguous float64 tensor on the context's GPU of at least (exact: exactly) rows * n values."""
    if values is None:
        return None
    if form.device:
        if not (form.owns(values) and values.is_contiguous()):
            raise ValueError(f"{who}: device values must be a contiguous float64 tensor on the context's GPU")
        if exact and values.numel() != rows * n:
            raise ValueError(f"{who}: values rows of {values.numel() // max(rows, 1)} for {n} particles")
        if values.numel() < rows * n:
            raise ValueError(f"{who}: values need {rows} rows of {n}")
        return values
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim != 2:
        v = v.reshape(1, -1)
    if v.shape[1] != n:
        raise ValueError(f"{who}: values rows of {v.shape[1]} for {n} particles")
    if v.shape[0] < rows:
        v = np.concatenate([v, np.zeros((rows - v.shape[0], n))])
    return v


def _values_one(who, values, n, form):
    """The single-row rule: n values in the upload order, float64 numpy (host form) or a contiguous float64 tensor on the
    context's GPU (device form)."""
    if form.device:
        if not (form.owns(values) and values.is_contiguous() and values.numel() == n):
            raise ValueError(f"{who}: device values must be a contiguous float64 tensor of sph_count() on the context's GPU")
        return values
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    if v.size != n:
        raise ValueError(f"{who}: {v.size} values for {n} particles")
    return v


class Context:
    """Thin object wrapper over an sph_ctx*.  Arrays are float64 numpy (host) unless a method says _dev."""

    def __init__(self, params: Params | None = None, device: int = 0, variable: bool = False, **overrides):
        self.lib = load()
        p = params if params is not None else default_params(variable)
        for k, v in overrides.items():
            setattr(p, k, v)
        self.params = p
        self.device = int(device)
        h = C.c_void_p()
        st = self.lib.sph_ctx_create(C.byref(p), int(device), C.byref(h))
        if st != 0:
            raise SphError(st, self.lib.sph_strerror(st).decode())
        self._h = h

    def _ck(self, st):
        if st != 0:
            raise SphError(st, self.lib.sph_strerror(st).decode() + " -- " + self.lib.sph_last_error(self._h).decode())

    def _form(self, device):
        """the host or device form of an analysis call"""
        return _DeviceForm(self) if device else _HostForm(self)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.sph_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state -------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return int(self.lib.sph_count(self._h))

    def upload(self, gas: dict):
        arrs = [np.ascontiguousarray(gas[k], dtype=np.float64) for k in "x y z vx vy vz u m".split()]
        al = gas.get("alpha")
        al = None if al is None else np.ascontiguousarray(al, dtype=np.float64)
        self._ck(self.lib.sph_upload(self._h, arrs[0].size, *[_hp(a) for a in arrs], _hp(al)))
        if gas.get("h") is not None and (self.params.flags & FLAG_VARIABLE_H):
            self.upload_field("h", gas["h"])

    def upload_field(self, name: str, values):
        a = np.ascontiguousarray(values, dtype=np.float64)
        self._ck(self.lib.sph_upload_field(self._h, FIELDS.index(name), _hp(a), a.size))

    def upload_field_dev(self, name: str, dev_ptr: int, n: int):
        self._ck(self.lib.sph_upload_field_dev(self._h, FIELDS.index(name), C.c_void_p(int(dev_ptr)), int(n)))

    def update_h(self):
        self._ck(self.lib.sph_update_h(self._h))

    def upload_dev(self, n: int, ptrs):
        """ptrs: 9 device addresses (ints; alpha may be 0/None), e.g. torch tensors' data_ptr()"""
        self._ck(self.lib.sph_upload_dev(self._h, int(n), *[C.c_void_p(int(p) if p else 0) for p in ptrs]))

    def set_sinks(self, sinks: dict):
        arrs = [np.ascontiguousarray(sinks[k], dtype=np.float64) for k in "x y z vx vy vz m".split()]
        self._ck(self.lib.sph_set_sinks(self._h, arrs[0].size, *[_hp(a) for a in arrs]))
        self.ns = int(arrs[0].size)
        if sinks.get("radius") is not None:
            r = np.ascontiguousarray(sinks["radius"], dtype=np.float64)
            self._ck(self.lib.sph_set_sink_radii(self._h, r.size, _hp(r)))

    def accrete_and_cull(self) -> int:
        r = C.c_int64(0)
        self._ck(self.lib.sph_accrete_and_cull(self._h, C.byref(r)))
        return int(r.value)

    def get_sinks(self) -> dict:
        ns = self.ns = int(self.lib.sph_sink_count(self._h))      # check_sink_creation may have added one
        out = {k: np.zeros(ns) for k in "x y z vx vy vz m ax ay az".split()}
        self._ck(self.lib.sph_get_sinks(self._h, ns, *[_hp(out[k]) for k in "x y z vx vy vz m ax ay az".split()]))
        out["radius"] = np.zeros(ns)
        self._ck(self.lib.sph_get_sink_radii(self._h, ns, _hp(out["radius"])))
        return out

    def sink_candidate_dev(self, dev_ptr: int):
        self._ck(self.lib.sph_sink_candidate_dev(self._h, C.c_void_p(int(dev_ptr))))

    def add_sink_checked_dev(self, dev_ptr: int) -> bool:
        cr = C.c_int32(0)
        self._ck(self.lib.sph_add_sink_checked_dev(self._h, C.c_void_p(int(dev_ptr)), C.byref(cr)))
        return bool(cr.value)

    def check_sink_creation(self) -> bool:
        cr = C.c_int32(0)
        self._ck(self.lib.sph_check_sink_creation(self._h, C.byref(cr)))
        return bool(cr.value)

    # ---- hot path ------------------------------------------------------------------------
    def density(self):
        """density, forces, step and run raise SphError (SPH_ERR_STATE) after a fixed-h list overflow was reported, until the
        next upload (include/summersph.h, SPH_ERR_STATE)"""
        self._ck(self.lib.sph_density(self._h))

    def forces(self):
        self._ck(self.lib.sph_forces(self._h))

    def kick(self, dt: float):
        self._ck(self.lib.sph_kick(self._h, float(dt)))

    def drift(self, dt: float):
        self._ck(self.lib.sph_drift(self._h, float(dt)))

    def next_dt(self, dt: float) -> float:
        d = C.c_double(dt)
        self._ck(self.lib.sph_next_dt(self._h, C.byref(d)))
        return d.value

    def step(self, dt: float, t: float = 0.0):
        d, tt = C.c_double(dt), C.c_double(t)
        self._ck(self.lib.sph_step(self._h, C.byref(d), C.byref(tt)))
        return d.value, tt.value

    def run(self, nsteps: int, dt: float, t: float = 0.0):
        d, tt = C.c_double(dt), C.c_double(t)
        self._ck(self.lib.sph_run(self._h, int(nsteps), C.byref(d), C.byref(tt)))
        return d.value, tt.value

    # ---- multi-GPU building blocks ---------------------------------------------------------
    def set_owned(self, n_owned: int):
        self._ck(self.lib.sph_set_owned(self._h, int(n_owned)))

    def set_rank(self, rank: int, nranks: int):
        self._ck(self.lib.sph_set_rank(self._h, int(rank), int(nranks)))

    def scatter_field_dev(self, name: str, first: int, count: int, dev_ptr: int):
        self._ck(self.lib.sph_scatter_field_dev(self._h, FIELDS.index(name), int(first), int(count), C.c_void_p(int(dev_ptr))))

    def gather_fields_dev(self, names, count: int, ids_ptr: int, out_ptr: int):
        """out[f, k] = field names[f] of original id ids[k] (ids_ptr 0: ids 0..count-1); device pointers"""
        f = (C.c_int32 * len(names))(*[FIELDS.index(n) for n in names])
        self._ck(self.lib.sph_gather_fields_dev(self._h, len(names), f, int(count), C.c_void_p(int(ids_ptr) or None),
                                                C.c_void_p(int(out_ptr))))

    def scatter_fields_dev(self, names, first: int, count: int, vals_ptr: int):
        f = (C.c_int32 * len(names))(*[FIELDS.index(n) for n in names])
        self._ck(self.lib.sph_scatter_fields_dev(self._h, len(names), f, int(first), int(count), C.c_void_p(int(vals_ptr))))

    # ---- the device-resident multi-GPU exchange (include/summersph.h, "kept on the device") ----
    def set_stream(self, stream_handle: int):
        self._ck(self.lib.sph_set_stream(self._h, C.c_void_p(stream_handle)))

    def reserve(self, n_slots: int):
        self._ck(self.lib.sph_reserve(self._h, n_slots))

    def owned_bbox(self, dev_ptr: int = 0) -> np.ndarray | None:
        """dev_ptr == 0: returns min xyz, max xyz on the host; else writes them to device memory (no sync)"""
        if dev_ptr:
            self._ck(self.lib.sph_owned_bbox(self._h, None, C.c_void_p(dev_ptr)))
            return None
        out = np.empty(6)
        self._ck(self.lib.sph_owned_bbox(self._h, out.ctypes.data, None))
        return out

    def select_boxes(self, boxes: np.ndarray) -> np.ndarray:
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
        counts = np.zeros(boxes.shape[0], dtype=np.int64)
        self._ck(self.lib.sph_select_boxes(self._h, boxes.shape[0], boxes.ctypes.data, counts.ctypes.data))
        return counts

    def select_boxes_async(self, boxes: np.ndarray):
        """the same selection without waiting for its counts (read them with selected_counts after a synchronisation)"""
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
        self._ck(self.lib.sph_select_boxes_async(self._h, boxes.shape[0], boxes.ctypes.data))
        return boxes.shape[0]

    def selected_counts(self, nbox: int) -> np.ndarray:
        counts = np.zeros(nbox, dtype=np.int64)
        self._ck(self.lib.sph_selected_counts(self._h, int(nbox), counts.ctypes.data))
        return counts

    def gather_selected_dev(self, box: int, names, capacity: int, out_ptr: int):
        """out[0] = count, out[1] = 0, out[2 + f*count + k] (if count <= capacity) for selection `box`; device pointer"""
        f = (C.c_int32 * len(names))(*[FIELDS.index(n) for n in names])
        self._ck(self.lib.sph_gather_selected_dev(self._h, int(box), len(names), f, int(capacity), C.c_void_p(int(out_ptr))))

    def selected_ids_dev(self, box: int, count: int, dev_ptr: int):
        self._ck(self.lib.sph_selected_ids_dev(self._h, box, count, C.c_void_p(dev_ptr)))

    def replace_ghosts_dev(self, count: int, dev_ptr: int):
        self._ck(self.lib.sph_replace_ghosts_dev(self._h, count, C.c_void_p(dev_ptr)))

    def set_dt(self, dt: float, t: float = 0.0):
        self._ck(self.lib.sph_set_dt(self._h, dt, t))

    def get_dt(self):
        dt, t = C.c_double(0.0), C.c_double(0.0)
        self._ck(self.lib.sph_get_dt(self._h, C.byref(dt), C.byref(t)))
        return dt.value, t.value

    def kick_devdt(self):
        self._ck(self.lib.sph_kick_devdt(self._h))

    def drift_devdt(self):
        self._ck(self.lib.sph_drift_devdt(self._h))

    def dt_candidate_dev(self):
        self._ck(self.lib.sph_dt_candidate_dev(self._h))

    def kick_drift_devdt(self):
        self._ck(self.lib.sph_kick_drift_devdt(self._h))

    def kick_dt_candidate_dev(self):
        self._ck(self.lib.sph_kick_dt_candidate_dev(self._h))

    def kick_dt_candidate_gas_dev(self):
        self._ck(self.lib.sph_kick_dt_candidate_gas_dev(self._h))

    def kick_sinks_devdt(self):
        self._ck(self.lib.sph_kick_sinks_devdt(self._h))

    def pack_partials_dev(self, dev_ptr: int, predict_box: bool = True):
        self._ck(self.lib.sph_pack_partials_ex_dev(self._h, C.c_void_p(dev_ptr), 1 if predict_box else 0))

    def apply_partials_dev(self, dev_ptr: int, nranks: int, stride: int, apply_dt: bool):
        self._ck(self.lib.sph_apply_partials_dev(self._h, C.c_void_p(dev_ptr), nranks, stride, 1 if apply_dt else 0))

    def set_boundary_boxes(self, boxes: np.ndarray):
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
        self._ck(self.lib.sph_set_boundary_boxes(self._h, boxes.shape[0], boxes.ctypes.data if boxes.size else None))

    def forces_part(self, part: int):
        """1: sink gravity + the wavefronts that cannot see a ghost; 2: the others (after refresh_eos)"""
        self._ck(self.lib.sph_forces_part(self._h, part))

    def set_gravity_sources_dev(self, n_src: int, dev_ptr: int, lo_hi):
        """n_src records {x,y,z,m} at dev_ptr (kept alive by the caller) + their bounding box; n_src = 0 resets"""
        box = np.ascontiguousarray(lo_hi, dtype=np.float64) if n_src else np.zeros(6)
        self._ck(self.lib.sph_set_gravity_sources_dev(self._h, int(n_src), C.c_void_p(int(dev_ptr)) if n_src else None,
                                                      box.ctypes.data))

    def set_numbers_dev(self, first: int, count: int, dev_ptr: int):
        """global particle numbers (int64 on the device) of original ids [first, first + count)"""
        self._ck(self.lib.sph_set_numbers_dev(self._h, int(first), int(count), C.c_void_p(int(dev_ptr)) if count else None))

    def accrete_mark_dev(self, src_offset: int, partials_ptr: int):
        self._ck(self.lib.sph_accrete_mark_dev(self._h, int(src_offset), C.c_void_p(int(partials_ptr))))

    def accrete_apply_dev(self, all_ptr: int, nranks: int, stride: int, keep_ptr: int = 0) -> int:
        r = C.c_int64(0)
        self._ck(self.lib.sph_accrete_apply_dev(self._h, C.c_void_p(int(all_ptr)), nranks, stride,
                                                C.c_void_p(int(keep_ptr)) if keep_ptr else None, C.byref(r)))
        return int(r.value)

    def refresh_eos(self, ghosts_only: bool = False):
        self._ck((self.lib.sph_refresh_eos_ghosts if ghosts_only else self.lib.sph_refresh_eos)(self._h))

    def dt_candidate(self) -> float:
        d = C.c_double(0)
        self._ck(self.lib.sph_dt_candidate(self._h, C.byref(d)))
        return d.value

    def set_sink_accel(self, ax, ay, az):
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (ax, ay, az)]
        self._ck(self.lib.sph_set_sink_accel(self._h, a[0].size, *[_hp(v) for v in a]))

    # ---- read-back -----------------------------------------------------------------------
    def field(self, name: str) -> np.ndarray:
        out = np.zeros(self.n)
        self._ck(self.lib.sph_download_field(self._h, FIELDS.index(name), _hp(out), out.size))
        return out

    def field_dev(self, name: str, dev_ptr: int, n: int):
        self._ck(self.lib.sph_download_field_dev(self._h, FIELDS.index(name), C.c_void_p(int(dev_ptr)), int(n)))

    def state(self) -> dict:
        return {k: self.field(k) for k in FIELDS[:9]}

    # ---- density rendering (sph_render_density) --------------------------------------------------
    def render_desc(self, shape, bounds=None, axis=None, h=None, clip=None, spacing=False) -> RenderDesc:
        """The descriptor of render_density's arguments (see there)."""
        n = (int(shape),) * 3 if np.isscalar(shape) else tuple(int(v) for v in shape)
        if len(n) != 3:
            raise ValueError("shape: one node count or three")
        d = RenderDesc()
        d.n[:] = n
        d.axis = -1 if axis is None else ("xyz".index(axis) if isinstance(axis, str) else int(axis))
        d.h = 0.0 if h is None else float(h)
        d.flags = (RENDER_AUTO_BOUNDS if bounds is None else 0) | (RENDER_SPACING if spacing else 0)
        if bounds is not None:
            b = np.asarray(bounds, dtype=np.float64).reshape(2, 3)
            d.lo[:] = b[0].tolist(); d.hi[:] = b[1].tolist()
        cb = np.array([[-np.inf] * 3, [np.inf] * 3]) if clip is None else np.asarray(clip, dtype=np.float64).reshape(2, 3)
        d.clip_lo[:] = cb[0].tolist(); d.clip_hi[:] = cb[1].tolist()
        return d

    @staticmethod
    def render_shape(d: RenderDesc):
        n = tuple(d.n)
        return n if d.axis < 0 else tuple(v for a, v in enumerate(n) if a != d.axis)

    def render_density(self, shape, bounds=None, axis=None, h=None, clip=None, spacing=False, device=False):
        """SPH density m W(|g - r_j|, h_j) summed on an np.linspace node grid (include/summersph.h, sph_render_density).
        shape: nodes per axis (n or (n0, n1, n2)); bounds: ((lo xyz), (hi xyz)) or None = the selected particles' min / max;
        axis: None = the 3-D grid (x slowest), 0 / 1 / 2 or 'x' / 'y' / 'z' = column sums along it; h: None = each particle's
        own h, else one h for all; clip: ((lo xyz), (hi xyz)), strict; spacing: column sums times the node spacing.
        Returns float64 numpy (device=False) or a torch tensor on the context's GPU; the node box used is left in
        self.render_bounds."""
        d = self.render_desc(shape, bounds, axis, h, clip, spacing)
        oshape = self.render_shape(d)
        f = self._form(device)
        out = f.empty(oshape)
        f.call("sph_render_density", C.byref(d), f.ptr(out), int(np.prod(oshape, dtype=np.int64)))
        self.render_bounds = (np.array(d.lo[:]), np.array(d.hi[:]))
        return out

    def render_field_desc(self, field, shape, bounds=None, axis=None, h=None, clip=None, spacing=False, weight="mass",
                          normalise=False) -> RenderFieldDesc:
        """The descriptor of render_field's arguments (field: an SPH_F_* name or id, or RENDER_FIELD_VALUES)."""
        d = RenderFieldDesc()
        d.base = self.render_desc(shape, bounds, axis, h, clip, spacing)
        d.field = FIELDS.index(field) if isinstance(field, str) else int(field)
        d.weight = {"mass": RENDER_WEIGHT_MASS, "volume": RENDER_WEIGHT_VOLUME}[weight] if isinstance(weight, str) else int(weight)
        d.normalise = int(normalise)
        return d

    def render_field(self, field, shape, bounds=None, axis=None, h=None, clip=None, spacing=False, weight="mass",
                     normalise=False, weight_out=False, device=False):
        """Any per-particle quantity A on render_density's nodes (include/summersph.h, sph_render_field): with
        ws = w_j / (pi h_j^3), w_j = m_j (weight='mass') or m_j / rho_j ('volume'), num = sum ws A Wn and den = sum ws Wn.
        Returns num (column sums times the spacing with spacing=True) or, normalise=True, num / den (0 where den is 0); with
        weight_out=True, (image, den) (the column den times the spacing).  field: an SPH_F_* name ('u', 'vz', 'rho', ...)
        read from the context, or sph_count() values in the upload order -- a float64 numpy array (host form, device must
        be False) or a contiguous float64 torch tensor on the context's GPU (device form, device must be True).  The
        other arguments and self.render_bounds are render_density's."""
        f = self._form(device)
        values = None
        if not isinstance(field, str):                            # the values' kind must be the form's
            if isinstance(field, np.ndarray):
                if device:
                    raise ValueError("render_field: a numpy values array renders with device=False")
            elif not (_on_gpu(field, self.device) and field.is_contiguous()):
                raise ValueError("render_field: values must be float64 numpy or a contiguous float64 tensor on the context's GPU")
            elif not device:
                raise ValueError("render_field: a device values tensor renders with device=True")
            elif field.numel() != self.n:
                raise ValueError(f"render_field: {field.numel()} values for {self.n} particles")
            values, field = _values_one("render_field", field, self.n, f), RENDER_FIELD_VALUES
        d = self.render_field_desc(field, shape, bounds, axis, h, clip, spacing, weight, normalise)
        oshape = self.render_shape(d.base)
        out = f.empty(oshape)
        wout = f.empty(oshape) if weight_out else None
        f.call("sph_render_field", C.byref(d), f.ptr(values), f.ptr(out), f.ptr(wout), int(np.prod(oshape, dtype=np.int64)))
        self.render_bounds = (np.array(d.base.lo[:]), np.array(d.base.hi[:]))
        return (out, wout) if weight_out else out

    # ---- disc profiles (sph_profile) -----------------------------------------------------------
    def profile(self, r_min, r_max, n_r, n_phi=1, log=False, centre=None, sink=None, normal=(0.0, 0.0, 1.0), z_max=np.inf,
                sums_only=False, device=False):
        """Mass-weighted moments of the owned gas in rings (n_phi > 1: ring sectors) about a centre (include/summersph.h,
        sph_profile).  centre: None (the origin at rest, no eccentricity) or (xyz, vxyz, central mass); sink=k: sink k's
        position, velocity and mass instead; normal: three numbers or 'auto' (the shell's total angular momentum);
        z_max: strict |z'| cut; log: logarithmic ring edges.  Bin b = ring * n_phi + sector.
        Returns (table, sums): table a structured array of n_bins records (PROFILE_COLUMNS), sums (n_bins, PROFILE_NSUM)
        float64; sums_only=True: (None, sums).  device=True: the sums only, as a torch tensor on the context's GPU.  The
        descriptor used (normal written back) is left in self.profile_desc."""
        d = profile_desc(r_min, r_max, n_r, n_phi, log, centre, sink, normal, z_max)
        nb = int(n_r) * int(n_phi)
        f = self._form(device)
        sums = f.empty((nb, PROFILE_NSUM))
        if device:                                                # sph_profile_dev takes no table
            f.call("sph_profile", C.byref(d), f.ptr(sums), nb)
        else:
            table = None if sums_only else f.empty((nb, PROFILE_NCOL))
            f.call("sph_profile", C.byref(d), f.ptr(sums), f.ptr(table), nb)
        self.profile_desc = d
        return sums if device else ((None if table is None else profile_table(table)), sums)

    # ---- conserved totals and the potential (sph_energy) ---------------------------------------
    def energy(self, phi=False, device=False, src_offset=0):
        """Energy, momentum and angular momentum of the owned gas and the sinks, with the gravitational potential
        (include/summersph.h, sph_energy).  Returns energy_total(sums) (the named sums, E, P, L, com) plus "sums", the raw
        ENERGY_NSUM values (they add over contexts and ranks).  phi=True: also "phi", Phi_self + Phi_sink of every particle
        in the upload order (sph_count values, 0 for ghosts).  device=True: "sums" and "phi" are torch tensors on the
        context's GPU (sph_energy_dev); the named values are read from them.  src_offset: the position of this context's
        owned particles in the external source set (sph_set_gravity_sources_dev), ignored without one."""
        n = self.n
        f = self._form(device)
        sums = f.empty(ENERGY_NSUM)
        ph = f.empty(n) if phi else None
        f.call("sph_energy", int(src_offset), f.ptr(sums), f.ptr(ph), n)
        out = energy_total(f.host(sums))
        out["sums"] = sums
        if phi:
            out["phi"] = ph
        return out

    # ---- the per-step time series (sph_history) ---------------------------------------------------
    def history_begin(self, capacity, every=1, max_sinks=None):
        """Starts (or restarts) the device-resident log of one row per every-th step of step / run (include/summersph.h,
        sph_history): capacity rows, the per-sink columns of max_sinks sinks (None: the current sink count)."""
        ms = int(self.lib.sph_sink_count(self._h)) if max_sinks is None else max_sinks
        d = history_desc(capacity, every, ms)
        self._ck(self.lib.sph_history_begin(self._h, C.byref(d)))
        self.history_desc = d

    def history_record(self):
        """Appends a row for the state as it is now (the step number is not advanced)."""
        self._ck(self.lib.sph_history_record(self._h))

    def history_end(self):
        self._ck(self.lib.sph_history_end(self._h))

    def history_info(self) -> dict:
        """rows held, rows dropped, steps counted since history_begin and the row width"""
        r, d, s, w = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._ck(self.lib.sph_history_info(self._h, C.byref(r), C.byref(d), C.byref(s), C.byref(w)))
        return {"rows": r.value, "dropped": d.value, "steps": s.value, "width": w.value}

    def history(self, first=0, count=None, device=False):
        """Rows [first, first + count) of the log (count None: all from first) as history_columns' dict of named columns.
        device=True: the rows are copied on the context's GPU in the stream's order (sph_history_read_dev) and "rows" is
        that torch tensor; the named columns are read from it."""
        info = self.history_info()
        first = int(first)
        cnt = info["rows"] - first if count is None else int(count)
        f = self._form(device)
        rows = f.empty((max(cnt, 0), info["width"]))
        f.call("sph_history_read", first, cnt, f.ptr(rows))
        out = history_columns(f.host(rows), info["dropped"])
        out["rows"] = rows
        return out

    # ---- trajectories and fates of chosen particles (sph_track) ------------------------------------
    def track_begin(self, ids, capacity, every=1):
        """Starts (or restarts) the device-resident log of the particles that are ids[k] in today's caller order
        (include/summersph.h, sph_track): one row per every-th step of step / run, capacity rows.  ids: integers (numpy, a
        list) or an int64 torch tensor on the context's GPU (sph_track_begin_dev)."""
        d = track_desc(capacity, every)
        if _on_gpu(ids, self.device, np.int64):
            f = self._form(True)
            if ids.dim() != 1 or ids.numel() < 1:
                raise ValueError("track: ids must be a 1-D tensor of at least one id")
            ids = ids.contiguous()
            f.call("sph_track_begin", C.byref(d), ids.numel(), f.ptr(ids))
        else:
            a = track_ids(ids)
            self._ck(self.lib.sph_track_begin(self._h, C.byref(d), a.size, a.ctypes.data))
        self.track_desc = d

    def track_record(self):
        """Appends a row for the state as it is now (the step number is not advanced)."""
        self._ck(self.lib.sph_track_record(self._h))

    def track_end(self):
        self._ck(self.lib.sph_track_end(self._h))

    def track_info(self, live=True) -> dict:
        """rows held, rows dropped, steps counted since track_begin, the tracked particles, whether the tracker is closed and
        (live=True: one read-back, waits for the stream) how many of them are still alive"""
        v = [C.c_int64(0) for _ in range(5)]
        closed = C.c_int32(0)
        self._ck(self.lib.sph_track_info(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]),
                                         C.byref(v[4]) if live else None, C.byref(closed)))
        out = {"rows": v[0].value, "dropped": v[1].value, "steps": v[2].value, "n_tracked": v[3].value, "closed": bool(closed.value)}
        if live:
            out["n_live"] = v[4].value
        return out

    def track(self, first=0, count=None, device=False):
        """Rows [first, first + count) of the log (count None: all from first) as track_columns' dict: step, t, n, n_live
        per row, one (rows, K) array per name of TRACK_COLUMNS (column k is the particle that was ids[k] at track_begin;
        NaN once it is gone) and body (rows, 10, K).  device=True: the rows are copied on the context's GPU in the stream's
        order (sph_track_read_dev); body, head and the named columns are torch tensors, the head's columns are read from it."""
        info = self.track_info(live=False)
        first = int(first)
        cnt = info["rows"] - first if count is None else int(count)
        f = self._form(device)
        head = f.empty((max(cnt, 0), TRACK_NHEAD))
        body = f.empty((max(cnt, 0), TRACK_NCOL, info["n_tracked"]))
        f.call("sph_track_read", first, cnt, f.ptr(head), f.ptr(body))
        if not device:
            return track_columns(head, body, info["dropped"])
        out = track_columns(f.host(head), np.empty((head.shape[0], TRACK_NCOL, 0)), info["dropped"])
        for i, k in enumerate(TRACK_COLUMNS):
            out[k] = body[:, i, :]
        out["body"], out["head"] = body, head
        return out

    def track_fates(self, device=False) -> dict:
        """The fates of the tracked particles: {"fate", "step", "sink", "current_id"}, four (K,) int32 arrays (torch tensors
        with device=True).  fate: TRACK_ALIVE, TRACK_ACCRETED, TRACK_CULLED."""
        k = self.track_info(live=False)["n_tracked"]
        f = self._form(device)
        fates = f.empty((k, len(TRACK_FATES)), np.int32)
        f.call("sph_track_fates", f.ptr(fates))
        if not device:
            return track_fates_columns(fates)
        return {name: fates[:, i] for i, name in enumerate(TRACK_FATES)}

    # ---- drag-coupled tracer grains (sph_dust) -------------------------------------------------------
    def dust_begin(self, x, v, par, law="epstein", rho_grain=None, capacity=0, every=1, record_every=1, remove=False):
        """Starts (or restarts) M tracer grains (include/summersph.h, sph_dust) at positions x and velocities v, each an
        (M, 3) array or three arrays of M, with the drag parameter par (M values: the grain size under law="epstein" with
        rho_grain in code units, the stopping time under law="fixed_ts").  Every every-th step of step / run advances them,
        every record_every-th advance appends a row to a log of capacity rows; remove=True lets sinks accrete them and the
        bound cull them.  numpy arrays, or float64 torch tensors on the context's GPU (sph_dust_begin_dev)."""
        d = dust_desc(law, rho_grain, capacity, every, record_every, remove)
        device = any(_on_gpu(t, self.device) for t in (*(x if isinstance(x, (tuple, list)) else (x,)), par))
        f = self._form(device)
        p, m = _points("dust", x, f, noun="grain")
        q, mv = _points("dust", v, f, {"par": par}, noun="grain")
        if mv != m or q[3] is None:
            raise ValueError(f"dust: {m} positions, {mv} velocities; par must be given")
        f.call("sph_dust_begin", C.byref(d), m, *(f.ptr(a) for a in p), *(f.ptr(a) for a in q))
        self.dust_desc = d

    def dust_advance(self):
        """Advances the grains to the clock now, outside a step, and appends a row (the first call after dust_begin is the
        t = 0 row)."""
        self._ck(self.lib.sph_dust_advance(self._h))

    def dust_end(self):
        self._ck(self.lib.sph_dust_end(self._h))

    def dust_info(self, live=True) -> dict:
        """rows held, rows dropped, advances counted since dust_begin, the grains and (live=True: one read-back, waits for
        the stream) how many of them are still alive"""
        v = [C.c_int64(0) for _ in range(5)]
        self._ck(self.lib.sph_dust_info(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]),
                                        C.byref(v[4]) if live else None))
        out = {"rows": v[0].value, "dropped": v[1].value, "advances": v[2].value, "n_grains": v[3].value}
        if live:
            out["n_live"] = v[4].value
        return out

    def dust(self, first=0, count=None, device=False):
        """Rows [first, first + count) of the grains' log (count None: all from first) as dust_columns' dict: advance, t,
        delta, n_live per row, one (rows, M) array per name of DUST_COLUMNS (NaN once a grain has a fate) and body
        (rows, 12, M).  device=True: the rows are copied on the context's GPU in the stream's order (sph_dust_read_dev);
        body, head and the named columns are torch tensors, the head's columns are read from it."""
        info = self.dust_info(live=False)
        first = int(first)
        cnt = info["rows"] - first if count is None else int(count)
        f = self._form(device)
        head = f.empty((max(cnt, 0), DUST_NHEAD))
        body = f.empty((max(cnt, 0), DUST_NCOL, info["n_grains"]))
        f.call("sph_dust_read", first, cnt, f.ptr(head), f.ptr(body))
        if not device:
            return dust_columns(head, body, info["dropped"])
        out = dust_columns(f.host(head), np.empty((head.shape[0], DUST_NCOL, 0)), info["dropped"])
        for i, k in enumerate(DUST_COLUMNS):
            out[k] = body[:, i, :]
        out["body"], out["head"] = body, head
        return out

    def dust_state(self, device=False) -> dict:
        """The grains as they are now: {"x", "y", "z", "vx", "vy", "vz", "par"}, seven (M,) arrays (torch tensors with
        device=True); dust_begin of them continues the run.  A removed grain keeps its last values."""
        m = self.dust_info(live=False)["n_grains"]
        f = self._form(device)
        a = [f.empty(m) for _ in DUST_STATE]
        f.call("sph_dust_state", *(f.ptr(t) for t in a))
        return dict(zip(DUST_STATE, a))

    def dust_fates(self, device=False) -> dict:
        """The fates of the grains: {"fate", "advance", "sink"}, three (M,) int32 arrays (torch tensors with device=True).
        fate: DUST_ALIVE, DUST_ACCRETED, DUST_CULLED, DUST_NONFINITE."""
        m = self.dust_info(live=False)["n_grains"]
        f = self._form(device)
        fates = f.empty((m, len(DUST_FATES)), np.int32)
        f.call("sph_dust_fates", f.ptr(fates))
        return {name: fates[:, i] for i, name in enumerate(DUST_FATES)}

    # ---- friends-of-friends groups (sph_groups) --------------------------------------------------
    # ---- the movie of a run (sph_frames) -------------------------------------------------------------
    def frames_begin(self, shape, bounds, capacity, every=1, dt_frame=None, rot=None, centre=None, centre_sink=None, fields=(),
                     h=None, clip=None):
        """Starts (or restarts) the device-resident log of frames (include/summersph.h, sph_frames): column-density maps of
        the owned gas on shape nodes over bounds = ((lo_u, lo_v), (hi_u, hi_v)), plus one plane per field weighted by it,
        appended every every-th step of step / run or, with dt_frame, whenever t passes the next multiple of dt_frame since
        now.  rot, centre, h, clip: as cube; centre_sink: the frame follows that sink.  The descriptor is left in
        self.frames_desc."""
        d = frames_desc(shape, bounds, capacity, every, dt_frame, rot, centre, centre_sink, fields, h, clip)
        self._ck(self.lib.sph_frames_begin(self._h, C.byref(d)))
        self.frames_desc = d

    def frames_record(self):
        """Appends a frame of the state as it is now, whatever the cadence (the step number is not advanced)."""
        self._ck(self.lib.sph_frames_record(self._h))

    def frames_rewind(self):
        """Sets the row count to 0 and keeps the allocation: drain a long movie between runs."""
        self._ck(self.lib.sph_frames_rewind(self._h))

    def frames_end(self):
        self._ck(self.lib.sph_frames_end(self._h))

    def frames_info(self) -> dict:
        """rows held, frames dropped and steps counted since frames_begin (reads the device's counts: waits for the stream)"""
        r, d, s = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.lib.sph_frames_info(self._h, C.byref(r), C.byref(d), C.byref(s)))
        return {"rows": r.value, "dropped": d.value, "steps": s.value}

    def frames(self, first=0, count=None, device=False):
        """Frames [first, first + count) of the log (count None: all from first) as frames_columns' dict: step, t, n, n_sel,
        centre, exp, status per frame, planes (rows, 1 + nq, n_u, n_v) and dropped.  device=True: planes and head are torch
        tensors copied on the context's GPU in the stream's order (sph_frames_read_dev); the named columns are read from
        the head."""
        info = self.frames_info()
        d = self.frames_desc
        first = int(first)
        cnt = info["rows"] - first if count is None else int(count)
        f = self._form(device)
        head = f.empty((max(cnt, 0), FRAMES_NHEAD))
        planes = f.empty((max(cnt, 0), 1 + d.nq, d.n_u, d.n_v))
        if device and not 0 <= first <= first + cnt <= info["rows"]:
            raise SphError(-1, "sph_frames_read_dev: first / count outside [0, rows]")
        f.call("sph_frames_read", first, cnt, f.ptr(head), f.ptr(planes))
        out = frames_columns(f.host(head), planes, info["dropped"])
        if device:
            out["head"] = head
        return out

    def frame(self, shape, bounds, rot=None, centre=None, centre_sink=None, fields=(), h=None, clip=None, device=False):
        """One frame of the state as it is now (sph_frame): (head, planes) with head the FRAMES_NHEAD doubles of a log's head
        and planes (1 + nq, n_u, n_v); frames_columns(head[None], planes[None]) names the head's entries.  device=True:
        torch tensors, no stream synchronisation and no read-back (sph_frame_dev).  The descriptor is left in
        self.frame_desc."""
        d = self.frame_desc = frames_desc(shape, bounds, 1, 1, None, rot, centre, centre_sink, fields, h, clip)
        oshape = (1 + d.nq, d.n_u, d.n_v)
        size = int(np.prod(oshape, dtype=np.int64)) if min(oshape) > 0 else 0
        f = self._form(device)
        head = f.empty(FRAMES_NHEAD)
        planes = f.empty([max(k, 0) for k in oshape])
        f.call("sph_frame", C.byref(d), f.ptr(head), f.ptr(planes), size)
        return head, planes

    def _components(self, name, d, n_col, n_count, max_groups, labels, f):
        """the call groups and peaks share: (labels, the max_groups table rows, max_groups, the counts buffer)"""
        n = self.n
        mg = n if max_groups is None else int(max_groups)
        lab = f.empty(n, np.int32) if labels else None
        tab = f.empty((mg, n_col)) if mg > 0 else None
        cnt = f.counts(n_count)
        f.call(name, C.byref(d), f.ptr(lab), n, f.ptr(tab), mg, f.ptr(cnt))
        return lab, tab, mg, cnt

    def groups(self, link, rho_min=-np.inf, min_members=1, link_h=False, clip=None, max_groups=None, labels=True,
               device=False):
        """The friends-of-friends groups of the owned gas (include/summersph.h, sph_groups): particles with rho >= rho_min
        inside the strict clip box ((lo xyz, hi xyz) or None) are linked when closer than link (link_h=True: link *
        max(h_i, h_j)); components with >= min_members members are numbered by N descending, then the smallest id.
        Returns (labels, table, n_groups): labels int32 per particle in the upload order (-1: in no group; None with
        labels=False), table a structured array (GROUPS_COLUMNS) of the first min(n_groups, max_groups) groups (None with
        max_groups == 0; max_groups=None: every group), n_groups the full count.  device=True: labels and the table rows
        (max_groups of them, the first min(n_groups, max_groups) written) are torch tensors on the context's GPU
        (sph_groups_dev); the table is then an (max_groups, GROUPS_NCOL) float64 tensor.  The descriptor used is left in
        self.groups_desc."""
        d = self.groups_desc = groups_desc(link, rho_min, min_members, link_h, clip)
        f = self._form(device)
        lab, tab, mg, cnt = self._components("sph_groups", d, GROUPS_NCOL, 1, max_groups, labels, f)
        ng = f.read(cnt)[0]
        if tab is not None and not device:
            tab = groups_table(tab[:min(ng, mg)])
        return lab, tab, ng

    # ---- density-peak clumps (sph_peaks) ---------------------------------------------------------
    def peaks(self, link, contrast=2.0, rho_min=-np.inf, peak_min=-np.inf, min_members=1, link_h=False, clip=None,
              max_groups=None, labels=True, device=False):
        """The density-peak clumps of the owned gas (include/summersph.h, sph_peaks): among the particles Context.groups
        would select and link, every particle climbs to its densest neighbour; the basins merge across saddles S with
        rho(lower top) < contrast * S (1: the raw basins, inf: the friends-of-friends groups); components whose top is below
        peak_min or with fewer than min_members members are dropped, the rest numbered by N descending, then the smallest id.
        Returns (labels, table, n_groups, counts): labels and table keyed as Context.groups' are (PEAKS_COLUMNS: the
        GROUPS_COLUMNS, S_out and n_peaks), counts = (n_groups, n_raw_peaks, n_edges).  device=True: labels, the
        (max_groups, PEAKS_NCOL) table and the three counts are torch tensors on the context's GPU (sph_peaks_dev; counts[0]
        == -1 tells of a bad h under link_h); the call still waits for the stream, since the merge runs on the host.  The
        descriptor used is left in self.peaks_desc."""
        d = self.peaks_desc = peaks_desc(link, contrast, rho_min, peak_min, min_members, link_h, clip)
        f = self._form(device)
        lab, tab, mg, cnt = self._components("sph_peaks", d, PEAKS_NCOL, PEAKS_NCOUNT, max_groups, labels, f)
        counts = f.read(cnt)
        if device:
            return lab, tab, counts[0], cnt
        return lab, (None if tab is None else peaks_table(tab[:min(counts[0], mg)])), counts[0], counts

    # ---- SPH gradients (sph_gradients) ------------------------------------------------------------
    def gradients(self, fields=("vx", "vy", "vz"), values=None, corrected=True, h=None, clip=None, rho=False, device=False):
        """SPH gradients at the owned gas inside the strict clip box ((lo xyz, hi xyz) or None) (include/summersph.h,
        sph_gradients): corrected=True: adj(C) b / det C (exact for linear fields; NaN at singular targets), False: the
        standard difference form b / rho~.  fields: up to four SPH_F_* names or ids, or GRAD_VALUES for row k of values,
        an (n_rows, sph_count) array in the upload order (float64 numpy; device=True: a contiguous float64 torch tensor on
        the context's GPU).  h: None = each particle's own h, else one h for every target.  Returns (grad, rho~, counts):
        grad an (n_fields, 3, n) array (NaN rows for non-targets), rho~ (n,) or None (rho=False), counts = (n_targets,
        n_singular).  device=True: grad and rho~ are torch tensors on the context's GPU (sph_gradients_dev).  The
        descriptor used is left in self.gradients_desc."""
        d = self.gradients_desc = gradients_desc(fields, corrected, h, clip)
        n, nf = self.n, d.n_fields
        f = self._form(device)
        v = _values_rows("gradients", values, nf if GRAD_VALUES in d.fields[:nf] else 0, n, f)
        out = f.empty((nf, 3, n))
        r = f.empty(n) if rho else None
        args = (C.byref(d), f.ptr(v), f.ptr(out), 3 * nf * n, f.ptr(r))
        if device:                                                # sph_gradients_dev: one pointer to both counts
            cnt = f.counts(2)
            f.call("sph_gradients", *args, f.ptr(cnt))
            return out, r, f.read(cnt)
        nt, ns = C.c_int64(0), C.c_int64(0)
        f.call("sph_gradients", *args, C.byref(nt), C.byref(ns))
        return out, r, (int(nt.value), int(ns.value))

    # ---- SPH interpolation at arbitrary points (sph_sample) ----------------------------------------
    def sample(self, points, fields=(), values=None, weight="mass", normalise=False, h=None, clip=None, weight_out=False,
               counts=False, device=False):
        """The SPH interpolant of the owned gas at arbitrary points (include/summersph.h, sph_sample): with ws = w_j /
        (pi h_j^3), w_j = m_j (weight='mass') or m_j / rho_j ('volume'), den = sum ws Wn and num_k = sum ws A_k Wn over the
        sources strictly inside the clip box ((lo xyz, hi xyz) or None).  points: an (M, 3) array or three arrays of M --
        float64 numpy (host form) or, device=True, contiguous float64 torch tensors on the context's GPU (an (M, 3) tensor
        is split into three).  fields: up to four SPH_F_* names or ids, or SAMPLE_VALUES for row k of values, an (n_rows,
        sph_count) array in the upload order (numpy, or a device tensor with device=True); fields=() gives the weight
        alone (with weight='mass' the SPH density at the points).  h: None = each particle's own h, else one h for all.
        Returns the (K, M) array num, or num / den (0 where den is 0) with normalise=True; with weight_out (always with
        fields=()) and / or counts a tuple (out, den, (n_hit, n_nonfinite)) of the parts asked for -- with fields=() and
        neither flag just den.  device=True: torch tensors (sph_sample_dev).  The descriptor used is left in
        self.sample_desc."""
        d = self.sample_desc = sample_desc(fields, weight, normalise, h, clip)
        n, nf = self.n, d.n_fields
        want_w = weight_out or nf == 0
        f = self._form(device)
        p, m = _points("sample", points, f)
        v = _values_rows("sample", values, nf if SAMPLE_VALUES in d.fields[:nf] else 0, n, f)
        out = f.empty((nf, m))
        w = f.empty(m) if want_w else None
        cnt = f.counts(2)
        f.call("sph_sample", C.byref(d), m, *map(f.ptr, p), f.ptr(v), f.ptr(out) if nf else None, nf * m, f.ptr(w), f.ptr(cnt))
        if nf == 0 and not weight_out and not counts:
            return w
        parts = [out] + ([w] if want_w else []) + ([f.read(cnt)] if counts else [])
        return parts[0] if len(parts) == 1 else tuple(parts)

    # ---- field lines of an SPH-interpolated vector field (sph_trace) -------------------------------
    def trace(self, seeds, n_steps, ds, fields=("vx", "vy", "vz"), values=None, carry=None, arclength=False, omega=None,
              centre=(0.0, 0.0, 0.0), normal=None, box=None, stride=1, weight="mass", h=None, clip=None, counts=False,
              device=False):
        """Field lines of the SPH-interpolated vector field (fields[0], fields[1], fields[2]) of the owned gas (include/
        summersph.h, sph_trace): n_steps classical RK4 steps of ds per seed through the frozen field, the stage velocity being
        exactly Context.sample(..., normalise=True) at the stage point.  seeds: as Context.sample takes points.  fields and
        carry: SPH_F_* names or ids, or TRACE_VALUES for row k (carry: row 3) of values, an (n_rows, sph_count) array in the
        upload order.  ds: a time, or with arclength=True a length along v / |v|; ds < 0 traces upstream.  omega, centre:
        the frame v - omega x (p - centre).  normal: remove v's component along it (TRACE_PLANAR).  box: (lo xyz, hi xyz),
        a line stops outside it.  stride: every stride-th vertex is recorded (divides n_steps).  weight, h, clip: as
        Context.sample.  Returns (path (n_rec + 1, 3, M), status (M) int32, n_done (M) int32[, carry (n_rec + 1, M)][, counts:
        the seeds per status code, TRACE_STATUS]); rows after a line's last vertex are NaN.  device=True: torch tensors
        (sph_trace_dev).  The descriptor used is left in self.trace_desc."""
        d = self.trace_desc = trace_desc(n_steps, ds, fields, carry, arclength, omega, centre, normal, box, stride, weight, h, clip)
        n = self.n
        if d.stride < 1 or d.n_steps < 1 or d.n_steps % d.stride:
            raise ValueError("trace: n_steps >= 1 and stride >= 1 dividing n_steps")
        n_rec = d.n_steps // d.stride
        has_carry = d.carry != TRACE_NONE
        rows = 4 if d.carry == TRACE_VALUES else max([k + 1 for k in range(3) if d.fields[k] == TRACE_VALUES], default=0)
        f = self._form(device)
        p, m = _points("trace", seeds, f, noun="seed")
        v = _values_rows("trace", values, rows, n, f)
        path = f.empty((n_rec + 1, 3, m))
        car = f.empty((n_rec + 1, m)) if has_carry else None
        status, done = f.empty(m, np.int32), f.empty(m, np.int32)
        cnt = f.counts(5)
        f.call("sph_trace", C.byref(d), m, *map(f.ptr, p), f.ptr(v), f.ptr(path), 3 * (n_rec + 1) * m, f.ptr(car), f.ptr(status),
               f.ptr(done), f.ptr(cnt))
        return tuple([path, status, done] + ([car] if has_carry else []) + ([f.read(cnt)] if counts else []))

    # ---- spectral cubes (sph_cube) -----------------------------------------------------------------
    def cube(self, shape, bounds, v0, dv, n_chan, rot=None, centre=(0.0, 0.0, 0.0), v_ref=(0.0, 0.0, 0.0), sigma_scale=0.0,
             sigma_floor=0.0, values=None, h=None, clip=None, per_velocity=False, device=False):
        """The optically thin position-position-velocity cube of the owned gas (include/summersph.h, sph_cube), shape
        (n_chan, n_u, n_v).  shape: image nodes (n or (n_u, n_v)) on the np.linspace node box bounds = ((lo_u, lo_v), (hi_u,
        hi_v)); rot: the 3 x 3 matrix with rows u^, v^, w^ (summersph_amd.cube.view; None = the identity: looking down z);
        channel k is centred on v0 + k dv; sigma_j = sqrt((sigma_scale c_j)^2 + sigma_floor^2); values: None (A = 1: the
        column of mass per channel) or sph_count() numbers in the upload order -- float64 numpy (device=False) or a
        contiguous float64 torch tensor on the context's GPU (device=True); h, clip: as render_density; per_velocity:
        divide by dv.  Returns float64 numpy or, device=True, a torch tensor (sph_cube_dev).  The descriptor used is left
        in self.cube_desc."""
        d = self.cube_desc = cube_desc(shape, bounds, v0, dv, n_chan, rot, centre, v_ref, sigma_scale, sigma_floor, h, clip,
                                       per_velocity)
        oshape = (d.n_chan, d.n_u, d.n_v)
        size = int(np.prod(oshape, dtype=np.int64)) if min(oshape) > 0 else 0
        f = self._form(device)
        v = None if values is None else _values_one("cube", values, self.n, f)
        out = f.empty([max(k, 0) for k in oshape])
        f.call("sph_cube", C.byref(d), f.ptr(v), f.ptr(out), size)
        return out

    # ---- emission-absorption images (sph_transfer) -------------------------------------------------
    def transfer(self, shape, bounds, rot=None, centre=(0.0, 0.0, 0.0), source="u", kappa=None, kappa_scale=1.0, tau_surface=1.0,
                 tau_max=np.inf, background=0.0, h=None, clip=None, device=False):
        """The emission-absorption image of the owned gas (include/summersph.h, sph_transfer), shape (4, n_u, n_v): the planes
        TRANSFER_PLANES -- I + T background, the optical depth, the transmission T and the depth of the tau = tau_surface
        surface (NaN where tau never reaches it).  shape, bounds, rot, centre, h, clip: as cube.  source (S_j) and kappa (K_j,
        the opacity is kappa_scale K_j): a field name or id, None (the constant 1) or sph_count() numbers in the upload
        order -- float64 numpy (device=False) or a contiguous float64 torch tensor on the context's GPU (device=True).  The
        particles are composited front to back; a node stops at tau >= tau_max.  Returns float64 numpy or, device=True, a
        torch tensor (sph_transfer_dev).  The descriptor used is left in self.transfer_desc."""
        d = self.transfer_desc = transfer_desc(shape, bounds, rot, centre, source, kappa, kappa_scale, tau_surface, tau_max,
                                               background, h, clip)
        oshape = (4, d.n_u, d.n_v)
        size = int(np.prod(oshape, dtype=np.int64)) if min(oshape) > 0 else 0
        f = self._form(device)
        sv = _values_one("transfer", source, self.n, f) if d.source == TRANSFER_VALUES else None
        kv = _values_one("transfer", kappa, self.n, f) if d.kappa == TRANSFER_VALUES else None
        out = f.empty([max(k, 0) for k in oshape])
        f.call("sph_transfer", C.byref(d), f.ptr(sv), f.ptr(kv), f.ptr(out), size)
        return out

    # ---- the rates split by physical term (sph_force_terms) -----------------------------------------
    def force_terms(self, skip_gas_gravity=False, device=False, refresh=False):
        """The rates sph_forces would write now, split by term (include/summersph.h, sph_force_terms): a (16, n) array whose
        rows are TERM_ROWS, n = sph_count(), columns in the upload order; ghosts' columns are NaN.  The context must be in
        the state sph_forces needs; refresh=True calls density() first (after a step the records are stale).
        skip_gas_gravity: rows 9-11 are NaN and no tree is walked.  Returns float64 numpy or, device=True, a torch tensor on
        the context's GPU (sph_force_terms_dev).  Every row is a contiguous array that render_field accepts as values."""
        if refresh:
            self.density()
        d = ForceTermsDesc()
        d.flags = TERMS_SKIP_GAS_GRAVITY if skip_gas_gravity else 0
        n = self.n
        f = self._form(device)
        out = f.empty((TERMS_NROW, n))
        f.call("sph_force_terms", C.byref(d), f.ptr(out), TERMS_NROW * n)
        return out

    # ---- binned sums (sph_binned) ---------------------------------------------------------------------
    def binned(self, axes, bins, ranges=None, edges=None, log=(), q=(), weight="mass", values=None, squares=False,
               skip_nan=True, device=False):
        """Per-bin count, sum of a weight and sums of the weight times up to eight quantities of the owned gas over one or
        two binned axes (include/summersph.h, sph_binned).  A source (axes, q) is a field name, an SPH_F_* id or
        binned_row(k): row k of values, an (n_rows, sph_count) array in the upload order (float64 numpy; device=True: a
        contiguous float64 torch tensor on the context's GPU, e.g. what force_terms(device=True) returned).  bins, ranges,
        edges, log: see binned_desc.  weight: "one", "mass" or "volume" (m / rho).  squares: also the sums of w A A;
        skip_nan: drop a particle with a NaN quantity (the non-targets of gradients and force_terms).
        Returns (sums, counts): sums (n0, n1, nsum) float64 with nsum = 2 + n_q (1 + squares), [..., 0] = N, [..., 1] =
        sum w, [..., 2 + k] = sum w A_k, [..., 2 + n_q + k] = sum w A_k A_k (binned.finish turns them into means and
        dispersions); counts = (selected, outside the range, dropped as NaN).  device=True: sums and counts (int64) are torch
        tensors on the context's GPU (sph_binned_dev); as with every device form, torch's current stream is synchronised before
        the call and made to wait for it afterwards.  The descriptor used is left in self.binned_desc."""
        n = self.n
        n_rows = 0
        if values is not None:
            n_rows = int(values.shape[0]) if values.ndim == 2 else 1
        d, tab = binned_desc(axes, bins, ranges, edges, log, q, weight, n_rows, squares, skip_nan)
        self.binned_desc = d
        shape = (max(int(d.n[0]), 0), max(int(d.n[1]), 0), binned_nsum(d.n_q, squares))
        f = self._form(device)
        v = _values_rows("binned", values, n_rows, n, f, exact=True)
        out = f.empty(shape)
        cnt = f.counts(3)
        f.call("sph_binned", C.byref(d), f.ptr(v), None if tab is None else tab.ctypes.data, f.ptr(out),
               shape[0] * shape[1] * shape[2], f.ptr(cnt))
        return out, (cnt if device else f.read(cnt))

    # ---- pair sums (sph_pairs) --------------------------------------------------------------------------
    def pairs(self, r_range, bins, *, log=False, edges=None, scale_h=False, q=(), weight="one", velocity=False, clip=None,
              stride=1, phase=0, values=None, raw=False, device=False):
        """Per bin of the pair separation r (scale_h: of r / h_i), the count of the ordered pairs (i, j), j != i, of the
        owned gas and exact sums over them (include/summersph.h, sph_pairs).  r_range: (lo, hi), or None with edges (bins + 1
        values); log: logarithmic bins.  q: up to PAIRS_MAX_Q quantities A_k, each a field name, an SPH_F_* id or
        pairs_row(k): row k of values, an (n_rows, sph_count) array in the upload order (float64 numpy; device=True: a
        contiguous float64 torch tensor on the context's GPU).  weight: "one" or "mass" (w = m_i m_j).  velocity: also the
        sums of w u, w u^2, w u^3 and w |dv|^2, u the pairwise radial velocity.  The targets i are the usable owned gas
        strictly inside clip (None: everywhere) whose upload index has index % stride == phase; every usable owned gas
        particle is a source.
        Returns (sums, counts, exps) and, with raw=True, also the limbs: sums (n_bins, nsum) float64, nsum = 2 + 2 n_q +
        (4 with velocity), [:, 0] = N, [:, 1] = sum w, [:, 2 + k] = sum w dA_k, [:, 2 + n_q + k] = sum w dA_k^2, then the
        velocity sums (pairs.finish turns them into means); counts = (targets, sources, not usable); exps (nsum,) int32, the
        sums' binary exponents; raw (n_bins, nsum, 2) uint64, the exact 128-bit sums as {low, high} limbs in units of
        2^(exps - 62), which add exactly across calls (pairs.add_raw, then pairs_finish).  device=True: sums, counts
        (int64), exps and raw (as int64, the same bits) are torch tensors on the context's GPU (sph_pairs_dev).  The descriptor
        used is left in self.pairs_desc."""
        n = self.n
        n_rows = 0
        if values is not None:
            n_rows = int(values.shape[0]) if values.ndim == 2 else 1
        d, tab = pairs_desc(r_range, bins, log, edges, scale_h, q, weight, velocity, clip, stride, phase, n_rows)
        self.pairs_desc = d
        nb, nsum = max(int(d.n_bins), 0), pairs_nsum(d.n_q, velocity)
        f = self._form(device)
        v = _values_rows("pairs", values, n_rows, n, f, exact=True)
        out = f.empty((nb, nsum))
        lim = f.empty((nb, nsum, 2), np.int64 if device else np.uint64) if raw else None
        ex = f.empty((nsum,), np.int32)
        cnt = f.counts(3)
        f.call("sph_pairs", C.byref(d), f.ptr(v), None if tab is None else tab.ctypes.data, f.ptr(out), nb * nsum, f.ptr(lim),
               f.ptr(ex), f.ptr(cnt))
        res = (out, cnt if device else f.read(cnt), ex)
        return res + (lim,) if raw else res

    # ---- mode sums (sph_modes) --------------------------------------------------------------------------
    def modes(self, r_range, n_r, m_max, *, log=False, z_max=np.inf, centre=None, centre_v=None, sink=None,
              normal=(0.0, 0.0, 1.0), weight="mass", q=None, values=None, spiral=None, r_ref=1.0, raw=False, device=False):
        """The azimuthal Fourier sums of a weight per ring and the logarithmic-spiral sums of the annulus, exact
        (include/summersph.h, sph_modes).  r_range: (r_min, r_max), n_r rings (log: logarithmic), m = 0 .. m_max; the frame
        as in profile(): centre (and centre_v) or sink, and the normal profile() wrote back; |z'| < z_max.  weight: "one"
        or "mass", times q: None, a field name, an SPH_F_* id or modes_row(k): row k of values, an (n_rows, sph_count) array
        in the upload order (float64 numpy; device=True: a contiguous float64 torch tensor on the context's GPU).  spiral:
        None or (p_min, p_max, n_p), the wavenumbers of the spiral sums of m phi + p ln(R / r_ref).
        Returns (ring, spiral, ring_counts, counts, exp) and, with raw=True, also the limbs: ring (n_r, m_max + 1, 2) float64,
        [k, m, 0] = C = sum w cos m phi, [k, m, 1] = S = sum w sin m phi; spiral (m_max + 1, n_p, 2), [m, l, 0] = CS and
        [m, l, 1] = SN, or None without spiral (modes.finish turns both into amplitudes, phases and pitch angles);
        ring_counts (n_r,) int64; counts = (selected and usable, outside, not usable, at R == 0); exp: the sums' binary
        exponent; raw = (ring limbs (n_r, m_max + 1, 2, 2), spiral limbs or None) uint64, the exact 128-bit sums as {low,
        high} in units of 2^(exp - 62), which add exactly across calls of equal exp (modes.add_raw, then modes_finish).
        device=True: ring, spiral, ring_counts, counts (int64), exp (int32, one element) and raw (as int64, the same bits)
        are torch tensors on the context's GPU (sph_modes_dev).  The descriptor used is left in self.modes_desc."""
        n = self.n
        n_rows = 0
        if values is not None:
            if not device:                                # any array-like of rows; the device form wants its tensor as it is
                values = np.asarray(values, dtype=np.float64)
            n_rows = int(values.shape[0]) if getattr(values, "ndim", 1) == 2 else 1      # not a tensor: _values_rows says so
        d = self.modes_desc = modes_desc(r_range, n_r, m_max, log, z_max, centre, centre_v, sink, normal, weight, q, spiral, r_ref,
                                         n_rows)
        nr, m1, n_p = _modes_sizes(d)
        n_out = 2 * m1 * (nr + n_p)
        f = self._form(device)
        v = _values_rows("modes", values, n_rows, n, f, exact=True)
        out = f.empty((n_out,))
        lim = f.empty((n_out, 2), np.int64 if device else np.uint64) if raw else None
        ex = f.empty((1,), np.int32)
        rc = f.empty((nr,), np.int64)
        cnt = f.counts(4)
        f.call("sph_modes", C.byref(d), f.ptr(v), f.ptr(out), n_out, f.ptr(lim), f.ptr(ex), f.ptr(rc), f.ptr(cnt))
        ring, sp = modes_split(d, out)
        res = (ring, sp, rc, cnt if device else f.read(cnt), ex if device else int(ex[0]))
        return res + (modes_split(d, lim),) if raw else res

    # ---- potential and acceleration at arbitrary points (sph_gravity_at) ---------------------------
    def gravity_at(self, points, h=None, ph=None, soft2=GRAVAT_REF_SOFT2, gas=True, sinks=True, split=False, counts=False,
                   device=False):
        """The gravitational potential and acceleration at arbitrary points (include/summersph.h, sph_gravity_at): the
        Barnes-Hut field of the gas sources (gas=True, with or without FLAG_SELF_GRAVITY) and the unsoftened field of the
        sinks (sinks=True).  points: as Context.sample takes them.  The points' softening length: ph, an array (a device
        tensor with device=True) of M values, else h, else params.h (fixed-h contexts).  Returns (phi, acc) of shapes (M,)
        and (3, M), the sum of the selected parts; split=True: (2, M) and (2, 3, M), the gas first, then the sinks.
        counts=True: (phi, acc, (n_nonfinite_points, n_bad_h)).  device=True: torch tensors (sph_gravity_at_dev).  The
        descriptor used is left in self.gravity_at_desc."""
        d = self.gravity_at_desc = gravity_at_desc(h, soft2, gas, sinks, split)
        rows = 8 if split else 4
        f = self._form(device)
        p, m = _points("gravity_at", points, f, {"ph": ph})
        out = f.empty((rows, m))
        cnt = f.counts(2)
        f.call("sph_gravity_at", C.byref(d), m, *map(f.ptr, p), f.ptr(out), rows * m, f.ptr(cnt))
        if split:
            out = out.reshape(2, 4, m)
            phi, acc = out[:, 0], out[:, 1:]
        else:
            phi, acc = out[0], out[1:]
        return (phi, acc, f.read(cnt)) if counts else (phi, acc)

    # ---- binding energies and unbinding of groups (sph_bound) ----------------------------------------
    def bound(self, labels, n_groups, h=None, soft2=GRAVAT_REF_SOFT2, thermal=False, max_rounds=0, min_members=1,
              max_members=2**31 - 1, device=False):
        """Is each group bound, and which members form its bound core (include/summersph.h, sph_bound): labels is one
        int32 per particle in the upload order (Context.groups' labels, or any partition; values outside 0 ..
        n_groups - 1 mean "in no group").  Every group's own softened potential Phi is a direct pair sum over its members,
        e = 0.5 |v - V|^2 (+ u with thermal=True) + Phi, and up to max_rounds times the members with e >= 0 are removed
        and the rest evaluated again; a set that falls below min_members dissolves, a group with more than max_members
        members is skipped (the cost is the sum of N^2).  h: None = each particle's own h, else one softening length.
        Returns (bound_labels, e, phi, table, counts): bound_labels int32 (the group, or -1), e and phi per particle (NaN
        for non-members), table a structured array (BOUND_COLUMNS) of n_groups rows, counts = (members, skipped,
        dissolved, stopped at max_rounds).  device=True: labels is an int32 tensor on the context's GPU and bound_labels,
        e, phi and the (n_groups, BOUND_NCOL) table are torch tensors (sph_bound_dev); counts[0] == -1 then tells of a
        member with an unusable h.  The descriptor used is left in self.bound_desc."""
        d = self.bound_desc = bound_desc(h, soft2, thermal, max_rounds, min_members, max_members)
        n, ng = self.n, int(n_groups)
        f = self._form(device)
        if not device:
            labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        elif not (f.owns(labels, "int32") and labels.is_contiguous() and labels.numel() == n):
            raise ValueError("bound: device labels must be a contiguous int32 tensor of sph_count values on the context's GPU")
        bl = f.empty(n, np.int32)
        out = f.empty((2, n))
        tab = f.empty((max(ng, 0), BOUND_NCOL))
        cnt = f.counts(4)
        f.call("sph_bound", C.byref(d), f.ptr(labels), n if device else labels.size, ng, f.ptr(bl), f.ptr(out), 2 * n, f.ptr(tab),
               f.ptr(cnt))
        return bl, out[0], out[1], (tab if device else bound_table(tab)), f.read(cnt)

    # ---- diagnostics ---------------------------------------------------------------------
    def stats(self) -> Stats:
        s = Stats()
        self._ck(self.lib.sph_get_stats(self._h, C.byref(s)))
        return s

    def grid_info(self) -> GridInfo:
        """the cell grid of the last build: kind 1 = hashed (SPH_FLAG_HASHED_GRID or a box too sparse for a dense table)"""
        g = GridInfo()
        self._ck(self.lib.sph_get_grid_info(self._h, C.byref(g)))
        return g

    def bbox(self):
        lo = (C.c_double * 3)(); hi = (C.c_double * 3)()
        self._ck(self.lib.sph_get_bbox(self._h, lo, hi))
        return np.array(lo[:]), np.array(hi[:])

    def timing(self, on, only=None, stride=1):
        """HIP events around every kernel group (on=True), none (False), or only the groups named in `only`; stride: bracket
        only every stride-th launch of a timed group (a sample: timing_get returns the bracketed launches)"""
        mask = 0 if not on else (1 if only is None else sum(2 << KERNELS.index(k) for k in only))
        self._ck(self.lib.sph_timing_stride(self._h, max(int(stride), 1)))
        self._ck(self.lib.sph_timing_enable(self._h, mask))

    def timing_reset(self):
        self._ck(self.lib.sph_timing_reset(self._h))

    def timing_get(self, kernel: str):
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._ck(self.lib.sph_timing_get(self._h, KERNELS.index(kernel), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def synchronize(self):
        self._ck(self.lib.sph_synchronize(self._h))

    def stream(self) -> int:
        return int(self.lib.sph_stream(self._h) or 0)
