"""ctypes binding of librsx.so (include/rsx.h).  Thin: argument marshalling and status -> exception.

The library is the product; this module never computes anything itself and there is no CPU
fallback: if librsx.so is missing or no GPU is visible, calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSX_LIB_PATH") or os.path.join(_HERE, "librsx.so")  # override: kernel experiments

NUM_RING, NUM_SECTOR, DESC_SIZE, MAX_TOPK = 20, 60, 1200, 32
MODE_CANDIDATE, MODE_EXHAUSTIVE = 0, 1
# one column of the packed image of the database (rsx_sc_packed_export, include/rsx_diag.h)
PACKED_COL_DTYPE = np.dtype([("bits", np.uint32), ("val", np.float32), ("norm", np.float64)])
FILTER_AUTO, FILTER_OFF, FILTER_FORCE, FILTER_Q1 = 0, 1, 2, 3   # rsx_sc_params.filter_mode
KIND_AUTO, KIND_DIRECT, KIND_SPECTRAL, KIND_SPECTRAL2 = 0, 1, 2, 3   # rsx_sc_params.filter_kind; KIND_SPECTRAL is a synonym of
                                                                     # KIND_SPECTRAL2 (sc_spec2_filter_kernel), kept for callers
SUM_EIGEN_SSE2, SUM_SEQ, SUM_EIGEN_AVX_FMA, SUM_EIGEN34_AVX_FMA = 0, 1, 2, 3   # rsx_sc_params.sum_order (how the reference was built)
default_filter_kind = KIND_AUTO   # what SCManager(filter_kind=KIND_AUTO) passes on (tests flip it to cover both forms)

HIT_DTYPE = np.dtype([("dist", "<f8"), ("index", "<i4"), ("shift", "<i4")])


class RsxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"rsx status {status}: {msg}")
        self.status = status


class ScParams(C.Structure):
    _fields_ = [
        ("lidar_height", C.c_double),
        ("max_radius", C.c_double),
        ("num_exclude_recent", C.c_int32),
        ("num_candidates", C.c_int32),
        ("search_ratio", C.c_double),
        ("dist_thres", C.c_double),
        ("tree_making_period", C.c_int32),
        ("device", C.c_int32),
        ("shard_rank", C.c_int32),
        ("shard_world", C.c_int32),
        ("capacity_hint", C.c_int64),
        ("filter_mode", C.c_int32),
        ("filter_kind", C.c_int32),
        ("sum_order", C.c_int32),
    ]


class RescoringStats(C.Structure):  # rsx_sc_rescoring_stats (include/rsx_diag.h)
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("candidates", C.c_int64), ("exact_evals", C.c_int64),
                ("queries_rescored", C.c_int64), ("window_previews", C.c_int64), ("valu_previews", C.c_int64),
                ("exact_window_shifts", C.c_int64)]


class RescoringStatsTail(RescoringStats):  # the same struct with the fields appended since (struct_size tells the library)
    _fields_ = [("tail_evals", C.c_int64), ("tail_queries", C.c_int64)]


ORORA_PMC = 4  # rsx_orora_params.flags: max-clique inlier selection before the solver
ORORA_PMC_EXACT = 8  # (with ORORA_PMC) exact maximum clique within the handle's node budget
ORORA_PMC_PROVEN, ORORA_PMC_PASSTHROUGH, ORORA_PMC_NO_WORKSPACE, ORORA_PMC_MAXIMUM, ORORA_PMC_BUDGET = 1, 2, 4, 8, 16
PMC_INFO_DTYPE = np.dtype([("size", "<i4"), ("max_core", "<i4"), ("seeds", "<i4"), ("flags", "<i4")])


class ScDetection(C.Structure):
    _fields_ = [("loop_id", C.c_int32), ("yaw_diff_rad", C.c_float), ("min_dist", C.c_double), ("nn_idx", C.c_int32),
                ("query_idx", C.c_int32), ("searched", C.c_int32), ("reserved", C.c_int32), ("dist_thres", C.c_double)]


class OroraParams(C.Structure):
    _fields_ = [("tim_noise_bound", C.c_double), ("noise_bound_radial", C.c_double),
                ("noise_bound_tangential", C.c_double), ("gnc_factor", C.c_double),
                ("cost_threshold", C.c_double), ("max_iterations", C.c_int32), ("flags", C.c_int32)]


class IcpParams(C.Structure):
    _fields_ = [("max_corr_dist", C.c_double), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("max_iterations", C.c_int32), ("flags", C.c_int32)]


class IcpResult(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("fitness", C.c_double), ("iterations", C.c_int32),
                ("converged", C.c_int32), ("state", C.c_int32), ("reserved", C.c_int32)]


class LoopVerifyParams(C.Structure):
    _fields_ = [("history_keyframe_search_num", C.c_int32), ("leaf", C.c_float), ("fitness_threshold", C.c_double), ("icp", IcpParams)]


class LoopVerifyResult(C.Structure):
    _fields_ = [("accepted", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32), ("state", C.c_int32),
                ("fitness", C.c_double), ("transform", C.c_float * 16),
                ("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("roll", C.c_float), ("pitch", C.c_float), ("yaw", C.c_float),
                ("relative", C.c_double * 16), ("n_source", C.c_int64), ("n_target", C.c_int64)]


class FrontendParams(C.Structure):
    _fields_ = [("cart_pixel_width", C.c_int32), ("cart_resolution", C.c_float), ("ratio", C.c_float), ("flags", C.c_int32)]


class Cen2019Params(C.Structure):
    _fields_ = [("max_points", C.c_int32), ("min_range", C.c_int32)]


class Cen2018Params(C.Structure):
    _fields_ = [("zq", C.c_float), ("sigma_gauss", C.c_int32), ("min_range", C.c_int32), ("reserved", C.c_int32)]


class KStrongestParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("z_min", C.c_int32), ("min_range", C.c_int32), ("max_range", C.c_int32),
                ("min_separation", C.c_int32), ("reserved", C.c_int32)]


class CfarParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("train", C.c_int32), ("guard", C.c_int32), ("scale_q8", C.c_int32), ("offset", C.c_int32), ("mode", C.c_int32),
                ("min_range", C.c_int32), ("max_range", C.c_int32), ("min_separation", C.c_int32), ("reserved", C.c_int32)]


CFAR_CA, CFAR_GO, CFAR_SO = 0, 1, 2  # rsx_cfar_params.mode (RSX_CFAR_*)


class CfearParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("max_condition", C.c_double), ("cos_max_normal_angle", C.c_double), ("huber_delta", C.c_double),
                ("step_epsilon", C.c_double), ("min_points", C.c_int32), ("max_iterations", C.c_int32), ("min_correspondences", C.c_int32),
                ("cost", C.c_int32), ("loss", C.c_int32), ("weights", C.c_int32)]


class CfearTrackParams(C.Structure):
    _fields_ = [("keyframe_distance", C.c_double), ("keyframe_rotation", C.c_double), ("n_keyframes", C.c_int32), ("predict", C.c_int32),
                ("search", C.c_int32), ("reserved", C.c_int32 * 2), ("compensate", C.c_int32)]


CFEAR_MAX_POINTS, CFEAR_MAX_SURFACE_POINTS = 16384, 4096
CFEAR_MAX_KEYFRAMES = 4
CFEAR_SEARCH_CELLS, CFEAR_SEARCH_BRUTE = 0, 1  # rsx_cfear_track_params.search
CFEAR_COST_P2L, CFEAR_COST_P2P, CFEAR_COST_P2D = 0, 1, 2  # rsx_cfear_params.cost
CFEAR_LOSS_HUBER, CFEAR_LOSS_CAUCHY, CFEAR_LOSS_NONE = 0, 1, 2  # rsx_cfear_params.loss
CFEAR_STATUS_RANGE, CFEAR_STATUS_POINTS = 1, 2  # scan status word
CFEAR_SURFACE_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("lambda_max", "<f4"), ("lambda_min", "<f4"),
                                      ("n_points", "<i4"), ("cell", "<i4")])
CFEAR_RESULT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("cost", "<f8"), ("iterations", "<i4"), ("correspondences", "<i4"),
                               ("status", "<i4"), ("reserved", "<i4")])
CFEAR_TRACK_RESULT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("reg", CFEAR_RESULT_DTYPE), ("keyframe", "<i4"),
                                     ("n_keyframes", "<i4")])


class CoralParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("det_min", C.c_double), ("min_points", C.c_int32), ("min_other", C.c_int32)]


class CoralResult(C.Structure):
    _fields_ = [("quality", C.c_double), ("h_joint", C.c_double), ("h_separate", C.c_double), ("n_scored", C.c_int32),
                ("n_scored_a", C.c_int32), ("n_valid", C.c_int32), ("status", C.c_int32)]


CORAL_MAX_POINTS = 8192  # per cloud of a job
CORAL_STATUS_RANGE, CORAL_STATUS_POINTS, CORAL_STATUS_EMPTY = 1, 2, 4  # rsx_coral_result.status
CORAL_RESULT_DTYPE = np.dtype([("quality", "<f8"), ("h_joint", "<f8"), ("h_separate", "<f8"), ("n_scored", "<i4"), ("n_scored_a", "<i4"),
                               ("n_valid", "<i4"), ("status", "<i4")])
CORAL_POINT_DTYPE = np.dtype([("det_separate", "<f8"), ("det_joint", "<f8"), ("m_separate", "<i4"), ("m_joint", "<i4")])


class PhasecorrParams(C.Structure):
    _fields_ = [("n", C.c_int32), ("min_range_bins", C.c_int32), ("resolution", C.c_double), ("range_resolution", C.c_double),
                ("max_rotation", C.c_double), ("resolve_half_turn", C.c_int32), ("reserved", C.c_int32)]


class OdometryPhasecorrParams(C.Structure):
    _fields_ = [("pc", PhasecorrParams), ("max_peak_ratio", C.c_double), ("min_peak", C.c_double), ("mode", C.c_int32), ("reserved", C.c_int32)]


PHASECORR_STATUS_ROTATION, PHASECORR_STATUS_INDEX = 1, 2  # rsx_phasecorr_result.status
ODOMETRY_PHASECORR_ESTIMATE, ODOMETRY_PHASECORR_FALLBACK = 0, 1  # rsx_odometry_phasecorr_params.mode
ODOMETRY_STATUS_PHASECORR = 16  # base of a phase-correlation record's non-zero status (| 1: rotation, | 2: a gate)
PHASECORR_RESULT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("peak", "<f8"), ("peak_ratio", "<f8"), ("rot_peak", "<f8"),
                                   ("half_turn", "<i4"), ("status", "<i4")])


class RadarScParams(C.Structure):
    _fields_ = [("max_radius", C.c_double), ("resolution", C.c_float), ("min_range", C.c_int32), ("power_floor", C.c_int32),
                ("stat", C.c_int32)]


RADARSC_MEAN, RADARSC_MAX = 0, 1  # rsx_radarsc_params.stat


class GridmapParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("resolution", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double),
                ("range_resolution", C.c_double), ("max_range", C.c_double), ("min_range_bins", C.c_int32), ("range_halfwidth", C.c_int32),
                ("hit_threshold", C.c_int32), ("reserved", C.c_int32)]


GRIDMAP_MEAN, GRIDMAP_HITS = 0, 1  # render mode (RSX_GRIDMAP_*)
GRIDMAP_STATUS_TRANSFORM = 1  # per-scan status word of rsx_gridmap_add_batch_device


class GridmapMatchParams(C.Structure):
    _fields_ = [("angle_step", C.c_double), ("angle_steps", C.c_int32), ("x_cells", C.c_int32), ("y_cells", C.c_int32), ("reserved", C.c_int32)]


class GridmapMatchResult(C.Structure):
    _fields_ = [("transform", C.c_double * 6), ("k", C.c_int32), ("u", C.c_int32), ("v", C.c_int32), ("score", C.c_uint32),
                ("score_prior", C.c_uint32), ("score_runner_up", C.c_uint32), ("n_points", C.c_int32), ("n_inside", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


GRIDMAP_MATCH_MAX_POINTS = 8192  # RSX_GRIDMAP_MATCH_MAX_POINTS
GRIDMAP_MATCH_STATUS_TRANSFORM, GRIDMAP_MATCH_STATUS_POINTS, GRIDMAP_MATCH_STATUS_EMPTY = 1, 2, 4
GRIDMAP_MATCH_RESULT_DTYPE = np.dtype([("transform", "<f8", 6), ("k", "<i4"), ("u", "<i4"), ("v", "<i4"), ("score", "<u4"), ("score_prior", "<u4"),
                                       ("score_runner_up", "<u4"), ("n_points", "<i4"), ("n_inside", "<i4"), ("status", "<i4"), ("reserved", "<i4")])


class GridmapSearchParams(C.Structure):
    _fields_ = [("angle_step", C.c_double), ("angle_steps", C.c_int32), ("x_cells", C.c_int32), ("y_cells", C.c_int32), ("min_score", C.c_uint32)]


class GridmapSearchResult(C.Structure):
    _fields_ = [("transform", C.c_double * 6), ("k", C.c_int32), ("u", C.c_int32), ("v", C.c_int32), ("score", C.c_uint32),
                ("score_prior", C.c_uint32), ("bound_runner_up", C.c_uint32), ("n_points", C.c_int32), ("n_inside", C.c_int32),
                ("status", C.c_int32), ("n_blocks", C.c_int32), ("n_refined", C.c_int32), ("reserved", C.c_int32)]


GRIDMAP_SEARCH_STATUS_BELOW = 8  # RSX_GRIDMAP_SEARCH_STATUS_BELOW
GRIDMAP_SEARCH_MAX_CELLS, GRIDMAP_SEARCH_MAX_ANGLE_STEPS = 256, 180
GRIDMAP_SEARCH_RESULT_DTYPE = np.dtype([("transform", "<f8", 6), ("k", "<i4"), ("u", "<i4"), ("v", "<i4"), ("score", "<u4"), ("score_prior", "<u4"),
                                        ("bound_runner_up", "<u4"), ("n_points", "<i4"), ("n_inside", "<i4"), ("status", "<i4"), ("n_blocks", "<i4"),
                                        ("n_refined", "<i4"), ("reserved", "<i4")])


class GridmapRefineParams(C.Structure):
    _fields_ = [("damping", C.c_double), ("max_shift_step", C.c_double), ("max_rotation_step", C.c_double), ("shift_tolerance", C.c_double),
                ("rotation_tolerance", C.c_double), ("max_evaluations", C.c_int32), ("reserved", C.c_int32)]


class GridmapRefineResult(C.Structure):
    _fields_ = [("transform", C.c_double * 6), ("hessian", C.c_double * 6), ("cost_initial", C.c_double), ("cost", C.c_double),
                ("score_initial", C.c_double), ("score", C.c_double), ("evaluations", C.c_int32), ("accepted", C.c_int32),
                ("n_points", C.c_int32), ("n_inside", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


GRIDMAP_REFINE_STATUS_SINGULAR, GRIDMAP_REFINE_STATUS_MAX = 16, 32  # RSX_GRIDMAP_REFINE_STATUS_*
GRIDMAP_REFINE_RESULT_DTYPE = np.dtype([("transform", "<f8", 6), ("hessian", "<f8", 6), ("cost_initial", "<f8"), ("cost", "<f8"), ("score_initial", "<f8"),
                                        ("score", "<f8"), ("evaluations", "<i4"), ("accepted", "<i4"), ("n_points", "<i4"), ("n_inside", "<i4"),
                                        ("status", "<i4"), ("reserved", "<i4")])


class GridmapFieldParams(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("radius", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


GRIDMAP_FIELD_MAX_RADIUS = 64  # RSX_GRIDMAP_FIELD_MAX_RADIUS


class GridmapTrackParams(C.Structure):
    _fields_ = [("match", GridmapMatchParams), ("refine", GridmapRefineParams), ("min_score", C.c_uint32), ("predict", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class GridmapTrackResult(C.Structure):
    _fields_ = [("transform", C.c_double * 6), ("start", C.c_double * 6), ("match", GridmapMatchResult), ("refine", GridmapRefineResult),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


GRIDMAP_TRACK_LOST = 1  # RSX_GRIDMAP_TRACK_LOST
GRIDMAP_TRACK_MAX_ANGLE_STEPS, GRIDMAP_TRACK_MAX_CELLS = 8, 8
GRIDMAP_TRACK_RESULT_DTYPE = np.dtype([("transform", "<f8", 6), ("start", "<f8", 6), ("match", GRIDMAP_MATCH_RESULT_DTYPE),
                                       ("refine", GRIDMAP_REFINE_RESULT_DTYPE), ("flags", "<i4"), ("reserved", "<i4")])


class OroraResult(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double), ("iterations", C.c_int32), ("rot_inliers", C.c_int32),
                ("trans_inliers", C.c_int32), ("status", C.c_int32)]


class RansacParams(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("inlier_ratio", C.c_double), ("gn_epsilon", C.c_double), ("dt_scan", C.c_double),
                ("max_iterations", C.c_int32), ("max_gn_iterations", C.c_int32), ("seed", C.c_uint64), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


RANSAC_MOTION_COMPENSATED = 1  # rsx_ransac_params.flags
ESTIMATOR_ORORA, ESTIMATOR_RANSAC, ESTIMATOR_MCRANSAC = 0, 1, 2  # rsx_odometry_set_estimator
ESTIMATOR_CFEAR = 3  # selected by rsx_odometry_set_cfear
ESTIMATOR_PHASECORR = 4  # selected by rsx_odometry_set_phasecorr
RANSAC_RESULT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("wz", "<f8"), ("inliers", "<i4"),
                                ("hypotheses", "<i4"), ("gn_iterations", "<i4"), ("status", "<i4")])


class MocompParams(C.Structure):
    _fields_ = [("dt_scan", C.c_double), ("beta", C.c_double), ("rows", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


MOCOMP_DESKEW, MOCOMP_DOPPLER = 1, 2  # rsx_mocomp_params.flags
MOCOMP_STATUS_ANGLE = 1


class OdometryParams(C.Structure):
    _fields_ = [("cen", Cen2019Params), ("frontend", FrontendParams), ("orora", OroraParams), ("radar_resolution", C.c_float),
                ("col_offset", C.c_int32), ("max_keypoints", C.c_int32), ("device", C.c_int32)]


ODOMETRY_SCAN_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("iterations", "<i4"), ("rot_inliers", "<i4"),
                                ("trans_inliers", "<i4"), ("status", "<i4"), ("n_keypoints", "<i4"), ("n_matches", "<i4")])


ORORA_RESULT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("yaw", "<f8"), ("iterations", "<i4"),
                               ("rot_inliers", "<i4"), ("trans_inliers", "<i4"), ("status", "<i4")])

_lib = None

# every symbol include/rsx.h declares (tests check the .so exports exactly these)
SYMBOLS = [
    "rsx_last_error_string", "rsx_version", "rsx_device_count", "rsx_selftest_firewall", "rsx_selftest_wave",
    "rsx_sc_filter_range_device", "rsx_sc_query_bounds_device",
    "rsx_sc_default_params", "rsx_sc_create", "rsx_sc_destroy", "rsx_sc_set_dist_thres", "rsx_sc_size",
    "rsx_sc_local_size", "rsx_sc_add_points", "rsx_sc_add_descriptor", "rsx_sc_add_descriptors_f32",
    "rsx_sc_add_descriptors_f32_device", "rsx_sc_add_descriptor_rounded", "rsx_sc_export_descriptors_f32",
    "rsx_sc_save", "rsx_sc_load", "rsx_sc_get_descriptor", "rsx_sc_get_ringkey",
    "rsx_sc_get_sectorkey", "rsx_sc_detect_loop_closure", "rsx_sc_detect_loop_closure_ex", "rsx_sc_make_scancontext",
    "rsx_sc_make_keys", "rsx_sc_dist_direct", "rsx_sc_fast_align", "rsx_sc_distance", "rsx_sc_detect_between_session",
    "rsx_sc_tree_size", "rsx_sc_ringkey_tree_layout", "rsx_sc_query", "rsx_sc_query_device", "rsx_sc_query_stage1_device",
    "rsx_sc_query_stage1_elig_device",
    "rsx_sc_query_stage2_device", "rsx_sc_query_self_device",
    "rsx_sc_pair_distances", "rsx_sc_filter_bounds", "rsx_sc_filter_eps", "rsx_sc_profiled_kernel_name",
    "rsx_sc_merge_topk", "rsx_sc_merge_topk_device", "rsx_sc_hit_to_loop",
    "rsx_sc_dominant_kernel_name", "rsx_sc_profile_enable", "rsx_sc_profile_read", "rsx_sc_profile_read_rescoring", "rsx_sc_window_previews",
    "rsx_sc_packed_export", "rsx_sc_rescore_form", "rsx_sc_rescore_force_generic",
    "rsx_scs_create", "rsx_scs_create_layout", "rsx_scs_num_query_groups", "rsx_scs_destroy", "rsx_scs_num_shards", "rsx_scs_set_dist_thres", "rsx_scs_size",
    "rsx_scs_add_points", "rsx_scs_add_descriptors_f32", "rsx_scs_get_descriptor", "rsx_scs_query",
    "rsx_scs_detect_loop_closure",
    "rsx_orora_default_params", "rsx_orora_max_correspondences", "rsx_orora_create", "rsx_orora_destroy",
    "rsx_orora_register_batch", "rsx_orora_register_batch_device", "rsx_orora_max_clique_matches", "rsx_orora_reserve",
    "rsx_orora_max_clique_batch", "rsx_orora_max_clique_batch_device", "rsx_orora_last_pmc_info",
    "rsx_orora_set_clique_node_budget", "rsx_orora_clique_node_budget",
    "rsx_cen2019_default_params", "rsx_cen2019_create", "rsx_cen2019_destroy", "rsx_cen2019_extract",
    "rsx_cen2019_extract_batch", "rsx_cen2019_extract_batch_device",
    "rsx_cen2018_default_params", "rsx_cen2018_create", "rsx_cen2018_destroy", "rsx_cen2018_extract",
    "rsx_cen2018_extract_batch", "rsx_cen2018_extract_batch_device", "rsx_cen2018_gauss_weights", "rsx_cen2018_debug_image",
    "rsx_kstrongest_default_params", "rsx_kstrongest_create", "rsx_kstrongest_destroy", "rsx_kstrongest_extract",
    "rsx_kstrongest_extract_batch", "rsx_kstrongest_extract_batch_device", "rsx_odometry_set_kstrongest",
    "rsx_cfar_default_params", "rsx_cfar_create", "rsx_cfar_destroy", "rsx_cfar_extract", "rsx_cfar_extract_batch",
    "rsx_cfar_extract_batch_device", "rsx_odometry_set_cfar",
    "rsx_cfear_default_params", "rsx_cfear_create", "rsx_cfear_destroy", "rsx_cfear_surface_points_batch",
    "rsx_cfear_surface_points_batch_device", "rsx_cfear_register_batch", "rsx_cfear_register_batch_device", "rsx_odometry_set_cfear", "rsx_odometry_set_cfear_tracking",
    "rsx_cfear_default_track_params", "rsx_cfear_register_keyframes_batch", "rsx_cfear_register_keyframes_batch_device",
    "rsx_cfear_tracker_create", "rsx_cfear_tracker_destroy", "rsx_cfear_tracker_reset", "rsx_cfear_tracker_push", "rsx_cfear_tracker_push_device",
    "rsx_cfear_surface_points_timed_batch", "rsx_cfear_surface_points_timed_batch_device", "rsx_cfear_compensate_batch",
    "rsx_cfear_compensate_batch_device", "rsx_cfear_tracker_push_timed", "rsx_cfear_tracker_push_timed_device",
    "rsx_coral_default_params", "rsx_coral_create", "rsx_coral_destroy", "rsx_coral_quality_batch", "rsx_coral_quality_batch_device",
    "rsx_kfstore_alignment_quality",
    "rsx_phasecorr_default_params", "rsx_phasecorr_create", "rsx_phasecorr_destroy", "rsx_phasecorr_register_batch",
    "rsx_phasecorr_register_batch_device", "rsx_phasecorr_correlation",
    "rsx_odometry_default_phasecorr_params", "rsx_odometry_set_phasecorr",
    "rsx_radarsc_default_params", "rsx_radarsc_create", "rsx_radarsc_destroy", "rsx_radarsc_build_batch", "rsx_radarsc_build_batch_device",
    "rsx_sc_add_polar_batch_device", "rsx_sc_add_polar",
    "rsx_gridmap_default_params", "rsx_gridmap_create", "rsx_gridmap_destroy", "rsx_gridmap_clear", "rsx_gridmap_add_batch",
    "rsx_gridmap_add_batch_device", "rsx_gridmap_read", "rsx_gridmap_planes_device", "rsx_gridmap_render", "rsx_gridmap_render_device",
    "rsx_gridmap_match_default_params", "rsx_gridmap_likelihood_update", "rsx_gridmap_likelihood_set", "rsx_gridmap_likelihood_device",
    "rsx_gridmap_likelihood_read", "rsx_gridmap_match_batch", "rsx_gridmap_match_batch_device",
    "rsx_gridmap_search_default_params", "rsx_gridmap_search_prepare", "rsx_gridmap_search_batch", "rsx_gridmap_search_batch_device",
    "rsx_gridmap_refine_default_params", "rsx_gridmap_refine_batch", "rsx_gridmap_refine_batch_device",
    "rsx_gridmap_field_default_params", "rsx_gridmap_field_gaussian_table", "rsx_gridmap_likelihood_field",
    "rsx_gridmap_track_default_params", "rsx_gridmap_tracker_create", "rsx_gridmap_tracker_destroy", "rsx_gridmap_tracker_reset",
    "rsx_gridmap_tracker_set_pose", "rsx_gridmap_tracker_state", "rsx_gridmap_tracker_push", "rsx_gridmap_tracker_push_device",
    "rsx_odometry_set_cen2018", "rsx_odometry_set_estimator", "rsx_odometry_set_compensation",
    "rsx_mocomp_default_params", "rsx_mocomp_create", "rsx_mocomp_destroy", "rsx_mocomp_points_batch", "rsx_mocomp_points_batch_device",
    "rsx_mocomp_matches_batch", "rsx_mocomp_matches_batch_device",
    "rsx_ransac_default_params", "rsx_ransac_create", "rsx_ransac_destroy", "rsx_ransac_estimate_batch", "rsx_ransac_estimate_batch_device",
    "rsx_frontend_default_params", "rsx_frontend_create", "rsx_frontend_destroy", "rsx_frontend_cartesian",
    "rsx_frontend_describe", "rsx_frontend_match",
    "rsx_frontend_cartesian_batch_device", "rsx_frontend_cartesian_batch_device_az", "rsx_frontend_describe_batch_device", "rsx_frontend_match_consecutive_device",
    "rsx_frontend_read_images",
    "rsx_odometry_default_params", "rsx_odometry_create", "rsx_odometry_destroy", "rsx_odometry_reset", "rsx_odometry_window",
    "rsx_odometry_push", "rsx_odometry_push_device", "rsx_host_alloc_pinned", "rsx_host_free_pinned",
    "rsx_voxelgrid_create", "rsx_voxelgrid_destroy", "rsx_voxelgrid_filter", "rsx_sc_add_points_downsampled",
    "rsx_icp_default_params", "rsx_icp_create", "rsx_icp_destroy", "rsx_icp_align",
    "rsx_kfstore_create", "rsx_kfstore_destroy", "rsx_kfstore_add", "rsx_kfstore_add_device", "rsx_kfstore_size", "rsx_kfstore_get",
    "rsx_loop_verify_default_params", "rsx_loop_submap", "rsx_loop_verify", "rsx_loop_verify_clouds", "rsx_kfstore_build_map", "rsx_sc_add_keyframe",
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RsxError(-7, f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64 (same SONAME
        # as /opt/rocm's).  If librsx pulled in the system runtime first, a later `import torch`
        # would load a second runtime and find no GPU; loading torch first makes librsx bind to
        # the runtime torch already loaded.  (A C++/ROS host has only the system runtime.)
        if os.environ.get("RSX_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        L.rsx_last_error_string.restype = C.c_char_p
        L.rsx_version.restype = C.c_char_p
        L.rsx_sc_dominant_kernel_name.restype = C.c_char_p
        L.rsx_sc_profiled_kernel_name.restype = C.c_char_p
        L.rsx_sc_profiled_kernel_name.argtypes = [C.c_void_p]
        L.rsx_sc_filter_eps.restype = C.c_double
        L.rsx_sc_filter_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.rsx_sc_default_params.argtypes = [C.POINTER(ScParams)]
        L.rsx_sc_create.argtypes = [C.POINTER(ScParams), C.POINTER(vp)]
        L.rsx_sc_destroy.argtypes = [vp]
        L.rsx_sc_set_dist_thres.argtypes = [vp, dbl]
        L.rsx_sc_size.argtypes = [vp, C.POINTER(i64)]
        L.rsx_sc_local_size.argtypes = [vp, C.POINTER(i64)]
        L.rsx_sc_tree_size.argtypes = [vp, C.POINTER(i64)]
        L.rsx_sc_ringkey_tree_layout.argtypes = [vp, i64, vp, vp, vp]
        L.rsx_sc_add_points.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(i32)]
        L.rsx_sc_add_descriptor.argtypes = [vp, vp, C.POINTER(i32)]
        L.rsx_sc_add_descriptors_f32.argtypes = [vp, vp, i64]
        L.rsx_sc_add_descriptors_f32_device.argtypes = [vp, vp, i64, vp]
        L.rsx_sc_add_descriptor_rounded.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(dbl)]
        L.rsx_sc_export_descriptors_f32.argtypes = [vp, i64, i64, vp]
        L.rsx_sc_save.argtypes = [vp, C.c_char_p]
        L.rsx_sc_load.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        L.rsx_sc_get_descriptor.argtypes = [vp, i64, vp]
        L.rsx_sc_get_ringkey.argtypes = [vp, i64, vp]
        L.rsx_sc_get_sectorkey.argtypes = [vp, i64, vp]
        L.rsx_sc_detect_loop_closure.argtypes = [vp, C.c_int, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(dbl), C.POINTER(i32)]
        L.rsx_sc_detect_loop_closure_ex.argtypes = [vp, C.c_int, C.POINTER(ScDetection)]
        L.rsx_sc_make_scancontext.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
        L.rsx_sc_make_keys.argtypes = [vp, vp, vp, vp]
        L.rsx_sc_dist_direct.argtypes = [vp, vp, vp, C.POINTER(dbl)]
        L.rsx_sc_fast_align.argtypes = [vp, vp, vp, C.POINTER(i32)]
        L.rsx_sc_distance.argtypes = [vp, vp, vp, C.POINTER(dbl), C.POINTER(i32)]
        L.rsx_sc_detect_between_session.argtypes = [vp, vp, vp, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(dbl), C.POINTER(i32)]
        L.rsx_sc_query.argtypes = [vp, vp, i32, i32, i64, vp]
        L.rsx_sc_query_device.argtypes = [vp, vp, i32, i32, i64, vp, vp]
        L.rsx_sc_query_stage1_device.argtypes = [vp, vp, i32, i32, i64, vp, vp]
        L.rsx_sc_filter_range_device.argtypes = [vp, vp, i32, i64, i64, vp, i64, vp]
        L.rsx_sc_query_bounds_device.argtypes = [vp, vp, i32, i32, i64, vp, i32, i64, i64, vp, vp]
        L.rsx_sc_query_stage1_elig_device.argtypes = [vp, vp, i32, i32, i64, vp, i32, vp, vp]
        L.rsx_sc_query_stage2_device.argtypes = [vp, i32, i32, vp, vp, vp]
        L.rsx_sc_query_self_device.argtypes = [vp, i64, i32, i32, i64, i32, vp, vp]
        L.rsx_sc_pair_distances.argtypes = [vp, vp, i64, i64, vp, vp]
        L.rsx_sc_merge_topk.argtypes = [vp, i32, i32, i32, vp]
        L.rsx_sc_merge_topk_device.argtypes = [vp, vp, i32, i32, i32, vp, vp]
        L.rsx_sc_profile_enable.argtypes = [vp, C.c_int]
        L.rsx_sc_profile_read.argtypes = [vp, C.POINTER(i64), C.POINTER(dbl)]
        L.rsx_sc_profile_read_rescoring.argtypes = [vp, C.POINTER(RescoringStats)]
        L.rsx_sc_window_previews.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp]
        L.rsx_sc_packed_export.argtypes = [vp, i64, i64, vp]
        L.rsx_sc_rescore_form.argtypes = [vp, C.POINTER(i32), C.POINTER(i64)]
        L.rsx_sc_rescore_force_generic.argtypes = [vp, C.c_int]
        L.rsx_sc_hit_to_loop.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(C.c_float)]
        L.rsx_scs_create.argtypes = [C.POINTER(ScParams), C.POINTER(i32), i32, C.POINTER(vp)]
        L.rsx_scs_create_layout.argtypes = [C.POINTER(ScParams), C.POINTER(i32), i32, i32, i32, C.POINTER(vp)]
        L.rsx_scs_num_query_groups.argtypes = [vp]
        L.rsx_scs_destroy.argtypes = [vp]
        L.rsx_scs_num_shards.argtypes = [vp]
        L.rsx_scs_set_dist_thres.argtypes = [vp, dbl]
        L.rsx_scs_size.argtypes = [vp, C.POINTER(i64)]
        L.rsx_scs_add_points.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(i32)]
        L.rsx_scs_add_descriptors_f32.argtypes = [vp, vp, i64]
        L.rsx_scs_get_descriptor.argtypes = [vp, i64, vp]
        L.rsx_scs_query.argtypes = [vp, vp, i32, i32, i64, vp]
        L.rsx_scs_detect_loop_closure.argtypes = [vp, C.POINTER(ScDetection)]
        L.rsx_orora_default_params.argtypes = [C.POINTER(OroraParams)]
        L.rsx_orora_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_orora_destroy.argtypes = [vp]
        L.rsx_orora_register_batch.argtypes = [vp, vp, vp, vp, i32, C.POINTER(OroraParams), vp]
        L.rsx_orora_register_batch_device.argtypes = [vp, vp, vp, vp, i32, C.POINTER(OroraParams), vp, vp]
        L.rsx_orora_reserve.argtypes = [vp, i64]
        L.rsx_orora_max_clique_batch.argtypes = [vp, vp, vp, vp, i32, C.POINTER(OroraParams), vp, vp]
        L.rsx_orora_max_clique_batch_device.argtypes = [vp, vp, vp, vp, i32, C.POINTER(OroraParams), vp, vp, vp]
        L.rsx_orora_last_pmc_info.argtypes = [vp, vp, i32]
        L.rsx_orora_set_clique_node_budget.argtypes = [vp, i64]
        L.rsx_orora_clique_node_budget.argtypes = [vp, C.POINTER(i64)]
        L.rsx_cen2019_default_params.argtypes = [C.POINTER(Cen2019Params)]
        L.rsx_cen2019_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        L.rsx_cen2019_destroy.argtypes = [vp]
        L.rsx_cen2019_extract.argtypes = [vp, vp, i32, i32, C.POINTER(Cen2019Params), vp, C.c_float, vp, vp, i32,
                                          C.POINTER(i32)]
        L.rsx_cen2019_extract_batch.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(Cen2019Params), vp, i32, C.c_float, vp, vp, i32, vp]
        L.rsx_cen2019_extract_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(Cen2019Params), vp, i32, C.c_float, vp, vp,
                                                       i32, vp, vp]
        L.rsx_cen2018_default_params.argtypes = [C.POINTER(Cen2018Params)]
        L.rsx_cen2018_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        L.rsx_cen2018_destroy.argtypes = [vp]
        L.rsx_cen2018_extract.argtypes = [vp, vp, i32, i32, C.POINTER(Cen2018Params), vp, C.c_float, vp, vp, i32, C.POINTER(i32)]
        L.rsx_cen2018_extract_batch.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(Cen2018Params), vp, i32, C.c_float, vp, vp, i32, vp]
        L.rsx_cen2018_extract_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(Cen2018Params), vp, i32, C.c_float, vp, vp,
                                                       i32, vp, vp]
        L.rsx_cen2018_gauss_weights.argtypes = [i32, vp, i32]
        L.rsx_cen2018_debug_image.argtypes = [vp, vp, i32, i32, C.POINTER(Cen2018Params), vp, vp, vp, vp]
        L.rsx_kstrongest_default_params.argtypes = [C.POINTER(KStrongestParams)]
        L.rsx_kstrongest_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        L.rsx_kstrongest_destroy.argtypes = [vp]
        L.rsx_kstrongest_extract.argtypes = [vp, vp, i32, i32, C.POINTER(KStrongestParams), vp, C.c_float, vp, vp, i32, C.POINTER(i32)]
        L.rsx_kstrongest_extract_batch.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(KStrongestParams), vp, i32, C.c_float, vp, vp, i32, vp]
        L.rsx_kstrongest_extract_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(KStrongestParams), vp, i32, C.c_float, vp, vp,
                                                          i32, vp, vp]
        L.rsx_odometry_set_kstrongest.argtypes = [vp, C.POINTER(KStrongestParams)]
        L.rsx_cfar_default_params.argtypes = [C.POINTER(CfarParams)]
        L.rsx_cfar_create.argtypes = [C.c_int, i32, i32, C.POINTER(vp)]
        L.rsx_cfar_destroy.argtypes = [vp]
        L.rsx_cfar_extract.argtypes = [vp, vp, i32, i32, C.POINTER(CfarParams), vp, C.c_float, vp, vp, i32, C.POINTER(i32)]
        L.rsx_cfar_extract_batch.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(CfarParams), vp, i32, C.c_float, vp, vp, i32, vp]
        L.rsx_cfar_extract_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, C.POINTER(CfarParams), vp, i32, C.c_float, vp, vp, i32, vp, vp]
        L.rsx_odometry_set_cfar.argtypes = [vp, C.POINTER(CfarParams)]
        L.rsx_cfear_default_params.argtypes = [C.POINTER(CfearParams)]
        L.rsx_cfear_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_cfear_destroy.argtypes = [vp]
        L.rsx_cfear_surface_points_batch.argtypes = [vp, vp, vp, i32, C.POINTER(CfearParams), vp, i32, vp, vp]
        L.rsx_cfear_surface_points_batch_device.argtypes = [vp, vp, vp, i32, C.POINTER(CfearParams), vp, i32, vp, vp, vp]
        L.rsx_cfear_register_batch.argtypes = [vp, vp, vp, vp, vp, i32, vp, C.POINTER(CfearParams), vp]
        L.rsx_cfear_register_batch_device.argtypes = [vp, vp, vp, vp, vp, i32, vp, C.POINTER(CfearParams), vp, vp]
        L.rsx_odometry_set_cfear.argtypes = [vp, C.POINTER(CfearParams)]
        L.rsx_odometry_set_cfear_tracking.argtypes = [vp, C.POINTER(CfearTrackParams)]
        L.rsx_cfear_default_track_params.argtypes = [C.POINTER(CfearTrackParams)]
        L.rsx_cfear_register_keyframes_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(CfearParams), C.POINTER(CfearTrackParams), vp]
        L.rsx_cfear_register_keyframes_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(CfearParams),
                                                                C.POINTER(CfearTrackParams), vp, vp]
        L.rsx_cfear_tracker_create.argtypes = [C.c_int, i32, C.POINTER(vp)]
        L.rsx_cfear_tracker_destroy.argtypes = [vp]
        L.rsx_cfear_tracker_reset.argtypes = [vp]
        L.rsx_cfear_tracker_push.argtypes = [vp, vp, vp, vp, C.POINTER(CfearParams), C.POINTER(CfearTrackParams), vp]
        L.rsx_cfear_tracker_push_device.argtypes = [vp, vp, vp, vp, C.POINTER(CfearParams), C.POINTER(CfearTrackParams), vp, vp]
        L.rsx_cfear_surface_points_timed_batch.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(CfearParams), vp, vp, i32, vp, vp]
        L.rsx_cfear_surface_points_timed_batch_device.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(CfearParams), vp, vp, i32, vp, vp, vp]
        L.rsx_cfear_compensate_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
        L.rsx_cfear_compensate_batch_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp]
        L.rsx_cfear_tracker_push_timed.argtypes = [vp, vp, vp, vp, vp, C.POINTER(CfearParams), C.POINTER(CfearTrackParams), vp]
        L.rsx_cfear_tracker_push_timed_device.argtypes = [vp, vp, vp, vp, vp, C.POINTER(CfearParams), C.POINTER(CfearTrackParams), vp, vp]
        L.rsx_coral_default_params.argtypes = [C.POINTER(CoralParams)]
        L.rsx_coral_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_coral_destroy.argtypes = [vp]
        L.rsx_coral_quality_batch.argtypes = [vp, vp, vp, vp, vp, i32, vp, C.POINTER(CoralParams), vp, vp]
        L.rsx_coral_quality_batch_device.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, C.POINTER(CoralParams), vp, vp, vp]
        L.rsx_kfstore_alignment_quality.argtypes = [vp, vp, i32, i32, vp, C.POINTER(CoralParams), C.POINTER(CoralResult)]
        L.rsx_phasecorr_default_params.argtypes = [C.POINTER(PhasecorrParams)]
        L.rsx_phasecorr_create.argtypes = [C.c_int, i32, i32, C.POINTER(PhasecorrParams), C.POINTER(vp)]
        L.rsx_phasecorr_destroy.argtypes = [vp]
        L.rsx_phasecorr_register_batch.argtypes = [vp, vp, i32, i64, i32, i32, vp, i32, vp, vp]
        L.rsx_phasecorr_register_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, vp, i32, vp, vp, vp]
        L.rsx_phasecorr_correlation.argtypes = [vp, i32, vp, vp]
        L.rsx_odometry_default_phasecorr_params.argtypes = [C.POINTER(OdometryPhasecorrParams)]
        L.rsx_odometry_set_phasecorr.argtypes = [vp, C.POINTER(OdometryPhasecorrParams)]
        L.rsx_radarsc_default_params.argtypes = [C.POINTER(RadarScParams)]
        L.rsx_radarsc_create.argtypes = [C.c_int, i32, i32, C.POINTER(RadarScParams), C.POINTER(vp)]
        L.rsx_radarsc_destroy.argtypes = [vp]
        L.rsx_radarsc_build_batch.argtypes = [vp, vp, i32, i64, i32, i32, vp, i32, vp]
        L.rsx_radarsc_build_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, vp, i32, vp, vp]
        L.rsx_sc_add_polar_batch_device.argtypes = [vp, vp, vp, i32, i64, i32, i32, vp, i32, vp]
        L.rsx_sc_add_polar.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(i32)]
        L.rsx_gridmap_default_params.argtypes = [C.POINTER(GridmapParams)]
        L.rsx_gridmap_create.argtypes = [C.c_int, i32, i32, C.POINTER(GridmapParams), C.POINTER(vp)]
        L.rsx_gridmap_destroy.argtypes = [vp]
        L.rsx_gridmap_clear.argtypes = [vp, vp]
        L.rsx_gridmap_add_batch.argtypes = [vp, vp, i32, i64, i32, i32, vp]
        L.rsx_gridmap_add_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, vp, vp, vp]
        L.rsx_gridmap_read.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
        L.rsx_gridmap_planes_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.rsx_gridmap_render.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp]
        L.rsx_gridmap_render_device.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp]
        L.rsx_gridmap_match_default_params.argtypes = [C.POINTER(GridmapMatchParams)]
        L.rsx_gridmap_likelihood_update.argtypes = [vp, i32, i32, vp]
        L.rsx_gridmap_likelihood_set.argtypes = [vp, vp]
        L.rsx_gridmap_likelihood_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.rsx_gridmap_likelihood_read.argtypes = [vp, i32, i32, i32, i32, vp]
        L.rsx_gridmap_match_batch.argtypes = [vp, vp, vp, i32, vp, C.POINTER(GridmapMatchParams), vp, vp]
        L.rsx_gridmap_match_batch_device.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(GridmapMatchParams), vp, vp, vp]
        L.rsx_gridmap_search_default_params.argtypes = [C.POINTER(GridmapSearchParams)]
        L.rsx_gridmap_search_prepare.argtypes = [vp, i32, vp]
        L.rsx_gridmap_search_batch.argtypes = [vp, vp, vp, i32, vp, C.POINTER(GridmapSearchParams), vp, vp]
        L.rsx_gridmap_search_batch_device.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(GridmapSearchParams), vp, vp, vp]
        L.rsx_gridmap_refine_default_params.argtypes = [C.POINTER(GridmapRefineParams)]
        L.rsx_gridmap_refine_batch.argtypes = [vp, vp, vp, i32, vp, C.POINTER(GridmapRefineParams), vp]
        L.rsx_gridmap_refine_batch_device.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(GridmapRefineParams), vp, vp]
        L.rsx_gridmap_field_default_params.argtypes = [C.POINTER(GridmapFieldParams)]
        L.rsx_gridmap_field_gaussian_table.argtypes = [C.c_double, i32, i32, vp]
        L.rsx_gridmap_likelihood_field.argtypes = [vp, C.POINTER(GridmapFieldParams), vp, vp]
        L.rsx_gridmap_track_default_params.argtypes = [C.POINTER(GridmapTrackParams)]
        L.rsx_gridmap_tracker_create.argtypes = [vp, i32, C.POINTER(vp)]
        L.rsx_gridmap_tracker_destroy.argtypes = [vp]
        L.rsx_gridmap_tracker_reset.argtypes = [vp, vp]
        L.rsx_gridmap_tracker_set_pose.argtypes = [vp, i32, vp]
        L.rsx_gridmap_tracker_state.argtypes = [vp, vp, vp, vp]
        L.rsx_gridmap_tracker_push.argtypes = [vp, vp, vp, vp, C.POINTER(GridmapTrackParams), vp]
        L.rsx_gridmap_tracker_push_device.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(GridmapTrackParams), vp, vp]
        L.rsx_odometry_set_cen2018.argtypes = [vp, C.POINTER(Cen2018Params)]
        L.rsx_odometry_set_estimator.argtypes = [vp, C.c_int, C.POINTER(RansacParams)]
        L.rsx_odometry_set_compensation.argtypes = [vp, C.POINTER(MocompParams)]
        L.rsx_mocomp_default_params.argtypes = [C.POINTER(MocompParams)]
        L.rsx_mocomp_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_mocomp_destroy.argtypes = [vp]
        L.rsx_mocomp_points_batch.argtypes = [vp, vp, vp, vp, i32, vp, C.POINTER(MocompParams), vp, vp]
        L.rsx_mocomp_points_batch_device.argtypes = [vp, vp, vp, vp, i32, vp, C.POINTER(MocompParams), vp, vp, vp]
        L.rsx_mocomp_matches_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(MocompParams), vp, vp, vp]
        L.rsx_mocomp_matches_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(MocompParams), vp, vp, vp, vp]
        L.rsx_ransac_default_params.argtypes = [C.POINTER(RansacParams)]
        L.rsx_ransac_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_ransac_destroy.argtypes = [vp]
        L.rsx_ransac_estimate_batch.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(RansacParams), vp, vp]
        L.rsx_ransac_estimate_batch_device.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(RansacParams), vp, vp, vp]
        L.rsx_frontend_default_params.argtypes = [C.POINTER(FrontendParams)]
        L.rsx_frontend_create.argtypes = [C.c_int, i32, i32, C.POINTER(FrontendParams), C.POINTER(vp)]
        L.rsx_frontend_destroy.argtypes = [vp]
        L.rsx_frontend_cartesian.argtypes = [vp, vp, i32, i32, vp, C.c_float, vp]
        L.rsx_frontend_describe.argtypes = [vp, vp, i32, vp, vp]
        L.rsx_frontend_match.argtypes = [vp, vp, vp, i32, vp, vp, i32, C.c_float, vp, vp, vp]
        L.rsx_frontend_cartesian_batch_device.argtypes = [vp, vp, i32, i64, i32, i32, vp, C.c_float, vp]
        L.rsx_frontend_cartesian_batch_device_az.argtypes = [vp, vp, i32, i64, i32, i32, vp, i64, C.c_float, vp]
        L.rsx_frontend_read_images.argtypes = [vp, i32, vp, vp]
        L.rsx_frontend_describe_batch_device.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
        L.rsx_frontend_match_consecutive_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]
        L.rsx_odometry_default_params.argtypes = [C.POINTER(OdometryParams)]
        L.rsx_odometry_create.argtypes = [C.POINTER(OdometryParams), i32, i32, C.POINTER(vp)]
        L.rsx_odometry_destroy.argtypes = [vp]
        L.rsx_odometry_reset.argtypes = [vp]
        L.rsx_odometry_push.argtypes = [vp, vp, i32, i64, i32, vp, i32, vp, vp, i32]
        L.rsx_odometry_push_device.argtypes = [vp, vp, i32, i64, i32, vp, i32, vp, vp, i32]
        L.rsx_host_alloc_pinned.argtypes = [C.c_size_t, C.POINTER(vp)]
        L.rsx_host_free_pinned.argtypes = [vp]
        L.rsx_voxelgrid_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_voxelgrid_destroy.argtypes = [vp]
        L.rsx_voxelgrid_filter.argtypes = [vp, vp, C.c_size_t, C.c_size_t, i32, C.c_float, vp, i64, C.POINTER(i64)]
        L.rsx_sc_add_points_downsampled.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_float, C.POINTER(i32)]
        L.rsx_icp_default_params.argtypes = [C.POINTER(IcpParams)]
        L.rsx_icp_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.rsx_icp_destroy.argtypes = [vp]
        L.rsx_icp_align.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.POINTER(IcpParams), vp,
                                    C.POINTER(IcpResult)]
        L.rsx_kfstore_create.argtypes = [i32, C.POINTER(vp)]
        L.rsx_kfstore_destroy.argtypes = [vp]
        L.rsx_kfstore_add.argtypes = [vp, vp, C.c_size_t, C.c_size_t, i32, C.POINTER(i32)]
        L.rsx_kfstore_add_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(i32)]
        L.rsx_kfstore_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        L.rsx_kfstore_get.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
        L.rsx_loop_verify_default_params.argtypes = [C.POINTER(LoopVerifyParams)]
        L.rsx_loop_submap.argtypes = [vp, i32, i32, vp, C.c_float, vp, i64, C.POINTER(i64)]
        L.rsx_loop_verify.argtypes = [vp, i32, i32, vp, C.POINTER(LoopVerifyParams), C.POINTER(LoopVerifyResult)]
        L.rsx_loop_verify_clouds.argtypes = [vp, i32, i32, vp, C.POINTER(LoopVerifyParams), vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64)]
        L.rsx_kfstore_build_map.argtypes =[vp, vp, i64, i32, C.c_float, vp, i64, C.POINTER(i64)]
        L.rsx_sc_add_keyframe.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, i32, C.c_float, C.POINTER(i32)]
        _lib = L
    return _lib


def check(status):
    if status != 0:
        raise RsxError(status, lib().rsx_last_error_string().decode())


def device_count():
    return lib().rsx_device_count()


def version():
    return lib().rsx_version().decode()


class PinnedArray:
    """A numpy array over page-locked host memory (rsx_host_alloc_pinned): what a caller hands the host-buffer entries
    (rsx_sc_query, rsx_odometry_push, rsx_cen2019_extract ...) so that their uploads run asynchronously at full PCIe rate.
    `.a` is the array; close() (or the context manager) frees the memory -- the array must not be used after that."""

    def __init__(self, shape, dtype):
        import numpy as np
        self._np = np
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        self._p = C.c_void_p()
        check(lib().rsx_host_alloc_pinned(max(n, 1), C.byref(self._p)))
        buf = (C.c_char * max(n, 1)).from_address(self._p.value)
        self.a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if self._p:
            self.a = None
            check(lib().rsx_host_free_pinned(self._p))
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
