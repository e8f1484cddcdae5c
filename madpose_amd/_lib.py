"""ctypes binding of libmadpose_mi355x.so (C ABI: include/madpose_mi355x.h).

The library is built in-tree by madpose_amd/build.py (or __graft_entry__.build()).
There is no CPU fallback: if the library is missing, importing the API raises; if no
MI355X is visible, every compute call raises RuntimeError.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MADPOSE_LIB_VARIANT=name loads lib/libmadpose_mi355x_<name>.so instead: same-box A/B
# of two builds)
_VARIANT = os.environ.get("MADPOSE_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, "lib", "libmadpose_mi355x" + (f"_{_VARIANT}" if _VARIANT.isidentifier() else "") + ".so")

MP_OK, MP_EINVAL, MP_EDEVICE = 0, 1, 2
CALIBRATED, SHARED_FOCAL, TWO_FOCAL, SCALE_ONLY = 0, 1, 2, 3
# the batched solvers (mp_*_batch): samples per call, samples per round when chunk == 0
SOLVE_BATCH_MAX, SOLVE_BATCH_CHUNK = 1 << 22, 32768
# mp_refine_batch: correspondences per resident run when chunk == 0
REFINE_RUN_CORRESPONDENCES = 1 << 22
# mp_select_batch: candidates per record slab when model_chunk == 0; candidates per device
# work item (MP_SELECT_SLAB_MODELS, MP_SELECT_TILE)
SELECT_SLAB_MODELS, SELECT_TILE = 1 << 16, 1
# mp_hypothesize_batch: samples per slab when sample_chunk == 0, samples per call, index
# slots per sample, model slots per sample by variant (MP_HYPOTHESIZE_*)
HYPOTHESIZE_SLAB_SAMPLES, HYPOTHESIZE_MAX_SAMPLES, HYPOTHESIZE_SAMPLE_STRIDE = 32768, 1 << 22, 8
RANSAC_ADAPTIVE_MAX_BUDGET = 1 << 20  # mp_ransac_adaptive_set: samples a pair may get at most
HYPOTHESIZE_SLOTS = (10, 16, 4)
# mp_draw_set: Philox blocks per sample at most, the largest point_share (MP_DRAW_*);
# mp_debug_ransac_timing's values
DRAW_BLOCKS, DRAW_POINT_SHARE_MAX, RANSAC_TIMING_VALUES = 16, 256, 18
# mp_debug_pair_set_record's and mp_debug_ingest_info's values (MP_PAIR_RECORD_VALUES, MP_INGEST_INFO_VALUES)
PAIR_RECORD_VALUES, INGEST_INFO_VALUES = 30, 3

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_int64_p = ctypes.POINTER(ctypes.c_int64)


class mp_ransac_options(ctypes.Structure):
    _fields_ = [
        ("success_probability", ctypes.c_double),
        ("squared_inlier_thresholds", ctypes.c_double * 2),
        ("data_type_weights", ctypes.c_double * 2),
        ("threshold_multiplier", ctypes.c_double),
        ("min_num_iterations", ctypes.c_uint32),
        ("max_num_iterations", ctypes.c_uint32),
        ("max_num_iterations_per_solver", ctypes.c_uint32),
        ("random_seed", ctypes.c_uint32),
        ("num_lo_steps", ctypes.c_int32),
        ("num_lsq_iterations", ctypes.c_int32),
        ("min_sample_multiplicator", ctypes.c_int32),
        ("non_min_sample_multiplier", ctypes.c_int32),
        ("lo_starting_iterations", ctypes.c_int32),
        ("final_least_squares", ctypes.c_int32),
        ("use_ours", ctypes.c_int32),
        ("use_4p4d", ctypes.c_int32),
    ]


class mp_estimator_config(ctypes.Structure):
    _fields_ = [
        ("ceres_function_tolerance", ctypes.c_double),
        ("ceres_gradient_tolerance", ctypes.c_double),
        ("ceres_parameter_tolerance", ctypes.c_double),
        ("ceres_max_num_iterations", ctypes.c_double),
        ("solver_type", ctypes.c_int32),
        ("score_type", ctypes.c_int32),
        ("lo_type", ctypes.c_int32),
        ("min_depth_constraint", ctypes.c_int32),
        ("use_shift", ctypes.c_int32),
        ("ceres_use_nonmonotonic_steps", ctypes.c_int32),
        ("ceres_num_threads", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class mp_device_pairs(ctypes.Structure):
    _fields_ = [
        ("x0", ctypes.c_void_p),
        ("x1", ctypes.c_void_p),
        ("xy_type", ctypes.c_int32),
        ("depth_type", ctypes.c_int32),
        ("d0", ctypes.c_void_p),
        ("d1", ctypes.c_void_p),
        ("depth_maps", ctypes.POINTER(ctypes.c_void_p)),
        ("map_dims", ctypes.POINTER(ctypes.c_int64)),
        ("map_ids", ctypes.POINTER(ctypes.c_int32)),
        ("num_maps", ctypes.c_int32),
        ("map_type", ctypes.c_int32),
        ("producer_stream", ctypes.c_void_p),
    ]


class mp_model(ctypes.Structure):
    _fields_ = [
        ("R", ctypes.c_double * 9),
        ("t", ctypes.c_double * 3),
        ("scale", ctypes.c_double),
        ("offset0", ctypes.c_double),
        ("offset1", ctypes.c_double),
        ("focal0", ctypes.c_double),
        ("focal1", ctypes.c_double),
    ]


class mp_stats(ctypes.Structure):
    _fields_ = [
        ("best_model_score", ctypes.c_double),
        ("inlier_ratios", ctypes.c_double * 3),
        ("num_hypotheses", ctypes.c_uint64),
        ("num_lo_sweeps", ctypes.c_uint64),
        ("num_iterations_total", ctypes.c_uint32),
        ("num_iterations_per_solver", ctypes.c_uint32 * 2),
        ("best_num_inliers", ctypes.c_int32),
        ("best_solver_type", ctypes.c_int32),
        ("number_lo_iterations", ctypes.c_int32),
        ("num_inliers", ctypes.c_int32 * 3),
        ("num_batches", ctypes.c_int32),
        ("seconds_total", ctypes.c_double),
        ("seconds_lo", ctypes.c_double),
        ("seconds_gpu_wait", ctypes.c_double),
    ]


class mp_kernel_profile(ctypes.Structure):
    _fields_ = [
        ("batches", ctypes.c_uint64),
        ("iterations", ctypes.c_uint64),
        ("hypotheses", ctypes.c_uint64),
        ("correspondences", ctypes.c_uint64),
        ("sweeps", ctypes.c_uint64),
        ("solve_ms", ctypes.c_double),
        ("score_ms", ctypes.c_double),
        ("lm_calls", ctypes.c_uint64),
        ("lm_wall_ms", ctypes.c_double),
        ("sweep_wall_ms", ctypes.c_double),
        ("sample_wall_ms", ctypes.c_double),
        ("wait_wall_ms", ctypes.c_double),
        ("run_wall_ms", ctypes.c_double),
        ("lm_blocks", ctypes.c_uint64),
        ("lm_big_calls", ctypes.c_uint64),
        ("lm_big_wall_ms", ctypes.c_double),
        ("model_trips", ctypes.c_uint64),
        ("model_trips_full", ctypes.c_uint64),
        ("accepted", ctypes.c_uint64),
        ("scored", ctypes.c_uint64),
        ("tie_checks", ctypes.c_uint64),
    ]


class mp_refine_result(ctypes.Structure):
    _fields_ = [
        ("score_initial", ctypes.c_double),
        ("score_final", ctypes.c_double),
        ("norm_scale", ctypes.c_double),
        ("rounds_run", ctypes.c_int32),
        ("rounds_accepted", ctypes.c_int32),
        ("lm_status", ctypes.c_int32),
        ("num_inliers", ctypes.c_int32 * 3),
    ]


class mp_select_result(ctypes.Structure):
    _fields_ = [
        ("best_score", ctypes.c_double),
        ("norm_scale", ctypes.c_double),
        ("best_index", ctypes.c_int32),
        ("num_inliers", ctypes.c_int32 * 3),
    ]


class mp_ransac_result(ctypes.Structure):
    _fields_ = [
        ("score_selected", ctypes.c_double),
        ("score_initial", ctypes.c_double),
        ("score_final", ctypes.c_double),
        ("norm_scale", ctypes.c_double),
        ("num_samples", ctypes.c_int32),
        ("num_candidates", ctypes.c_int32),
        ("best_candidate", ctypes.c_int32),
        ("best_sample", ctypes.c_int32),
        ("best_slot", ctypes.c_int32),
        ("best_type", ctypes.c_int32),
        ("rounds_run", ctypes.c_int32),
        ("rounds_accepted", ctypes.c_int32),
        ("lm_status", ctypes.c_int32),
        ("num_inliers", ctypes.c_int32 * 3),
    ]


class mp_ransac_lo_info(ctypes.Structure):
    _fields_ = [
        ("lo_runs", ctypes.c_int32),
        ("lo_accepted", ctypes.c_int32),
        ("lo_index", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


class mp_lsq_fit_result(ctypes.Structure):
    _fields_ = [
        ("score", ctypes.c_double),
        ("num_inliers", ctypes.c_int32 * 3),
        ("num_wide", ctypes.c_int32 * 3),
        ("subset_sizes", ctypes.c_int32 * 3),
        ("status", ctypes.c_int32),
    ]


class mp_ransac_lo_steps_info(ctypes.Structure):
    _fields_ = [
        ("lo_step", ctypes.c_int32),
        ("lo_stage", ctypes.c_int32),
        ("lo_step_offers", ctypes.c_int32),
        ("lo_step_accepted", ctypes.c_int32),
    ]


class mp_inlier_mass(ctypes.Structure):
    _fields_ = [
        ("mass", ctypes.c_uint32 * 3),
        ("total", ctypes.c_uint32),
        ("count", ctypes.c_int32 * 3),
        ("weighted", ctypes.c_int32),
    ]


class mp_residuals_out(ctypes.Structure):
    _fields_ = [
        ("mask", ctypes.c_void_p),
        ("errors", ctypes.c_void_p),
        ("on_device", ctypes.c_int32),
        ("pad", ctypes.c_int32),
        ("producer_stream", ctypes.c_void_p),
    ]


RESIDUALS_MAX_ENTRIES = 1 << 24  # mp_residuals_set's entries per call


class mp_information_out(ctypes.Structure):
    _fields_ = [
        ("H", ctypes.c_void_p),
        ("g", ctypes.c_void_p),
        ("cost", ctypes.c_void_p),
        ("cov", ctypes.c_void_p),
        ("on_device", ctypes.c_int32),
        ("pad", ctypes.c_int32),
        ("producer_stream", ctypes.c_void_p),
    ]


class mp_information_entry(ctypes.Structure):
    _fields_ = [
        ("col", ctypes.c_int32 * 11),
        ("pd", ctypes.c_int32),
        ("status", ctypes.c_int32),
        ("rows", ctypes.c_int32),
        ("counts", ctypes.c_int32 * 3),
    ]


INFORMATION_MAX_ENTRIES = 1 << 24  # mp_information_set's entries per call


class mp_ransac_out(ctypes.Structure):
    _fields_ = [
        ("mask", ctypes.c_void_p),
        ("errors", ctypes.c_void_p),
        ("models", ctypes.c_void_p),
        ("index", ctypes.c_void_p),
        ("counts", ctypes.c_void_p),
        ("producer_stream", ctypes.c_void_p),
    ]


# the weighted draw: the largest pair that may be given weights, the table entries (n + 1) the
# device sampler reads through LDS (MP_DRAW_WEIGHT_MAX_N, MP_DRAW_STAGE_ENTRIES)
DRAW_WEIGHT_MAX_N, DRAW_STAGE_ENTRIES = 65535, 4096
LSQ_RULES = {"lsq": 0, "nonmin": 1}
INLIER_MASS_MAX_ENTRIES = 1 << 24  # mp_inlier_mass_set's entries per call
LO_STEPS_MAX = 64

EXPORTS = {
    "mp_select_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p,
                                       c_double_p, c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                       ctypes.POINTER(mp_estimator_config), c_int64_p, ctypes.POINTER(mp_model),
                                       c_double_p, c_int32_p, ctypes.POINTER(mp_select_result), c_int32_p,
                                       ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "mp_hypothesize_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p,
                                            c_double_p, c_double_p, c_double_p, c_double_p,
                                            ctypes.POINTER(mp_ransac_options), ctypes.POINTER(mp_estimator_config),
                                            c_int64_p, c_int32_p, c_int32_p, ctypes.POINTER(mp_model), c_int32_p,
                                            c_double_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "mp_debug_hypothesize_timing": (ctypes.c_int, [c_double_p]),
    "mp_pair_set_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p,
                                          c_double_p, c_double_p, c_double_p, c_double_p,
                                          ctypes.POINTER(mp_ransac_options), ctypes.POINTER(mp_estimator_config),
                                          ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "mp_pair_set_create_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, c_int64_p,
                                                 ctypes.POINTER(mp_device_pairs), c_double_p, c_double_p, c_double_p,
                                                 ctypes.POINTER(mp_ransac_options),
                                                 ctypes.POINTER(mp_estimator_config), ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_void_p)]),
    "mp_debug_pair_set_record": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p]),
    "mp_debug_ingest_info": (ctypes.c_int, [c_int32_p]),
    "mp_debug_device_extent": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_int64_p]),
    "mp_pair_set_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mp_pair_set_info": (ctypes.c_int, [ctypes.c_void_p, c_int32_p, c_int32_p, c_int64_p, c_int64_p, c_int32_p]),
    "mp_pair_set_norm_scales": (ctypes.c_int, [ctypes.c_void_p, c_double_p]),
    "mp_refine_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int,
                                     ctypes.POINTER(mp_model), ctypes.POINTER(mp_refine_result), c_int32_p]),
    "mp_select_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, c_int64_p, ctypes.POINTER(mp_model),
                                     c_double_p, c_int32_p, ctypes.POINTER(mp_select_result), c_int32_p,
                                     ctypes.c_int64]),
    "mp_hypothesize_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, c_int64_p, c_int32_p, c_int32_p,
                                          ctypes.POINTER(mp_model), c_int32_p, ctypes.c_int64]),
    "mp_draw_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int32, ctypes.c_uint64,
                                   ctypes.c_int32, c_int32_p, c_int32_p, c_int32_p]),
    "mp_debug_draw_host": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int32, c_int32_p]),
    "mp_candidates_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, c_int64_p, c_int32_p, c_int32_p,
                                         ctypes.c_int64, c_int64_p]),
    "mp_candidates_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(mp_model), c_int64_p, c_int32_p,
                                           c_int32_p]),
    "mp_ransac_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int32, ctypes.c_uint64,
                                     ctypes.c_int32, c_int64_p, c_int32_p, c_int32_p, ctypes.c_int32,
                                     ctypes.POINTER(mp_model), ctypes.POINTER(mp_ransac_result), c_int32_p,
                                     ctypes.c_int64, ctypes.c_int64]),
    "mp_ransac_adaptive_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.POINTER(mp_model), ctypes.POINTER(mp_ransac_result), c_int32_p,
                                              c_int32_p, ctypes.c_int64, ctypes.c_int64]),
    "mp_refine_relaxed_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int,
                                             ctypes.POINTER(mp_model), ctypes.POINTER(mp_refine_result), c_int32_p]),
    "mp_ransac_lo_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.POINTER(mp_model), ctypes.POINTER(mp_ransac_result), c_int32_p,
                                        c_int32_p, ctypes.POINTER(mp_ransac_lo_info), ctypes.c_int64, ctypes.c_int64]),
    "mp_lsq_fit_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, c_int32_p, c_double_p, ctypes.c_int,
                                      ctypes.c_uint64, c_int32_p, c_int32_p, ctypes.POINTER(mp_model),
                                      ctypes.POINTER(mp_lsq_fit_result), c_int32_p, ctypes.c_int64]),
    "mp_debug_subset_select": (ctypes.c_int, [c_int64_p, c_int32_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, c_int32_p, c_int32_p,
                                              ctypes.c_int]),
    "mp_debug_subset_select_host": (ctypes.c_int, [c_int64_p, c_int32_p, ctypes.c_int64, ctypes.c_uint64,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                                   c_int32_p, c_int32_p]),
    "mp_debug_lsq_subset_size": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                                ctypes.c_int32, c_int32_p, c_int64_p, c_int32_p]),
    "mp_ransac_lo_steps_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(mp_model),
                                              ctypes.POINTER(mp_ransac_result), c_int32_p, c_int32_p,
                                              ctypes.POINTER(mp_ransac_lo_info),
                                              ctypes.POINTER(mp_ransac_lo_steps_info), ctypes.c_int64,
                                              ctypes.c_int64]),
    "mp_draw_weights_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.POINTER(ctypes.c_uint8), ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_void_p)]),
    "mp_draw_weights_info": (ctypes.c_int, [ctypes.c_void_p, c_int32_p, c_int32_p, ctypes.POINTER(ctypes.c_uint32)]),
    "mp_draw_weights_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mp_draw_weighted_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, c_int32_p,
                                            ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, c_int32_p, c_int32_p,
                                            c_int32_p]),
    "mp_ransac_weighted_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, c_int32_p,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.POINTER(mp_model), ctypes.POINTER(mp_ransac_result), c_int32_p,
                                              c_int32_p, ctypes.POINTER(mp_ransac_lo_info),
                                              ctypes.POINTER(mp_ransac_lo_steps_info), ctypes.c_int64,
                                              ctypes.c_int64]),
    "mp_inlier_mass_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, c_int32_p,
                                          ctypes.POINTER(mp_model), ctypes.POINTER(mp_inlier_mass)]),
    "mp_ransac_weighted_stop_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, c_int32_p,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.POINTER(mp_model), ctypes.POINTER(mp_ransac_result),
                                                   c_int32_p, c_int32_p, ctypes.POINTER(mp_ransac_lo_info),
                                                   ctypes.POINTER(mp_ransac_lo_steps_info), ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.POINTER(mp_inlier_mass)]),
    "mp_debug_ransac_required_mass": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                                     ctypes.POINTER(mp_ransac_options),
                                                     ctypes.POINTER(ctypes.c_uint32)]),
    "mp_debug_inlier_mass_host": (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(ctypes.c_uint32), c_int64_p, c_int32_p,
                                                 ctypes.POINTER(ctypes.c_uint32)]),
    "mp_debug_inlier_mass_stats": (ctypes.c_int, [c_int64_p, c_double_p, ctypes.c_int32]),
    "mp_residuals_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.POINTER(mp_model),
                                        c_double_p, ctypes.POINTER(mp_residuals_out), c_int64_p, c_int32_p]),
    "mp_debug_residuals_stats": (ctypes.c_int, [c_int64_p, c_double_p, ctypes.c_int32]),
    "mp_information_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.POINTER(mp_model),
                                          c_double_p, ctypes.POINTER(mp_information_out),
                                          ctypes.POINTER(mp_information_entry)]),
    "mp_debug_information_finish": (ctypes.c_int, [c_double_p, c_double_p, c_int32_p, c_double_p, c_int32_p]),
    "mp_debug_information_stats": (ctypes.c_int, [c_int64_p, c_double_p, c_double_p, ctypes.c_int32]),
    "mp_ransac_out_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, c_int32_p, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, c_int64_p, c_int32_p,
                                         c_int32_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.POINTER(mp_model), ctypes.POINTER(mp_ransac_result), c_int32_p,
                                         c_int32_p, ctypes.POINTER(mp_ransac_lo_info),
                                         ctypes.POINTER(mp_ransac_lo_steps_info), ctypes.c_int64, ctypes.c_int64,
                                         ctypes.POINTER(mp_inlier_mass), ctypes.POINTER(mp_ransac_out)]),
    "mp_debug_ransac_out_stats": (ctypes.c_int, [c_int64_p, c_double_p, ctypes.c_int32]),
    "mp_debug_draw_weights_host": (ctypes.c_int, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_uint32), c_int32_p]),
    "mp_debug_draw_weighted_host": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint32),
                                                   ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   c_int32_p]),
    "mp_debug_ransac_lo_track": (ctypes.c_int, [ctypes.c_int32, c_double_p, c_int32_p, c_int32_p, c_int32_p,
                                                c_double_p, c_int32_p, c_double_p, c_int32_p]),
    "mp_debug_ransac_required": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_int32_p,
                                                ctypes.POINTER(mp_ransac_options), ctypes.POINTER(ctypes.c_uint32)]),
    "mp_debug_select_argmin": (ctypes.c_int, [ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_int32_p,
                                              c_double_p, ctypes.c_int]),
    "mp_debug_ransac_timing": (ctypes.c_int, [c_double_p]),
    "mp_debug_pair_set_prep": (ctypes.c_int, [ctypes.c_int]),
    "mp_debug_pair_set_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p]),
    "mp_debug_select_tile": (ctypes.c_int, [ctypes.c_int]),
    "mp_debug_select_timing": (ctypes.c_int, [c_double_p]),
    "mp_refine_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p,
                                       c_double_p, c_double_p, c_double_p, c_double_p,
                                       ctypes.POINTER(mp_ransac_options), ctypes.POINTER(mp_estimator_config),
                                       ctypes.c_int32, ctypes.POINTER(mp_model), ctypes.POINTER(mp_refine_result),
                                       c_int32_p, ctypes.c_int64, ctypes.c_int]),
    "mp_estimate": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                   c_double_p, c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                   ctypes.POINTER(mp_estimator_config), ctypes.POINTER(mp_model),
                                   ctypes.POINTER(mp_stats), c_int32_p, ctypes.c_int]),
    "mp_estimate_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p,
                                         c_double_p, c_double_p, c_double_p, c_double_p,
                                         ctypes.POINTER(mp_ransac_options), ctypes.POINTER(mp_estimator_config),
                                         ctypes.POINTER(mp_model), ctypes.POINTER(mp_stats), c_int32_p, ctypes.c_int,
                                         ctypes.c_int]),
    "mp_get_depths": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, c_int64_p, c_int64_p, c_double_p,
                                     ctypes.c_void_p, ctypes.c_int]),
    "mp_lm_refine_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                          c_double_p, c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                          ctypes.POINTER(mp_estimator_config), ctypes.c_int32, c_int32_p, c_int64_p,
                                          c_int32_p, ctypes.POINTER(mp_model), c_int32_p, ctypes.c_int]),
    "mp_debug_lm_refine_host": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                                               c_double_p, c_double_p, c_double_p, c_double_p,
                                               ctypes.POINTER(mp_ransac_options), ctypes.POINTER(mp_estimator_config),
                                               ctypes.c_int32, c_int32_p, c_int64_p, c_int32_p,
                                               ctypes.POINTER(mp_model), c_int32_p]),
    "mp_debug_lm_system": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                                          c_double_p, c_double_p, c_double_p, c_double_p,
                                          ctypes.POINTER(mp_ransac_options), ctypes.POINTER(mp_estimator_config),
                                          ctypes.c_int32, c_int32_p, c_int64_p, c_int32_p, ctypes.POINTER(mp_model),
                                          c_double_p, ctypes.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p,
                                          c_int32_p, c_double_p, c_int32_p, c_int32_p, ctypes.c_int]),
    "mp_bougnoux_focals": (ctypes.c_int, [ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int]),
    "mp_pose_eval": (ctypes.c_int, [ctypes.c_int64, c_double_p, c_double_p, c_double_p, ctypes.c_double, c_double_p,
                                    c_double_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_int]),
    "mp_pose_auc": (ctypes.c_int, [ctypes.c_int64, c_double_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_int]),
    "mp_estimate_scale_and_pose": (ctypes.c_int, [c_double_p, c_double_p, c_double_p, ctypes.c_int64,
                                                  ctypes.POINTER(mp_model), ctypes.c_int]),
    "mp_solve_scale_and_shift": (ctypes.c_int, [ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                                c_double_p, ctypes.c_int, ctypes.c_int]),
    "mp_solve_scale_shift_pose": (ctypes.c_int, [ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                                 ctypes.POINTER(mp_model), ctypes.c_int, ctypes.c_int]),
    "mp_solve_scale_shift_pose_alt": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                                     c_double_p, ctypes.POINTER(mp_model), ctypes.c_int, ctypes.c_int]),
    "mp_score_models": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                       c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                       ctypes.POINTER(mp_estimator_config), ctypes.POINTER(mp_model), ctypes.c_int32,
                                       c_double_p, c_double_p, ctypes.c_int]),
    "mp_debug_score_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                                            c_double_p, c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                            ctypes.POINTER(mp_estimator_config), ctypes.c_int32, c_int32_p,
                                            ctypes.POINTER(mp_model), ctypes.c_double, ctypes.c_int32, c_double_p,
                                            c_int32_p, ctypes.POINTER(mp_model), c_double_p, c_double_p,
                                            ctypes.c_int]),
    "mp_debug_score_terms": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                                            c_double_p, c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                            ctypes.POINTER(mp_estimator_config), ctypes.POINTER(mp_model),
                                            ctypes.c_int32, c_double_p, c_int32_p, c_double_p, c_double_p,
                                            ctypes.c_int]),
    "mp_debug_score_margins": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                                              c_double_p, c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                              ctypes.POINTER(mp_estimator_config), ctypes.POINTER(mp_model),
                                              ctypes.c_int32, c_double_p, c_double_p]),
    "mp_debug_lo_sweep": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                         c_double_p, c_double_p, ctypes.POINTER(mp_ransac_options),
                                         ctypes.POINTER(mp_estimator_config), ctypes.POINTER(mp_model), ctypes.c_int32,
                                         c_double_p, c_double_p, c_double_p]),
    "mp_relpose_5pt": (ctypes.c_int, [c_double_p, c_double_p, ctypes.POINTER(mp_model), ctypes.c_int, ctypes.c_int]),
    "mp_debug_pt5_roots": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                                          ctypes.POINTER(ctypes.c_int32), ctypes.c_int]),
    "mp_debug_pt_roots": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p,
                                         c_double_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]),
    "mp_solve_scale_and_shift_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p,
                                                      c_double_p, c_double_p, c_double_p, c_int32_p,
                                                      ctypes.c_int64, ctypes.c_int]),
    "mp_solve_scale_shift_pose_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_double_p,
                                                       c_double_p, c_double_p, c_double_p,
                                                       ctypes.POINTER(mp_model), c_int32_p, ctypes.c_int64,
                                                       ctypes.c_int]),
    "mp_relpose_batch": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p,
                                        ctypes.POINTER(mp_model), c_int32_p, ctypes.c_int64, ctypes.c_int]),
    "mp_relpose_6pt_shared_focal": (ctypes.c_int, [c_double_p, c_double_p, ctypes.POINTER(mp_model), ctypes.c_int,
                                                   ctypes.c_int]),
    "mp_relpose_7pt_two_focal": (ctypes.c_int, [c_double_p, c_double_p, ctypes.POINTER(mp_model), ctypes.c_int,
                                                ctypes.c_int]),
    "mp_debug_random_stream": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int32, c_double_p]),
    "mp_debug_iteration_stream": (ctypes.c_int, [ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32,
                                                 ctypes.c_int32, c_int32_p, c_int32_p]),
    "mp_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "mp_profile_reset": (ctypes.c_int, []),
    "mp_profile_read": (ctypes.c_int, [ctypes.POINTER(mp_kernel_profile)]),
    "mp_last_error": (ctypes.c_char_p, []),
    "mp_device_count": (ctypes.c_int, []),
    "mp_lo_spin_us": (ctypes.c_int, []),
    "mp_version": (ctypes.c_char_p, []),
}

_lib = None


def lib():
    """Load the engine library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"madpose_amd: native library not found at {LIB_PATH}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)"
            )
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code == MP_OK:
        return
    msg = lib().mp_last_error().decode(errors="replace")
    if code == MP_EINVAL:
        raise ValueError(msg)
    raise RuntimeError(f"madpose_amd device error: {msg}")
