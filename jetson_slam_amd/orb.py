"""Python host mirror of the reference's front-end interface, bound to libjsorb.so through its C ABI (include/jsorb.h).

Names and argument meaning follow the reference so that parity tests read like its call sites:
  ORBExtractor(...)            <- Jetson_SLAM::ORBExtractor::ORBExtractor       include/ORBextractor.h:25-35
  ORBExtractor.extract(image)  <- ORBExtractor::extract -> ORB_GPU::extract     include/ORBextractor.h:40-42, src/cuda/orb_gpu.cpp:489
  get_levels/get_scale_factor/get_scale_factors/get_inverse_scale_factors/
  get_scale_sigma_squares/get_inverse_scale_sigma_squares                      include/ORBextractor.h:44-72, src/ORBextractor.cpp:43-71
  compute_stereo_matches(l, r) <- Frame::ComputeStereoMatches                   src/Frame.cpp:780-803
There is no CPU fallback here: if libjsorb.so or a gfx950 device is missing the calls raise.
"""
import ctypes as C
import os

# the library's default for the HIP runtime (csrc/jsorb_api.hip, jsorb_runtime_defaults); effective when nothing has touched the GPU yet
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libjsorb.so")

MAX_LEVELS = 16
TH_HIGH, TH_LOW = 100, 50   # ORBmatcher::TH_HIGH / TH_LOW, src/ORBmatcher.cpp:24-25

KERNELS = ["k_pyramid", "k_detect", "k_compact", "k_blur", "k_describe", "k_stereo", "k_median", "k_nms_ms"]
# kernel ids beyond KERNELS (jsorb_kernel_time; KERNELS stays the list of the eight pipeline stages)
K_RECTIFY = 8
K_UNDISTORT = 9     # JSORB_K_UNDISTORT (jsorb_set_camera)
K_RGBD = 10         # JSORB_K_RGBD (jsorb_rgbd_depth*)
# jsorb_search_local_points*: ids after JSORB_K_COUNT_ALL (11, which names no kernel)
K_ASSIGN_GRID, K_LOCAL_CANDIDATES, K_LOCAL_RESOLVE = 12, 13, 14
# jsorb_search_last_frame*: ids from JSORB_K_ID_END (15) on; the grid is K_ASSIGN_GRID again
K_LAST_MATCH, K_LAST_RESOLVE = 15, 16
# jsorb_bow_transform* / jsorb_search_by_bow*: ids after JSORB_K_ID_COUNT (17, which names no kernel)
K_BOW_TRANSFORM, K_BOW_GROUP, K_BOW_MATCH, K_BOW_RESOLVE = 18, 19, 20, 21
# jsorb_search_by_projection_kf*: ids after JSORB_K_ID_ALL (22, which names no kernel); the grid is K_ASSIGN_GRID again
K_KF_CANDIDATES, K_KF_RESOLVE = 23, 24
DEPTH_F32, DEPTH_U16 = 0, 1      # JSORB_DEPTH_F32 / JSORB_DEPTH_U16

EXPORTS = [
    "jsorb_create", "jsorb_destroy", "jsorb_last_error", "jsorb_version", "jsorb_plan_launch", "jsorb_extract", "jsorb_extract_into", "jsorb_extract_device",
    "jsorb_extract_batch_device_async", "jsorb_extract_batch_host_async", "jsorb_sync", "jsorb_n_images", "jsorb_n_keypoints",
    "jsorb_level_n_keypoints", "jsorb_keypoints_device", "jsorb_descriptors_device", "jsorb_copy_keypoints",
    "jsorb_copy_descriptors", "jsorb_n_levels", "jsorb_level_dims", "jsorb_level_tiles", "jsorb_total_tiles", "jsorb_scale",
    "jsorb_inv_scale", "jsorb_level_image_device", "jsorb_copy_level_image", "jsorb_copy_tile_candidates", "jsorb_copy_angles",
    "jsorb_stereo_match", "jsorb_stereo_match_batch_async", "jsorb_stereo_uright_device", "jsorb_stereo_depth_device",
    "jsorb_copy_stereo", "jsorb_copy_stereo_l1", "jsorb_set_stereo_diagnostics", "jsorb_copy_stereo_diagnostics", "jsorb_set_speculative_stereo", "jsorb_speculative_stereo_stats", "jsorb_gather_counts_async", "jsorb_set_stream", "jsorb_get_stream", "jsorb_stream_wait_done", "jsorb_enable_kernel_timing", "jsorb_kernel_time",
    "jsorb_reset_kernel_timing", "jsorb_kernel_name", "jsorb_project_points", "jsorb_hamming_pairs", "jsorb_is_in_frustum",
    "jsorb_unpack_frame", "jsorb_assign_features_to_grid", "jsorb_copy_level_mask",
    "jsorb_mem_set_device", "jsorb_mem_alloc_host", "jsorb_mem_alloc_device", "jsorb_mem_alloc_device_pitched", "jsorb_mem_free_host",
    "jsorb_mem_free_device", "jsorb_mem_stream_create", "jsorb_mem_stream_destroy", "jsorb_mem_stream_sync", "jsorb_mem_device_sync", "jsorb_mem_buffer_sync", "jsorb_mem_h2d", "jsorb_mem_d2h",
    "jsorb_mem_d2d", "jsorb_mem_h2d_async", "jsorb_mem_d2h_async", "jsorb_mem_d2d_async", "jsorb_mem_set_zero", "jsorb_mem_set_zero_async",
    "jsorb_mem_last_error", "jsorb_read_mask_image", "jsorb_mask_image_last_error", "jsorb_create_masked",
    "jsorb_set_rectify_maps", "jsorb_set_rectify_maps_fixed", "jsorb_clear_rectify_maps", "jsorb_rectify_enabled", "jsorb_rectify_convert_maps",
    "jsorb_set_camera", "jsorb_camera_enabled", "jsorb_image_bounds", "jsorb_keypoints_un_device", "jsorb_copy_keypoints_un", "jsorb_unpack_frame_un",
    "jsorb_rgbd_depth", "jsorb_rgbd_depth_batch_device_async", "jsorb_rgbd_uright_device", "jsorb_rgbd_depth_device", "jsorb_copy_rgbd",
    "jsorb_search_local_points_async", "jsorb_search_local_points", "jsorb_search_local_stats", "jsorb_plan_forms", "jsorb_handle_forms",
    "jsorb_search_last_frame_async", "jsorb_search_last_frame", "jsorb_search_last_frame_stats",
    "jsorb_search_for_initialization_async", "jsorb_search_for_initialization", "jsorb_search_for_initialization_stats",
    "jsorb_init_reference_set", "jsorb_init_reference_clear", "jsorb_init_reference_n", "jsorb_search_initial_frame",
    "jsorb_vocabulary_create", "jsorb_vocabulary_destroy", "jsorb_vocabulary_info", "jsorb_bow_transform_descriptors", "jsorb_bow_transform_async",
    "jsorb_bow_word_device", "jsorb_bow_node_device", "jsorb_copy_bow", "jsorb_bow_transform_stats", "jsorb_search_by_bow_async",
    "jsorb_search_by_bow", "jsorb_search_by_bow_stats", "jsorb_bow_build_caps",
    "jsorb_search_by_projection_kf_async", "jsorb_search_by_projection_kf", "jsorb_search_by_projection_kf_stats", "jsorb_search_kf_build_caps",
    "jsorb_keyframe_matcher_create", "jsorb_keyframe_matcher_destroy", "jsorb_keyframe_matcher_set_stream", "jsorb_keyframe_matcher_get_stream",
    "jsorb_keyframe_matcher_last_error", "jsorb_search_for_triangulation_async", "jsorb_search_for_triangulation",
    "jsorb_search_for_triangulation_stats", "jsorb_fuse_async", "jsorb_fuse", "jsorb_fuse_stats",
    "jsorb_search_by_bow_kf_async", "jsorb_search_by_bow_kf", "jsorb_search_by_bow_kf_stats", "jsorb_loop_build_caps",
    "jsorb_search_by_sim3_async", "jsorb_search_by_sim3", "jsorb_search_by_sim3_stats",
    "jsorb_search_by_projection_sim3_async", "jsorb_search_by_projection_sim3", "jsorb_search_by_projection_sim3_stats", "jsorb_scw_build_caps",
    "jsorb_distinctive_descriptors_async", "jsorb_distinctive_descriptors", "jsorb_distinctive_descriptors_stats", "jsorb_distinct_build_caps",
    "jsorb_keyframe_database_create", "jsorb_keyframe_database_destroy", "jsorb_keyframe_database_set_stream", "jsorb_keyframe_database_get_stream",
    "jsorb_keyframe_database_last_error", "jsorb_keyframe_database_size", "jsorb_bow_vector_async", "jsorb_keyframe_database_add_async",
    "jsorb_keyframe_database_erase", "jsorb_keyframe_database_clear", "jsorb_keyframe_database_score_async", "jsorb_detect_loop_candidates_async",
    "jsorb_detect_relocalization_candidates_async", "jsorb_detect_loop_candidates", "jsorb_detect_relocalization_candidates",
    "jsorb_detect_candidates_stats", "jsorb_keyframe_database_copy_state", "jsorb_kfdb_build_caps",
    "jsorb_vocabulary_train", "jsorb_vocabulary_train_last_error", "jsorb_vocab_train_result_destroy", "jsorb_vocab_train_result_info",
    "jsorb_vocab_train_result_copy", "jsorb_vocab_train_result_copy_assignment", "jsorb_vocab_train_stats", "jsorb_vocab_train_build_caps",
    "jsorb_local_map_points_async", "jsorb_local_map_points", "jsorb_local_map_stats", "jsorb_local_map_build_caps", "jsorb_map_points_scatter_async",
    "jsorb_local_keyframes_async", "jsorb_local_keyframes", "jsorb_local_keyframes_stats", "jsorb_local_keyframes_build_caps",
    "jsorb_update_connections_async", "jsorb_update_connections", "jsorb_update_connections_stats", "jsorb_erase_connections_async",
    "jsorb_connected_mask_async", "jsorb_best_covisibles_async", "jsorb_covisibility_copy", "jsorb_covisibility_build_caps",
    "jsorb_update_connections_scratch",
    "jsorb_cull_keyframes_async", "jsorb_cull_keyframes", "jsorb_cull_keyframes_stats", "jsorb_cull_keyframes_build_caps",
    "jsorb_fuse_map_async", "jsorb_fuse_map", "jsorb_fuse_map_stats", "jsorb_fuse_map_build_caps",
    "jsorb_create_new_map_points_async", "jsorb_create_new_map_points", "jsorb_create_new_map_points_stats", "jsorb_create_new_map_points_build_caps",
    "jsorb_pose_optimization_async", "jsorb_pose_optimization", "jsorb_pose_optimization_stats", "jsorb_pose_optimization_build_caps",
    "jsorb_apply_matches_async",
]


# memory layout of cv::KeyPoint (jsorb_keypoint in include/jsorb.h)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class JsorbParams(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("n_levels", C.c_int), ("scale_factor", C.c_float),
                ("fast_n_min", C.c_int), ("fast_n_max", C.c_int), ("th_fast_min", C.c_int), ("th_fast_max", C.c_int),
                ("tile_h", C.c_int), ("tile_w", C.c_int), ("fixed_multi_scale_tile_size", C.c_int),
                ("apply_nms_ms", C.c_int), ("nms_ms_mode_gpu", C.c_int), ("device_id", C.c_int), ("max_batch", C.c_int)]


class JsorbStereoStats(C.Structure):
    _fields_ = [("n_left", C.c_int), ("n_right", C.c_int), ("n_candidate_pairs", C.c_int), ("n_corr_match", C.c_int),
                ("n_depth", C.c_int), ("n_final", C.c_int)]


class JsorbCamera(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class JsorbSearchParams(C.Structure):
    _fields_ = [("th", C.c_float), ("nn_ratio", C.c_float), ("th_high", C.c_int), ("mbf", C.c_float), ("min_x", C.c_float), ("min_y", C.c_float),
                ("inv_w", C.c_float), ("inv_h", C.c_float), ("cols", C.c_int), ("rows", C.c_int)]


class JsorbLastFrameParams(C.Structure):
    _fields_ = [("th", C.c_float), ("th_high", C.c_int), ("check_orientation", C.c_int), ("direction", C.c_int), ("retry_below", C.c_int)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h")] + \
               [("cols", C.c_int), ("rows", C.c_int), ("mbf", C.c_float), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3)]


def make_last_frame_params(Rcw, tcw, camera, bounds, grid, th=7.0, direction=0, mbf=0.0, check_orientation=True, retry_below=20, th_high=TH_HIGH,
                           cols=64, rows=48):
    """jsorb_last_frame_params: Rcw (3x3) and tcw (3) of CurrentFrame.mTcw as float32, camera = (fx, fy, cx, cy), bounds = (mnMinX, mnMaxX, mnMinY,
    mnMaxY), grid = (mfGridElementWidthInv, mfGridElementHeightInv) over cols x rows"""
    R = np.asarray(Rcw, np.float32).ravel()
    t = np.asarray(tcw, np.float32).ravel()
    assert R.size == 9 and t.size == 3
    return JsorbLastFrameParams(th, th_high, int(check_orientation), direction, retry_below, *camera, *bounds, *grid, cols, rows, mbf,
                                (C.c_float * 9)(*R.tolist()), (C.c_float * 3)(*t.tolist()))


class JsorbKfProjectionParams(C.Structure):
    _fields_ = [("th", C.c_float), ("orb_dist", C.c_int), ("check_orientation", C.c_int)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h")] + \
               [("cols", C.c_int), ("rows", C.c_int), ("log_scale_factor", C.c_float), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3)]


def make_kf_projection_params(Rcw, tcw, camera, bounds, grid, log_scale_factor, th=10.0, orb_dist=100, check_orientation=True, cols=64, rows=48, Ow=None):
    """jsorb_kf_projection_params: Rcw (3x3) and tcw (3) of CurrentFrame.mTcw as float32, camera = (fx, fy, cx, cy), bounds = (mnMinX, mnMaxX, mnMinY,
    mnMaxY), grid = (mfGridElementWidthInv, mfGridElementHeightInv) over cols x rows, log_scale_factor = mfLogScaleFactor.  Ow: the camera centre
    as float32 (None: -Rcw^T tcw computed in float32, ORBmatcher.cpp:1974)"""
    R = np.asarray(Rcw, np.float32).reshape(3, 3)
    t = np.asarray(tcw, np.float32).ravel()
    assert t.size == 3
    o = (-(R.T @ t)).astype(np.float32) if Ow is None else np.asarray(Ow, np.float32).ravel()
    assert o.size == 3
    return JsorbKfProjectionParams(th, orb_dist, int(check_orientation), *camera, *bounds, *grid, cols, rows, log_scale_factor,
                                   (C.c_float * 9)(*R.ravel().tolist()), (C.c_float * 3)(*t.tolist()), (C.c_float * 3)(*o.tolist()))


class JsorbInitParams(C.Structure):
    _fields_ = [("window", C.c_float), ("nn_ratio", C.c_float), ("th_low", C.c_int), ("check_orientation", C.c_int), ("min_x", C.c_float),
                ("min_y", C.c_float), ("inv_w", C.c_float), ("inv_h", C.c_float), ("cols", C.c_int), ("rows", C.c_int)]


def make_init_params(grid, window=50.0, nn_ratio=0.9, th_low=TH_LOW, check_orientation=True, cols=64, rows=48):
    """jsorb_init_params of MonocularInitialization's ORBmatcher(0.9, true) and windowSize 50: grid = (mnMinX, mnMinY, mfGridElementWidthInv,
    mfGridElementHeightInv) of the current frame over cols x rows"""
    return JsorbInitParams(window, nn_ratio, th_low, int(check_orientation), grid[0], grid[1], grid[2], grid[3], cols, rows)


class JsorbBowParams(C.Structure):
    _fields_ = [("nn_ratio", C.c_float), ("th_low", C.c_int), ("check_orientation", C.c_int)]


def make_bow_params(nn_ratio=0.7, th_low=TH_LOW, check_orientation=True):
    """jsorb_bow_params: ORBmatcher matcher(0.7, true) of TrackReferenceKeyFrame (Tracking.cpp:925), (0.75, true) of Relocalization (:1975)"""
    return JsorbBowParams(nn_ratio, th_low, int(check_orientation))


class JsorbTriangulationParams(C.Structure):
    _fields_ = [("th_low", C.c_int), ("check_orientation", C.c_int), ("only_stereo", C.c_int), ("n_levels", C.c_int),
                ("scale_factor", C.c_float * MAX_LEVELS), ("level_sigma2", C.c_float * MAX_LEVELS)]


def make_triangulation_params(scale_factor, level_sigma2=None, th_low=TH_LOW, check_orientation=True, only_stereo=False):
    """jsorb_triangulation_params: ORBmatcher matcher(0.6, false) of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:221) has
    check_orientation=False; scale_factor / level_sigma2 are the float tables mvScaleFactors / mvLevelSigma2 of the neighbours (level_sigma2 None:
    scale_factor squared in float32, ORBextractor.cpp:43-71)"""
    sf = np.ascontiguousarray(scale_factor, np.float32).ravel()
    s2 = (sf * sf).astype(np.float32) if level_sigma2 is None else np.ascontiguousarray(level_sigma2, np.float32).ravel()
    if len(s2) != len(sf):
        raise JsorbError("make_triangulation_params: scale_factor and level_sigma2 must have one entry per level")
    p = JsorbTriangulationParams(int(th_low), int(check_orientation), int(only_stereo), len(sf))
    for l in range(min(len(sf), MAX_LEVELS)):
        p.scale_factor[l] = sf[l]
        p.level_sigma2[l] = s2[l]
    return p


class JsorbFuseParams(C.Structure):
    _fields_ = [("th", C.c_float), ("th_low", C.c_int), ("check_reprojection", C.c_int)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h")] + \
               [("cols", C.c_int), ("rows", C.c_int), ("log_scale_factor", C.c_float), ("n_levels", C.c_int),
                ("scale_factor", C.c_float * MAX_LEVELS), ("inv_level_sigma2", C.c_float * MAX_LEVELS)]


def make_fuse_params(camera, bounds, grid, log_scale_factor, scale_factor, inv_level_sigma2=None, th=3.0, th_low=TH_LOW, check_reprojection=True,
                     bf=0.0, cols=64, rows=48):
    """jsorb_fuse_params: camera = (fx, fy, cx, cy) and bf = mbf of the keyframes, bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), grid =
    (mfGridElementWidthInv, mfGridElementHeightInv) over cols x rows, log_scale_factor = mfLogScaleFactor, scale_factor / inv_level_sigma2 the float
    tables mvScaleFactors / mvInvLevelSigma2 (None: 1.0f / (scale_factor squared) in float32, ORBextractor.cpp:43-71).  th = 3 and
    check_reprojection = True are LocalMapping::SearchInNeighbors' Fuse (ORBmatcher.cpp:812); th = 4 and False the loop-closing overload (:964)"""
    sf = np.ascontiguousarray(scale_factor, np.float32).ravel()
    i2 = (np.float32(1) / (sf * sf).astype(np.float32)).astype(np.float32) if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32).ravel()
    if len(i2) != len(sf):
        raise JsorbError("make_fuse_params: scale_factor and inv_level_sigma2 must have one entry per level")
    p = JsorbFuseParams(th, int(th_low), int(check_reprojection), *camera, bf, *bounds, *grid, cols, rows, log_scale_factor, len(sf))
    for l in range(min(len(sf), MAX_LEVELS)):
        p.scale_factor[l] = sf[l]
        p.inv_level_sigma2[l] = i2[l]
    return p


class JsorbSim3Params(C.Structure):
    _fields_ = [("th", C.c_float), ("th_high", C.c_int)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h")] + \
               [("cols", C.c_int), ("rows", C.c_int), ("log_scale_factor", C.c_float), ("n_levels", C.c_int), ("scale_factor", C.c_float * MAX_LEVELS)]


class JsorbSim3Side(C.Structure):
    _fields_ = [("n", C.c_int)] + [(k, C.c_void_p) for k in ("x", "y", "octave", "kp_desc", "Px", "Py", "Pz", "max_distance", "min_dist_inv",
                                                             "max_dist_inv", "mp_desc", "search")] + \
               [("Rw", C.c_float * 9), ("tw", C.c_float * 3), ("sR", C.c_float * 9), ("t", C.c_float * 3)]


def make_sim3_params(camera, bounds, grid, log_scale_factor, scale_factor, th=7.5, th_high=TH_HIGH, cols=64, rows=48):
    """jsorb_sim3_params of LoopClosing::ComputeSim3's SearchBySim3 (th = 7.5, ORBmatcher.cpp:1089): camera = (fx, fy, cx, cy) of pKF1 (it serves
    both directions), bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), grid = (mfGridElementWidthInv, mfGridElementHeightInv) over cols x rows,
    log_scale_factor = mfLogScaleFactor, scale_factor the float table mvScaleFactors"""
    sf = np.ascontiguousarray(scale_factor, np.float32).ravel()
    p = JsorbSim3Params(th, int(th_high), *camera, *bounds, *grid, cols, rows, log_scale_factor, len(sf))
    for l in range(min(len(sf), MAX_LEVELS)):
        p.scale_factor[l] = sf[l]
    return p


class JsorbScwParams(C.Structure):
    _fields_ = [("th", C.c_float), ("th_low", C.c_int)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h")] + \
               [("cols", C.c_int), ("rows", C.c_int), ("log_scale_factor", C.c_float), ("n_levels", C.c_int), ("scale_factor", C.c_float * MAX_LEVELS),
                ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3)]


def scw_from_pose(Scw):
    """Scw (4 x 4) decomposed in float32, term for term as ORBmatcher.cpp:286-290 does: scw = sqrt(row 0 of sRcw . itself) with the products
    summed left to right, Rcw = sRcw / scw, tcw = Scw's translation / scw, Ow = -Rcw^T tcw (each row: the products summed left to right, then the
    sign).  -> (Rcw float32[9] row-major, tcw float32[3], Ow float32[3])"""
    f = np.float32
    S = np.asarray(Scw, np.float32).reshape(4, 4)
    sR = S[:3, :3]
    scw = f(np.sqrt(f(f(f(sR[0, 0] * sR[0, 0]) + f(sR[0, 1] * sR[0, 1])) + f(sR[0, 2] * sR[0, 2]))))
    R = (sR / scw).astype(np.float32)
    t = (S[:3, 3] / scw).astype(np.float32)
    O = np.array([-f(f(f(R[0, c] * t[0]) + f(R[1, c] * t[1])) + f(R[2, c] * t[2])) for c in range(3)], np.float32)
    return R.ravel(), t, O


def scw_params(camera, bounds, grid, log_scale_factor, scale_factor, Rcw, tcw, Ow, th=10.0, th_low=TH_LOW, cols=64, rows=48):
    """jsorb_scw_params of LoopClosing::ComputeSim3's SearchByProjection(pKF, Scw, vpPoints, vpMatched, 10) (ORBmatcher.cpp:277): camera = (fx, fy,
    cx, cy) of pKF, bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), grid = (mfGridElementWidthInv, mfGridElementHeightInv) over cols x rows,
    log_scale_factor = mfLogScaleFactor, scale_factor the float table mvScaleFactors; Rcw (9, row-major), tcw (3), Ow (3) as scw_from_pose gives them"""
    sf = np.ascontiguousarray(scale_factor, np.float32).ravel()
    p = JsorbScwParams(th, int(th_low), *camera, *bounds, *grid, cols, rows, log_scale_factor, len(sf))
    for l in range(min(len(sf), MAX_LEVELS)):
        p.scale_factor[l] = sf[l]
    for name, v, size in (("Rcw", Rcw, 9), ("tcw", tcw, 3), ("Ow", Ow, 3)):
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        if len(v) != size:
            raise JsorbError("scw_params: %s must hold %d floats" % (name, size))
        setattr(p, name, (C.c_float * size)(*v.tolist()))
    return p


class JsorbMapPointTable(C.Structure):
    _fields_ = [("n_rows", C.c_int)] + [(k, C.c_void_p) for k in ("Px", "Py", "Pz", "Pnx", "Pny", "Pnz", "MaxDistance", "invariance_maxDistance",
                                                                 "invariance_minDistance", "desc", "bad")]


class JsorbFrustumParams(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3)] + [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")] + \
               [(k, C.c_int) for k in ("minX", "maxX", "minY", "maxY", "nScaleLevels")] + [("logScaleFactor", C.c_float), ("viewCosAngle", C.c_float)]


def make_frustum_params(Rcw, tcw, Ow, camera, bounds, n_levels, log_scale_factor, view_cos_angle=0.5):
    """jsorb_frustum_params, the host arguments of jsorb_is_in_frustum: Rcw (3x3), tcw (3) and Ow (3) as float32, camera = (fx, fy, cx, cy), bounds =
    (minX, maxX, minY, maxY) as ints, n_levels = nScaleLevels, log_scale_factor = mfLogScaleFactor, view_cos_angle = viewingCosLimit (0.5)"""
    R = np.asarray(Rcw, np.float32).ravel()
    t = np.asarray(tcw, np.float32).ravel()
    o = np.asarray(Ow, np.float32).ravel()
    assert R.size == 9 and t.size == 3 and o.size == 3
    return JsorbFrustumParams((C.c_float * 9)(*R.tolist()), (C.c_float * 3)(*t.tolist()), (C.c_float * 3)(*o.tolist()), *[float(x) for x in camera],
                               *[int(b) for b in bounds], int(n_levels), float(log_scale_factor), float(view_cos_angle))


# jsorb_map_point_record: what MapPointTable.scatter uploads per changed row
MAP_POINT_RECORD_DTYPE = np.dtype([("P", "<f4", 3), ("Pn", "<f4", 3), ("MaxDistance", "<f4"), ("invariance_maxDistance", "<f4"),
                                   ("invariance_minDistance", "<f4"), ("bad", "u1"), ("pad", "u1", 3)])
MAP_POINT_FLOATS = ("Px", "Py", "Pz", "Pnx", "Pny", "Pnz", "MaxDistance", "invariance_maxDistance", "invariance_minDistance")


class JsorbPoseParams(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "bf")] + [("inv_level_sigma2", C.c_float * 16)]


def make_pose_params(camera, bf, inv_level_sigma2):
    """jsorb_pose_params: camera = (fx, fy, cx, cy), bf = mbf, inv_level_sigma2 = mvInvLevelSigma2 (up to 16 floats, the rest 0)"""
    v = np.asarray(inv_level_sigma2, np.float32).ravel()
    if v.size > 16:
        raise JsorbError("make_pose_params: at most 16 levels")
    return JsorbPoseParams(*[float(x) for x in camera], float(bf), (C.c_float * 16)(*v.tolist()))


POSE_COUNTS = ("n_initial", "n_bad", "n_inliers", "rounds")
POSE_STATS = ("n_outside_rows", "n_mono", "n_stereo", "iterations", "trials", "rejected", "failed", "idle_rounds")


def apply_matches(point_row, match_kp, frame_point_row, stream_ptr=None, wait=True):
    """jsorb_apply_matches_async: frame_point_row[match_kp[i]] = point_row[i] wherever 0 <= match_kp[i] < N and point_row[i] >= 0, in place.  int32
    device tensors: point_row and match_kp of the same length (a matcher's point rows and its match_kp), frame_point_row[N].  stream_ptr None:
    the default stream, after the current torch stream has been waited for; wait: the call waits for its own work."""
    import torch
    n = int(match_kp.shape[0])
    a = _i32_ptr("apply_matches: point_row", point_row, n, flat=True)
    b = _i32_ptr("apply_matches: match_kp", match_kp, n, flat=True)
    f = _i32_ptr("apply_matches: frame_point_row", frame_point_row, flat=True)
    if stream_ptr is None:
        torch.cuda.current_stream(frame_point_row.device).synchronize()
    rc = load_library().jsorb_apply_matches_async(stream_ptr, n, a, b, int(frame_point_row.shape[0]), f)
    if rc:
        raise JsorbError("jsorb_apply_matches_async: error %d" % rc)
    if wait:
        torch.cuda.synchronize(frame_point_row.device)
    return frame_point_row


class MapPointTable:
    """The device table of map points jsorb_local_map_points reads (jsorb_map_point_table): nine float32[n_rows] arrays, desc uint8[n_rows, 32] and
    bad uint8[n_rows] as torch tensors it owns, rows chosen by the caller (the rows of desc_out in distinctive_descriptors, which may write
    `desc` in place).  scatter() writes the rows a local BA, UpdateNormalAndDepth or SetBadFlag changed."""

    def __init__(self, n_rows, device="cuda"):
        import torch
        self.n_rows = int(n_rows)
        n = max(self.n_rows, 1)
        self.floats = torch.zeros((9, n), dtype=torch.float32, device=device)
        self.desc = torch.zeros((n, 32), dtype=torch.uint8, device=device)
        self.bad = torch.zeros(n, dtype=torch.uint8, device=device)

    def struct(self):
        return JsorbMapPointTable(self.n_rows, *[self.floats[i].data_ptr() for i in range(9)], self.desc.data_ptr(), self.bad.data_ptr())

    def scatter(self, rows, records, stream_ptr=None, wait=True):
        """rows int32[n] (numpy or device tensor) and records MAP_POINT_RECORD_DTYPE[n] (numpy, or a uint8[n, 40] device tensor): one upload each, one
        kernel.  Rows outside the table are skipped."""
        import torch
        dev = self.floats.device
        if not hasattr(rows, "data_ptr"):
            rows = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(dev)
        if not hasattr(records, "data_ptr"):
            rec = np.ascontiguousarray(records, MAP_POINT_RECORD_DTYPE)
            records = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), MAP_POINT_RECORD_DTYPE.itemsize)).to(dev)
        n = int(rows.shape[0])
        if rows.dtype != torch.int32 or not rows.is_contiguous() or records.dtype != torch.uint8 or tuple(records.shape) != (n, 40) or not records.is_contiguous():
            raise JsorbError("MapPointTable.scatter: rows must be int32[n] and records %d bytes each" % MAP_POINT_RECORD_DTYPE.itemsize)
        if stream_ptr is None:
            torch.cuda.current_stream(dev).synchronize()
        rc = load_library().jsorb_map_points_scatter_async(stream_ptr, self.n_rows, *[self.floats[i].data_ptr() for i in range(9)], self.bad.data_ptr(), n,
                                                           rows.data_ptr(), records.data_ptr())
        if rc:
            raise JsorbError("jsorb_map_points_scatter_async: error %d" % rc)
        if wait:
            torch.cuda.synchronize(dev)


class JsorbKeyframeGraph(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("max_keyframes", "pool_entries", "child_entries")] + \
               [(k, C.c_void_p) for k in ("state", "order_key", "point_off", "point_len", "point_pool", "registered", "neighbours", "child_off", "child_len",
                                          "child_pool", "parent")]


KF_ABSENT, KF_GOOD, KF_BAD = 0, 1, 2             # jsorb_keyframe_graph.state
KF_NEIGHBOURS = 10                               # GetBestCovisibilityKeyFrames(10)
LOCAL_KF_MIN_CAPACITY = 84                       # the first list up to 80 and three more (Tracking.cpp:1898)
LOCAL_KF_COUNTS = ("n_counter", "n_first", "n_local", "ref_slot", "E_total", "kf_overflow", "entry_overflow", "kept_previous")


class KeyframeGraph:
    """The keyframes as jsorb_local_keyframes reads them (jsorb_keyframe_graph): torch device arrays over max_keyframes slots the caller chooses, as
    for KeyframeDatabase.  What the reference changes, and where it lands here: AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch -> the
    keyframe's run in point_pool (set_keyframe, or a write into point_pool at point_off[slot] + i); AddObservation / EraseObservation ->
    `registered`; UpdateBestCovisibles -> set_neighbours, or nothing where KeyframeMatcher.update_connections keeps `neighbours` current; AddChild / EraseChild / ChangeParent -> set_children, set_parent; SetBadFlag ->
    set_state(slot, KF_BAD), and for the keyframes KeyframeMatcher.cull_keyframes culls nothing: the call itself sets state, clears the
    keyframe's `registered` bytes and the observers' entries of the rows it turns bad, and repairs `parent` (with apply=True the child runs
    too); erase(slot) frees the slot.  Runs are handed out from the pools front to back; a run that still fits is rewritten
    in place, and a full pool is an error (the caller builds a new graph)."""
    ARRAYS = ("state", "order_key", "point_off", "point_len", "point_pool", "registered", "neighbours", "child_off", "child_len", "child_pool", "parent")

    def __init__(self, max_keyframes, pool_entries, child_entries, device="cuda"):
        import torch
        self.max_keyframes, self.pool_entries, self.child_entries = int(max_keyframes), int(pool_entries), int(child_entries)
        S, Pn, Cn = max(self.max_keyframes, 1), max(self.pool_entries, 1), max(self.child_entries, 1)
        z = lambda n, dt, fill=0: torch.full((n,), fill, dtype=dt, device=device)
        self.state, self.order_key = z(S, torch.uint8), z(S, torch.int64)
        self.point_off, self.point_len, self.point_pool, self.registered = z(S, torch.int32), z(S, torch.int32), z(Pn, torch.int32, -1), z(Pn, torch.uint8, 1)
        self.neighbours = torch.full((S, KF_NEIGHBOURS), -1, dtype=torch.int32, device=device)
        self.child_off, self.child_len, self.child_pool, self.parent = z(S, torch.int32), z(S, torch.int32), z(Cn, torch.int32, -1), z(S, torch.int32, -1)
        self._run = {"point": {}, "child": {}}     # slot -> (offset, entries reserved)
        self._used = {"point": 0, "child": 0}

    def struct(self):
        """(`registered` may be set to None: every entry then counts as registered)"""
        ptr = [None if getattr(self, k) is None else getattr(self, k).data_ptr() for k in self.ARRAYS]
        return JsorbKeyframeGraph(self.max_keyframes, self.pool_entries, self.child_entries, *ptr)

    def load(self, **arrays):
        """whole arrays at once (numpy, the layouts of jsorb_keyframe_graph); the setters then rewrite the loaded runs in place
        and hand out new ones behind the largest run end"""
        import torch
        for k, v in arrays.items():
            if k not in self.ARRAYS:
                raise JsorbError("KeyframeGraph.load: no array %s" % k)
            t = getattr(self, k)
            v = torch.from_numpy(np.ascontiguousarray(v)).to(t.device)
            if v.dtype != t.dtype or v.numel() > t.numel():
                raise JsorbError("KeyframeGraph.load: %s must be %s with at most %d entries" % (k, t.dtype, t.numel()))
            t.view(-1)[:v.numel()].copy_(v.view(-1))
        for kind, off, ln, total in (("point", self.point_off, self.point_len, self.pool_entries), ("child", self.child_off, self.child_len, self.child_entries)):
            o, n = off.cpu().numpy().astype(np.int64)[:self.max_keyframes], ln.cpu().numpy().astype(np.int64)[:self.max_keyframes]
            ok = (o >= 0) & (n >= 0) & (o + n <= total)
            self._run[kind] = {int(s): (int(o[s]), int(n[s])) for s in np.nonzero(ok)[0]}
            self._used[kind] = int((o + n)[ok].max()) if ok.any() else 0

    def _slot(self, slot):
        if not 0 <= int(slot) < self.max_keyframes:
            raise JsorbError("KeyframeGraph: slot %d outside [0, %d)" % (slot, self.max_keyframes))
        return int(slot)

    def _write_run(self, kind, slot, values, pool, off, length, total):
        import torch
        n = len(values)
        at, room = self._run[kind].get(slot, (0, -1))
        if n > room:
            at, room = self._used[kind], n
            if at + n > total:
                raise JsorbError("KeyframeGraph: the %s pool is full (%d of %d entries used, %d wanted)" % (kind, at, total, n))
            self._used[kind] += n
            self._run[kind][slot] = (at, room)
        if n:
            pool[at:at + n] = torch.from_numpy(values).to(pool.device)
        off[slot], length[slot] = at, n
        return at

    def set_keyframe(self, slot, rows, key, state=KF_GOOD, registered=None):
        """GetMapPointMatches() of the keyframe as table rows (-1 = NULL), its place in std::map<KeyFrame*, int> ((intptr_t)pKF in the binding), its
        state, and per entry whether the point holds the keyframe in its observations (None: all do)"""
        import torch
        slot = self._slot(slot)
        rows = np.ascontiguousarray(rows, np.int32).ravel()
        at = self._write_run("point", slot, rows, self.point_pool, self.point_off, self.point_len, self.pool_entries)
        if len(rows) and self.registered is not None:
            reg = np.ones(len(rows), np.uint8) if registered is None else np.ascontiguousarray(registered, np.uint8).ravel()
            if len(reg) != len(rows):
                raise JsorbError("KeyframeGraph.set_keyframe: one registered byte per row")
            self.registered[at:at + len(rows)] = torch.from_numpy(reg).to(self.registered.device)
        self.order_key[slot] = int(key)
        self.state[slot] = int(state)

    def set_state(self, slot, state):
        self.state[self._slot(slot)] = int(state)

    def set_neighbours(self, slot, slots):
        import torch
        row = np.full(KF_NEIGHBOURS, -1, np.int32)
        v = np.asarray(slots, np.int32).ravel()[:KF_NEIGHBOURS]
        row[:len(v)] = v
        self.neighbours[self._slot(slot)] = torch.from_numpy(row).to(self.neighbours.device)

    def set_children(self, slot, slots):
        """GetChilds() as slots in std::set<KeyFrame*> order"""
        slot = self._slot(slot)
        self._write_run("child", slot, np.ascontiguousarray(slots, np.int32).ravel(), self.child_pool, self.child_off, self.child_len, self.child_entries)

    def set_parent(self, slot, parent):
        self.parent[self._slot(slot)] = -1 if parent is None else int(parent)

    def erase(self, slot):
        slot = self._slot(slot)
        self.state[slot], self.point_len[slot], self.child_len[slot], self.parent[slot] = KF_ABSENT, 0, 0, -1
        self.neighbours[slot] = -1


class JsorbCovisibility(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("max_keyframes", "conn_capacity")] + \
               [(k, C.c_void_p) for k in ("conn_len", "conn_slot", "conn_weight", "ord_len", "ord_slot", "ord_weight", "first_connection")]


class JsorbConnSnapshot(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("slot", "weight", "len")]


UPDATE_CONNECTIONS_MAX = 32                      # keyframes per jsorb_update_connections call
UPDATE_CONNECTIONS_COUNTS = ("n_processed", "n_skipped", "n_empty", "n_add_connection", "n_resorted", "n_fallback", "n_overflow")


class Covisibility:
    """The covisibility graph as jsorb_update_connections keeps it (jsorb_covisibility): torch device arrays over the max_keyframes slots of a
    KeyframeGraph, conn_capacity entries per slot.  conn_*: mConnectedKeyFrameWeights in (order_key, slot) order; ord_*:
    mvpOrderedConnectedKeyFrames / mvOrderedWeights; first_connection: mbFirstConnection && mnId != 0 (created(slot) sets it).  The getters copy
    one slot to the host (jsorb_covisibility_copy) and wait for the device."""
    ARRAYS = ("conn_len", "conn_slot", "conn_weight", "ord_len", "ord_slot", "ord_weight", "first_connection")

    def __init__(self, max_keyframes, conn_capacity, device="cuda"):
        import torch
        self.max_keyframes, self.conn_capacity = int(max_keyframes), int(conn_capacity)
        lo, hi = covisibility_build_caps()
        if not lo <= self.conn_capacity <= hi:
            raise JsorbError("Covisibility: conn_capacity must be in [%d, %d]" % (lo, hi))
        S, Cn = max(self.max_keyframes, 1), self.conn_capacity
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
        self.conn_len, self.conn_slot, self.conn_weight = z(S), z(S, Cn), z(S, Cn)
        self.ord_len, self.ord_slot, self.ord_weight = z(S), z(S, Cn), z(S, Cn)
        self.first_connection = torch.zeros(S, dtype=torch.uint8, device=device)

    def struct(self):
        return JsorbCovisibility(self.max_keyframes, self.conn_capacity, *[getattr(self, k).data_ptr() for k in self.ARRAYS])

    def load(self, **arrays):
        """whole arrays at once (numpy, the layouts of jsorb_covisibility)"""
        import torch
        for k, v in arrays.items():
            if k not in self.ARRAYS:
                raise JsorbError("Covisibility.load: no array %s" % k)
            t = getattr(self, k)
            v = torch.from_numpy(np.ascontiguousarray(v)).to(t.device)
            if v.dtype != t.dtype or v.shape != t.shape:
                raise JsorbError("Covisibility.load: %s must be %s of shape %s" % (k, t.dtype, tuple(t.shape)))
            t.copy_(v)

    def arrays(self):
        """every array on the host (numpy)"""
        return {k: getattr(self, k).cpu().numpy() for k in self.ARRAYS}

    def created(self, slot, first_keyframe=False):
        """a new keyframe in `slot`: empty map and lists, first_connection = 1 unless it is the map's first keyframe"""
        if not 0 <= int(slot) < self.max_keyframes:
            raise JsorbError("Covisibility: slot %d outside [0, %d)" % (slot, self.max_keyframes))
        self.conn_len[slot], self.ord_len[slot], self.first_connection[slot] = 0, 0, 0 if first_keyframe else 1

    def _copy(self, slot):
        Cn = self.conn_capacity
        lens = np.zeros(2, np.int32)
        a = [np.zeros(Cn, np.int32) for _ in range(4)]
        st = self.struct()
        rc = load_library().jsorb_covisibility_copy(C.byref(st), int(slot), lens.ctypes.data, *[x.ctypes.data for x in a])
        if rc != 0:
            raise JsorbError("jsorb_covisibility_copy rc=%d" % rc)
        nc, no = (int(min(max(v, 0), Cn)) for v in lens)
        return a[0][:nc], a[1][:nc], a[2][:no], a[3][:no]

    def ordered(self, slot):
        """GetVectorCovisibleKeyFrames(): the ordered list's slots"""
        return self._copy(slot)[2]

    def weights(self, slot):
        """mvOrderedWeights"""
        return self._copy(slot)[3]

    def connected(self, slot):
        """GetConnectedKeyFrames(): the map's slots in (order_key, slot) order"""
        return self._copy(slot)[0]

    def weight(self, slot, other):
        """GetWeight(pKF) (KeyFrame.cpp:205-212): 0 when the map does not hold it"""
        cs, cw, _, _ = self._copy(slot)
        hit = np.nonzero(cs == int(other))[0]
        return int(cw[hit[0]]) if len(hit) else 0

    def best(self, slot, N):
        """GetBestCovisibilityKeyFrames(N) (KeyFrame.cpp:178-186)"""
        return self._copy(slot)[2][:max(int(N), 0)]

    def by_weight(self, slot, w):
        """GetCovisiblesByWeight(w) (KeyFrame.cpp:188-203): upper_bound over the descending weights with weightComp (a > b) - the entries whose
        weight is at least w, and, as the reference has it, an EMPTY list when every weight is (it == end)"""
        _, _, os_, ow = self._copy(slot)
        if len(os_) == 0:
            return os_
        n = int(np.count_nonzero(ow >= int(w)))          # upper_bound(first, last, w, a > b): the first element with w > element
        return os_[:0] if n == len(ow) else os_[:n]


class JsorbKeyframeViews(C.Structure):
    _fields_ = [("pool_entries", C.c_int)] + [(k, C.c_void_p) for k in ("octave", "stereo", "depth", "th_depth")]


class JsorbCullingState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("state", "registered", "bad", "point_pool", "parent", "not_erase", "to_be_erased", "ref_slot")]


CULL_MAX = 16                                    # keyframes culled per jsorb_cull_keyframes call
CULL_COUNTS = ("next", "n_kept", "n_culled", "n_deferred", "n_skipped", "n_rows_bad", "n_observations_erased", "n_ref_moved", "n_reparent",
               "reparent_overflow")
CULL_KEPT, CULL_CULLED, CULL_DEFERRED, CULL_SKIPPED, CULL_NOT_REACHED = 0, 1, 2, 3, -1      # decision[i]


class KeyframeViews:
    """What LocalMapping::KeyFrameCulling reads of a keyframe's keypoints (jsorb_keyframe_views): torch device arrays parallel to a
    KeyframeGraph's point_pool - octave uint8 (mvKeysUn[i].octave), stereo uint8 (mvuRight[i] >= 0), depth float32 (mvDepth[i]; None for a
    monocular map) - and th_depth float32[max_keyframes] (mThDepth)."""

    def __init__(self, graph, depth=True):
        import torch
        dev = graph.point_pool.device
        self.pool_entries, self.max_keyframes = graph.pool_entries, graph.max_keyframes
        n = max(self.pool_entries, 1)
        self.octave = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.stereo = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.depth = torch.zeros(n, dtype=torch.float32, device=dev) if depth else None
        self.th_depth = torch.zeros(max(self.max_keyframes, 1), dtype=torch.float32, device=dev)

    def struct(self):
        return JsorbKeyframeViews(self.pool_entries, self.octave.data_ptr(), self.stereo.data_ptr(), None if self.depth is None else self.depth.data_ptr(),
                                  self.th_depth.data_ptr())

    def load(self, **arrays):
        """whole arrays at once (numpy): octave, stereo, depth, th_depth"""
        import torch
        for k, v in arrays.items():
            t = getattr(self, k, None) if k in ("octave", "stereo", "depth", "th_depth") else None
            if t is None:
                raise JsorbError("KeyframeViews.load: no array %s" % k)
            v = torch.from_numpy(np.ascontiguousarray(v)).to(t.device)
            if v.dtype != t.dtype or v.numel() > t.numel():
                raise JsorbError("KeyframeViews.load: %s must be %s with at most %d entries" % (k, t.dtype, t.numel()))
            t.view(-1)[:v.numel()].copy_(v.view(-1))

    def set_keyframe_views(self, graph, slot, octave, stereo, depth=None, th_depth=0.0):
        """the views of the keyframe in `slot`, written at its run (after graph.set_keyframe)"""
        set_keyframe_views(graph, self, slot, octave, stereo, depth, th_depth)


def set_keyframe_views(graph, views, slot, octave, stereo, depth=None, th_depth=0.0):
    """the views of the keyframe in `slot`, written at its run in the graph's point_pool (after graph.set_keyframe): one entry per entry of the run"""
    import torch
    slot = graph._slot(slot)
    at, n = int(graph.point_off[slot]), int(graph.point_len[slot])
    for name, v, dt in (("octave", octave, np.uint8), ("stereo", stereo, np.uint8), ("depth", depth, np.float32)):
        t = getattr(views, name)
        if t is None or v is None:
            if name != "depth" or (t is not None and v is None):
                raise JsorbError("set_keyframe_views: %s is missing" % name)
            continue
        v = np.ascontiguousarray(v, dt).ravel()
        if len(v) != n:
            raise JsorbError("set_keyframe_views: %s must have the run's %d entries" % (name, n))
        if n:
            t[at:at + n] = torch.from_numpy(v).to(t.device)
    views.th_depth[slot] = float(th_depth)


def culling_state(graph, table, not_erase=None, to_be_erased=None, ref_slot=None):
    """jsorb_culling_state: the graph's and the table's arrays as the writable pointers jsorb_cull_keyframes takes, with not_erase /
    to_be_erased uint8[max_keyframes] and ref_slot int32[n_rows] device tensors (or None).  The caller keeps the tensors alive."""
    import torch
    if graph.registered is None:
        raise JsorbError("culling_state: the graph has no registered bytes (the call writes them)")
    for name, t, dt, n in (("not_erase", not_erase, torch.uint8, graph.max_keyframes), ("to_be_erased", to_be_erased, torch.uint8, graph.max_keyframes),
                           ("ref_slot", ref_slot, torch.int32, table.n_rows)):
        if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() < n):
            raise JsorbError("culling_state: %s must be a contiguous %s device tensor of at least %d entries" % (name, dt, n))
    if not_erase is not None and to_be_erased is None:
        raise JsorbError("culling_state: not_erase needs to_be_erased")
    p = lambda t: None if t is None else t.data_ptr()
    return JsorbCullingState(graph.state.data_ptr(), graph.registered.data_ptr(), table.bad.data_ptr(), graph.point_pool.data_ptr(), graph.parent.data_ptr(),
                             p(not_erase), p(to_be_erased), p(ref_slot))


class JsorbKeyframeKeypoints(C.Structure):
    _fields_ = [("pool_entries", C.c_int)] + [(k, C.c_void_p) for k in ("x", "y", "octave", "uright", "desc")]


class JsorbFuseState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("point_pool", "registered", "bad", "desc", "replaced", "visible", "found")]


FUSE_MAP_COUNTS = ("n_fused", "n_replace", "n_add", "n_bad_in_slot", "n_rows_bad", "n_descriptors_changed", "n_skipped_targets", "n_dropped", "n_log",
                   "log_overflow")
FUSE_MAP_OUTPUTS = ("best_idx", "best_dist", "replace_point", "n_fused", "log", "counts")
EV_REPLACE, EV_ADD_MAP_POINT = 2, 3              # the codes of fuse_map's log records: (2, p, q, -1), (3, row, slot, keypoint)


class KeyframeKeypoints:
    """What ORBmatcher::Fuse reads of the keyframes' keypoints (jsorb_keyframe_keypoints): torch device arrays parallel to a KeyframeGraph's
    point_pool - x, y float32 (mvKeysUn), octave int32, uright float32 (mvuRight; None for a monocular map), desc uint8[., 32]."""
    ARRAYS = ("x", "y", "octave", "uright", "desc")

    def __init__(self, graph, stereo=True):
        import torch
        dev = graph.point_pool.device
        self.pool_entries = graph.pool_entries
        n = max(self.pool_entries, 1)
        self.x = torch.zeros(n, dtype=torch.float32, device=dev)
        self.y = torch.zeros(n, dtype=torch.float32, device=dev)
        self.octave = torch.zeros(n, dtype=torch.int32, device=dev)
        self.uright = torch.full((n,), -1.0, dtype=torch.float32, device=dev) if stereo else None
        self.desc = torch.zeros((n, 32), dtype=torch.uint8, device=dev)

    def struct(self):
        return JsorbKeyframeKeypoints(self.pool_entries, self.x.data_ptr(), self.y.data_ptr(), self.octave.data_ptr(),
                                      None if self.uright is None else self.uright.data_ptr(), self.desc.data_ptr())

    def load(self, **arrays):
        """whole arrays at once (numpy): x, y, octave, uright, desc"""
        import torch
        for k, v in arrays.items():
            t = getattr(self, k, None) if k in self.ARRAYS else None
            if t is None:
                raise JsorbError("KeyframeKeypoints.load: no array %s" % k)
            v = torch.from_numpy(np.ascontiguousarray(v)).to(t.device)
            if v.dtype != t.dtype or v.numel() > t.numel():
                raise JsorbError("KeyframeKeypoints.load: %s must be %s with at most %d entries" % (k, t.dtype, t.numel()))
            t.view(-1)[:v.numel()].copy_(v.view(-1))

    def set_keyframe(self, graph, slot, x, y, octave, desc, uright=None):
        """the keypoints of the keyframe in `slot`, written at its run (after graph.set_keyframe): one entry per entry of the run"""
        import torch
        slot = graph._slot(slot)
        at, n = int(graph.point_off[slot]), int(graph.point_len[slot])
        for name, v, dt in (("x", x, np.float32), ("y", y, np.float32), ("octave", octave, np.int32), ("uright", uright, np.float32), ("desc", desc, np.uint8)):
            t = getattr(self, name)
            if t is None or v is None:
                if name != "uright" or (t is None and v is not None):
                    raise JsorbError("KeyframeKeypoints.set_keyframe: %s is missing" % name)
                v = np.full(n, -1.0, np.float32)     # (a monocular keyframe in a stereo map)
                if t is None:
                    continue
            v = np.ascontiguousarray(v, dt).reshape((n, 32) if name == "desc" else (-1,))
            if len(v) != n:
                raise JsorbError("KeyframeKeypoints.set_keyframe: %s must have the run's %d entries" % (name, n))
            if n:
                t[at:at + n] = torch.from_numpy(v).to(t.device)


def fuse_state(graph, table, replaced=None, visible=None, found=None):
    """jsorb_fuse_state: the graph's point_pool / registered and the table's bad / desc as the writable pointers jsorb_fuse_map takes, with
    replaced, visible, found int32[n_rows] device tensors (or None; visible and found both or neither).  The caller keeps the tensors alive."""
    import torch
    if graph.registered is None:
        raise JsorbError("fuse_state: the graph has no registered bytes (the call writes them)")
    for name, t in (("replaced", replaced), ("visible", visible), ("found", found)):
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() < table.n_rows):
            raise JsorbError("fuse_state: %s must be a contiguous int32 device tensor of at least %d entries" % (name, table.n_rows))
    if (visible is None) != (found is None):
        raise JsorbError("fuse_state: visible and found go together")
    p = lambda t: None if t is None else t.data_ptr()
    return JsorbFuseState(graph.point_pool.data_ptr(), graph.registered.data_ptr(), table.bad.data_ptr(), table.desc.data_ptr(), p(replaced), p(visible), p(found))


class JsorbNewPointKeypoints(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("node", "depth", "raw_x", "raw_y", "cos_stereo")]


class JsorbNewPointState(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("point_pool", "registered", "bad", "desc") + MAP_POINT_FLOATS[:6] +
                ("MaxDistance", "invariance_maxDistance", "invariance_minDistance", "ref_slot", "replaced", "visible", "found", "first_kf_id")]


# jsorb_keyframe_pose: what create_new_map_points takes per keyframe, the current one first (make_keyframe_pose)
KEYFRAME_POSE_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3)] +
                               [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")])
NEW_POINTS_COUNTS = ("n_matches", "n_accepted", "n_owning", "n_created", "n_shared_kf2", "n_no_row", "n_taken", "n_skipped_neighbours", "log_overflow",
                     "n_svd", "n_unprojected", "no_current")
NEW_POINTS_OUTPUTS = ("verdict", "path", "x3D", "log", "counts")
# the verdict codes of create_new_map_points, one per exit of LocalMapping.cpp:297-437
NEW_POINTS_VERDICTS = ("no_match", "created", "taken", "low_parallax", "w_zero", "z1", "z2", "reprojection1", "reprojection2", "zero_distance",
                       "scale_ratio", "no_row", "empty_unprojection", "skipped_neighbour")
NP_PATH_NONE, NP_PATH_SVD, NP_PATH_UNPROJECT1, NP_PATH_UNPROJECT2 = 0, 1, 2, 3


def make_keyframe_pose(Rcw, tcw, camera, mb=0.0, mbf=0.0, Ow=None):
    """one jsorb_keyframe_pose record (KEYFRAME_POSE_DTYPE): Rcw (3x3) and tcw (3) as float32, camera = (fx, fy, cx, cy), mb and mbf the keyframe's.
    invfx, invfy = 1.0f / fx, 1.0f / fy (Frame.cpp); Ow = -Rcw^T tcw in float32 summed left to right unless given (KeyFrame::SetPose)"""
    R = np.asarray(Rcw, np.float32).reshape(3, 3)
    t = np.asarray(tcw, np.float32).reshape(3)
    if Ow is None:
        Ow = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)], np.float32)
    fx, fy, cx, cy = (np.float32(v) for v in camera)
    rec = np.zeros((), KEYFRAME_POSE_DTYPE)
    rec["Rcw"], rec["tcw"], rec["Ow"] = R.ravel(), t, np.asarray(Ow, np.float32).reshape(3)
    rec["fx"], rec["fy"], rec["cx"], rec["cy"] = fx, fy, cx, cy
    rec["invfx"], rec["invfy"], rec["mb"], rec["mbf"] = np.float32(1) / fx, np.float32(1) / fy, np.float32(mb), np.float32(mbf)
    return rec


class NewPointKeypoints:
    """What CreateNewMapPoints reads of the keyframes' keypoints beyond KeyframeKeypoints (jsorb_new_point_keypoints): torch device arrays parallel
    to a KeyframeGraph's point_pool - node int32 (the mFeatVec node, -1: none), depth float32 (mvDepth), cos_stereo float32 (cos(2*atan2(mb/2,
    depth)) from the host's libm), raw_x / raw_y float32 (mvKeys; raw=False: the undistorted points are used)."""
    ARRAYS = ("node", "depth", "raw_x", "raw_y", "cos_stereo")

    def __init__(self, graph, stereo=True, raw=True):
        import torch
        dev = graph.point_pool.device
        n = max(graph.pool_entries, 1)
        self.node = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.depth, self.cos_stereo = ((torch.full((n,), v, dtype=torch.float32, device=dev) if stereo else None) for v in (-1.0, 1.0))
        self.raw_x, self.raw_y = ((torch.zeros(n, dtype=torch.float32, device=dev) if raw else None) for _ in range(2))

    def struct(self):
        return JsorbNewPointKeypoints(*[None if getattr(self, k) is None else getattr(self, k).data_ptr() for k in self.ARRAYS])

    def load(self, **arrays):
        """whole arrays at once (numpy)"""
        import torch
        for k, v in arrays.items():
            t = getattr(self, k, None) if k in self.ARRAYS else None
            if t is None:
                raise JsorbError("NewPointKeypoints.load: no array %s" % k)
            v = torch.from_numpy(np.ascontiguousarray(v)).to(t.device)
            if v.dtype != t.dtype or v.numel() > t.numel():
                raise JsorbError("NewPointKeypoints.load: %s must be %s with at most %d entries" % (k, t.dtype, t.numel()))
            t.view(-1)[:v.numel()].copy_(v.view(-1))


def new_point_state(graph, table, ref_slot=None, replaced=None, visible=None, found=None, first_kf_id=None):
    """jsorb_new_point_state: the graph's point_pool / registered and the table's arrays as the writable pointers jsorb_create_new_map_points takes,
    with ref_slot, replaced, visible, found, first_kf_id int32[n_rows] device tensors (or None; visible and found both or neither).  The caller
    keeps the tensors alive."""
    import torch
    if graph.registered is None:
        raise JsorbError("new_point_state: the graph has no registered bytes (the call writes them)")
    side = (("ref_slot", ref_slot), ("replaced", replaced), ("visible", visible), ("found", found), ("first_kf_id", first_kf_id))
    for name, t in side:
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() < table.n_rows):
            raise JsorbError("new_point_state: %s must be a contiguous int32 device tensor of at least %d entries" % (name, table.n_rows))
    if (visible is None) != (found is None):
        raise JsorbError("new_point_state: visible and found go together")
    return JsorbNewPointState(graph.point_pool.data_ptr(), graph.registered.data_ptr(), table.bad.data_ptr(), table.desc.data_ptr(),
                              *[table.floats[i].data_ptr() for i in range(9)], *[None if t is None else t.data_ptr() for _, t in side])


def make_camera(K, D):
    """jsorb_camera from Tracking's mK (3x3) and mDistCoef (k1, k2, p1, p2[, k3]) - both taken as float32, as the reference stores them (Tracking.cpp:80-91)"""
    K = np.asarray(K, np.float32)
    D = np.asarray(D, np.float32).ravel()
    assert K.shape == (3, 3) and D.size in (4, 5)
    k3 = D[4] if D.size == 5 else np.float32(0)
    return JsorbCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], D[0], D[1], D[2], D[3], k3)


class JsorbError(RuntimeError):
    pass


_lib = None
_libs_by_path = {}


def load_library(path=None):
    """dlopen libjsorb.so (the in-tree build).  Raises if it has not been built: there is no fallback path.
    With an explicit path: another build of the same ABI (jetson_slam_amd/build.py VARIANTS), loaded next to the default one and returned
    without replacing it - tests that need it swap the module's `_lib` for their duration."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    explicit = path is not None
    path = path or os.environ.get("JSORB_LIBRARY") or _LIB_PATH      # JSORB_LIBRARY: an alternative build of the same ABI
    if path in _libs_by_path:
        if not explicit:
            _lib = _libs_by_path[path]
        return _libs_by_path[path]
    if not os.path.exists(path):
        raise JsorbError("%s not found - run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)" % path)
    lib = C.CDLL(path)
    P, I, F = C.c_void_p, C.c_int, C.c_float
    sig = {
        "jsorb_create": (I, [C.POINTER(JsorbParams), P, C.POINTER(P)]),
        "jsorb_create_masked": (I, [C.POINTER(JsorbParams), P, I, I, C.POINTER(P)]),
        "jsorb_destroy": (None, [P]),
        "jsorb_last_error": (C.c_char_p, [P]),
        "jsorb_version": (C.c_char_p, []),
        "jsorb_plan_launch": (I, [C.POINTER(JsorbParams), P, I]),
        "jsorb_extract": (I, [P, P, I, C.POINTER(I)]),
        "jsorb_extract_into": (I, [P, P, I, C.POINTER(I), P, P]),
        "jsorb_extract_device": (I, [P, P, I, C.POINTER(I)]),
        "jsorb_extract_batch_device_async": (I, [P, P, C.c_size_t, I, I]),
        "jsorb_extract_batch_host_async": (I, [P, P, C.c_size_t, I, I]),
        "jsorb_sync": (I, [P]),
        "jsorb_n_images": (I, [P]),
        "jsorb_n_keypoints": (I, [P, I]),
        "jsorb_level_n_keypoints": (I, [P, I, I]),
        "jsorb_keypoints_device": (P, [P, I]),
        "jsorb_descriptors_device": (P, [P, I]),
        "jsorb_copy_keypoints": (I, [P, I, P]),
        "jsorb_copy_descriptors": (I, [P, I, P]),
        "jsorb_n_levels": (I, [P]),
        "jsorb_level_dims": (I, [P, I, C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
        "jsorb_level_tiles": (I, [P, I, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
        "jsorb_total_tiles": (I, [P]),
        "jsorb_scale": (F, [P, I]),
        "jsorb_inv_scale": (F, [P, I]),
        "jsorb_level_image_device": (P, [P, I, I, I]),
        "jsorb_copy_level_image": (I, [P, I, I, I, P]),
        "jsorb_copy_level_mask": (I, [P, I, P]),
        "jsorb_read_mask_image": (I, [C.c_char_p, C.POINTER(I), C.POINTER(I), P, C.c_size_t]),
        "jsorb_mask_image_last_error": (C.c_char_p, []),
        "jsorb_copy_tile_candidates": (I, [P, I, P, P, P]),
        "jsorb_copy_angles": (I, [P, I, P]),
        "jsorb_stereo_match": (I, [P, P, F, F, I, I, P, P, C.POINTER(JsorbStereoStats)]),
        "jsorb_stereo_match_batch_async": (I, [P, P, F, F, I, I]),
        "jsorb_stereo_uright_device": (P, [P, I]),
        "jsorb_stereo_depth_device": (P, [P, I]),
        "jsorb_copy_stereo": (I, [P, I, P, P, C.POINTER(JsorbStereoStats)]),
        "jsorb_gather_counts_async": (I, [P, P, P]),
        "jsorb_copy_stereo_l1": (I, [P, I, P]),
        "jsorb_set_stereo_diagnostics": (I, [P, I]),
        "jsorb_copy_stereo_diagnostics": (I, [P, I, P]),
        "jsorb_set_speculative_stereo": (I, [P, I]),
        "jsorb_speculative_stereo_stats": (I, [P, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "jsorb_set_stream": (I, [P, P]),
        "jsorb_get_stream": (P, [P]),
        "jsorb_stream_wait_done": (I, [P, P]),
        "jsorb_enable_kernel_timing": (I, [P, I]),
        "jsorb_kernel_time": (I, [P, I, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
        "jsorb_reset_kernel_timing": (I, [P]),
        "jsorb_kernel_name": (C.c_char_p, [I]),
        "jsorb_project_points": (I, [P, I] + [P] * 5 + [F] * 8 + [P] * 4),
        "jsorb_hamming_pairs": (I, [P, I] + [P] * 5),
        "jsorb_is_in_frustum": (I, [P, I] + [P] * 12 + [F] * 4 + [I] * 5 + [F] * 2 + [P] * 6),
        "jsorb_unpack_frame": (I, [P, I, P, P]),
        "jsorb_assign_features_to_grid": (I, [P, I] + [F] * 4 + [I] * 2 + [P] * 2),
        "jsorb_set_rectify_maps": (I, [P, P, P, I, I, I]),
        "jsorb_set_rectify_maps_fixed": (I, [P, P, P, I, I, I, I]),
        "jsorb_clear_rectify_maps": (I, [P]),
        "jsorb_rectify_enabled": (I, [P]),
        "jsorb_rectify_convert_maps": (I, [P, P, I, P, P]),
        "jsorb_set_camera": (I, [P, C.POINTER(JsorbCamera)]),
        "jsorb_camera_enabled": (I, [P]),
        "jsorb_image_bounds": (I, [C.POINTER(JsorbCamera), I, I, P]),
        "jsorb_keypoints_un_device": (P, [P, I]),
        "jsorb_copy_keypoints_un": (I, [P, I, P]),
        "jsorb_unpack_frame_un": (I, [P, I, P, P, P]),
        "jsorb_rgbd_depth": (I, [P, P, I, C.c_size_t, F, F, P, P]),
        "jsorb_rgbd_depth_batch_device_async": (I, [P, P, C.c_size_t, C.c_size_t, I, F, F, I]),
        "jsorb_rgbd_uright_device": (P, [P, I]),
        "jsorb_rgbd_depth_device": (P, [P, I]),
        "jsorb_copy_rgbd": (I, [P, I, P, P]),
        "jsorb_search_local_points_async": (I, [P, I, C.POINTER(JsorbSearchParams), I] + [P] * 13),
        "jsorb_search_local_points": (I, [P, I, C.POINTER(JsorbSearchParams), I] + [P] * 9 + [P, C.POINTER(I)]),
        "jsorb_search_local_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
        "jsorb_search_last_frame_async": (I, [P, I, C.POINTER(JsorbLastFrameParams), I] + [P] * 11),
        "jsorb_search_last_frame": (I, [P, I, C.POINTER(JsorbLastFrameParams), I] + [P] * 7 + [P, C.POINTER(I)]),
        "jsorb_search_last_frame_stats": (I, [P, C.POINTER(I), C.POINTER(I), P]),
        "jsorb_search_for_initialization_async": (I, [P, I, C.POINTER(JsorbInitParams), I] + [P] * 7),
        "jsorb_search_for_initialization": (I, [P, I, C.POINTER(JsorbInitParams), I] + [P] * 6 + [C.POINTER(I)]),
        "jsorb_search_for_initialization_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I), P]),
        "jsorb_init_reference_set": (I, [P, I]),
        "jsorb_init_reference_clear": (I, [P]),
        "jsorb_init_reference_n": (I, [P]),
        "jsorb_search_initial_frame": (I, [P, I, C.POINTER(JsorbInitParams), P, P, C.POINTER(I)]),
        "jsorb_vocabulary_create": (I, [I, I, I, I, P, P, P, P, P, C.POINTER(P)]),
        "jsorb_vocabulary_destroy": (None, [P]),
        "jsorb_vocabulary_info": (I, [P] + [C.POINTER(I)] * 5),
        "jsorb_bow_transform_descriptors": (I, [P, P, I, P, P, P]),
        "jsorb_bow_transform_async": (I, [P, I, P]),
        "jsorb_bow_word_device": (P, [P, I]),
        "jsorb_bow_node_device": (P, [P, I]),
        "jsorb_copy_bow": (I, [P, I, P, P]),
        "jsorb_bow_transform_stats": (I, [P, C.POINTER(I)]),
        "jsorb_search_by_bow_async": (I, [P, I, C.POINTER(JsorbBowParams), P, I] + [P] * 7),
        "jsorb_search_by_bow": (I, [P, I, C.POINTER(JsorbBowParams), P, I] + [P] * 7),
        "jsorb_search_by_bow_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), P]),
        "jsorb_bow_build_caps": (I, [C.POINTER(I), C.POINTER(I)]),
        "jsorb_search_by_projection_kf_async": (I, [P, I, C.POINTER(JsorbKfProjectionParams), I] + [P] * 13),
        "jsorb_search_by_projection_kf": (I, [P, I, C.POINTER(JsorbKfProjectionParams), I] + [P] * 9 + [P, C.POINTER(I)]),
        "jsorb_search_by_projection_kf_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), P]),
        "jsorb_search_kf_build_caps": (I, [C.POINTER(I), C.POINTER(I)]),
        "jsorb_plan_forms": (I, [C.POINTER(JsorbParams), P, I]),
        "jsorb_handle_forms": (I, [P, P, I]),
        "jsorb_keyframe_matcher_create": (I, [I, C.POINTER(P)]),
        "jsorb_keyframe_matcher_destroy": (None, [P]),
        "jsorb_keyframe_matcher_set_stream": (I, [P, P]),
        "jsorb_keyframe_matcher_get_stream": (P, [P]),
        "jsorb_keyframe_matcher_last_error": (C.c_char_p, [P]),
        "jsorb_search_for_triangulation_async": (I, [P, C.POINTER(JsorbTriangulationParams), I] + [P] * 7 + [I] + [P] * 13),
        "jsorb_search_for_triangulation": (I, [P, C.POINTER(JsorbTriangulationParams), I] + [P] * 7 + [I] + [P] * 13),
        "jsorb_search_for_triangulation_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I), P]),
        "jsorb_fuse_async": (I, [P, C.POINTER(JsorbFuseParams), I] + [P] * 10 + [I] + [P] * 13),
        "jsorb_fuse": (I, [P, C.POINTER(JsorbFuseParams), I] + [P] * 10 + [I] + [P] * 13),
        "jsorb_fuse_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
        "jsorb_search_by_bow_kf_async": (I, [P, C.POINTER(JsorbBowParams), I] + [P] * 4 + [I] + [P] * 7),
        "jsorb_search_by_bow_kf": (I, [P, C.POINTER(JsorbBowParams), I] + [P] * 4 + [I] + [P] * 7),
        "jsorb_search_by_bow_kf_stats": (I, [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), P]),
        "jsorb_loop_build_caps": (I, [C.POINTER(I)]),
        "jsorb_search_by_sim3_async": (I, [P, C.POINTER(JsorbSim3Params), C.POINTER(JsorbSim3Side), C.POINTER(JsorbSim3Side)] + [P] * 4),
        "jsorb_search_by_sim3": (I, [P, C.POINTER(JsorbSim3Params), C.POINTER(JsorbSim3Side), C.POINTER(JsorbSim3Side)] + [P] * 3 + [C.POINTER(I)]),
        "jsorb_search_by_sim3_stats": (I, [P] + [C.POINTER(I)] * 5),
        "jsorb_search_by_projection_sim3_async": (I, [P, C.POINTER(JsorbScwParams), I] + [P] * 10 + [I] + [P] * 9),
        "jsorb_search_by_projection_sim3": (I, [P, C.POINTER(JsorbScwParams), I] + [P] * 10 + [I] + [P] * 8 + [C.POINTER(I)]),
        "jsorb_search_by_projection_sim3_stats": (I, [P] + [C.POINTER(I)] * 6),
        "jsorb_scw_build_caps": (I, [C.POINTER(I), C.POINTER(I)]),
        "jsorb_distinctive_descriptors_async": (I, [P, I, P, I, P, P, I, P, I] + [P] * 4),
        "jsorb_distinctive_descriptors": (I, [P, I, P, I, P, P, I, P, I] + [P] * 4),
        "jsorb_distinctive_descriptors_stats": (I, [P] + [C.POINTER(I)] * 8),
        "jsorb_distinct_build_caps": (I, [C.POINTER(I)] * 3),
        "jsorb_keyframe_database_create": (I, [I, I, I, P, C.POINTER(P)]),
        "jsorb_keyframe_database_destroy": (None, [P]),
        "jsorb_keyframe_database_set_stream": (I, [P, P]),
        "jsorb_keyframe_database_get_stream": (P, [P]),
        "jsorb_keyframe_database_last_error": (C.c_char_p, [P]),
        "jsorb_keyframe_database_size": (I, [P]),
        "jsorb_bow_vector_async": (I, [P, P, I, P, P, P]),
        "jsorb_keyframe_database_add_async": (I, [P, I, P, P, I, P]),
        "jsorb_keyframe_database_erase": (I, [P, I]),
        "jsorb_keyframe_database_clear": (I, [P]),
        "jsorb_keyframe_database_score_async": (I, [P, P, P, I, P, P, I, P, P, P]),
        "jsorb_detect_loop_candidates_async": (I, [P, P, P, I, P, C.c_uint64, P, P, F, P, P, P]),
        "jsorb_detect_relocalization_candidates_async": (I, [P, P, P, I, P, C.c_uint64, P, P, P]),
        "jsorb_detect_loop_candidates": (I, [P, P, P, I, P, C.c_uint64, P, P, F, P, P, C.POINTER(I)]),
        "jsorb_detect_relocalization_candidates": (I, [P, P, P, I, P, C.c_uint64, P, P, C.POINTER(I)]),
        "jsorb_detect_candidates_stats": (I, [P] + [C.POINTER(I)] * 5 + [C.POINTER(F), C.POINTER(I)]),
        "jsorb_keyframe_database_copy_state": (I, [P] * 8),
        "jsorb_kfdb_build_caps": (I, [C.POINTER(I)] * 2),
        "jsorb_vocabulary_train": (I, [I, P, P, I, P, I, I, I, I, I, C.c_uint64, I, C.POINTER(P)]),
        "jsorb_vocabulary_train_last_error": (C.c_char_p, []),
        "jsorb_vocab_train_result_destroy": (None, [P]),
        "jsorb_vocab_train_result_info": (I, [P] + [C.POINTER(I)] * 7),
        "jsorb_vocab_train_result_copy": (I, [P] * 8),
        "jsorb_vocab_train_result_copy_assignment": (I, [P, P]),
        "jsorb_vocab_train_stats": (I, [P, C.POINTER(I), C.POINTER(C.c_longlong), C.POINTER(I), C.POINTER(I), P]),
        "jsorb_vocab_train_build_caps": (I, [C.POINTER(I)] * 2),
        "jsorb_local_map_points_async": (I, [P, I, C.POINTER(JsorbMapPointTable), C.POINTER(JsorbFrustumParams), I, P, P, P, I] + [P] * 10),
        "jsorb_local_map_points": (I, [P, I, C.POINTER(JsorbMapPointTable), C.POINTER(JsorbFrustumParams), I, P, P, P, I] + [P] * 12),
        "jsorb_local_map_stats": (I, [P] + [C.POINTER(I)] * 6),
        "jsorb_local_map_build_caps": (I, [C.POINTER(I)]),
        "jsorb_local_keyframes_async": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable), P, I, I, I] + [P] * 5),
        "jsorb_local_keyframes": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable), P, I, I, I] + [P] * 8),
        "jsorb_local_keyframes_stats": (I, [P] + [C.POINTER(I)] * 8),
        "jsorb_local_keyframes_build_caps": (I, [C.POINTER(I)] * 2),
        "jsorb_map_points_scatter_async": (I, [P, I] + [P] * 10 + [I, P, P]),
        "jsorb_update_connections_async": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable), C.POINTER(JsorbCovisibility), I, P, P, P,
                                               C.POINTER(JsorbConnSnapshot), P]),
        "jsorb_update_connections": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable), C.POINTER(JsorbCovisibility), I, P, P, P,
                                         C.POINTER(JsorbConnSnapshot), P, P, P]),
        "jsorb_update_connections_stats": (I, [P] + [C.POINTER(I)] * 7),
        "jsorb_update_connections_scratch": (I, [P] + [C.POINTER(I)] * 2),
        "jsorb_erase_connections_async": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbCovisibility), I, P, P]),
        "jsorb_connected_mask_async": (I, [P, C.POINTER(JsorbCovisibility), I, P]),
        "jsorb_best_covisibles_async": (I, [P, C.POINTER(JsorbCovisibility), I, P, I, P, P]),
        "jsorb_covisibility_copy": (I, [C.POINTER(JsorbCovisibility), I] + [P] * 5),
        "jsorb_covisibility_build_caps": (I, [C.POINTER(I)] * 2),
        "jsorb_cull_keyframes_async": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable), C.POINTER(JsorbCovisibility),
                                           C.POINTER(JsorbKeyframeViews), C.POINTER(JsorbCullingState), I, I, I, P, I, P, I] + [P] * 6),
        "jsorb_cull_keyframes": (I, [P, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable), C.POINTER(JsorbCovisibility),
                                     C.POINTER(JsorbKeyframeViews), C.POINTER(JsorbCullingState), I, I, I, P, I, P, I] + [P] * 12),
        "jsorb_cull_keyframes_stats": (I, [P, P]),
        "jsorb_cull_keyframes_build_caps": (I, [C.POINTER(I)] * 2),
        "jsorb_fuse_map_async": (I, [P, C.POINTER(JsorbFuseParams), I, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable),
                                     C.POINTER(JsorbKeyframeKeypoints), C.POINTER(JsorbFuseState), I, P, I] + [P] * 8 + [I, P, P]),
        "jsorb_fuse_map": (I, [P, C.POINTER(JsorbFuseParams), I, C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable),
                               C.POINTER(JsorbKeyframeKeypoints), C.POINTER(JsorbFuseState), I, P, I] + [P] * 8 + [I, P, P] + [P] * 6),
        "jsorb_fuse_map_stats": (I, [P, P]),
        "jsorb_fuse_map_build_caps": (I, [C.POINTER(I)]),
        "jsorb_create_new_map_points_async": (I, [P, C.POINTER(JsorbTriangulationParams), C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable),
                                                  C.POINTER(JsorbKeyframeKeypoints), C.POINTER(JsorbNewPointKeypoints), C.POINTER(JsorbNewPointState),
                                                  I, I, I, I, P, P, P, P, C.c_float, I, I, P, I] + [P] * 5),
        "jsorb_create_new_map_points": (I, [P, C.POINTER(JsorbTriangulationParams), C.POINTER(JsorbKeyframeGraph), C.POINTER(JsorbMapPointTable),
                                            C.POINTER(JsorbKeyframeKeypoints), C.POINTER(JsorbNewPointKeypoints), C.POINTER(JsorbNewPointState),
                                            I, I, I, I, P, P, P, P, C.c_float, I, I, P, I] + [P] * 10),
        "jsorb_create_new_map_points_stats": (I, [P, P]),
        "jsorb_create_new_map_points_build_caps": (I, [C.POINTER(I)]),
        "jsorb_pose_optimization_async": (I, [P, I, C.POINTER(JsorbPoseParams), C.POINTER(JsorbMapPointTable), I] + [P] * 8),
        "jsorb_pose_optimization": (I, [P, I, C.POINTER(JsorbPoseParams), C.POINTER(JsorbMapPointTable), I] + [P] * 8),
        "jsorb_pose_optimization_stats": (I, [P, P]),
        "jsorb_pose_optimization_build_caps": (I, [C.POINTER(I)] * 2),
        "jsorb_apply_matches_async": (I, [P, I, P, P, I, P]),
    }
    for name, (rt, at) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = rt, at
    _libs_by_path[path] = lib
    if not explicit:
        _lib = lib
    return lib


def read_mask_image(path):
    """cv::imread(path) + cvtColor(BGR2GRAY) of the reference's mask loading (orb_gpu.cpp:64-75) without OpenCV: PNG / binary PGM / PPM -> (H, W)
    uint8.  Returns None when the file cannot be opened (the reference then runs without a mask); raises on an unsupported format."""
    lib = load_library()
    w, h = C.c_int(), C.c_int()
    rc = lib.jsorb_read_mask_image(os.fsencode(path), C.byref(w), C.byref(h), None, 0)
    if rc == -4:
        return None
    if rc != 0:
        raise JsorbError("jsorb_read_mask_image rc=%d: %s" % (rc, lib.jsorb_mask_image_last_error().decode()))
    out = np.zeros((h.value, w.value), np.uint8)
    rc = lib.jsorb_read_mask_image(os.fsencode(path), C.byref(w), C.byref(h), out.ctypes.data, out.size)
    if rc != 0:
        raise JsorbError("jsorb_read_mask_image rc=%d: %s" % (rc, lib.jsorb_mask_image_last_error().decode()))
    return out


def convert_maps(mapx, mapy):
    """jsorb_rectify_convert_maps (host only, no GPU): float maps (CV_32FC1) -> OpenCV's fixed-point form, what cv::convertMaps(..., CV_16SC2)
    returns: (xy int16[H, W, 2], a uint16[H, W] = fy << 5 | fx)."""
    lib = load_library()
    mapx = np.ascontiguousarray(mapx, np.float32)
    mapy = np.ascontiguousarray(mapy, np.float32)
    assert mapx.shape == mapy.shape
    xy = np.zeros(mapx.shape + (2,), np.int16)
    a = np.zeros(mapx.shape, np.uint16)
    rc = lib.jsorb_rectify_convert_maps(mapx.ctypes.data, mapy.ctypes.data, mapx.size, xy.ctypes.data, a.ctypes.data)
    if rc != 0:
        raise JsorbError("jsorb_rectify_convert_maps rc=%d" % rc)
    return xy, a


def image_bounds(K, D, width, height):
    """jsorb_image_bounds (host only, no GPU): Frame::ComputeImageBounds (Frame.cpp:750-778) -> float32 [minX, maxX, minY, maxY]"""
    lib = load_library()
    out = np.zeros(4, np.float32)
    cam = make_camera(K, D)
    rc = lib.jsorb_image_bounds(C.byref(cam), int(width), int(height), out.ctypes.data)
    if rc != 0:
        raise JsorbError("jsorb_image_bounds rc=%d" % rc)
    return out


def plan_launch(im_height, im_width, scale_factor, n_levels, tile_h=30, tile_w=30, fixed_multi_scale_tile_size=False, max_batch=1,
                FAST_N_MIN=9, FAST_N_MAX=14, th_FAST_MAX=20):
    """jsorb_plan_launch: the launch plan of a handle with these parameters, computed on the host (no GPU needed).  Returns a dict with the
    launch-wide numbers and a list of per-level dicts."""
    lib = load_library()
    prm = JsorbParams(im_height, im_width, n_levels, scale_factor, FAST_N_MIN, FAST_N_MAX, 7, th_FAST_MAX, tile_h, tile_w,
                      int(fixed_multi_scale_tile_size), 0, 0, 0, max_batch)
    out = np.zeros(8 + 8 * 16, np.int32)
    rc = lib.jsorb_plan_launch(C.byref(prm), out.ctypes.data, out.size)
    if rc != 0:
        raise JsorbError("jsorb_plan_launch rc=%d" % rc)
    keys = ("levels", "compact", "detect_lds", "spill_chunks", "pyramid_lds", "detect_blocks", "spill_chunk_entries", "reserved")
    res = dict(zip(keys, (int(v) for v in out[:8])))
    lk = ("det_R", "k_tiles", "pool", "score_stride", "list_cap", "pyr_ns16", "pyr_ns_dispatched", "tile_rows")
    res["per_level"] = [dict(zip(lk, (int(v) for v in out[8 + 8 * i:16 + 8 * i]))) for i in range(res["levels"])]
    return res


# jsorb_plan_forms / jsorb_handle_forms slots (include/jsorb.h); COMPACT_FORMS names the JSORB_COMPACT_* launches by id
FORM_KEYS = ("detect_compact", "compact_form", "stereo_buckets", "blur_compact_fusable", "frame_fuses_detect_blur", "tree_replay_levels",
             "nms_ms_cpu_ok", "reserved")
LANE_KEYS = ("lanes", "lane_order", "blur_compact_lanes", "blur_first_lanes")
COMPACT_FORMS = ("flat_reg_1024", "flat_reg_batch", "flat_batch", "flat_1024", "levels_1024")


def plan_forms(im_height, im_width, scale_factor, n_levels, tile_h=30, tile_w=30, fixed_multi_scale_tile_size=False, max_batch=1,
               FAST_N_MIN=9, FAST_N_MAX=14, th_FAST_MAX=20):
    """jsorb_plan_forms: the kernel forms a handle with these parameters selects from its geometry, computed on the host (no GPU needed).
    Returns a dict keyed by FORM_KEYS."""
    lib = load_library()
    prm = JsorbParams(im_height, im_width, n_levels, scale_factor, FAST_N_MIN, FAST_N_MAX, 7, th_FAST_MAX, tile_h, tile_w,
                      int(fixed_multi_scale_tile_size), 0, 0, 0, max_batch)
    out = np.zeros(len(FORM_KEYS), np.int32)
    rc = lib.jsorb_plan_forms(C.byref(prm), out.ctypes.data, out.size)
    if rc != 0:
        raise JsorbError("jsorb_plan_forms rc=%d" % rc)
    return dict(zip(FORM_KEYS, (int(v) for v in out)))


class Vocabulary:
    """jsorb_vocabulary: a vocabulary tree on one device (include/jsorb.h).  `tree` is a dict of flat host arrays as jetson_slam_amd.vocabulary
    builds them (load_text, random_tree, sampled_tree): child_start, children, descriptors, word_id, weight, depth_L.  levels_up is the 4 of
    Frame::ComputeBoW.  Raises JsorbError when the arrays are not a tree the library accepts."""

    def __init__(self, tree, levels_up=4, device_id=0):
        self._lib = load_library()
        self._v = C.c_void_p()
        cs = np.ascontiguousarray(tree["child_start"], np.int32)
        ch = np.ascontiguousarray(tree["children"], np.int32)
        de = np.ascontiguousarray(tree["descriptors"], np.uint8)
        wi = np.ascontiguousarray(tree["word_id"], np.int32)
        we = np.ascontiguousarray(tree["weight"], np.float64)
        n = len(wi)
        if len(cs) != n + 1 or de.size != 32 * n or len(we) != n or (n >= 1 and len(ch) < max(int(cs[-1]), 0)):
            raise JsorbError("Vocabulary: array lengths do not fit n_nodes = %d" % n)
        rc = self._lib.jsorb_vocabulary_create(device_id, n, int(tree["depth_L"]), int(levels_up), cs.ctypes.data, ch.ctypes.data, de.ctypes.data,
                                               wi.ctypes.data, we.ctypes.data, C.byref(self._v))
        if rc != 0:
            self._v = C.c_void_p()
            raise JsorbError("jsorb_vocabulary_create rc=%d" % rc)
        self.levels_up = int(levels_up)
        # the leaves' weights by word id, as double: what KeyframeDatabase folds BowVectors with (the device tree keeps one byte of them)
        leaf = wi >= 0
        self.word_weight = np.zeros(int(wi[leaf].max()) + 1 if leaf.any() else 0, np.float64)
        self.word_weight[wi[leaf]] = we[leaf]

    def info(self):
        """dict(n_nodes, n_words, depth_L, levels_up, max_children)"""
        v = [C.c_int() for _ in range(5)]
        rc = self._lib.jsorb_vocabulary_info(self._v, *[C.byref(t) for t in v])
        if rc != 0:
            raise JsorbError("jsorb_vocabulary_info rc=%d" % rc)
        return dict(zip(("n_nodes", "n_words", "depth_L", "levels_up", "max_children"), (t.value for t in v)))

    @property
    def handle(self):
        return self._v

    def close(self):
        if getattr(self, "_v", None):
            self._lib.jsorb_vocabulary_destroy(self._v)
            self._v = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _build_caps(name, n):
    """the n ints jsorb_<name>_build_caps of the loaded library hands back: a tuple, or the value itself when it is one"""
    v = [C.c_int() for _ in range(n)]
    getattr(load_library(), "jsorb_%s_build_caps" % name)(*[C.byref(x) for x in v])
    return v[0].value if n == 1 else tuple(x.value for x in v)


def bow_build_caps():
    """jsorb_bow_build_caps of the loaded library: (frame entries per lane k_bow_match keeps in registers, keys k_bow_group sorts in LDS)"""
    return _build_caps("bow", 2)


def search_kf_build_caps():
    """jsorb_search_kf_build_caps of the loaded library: (keys k_kf_candidates keeps per point, keypoints up to which k_kf_resolve claims in LDS)"""
    return _build_caps("search_kf", 2)


def loop_build_caps():
    """jsorb_loop_build_caps of the loaded library: candidate entries of a node a lane of k_loop_bow_match keeps in registers"""
    return _build_caps("loop", 1)


def scw_build_caps():
    """jsorb_scw_build_caps of the loaded library: (keys k_scw_candidates keeps per point, keypoints up to which k_scw_resolve claims in LDS)"""
    return _build_caps("scw", 2)


def distinct_build_caps():
    """jsorb_distinct_build_caps of the loaded library: (lanes per point of k_distinct's group tier, the largest N of its wave tier, descriptors its
    block tier holds in LDS)"""
    return _build_caps("distinct", 3)


def _i32_ptr(what, t, n=None, flat=False):
    """the pointer of a contiguous int32 device tensor (of at least n entries; flat: one-dimensional), or the JsorbError that says so about `what`"""
    import torch
    if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or (flat and t.dim() != 1) or (n is not None and t.numel() < n):
        raise JsorbError("%s must be a contiguous int32 device tensor%s" % (what, "" if n is None else " of at least %d entries" % n))
    return t.data_ptr()


def _uploaded_i32(x, dev):
    """(x as an int32 device tensor, whether it was made here): a tensor as it is, a host sequence uploaded"""
    import torch
    if torch.is_tensor(x):
        return x, False
    return torch.tensor([int(v) for v in x], dtype=torch.int32, device=dev), True


def bow_transform_descriptors(voc, descriptors):
    """jsorb_bow_transform_descriptors: a device tensor uint8[n, 32] (16-byte aligned) -> (word_id int32[n], node_id int32[n]) device tensors;
    waits for the current torch stream before it starts and for its own work before it returns"""
    import torch
    if not hasattr(descriptors, "data_ptr") or not getattr(descriptors, "is_cuda", False) or descriptors.dtype != torch.uint8:
        raise JsorbError("bow_transform_descriptors: descriptors must be a uint8 device tensor")
    if descriptors.dim() != 2 or descriptors.shape[1] != 32 or not descriptors.is_contiguous():
        raise JsorbError("bow_transform_descriptors: descriptors must be a contiguous tensor of shape (n, 32)")
    n = int(descriptors.shape[0])
    if n and descriptors.data_ptr() % 16:
        raise JsorbError("bow_transform_descriptors: descriptors must be 16-byte aligned")
    word = torch.full((max(n, 1),), -1, dtype=torch.int32, device=descriptors.device)
    node = torch.full((max(n, 1),), -1, dtype=torch.int32, device=descriptors.device)
    torch.cuda.current_stream(descriptors.device).synchronize()
    rc = voc._lib.jsorb_bow_transform_descriptors(None, voc.handle, n, descriptors.data_ptr() if n else None, word.data_ptr(), node.data_ptr())
    if rc != 0:
        raise JsorbError("jsorb_bow_transform_descriptors rc=%d" % rc)
    torch.cuda.synchronize(descriptors.device)
    return word[:n], node[:n]


class KeyframeMatcher:
    """jsorb_keyframe_matcher: the keyframe-to-keyframe matcher of LocalMapping (include/jsorb.h), with a stream and scratch of its own - it
    belongs to no ORBExtractor and may be used from another thread than the extractors.  A keyframe side is a dict of device tensors: node int32[n],
    free uint8 / bool [n], stereo uint8 / bool [n], x, y, angle float32[n], desc uint8[n, 32] (16-byte aligned) and, for the KF2 side, octave
    int32[n]."""
    KF1_KEYS = ("node", "free", "stereo", "x", "y", "angle", "desc")
    KF2_KEYS = ("node", "free", "stereo", "x", "y", "octave", "angle", "desc")

    def __init__(self, device_id=0):
        self._lib = load_library()
        self._m = C.c_void_p()
        rc = self._lib.jsorb_keyframe_matcher_create(int(device_id), C.byref(self._m))
        if rc != 0:
            self._m = C.c_void_p()
            raise JsorbError("jsorb_keyframe_matcher_create rc=%d" % rc)
        self.device_id = int(device_id)

    @property
    def handle(self):
        return self._m

    def close(self):
        if getattr(self, "_m", None):
            self._lib.jsorb_keyframe_matcher_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise JsorbError("libjsorb rc=%d: %s" % (rc, self._lib.jsorb_keyframe_matcher_last_error(self._m).decode()))

    def set_stream(self, stream_ptr):
        """use an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None restores the matcher's own"""
        self._chk(self._lib.jsorb_keyframe_matcher_set_stream(self._m, stream_ptr))

    def get_stream(self):
        return self._lib.jsorb_keyframe_matcher_get_stream(self._m) or 0

    def sync(self):
        rc = self._lib.jsorb_mem_stream_sync(C.c_void_p(self.get_stream()))
        if rc != 0:
            raise JsorbError("KeyframeMatcher.sync: jsorb_mem_stream_sync rc=%d" % rc)

    # ---- the argument builders' shared parts: one side checker, one kf_start reader, one runner per call form ----
    @staticmethod
    def _side(what, d, keys, dtypes, name, n, optional=None):
        """the pointers of one side of a call (NULL when n is 0): d[k] for every key a contiguous device tensor of shape (n,), or (n, 32) and
        16-byte aligned for a descriptor key (*desc); dtypes: the dtypes a key may have (float32 when absent).  optional: the keys that may be
        None or absent (a NULL pointer) - a side that has some is read with .get, so that a missing key is "not a device tensor" there"""
        import torch
        ptrs = []
        for k in keys:
            t = d[k] if optional is None else d.get(k)
            if t is None and optional and k in optional:
                ptrs.append(None)
                continue
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("%s: %s[%r] must be a device tensor" % (what, name, k))
            shape = (n, 32) if k.endswith("desc") else (n,)
            ok = dtypes.get(k, (torch.float32,))
            if t.dtype not in ok or tuple(t.shape) != shape or not t.is_contiguous():
                raise JsorbError("%s: %s[%r] must be a contiguous %s tensor of shape %s" % (what, name, k, " / ".join(str(x) for x in ok), shape))
            if n and k.endswith("desc") and t.data_ptr() % 16:
                raise JsorbError("%s: %s[%r] must be 16-byte aligned" % (what, name, k))
            ptrs.append(t.data_ptr() if n else None)
        return ptrs

    @staticmethod
    def _kf_start(what, kf_start):
        """kf_start as a host int32 array -> (the array, n_keyframes, the keypoints of all keyframes)"""
        ks = np.ascontiguousarray(kf_start, np.int32)
        if ks.ndim != 1 or len(ks) < 1:
            raise JsorbError("%s: kf_start must be a host array of n_keyframes + 1 offsets" % what)
        return ks, len(ks) - 1, int(ks[-1])

    @staticmethod
    def _c_args(args):
        """a builder's arguments as the C call takes them.  The converted host arrays (kf_start, the per-keyframe geometry) stand in `args` as
        numpy arrays and give their address only here: whoever holds `args` across the call keeps them alive - np.ascontiguousarray copies a
        list, another dtype or a strided array, and an address taken from such a copy inside the builder would outlive it"""
        return [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]

    def _enqueue(self, name, args, dev, shapes, wait):
        """the asynchronous form `name`: the outputs (int32 device tensors of `shapes`, allocated -7-filled with no dimension below 1) behind
        `args`; wait as in search_for_triangulation.  Returns the outputs cut to their shapes."""
        import torch
        outs = [torch.full([max(s, 1) for s in shape], -7, dtype=torch.int32, device=dev) for shape in shapes]
        if wait:
            torch.cuda.current_stream(dev).synchronize()
        self._chk(getattr(self._lib, name)(self._m, *self._c_args(args), *[o.data_ptr() for o in outs]))
        if wait:
            self.sync()
        return tuple(o.reshape(-1)[:int(np.prod(shape))].reshape(shape) for o, shape in zip(outs, shapes))

    def _call_host(self, name, args, dev, shapes):
        """the synchronous form `name`: the same with host arrays; a shape () is one int, returned as a number"""
        import torch
        outs = [C.c_int(-7) if shape == () else np.full(max(int(np.prod(shape)), 1), -7, np.int32) for shape in shapes]
        torch.cuda.current_stream(dev).synchronize()
        self._chk(getattr(self._lib, name)(self._m, *self._c_args(args), *[C.byref(o) if shape == () else o.ctypes.data for o, shape in zip(outs, shapes)]))
        return tuple(o.value if shape == () else o[:int(np.prod(shape))].reshape(shape) for o, shape in zip(outs, shapes))

    def _args(self, kf1, kf_start, kf2, F12, epipole, params):
        """-> (device, output shapes, arguments) of jsorb_search_for_triangulation*"""
        import torch
        what = "search_for_triangulation"
        if not isinstance(params, JsorbTriangulationParams):
            raise JsorbError("%s: params must come from make_triangulation_params" % what)
        ks, nk, total = self._kf_start(what, kf_start)
        F = np.ascontiguousarray(F12, np.float32).reshape(-1)
        E = np.ascontiguousarray(epipole, np.float32).reshape(-1)
        if len(F) != 9 * nk or len(E) != 2 * nk:
            raise JsorbError("%s: F12 must hold 9 and epipole 2 floats per keyframe" % what)
        dt = dict(node=(torch.int32,), octave=(torch.int32,), free=(torch.uint8, torch.bool), stereo=(torch.uint8, torch.bool), desc=(torch.uint8,))
        n1 = int(kf1["node"].shape[0])
        p1, p2 = self._side(what, kf1, self.KF1_KEYS, dt, "kf1", n1), self._side(what, kf2, self.KF2_KEYS, dt, "kf2", total)
        return kf1["node"].device, [(nk, n1), (nk,)], [C.byref(params), n1] + p1 + [nk, ks] + p2 + [F, E]

    def search_for_triangulation(self, kf1, kf_start, kf2, F12, epipole, params, wait=True):
        """jsorb_search_for_triangulation_async: KF1 against the len(kf_start) - 1 concatenated KF2s (kf_start: HOST int32 offsets; F12 host
        float32[n_keyframes, 9] row-major, epipole host float32[n_keyframes, 2]).  Returns (match12 int32[n_keyframes, n1], n_matches
        int32[n_keyframes]) as device tensors, enqueued on the matcher's stream.  wait=True: the call waits for the current torch stream before
        it starts and for its own work before it returns; wait=False only enqueues - the caller orders the streams (set_stream).  With
        wait=False the returned tensors come from torch's caching allocator on the CURRENT torch stream but are written on the matcher's stream:
        keep them alive until the matcher's stream has finished (or make that stream the current torch stream, as set_stream with
        torch.cuda.current_stream().cuda_stream does), or the allocator may hand their memory out again while the kernels still write it."""
        dev, shapes, args = self._args(kf1, kf_start, kf2, F12, epipole, params)
        return self._enqueue("jsorb_search_for_triangulation_async", args, dev, shapes, wait)

    def search_for_triangulation_host(self, kf1, kf_start, kf2, F12, epipole, params):
        """jsorb_search_for_triangulation, the synchronous form: the same inputs, (match12 int32[n_keyframes, n1], n_matches int32[n_keyframes]) on
        the host with one copy back"""
        dev, shapes, args = self._args(kf1, kf_start, kf2, F12, epipole, params)
        return self._call_host("jsorb_search_for_triangulation", args, dev, shapes)

    def stats(self):
        """((keyframe, node) pairs on both sides, Hamming distances, candidates at the line test, most KF2 keypoints in such a node, keyframe 0's
        (ind1, ind2, ind3)) of the last search_for_triangulation"""
        p, d, l, m, b = C.c_int(), C.c_int(), C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self._lib.jsorb_search_for_triangulation_stats(self._m, C.byref(p), C.byref(d), C.byref(l), C.byref(m), b))
        return p.value, d.value, l.value, m.value, tuple(b)


    POINT_KEYS = ("Px", "Py", "Pz", "Nx", "Ny", "Nz", "max_distance", "min_dist_inv", "max_dist_inv", "desc")
    FUSE_KF_KEYS = ("x", "y", "octave", "uright", "desc")

    def _fuse_args(self, points, kf_start, keyframes, Rcw, tcw, Ow, params, skip):
        """-> (device, output shapes, arguments) of jsorb_fuse*"""
        import torch
        what = "fuse"
        if not isinstance(params, JsorbFuseParams):
            raise JsorbError("%s: params must come from make_fuse_params" % what)
        ks, nk, total = self._kf_start(what, kf_start)
        R, t, O = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (Rcw, tcw, Ow))
        if len(R) != 9 * nk or len(t) != 3 * nk or len(O) != 3 * nk:
            raise JsorbError("%s: Rcw must hold 9, tcw 3 and Ow 3 floats per keyframe" % what)
        dt = dict(octave=(torch.int32,), desc=(torch.uint8,))
        n = int(points["Px"].shape[0])
        pp = self._side(what, points, self.POINT_KEYS, dt, "points", n, optional=())
        pk = self._side(what, keyframes, self.FUSE_KF_KEYS, dt, "keyframes", total, optional=("uright",))
        sp = None
        if skip is not None:
            if not getattr(skip, "is_cuda", False) or skip.dtype not in (torch.uint8, torch.bool) or skip.numel() != nk * n or not skip.is_contiguous():
                raise JsorbError("%s: skip must be a contiguous uint8 / bool device tensor of n_keyframes x n_points entries" % what)
            sp = skip.data_ptr() if nk * n else None
        return points["Px"].device, [(nk, n), (nk, n), (nk,)], \
            [C.byref(params), n] + pp + [nk, ks] + pk + [R, t, O, sp]

    def fuse(self, points, kf_start, keyframes, Rcw, tcw, Ow, params, skip=None, wait=True):
        """jsorb_fuse_async: the n map points (dict of device tensors: Px, Py, Pz, Nx, Ny, Nz, max_distance, min_dist_inv, max_dist_inv float32[n],
        desc uint8[n, 32]) against the len(kf_start) - 1 concatenated keyframes (dict: x, y float32, octave int32, desc uint8[., 32] and uright float32 or
        None / absent: monocular; kf_start: HOST int32 offsets; Rcw host float32[n_keyframes, 9] row-major, tcw and Ow host float32[n_keyframes, 3]).
        skip: uint8 / bool device tensor [n_keyframes, n] or None.  Returns (best_idx, best_dist int32[n_keyframes, n], n_matched
        int32[n_keyframes]) as device tensors; wait= as in search_for_triangulation, with the same rule for the returned tensors' lifetime."""
        dev, shapes, args = self._fuse_args(points, kf_start, keyframes, Rcw, tcw, Ow, params, skip)
        return self._enqueue("jsorb_fuse_async", args, dev, shapes, wait)

    def fuse_host(self, points, kf_start, keyframes, Rcw, tcw, Ow, params, skip=None):
        """jsorb_fuse, the synchronous form: the same inputs, (best_idx, best_dist int32[n_keyframes, n], n_matched int32[n_keyframes]) on the host
        with one copy back"""
        dev, shapes, args = self._fuse_args(points, kf_start, keyframes, Rcw, tcw, Ow, params, skip)
        return self._call_host("jsorb_fuse", args, dev, shapes)

    def fuse_stats(self):
        """((keyframe, point) pairs that reached a window, keypoints walked, Hamming distances, the largest window) of the last fuse"""
        w, k, d, l = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.jsorb_fuse_stats(self._m, C.byref(w), C.byref(k), C.byref(d), C.byref(l)))
        return w.value, k.value, d.value, l.value


    # ---- LoopClosing::ComputeSim3: SearchByBoW(KF, KF) for all candidates, SearchBySim3 ----
    BOW_KF_KEYS = ("node", "valid", "angle", "desc")

    def _bow_kf_args(self, kf1, kf_start, candidates, params):
        """-> (device, output shapes, arguments) of jsorb_search_by_bow_kf*"""
        import torch
        what = "search_by_bow_kf"
        if not isinstance(params, JsorbBowParams):
            raise JsorbError("%s: params must come from make_bow_params" % what)
        ks, nk, total = self._kf_start(what, kf_start)
        dt = dict(node=(torch.int32,), valid=(torch.uint8, torch.bool), desc=(torch.uint8,))
        n1 = int(kf1["node"].shape[0])
        p1, p2 = self._side(what, kf1, self.BOW_KF_KEYS, dt, "kf1", n1), self._side(what, candidates, self.BOW_KF_KEYS, dt, "candidates", total)
        return kf1["node"].device, [(nk, n1), (nk,)], [C.byref(params), n1] + p1 + [nk, ks] + p2

    def search_by_bow_kf(self, kf1, kf_start, candidates, params, wait=True):
        """jsorb_search_by_bow_kf_async: the current keyframe (dict of device tensors: node int32[n1], valid uint8 / bool [n1], angle float32[n1],
        desc uint8[n1, 32]) against the len(kf_start) - 1 concatenated loop candidates (the same keys; kf_start: HOST int32 offsets into them, the
        arrays hold kf_start[-1] entries).  Returns (match12 int32[n_keyframes, n1], n_matches int32[n_keyframes]) as device tensors; wait= as in
        search_for_triangulation, with the same rule for the returned tensors' lifetime."""
        dev, shapes, args = self._bow_kf_args(kf1, kf_start, candidates, params)
        return self._enqueue("jsorb_search_by_bow_kf_async", args, dev, shapes, wait)

    def search_by_bow_kf_host(self, kf1, kf_start, candidates, params):
        """jsorb_search_by_bow_kf, the synchronous form: the same inputs, (match12 int32[n_keyframes, n1], n_matches int32[n_keyframes]) on the host
        with one copy back"""
        dev, shapes, args = self._bow_kf_args(kf1, kf_start, candidates, params)
        return self._call_host("jsorb_search_by_bow_kf", args, dev, shapes)

    def search_by_bow_kf_stats(self):
        """((candidate, node) pairs on both sides, Hamming distances, most candidate keypoints in such a node, candidate 0's (ind1, ind2, ind3)) of
        the last search_by_bow_kf"""
        p, d, m, b = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self._lib.jsorb_search_by_bow_kf_stats(self._m, C.byref(p), C.byref(d), C.byref(m), b))
        return p.value, d.value, m.value, tuple(b)

    SIM3_KEYS = ("x", "y", "octave", "kp_desc", "Px", "Py", "Pz", "max_distance", "min_dist_inv", "max_dist_inv", "mp_desc", "search")
    SIM3_POSE = (("Rw", 9), ("tw", 3), ("sR", 9), ("t", 3))

    def _sim3_args(self, side1, side2, params):
        """-> (jsorb_sim3_side of side1, of side2, arguments) of jsorb_search_by_sim3* (nothing of `self` is read)"""
        import torch
        what, K = "search_by_sim3", KeyframeMatcher
        if not isinstance(params, JsorbSim3Params):
            raise JsorbError("%s: params must come from make_sim3_params" % what)
        dt = dict(octave=(torch.int32,), kp_desc=(torch.uint8,), mp_desc=(torch.uint8,), search=(torch.uint8, torch.bool))
        sides = []
        for d, name in ((side1, "side1"), (side2, "side2")):
            s = JsorbSim3Side(int(d["x"].shape[0]))
            for k, ptr in zip(K.SIM3_KEYS, K._side(what, d, K.SIM3_KEYS, dt, name, s.n)):
                setattr(s, k, ptr)
            for k, size in K.SIM3_POSE:
                v = np.ascontiguousarray(d[k], np.float32).reshape(-1)
                if len(v) != size:
                    raise JsorbError("%s: %s[%r] must hold %d floats" % (what, name, k, size))
                setattr(s, k, (C.c_float * size)(*v.tolist()))
            sides.append(s)
        return sides[0], sides[1], [C.byref(params), C.byref(sides[0]), C.byref(sides[1])]

    def search_by_sim3(self, side1, side2, params, wait=True):
        """jsorb_search_by_sim3_async: each side a dict of device tensors aligned with the keyframe's keypoints (x, y float32, octave int32, kp_desc
        uint8[n, 32]; Px, Py, Pz, max_distance, min_dist_inv, max_dist_inv float32, mp_desc uint8[n, 32], search uint8 / bool) and of HOST float32
        arrays: Rw (9, row-major), tw (3) of the keyframe itself, sR (9), t (3) into the OTHER camera (side 1: sR21, t21; side 2: sR12, t12).
        Returns (match1 int32[n1], match2 int32[n2], match12 int32[n1], n_found int32[1]) as device tensors; wait= as in
        search_for_triangulation, with the same rule for the returned tensors' lifetime."""
        s1, s2, args = self._sim3_args(side1, side2, params)
        return self._enqueue("jsorb_search_by_sim3_async", args, side1["x"].device, [(s1.n,), (s2.n,), (s1.n,), (1,)], wait)

    def search_by_sim3_host(self, side1, side2, params):
        """jsorb_search_by_sim3, the synchronous form: the same inputs, (match1 int32[n1], match2 int32[n2], match12 int32[n1], n_found) on the host
        with one copy back"""
        s1, s2, args = self._sim3_args(side1, side2, params)
        return self._call_host("jsorb_search_by_sim3", args, side1["x"].device, [(s1.n,), (s2.n,), (s1.n,), ()])

    def search_by_sim3_stats(self):
        """(slots that reached a window, keypoints walked, Hamming distances, the largest window, agreements) of the last search_by_sim3, both
        directions together"""
        v = [C.c_int() for _ in range(5)]
        self._chk(self._lib.jsorb_search_by_sim3_stats(self._m, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


    # ---- LoopClosing::ComputeSim3's acceptance test: SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) ----
    SCW_KF_KEYS = ("x", "y", "octave", "desc", "blocked")

    def _scw_args(self, points, keyframe, params):
        """-> (device, n_points, N, arguments) of jsorb_search_by_projection_sim3* (nothing of `self` is read)"""
        import torch
        what, K = "search_by_projection_sim3", KeyframeMatcher
        if not isinstance(params, JsorbScwParams):
            raise JsorbError("%s: params must come from scw_params" % what)
        dt = dict(octave=(torch.int32,), desc=(torch.uint8,), blocked=(torch.uint8, torch.bool))
        if not hasattr(points.get("Px"), "shape") or not hasattr(keyframe.get("x"), "shape"):
            raise JsorbError("%s: points['Px'] and keyframe['x'] must be device tensors" % what)
        n, N = int(points["Px"].shape[0]), int(keyframe["x"].shape[0])
        pp = K._side(what, points, K.POINT_KEYS, dt, "points", n, optional=())
        pk = K._side(what, keyframe, K.SCW_KF_KEYS, dt, "keyframe", N, optional=("blocked",))
        return points["Px"].device, n, N, [C.byref(params), n] + pp + [N] + pk

    def search_by_projection_sim3(self, points, keyframe, params, sync=False, wait=True):
        """jsorb_search_by_projection_sim3_async (sync=False) or jsorb_search_by_projection_sim3 (sync=True): the n loop points the reference would
        search, in vpPoints order (dict of device tensors: Px, Py, Pz, Nx, Ny, Nz, max_distance, min_dist_inv, max_dist_inv float32[n], desc
        uint8[n, 32]) against the keyframe (dict: x, y float32[N], octave int32[N], desc uint8[N, 32] and blocked uint8 / bool [N] or None / absent:
        nothing blocked).  Returns (match_kp int32[n], match_dist int32[n], kp_match int32[N], n_matches): device tensors (n_matches int32[1]) with
        sync=False - wait= as in search_for_triangulation, with the same rule for the returned tensors' lifetime - or host arrays and a number
        with sync=True."""
        dev, n, N, args = self._scw_args(points, keyframe, params)
        if sync:
            return self._call_host("jsorb_search_by_projection_sim3", args, dev, [(n,), (n,), (N,), ()])
        return self._enqueue("jsorb_search_by_projection_sim3_async", args, dev, [(n,), (n,), (N,), (1,)], wait)

    def search_by_projection_sim3_stats(self):
        """(rounds of the fixed point, keys kept, points over the list cap, points that reached a window, Hamming distances, the largest window) of
        the last search_by_projection_sim3"""
        v = [C.c_int() for _ in range(6)]
        self._chk(self._lib.jsorb_search_by_projection_sim3_stats(self._m, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


    # ---- between two matcher calls: MapPoint::ComputeDistinctiveDescriptors for many points ----
    @staticmethod
    def _distinct_args(obs_start, obs_row, kf_desc, out_row, desc_out, changed):
        """-> (device, n_points, the `changed` tensor or None, arguments) of jsorb_distinctive_descriptors* (nothing of `self` is read)"""
        import torch
        what, K = "distinctive_descriptors", KeyframeMatcher
        for name, t in (("obs_start", obs_start), ("obs_row", obs_row), ("kf_desc", kf_desc)):
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("%s: %s must be a device tensor" % (what, name))
        if obs_start.dtype != torch.int32 or len(obs_start.shape) != 1 or obs_start.shape[0] < 1 or not obs_start.is_contiguous():
            raise JsorbError("%s: obs_start must be a contiguous torch.int32 tensor of n_points + 1 offsets" % what)
        n, n_obs, n_rows = int(obs_start.shape[0]) - 1, int(obs_row.shape[0]), int(kf_desc.shape[0])
        dt = dict(obs_row=(torch.int32,), out_row=(torch.int32,), kf_desc=(torch.uint8,), desc=(torch.uint8,))
        (po,) = K._side(what, dict(obs_row=obs_row), ("obs_row",), dt, "observations", n_obs)
        (pk,) = K._side(what, dict(kf_desc=kf_desc), ("kf_desc",), dt, "keyframes", n_rows)
        n_out = 0 if desc_out is None else int(desc_out.shape[0]) if hasattr(desc_out, "shape") and len(desc_out.shape) else -1
        (pd,) = K._side(what, dict(desc=desc_out), ("desc",), dt, "desc_out", n_out, optional=("desc",))
        (pr,) = K._side(what, dict(out_row=out_row), ("out_row",), dt, "points", n, optional=("out_row",))
        if changed and desc_out is None:
            raise JsorbError("%s: changed needs desc_out" % what)
        ch = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=obs_start.device) if changed else None
        return obs_start.device, n, ch, [n, obs_start.data_ptr(), n_obs, po, pk, n_rows, pr, n_out, pd, ch.data_ptr() if changed and pd else None]      # (no rows at all: no desc_out pointer, so none for changed)

    def distinctive_descriptors(self, obs_start, obs_row, kf_desc, out_row=None, desc_out=None, changed=False, sync=False, wait=True):
        """jsorb_distinctive_descriptors_async (sync=False) or jsorb_distinctive_descriptors (sync=True): MapPoint::ComputeDistinctiveDescriptors for
        the len(obs_start) - 1 points whose observations are the CSR obs_start int32[n + 1] / obs_row int32[n_obs] into the rows of kf_desc
        uint8[n_rows, 32] (device tensors, the observations of a point in the caller's map order with the bad keyframes left out).  desc_out: None
        or a uint8[n_out_rows, 32] device tensor whose row out_row[p] (int32[n] device tensor; None: row p) is overwritten IN PLACE with the winner's
        bytes; changed=True also returns a uint8[n] device tensor, 1 where a row was written with other bytes than it held.  Returns (best_obs
        int32[n], best_median int32[n]) - device tensors with sync=False (wait= as in search_for_triangulation, with the same rule for the returned
        tensors' lifetime), host arrays with sync=True - followed by the `changed` tensor when asked for."""
        dev, n, ch, args = self._distinct_args(obs_start, obs_row, kf_desc, out_row, desc_out, changed)
        if sync:
            out = self._call_host("jsorb_distinctive_descriptors", args, dev, [(n,), (n,)])
        else:
            out = self._enqueue("jsorb_distinctive_descriptors_async", args, dev, [(n,), (n,)], wait)
        return out + (ch[:n],) if changed else out

    def distinctive_descriptors_stats(self):
        """(points of the group tier, of the wave tier, of the block tier, those of the block tier beyond its LDS cap, empty points, invalid points,
        rows changed, the largest N) of the last distinctive_descriptors"""
        v = [C.c_int() for _ in range(8)]
        self._chk(self._lib.jsorb_distinctive_descriptors_stats(self._m, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # ---- the covisibility graph: KeyFrame::UpdateConnections / AddConnection / EraseConnection (KeyFrame.cpp:127-161, :293-383, :557-571) ----
    def _run_outputs(self, name, args, keys, shapes, out, dev, sync, wait, made):
        """jsorb_<name>_async, or with sync jsorb_<name>, for the calls that return a dict of int32 outputs.  args: the call's arguments behind the
        matcher, an output's key standing for its pointer; shapes: per key the shape the call fills.  The buffers are those of `out` (the dict of
        an earlier call) or new ones of at least one element each.  The current torch stream is waited for first with wait or sync, and where a
        tensor was made for the call (`made`, or the buffers are new).  Returns the dict: per key the buffer's view of that shape, "_bufs", and
        with sync the same as numpy arrays under *_host (-7 where the call writes nothing)."""
        import torch
        size = {k: int(np.prod(shapes[k])) for k in keys}
        bufs = out["_bufs"] if out is not None else {k: torch.empty([max(int(x), 1) for x in shapes[k]], dtype=torch.int32, device=dev) for k in keys}
        args = [self._m] + [bufs[a].data_ptr() if isinstance(a, str) else a for a in args]
        if wait or sync or made or out is None:
            torch.cuda.current_stream(dev).synchronize()     # (tensors were made on it)
        out = {k: bufs[k].reshape(-1)[:size[k]].reshape(shapes[k]) for k in keys}
        out["_bufs"] = bufs
        if sync:
            host = {k: np.full(max(size[k], 1), -7, np.int32) for k in keys}
            self._chk(getattr(self._lib, "jsorb_" + name)(*args, *[host[k].ctypes.data for k in keys]))
            out.update({k + "_host": host[k][:size[k]].reshape(shapes[k]) for k in keys})
        else:
            self._chk(getattr(self._lib, "jsorb_%s_async" % name)(*args))
            if wait:
                self.sync()
        return out

    def update_connections(self, graph, table, cov, slots, neighbours=None, snapshot=False, sync=False, out=None, wait=True):
        """jsorb_update_connections*: UpdateConnections() of the keyframes `slots` (at most 32: an int32 device tensor, or a host sequence that is
        uploaded) one after the other.  graph a KeyframeGraph, table a MapPointTable, cov a Covisibility.  neighbours: None, or the writable
        int32[S, 10] table (graph.neighbours) whose rows follow the rewritten lists.  snapshot=True also returns each member's map as its own
        update left it.  Returns a dict of device tensors - parent_out int32[n], counts int32[8] (UPDATE_CONNECTIONS_COUNTS), with snapshot
        snap_slot / snap_weight int32[n, C] and snap_len int32[n] - and with sync=True parent_host and counts_host (numpy).  out: the dict of an
        earlier call with as many slots, written again.  wait=True waits for the current torch stream before and for the matcher behind; with
        wait=False the call only enqueues, and waits for the torch stream just where it made a tensor itself (slots uploaded, out=None)."""
        import torch
        dev = cov.conn_len.device
        slots, made = _uploaded_i32(slots, dev)
        made = made or out is None
        n = int(slots.numel())
        sp = _i32_ptr("update_connections: slots", slots) if n else None
        nb = None if neighbours is None else _i32_ptr("update_connections: neighbours", neighbours, cov.max_keyframes * KF_NEIGHBOURS)
        if out is None:
            Cn, n1 = cov.conn_capacity, max(n, 1)   # (a call with no slots still hands over valid arrays)
            bufs = dict(parent_out=torch.empty(n1, dtype=torch.int32, device=dev), counts=torch.empty(8, dtype=torch.int32, device=dev))
            if snapshot:
                bufs.update(snap_slot=torch.zeros((n1, Cn), dtype=torch.int32, device=dev), snap_weight=torch.zeros((n1, Cn), dtype=torch.int32, device=dev),
                            snap_len=torch.empty(n1, dtype=torch.int32, device=dev))
            out = {k: (v if k == "counts" else v[:n]) for k, v in bufs.items()}
            out["_bufs"] = bufs
        bufs = out["_bufs"]
        snap = None
        if "snap_len" in bufs:
            snap = C.byref(JsorbConnSnapshot(bufs["snap_slot"].data_ptr(), bufs["snap_weight"].data_ptr(), bufs["snap_len"].data_ptr()))
        gs, tb, cs = graph.struct(), table.struct(), cov.struct()
        args = [self._m, C.byref(gs), C.byref(tb), C.byref(cs), n, sp, nb, bufs["parent_out"].data_ptr(), snap, bufs["counts"].data_ptr()]
        if wait or sync or made:
            torch.cuda.current_stream(dev).synchronize()
        if sync:
            parent_h, counts_h = np.full(max(n, 1), -2, np.int32), np.zeros(8, np.int32)
            self._chk(self._lib.jsorb_update_connections(*args, parent_h.ctypes.data, counts_h.ctypes.data))
            out = dict(out, parent_host=parent_h[:n], counts_host=counts_h)
        else:
            self._chk(self._lib.jsorb_update_connections_async(*args))
            if wait:
                self.sync()
        out["slots"] = slots                     # (kept alive with the result: the device reads it after the call returns)
        return out

    def update_connections_stats(self):
        """dict of UPDATE_CONNECTIONS_COUNTS of the last update_connections (waits for it)"""
        v = [C.c_int() for _ in range(7)]
        self._chk(self._lib.jsorb_update_connections_stats(self._m, *[C.byref(x) for x in v]))
        return dict(zip(UPDATE_CONNECTIONS_COUNTS, (x.value for x in v)))

    def update_connections_scratch(self):
        """(row words of the scratch, how many are not zero - 0 between calls) after the last update_connections (waits for it)"""
        n, nz = C.c_int(), C.c_int()
        self._chk(self._lib.jsorb_update_connections_scratch(self._m, C.byref(n), C.byref(nz)))
        return n.value, nz.value

    def erase_connections(self, graph, cov, slot, neighbours=None, wait=True):
        """jsorb_erase_connections_async: SetBadFlag's EraseConnection walk for `slot`; returns counts int32[2] (device): the keys walked, the maps
        that held the slot"""
        import torch
        dev = cov.conn_len.device
        nb = None if neighbours is None else _i32_ptr("erase_connections: neighbours", neighbours, cov.max_keyframes * KF_NEIGHBOURS)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        gs, cs = graph.struct(), cov.struct()
        if wait:
            torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_erase_connections_async(self._m, C.byref(gs), C.byref(cs), int(slot), nb, counts.data_ptr()))
        if wait:
            self.sync()
        return counts

    def connected_mask(self, cov, slot, out=None, wait=True):
        """jsorb_connected_mask_async: GetConnectedKeyFrames() of `slot` as a uint8[S] device tensor (what detect_loop_candidates takes)"""
        import torch
        dev = cov.conn_len.device
        if out is None:
            out = torch.empty(max(cov.max_keyframes, 1), dtype=torch.uint8, device=dev)[:cov.max_keyframes]
        cs = cov.struct()
        if wait:
            torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_connected_mask_async(self._m, C.byref(cs), int(slot), out.data_ptr()))
        if wait:
            self.sync()
        return out

    def best_covisibles(self, cov, slots, N, wait=True):
        """jsorb_best_covisibles_async: GetBestCovisibilityKeyFrames(N) of many slots (an int32 device tensor or a host sequence); returns
        (out int32[n, N] -1 padded, out_len int32[n]) device tensors"""
        import torch
        dev = cov.conn_len.device
        slots, made = _uploaded_i32(slots, dev)
        n, N = int(slots.numel()), int(N)
        sp = _i32_ptr("best_covisibles: slots", slots) if n else None
        out = torch.empty((max(n, 1), max(N, 1)), dtype=torch.int32, device=dev)[:n]
        out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        cs = cov.struct()
        if wait or made:
            torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_best_covisibles_async(self._m, C.byref(cs), n, sp, N, out.data_ptr(), out_len.data_ptr()))
        if wait:
            self.sync()
        return out, out_len


    # ---- culling: LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag (LocalMapping.cpp:638-702, KeyFrame.cpp:457-549) ----
    def cull_keyframes(self, graph, table, cov, views, state, candidates, first_slot=-1, monocular=False, max_cull=4, neighbours=None,
                       reparent_cap=64, sync=False, wait=True, apply=False, database=None, out=None):
        """jsorb_cull_keyframes*: KeyFrameCulling over `candidates` (an int32 device tensor - what best_covisibles(cov, [current],
        cov.conn_capacity) returned, flattened - or a host sequence that is uploaded), in order, each culled keyframe's SetBadFlag complete before the
        next candidate is looked at.  views a KeyframeViews, state a culling_state(graph, table, ...).  At most max_cull (<= 16) keyframes are culled
        per call (every round is enqueued whether it finds a cull or not, about 7 us each on an MI355X, hence the default of 4); counts[0] = next
        says where a second call continues (candidates[next:]).  Returns a dict of device tensors: decision, n_mps,
        n_redundant int32[n], culled_slot int32[max_cull], reparent_out int32[reparent_cap, 2], counts int32[10] (CULL_COUNTS); with sync=True
        the same as numpy arrays under *_host.  apply=True (implies sync) does the binding's part of SetBadFlag from what came back: the child runs
        of the culled keyframes and of every parent that lost or gained a child are rewritten with graph.set_children (children in (order_key,
        slot) order; only keyframes with state 1 are listed - a bad keyframe that parent[] still names as a child, which the fallback hands on,
        is in no child run, as after the reference's EraseChild), and the culled slots are erased from `database` (a KeyframeDatabase) when one
        is passed.  out: the dict of an earlier call with the same n, max_cull and reparent_cap, written again.  The call waits for the current
        torch stream before it enqueues, except with wait=False, out given and candidates a device tensor: then it makes no tensor, waits for
        nothing and only enqueues - the form a graph capture takes."""
        dev = cov.conn_len.device
        candidates, made = _uploaded_i32(candidates, dev)
        candidates = candidates.reshape(-1)
        n, max_cull, cap = int(candidates.numel()), int(max_cull), int(reparent_cap)
        cp = _i32_ptr("cull_keyframes: candidates", candidates) if n else None
        nb = None if neighbours is None else _i32_ptr("cull_keyframes: neighbours", neighbours, cov.max_keyframes * KF_NEIGHBOURS)
        shapes = dict(decision=(n,), n_mps=(n,), n_redundant=(n,), culled_slot=(max(max_cull, 0),), reparent_out=(max(cap, 0), 2), counts=(10,))
        gs, tb, cs, vs = graph.struct(), table.struct(), cov.struct(), views.struct()
        keys = ("decision", "n_mps", "n_redundant", "culled_slot", "reparent_out", "counts")
        args = [C.byref(gs), C.byref(tb), C.byref(cs), C.byref(vs), C.byref(state), int(bool(monocular)), int(first_slot), n, cp, max_cull, nb, cap, *keys]
        out = self._run_outputs("cull_keyframes", args, keys, shapes, out, dev, sync or apply, wait, made)
        out["candidates"] = candidates           # (kept alive with the result: the device reads it after the call returns)
        if apply:
            culled = [int(s) for s in out["culled_slot_host"] if s >= 0]
            if culled:
                parent, st, key = graph.parent.cpu().numpy(), graph.state.cpu().numpy(), graph.order_key.cpu().numpy()
                rec = out["reparent_out_host"][:min(int(out["counts_host"][8]), cap)]
                touched = set(culled) | {int(p) for p in rec[:, 1]} | {int(parent[s]) for s in culled}
                for p in sorted(t for t in touched if 0 <= t < graph.max_keyframes):
                    kids = [] if p in culled else [int(s) for s in np.nonzero((parent[:graph.max_keyframes] == p) & (st[:graph.max_keyframes] == KF_GOOD))[0]]
                    graph.set_children(p, sorted(kids, key=lambda s: (int(key[s]), s)))
                if database is not None:
                    for s in culled:
                        database.erase(s)
            out["culled"] = culled
        return out

    def cull_keyframes_stats(self):
        """dict of CULL_COUNTS of the last cull_keyframes (waits for it)"""
        v = np.zeros(10, np.int32)
        self._chk(self._lib.jsorb_cull_keyframes_stats(self._m, v.ctypes.data))
        return dict(zip(CULL_COUNTS, (int(x) for x in v)))

    # ---- Fuse applied to the map: ORBmatcher::Fuse with MapPoint::Replace / AddObservation (ORBmatcher.cpp:812-1087, MapPoint.cpp:208-246) ----
    def fuse_map(self, params, graph, table, kp, state, list_row, target_slots, Rcw, tcw, Ow, replace_loop=False, log_cap=None, sync=False, wait=True,
                 out=None):
        """jsorb_fuse_map*: Fuse with its map mutations of the points `list_row` (an int32 device tensor of table rows, -1 = NULL, or a host
        sequence that is uploaded) into the keyframes `target_slots` (HOST sequence of slots, at most 256) one after the other, on the device state:
        graph a KeyframeGraph, table a MapPointTable, kp a KeyframeKeypoints, state a fuse_state(graph, table, ...).  params from make_fuse_params:
        check_reprojection picks the overload (False: the one with Scw, whose Replace loop runs with replace_loop=True); Rcw host float32[T, 9]
        row-major, tcw and Ow host float32[T, 3].  log_cap: records the log holds (default T x n).  Returns a dict of device tensors: best_idx,
        best_dist, replace_point int32[T, n], n_fused int32[T], log int32[log_cap, 4] (-1 padded: (EV_REPLACE, p, q, -1) and (EV_ADD_MAP_POINT,
        row, slot, keypoint) in the order they were made), counts int32[10] (FUSE_MAP_COUNTS); with sync=True the same as numpy arrays under
        *_host.  out: the dict of an earlier call with the same sizes, written again.  The call waits for the current torch stream before it
        enqueues, except with wait=False, out given and list_row a device tensor: then it makes no tensor, waits for nothing and only enqueues -
        the form a graph capture takes (the targets and their poses are host values: a replay runs the captured ones)."""
        what = "fuse_map"
        if not isinstance(params, JsorbFuseParams):
            raise JsorbError("%s: params must come from make_fuse_params" % what)
        dev = graph.point_pool.device
        list_row, made = _uploaded_i32(list_row, dev)
        list_row = list_row.reshape(-1)
        n = int(list_row.numel())
        lp = _i32_ptr("%s: list_row" % what, list_row) if n else None
        ts = np.ascontiguousarray(target_slots, np.int32).reshape(-1)
        T = len(ts)
        R, t, O = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (Rcw, tcw, Ow))
        if len(R) != 9 * T or len(t) != 3 * T or len(O) != 3 * T:
            raise JsorbError("%s: Rcw must hold 9, tcw 3 and Ow 3 floats per target" % what)
        cap = max(T * n, 1) if log_cap is None else int(log_cap)
        shapes = dict(best_idx=(T, n), best_dist=(T, n), replace_point=(T, n), n_fused=(T,), log=(max(cap, 0), 4), counts=(10,))
        gs, tb, ks = graph.struct(), table.struct(), kp.struct()
        args = [C.byref(params), int(bool(replace_loop)), C.byref(gs), C.byref(tb), C.byref(ks), C.byref(state), n, lp, T, ts.ctypes.data, R.ctypes.data,
                t.ctypes.data, O.ctypes.data, "best_idx", "best_dist", "replace_point", "n_fused", cap, "log", "counts"]
        out = self._run_outputs(what, args, FUSE_MAP_OUTPUTS, shapes, out, dev, sync, wait, made)
        out["list_row"] = list_row               # (kept alive with the result: the device reads it after the call returns)
        return out

    def fuse_map_host(self, params, graph, table, kp, state, list_row, target_slots, Rcw, tcw, Ow, replace_loop=False, log_cap=None):
        """jsorb_fuse_map, the synchronous form: the same inputs, the outputs as numpy arrays (one copy back) under the keys of FUSE_MAP_OUTPUTS"""
        out = self.fuse_map(params, graph, table, kp, state, list_row, target_slots, Rcw, tcw, Ow, replace_loop=replace_loop, log_cap=log_cap, sync=True)
        return {k: out[k + "_host"] for k in FUSE_MAP_OUTPUTS}

    def fuse_map_stats(self):
        """dict of FUSE_MAP_COUNTS of the last fuse_map (waits for it)"""
        v = np.zeros(10, np.int32)
        self._chk(self._lib.jsorb_fuse_map_stats(self._m, v.ctypes.data))
        return dict(zip(FUSE_MAP_COUNTS, (int(x) for x in v)))

    # ---- new map points: the loop of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:243-457) ----
    def create_new_map_points(self, params, graph, table, kp, extra, state, current_slot, n1, run_capacity, neighbour_slots, poses, F12, epipole,
                              ratio_factor, current_kf_id, new_row, log_cap=None, sync=False, wait=True, out=None):
        """jsorb_create_new_map_points*: matching, triangulation and the new rows for the keyframe in `current_slot` (n1 keypoints) against the
        neighbours `neighbour_slots` (HOST sequence of slots in GetBestCovisibilityKeyFrames order, at most 256, each run at most run_capacity
        long) on the device state: graph a KeyframeGraph, table a MapPointTable, kp a KeyframeKeypoints, extra a NewPointKeypoints, state a
        new_point_state(graph, table, ...).  params from make_triangulation_params(check_orientation=False); poses KEYFRAME_POSE_DTYPE[1 + T], the
        current keyframe first; F12 host float32[T, 9], epipole host float32[T, 2]; new_row the free table rows in the order they are used (an
        int32 device tensor, or a host sequence that is uploaded).  log_cap: records the log holds (default len(new_row)).  Returns a dict of device
        tensors: verdict int32[T, n1], path uint8[T, n1], x3D float32[T, n1, 3], log int32[log_cap, 4] (-1 padded: (row, idx1, neighbour, idx2) per
        owning pair), counts int32[12] (NEW_POINTS_COUNTS); with sync=True the same as numpy arrays under *_host.  out: the dict of an earlier
        call with the same sizes, written again.  The call waits for the current torch stream before it enqueues, except with wait=False, out
        given and new_row a device tensor: then it makes no tensor, waits for nothing and only enqueues - the form a graph capture takes."""
        import torch
        what = "create_new_map_points"
        if not isinstance(params, JsorbTriangulationParams):
            raise JsorbError("%s: params must come from make_triangulation_params" % what)
        dev = graph.point_pool.device
        new_row, made = _uploaded_i32(new_row, dev)
        new_row = new_row.reshape(-1)
        n_new = int(new_row.numel())
        rp = _i32_ptr("%s: new_row" % what, new_row) if n_new else None
        ns = np.ascontiguousarray(neighbour_slots, np.int32).reshape(-1)
        T, n1 = len(ns), int(n1)
        ps = np.ascontiguousarray(poses, KEYFRAME_POSE_DTYPE).reshape(-1)
        F, ep = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (F12, epipole))
        if len(ps) != T + 1 or len(F) != 9 * T or len(ep) != 2 * T:
            raise JsorbError("%s: poses must hold 1 + T records, F12 9 and epipole 2 floats per neighbour" % what)
        cap = n_new if log_cap is None else int(log_cap)
        shapes = dict(verdict=(T, n1), path=(T, n1), x3D=(T, n1, 3), log=(max(cap, 0), 4), counts=(12,))
        dtypes = dict(verdict=torch.int32, path=torch.uint8, x3D=torch.float32, log=torch.int32, counts=torch.int32)
        size = {k: int(np.prod(shapes[k])) for k in NEW_POINTS_OUTPUTS}
        made = made or out is None
        bufs = out["_bufs"] if out is not None else {k: torch.empty(max(size[k], 1), dtype=dtypes[k], device=dev) for k in NEW_POINTS_OUTPUTS}
        gs, tb, ks, es = graph.struct(), table.struct(), kp.struct(), extra.struct()
        args = [self._m, C.byref(params), C.byref(gs), C.byref(tb), C.byref(ks), C.byref(es), C.byref(state), int(current_slot), n1, int(run_capacity), T,
                ns.ctypes.data, ps.ctypes.data, F.ctypes.data, ep.ctypes.data, float(ratio_factor), int(current_kf_id), n_new, rp, cap] + \
               [bufs[k].data_ptr() for k in NEW_POINTS_OUTPUTS]
        if wait or sync or made:
            torch.cuda.current_stream(dev).synchronize()     # (tensors were made on it)
        out = {k: bufs[k][:size[k]].reshape(shapes[k]) for k in NEW_POINTS_OUTPUTS}
        out["_bufs"] = bufs
        out["new_row"] = new_row                 # (kept alive with the result: the device reads it after the call returns)
        if sync:
            np_dtypes = dict(verdict=np.int32, path=np.uint8, x3D=np.float32, log=np.int32, counts=np.int32)
            host = {k: np.zeros(max(size[k], 1), np_dtypes[k]) for k in NEW_POINTS_OUTPUTS}
            self._chk(self._lib.jsorb_create_new_map_points(*args, *[host[k].ctypes.data for k in NEW_POINTS_OUTPUTS]))
            out.update({k + "_host": host[k][:size[k]].reshape(shapes[k]) for k in NEW_POINTS_OUTPUTS})
        else:
            self._chk(self._lib.jsorb_create_new_map_points_async(*args))
            if wait:
                self.sync()
        return out

    def create_new_map_points_host(self, *args, **kw):
        """jsorb_create_new_map_points, the synchronous form: the same inputs, the outputs as numpy arrays under the keys of NEW_POINTS_OUTPUTS"""
        out = self.create_new_map_points(*args, sync=True, **kw)
        return {k: out[k + "_host"] for k in NEW_POINTS_OUTPUTS}

    def create_new_map_points_stats(self):
        """dict of NEW_POINTS_COUNTS of the last create_new_map_points (waits for it)"""
        v = np.zeros(12, np.int32)
        self._chk(self._lib.jsorb_create_new_map_points_stats(self._m, v.ctypes.data))
        return dict(zip(NEW_POINTS_COUNTS, (int(x) for x in v)))


def new_points_build_caps():
    """jsorb_create_new_map_points_build_caps of the loaded library: the pairs per chunk of the order-preserving compaction"""
    return _build_caps("create_new_map_points", 1)


def fuse_map_build_caps():
    """jsorb_fuse_map_build_caps of the loaded library: the entries of an observation list staged at a time"""
    return _build_caps("fuse_map", 1)


def cull_keyframes_build_caps():
    """jsorb_cull_keyframes_build_caps of the loaded library: the most candidates and the largest max_cull of one call"""
    return _build_caps("cull_keyframes", 2)


def covisibility_build_caps():
    """jsorb_covisibility_build_caps of the loaded library: the smallest and the largest conn_capacity"""
    return _build_caps("covisibility", 2)


def kfdb_build_caps():
    """jsorb_kfdb_build_caps of the loaded library: (query entries k_kfdb stages in LDS, word ids jsorb_bow_vector_async sorts in LDS)"""
    return _build_caps("kfdb", 2)


def vocab_train_build_caps():
    """jsorb_vocab_train_build_caps of the loaded library: (positions per chunk of k_vocab_train, chunk sums its scan takes per tile)"""
    return _build_caps("vocab_train", 2)


def pose_optimization_build_caps():
    """jsorb_pose_optimization_build_caps of the loaded library: (threads of a problem's workgroup, edges a thread keeps in registers)"""
    return _build_caps("pose_optimization", 2)


def local_map_build_caps():
    """jsorb_local_map_build_caps of the loaded library: entries per chunk of k_local_map's compaction"""
    return _build_caps("local_map", 1)


def local_keyframes_build_caps():
    """jsorb_local_keyframes_build_caps of the loaded library: (slots whose membership bit k_lk_expand keeps in LDS, child candidates it keeps there)"""
    return _build_caps("local_keyframes", 2)


WEIGHTING_TF_IDF, WEIGHTING_TF, WEIGHTING_IDF, WEIGHTING_BINARY = 0, 1, 2, 3     # DBoW2::WeightingType


def train_vocabulary(descriptors, doc_start, k, L, weighting=WEIGHTING_TF_IDF, scoring=0, seed=0, max_iterations=0, stream_ptr=None, device_id=0):
    """jsorb_vocabulary_train (include/jsorb.h): TemplatedVocabulary::create on the device.  descriptors: uint8[n, 32], a contiguous torch device
    tensor (16-byte aligned) or a numpy array, which is uploaded; doc_start: n_docs + 1 ascending offsets from 0 to n (host).  Returns the tree
    as the dict jetson_slam_amd.vocabulary builds (n_nodes, depth_L, k, child_start, children, descriptors, word_id, weight: what orb.Vocabulary
    and vocabulary.save_text take) with scoring, weighting, parent, Ni (per node), leaf (the node each descriptor's associations ended in) and the
    statistics n_words, n_kmeans_runs, n_draws, n_empty_clusters, n_unconverged, lloyd_passes (per level).  stream_ptr: a hipStream_t to enqueue
    on (None: the null stream); the call waits for the current torch stream before it starts and for its own work before it returns."""
    import torch
    lib = load_library()
    if isinstance(descriptors, np.ndarray):
        descriptors = torch.from_numpy(np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)).to(torch.device("cuda", device_id))
    if not getattr(descriptors, "is_cuda", False) or descriptors.dtype != torch.uint8:
        raise JsorbError("train_vocabulary: descriptors must be a uint8 device tensor or a numpy array")
    if descriptors.dim() != 2 or descriptors.shape[1] != 32 or not descriptors.is_contiguous():
        raise JsorbError("train_vocabulary: descriptors must be contiguous, of shape (n, 32)")
    n = int(descriptors.shape[0])
    ds = np.ascontiguousarray(doc_start, np.int32)
    if ds.ndim != 1 or len(ds) < 1:
        raise JsorbError("train_vocabulary: doc_start must hold n_docs + 1 offsets")
    torch.cuda.current_stream(descriptors.device).synchronize()
    res = C.c_void_p()
    rc = lib.jsorb_vocabulary_train(descriptors.device.index or 0, stream_ptr, descriptors.data_ptr() if n else None, n, ds.ctypes.data, len(ds) - 1,
                                    int(k), int(L), int(weighting), int(scoring), int(seed) & (2 ** 64 - 1), int(max_iterations), C.byref(res))
    if rc != 0:
        raise JsorbError("jsorb_vocabulary_train rc=%d: %s" % (rc, lib.jsorb_vocabulary_train_last_error().decode()))
    try:
        v = [C.c_int() for _ in range(7)]
        lib.jsorb_vocab_train_result_info(res, *[C.byref(x) for x in v])
        nn, n_words = v[0].value, v[1].value
        t = dict(n_nodes=nn, n_words=n_words, depth_L=int(L), k=int(k), scoring=int(scoring), weighting=int(weighting),
                 parent=np.zeros(nn, np.int32), child_start=np.zeros(nn + 1, np.int32), children=np.zeros(nn - 1, np.int32),
                 descriptors=np.zeros((nn, 32), np.uint8), word_id=np.zeros(nn, np.int32), weight=np.zeros(nn, np.float64), Ni=np.zeros(nn, np.int32),
                 leaf=np.zeros(n, np.int32))
        lib.jsorb_vocab_train_result_copy(res, *[t[key].ctypes.data for key in ("parent", "child_start", "children", "descriptors", "word_id", "weight", "Ni")])
        lib.jsorb_vocab_train_result_copy_assignment(res, t["leaf"].ctypes.data)
        runs, draws, empty, unconv, passes = C.c_int(), C.c_longlong(), C.c_int(), C.c_int(), np.zeros(16, np.int32)
        lib.jsorb_vocab_train_stats(res, C.byref(runs), C.byref(draws), C.byref(empty), C.byref(unconv), passes.ctypes.data)
        t.update(n_kmeans_runs=runs.value, n_draws=draws.value, n_empty_clusters=empty.value, n_unconverged=unconv.value, lloyd_passes=[int(x) for x in passes])
    finally:
        lib.jsorb_vocab_train_result_destroy(res)
    return t


class KeyframeDatabase:
    """jsorb_keyframe_database: KeyFrameDatabase's BoW queries on the device (include/jsorb.h), with a stream and scratch of its own.
    word_weight: the leaves' weights by word id (a host array of double), or an orb.Vocabulary, whose word_weight is taken.  A BowVector is the
    triple (word int32[cap], value float64[cap], count int32[1]) of device tensors bow_vector returns.  wait (every call): True waits for the
    current torch stream before the call and for the database's stream after it; False only enqueues."""
    STATE_KEYS = ("present", "loop_query", "reloc_query", "loop_words", "reloc_words", "loop_score", "reloc_score")
    STATE_TYPES = (np.int32, np.uint64, np.uint64, np.int32, np.int32, np.float32, np.float32)

    def __init__(self, word_weight, max_keyframes, device_id=0):
        self._lib = load_library()
        self._d = C.c_void_p()
        w = np.ascontiguousarray(getattr(word_weight, "word_weight", word_weight), np.float64)
        rc = self._lib.jsorb_keyframe_database_create(int(device_id), int(max_keyframes), len(w), w.ctypes.data, C.byref(self._d))
        if rc != 0:
            self._d = C.c_void_p()
            raise JsorbError("jsorb_keyframe_database_create rc=%d" % rc)
        self.device_id, self.max_keyframes, self.n_words = int(device_id), int(max_keyframes), len(w)

    @property
    def handle(self):
        return self._d

    def close(self):
        if getattr(self, "_d", None):
            self._lib.jsorb_keyframe_database_destroy(self._d)
            self._d = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise JsorbError("libjsorb rc=%d: %s" % (rc, self._lib.jsorb_keyframe_database_last_error(self._d).decode()))

    def set_stream(self, stream_ptr):
        """use an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None restores the database's own"""
        self._chk(self._lib.jsorb_keyframe_database_set_stream(self._d, stream_ptr))

    def get_stream(self):
        return self._lib.jsorb_keyframe_database_get_stream(self._d) or 0

    def sync(self):
        rc = self._lib.jsorb_mem_stream_sync(C.c_void_p(self.get_stream()))
        if rc != 0:
            raise JsorbError("KeyframeDatabase.sync: jsorb_mem_stream_sync rc=%d" % rc)

    def size(self):
        return self._lib.jsorb_keyframe_database_size(self._d)

    def _dev(self):
        import torch
        return torch.device("cuda", self.device_id)

    def _run(self, wait, fn, *args):
        import torch
        if wait:
            torch.cuda.current_stream(self._dev()).synchronize()
        self._chk(fn(self._d, *args))
        if wait:
            self.sync()

    @staticmethod
    def _tensor(what, t, dtype, n=None):
        import torch
        if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False) or t.dtype != dtype or not t.is_contiguous() or t.dim() != 1 or \
                (n is not None and t.numel() != n):
            raise JsorbError("KeyframeDatabase: %s must be a contiguous 1-d %s device tensor%s" % (what, dtype, "" if n is None else " of %d entries" % n))
        return t

    def _vec(self, vec):
        import torch
        word, value, count = vec
        self._tensor("a BowVector's word", word, torch.int32)
        self._tensor("a BowVector's value", value, torch.float64, word.numel())
        self._tensor("a BowVector's count", count, torch.int32, 1)
        cap = word.numel()
        return [word.data_ptr() if cap else None, value.data_ptr() if cap else None, cap, count.data_ptr()]

    def bow_vector(self, word_ids, n=None, wait=True):
        """jsorb_bow_vector_async: word ids (an int32 device tensor; or a raw device pointer of n entries, e.g. ORBExtractor.bow_device_pointers'
        first) -> (word, value, count)"""
        import torch
        if isinstance(word_ids, int):
            ptr, n = word_ids, int(n)
        else:
            self._tensor("word_ids", word_ids, torch.int32)
            ptr, n = word_ids.data_ptr(), word_ids.numel()
        word = torch.full((n,), -7, dtype=torch.int32, device=self._dev())
        value = torch.full((n,), -7.0, dtype=torch.float64, device=self._dev())
        count = torch.full((1,), -7, dtype=torch.int32, device=self._dev())
        self._run(wait, self._lib.jsorb_bow_vector_async, ptr if n else None, n, word.data_ptr() if n else None,
                  value.data_ptr() if n else None, count.data_ptr())
        return word, value, count

    def add(self, slot, vec, wait=True):
        self._run(wait, self._lib.jsorb_keyframe_database_add_async, int(slot), *self._vec(vec))

    def erase(self, slot):
        self._chk(self._lib.jsorb_keyframe_database_erase(self._d, int(slot)))

    def clear(self):
        self._chk(self._lib.jsorb_keyframe_database_clear(self._d))

    def score(self, vec, slots, f64=True, wait=True):
        """jsorb_keyframe_database_score_async over the int32 device tensor `slots` -> (score float32[n], score_f64 float64[n] or None,
        min_score float32[1]) device tensors"""
        import torch
        self._tensor("slots", slots, torch.int32)
        n = slots.numel()
        score = torch.full((n,), -7.0, dtype=torch.float32, device=self._dev())
        score64 = torch.full((n,), -7.0, dtype=torch.float64, device=self._dev()) if f64 else None
        mn = torch.full((1,), -7.0, dtype=torch.float32, device=self._dev())
        self._run(wait, self._lib.jsorb_keyframe_database_score_async, *self._vec(vec), slots.data_ptr() if n else None, n, score.data_ptr() if n else None,
                  score64.data_ptr() if f64 and n else None, mn.data_ptr())
        return score, score64, mn

    def _neighbours(self, neighbours):
        import torch
        if not hasattr(neighbours, "data_ptr") or not getattr(neighbours, "is_cuda", False) or neighbours.dtype != torch.int32 or \
                tuple(neighbours.shape) != (self.max_keyframes, 10) or not neighbours.is_contiguous():
            raise JsorbError("KeyframeDatabase: neighbours must be a contiguous int32 device tensor of shape (%d, 10)" % self.max_keyframes)
        return neighbours.data_ptr()

    def _query(self, name, args, wait, sync):
        import torch
        if sync:
            out, n = np.full(self.max_keyframes, -7, np.int32), C.c_int(-7)
            torch.cuda.current_stream(self._dev()).synchronize()
            self._chk(getattr(self._lib, name)(self._d, *args, out.ctypes.data, C.byref(n)))
            return out[:n.value].copy()
        cand = torch.full((self.max_keyframes,), -7, dtype=torch.int32, device=self._dev())
        n = torch.full((1,), -7, dtype=torch.int32, device=self._dev())
        self._run(wait, getattr(self._lib, name + "_async"), *args, cand.data_ptr(), n.data_ptr())
        return cand, n

    def detect_loop_candidates(self, vec, query_id, neighbours, min_score=0.0, connected=None, wait=True, sync=False):
        """jsorb_detect_loop_candidates_async -> (candidates int32[max_keyframes], count int32[1]) device tensors; sync=True: the synchronous
        form, a host array of the candidates.  min_score: a number, or a float32[1] device tensor (score()'s third output, no wait in between).
        connected: a uint8 / bool device tensor of max_keyframes entries, or None."""
        import torch
        dev_min = hasattr(min_score, "data_ptr")
        if dev_min:
            self._tensor("min_score", min_score, torch.float32, 1)
        if connected is not None:
            if connected.dtype == torch.bool:
                connected = connected.view(torch.uint8)
            self._tensor("connected", connected, torch.uint8, self.max_keyframes)
        args = self._vec(vec) + [C.c_uint64(int(query_id)), connected.data_ptr() if connected is not None else None, self._neighbours(neighbours),
                                 0.0 if dev_min else float(min_score), min_score.data_ptr() if dev_min else None]
        return self._query("jsorb_detect_loop_candidates", args, wait, sync)

    def detect_relocalization_candidates(self, vec, query_id, neighbours, wait=True, sync=False):
        """jsorb_detect_relocalization_candidates_async, as detect_loop_candidates"""
        args = self._vec(vec) + [C.c_uint64(int(query_id)), self._neighbours(neighbours)]
        return self._query("jsorb_detect_relocalization_candidates", args, wait, sync)

    def stats(self):
        """jsorb_detect_candidates_stats of the last query: dict(n_sharing, max_common, min_common, n_scored, n_kept, best_acc, n_candidates)"""
        v = [C.c_int() for _ in range(5)]
        best, n = C.c_float(), C.c_int()
        self._chk(self._lib.jsorb_detect_candidates_stats(self._d, *[C.byref(t) for t in v], C.byref(best), C.byref(n)))
        out = dict(zip(("n_sharing", "max_common", "min_common", "n_scored", "n_kept"), (t.value for t in v)))
        out.update(best_acc=np.float32(best.value), n_candidates=n.value)
        return out

    def state(self):
        """jsorb_keyframe_database_copy_state: dict of host arrays of max_keyframes entries (STATE_KEYS)"""
        out = {k: np.zeros(self.max_keyframes, t) for k, t in zip(self.STATE_KEYS, self.STATE_TYPES)}
        self._chk(self._lib.jsorb_keyframe_database_copy_state(self._d, *[out[k].ctypes.data for k in self.STATE_KEYS]))
        return out


def matched_pairs(match12_row):
    """vMatchedPairs of ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:799-807) from one row of match12: int64[k, 2] of (idx1, idx2), ascending idx1"""
    row = np.asarray(match12_row)
    idx1 = np.nonzero(row >= 0)[0]
    return np.stack([idx1, row[idx1]], axis=1).astype(np.int64) if len(idx1) else np.zeros((0, 2), np.int64)


class ORBExtractor:
    """Mirror of Jetson_SLAM::ORBExtractor (include/ORBextractor.h:21-93) over the C ABI.

    Argument order and meaning are the reference constructor's; `use_gpu` is accepted and ignored exactly as the
    reference does (src/ORBextractor.cpp:75-87 always builds the GPU object).  `max_batch` and `device_id` are additions.
    """

    def __init__(self, im_height, im_width, scale_factor, n_levels, FAST_N_MIN, FAST_N_MAX, th_FAST_MIN, th_FAST_MAX,
                 str_mask=None, tile_h=30, tile_w=30, fixed_multi_scale_tile_size=False, apply_nms_ms=False,
                 nms_ms_mode_gpu=False, use_gpu=True, device_id=0, max_batch=1):
        self._lib = load_library()
        self._h = C.c_void_p()
        mask = None
        if isinstance(str_mask, str) and str_mask:
            # the reference's image path (None = unreadable = no mask, orb_gpu.cpp:69-73); whatever size the image has, every level is
            # resized from it directly with INTER_NN (orb_gpu.cpp:77-81): it goes through the ABI at its own size
            mask = read_mask_image(str_mask)
        elif str_mask is not None and not isinstance(str_mask, str):
            mask = np.ascontiguousarray(str_mask, np.uint8)   # a 2-D array (any size) instead of the reference's image path
            assert mask.ndim == 2
        self.params = JsorbParams(im_height, im_width, n_levels, scale_factor, FAST_N_MIN, FAST_N_MAX, th_FAST_MIN,
                                  th_FAST_MAX, tile_h, tile_w, int(fixed_multi_scale_tile_size), int(apply_nms_ms),
                                  int(nms_ms_mode_gpu), device_id, max_batch)
        if mask is None:
            rc = self._lib.jsorb_create(C.byref(self.params), None, C.byref(self._h))
        else:
            rc = self._lib.jsorb_create_masked(C.byref(self.params), mask.ctypes.data, int(mask.shape[1]), int(mask.shape[0]), C.byref(self._h))
        if rc != 0:
            msg = self._lib.jsorb_last_error(self._h).decode() if self._h else "jsorb_create failed"
            if self._h:
                self._lib.jsorb_destroy(self._h)
                self._h = C.c_void_p()
            raise JsorbError("jsorb_create rc=%d: %s" % (rc, msg))
        self.n_levels_ = n_levels
        self.scale_factor_ = np.float32(scale_factor)
        # scale tables for the SLAM side (src/ORBextractor.cpp:43-71), float32 arithmetic as in the reference
        s = np.ones(n_levels, np.float32)
        for i in range(1, n_levels):
            s[i] = np.float32(s[i - 1] * self.scale_factor_)
        self.scale_ = s
        self.level_sigma2_ = (s * s).astype(np.float32)
        self.level_sigma2_[0] = np.float32(1.0)
        self.inv_scale_ = (np.float32(1.0) / s).astype(np.float32)
        self.inv_level_sigma2_ = (np.float32(1.0) / self.level_sigma2_).astype(np.float32)
        self.T = self._lib.jsorb_total_tiles(self._h)
        self.max_batch = max_batch
        self._keep = None

    # ---- reference getters ----
    def get_levels(self):
        return self.n_levels_

    def get_scale_factor(self):
        return float(self.scale_factor_)

    def get_scale_factors(self):
        return self.scale_.copy()

    def get_inverse_scale_factors(self):
        return self.inv_scale_.copy()

    def get_scale_sigma_squares(self):
        return self.level_sigma2_.copy()

    def get_inverse_scale_sigma_squares(self):
        return self.inv_level_sigma2_.copy()

    # ---- helpers ----
    def _chk(self, rc):
        if rc != 0:
            raise JsorbError("libjsorb rc=%d: %s" % (rc, self._lib.jsorb_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.jsorb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def launch_forms(self):
        """jsorb_handle_forms: the kernel forms this handle runs (FORM_KEYS) and the lane schedule of its last extract call (LANE_KEYS;
        lanes = 0 and lane_order = -1 before the first one)"""
        out = np.zeros(len(FORM_KEYS) + len(LANE_KEYS), np.int32)
        self._chk(self._lib.jsorb_handle_forms(self._h, out.ctypes.data, out.size))
        return dict(zip(FORM_KEYS + LANE_KEYS, (int(v) for v in out)))

    # ---- extraction ----
    def extract(self, image):
        """ORBExtractor::extract: one host image -> (keypoints int32[6N] SoA, descriptors uint8[N,32]) pulled to the host
        (the reference leaves them in SyncedMem and the Frame ctor calls to_cpu(), Frame.cpp:119-122)."""
        image = np.ascontiguousarray(image, np.uint8)
        assert image.shape == (self.params.height, self.params.width)
        n = C.c_int()
        self._chk(self._lib.jsorb_extract(self._h, image.ctypes.data, image.strides[0], C.byref(n)))
        return self.keypoints(0), self.descriptors(0)

    def extract_batch_device_async(self, dev_ptr, image_stride, step, n_images, keep=None):
        """Batch mode on images already resident in HBM (raw device pointer). `keep` pins a Python owner of the memory."""
        self._keep = keep
        self._chk(self._lib.jsorb_extract_batch_device_async(self._h, dev_ptr, image_stride, step, n_images))

    def extract_batch_host_async(self, images):
        images = np.ascontiguousarray(images, np.uint8)
        assert images.ndim == 3 and images.shape[1:] == (self.params.height, self.params.width)
        self._keep = images
        self._chk(self._lib.jsorb_extract_batch_host_async(self._h, images.ctypes.data, images.strides[0], images.strides[1],
                                                           images.shape[0]))

    def sync(self):
        self._chk(self._lib.jsorb_sync(self._h))

    def n_keypoints(self, image=0):
        return self._lib.jsorb_n_keypoints(self._h, image)

    def level_n_keypoints(self, image=0):
        return [self._lib.jsorb_level_n_keypoints(self._h, image, l) for l in range(self.n_levels_)]

    def keypoints(self, image=0):
        n = self.n_keypoints(image)
        if n < 0:
            raise JsorbError("no extract result for image %d" % image)
        out = np.zeros(6 * n, np.int32)
        if n:
            self._chk(self._lib.jsorb_copy_keypoints(self._h, image, out.ctypes.data))
        return out

    def descriptors(self, image=0):
        n = self.n_keypoints(image)
        out = np.zeros((n, 32), np.uint8)
        if n:
            self._chk(self._lib.jsorb_copy_descriptors(self._h, image, out.ctypes.data))
        return out

    def unpack_frame(self, image=0):
        """Frame.cpp:119-196 on the device: (keypoints as a structured array with the layout of cv::KeyPoint, descriptors N x 32)."""
        n = self.n_keypoints(image)
        if n < 0:
            raise JsorbError("no extract result for image %d" % image)
        kps = np.zeros(n, KEYPOINT_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        if n:
            self._chk(self._lib.jsorb_unpack_frame(self._h, image, kps.ctypes.data, desc.ctypes.data))
        return kps, desc

    def assign_features_to_grid(self, min_x, min_y, grid_element_width_inv, grid_element_height_inv, cols=64, rows=48, image=0):
        """Frame::AssignFeaturesToGrid (Frame.cpp:463-479) as CSR: (cell_start[cols*rows+1], cell_items); cell (i, j) = i*rows + j."""
        n = self.n_keypoints(image)
        if n < 0:
            raise JsorbError("no extract result for image %d" % image)
        start = np.zeros(cols * rows + 1, np.int32)
        items = np.zeros(max(n, 1), np.int32)
        self._chk(self._lib.jsorb_assign_features_to_grid(self._h, image, min_x, min_y, grid_element_width_inv, grid_element_height_inv,
                                                          cols, rows, start.ctypes.data, items.ctypes.data))
        return start, items[:start[-1]]

    def angles(self, image=0):
        n = self.n_keypoints(image)
        out = np.zeros(n, np.float32)
        if n:
            self._chk(self._lib.jsorb_copy_angles(self._h, image, out.ctypes.data))
        return out

    def level_dims(self):
        res = []
        for l in range(self.n_levels_):
            h, w, p = C.c_int(), C.c_int(), C.c_int()
            self._chk(self._lib.jsorb_level_dims(self._h, l, C.byref(h), C.byref(w), C.byref(p)))
            res.append((h.value, w.value))
        return res

    def level_tiles(self):
        res = []
        for l in range(self.n_levels_):
            v = [C.c_int() for _ in range(5)]
            self._chk(self._lib.jsorb_level_tiles(self._h, l, *[C.byref(t) for t in v]))
            res.append(tuple(t.value for t in v))   # (tile_h, tile_w, n_tile_h, n_tile_w, level_offset)
        return res

    def level_image(self, level, image=0, blurred=False):
        h, w = self.level_dims()[level]
        out = np.zeros((h, w), np.uint8)
        self._chk(self._lib.jsorb_copy_level_image(self._h, image, level, int(blurred), out.ctypes.data))
        return out

    def level_mask(self, level):
        """ORB_GPU::masks_[level] (orb_gpu.cpp:64-91): 0 / 255 plane of the level"""
        h, w = self.level_dims()[level]
        out = np.zeros((h, w), np.uint8)
        self._chk(self._lib.jsorb_copy_level_mask(self._h, level, out.ctypes.data))
        return out

    def tile_candidates(self, image=0):
        x, y, s = (np.zeros(self.T, np.int32) for _ in range(3))
        self._chk(self._lib.jsorb_copy_tile_candidates(self._h, image, x.ctypes.data, y.ctypes.data, s.ctypes.data))
        return x, y, s

    # ---- rectification of raw input (Examples/Stereo/stereo_euroc.cpp:106-107, 145-146) ----
    def set_rectify_maps(self, mapx, mapy):
        """From now on every extract reads RAW images and level 0 is cv::remap(raw, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT 0) computed on the
        device.  float32 (H, W) maps of the handle's image size.  A set-up call (waits for the handle's work), not a per-frame one."""
        mapx = np.ascontiguousarray(mapx, np.float32)
        mapy = np.ascontiguousarray(mapy, np.float32)
        assert mapx.shape == mapy.shape and mapx.ndim == 2
        self._chk(self._lib.jsorb_set_rectify_maps(self._h, mapx.ctypes.data, mapy.ctypes.data, mapx.shape[1], mapx.shape[0], mapx.shape[1]))

    def set_rectify_maps_fixed(self, xy, a):
        """The same from maps in cv::convertMaps' fixed-point form: xy int16 (H, W, 2), a uint16 (H, W)."""
        xy = np.ascontiguousarray(xy, np.int16)
        a = np.ascontiguousarray(a, np.uint16)
        assert xy.ndim == 3 and xy.shape[2] == 2 and a.shape == xy.shape[:2]
        self._chk(self._lib.jsorb_set_rectify_maps_fixed(self._h, xy.ctypes.data, a.ctypes.data, a.shape[1], a.shape[0], a.shape[1], a.shape[1]))

    def clear_rectify_maps(self):
        self._chk(self._lib.jsorb_clear_rectify_maps(self._h))

    def rectify_enabled(self):
        rc = self._lib.jsorb_rectify_enabled(self._h)
        if rc < 0:
            self._chk(rc)
        return bool(rc)

    # ---- camera: Frame::UndistortKeyPoints (Frame.cpp:718-748) on the device ----
    def set_camera(self, K, D):
        """Tracking's mK / mDistCoef: from now on every extract also undistorts its keypoints (k_undistort) when k1 != 0; a set-up call"""
        cam = make_camera(K, D)
        self._chk(self._lib.jsorb_set_camera(self._h, C.byref(cam)))

    def clear_camera(self):
        self._chk(self._lib.jsorb_set_camera(self._h, None))

    def camera_enabled(self):
        rc = self._lib.jsorb_camera_enabled(self._h)
        if rc < 0:
            self._chk(rc)
        return bool(rc)

    def keypoints_undistorted(self, image=0):
        """mvKeysUn coordinates: (x_un float32[N], y_un float32[N]) - the keypoint coordinates without an active camera"""
        n = self.n_keypoints(image)
        if n < 0:
            raise JsorbError("no extract result for image %d" % image)
        out = np.zeros(2 * n, np.float32)
        if n:
            self._chk(self._lib.jsorb_copy_keypoints_un(self._h, image, out.ctypes.data))
        return out[:n].copy(), out[n:].copy()

    def unpack_frame_undistorted(self, image=0):
        """(mvKeys, mvKeysUn as cv::KeyPoint-shaped structured arrays, descriptors N x 32) with one synchronisation"""
        n = self.n_keypoints(image)
        if n < 0:
            raise JsorbError("no extract result for image %d" % image)
        keys, keys_un = np.zeros(n, KEYPOINT_DTYPE), np.zeros(n, KEYPOINT_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        if n:
            self._chk(self._lib.jsorb_unpack_frame_un(self._h, image, keys.ctypes.data, keys_un.ctypes.data, desc.ctypes.data))
        return keys, keys_un, desc

    def undistort_kernel_time(self):
        """(total_ms, launches) of k_undistort (kernel id K_UNDISTORT), measured like kernel_times()."""
        return self._kernel_time(K_UNDISTORT)

    def rgbd_kernel_time(self):
        return self._kernel_time(K_RGBD)

    def _kernel_time(self, kid):
        ms, n = C.c_double(), C.c_long()
        self._chk(self._lib.jsorb_kernel_time(self._h, kid, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- RGB-D: Frame::ComputeStereoFromRGBD (Frame.cpp:996-1017) with Tracking.cpp:333-334's conversion ----
    def rgbd_depth(self, depth, mbf, factor=1.0, image_stride=None, n_images=None):
        """Host numpy (H, W) uint16 / float32 depth: synchronous, image 0 -> (uRight float32[N], depth float32[N]).
        A device tensor (uint16 / float32, (B, H, W) or (H, W)): image i of the last batch against depth image i, enqueued (read the results with
        rgbd_result after sync()).  factor: Tracking's mDepthMapFactor (already inverted, e.g. 1/5000 for TUM)."""
        if hasattr(depth, "data_ptr"):           # a torch tensor: device memory only, 16-bit (read as uint16) or float32 elements
            if not getattr(depth, "is_cuda", False):
                raise JsorbError("rgbd_depth: a torch tensor must be in device memory (pass host depth as a numpy array)")
            dt = str(depth.dtype)
            if dt in ("torch.uint16", "torch.int16"):
                fmt = DEPTH_U16
            elif dt == "torch.float32":
                fmt = DEPTH_F32
            else:
                raise JsorbError("rgbd_depth: depth must be uint16 / int16 (raw 16-bit) or float32, not %s" % dt)
            if depth.dim() not in (2, 3) or tuple(depth.shape[-2:]) != (self.params.height, self.params.width) or depth.stride(-1) != 1:
                raise JsorbError("rgbd_depth: depth must be (H, W) or (B, H, W) of the handle's image size with dense rows")
            es = depth.element_size()
            H, W = depth.shape[-2], depth.shape[-1]
            n = n_images if n_images is not None else (depth.shape[0] if depth.dim() == 3 else 1)
            if n > (depth.shape[0] if depth.dim() == 3 else 1) and image_stride is None:
                raise JsorbError("rgbd_depth: %d images asked for, the tensor holds fewer" % n)
            stride = image_stride if image_stride is not None else (depth.stride(0) * es if depth.dim() == 3 else H * depth.stride(-2) * es)
            self._keep = (self._keep, depth)
            self._chk(self._lib.jsorb_rgbd_depth_batch_device_async(self._h, depth.data_ptr(), stride, depth.stride(-2) * es, fmt, factor, mbf, n))
            return None
        d = np.asarray(depth)
        if d.dtype == np.uint16:
            fmt = DEPTH_U16
        elif d.dtype == np.float32:
            fmt = DEPTH_F32
        else:
            raise JsorbError("rgbd_depth: depth must be uint16 (raw 16-bit) or float32, not %s" % d.dtype)
        d = np.ascontiguousarray(d)
        assert d.shape == (self.params.height, self.params.width)
        n = self.n_keypoints(0)
        u = np.full(max(n, 1), -1, np.float32)
        dd = np.full(max(n, 1), -1, np.float32)
        self._chk(self._lib.jsorb_rgbd_depth(self._h, d.ctypes.data, fmt, d.strides[0], factor, mbf, u.ctypes.data, dd.ctypes.data))
        return u[:n], dd[:n]

    def rgbd_result(self, image=0):
        n = self.n_keypoints(image)
        u = np.full(max(n, 1), -1, np.float32)
        d = np.full(max(n, 1), -1, np.float32)
        self._chk(self._lib.jsorb_copy_rgbd(self._h, image, u.ctypes.data, d.ctypes.data))
        return u[:n], d[:n]

    # ---- local map matching: ORBmatcher::SearchByProjection(Frame&, map points, th) (ORBmatcher.cpp:32-116) on the device ----
    def search_local_points(self, u, v, invz, predicted_level, view_cos, in_frustum, mp_descriptors, grid, th=1.0, mbf=0.0, u_right=None,
                            blocked=None, nn_ratio=0.8, th_high=TH_HIGH, cols=64, rows=48, image=0):
        """Tracking::SearchLocalPoints' matching step over image `image` of the last extract.  Device tensors, as jsorb_is_in_frustum writes them:
        u, v, invz, view_cos float32[n]; predicted_level int32[n]; in_frustum uint8[n]; mp_descriptors uint8[n, 32]; u_right float32[N] or None
        (monocular); blocked uint8 / bool [N] or None.  grid = (mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv) over cols x rows.
        Returns (match_kp int32[n], match_dist int32[n], kp_match int32[N], n_matches int32[1]) as device tensors; the call waits for the
        current torch stream before it starts and for its own work before it returns."""
        import torch
        n = int(u.shape[0]) if u.dim() == 1 else -1
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("search_local_points: no extract result for image %d" % image)

        def chk(t, name, dtypes, shape):
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("search_local_points: %s must be a device tensor" % name)
            if t.dtype not in dtypes:
                raise JsorbError("search_local_points: %s must be %s, not %s" % (name, " / ".join(str(d) for d in dtypes), t.dtype))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise JsorbError("search_local_points: %s must be a contiguous tensor of shape %s, not %s" % (name, shape, tuple(t.shape)))
            return t.data_ptr()

        if n < 0:
            raise JsorbError("search_local_points: u must be one-dimensional")
        f32, i32, u8 = (torch.float32,), (torch.int32,), (torch.uint8, torch.bool)
        ptrs = [chk(u, "u", f32, (n,)), chk(v, "v", f32, (n,)), chk(invz, "invz", f32, (n,)), chk(predicted_level, "predicted_level", i32, (n,)),
                chk(view_cos, "view_cos", f32, (n,)), chk(in_frustum, "in_frustum", u8, (n,)), chk(mp_descriptors, "mp_descriptors", (torch.uint8,), (n, 32))]
        if n and mp_descriptors.data_ptr() % 16:
            raise JsorbError("search_local_points: mp_descriptors must be 16-byte aligned")
        ptrs.append(None if u_right is None else chk(u_right, "u_right", f32, (N,)))
        ptrs.append(None if blocked is None else chk(blocked, "blocked", u8, (N,)))
        dev = u.device
        match_kp = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        match_dist = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        kp_match = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        prm = JsorbSearchParams(th, nn_ratio, th_high, mbf, grid[0], grid[1], grid[2], grid[3], cols, rows)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_search_local_points_async(self._h, image, C.byref(prm), n, *ptrs, match_kp.data_ptr(), match_dist.data_ptr(),
                                                            kp_match.data_ptr(), count.data_ptr()))
        self.sync()
        return match_kp[:n], match_dist[:n], kp_match[:N], count

    def search_local_stats(self):
        """(fixed-point rounds, candidates, points over the per-point candidate list) of the last search_local_points"""
        r, c, o = C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.jsorb_search_local_stats(self._h, C.byref(r), C.byref(c), C.byref(o)))
        return r.value, c.value, o.value

    def search_local_kernel_times(self):
        """{kernel: (total_ms, launches)} of the grid, candidate and resolve kernels, measured like kernel_times()"""
        return {name: self._kernel_time(k) for name, k in (("k_assign_grid", K_ASSIGN_GRID), ("k_local_candidates", K_LOCAL_CANDIDATES),
                                                           ("k_local_resolve", K_LOCAL_RESOLVE))}

    # ---- the local map: Tracking::UpdateLocalPoints, the frame marks and K16 (Tracking.cpp:1818-1841, :1352-1367, :1410-1420) on the device ----
    def local_map_points(self, table, frustum, kf_start, kf_point_row, frame_point_row, capacity, image=0, sync=False, out=None, wait=True):
        """jsorb_local_map_points*: table a MapPointTable, frustum a JsorbFrustumParams (make_frustum_params), kf_start host ints (n_keyframes + 1),
        kf_point_row int32 device tensor (kf_start[-1] entries), frame_point_row int32[N] device tensor or None.  Returns a dict of device
        tensors with `capacity` entries - point_row, u, v, invz, predicted_level, view_cos, in_frustum, mp_descriptors (capacity x 32) -
        blocked_in uint8[N] and counts int32[5]: the point arguments of search_local_points.  out: the dict of an earlier call, written again
        (nothing is allocated).  sync=True: the synchronous form; the dict also holds point_row_host and counts_host (numpy).  Otherwise the
        call waits for the current torch stream before it starts and for its own work before it returns; wait=False: it only enqueues on the
        handle's stream (the caller orders the streams - the form a graph capture of that stream takes)."""
        import torch
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("local_map_points: no extract result for image %d" % image)
        ks = np.ascontiguousarray(kf_start, np.int32).ravel()
        n_kf = len(ks) - 1
        if n_kf < 0:
            raise JsorbError("local_map_points: kf_start needs n_keyframes + 1 entries")
        dev = table.floats.device
        kp = _i32_ptr("local_map_points: kf_point_row", kf_point_row, int(ks[-1]), flat=True) if n_kf > 0 and ks[-1] > 0 else None
        fp = None if frame_point_row is None else _i32_ptr("local_map_points: frame_point_row", frame_point_row, N, flat=True)
        cap = int(capacity)
        if out is None:
            c1 = max(cap, 1)
            out = dict(point_row=torch.empty(c1, dtype=torch.int32, device=dev)[:max(cap, 0)], predicted_level=torch.empty(c1, dtype=torch.int32, device=dev)[:max(cap, 0)],
                       in_frustum=torch.empty(c1, dtype=torch.uint8, device=dev)[:max(cap, 0)], mp_descriptors=torch.empty((c1, 32), dtype=torch.uint8, device=dev)[:max(cap, 0)],
                       blocked_in=torch.empty(max(N, 1), dtype=torch.uint8, device=dev)[:N], counts=torch.empty(5, dtype=torch.int32, device=dev))
            for k in ("u", "v", "invz", "view_cos"):
                out[k] = torch.empty(c1, dtype=torch.float32, device=dev)[:max(cap, 0)]
        tb = table.struct()
        args = [self._h, image, C.byref(tb), C.byref(frustum), n_kf, ks.ctypes.data, kp, fp, cap] + \
               [out[k].data_ptr() for k in ("point_row", "u", "v", "invz", "predicted_level", "view_cos", "in_frustum", "mp_descriptors", "blocked_in", "counts")]
        if wait or sync:
            torch.cuda.current_stream(dev).synchronize()
        if sync:
            rows_h, counts_h = np.full(max(cap, 1), -2, np.int32), np.zeros(5, np.int32)
            self._chk(self._lib.jsorb_local_map_points(*args, rows_h.ctypes.data, counts_h.ctypes.data))
            out = dict(out, point_row_host=rows_h[:max(cap, 0)], counts_host=counts_h)
        else:
            self._chk(self._lib.jsorb_local_map_points_async(*args))
            if wait:
                self.sync()
        return out

    def local_map_stats(self):
        """dict(n_entries, n_null, n_invalid_rows, n_duplicates, n_bad, n_seen) of the last local_map_points"""
        v = [C.c_int() for _ in range(6)]
        self._chk(self._lib.jsorb_local_map_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_entries", "n_null", "n_invalid_rows", "n_duplicates", "n_bad", "n_seen"), (x.value for x in v)))

    # ---- the frame's pose: Optimizer::PoseOptimization (Optimizer.cpp:244-456) on the device ----
    def pose_optimization(self, table, params, frame_point_row, Tcw, u_right=None, image=0, sync=False, out=None, wait=True, point_rows=True):
        """jsorb_pose_optimization*: table a MapPointTable, params a JsorbPoseParams (make_pose_params), frame_point_row an int32 device tensor
        [n_problems, N] (or [N]: one problem), u_right float32[N] device tensor or None (monocular).  Tcw: float32 [n_problems, 4, 4] (or [4, 4]) -
        a device tensor, or with sync=True a host array.  Returns a dict of device tensors - Tcw_out float32[n_problems, 4, 4], pose
        float64[n_problems, 12] (R row-major, t), outlier uint8[n_problems, N], point_row_out int32[n_problems, N] (point_rows=False: left out),
        counts int32[n_problems, 4] (POSE_COUNTS).  out: the dict of an earlier call, written again (nothing is allocated).  sync=True: the
        synchronous form; the dict holds Tcw_out, pose, outlier and counts as numpy arrays instead.  Otherwise the call waits for the current
        torch stream before it starts and for its own work before it returns; wait=False: it only enqueues on the handle's stream."""
        import torch
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("pose_optimization: no extract result for image %d" % image)
        dev = table.floats.device
        rows = frame_point_row if frame_point_row.dim() == 2 else frame_point_row.reshape(1, -1)
        n = int(rows.shape[0])
        if int(rows.shape[1]) != N:
            raise JsorbError("pose_optimization: frame_point_row must have %d columns" % N)
        fp = _i32_ptr("pose_optimization: frame_point_row", rows, n * N) if n * N else None
        ur = None
        if u_right is not None:
            if u_right.dtype != torch.float32 or not u_right.is_cuda or not u_right.is_contiguous() or u_right.numel() < N:
                raise JsorbError("pose_optimization: u_right must be a contiguous float32 device tensor of at least %d entries" % N)
            ur = u_right.data_ptr()
        tb = table.struct()
        n1 = max(n, 1)
        if sync:
            T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1, 16))
            if len(T) != n:
                raise JsorbError("pose_optimization: one Tcw per problem")
            To, po = np.zeros((n1, 16), np.float32), np.zeros((n1, 12), np.float64)
            fl, cn = np.zeros((n1, max(N, 1)), np.uint8)[:, :N].copy(), np.zeros((n1, 4), np.int32)
            ro = torch.empty((n1, max(N, 1)), dtype=torch.int32, device=dev) if point_rows else None
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self._lib.jsorb_pose_optimization(self._h, image, C.byref(params), C.byref(tb), n, fp, ur, T.ctypes.data, To.ctypes.data, po.ctypes.data,
                                                        fl.ctypes.data, None if ro is None else ro.data_ptr(), cn.ctypes.data))
            r = dict(Tcw_out=To[:n].reshape(n, 4, 4), pose=po[:n], outlier=fl[:n], counts=cn[:n])
            if ro is not None:
                r["point_row_out"] = ro.reshape(-1)[:n * N].reshape(n, N)
            return r
        if not torch.is_tensor(Tcw) or not Tcw.is_cuda or Tcw.dtype != torch.float32 or not Tcw.is_contiguous() or Tcw.numel() != 16 * n:
            raise JsorbError("pose_optimization: Tcw must be a contiguous float32 device tensor of %d entries" % (16 * n))
        if out is None:
            out = dict(Tcw_out=torch.empty((n1, 4, 4), dtype=torch.float32, device=dev)[:n], pose=torch.empty((n1, 12), dtype=torch.float64, device=dev)[:n],
                       outlier=torch.empty(n1 * max(N, 1), dtype=torch.uint8, device=dev)[:n * N].reshape(n, N),
                       counts=torch.empty((n1, 4), dtype=torch.int32, device=dev)[:n])
            if point_rows:
                out["point_row_out"] = torch.empty(n1 * max(N, 1), dtype=torch.int32, device=dev)[:n * N].reshape(n, N)
        if wait:
            torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_pose_optimization_async(self._h, image, C.byref(params), C.byref(tb), n, fp, ur, Tcw.data_ptr(), out["Tcw_out"].data_ptr(),
                                                          out["pose"].data_ptr(), out["outlier"].data_ptr(),
                                                          out["point_row_out"].data_ptr() if "point_row_out" in out else None, out["counts"].data_ptr()))
        if wait:
            self.sync()
        return out

    def pose_optimization_stats(self):
        """dict over POSE_STATS of the last pose_optimization, summed over its problems (diagnostics)"""
        v = np.zeros(8, np.int32)
        self._chk(self._lib.jsorb_pose_optimization_stats(self._h, v.ctypes.data))
        return dict(zip(POSE_STATS, (int(x) for x in v)))

    # ---- the local keyframes: Tracking::UpdateLocalKeyFrames (Tracking.cpp:1844-1952) and the concatenation of their rows on the device ----
    def local_keyframes(self, graph, table, frame_point_row, kf_capacity, entry_capacity, state=None, sync=False, out=None, wait=True):
        """jsorb_local_keyframes*: graph a KeyframeGraph, table a MapPointTable, frame_point_row an int32 device tensor (all of it is read) or None.
        state: the `state` of the previous call's result - (local_kf_slot, state_io), the list and {n_local, ref_slot} the reference keeps when no
        keyframe gets a vote; None starts with an empty list and ref_slot -1.  Returns a dict of device tensors - local_kf_slot
        int32[kf_capacity], state_io int32[2], local_kf_start int32[kf_capacity + 1], local_point_row int32[entry_capacity], counts int32[8]
        (LOCAL_KF_COUNTS) - and `state` for the next call; local_map_points(table, frustum, [0, entry_capacity], local_point_row, ...) takes
        it from there.  out: the dict of an earlier call, written again.  sync=True: the synchronous form; the dict also holds
        local_kf_slot_host, state_host and counts_host (numpy).  wait as for local_map_points."""
        import torch
        dev = table.floats.device
        kc, ec = int(kf_capacity), int(entry_capacity)
        fp, n_frame = None, 0
        if frame_point_row is not None:
            fp, n_frame = _i32_ptr("local_keyframes: frame_point_row", frame_point_row, flat=True), int(frame_point_row.shape[0])
        if out is None:
            if state is None:
                state = (torch.zeros(max(kc, 1), dtype=torch.int32, device=dev), torch.tensor([0, -1], dtype=torch.int32, device=dev))
            slot, sio = state
            if slot.dtype != torch.int32 or sio.dtype != torch.int32 or int(slot.shape[0]) < kc or int(sio.shape[0]) != 2 or not slot.is_contiguous():
                raise JsorbError("local_keyframes: state must be (int32[kf_capacity], int32[2]) of an earlier call")
            out = dict(local_kf_slot=slot, state_io=sio, local_kf_start=torch.empty(max(kc, 0) + 1, dtype=torch.int32, device=dev),
                       local_point_row=torch.empty(max(ec, 1), dtype=torch.int32, device=dev)[:max(ec, 0)], counts=torch.empty(8, dtype=torch.int32, device=dev))
        gs, tb = graph.struct(), table.struct()
        args = [self._h, C.byref(gs), C.byref(tb), fp, n_frame, kc, ec] + [out[k].data_ptr() for k in ("local_kf_slot", "state_io", "local_kf_start", "local_point_row", "counts")]
        if wait or sync:
            torch.cuda.current_stream(dev).synchronize()
        if sync:
            slot_h, state_h, counts_h = np.full(max(kc, 1), -2, np.int32), np.zeros(2, np.int32), np.zeros(8, np.int32)
            self._chk(self._lib.jsorb_local_keyframes(*args, slot_h.ctypes.data, state_h.ctypes.data, counts_h.ctypes.data))
            out = dict(out, local_kf_slot_host=slot_h[:max(kc, 0)], state_host=state_h, counts_host=counts_h)
        else:
            self._chk(self._lib.jsorb_local_keyframes_async(*args))
            if wait:
                self.sync()
        out["state"] = (out["local_kf_slot"], out["state_io"])
        return out

    def local_keyframes_stats(self):
        """dict(n_counter, n_first, n_local, n_neighbours, n_children, n_parents, n_invalid_runs, end_reason) of the last local_keyframes; end_reason: 0
        the list's end, 1 more than 80 keyframes, 2 a parent"""
        v = [C.c_int() for _ in range(8)]
        self._chk(self._lib.jsorb_local_keyframes_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_counter", "n_first", "n_local", "n_neighbours", "n_children", "n_parents", "n_invalid_runs", "end_reason"), (x.value for x in v)))

    # ---- motion-model matching: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cpp:1647-1963) on the device ----
    def search_last_frame(self, Px, Py, Pz, last_octave, last_angle, mp_descriptors, params, u_right=None, image=0):
        """TrackWithMotionModel's matching step (retry included) over image `image` of the last extract.  Device tensors: Px, Py, Pz, last_angle
        float32[n]; last_octave int32[n]; mp_descriptors uint8[n, 32]; u_right float32[N] or None (monocular).  params: make_last_frame_params(...).
        Returns (match_kp int32[n], match_dist int32[n], kp_match int32[N], n_matches int32[1]) as device tensors; the call waits for the current
        torch stream before it starts and for its own work before it returns."""
        import torch
        n = int(Px.shape[0]) if Px.dim() == 1 else -1
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("search_last_frame: no extract result for image %d" % image)
        if not isinstance(params, JsorbLastFrameParams):
            raise JsorbError("search_last_frame: params must come from make_last_frame_params")

        def chk(t, name, dtypes, shape):
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("search_last_frame: %s must be a device tensor" % name)
            if t.dtype not in dtypes:
                raise JsorbError("search_last_frame: %s must be %s, not %s" % (name, " / ".join(str(d) for d in dtypes), t.dtype))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise JsorbError("search_last_frame: %s must be a contiguous tensor of shape %s, not %s" % (name, shape, tuple(t.shape)))
            return t.data_ptr()

        if n < 0:
            raise JsorbError("search_last_frame: Px must be one-dimensional")
        f32, i32 = (torch.float32,), (torch.int32,)
        ptrs = [chk(Px, "Px", f32, (n,)), chk(Py, "Py", f32, (n,)), chk(Pz, "Pz", f32, (n,)), chk(last_octave, "last_octave", i32, (n,)),
                chk(last_angle, "last_angle", f32, (n,)), chk(mp_descriptors, "mp_descriptors", (torch.uint8,), (n, 32))]
        if n and mp_descriptors.data_ptr() % 16:
            raise JsorbError("search_last_frame: mp_descriptors must be 16-byte aligned")
        ptrs.append(None if u_right is None else chk(u_right, "u_right", f32, (N,)))
        dev = Px.device
        match_kp = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        match_dist = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        kp_match = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_search_last_frame_async(self._h, image, C.byref(params), n, *ptrs, match_kp.data_ptr(), match_dist.data_ptr(),
                                                          kp_match.data_ptr(), count.data_ptr()))
        self.sync()
        return match_kp[:n], match_dist[:n], kp_match[:N], count

    def search_last_frame_stats(self):
        """(passes, candidates, (ind1, ind2, ind3)) of the last search_last_frame: for the pass whose results stand"""
        p, c, b = C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self._lib.jsorb_search_last_frame_stats(self._h, C.byref(p), C.byref(c), b))
        return p.value, c.value, tuple(b)

    def search_last_frame_kernel_times(self):
        """{kernel: (total_ms, launches)} of the grid, match and resolve kernels, measured like kernel_times()"""
        return {name: self._kernel_time(k) for name, k in (("k_assign_grid", K_ASSIGN_GRID), ("k_last_match", K_LAST_MATCH), ("k_last_resolve", K_LAST_RESOLVE))}

    # ---- monocular initialisation matching: ORBmatcher::SearchForInitialization (ORBmatcher.cpp:392-507) on the device ----
    def search_for_initialization(self, f1_octave, f1_angle, f1_descriptors, prev_matched, params, image=0):
        """MonocularInitialization's matching step: F1 as device tensors (f1_octave int32[n1], f1_angle float32[n1], f1_descriptors uint8[n1, 32],
        prev_matched float32[2, n1]: x then y, UPDATED IN PLACE) against image `image` of the last extract.  params: make_init_params(...).
        Returns (matches12 int32[n1], matches21 int32[N], n_matches int32[1]) as device tensors; the call waits for the current torch stream
        before it starts and for its own work before it returns."""
        import torch
        n1 = int(f1_octave.shape[0]) if hasattr(f1_octave, "dim") and f1_octave.dim() == 1 else -1
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("search_for_initialization: no extract result for image %d" % image)
        if not isinstance(params, JsorbInitParams):
            raise JsorbError("search_for_initialization: params must come from make_init_params")
        if n1 < 0:
            raise JsorbError("search_for_initialization: f1_octave must be a one-dimensional device tensor")

        def chk(t, name, dtype, shape):
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("search_for_initialization: %s must be a device tensor" % name)
            if t.dtype != dtype:
                raise JsorbError("search_for_initialization: %s must be %s, not %s" % (name, dtype, t.dtype))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise JsorbError("search_for_initialization: %s must be a contiguous tensor of shape %s, not %s" % (name, shape, tuple(t.shape)))
            return t.data_ptr()

        ptrs = [chk(f1_octave, "f1_octave", torch.int32, (n1,)), chk(f1_angle, "f1_angle", torch.float32, (n1,)),
                chk(f1_descriptors, "f1_descriptors", torch.uint8, (n1, 32)), chk(prev_matched, "prev_matched", torch.float32, (2, n1))]
        if n1 and f1_descriptors.data_ptr() % 16:
            raise JsorbError("search_for_initialization: f1_descriptors must be 16-byte aligned")
        dev = f1_octave.device
        matches12 = torch.full((max(n1, 1),), -1, dtype=torch.int32, device=dev)
        matches21 = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_search_for_initialization_async(self._h, image, C.byref(params), n1, *ptrs, matches12.data_ptr(),
                                                                  matches21.data_ptr(), count.data_ptr()))
        self.sync()
        return matches12[:n1], matches21[:N], count

    def search_for_initialization_stats(self):
        """(fixed-point rounds over all chunks, candidates, points over the per-point list, displaced claims, (ind1, ind2, ind3)) of the last
        search_for_initialization / search_initial_frame"""
        r, c, o, d, b = C.c_int(), C.c_int(), C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self._lib.jsorb_search_for_initialization_stats(self._h, C.byref(r), C.byref(c), C.byref(o), C.byref(d), b))
        return r.value, c.value, o.value, d.value, tuple(b)

    def set_initial_frame(self, image=0):
        """keep image `image` of the last extract as mInitialFrame on the device (octaves, angles, descriptors; prev_matched = mvKeysUn);
        returns its keypoint count"""
        self._chk(self._lib.jsorb_init_reference_set(self._h, image))
        return self._lib.jsorb_init_reference_n(self._h)

    def clear_initial_frame(self):
        self._chk(self._lib.jsorb_init_reference_clear(self._h))

    def initial_frame_n(self):
        """keypoints of the kept initial frame, -1 when none is kept"""
        return self._lib.jsorb_init_reference_n(self._h)

    def search_initial_frame(self, params, image=0):
        """the kept initial frame against image `image` of the last extract: (matches12 int32[n1], prev_matched float32[2, n1], n_matches) on the
        host; the kept prev_matched is consumed and updated"""
        if not isinstance(params, JsorbInitParams):
            raise JsorbError("search_initial_frame: params must come from make_init_params")
        n1 = max(self._lib.jsorb_init_reference_n(self._h), 0)
        m12 = np.full(max(n1, 1), -1, np.int32)
        prev = np.zeros((2, max(n1, 1)), np.float32)
        cnt = C.c_int()
        self._chk(self._lib.jsorb_search_initial_frame(self._h, image, C.byref(params), m12.ctypes.data, prev.ctypes.data, C.byref(cnt)))
        return m12[:n1], prev.reshape(-1)[:2 * n1].reshape(2, n1), cnt.value

    # ---- bag of words: Frame::ComputeBoW (Frame.cpp:709-716) and ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (ORBmatcher.cpp:146-275) ----
    def bow_transform(self, voc, image=0):
        """jsorb_bow_transform_async: word and node ids of image `image` of the last extract (-1: every image, one launch) into buffers of the
        handle, enqueued on its stream; read them with bow() or use them through search_by_bow(f_node=None)"""
        if not isinstance(voc, Vocabulary):
            raise JsorbError("bow_transform: voc must be a Vocabulary")
        self._chk(self._lib.jsorb_bow_transform_async(self._h, image, voc.handle))

    def bow(self, image=0):
        """(word_id int32[N], node_id int32[N]) of the last bow_transform of this image, on the host (waits).  node_id -1: a stopped word"""
        n = self.n_keypoints(image)
        if n < 0:
            raise JsorbError("no extract result for image %d" % image)
        word, node = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
        rc = self._lib.jsorb_copy_bow(self._h, image, word.ctypes.data, node.ctypes.data)
        if rc != 0:
            raise JsorbError("jsorb_copy_bow rc=%d: no bow_transform of image %d since the last extract" % (rc, image))
        return word[:n], node[:n]

    def bow_device_pointers(self, image=0):
        """(jsorb_bow_word_device, jsorb_bow_node_device) as integers, 0 when the image has no transform since the last extract"""
        return self._lib.jsorb_bow_word_device(self._h, image) or 0, self._lib.jsorb_bow_node_device(self._h, image) or 0

    def bow_transform_stats(self):
        """descriptors of the last bow_transform whose leaf lay above the node level"""
        s = C.c_int()
        self._chk(self._lib.jsorb_bow_transform_stats(self._h, C.byref(s)))
        return s.value

    def _bow_keyframes(self, what, kf_start, kf_node, kf_valid, kf_angle, kf_descriptors):
        import torch
        ks = np.ascontiguousarray(kf_start, np.int32)
        if ks.ndim != 1 or len(ks) < 1:
            raise JsorbError("%s: kf_start must be a host array of n_keyframes + 1 offsets" % what)
        total = int(ks[-1])

        def chk(t, name, dtypes, shape):
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("%s: %s must be a device tensor" % (what, name))
            if t.dtype not in dtypes:
                raise JsorbError("%s: %s must be %s, not %s" % (what, name, " / ".join(str(d) for d in dtypes), t.dtype))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise JsorbError("%s: %s must be a contiguous tensor of shape %s, not %s" % (what, name, shape, tuple(t.shape)))
            return t.data_ptr()

        ptrs = [chk(kf_node, "kf_node", (torch.int32,), (total,)), chk(kf_valid, "kf_valid", (torch.uint8, torch.bool), (total,)),
                chk(kf_angle, "kf_angle", (torch.float32,), (total,)), chk(kf_descriptors, "kf_descriptors", (torch.uint8,), (total, 32))]
        if total and kf_descriptors.data_ptr() % 16:
            raise JsorbError("%s: kf_descriptors must be 16-byte aligned" % what)
        return ks, ptrs, chk

    def search_by_bow(self, kf_start, kf_node, kf_valid, kf_angle, kf_descriptors, params, f_node=None, image=0):
        """TrackReferenceKeyFrame's / Relocalization's matching step: len(kf_start) - 1 keyframes against image `image` of the last extract.
        kf_start: HOST int32 offsets; device tensors kf_node int32[n], kf_valid uint8 / bool [n], kf_angle float32[n], kf_descriptors uint8[n, 32];
        f_node int32[N] device tensor, or None: the handle's last bow_transform of this image.  params: make_bow_params(...).  Returns (match_kf
        int32[n_keyframes, N], n_matches int32[n_keyframes]) as device tensors; the call waits for the current torch stream before it starts
        and for its own work before it returns."""
        import torch
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("search_by_bow: no extract result for image %d" % image)
        if not isinstance(params, JsorbBowParams):
            raise JsorbError("search_by_bow: params must come from make_bow_params")
        ks, ptrs, chk = self._bow_keyframes("search_by_bow", kf_start, kf_node, kf_valid, kf_angle, kf_descriptors)
        fn = None if f_node is None else chk(f_node, "f_node", (torch.int32,), (N,))
        nk = len(ks) - 1
        dev = kf_node.device
        match_kf = torch.full((max(nk, 1), max(N, 1)), -7, dtype=torch.int32, device=dev)
        count = torch.full((max(nk, 1),), -7, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_search_by_bow_async(self._h, image, C.byref(params), fn, nk, ks.ctypes.data, *ptrs, match_kf.data_ptr(), count.data_ptr()))
        self.sync()
        return match_kf.reshape(-1)[:nk * N].reshape(nk, N), count[:nk]

    def search_by_bow_host(self, kf_start, kf_node, kf_valid, kf_angle, kf_descriptors, params, f_node=None, image=0):
        """jsorb_search_by_bow, the synchronous form: the same inputs, (match_kf int32[n_keyframes, N], n_matches int32[n_keyframes]) on the host
        with one synchronisation"""
        import torch
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("search_by_bow: no extract result for image %d" % image)
        if not isinstance(params, JsorbBowParams):
            raise JsorbError("search_by_bow: params must come from make_bow_params")
        ks, ptrs, chk = self._bow_keyframes("search_by_bow", kf_start, kf_node, kf_valid, kf_angle, kf_descriptors)
        fn = None if f_node is None else chk(f_node, "f_node", (torch.int32,), (N,))
        nk = len(ks) - 1
        match_kf = np.full(max(nk * N, 1), -7, np.int32)
        count = np.full(max(nk, 1), -7, np.int32)
        torch.cuda.current_stream(kf_node.device).synchronize()
        self._chk(self._lib.jsorb_search_by_bow(self._h, image, C.byref(params), fn, nk, ks.ctypes.data, *ptrs, match_kf.ctypes.data, count.ctypes.data))
        return match_kf[:nk * N].reshape(nk, N), count[:nk]

    def search_by_bow_stats(self):
        """((keyframe, node) pairs on both sides, Hamming distances, most frame keypoints in such a node, keyframe 0's (ind1, ind2, ind3)) of the
        last search_by_bow"""
        p, d, m, b = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self._lib.jsorb_search_by_bow_stats(self._h, C.byref(p), C.byref(d), C.byref(m), b))
        return p.value, d.value, m.value, tuple(b)

    def bow_kernel_times(self):
        """{kernel: (total_ms, launches)} of the transform, group, match and resolve kernels, measured like kernel_times()"""
        return {name: self._kernel_time(k) for name, k in (("k_bow_transform", K_BOW_TRANSFORM), ("k_bow_group", K_BOW_GROUP),
                                                           ("k_bow_match", K_BOW_MATCH), ("k_bow_resolve", K_BOW_RESOLVE))}

    # ---- relocalisation matching: ORBmatcher::SearchByProjection(CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1968-2095) ----
    def _kf_points(self, Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle, mp_descriptors, params, blocked, image):
        import torch
        what = "search_by_projection_kf"
        n = int(Px.shape[0]) if hasattr(Px, "dim") and Px.dim() == 1 else -1
        N = self.n_keypoints(image)
        if N < 0:
            raise JsorbError("%s: no extract result for image %d" % (what, image))
        if not isinstance(params, JsorbKfProjectionParams):
            raise JsorbError("%s: params must come from make_kf_projection_params" % what)
        if n < 0:
            raise JsorbError("%s: Px must be a one-dimensional device tensor" % what)

        def chk(t, name, dtypes, shape):
            if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
                raise JsorbError("%s: %s must be a device tensor" % (what, name))
            if t.dtype not in dtypes:
                raise JsorbError("%s: %s must be %s, not %s" % (what, name, " / ".join(str(d) for d in dtypes), t.dtype))
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise JsorbError("%s: %s must be a contiguous tensor of shape %s, not %s" % (what, name, shape, tuple(t.shape)))
            return t.data_ptr()

        f32 = (torch.float32,)
        ptrs = [chk(t, name, f32, (n,)) for t, name in ((Px, "Px"), (Py, "Py"), (Pz, "Pz"), (max_distance, "max_distance"), (max_dist_inv, "max_dist_inv"),
                                                        (min_dist_inv, "min_dist_inv"), (kf_angle, "kf_angle"))]
        ptrs.append(chk(mp_descriptors, "mp_descriptors", (torch.uint8,), (n, 32)))
        if n and mp_descriptors.data_ptr() % 16:
            raise JsorbError("%s: mp_descriptors must be 16-byte aligned" % what)
        ptrs.append(None if blocked is None else chk(blocked, "blocked", (torch.uint8, torch.bool), (N,)))
        return n, N, ptrs

    def search_by_projection_kf(self, Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle, mp_descriptors, params, blocked=None, image=0):
        """Relocalization's projection matcher over image `image` of the last extract.  Device tensors, one entry per keyframe point in ascending
        keyframe slot: Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle float32[n]; mp_descriptors uint8[n, 32]; blocked uint8 /
        bool [N] or None (CurrentFrame.mvpMapPoints[k] != NULL before the call).  params: make_kf_projection_params(...).  Returns (match_kp
        int32[n], match_dist int32[n], kp_match int32[N], n_matches int32[1]) as device tensors; the call waits for the current torch stream before
        it starts and for its own work before it returns."""
        import torch
        n, N, ptrs = self._kf_points(Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle, mp_descriptors, params, blocked, image)
        dev = Px.device
        match_kp = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        match_dist = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        kp_match = torch.full((max(N, 1),), -1, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._lib.jsorb_search_by_projection_kf_async(self._h, image, C.byref(params), n, *ptrs, match_kp.data_ptr(), match_dist.data_ptr(),
                                                                kp_match.data_ptr(), count.data_ptr()))
        self.sync()
        return match_kp[:n], match_dist[:n], kp_match[:N], count

    def search_by_projection_kf_host(self, Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle, mp_descriptors, params, blocked=None, image=0):
        """jsorb_search_by_projection_kf, the synchronous form: the same inputs, (kp_match int32[N] on the host, n_matches) with one copy back"""
        import torch
        n, N, ptrs = self._kf_points(Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle, mp_descriptors, params, blocked, image)
        kp_match = np.full(max(N, 1), -7, np.int32)
        count = C.c_int(-7)
        torch.cuda.current_stream(Px.device).synchronize()
        self._chk(self._lib.jsorb_search_by_projection_kf(self._h, image, C.byref(params), n, *ptrs, kp_match.ctypes.data, C.byref(count)))
        return kp_match[:N], count.value

    def search_by_projection_kf_stats(self):
        """(fixed-point rounds, candidates, points over the per-point list, (ind1, ind2, ind3)) of the last search_by_projection_kf"""
        r, c, o, b = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self._lib.jsorb_search_by_projection_kf_stats(self._h, C.byref(r), C.byref(c), C.byref(o), b))
        return r.value, c.value, o.value, tuple(b)

    def search_by_projection_kf_kernel_times(self):
        """{kernel: (total_ms, launches)} of the grid, candidate and resolve kernels, measured like kernel_times()"""
        return {name: self._kernel_time(k) for name, k in (("k_assign_grid", K_ASSIGN_GRID), ("k_kf_candidates", K_KF_CANDIDATES),
                                                           ("k_kf_resolve", K_KF_RESOLVE))}

    # ---- profiling plumbing ----
    def set_stream(self, stream_ptr):
        self._chk(self._lib.jsorb_set_stream(self._h, stream_ptr))

    def stream_wait_done(self, other_stream_ptr):
        """make another HIP stream (raw pointer, 0 = null stream) wait for everything enqueued on this handle"""
        self._chk(self._lib.jsorb_stream_wait_done(self._h, other_stream_ptr))

    def enable_kernel_timing(self, on=True):
        self._chk(self._lib.jsorb_enable_kernel_timing(self._h, int(on)))

    def reset_kernel_timing(self):
        self._chk(self._lib.jsorb_reset_kernel_timing(self._h))

    def kernel_times(self):
        """{kernel: (total_ms, launches)} measured with hipEvents on the stream the kernels run on."""
        res = {}
        for i, name in enumerate(KERNELS):
            ms, n = C.c_double(), C.c_long()
            self._chk(self._lib.jsorb_kernel_time(self._h, i, C.byref(ms), C.byref(n)))
            res[name] = (ms.value, n.value)
        return res

    def rectify_kernel_time(self):
        """(total_ms, launches) of k_rectify (kernel id K_RECTIFY), measured like kernel_times()."""
        ms, n = C.c_double(), C.c_long()
        self._chk(self._lib.jsorb_kernel_time(self._h, K_RECTIFY, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def compute_stereo_matches(left, right, mb, mbf, th_high=TH_HIGH, th_low=TH_LOW):
    """Frame::ComputeStereoMatches (src/Frame.cpp:780-803) on the last extract of two ORBExtractor objects.
    Returns (mvuRight, mvDepth, stats) as float32 arrays of length N_left (-1 = no match)."""
    n = left.n_keypoints(0)
    u = np.full(max(n, 1), -1, np.float32)
    d = np.full(max(n, 1), -1, np.float32)
    st = JsorbStereoStats()
    rc = left._lib.jsorb_stereo_match(left.handle, right.handle, mb, mbf, th_high, th_low, u.ctypes.data, d.ctypes.data, C.byref(st))
    left._chk(rc)
    return u[:n], d[:n], {k: getattr(st, k) for k, _ in JsorbStereoStats._fields_}


def set_speculative_stereo(left, on):
    """jsorb_set_speculative_stereo: the match enqueued behind the next pair of single-image extracts (include/jsorb.h)"""
    left._chk(left._lib.jsorb_set_speculative_stereo(left.handle, int(bool(on))))


def speculative_stereo_stats(left):
    """(adopted, dropped) speculative matches of the pair this left handle belongs to"""
    a, d = C.c_long(0), C.c_long(0)
    left._chk(left._lib.jsorb_speculative_stereo_stats(left.handle, C.byref(a), C.byref(d)))
    return a.value, d.value


def stereo_match_batch_async(left, right, mb, mbf, th_high=TH_HIGH, th_low=TH_LOW):
    left._chk(left._lib.jsorb_stereo_match_batch_async(left.handle, right.handle, mb, mbf, th_high, th_low))


def stereo_result(left, image=0):
    n = left.n_keypoints(image)
    u = np.full(max(n, 1), -1, np.float32)
    d = np.full(max(n, 1), -1, np.float32)
    st = JsorbStereoStats()
    left._chk(left._lib.jsorb_copy_stereo(left.handle, image, u.ctypes.data, d.ctypes.data, C.byref(st)))
    return u[:n], d[:n], {k: getattr(st, k) for k, _ in JsorbStereoStats._fields_}


def stereo_l1(left, image=0):
    """L1 distances the median cut sorted (-1 = no accepted refinement), int32[N_left]"""
    n = left.n_keypoints(image)
    out = np.full(max(n, 1), -1, np.int32)
    left._chk(left._lib.jsorb_copy_stereo_l1(left.handle, image, out.ctypes.data))
    return out[:n]


def set_stereo_diagnostics(left, on=True):
    """keep the matcher's intermediate results of the following matches (stereo_diagnostics)"""
    left._chk(left._lib.jsorb_set_stereo_diagnostics(left.handle, 1 if on else 0))


def stereo_diagnostics(left, image=0):
    """(best_right[N], best_dist[N], l1_sums[N, 11]) of the last match: K12's arg-min per left keypoint (-1 / th_high: none) and the 11 L1 window
    sums of K13 (-1 where no window search ran) - what the reference keeps on the host between its two kernels"""
    n = left.n_keypoints(image)
    out = np.full((max(n, 1), 13), -1, np.int32)
    left._chk(left._lib.jsorb_copy_stereo_diagnostics(left.handle, image, out.ctypes.data))
    out = out[:n]
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2:].copy()


def gather_counts_async(left, right, dev_dst_ptr):
    """(N_left, N_right, N_matched) per pair of the last batch -> int32[3*n] DEVICE buffer (payload of the RCCL all_gather)."""
    left._chk(left._lib.jsorb_gather_counts_async(left.handle, right.handle, dev_dst_ptr))
