"""ctypes view of libvoxgraph_amd.so (include/voxgraph_amd.h).

This module only declares the C ABI and wraps handles; all arithmetic happens in
the HIP library.  There is no fallback: if the shared object is missing the
import fails, and without a gfx950 device Context() raises.
"""
import collections
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VGX_LIB: an alternative build of the same library (A/B scripts under profiles/ only)
LIB_PATH = os.environ.get("VGX_LIB") or os.path.join(_HERE, "lib", "libvoxgraph_amd.so")
# test / benchmark tooling (include/voxgraph_amd_bench.h), built next to it from csrc/bench/
BENCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), os.path.basename(LIB_PATH).replace("libvoxgraph_amd", "libvoxgraph_amd_bench", 1))

OK = 0
EVALUATE_FALSE = 1
ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_UNSUPPORTED, ERR_NO_DEVICE = -1, -2, -3, -4, -5
ERR_NOT_POSITIVE_DEFINITE = -6

BRICKS_APRON, BRICKS_QUAD = 0, 1
SAMPLING_BRICKS_SAME, SAMPLING_BRICKS_QUAD = 0, 1
POINTS_ISOSURFACE = 0
POINTS_VOXELS = 1
POINTS_KEEP_ORDER = 0
POINTS_SORT_MORTON = 1

NORMAL_SIZE = 45

vp = C.c_void_p
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)


class RegConfig(C.Structure):
    """vgx_reg_config == RegistrationCostFunction::Config (registration_cost_function.h:17-41)."""
    _fields_ = [("registration_point_type", C.c_int32), ("sampling_ratio", C.c_float),
                ("no_correspondence_cost", C.c_double), ("use_esdf_distance", C.c_int32),
                ("sampler_seed", C.c_uint32)]


class EsdfConfig(C.Structure):
    """vgx_esdf_config == voxblox::EsdfIntegrator::Config (the fields used in batch mode)."""
    _fields_ = [("max_distance_m", C.c_float), ("min_distance_m", C.c_float),
                ("default_distance_m", C.c_float), ("min_diff_m", C.c_float),
                ("min_weight", C.c_float), ("num_buckets", C.c_int32)]


class MapFileSubmapInfo(C.Structure):
    _fields_ = [("id", C.c_int64), ("T_M_S", C.c_double * 7), ("voxel_size", C.c_double),
                ("voxels_per_side", C.c_int32), ("n_tsdf_blocks", C.c_int32),
                ("n_esdf_blocks", C.c_int32), ("layer_is_esdf", C.c_int32)]


class MapFileSubmapData(C.Structure):
    _fields_ = [("id", C.c_int64), ("T_M_S", C.c_double * 7), ("n_blocks", C.c_int32),
                ("block_index", C.POINTER(C.c_int32)), ("tsdf_distance", C.POINTER(C.c_float)),
                ("tsdf_weight", C.POINTER(C.c_float)), ("tsdf_rgba", C.POINTER(C.c_uint8)),
                ("esdf_distance", C.POINTER(C.c_float)), ("esdf_observed", C.POINTER(C.c_uint8))]


class MeshConfig(C.Structure):
    _fields_ = [("min_weight", C.c_float)]


class MeshMarkerConfig(C.Structure):
    """vgx_mesh_marker_config: voxblox ColorMode, SubmapVisuals::mesh_opacity_ and cblox colorMeshLayer's colour."""
    _fields_ = [("color_mode", C.c_int32), ("opacity", C.c_float), ("use_constant_color", C.c_int32),
                ("constant_rgba", C.c_uint8 * 4)]


# voxblox ColorMode, in its order [recalled]
MARKER_COLOR, MARKER_HEIGHT, MARKER_NORMALS, MARKER_GRAY, MARKER_LAMBERT, MARKER_LAMBERT_COLOR = 0, 1, 2, 3, 4, 5


class CloudConfig(C.Structure):
    """vgx_cloud_config: which voxels of a layer become points (include/voxgraph_amd.h, "Layer point clouds")."""
    _fields_ = [("kind", C.c_int32), ("surface_distance", C.c_float), ("min_weight", C.c_float),
                ("slice_axis", C.c_int32), ("slice_value", C.c_float)]


CLOUD_DISTANCE, CLOUD_SURFACE_DISTANCE, CLOUD_SURFACE_COLOR = 0, 1, 2


class PlanarMapConfig(C.Structure):
    """vgx_planar_map_config: the height band, the voxel classes, the grid box and the distance limit of a planar map
    (include/voxgraph_amd.h, "Planar map")."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("occupied_distance", C.c_float), ("min_weight", C.c_float),
                ("min_free_voxels", C.c_int32), ("unknown_is_obstacle", C.c_int32), ("max_distance_m", C.c_float),
                ("use_box", C.c_int32), ("cell_min", C.c_int32 * 2), ("cell_dim", C.c_int32 * 2)]


class ElevationMapConfig(C.Structure):
    """vgx_elevation_map_config: the height band, the crossing picked, the step window, the traversability limits, the
    grid box and the distance limit of an elevation map (include/voxgraph_amd.h, "Elevation map")."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("min_weight", C.c_float), ("min_free_voxels", C.c_int32),
                ("pick", C.c_int32), ("step_radius_cells", C.c_int32), ("min_support", C.c_int32), ("max_slope", C.c_float),
                ("max_step_m", C.c_float), ("min_headroom_voxels", C.c_int32), ("hole_is_obstacle", C.c_int32),
                ("unknown_is_obstacle", C.c_int32), ("max_distance_m", C.c_float), ("use_box", C.c_int32),
                ("cell_min", C.c_int32 * 2), ("cell_dim", C.c_int32 * 2)]


class ScanLayout(C.Structure):
    """vgx_scan_layout: a sensor_msgs/PointCloud2 header with the field names resolved to byte offsets."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("offset_x", C.c_uint32), ("offset_y", C.c_uint32), ("offset_z", C.c_uint32),
                ("color_kind", C.c_int32), ("color_offset", C.c_uint32), ("is_bigendian", C.c_int32)]


class ScanConfig(C.Structure):
    """vgx_scan_config: the grey scale's range and the colour of a cloud without colours."""
    _fields_ = [("intensity_min", C.c_float), ("intensity_max", C.c_float), ("constant_rgba", C.c_uint8 * 4)]


SCAN_COLOR_NONE, SCAN_COLOR_RGB, SCAN_COLOR_INTENSITY = 0, 1, 2


class ScanTimeField(C.Structure):
    """vgx_scan_time_field: where a point's time lies and t = offset_s + raw * scale."""
    _fields_ = [("kind", C.c_int32), ("offset", C.c_uint32), ("scale", C.c_double), ("offset_s", C.c_double)]


class ScanTrackView(C.Structure):
    """vgx_scan_track: host arrays of knot times [K] f64 and knot transforms [K][7] f32."""
    _fields_ = [("n_knots", C.c_int32), ("knot_time", C.POINTER(C.c_double)), ("knot_T", C.POINTER(C.c_float))]


SCAN_TIME_UINT32, SCAN_TIME_FLOAT32, SCAN_TIME_FLOAT64 = 0, 1, 2


class DepthImageLayout(C.Structure):
    """vgx_depth_image_layout: a sensor_msgs/Image depth frame's header and its registered colour image's."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("row_step", C.c_uint32), ("encoding", C.c_int32),
                ("is_bigendian", C.c_int32), ("color_kind", C.c_int32), ("color_row_step", C.c_uint32)]


class DepthCamera(C.Structure):
    """vgx_depth_camera: the rectified pinhole model, the depth unit and gate, and the pixel strides."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("depth_unit_m", C.c_float),
                ("min_depth_m", C.c_float), ("max_depth_m", C.c_float), ("stride_u", C.c_int32), ("stride_v", C.c_int32)]


class DepthRowTime(C.Structure):
    """vgx_depth_row_time: t = offset_s + v * scale of image row v."""
    _fields_ = [("scale", C.c_double), ("offset_s", C.c_double)]


class ProjectiveCounts(C.Structure):
    """vgx_projective_counts: of the last projectively integrated frame."""
    _fields_ = [("n_candidate_blocks", C.c_int64), ("n_new_blocks", C.c_int64), ("n_updates", C.c_int64),
                ("n_carved", C.c_int64), ("n_cleared", C.c_int64)]


class LidarModel(C.Structure):
    """vgx_lidar_model: a spinning LiDAR's spherical image -- azimuth columns, uniform beam rows."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("azimuth_first_rad", C.c_float), ("azimuth_clockwise", C.c_int32),
                ("elevation_first_rad", C.c_float), ("elevation_last_rad", C.c_float)]


class LidarBeamModel(C.Structure):
    """vgx_lidar_beam_model: a spinning LiDAR whose rows have elevations and azimuth offsets of their own (make one with
    lidar_beam_model(), which keeps the arrays alive)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("azimuth_first_rad", C.c_float), ("azimuth_clockwise", C.c_int32),
                ("row_elevation_rad", C.POINTER(C.c_float)), ("row_azimuth_offset_rad", C.POINTER(C.c_float)),
                ("row_half_extent_max_rad", C.c_float)]


class RangeImageCounts(C.Structure):
    """vgx_range_image_counts: of the range image a handle holds."""
    _fields_ = [("n_points", C.c_int64), ("n_kept", C.c_int64), ("n_filled", C.c_int64), ("n_collided", C.c_int64),
                ("n_rejected_range", C.c_int64), ("n_rejected_rows", C.c_int64), ("max_range", C.c_float),
                ("point_min", C.c_float * 3), ("point_max", C.c_float * 3), ("dir_min", C.c_float * 3), ("dir_max", C.c_float * 3),
                ("pad_", C.c_int32)]


DEPTH_16UC1, DEPTH_32FC1 = 0, 1
IMAGE_COLOR_NONE, IMAGE_COLOR_RGB8, IMAGE_COLOR_BGR8, IMAGE_COLOR_RGBA8, IMAGE_COLOR_BGRA8, IMAGE_COLOR_MONO8 = 0, 1, 2, 3, 4, 5
DEPTH_BYTES_PER_PIXEL = {DEPTH_16UC1: 2, DEPTH_32FC1: 4}
IMAGE_COLOR_BYTES_PER_PIXEL = {IMAGE_COLOR_NONE: 0, IMAGE_COLOR_RGB8: 3, IMAGE_COLOR_BGR8: 3, IMAGE_COLOR_RGBA8: 4,
                               IMAGE_COLOR_BGRA8: 4, IMAGE_COLOR_MONO8: 1}


class EvaluationDetails(C.Structure):
    """vgx_voxel_evaluation_details: voxblox::utils::VoxelEvaluationDetails plus the f64 sum and the true min |e|."""
    _fields_ = [("rmse", C.c_float), ("max_error", C.c_float), ("min_error", C.c_float),
                ("total_squared_error", C.c_double), ("min_abs_error", C.c_float),
                ("num_evaluated_voxels", C.c_int64), ("num_ignored_voxels", C.c_int64),
                ("num_overlapping_voxels", C.c_int64), ("num_non_overlapping_voxels", C.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# voxblox VoxelEvaluationMode order; which layer of the two submaps vgx_evaluate_layers_rmse compares
EVAL_ALL_VOXELS, EVAL_IGNORE_BEHIND_TEST, EVAL_IGNORE_BEHIND_GT, EVAL_IGNORE_BEHIND_ALL = 0, 1, 2, 3
EVAL_LAYER_ESDF, EVAL_LAYER_TSDF = 0, 1
QUERY_INTERPOLATE, QUERY_GRADIENT = 1, 2


class TsdfConfig(C.Structure):
    """vgx_tsdf_config == voxblox::TsdfIntegratorBase::Config (the fields that matter on a GPU)."""
    _fields_ = [("default_truncation_distance", C.c_float), ("max_weight", C.c_float),
                ("voxel_carving_enabled", C.c_int32), ("min_ray_length_m", C.c_float),
                ("max_ray_length_m", C.c_float), ("use_const_weight", C.c_int32),
                ("allow_clear", C.c_int32), ("use_weight_dropoff", C.c_int32),
                ("use_sparsity_compensation_factor", C.c_int32),
                ("sparsity_compensation_factor", C.c_float),
                ("start_voxel_subsampling_factor", C.c_float),
                ("max_consecutive_ray_collisions", C.c_int32),
                ("clear_checks_every_n_frames", C.c_int32), ("enable_anti_grazing", C.c_int32),
                ("deterministic", C.c_int32), ("integration_order", C.c_int32)]


class PoseGraphEdge(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("t_obs", C.c_double * 3), ("yaw_obs", C.c_double),
                ("sqrt_information", C.c_double * 16)]


class PoseGraphOptions(C.Structure):
    _fields_ = [("parameter_tolerance", C.c_double), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("max_solver_time_in_seconds", C.c_double), ("initial_trust_region_radius", C.c_double),
                ("max_num_iterations", C.c_int32), ("exclude_registration_constraints", C.c_int32)]


class PoseGraphSummary(C.Structure):
    _fields_ = [("termination_type", C.c_int32), ("termination_reason", C.c_int32), ("num_iterations", C.c_int32),
                ("num_successful_steps", C.c_int32), ("num_full_evaluations", C.c_int32), ("num_cost_evaluations", C.c_int32),
                ("num_factorization_failures", C.c_int32), ("num_free_nodes", C.c_int32), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("total_seconds", C.c_double), ("registration_seconds", C.c_double),
                ("linear_algebra_seconds", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PoseGraphIteration(C.Structure):
    _fields_ = [("cost", C.c_double), ("trial_cost", C.c_double), ("gain_ratio", C.c_double), ("radius", C.c_double),
                ("step_norm", C.c_double), ("accepted", C.c_int32), ("factorization_failed", C.c_int32)]


class PoseGraphStructureStats(C.Structure):
    _fields_ = [("n_free_variables", C.c_int32), ("n_panels", C.c_int32), ("n_launches", C.c_int32), ("reserved", C.c_int32),
                ("n_h_tiles", C.c_int64), ("n_l_tiles", C.c_int64), ("n_update_triples", C.c_int64), ("bytes", C.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class PoseGraphCovarianceStats(C.Structure):
    _fields_ = [("n_columns", C.c_int32), ("n_slabs", C.c_int32), ("n_launches", C.c_int32), ("reserved", C.c_int32),
                ("solve_bytes", C.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class ScanRegistrationConfig(C.Structure):
    _fields_ = [("min_range_m", C.c_float), ("max_range_m", C.c_float), ("max_abs_distance_m", C.c_float),
                ("point_stride", C.c_int32), ("min_valid_ratio", C.c_float)]


class ScanRegistrationSummary(C.Structure):
    _fields_ = [("usable", C.c_int32), ("termination_type", C.c_int32), ("termination_reason", C.c_int32),
                ("num_iterations", C.c_int32), ("num_successful_steps", C.c_int32), ("num_evaluations", C.c_int32),
                ("num_factorization_failures", C.c_int32), ("reserved", C.c_int32), ("n_candidates", C.c_int64),
                ("n_valid_first", C.c_int64), ("n_valid_last", C.c_int64), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("total_seconds", C.c_double), ("evaluation_seconds", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class ScanMapConfig(C.Structure):
    _fields_ = [("layer", C.c_int32), ("huber_delta_m", C.c_float), ("score_point_stride", C.c_int32), ("reserved", C.c_int32)]


class ViewConfig(C.Structure):
    _fields_ = [("s_min", C.c_float), ("s_max", C.c_float), ("step_scale", C.c_float), ("min_step", C.c_float),
                ("unknown_step", C.c_float), ("max_bracket", C.c_float), ("image_width", C.c_int32), ("flags", C.c_int32)]


class ViewCounts(C.Structure):
    _fields_ = [("n_rays", C.c_int64), ("n_hit", C.c_int64), ("n_hit_unsampled", C.c_int64), ("n_miss", C.c_int64),
                ("n_inside", C.c_int64), ("n_bad", C.c_int64), ("n_samples", C.c_int64), ("reserved", C.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


VIEW_MISS, VIEW_HIT, VIEW_INSIDE, VIEW_BAD, VIEW_HIT_UNSAMPLED = range(5)
VIEW_POINTS, VIEW_GRADIENT, VIEW_WEIGHT, VIEW_RGBA, VIEW_N_SAMPLES, VIEW_ALL = 1, 2, 4, 8, 16, 31

LINEAR_SOLVER_DENSE, LINEAR_SOLVER_TILE_SPARSE = 0, 1
ORDER_NATURAL, ORDER_RCM, ORDER_GIVEN = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2      # ceres::TerminationType
(TERMINATION_PARAMETER_TOLERANCE, TERMINATION_FUNCTION_TOLERANCE, TERMINATION_GRADIENT_TOLERANCE, TERMINATION_MAX_ITERATIONS,
 TERMINATION_MAX_SOLVER_TIME, TERMINATION_NO_FREE_NODES) = range(6)
TERMINATION_TOO_FEW_POINTS = 6                     # scan-to-map registration alone
TERMINATION_NAMES = ("parameter_tolerance", "function_tolerance", "gradient_tolerance", "max_iterations", "max_solver_time",
                     "no_free_nodes", "too_few_points")   # harness/lm.py's names for the same rules

TSDF_ORDER_MIXED, TSDF_ORDER_SORTED = 0, 1
# what a vgx_map_msg holds; voxblox MapDerializationAction (include/voxgraph_amd.h, "Map messages")
MSG_NONE, MSG_TSDF_LAYER, MSG_ESDF_LAYER, MSG_SURFACE_CLOUD = 0, 1, 2, 3
MSG_ACTION_UPDATE, MSG_ACTION_MERGE, MSG_ACTION_RESET = 0, 1, 2

# every symbol include/voxgraph_amd.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "vgx_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "vgx_ctx_destroy": (C.c_int, [vp]),
    "vgx_last_error": (C.c_char_p, [vp]),
    "vgx_ctx_set_stream": (C.c_int, [vp, vp]),
    "vgx_ctx_get_stream": (vp, [vp]),
    "vgx_ctx_set_tsdf_stream": (C.c_int, [vp, vp]),
    "vgx_ctx_get_tsdf_stream": (vp, [vp]),
    "vgx_ctx_synchronize": (C.c_int, [vp]),
    "vgx_ctx_synchronize_tsdf": (C.c_int, [vp]),
    "vgx_ctx_tsdf_wait_for_stream": (C.c_int, [vp, vp]),
    "vgx_ctx_stream_priorities": (C.c_int, [vp]),
    "vgx_ctx_set_brick_layout": (C.c_int, [vp, C.c_int32]),
    "vgx_ctx_set_sampling_bricks": (C.c_int, [vp, C.c_int32]),
    "vgx_ctx_timer_start": (C.c_int, [vp]),
    "vgx_ctx_timer_stop": (C.c_int, [vp, f32p]),
    "vgx_submap_create": (C.c_int, [vp, C.c_int32, C.c_float, C.c_int32, C.c_int32, i32p, f32p,
                                    f32p, f32p, u8p, C.POINTER(vp)]),
    "vgx_submap_destroy": (C.c_int, [vp]),
    "vgx_submap_id": (C.c_int32, [vp]),
    "vgx_submap_num_blocks": (C.c_int32, [vp]),
    "vgx_submap_set_points": (C.c_int, [vp, C.c_int32, C.c_int64, f32p, f32p, f32p, C.c_uint32]),
    "vgx_submap_extract_voxel_points": (C.c_int, [vp, C.c_double, C.c_double, C.c_int32, i64p]),
    "vgx_submap_extract_isosurface_points": (C.c_int, [vp, C.c_double, i64p]),
    "vgx_submap_num_points": (C.c_int64, [vp, C.c_int32]),
    "vgx_submap_point_order": (C.c_int, [vp, C.c_int32, i64p]),
    "vgx_submap_download_points": (C.c_int, [vp, C.c_int32, f32p, f32p, f32p]),
    "vgx_esdf_config_default": (None, [C.POINTER(EsdfConfig)]),
    "vgx_submap_generate_esdf": (C.c_int, [vp, C.POINTER(EsdfConfig), i32p]),
    "vgx_submap_from_tsdf_layer": (C.c_int, [vp, vp, C.c_int32, C.POINTER(vp)]),
    "vgx_submap_from_tsdf_layer_colored": (C.c_int, [vp, vp, C.c_int32, C.POINTER(vp)]),
    "vgx_submap_set_colors": (C.c_int, [vp, u8p]),
    "vgx_submap_has_colors": (C.c_int, [vp, i32p]),
    "vgx_submap_download_colors": (C.c_int, [vp, u8p]),
    "vgx_submap_release_raw_layers": (C.c_int, [vp]),
    "vgx_submap_download_layers": (C.c_int, [vp, f32p, f32p, f32p, u8p]),
    "vgx_submap_block_index": (C.c_int, [vp, i32p]),
    "vgx_reg_config_default": (None, [C.POINTER(RegConfig)]),
    "vgx_reg_create": (C.c_int, [vp, vp, vp, C.POINTER(RegConfig), C.POINTER(vp)]),
    "vgx_reg_destroy": (C.c_int, [vp]),
    "vgx_reg_num_residuals": (C.c_int64, [vp]),
    "vgx_reg_evaluate": (C.c_int, [vp, f64p, f64p, f64p, f64p, f64p]),
    "vgx_reg_evaluate_device_f32": (C.c_int, [vp, f64p, f64p, vp, vp, vp]),
    "vgx_reg_visuals_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_reg_visuals_destroy": (C.c_int, [vp]),
    "vgx_reg_evaluate_visuals": (C.c_int, [vp, f64p, f64p, f64p, f64p, f64p, C.c_int32, C.c_int32, vp]),
    "vgx_reg_visuals_stats": (C.c_int, [vp, i64p, i64p]),
    "vgx_reg_visuals_download": (C.c_int, [vp, vp, f64p, f64p, f64p]),
    "vgx_reg_visuals_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "vgx_reg_batch_create": (C.c_int, [vp, C.c_int32, C.POINTER(vp), i32p, i32p, C.c_int32,
                                       C.POINTER(vp)]),
    "vgx_reg_batch_destroy": (C.c_int, [vp]),
    "vgx_reg_batch_num_residuals": (C.c_int64, [vp]),
    "vgx_reg_batch_row_offsets": (C.c_int, [vp, i64p]),
    "vgx_reg_batch_evaluate_points": (C.c_int, [vp, f64p, C.c_int32, vp, vp, vp, i32p]),
    "vgx_reg_batch_evaluate_points_f64": (C.c_int, [vp, f64p, C.c_int32, vp, vp, vp, i32p]),
    "vgx_reg_batch_evaluate_rows_f64": (C.c_int, [vp, f64p, C.c_int32, C.c_int32, C.c_int32, i32p]),
    "vgx_reg_batch_fetch_rows_f64": (C.c_int, [vp, C.c_int32, f64p, f64p, f64p]),
    "vgx_reg_batch_evaluate_cost": (C.c_int, [vp, f64p, C.c_int32, vp, f64p, i32p]),
    "vgx_reg_batch_blocked_layout": (C.c_int, [vp, C.POINTER(C.c_int64), i32p, C.POINTER(C.c_int64)]),
    "vgx_reg_batch_evaluate_points_blocked": (C.c_int, [vp, f64p, C.c_int32, vp, i32p]),
    "vgx_reg_batch_choose_outputs": (C.c_int, [vp, f64p, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                               C.c_int32, i32p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vgx_reg_batch_alloc_outputs": (C.c_int, [vp, f64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(vp),
                                              C.POINTER(vp), C.POINTER(C.c_float)]),
    "vgx_reg_batch_free_outputs": (C.c_int, [vp, vp, vp, vp]),
    "vgx_reg_batch_evaluate_normal": (C.c_int, [vp, f64p, C.c_int32, vp, f64p, i32p]),
    "vgx_reg_batch_count_live": (C.c_int, [vp, f64p, C.c_int32, i64p, i64p]),
    "vgx_reg_batch_launch_order": (C.c_int, [vp, C.c_int32, i32p]),
    "vgx_reg_batch_count_live_each": (C.c_int, [vp, f64p, C.c_int32, i64p]),
    "vgx_reg_batch_assemble": (C.c_int, [vp, vp, C.c_int32, vp, C.c_int32]),
    "vgx_reg_fused_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "vgx_reg_batch_scatter_normal": (C.c_int, [vp, vp, vp, C.c_int32]),
    "vgx_reg_batch_brick_layout": (C.c_int32, [vp]),
    "vgx_reg_assembler_create": (C.c_int, [vp, C.c_int32, i32p, C.POINTER(vp)]),
    "vgx_reg_assembler_assemble": (C.c_int, [vp, vp, C.c_int32, vp]),
    "vgx_reg_assembler_destroy": (C.c_int, [vp]),
    "vgx_lpt_shards": (C.c_int, [C.c_int32, i64p, C.c_int32, i32p]),
    "vgx_contiguous_shards": (C.c_int, [C.c_int32, i64p, C.c_int32, i32p]),
    "vgx_reg_multi_create": (C.c_int, [C.c_int32, C.POINTER(vp), C.c_int32, C.POINTER(vp), i32p, C.POINTER(vp)]),
    "vgx_reg_multi_destroy": (C.c_int, [vp]),
    "vgx_reg_multi_num_shards": (C.c_int32, [vp]),
    "vgx_reg_multi_set_reduction": (C.c_int, [vp, C.c_int32]),
    "vgx_reg_multi_shard_of": (C.c_int, [vp, i32p]),
    "vgx_reg_multi_evaluate_fused": (C.c_int, [vp, f64p, C.c_int32, f64p, i32p]),
    "vgx_reg_multi_evaluate_normal": (C.c_int, [vp, f64p, C.c_int32, f64p, i32p]),
    "vgx_reg_multi_evaluate_cost": (C.c_int, [vp, f64p, C.c_int32, f64p, i32p]),
    "vgx_reg_compress_normal": (C.c_int, [f64p, f64p, f64p]),
    "vgx_submap_surface_obb": (C.c_int, [vp, f32p, f32p]),
    "vgx_submap_mission_surface_aabb": (C.c_int, [vp, f64p, f32p, f32p]),
    "vgx_find_overlapping_pairs": (C.c_int, [vp, C.c_int32, C.POINTER(vp), f64p, i32p, C.c_int32, i32p]),
    "vgx_tsdf_config_default": (None, [C.POINTER(TsdfConfig)]),
    "vgx_tsdf_layer_create": (C.c_int, [vp, C.c_float, C.c_int32, i32p, i32p, C.c_int32, C.POINTER(vp)]),
    "vgx_tsdf_layer_destroy": (C.c_int, [vp]),
    "vgx_tsdf_layer_stats": (C.c_int, [vp, i32p, i64p]),
    "vgx_tsdf_layer_reserve": (C.c_int, [vp, f32p, C.c_float]),
    "vgx_tsdf_layer_clear_dropped": (C.c_int, [vp]),
    "vgx_tsdf_layer_growths": (C.c_int64, [vp]),
    "vgx_tsdf_layer_download": (C.c_int, [vp, i32p, f32p, f32p, u8p]),
    "vgx_tsdf_layer_upload": (C.c_int, [vp, C.c_int32, i32p, f32p, f32p, u8p]),
    "vgx_tsdf_layer_merge_submaps": (C.c_int, [vp, C.c_int32, C.POINTER(vp), f32p, i64p]),
    "vgx_tsdf_layer_transform_submap": (C.c_int, [vp, vp, f32p, i64p]),
    "vgx_evaluate_layers_rmse": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.POINTER(EvaluationDetails), i32p, f32p, u8p,
                                           i32p]),
    "vgx_tsdf_integrator_create": (C.c_int, [vp, C.POINTER(TsdfConfig), vp, C.POINTER(vp)]),
    "vgx_tsdf_integrator_destroy": (C.c_int, [vp]),
    "vgx_tsdf_integrator_set_layer": (C.c_int, [vp, vp]),
    "vgx_tsdf_integrator_set_cloud_width": (C.c_int, [vp, C.c_int32]),
    "vgx_tsdf_integrate": (C.c_int, [vp, f32p, f32p, u8p, C.c_int64, C.c_int32, i64p]),
    "vgx_tsdf_integrate_device": (C.c_int, [vp, f32p, vp, vp, C.c_int64, C.c_int32, i64p]),
    "vgx_tsdf_integrate_merged": (C.c_int, [vp, f32p, f32p, u8p, C.c_int64, C.c_int32, i64p]),
    "vgx_tsdf_integrate_merged_device": (C.c_int, [vp, f32p, vp, vp, C.c_int64, C.c_int32, i64p]),
    "vgx_scan_config_default": (None, [C.POINTER(ScanConfig)]),
    "vgx_scan_layout_check": (C.c_int, [C.POINTER(ScanLayout), C.c_int64]),
    "vgx_scan_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_scan_destroy": (C.c_int, [vp]),
    "vgx_scan_decode_msg": (C.c_int, [vp, C.POINTER(ScanLayout), C.POINTER(ScanConfig), vp, C.c_int64]),
    "vgx_scan_decode_msg_device": (C.c_int, [vp, C.POINTER(ScanLayout), C.POINTER(ScanConfig), vp, C.c_int64]),
    "vgx_scan_stats": (C.c_int, [vp, i64p, i64p]),
    "vgx_scan_undistort_check": (C.c_int, [C.POINTER(ScanLayout), C.POINTER(ScanTimeField), C.POINTER(ScanTrackView), C.c_int64]),
    "vgx_scan_decode_msg_undistorted": (C.c_int, [vp, C.POINTER(ScanLayout), C.POINTER(ScanConfig), C.POINTER(ScanTimeField),
                                                  C.POINTER(ScanTrackView), vp, C.c_int64]),
    "vgx_scan_decode_msg_undistorted_device": (C.c_int, [vp, C.POINTER(ScanLayout), C.POINTER(ScanConfig), C.POINTER(ScanTimeField),
                                                         C.POINTER(ScanTrackView), vp, C.c_int64]),
    "vgx_scan_undistort_stats": (C.c_int, [vp, i64p, i64p, i64p]),
    "vgx_depth_camera_default": (None, [C.POINTER(DepthCamera)]),
    "vgx_depth_image_check": (C.c_int, [C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), C.c_int64, C.c_int64]),
    "vgx_depth_image_undistort_check": (C.c_int, [C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), C.POINTER(DepthRowTime),
                                                  C.POINTER(ScanTrackView), C.c_int64, C.c_int64]),
    "vgx_scan_decode_depth_image": (C.c_int, [vp, C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), C.POINTER(ScanConfig),
                                              vp, C.c_int64, vp, C.c_int64]),
    "vgx_scan_decode_depth_image_device": (C.c_int, [vp, C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), C.POINTER(ScanConfig),
                                                     vp, C.c_int64, vp, C.c_int64]),
    "vgx_scan_decode_depth_image_undistorted": (C.c_int, [vp, C.POINTER(DepthImageLayout), C.POINTER(DepthCamera),
                                                          C.POINTER(ScanConfig), C.POINTER(DepthRowTime), C.POINTER(ScanTrackView),
                                                          vp, C.c_int64, vp, C.c_int64]),
    "vgx_scan_decode_depth_image_undistorted_device": (C.c_int, [vp, C.POINTER(DepthImageLayout), C.POINTER(DepthCamera),
                                                                 C.POINTER(ScanConfig), C.POINTER(DepthRowTime),
                                                                 C.POINTER(ScanTrackView), vp, C.c_int64, vp, C.c_int64]),
    "vgx_scan_depth_stats": (C.c_int, [vp, i64p, i64p, i64p, i64p]),
    "vgx_tsdf_integrate_depth_image": (C.c_int, [vp, f32p, C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), vp, C.c_int64,
                                                 vp, C.c_int64, C.POINTER(ProjectiveCounts)]),
    "vgx_tsdf_integrate_depth_image_device": (C.c_int, [vp, f32p, C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), vp,
                                                        C.c_int64, vp, C.c_int64, C.POINTER(ProjectiveCounts)]),
    "vgx_tsdf_projective_box": (C.c_int, [C.POINTER(DepthImageLayout), C.POINTER(DepthCamera), C.POINTER(TsdfConfig), f32p,
                                          C.c_float, C.c_int32, i32p, i32p]),
    "vgx_atan2_rule": (C.c_float, [C.c_float, C.c_float]),
    "vgx_range_image_check": (C.c_int, [C.POINTER(LidarModel)]),
    "vgx_range_image_pixel": (C.c_int, [C.POINTER(LidarModel), C.c_float, C.c_float, C.c_float, i32p, i32p]),
    "vgx_range_image_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_range_image_destroy": (C.c_int, [vp]),
    "vgx_range_image_build": (C.c_int, [vp, C.POINTER(LidarModel), vp, C.POINTER(RangeImageCounts)]),
    "vgx_range_image_build_device": (C.c_int, [vp, C.POINTER(LidarModel), vp, vp, C.c_int64, C.POINTER(RangeImageCounts)]),
    "vgx_range_image_stats": (C.c_int, [vp, C.POINTER(RangeImageCounts), C.POINTER(LidarModel)]),
    "vgx_range_image_download": (C.c_int, [vp, f32p, u8p, i32p]),
    "vgx_tsdf_integrate_range_image": (C.c_int, [vp, f32p, vp, C.POINTER(ProjectiveCounts)]),
    "vgx_tsdf_range_image_box": (C.c_int, [C.POINTER(LidarModel), C.POINTER(RangeImageCounts), C.POINTER(TsdfConfig), f32p,
                                           C.c_float, C.c_int32, i32p, i32p]),
    "vgx_range_image_check_beams": (C.c_int, [C.POINTER(LidarBeamModel)]),
    "vgx_range_image_pixel_beams": (C.c_int, [C.POINTER(LidarBeamModel), C.c_float, C.c_float, C.c_float, i32p, i32p]),
    "vgx_range_image_build_beams": (C.c_int, [vp, C.POINTER(LidarBeamModel), vp, C.POINTER(RangeImageCounts)]),
    "vgx_range_image_build_beams_device": (C.c_int, [vp, C.POINTER(LidarBeamModel), vp, vp, C.c_int64, C.POINTER(RangeImageCounts)]),
    "vgx_range_image_beams": (C.c_int, [vp, i32p, f32p, f32p, f32p]),
    "vgx_tsdf_range_image_box_beams": (C.c_int, [C.POINTER(LidarBeamModel), C.POINTER(RangeImageCounts), C.POINTER(TsdfConfig), f32p,
                                                 C.c_float, C.c_int32, i32p, i32p]),
    "vgx_scan_download": (C.c_int, [vp, f32p, u8p]),
    "vgx_scan_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "vgx_tsdf_integrate_scan": (C.c_int, [vp, f32p, vp, C.c_int32, i64p]),
    "vgx_tsdf_integrate_merged_scan": (C.c_int, [vp, f32p, vp, C.c_int32, i64p]),
    "vgx_mesh_config_default": (None, [C.POINTER(MeshConfig)]),
    "vgx_mesh_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_mesh_destroy": (C.c_int, [vp]),
    "vgx_tsdf_layer_generate_mesh": (C.c_int, [vp, C.POINTER(MeshConfig), vp]),
    "vgx_submap_generate_mesh": (C.c_int, [vp, C.POINTER(MeshConfig), vp]),
    "vgx_tsdf_layer_generate_mesh_colored": (C.c_int, [vp, C.POINTER(MeshConfig), vp]),
    "vgx_submap_generate_mesh_colored": (C.c_int, [vp, C.POINTER(MeshConfig), vp]),
    "vgx_mesh_stats": (C.c_int, [vp, i32p, i64p]),
    "vgx_mesh_download": (C.c_int, [vp, i32p, i64p, f32p, f32p]),
    "vgx_mesh_write_ply": (C.c_int, [vp, C.c_char_p]),
    "vgx_mesh_triangle_table": (C.c_int, [C.POINTER(C.c_int8)]),
    "vgx_submaps_generate_separated_mesh": (C.c_int, [vp, C.c_int32, C.POINTER(vp), f32p, u8p, C.POINTER(MeshConfig), vp]),
    "vgx_mesh_has_colors": (C.c_int, [vp, i32p]),
    "vgx_mesh_download_colors": (C.c_int, [vp, u8p]),
    "vgx_mesh_color_layout": (C.c_int, [vp, i32p]),
    "vgx_mesh_download_vertex_colors": (C.c_int, [vp, u8p]),
    "vgx_connected_mesh_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_connected_mesh_destroy": (C.c_int, [vp]),
    "vgx_mesh_connect": (C.c_int, [vp, C.c_float, vp]),
    "vgx_connected_mesh_stats": (C.c_int, [vp, i64p, i64p, i32p]),
    "vgx_connected_mesh_download": (C.c_int, [vp, f32p, f32p, u8p, u32p]),
    "vgx_connected_mesh_write_ply": (C.c_int, [vp, C.c_char_p]),
    "vgx_mesh_marker_config_default": (None, [C.POINTER(MeshMarkerConfig)]),
    "vgx_mesh_marker_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_mesh_marker_destroy": (C.c_int, [vp]),
    "vgx_mesh_fill_marker": (C.c_int, [vp, C.POINTER(MeshMarkerConfig), vp]),
    "vgx_mesh_marker_stats": (C.c_int, [vp, i64p, i32p]),
    "vgx_mesh_marker_download": (C.c_int, [vp, f64p, f32p]),
    "vgx_mesh_marker_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "vgx_cloud_config_default": (None, [C.POINTER(CloudConfig)]),
    "vgx_cloud_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_cloud_destroy": (C.c_int, [vp]),
    "vgx_cloud_stats": (C.c_int, [vp, i64p, i32p]),
    "vgx_cloud_download": (C.c_int, [vp, f32p, f32p, u8p]),
    "vgx_cloud_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "vgx_submap_layer_cloud": (C.c_int, [vp, C.c_int32, C.POINTER(CloudConfig), vp]),
    "vgx_tsdf_layer_cloud": (C.c_int, [vp, C.POINTER(CloudConfig), vp]),
    "vgx_planar_map_config_default": (None, [C.POINTER(PlanarMapConfig)]),
    "vgx_planar_map_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_planar_map_destroy": (C.c_int, [vp]),
    "vgx_tsdf_layer_planar_map": (C.c_int, [vp, C.POINTER(PlanarMapConfig), vp]),
    "vgx_submap_layer_planar_map": (C.c_int, [vp, C.c_int32, C.POINTER(PlanarMapConfig), vp]),
    "vgx_planar_map_stats": (C.c_int, [vp, i32p, i32p, f32p, i64p]),
    "vgx_planar_map_set_timing": (C.c_int, [vp, C.c_int32]),
    "vgx_planar_map_pass_ms": (C.c_int, [vp, f32p]),
    "vgx_planar_map_download": (C.c_int, [vp, u8p, C.POINTER(C.c_int8), f32p, f32p, f32p]),
    "vgx_planar_map_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "vgx_elevation_map_config_default": (None, [C.POINTER(ElevationMapConfig)]),
    "vgx_elevation_map_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_elevation_map_destroy": (C.c_int, [vp]),
    "vgx_tsdf_layer_elevation_map": (C.c_int, [vp, C.POINTER(ElevationMapConfig), vp]),
    "vgx_submap_layer_elevation_map": (C.c_int, [vp, C.c_int32, C.POINTER(ElevationMapConfig), vp]),
    "vgx_elevation_map_stats": (C.c_int, [vp, i32p, i32p, f32p, i64p, i64p]),
    "vgx_elevation_map_set_timing": (C.c_int, [vp, C.c_int32]),
    "vgx_elevation_map_pass_ms": (C.c_int, [vp, f32p]),
    "vgx_elevation_map_download": (C.c_int, [vp, u8p, f32p, i32p, u8p, C.POINTER(C.c_uint16), f32p, f32p, f32p, u8p, u8p, f32p]),
    "vgx_elevation_map_device_pointers": (C.c_int, [vp] + [C.POINTER(vp)] * 11),
    "vgx_evaluate_layers_rmse_cloud": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.POINTER(EvaluationDetails),
                                                 C.POINTER(CloudConfig), vp]),
    "vgx_map_msg_create": (C.c_int, [vp, C.POINTER(vp)]),
    "vgx_map_msg_destroy": (C.c_int, [vp]),
    "vgx_map_msg_stats": (C.c_int, [vp, i32p, i64p, i32p, i64p]),
    "vgx_map_msg_layer_geometry": (C.c_int, [vp, f32p, i32p]),
    "vgx_map_msg_download": (C.c_int, [vp, i32p, vp]),
    "vgx_map_msg_device_pointers": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "vgx_tsdf_layer_serialize": (C.c_int, [vp, vp]),
    "vgx_submap_serialize_layer": (C.c_int, [vp, C.c_int32, vp]),
    "vgx_submap_surface_msg": (C.c_int, [vp, C.c_int32, f32p, vp]),
    "vgx_tsdf_layer_deserialize": (C.c_int, [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, i32p, u32p, C.c_int64]),
    "vgx_tsdf_layer_deserialize_msg": (C.c_int, [vp, C.c_int32, vp]),
    "vgx_submap_query": (C.c_int, [vp, C.c_int32, C.c_int32, f32p, C.c_int64, f32p, f32p, f32p, f32p, u8p]),
    "vgx_submap_query_device": (C.c_int, [vp, C.c_int32, C.c_int32, f32p, C.c_int64, vp, vp, vp, vp, vp]),
    "vgx_map_file_open": (C.c_int, [C.c_char_p, C.c_int32, C.POINTER(vp)]),
    "vgx_map_file_close": (C.c_int, [vp]),
    "vgx_map_file_last_error": (C.c_char_p, [vp]),
    "vgx_map_file_num_submaps": (C.c_int32, [vp]),
    "vgx_map_file_get_submap_info": (C.c_int, [vp, C.c_int32, C.POINTER(MapFileSubmapInfo)]),
    "vgx_map_file_read_submap": (C.c_int, [vp, C.c_int32, i32p, f32p, f32p, u8p, f32p, u8p]),
    "vgx_map_file_load_submap": (C.c_int, [vp, vp, C.c_int32, C.POINTER(vp)]),
    "vgx_map_file_write": (C.c_int, [C.c_char_p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                     C.POINTER(MapFileSubmapData)]),
    "vgx_pose_graph_create": (C.c_int, [vp, C.c_int32, i32p, C.POINTER(vp)]),
    "vgx_pose_graph_destroy": (C.c_int, [vp]),
    "vgx_pose_graph_set_registration": (C.c_int, [vp, vp]),
    "vgx_pose_graph_set_edges": (C.c_int, [vp, C.c_int32, C.POINTER(PoseGraphEdge)]),
    "vgx_pose_graph_options_default": (None, [C.POINTER(PoseGraphOptions)]),
    "vgx_pose_graph_optimize": (C.c_int, [vp, C.POINTER(PoseGraphOptions), f64p, C.POINTER(PoseGraphSummary)]),
    "vgx_pose_graph_history": (C.c_int, [vp, C.c_int32, C.POINTER(PoseGraphIteration), i32p]),
    "vgx_pose_graph_download_system": (C.c_int, [vp, i32p, f64p, f64p]),
    "vgx_dense_spd_solve": (C.c_int, [vp, C.c_int32, f64p, f64p, f64p, f64p]),
    "vgx_pose_graph_covariance": (C.c_int, [vp, f64p, C.c_int32, C.c_int32, i32p, f64p]),
    "vgx_dense_spd_solve_many": (C.c_int, [vp, C.c_int32, f64p, C.c_int32, f64p, f64p, f64p]),
    "vgx_pose_graph_set_linear_solver": (C.c_int, [vp, C.c_int32, C.c_int32, i32p]),
    "vgx_pose_graph_create_with_solver": (C.c_int, [vp, C.c_int32, i32p, C.c_int32, C.c_int32, i32p, C.POINTER(vp)]),
    "vgx_pose_graph_structure": (C.c_int, [vp, C.POINTER(PoseGraphStructureStats)]),
    "vgx_pose_graph_order": (C.c_int, [vp, i32p]),
    "vgx_pose_graph_tile_pattern": (C.c_int, [C.c_int32, C.c_int32, i32p, C.c_int32, i32p, i32p, C.c_int32, i32p, i32p]),
    "vgx_block_spd_solve": (C.c_int, [vp, C.c_int32, C.c_int32, i32p, i32p, f64p, f64p, f64p, C.POINTER(PoseGraphStructureStats),
                                      i32p, f64p]),
    "vgx_pose_graph_covariance_sparse": (C.c_int, [vp, f64p, C.c_int32, C.c_int32, i32p, C.c_int64, f64p,
                                                   C.POINTER(PoseGraphCovarianceStats)]),
    "vgx_block_spd_solve_many": (C.c_int, [vp, C.c_int32, C.c_int32, i32p, i32p, f64p, C.c_int32, f64p, f64p]),
    "vgx_scan_registration_config_default": (None, [C.POINTER(ScanRegistrationConfig)]),
    "vgx_scan_registration_create": (C.c_int, [vp, C.POINTER(ScanRegistrationConfig), C.POINTER(vp)]),
    "vgx_scan_registration_destroy": (C.c_int, [vp]),
    "vgx_scan_registration_set_points": (C.c_int, [vp, f32p, C.c_int64]),
    "vgx_scan_registration_set_points_device": (C.c_int, [vp, vp, C.c_int64]),
    "vgx_scan_registration_set_scan": (C.c_int, [vp, vp]),
    "vgx_scan_registration_evaluate": (C.c_int, [vp, vp, f32p, f64p, f64p, i64p, i64p]),
    "vgx_scan_registration_refine": (C.c_int, [vp, vp, f32p, C.POINTER(PoseGraphOptions), f32p, f64p,
                                               C.POINTER(ScanRegistrationSummary)]),
    "vgx_scan_registration_history": (C.c_int, [vp, C.c_int32, C.POINTER(PoseGraphIteration), i32p]),
    "vgx_scan_map_config_default": (None, [C.POINTER(ScanMapConfig)]),
    "vgx_scan_registration_set_map": (C.c_int, [vp, C.POINTER(ScanMapConfig), C.c_int32, C.POINTER(vp), f32p]),
    "vgx_scan_registration_evaluate_map": (C.c_int, [vp, f32p, f64p, f64p, i64p, i64p, i64p]),
    "vgx_scan_registration_refine_map": (C.c_int, [vp, f32p, C.POINTER(PoseGraphOptions), f32p, f64p,
                                                   C.POINTER(ScanRegistrationSummary)]),
    "vgx_scan_registration_score_poses": (C.c_int, [vp, C.c_int32, f32p, f64p, i64p, i64p, i64p]),
    "vgx_scan_registration_localize": (C.c_int, [vp, C.c_int32, f32p, C.POINTER(PoseGraphOptions), i32p, f32p, f64p,
                                                 C.POINTER(ScanRegistrationSummary)]),
    "vgx_view_config_default": (None, [C.POINTER(ViewConfig)]),
    "vgx_view_config_check": (C.c_int, [C.POINTER(ViewConfig)]),
    "vgx_view_create": (C.c_int, [vp, C.POINTER(ViewConfig), C.POINTER(vp)]),
    "vgx_view_destroy": (C.c_int, [vp]),
    "vgx_view_stats": (C.c_int, [vp, C.POINTER(ViewCounts)]),
    "vgx_view_download": (C.c_int, [vp, f32p, u8p, f32p, f32p, f32p, u32p, i32p]),
    "vgx_view_device_pointers": (C.c_int, [vp] + [C.POINTER(vp)] * 7),
    "vgx_tsdf_layer_render_view": (C.c_int, [vp, vp, f32p, C.c_int64, f32p]),
    "vgx_tsdf_layer_render_view_device": (C.c_int, [vp, vp, f32p, C.c_int64, vp]),
    "vgx_submap_render_view": (C.c_int, [vp, vp, f32p, C.c_int64, f32p]),
    "vgx_submap_render_view_device": (C.c_int, [vp, vp, f32p, C.c_int64, vp]),
    "vgx_view_rays_pinhole": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, f32p]),
    "vgx_view_rays_lidar": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, f32p]),
    "vgx_view_rays_lidar_beams": (C.c_int, [C.POINTER(LidarBeamModel), f32p]),
}

# every symbol include/voxgraph_amd_bench.h declares (libvoxgraph_amd_bench.so: test and benchmark tooling)
BENCH_SIGNATURES = {
    "vgx_synth_city_submap": (C.c_int, [vp, C.c_int32, C.c_float, C.c_int32, i32p, i32p, C.c_float,
                                        C.c_float, C.c_float, f64p, C.c_uint32, C.c_int32,
                                        C.POINTER(vp)]),
    "vgx_synth_city_scan": (C.c_int, [vp, f64p, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                      C.c_uint32, vp]),
    "vgx_bench_atomic_roundtrip": (C.c_int, [vp, C.c_int64, C.c_int32, C.c_int32, f32p]),
    "vgx_bench_stream_ceiling": (C.c_int, [vp, vp, C.c_int64, vp, C.c_int64, C.c_int32, f32p]),
    "vgx_bench_alloc_scattered": (C.c_int, [vp, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(vp)]),
    "vgx_bench_free_scattered": (C.c_int, [vp, vp]),
    "vgx_tsdf_integrator_walk_stats": (C.c_int, [vp, i64p]),
    "vgx_tsdf_integrator_read_trace": (C.c_int, [vp, i64p, C.c_int64, i64p, i64p]),
    "vgx_tsdf_integrator_set_speculation": (C.c_int, [vp, C.c_int32, C.c_int64]),
    "vgx_tsdf_integrator_set_event_trace": (C.c_int, [vp, C.c_int64]),
    "vgx_tsdf_integrator_read_event_trace": (C.c_int, [vp, C.POINTER(C.c_uint64), C.c_int64, i64p, i64p]),
    "vgx_tsdf_integrator_download_sets": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i64p]),
    "vgx_scan_set_age": (C.c_int, [vp, C.c_int64, C.c_int64]),
    "vgx_scan_get_age": (C.c_int, [vp, i64p, i64p]),
    "vgx_tsdf_integrator_set_projective_age": (C.c_int, [vp, C.c_int64, C.c_int64]),
    "vgx_tsdf_integrator_get_projective_age": (C.c_int, [vp, i64p, i64p]),
    "vgx_tsdf_integrator_set_reproducible_age": (C.c_int, [vp, C.c_int64]),
    "vgx_tsdf_integrator_get_reproducible_age": (C.c_int, [vp, i64p]),
}

CHAIN_EPOCH_MAX = (1 << 30) - 1   # csrc/vgx_chain_clock.h kChainEpochMax

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; two HIP
    runtimes in one process cannot both open the GPU.  If torch is installed, load
    ITS runtime first (RTLD_GLOBAL): libvoxgraph_amd.so's DT_NEEDED libamdhip64.so.7
    then resolves to the same copy by SONAME, and a later `import torch` reuses it."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    """dlopen libvoxgraph_amd.so and bind every declared symbol (loud on failure)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _share_hip_runtime_with_torch()
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)   # (the tooling library resolves its undefined symbols in it)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)     # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = _Libraries(lib)
    return _lib


class _Libraries:
    """The product library, plus -- bound at the first use of one of its symbols -- the tooling library: tests and bench.py
    call both through `ctx.lib`; an integration loads libvoxgraph_amd.so alone."""

    def __init__(self, product):
        self.product = product
        self.tooling = None

    def __getattr__(self, name):
        if name in SIGNATURES:
            return getattr(self.product, name)
        if name in BENCH_SIGNATURES:
            if self.tooling is None:
                if not os.path.exists(BENCH_LIB_PATH):
                    raise ImportError(f"{BENCH_LIB_PATH} is missing: build it with __graft_entry__.build()")
                tooling = C.CDLL(BENCH_LIB_PATH)
                for sym, (res, args) in BENCH_SIGNATURES.items():
                    fn = getattr(tooling, sym)
                    fn.restype = res
                    fn.argtypes = args
                self.tooling = tooling
            return getattr(self.tooling, name)
        raise AttributeError(name)


class VgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"vgx error {code}: {msg}")
        self.code = code


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Context:
    def __init__(self, device=0):
        self.lib = load()
        h = vp()
        rc = self.lib.vgx_ctx_create(device, C.byref(h))
        if rc != OK:
            raise VgxError(rc, self.lib.vgx_last_error(None).decode())
        self.h = h

    def check(self, rc):
        if rc < 0:
            raise VgxError(rc, self.lib.vgx_last_error(self.h).decode())
        return rc

    def set_stream(self, stream_ptr):
        self.check(self.lib.vgx_ctx_set_stream(self.h, vp(stream_ptr)))

    def get_stream(self):
        """the hipStream_t (as an int) the library launches on"""
        return int(self.lib.vgx_ctx_get_stream(self.h) or 0)

    def set_tsdf_stream(self, stream_ptr):
        """the TSDF side's stream (layers, integrators, scans); None restores the context's own"""
        self.check(self.lib.vgx_ctx_set_tsdf_stream(self.h, vp(stream_ptr) if stream_ptr else None))

    def get_tsdf_stream(self):
        return int(self.lib.vgx_ctx_get_tsdf_stream(self.h) or 0)

    def synchronize(self):
        self.check(self.lib.vgx_ctx_synchronize(self.h))

    def synchronize_tsdf(self):
        """waits for the TSDF side alone (a scan is in), whatever the registration side has queued"""
        self.check(self.lib.vgx_ctx_synchronize_tsdf(self.h))

    def tsdf_wait_for_stream(self, producer_stream=None):
        """the TSDF stream waits on the device for what producer_stream (None: the registration stream) holds now"""
        self.check(self.lib.vgx_ctx_tsdf_wait_for_stream(self.h, vp(int(producer_stream)) if producer_stream else None))

    def stream_priorities(self):
        return bool(self.lib.vgx_ctx_stream_priorities(self.h))

    def set_brick_layout(self, layout):
        """BRICKS_APRON (default) or BRICKS_QUAD, for the submaps created from now on"""
        self.check(self.lib.vgx_ctx_set_brick_layout(self.h, int(layout)))

    def set_sampling_bricks(self, mode):
        """SAMPLING_BRICKS_QUAD (default: all-sampling batches read quad bricks made on demand) or _SAME"""
        self.check(self.lib.vgx_ctx_set_sampling_bricks(self.h, int(mode)))

    def timer_start(self):
        self.check(self.lib.vgx_ctx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self.check(self.lib.vgx_ctx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.lib.vgx_ctx_destroy(self.h)
            self.h = None


MapQuery = collections.namedtuple("MapQuery", ["distance", "gradient", "weight", "valid"])


class Submap:
    """A finished VoxgraphSubmap resident on the GPU."""

    def __init__(self, ctx, submap_id, voxel_size, vps, block_index, tsdf_distance=None,
                 tsdf_weight=None, esdf_distance=None, esdf_observed=None):
        self.ctx = ctx
        bi = np.ascontiguousarray(block_index, dtype=np.int32).reshape(-1, 3)
        td, tw, ed = _f32(tsdf_distance), _f32(tsdf_weight), _f32(esdf_distance)
        eo = None if esdf_observed is None else np.ascontiguousarray(esdf_observed, np.uint8)
        h = vp()
        ctx.check(ctx.lib.vgx_submap_create(ctx.h, submap_id, float(voxel_size), vps, bi.shape[0],
                                            _ptr(bi, i32p), _ptr(td, f32p), _ptr(tw, f32p),
                                            _ptr(ed, f32p), _ptr(eo, u8p), C.byref(h)))
        self.h = h
        self.voxel_size, self.vps = float(voxel_size), int(vps)

    @classmethod
    def synth_city(cls, ctx, submap_id, voxel_size, vps, block_min, block_dims, truncation,
                   esdf_max, tsdf_weight, true_pose, seed, build_tsdf_grid=False):
        """Benchmark tooling: analytic city scene generated on the device."""
        self = cls.__new__(cls)
        self.ctx = ctx
        bmin = np.ascontiguousarray(block_min, np.int32)
        bdim = np.ascontiguousarray(block_dims, np.int32)
        pose = _f64(true_pose)
        h = vp()
        ctx.check(ctx.lib.vgx_synth_city_submap(
            ctx.h, submap_id, float(voxel_size), vps, _ptr(bmin, i32p), _ptr(bdim, i32p),
            float(truncation), float(esdf_max), float(tsdf_weight), _ptr(pose, f64p), seed,
            int(build_tsdf_grid), C.byref(h)))
        self.h = h
        self.voxel_size, self.vps = float(voxel_size), int(vps)
        return self

    @classmethod
    def from_tsdf_layer(cls, ctx, layer, submap_id):
        """finishSubmap() hand-off on the device (no host round trip)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_submap_from_tsdf_layer(ctx.h, layer.h, submap_id, C.byref(h)))
        self.h = h
        self.voxel_size, self.vps = layer.voxel_size, layer.vps
        return self

    @classmethod
    def from_tsdf_layer_colored(cls, ctx, layer, submap_id):
        """from_tsdf_layer plus the layer's voxel colours, copied on the device (vgx_submap_from_tsdf_layer_colored)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_submap_from_tsdf_layer_colored(ctx.h, layer.h, submap_id, C.byref(h)))
        self.h = h
        self.voxel_size, self.vps = layer.voxel_size, layer.vps
        return self

    def set_colors(self, rgba):
        """rgba [n_blocks][vps^3][4] uint8 in the order of block_index() (vgx_submap_set_colors)"""
        c = None if rgba is None else np.ascontiguousarray(rgba, np.uint8)
        if c is not None and c.size != self.num_blocks() * self.vps ** 3 * 4:
            raise ValueError("rgba must hold n_blocks * vps^3 * 4 bytes")
        self.ctx.check(self.ctx.lib.vgx_submap_set_colors(self.h, _ptr(c, u8p)))

    def has_colors(self):
        """True for a submap that carries voxel colours (vgx_submap_has_colors)"""
        has = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_submap_has_colors(self.h, C.byref(has)))
        return bool(has.value)

    def download_colors(self):
        """rgba [n_blocks][vps^3][4] uint8 (vgx_submap_download_colors; a submap without colours raises)"""
        out = np.zeros((self.num_blocks(), self.vps ** 3, 4), np.uint8)
        self.ctx.check(self.ctx.lib.vgx_submap_download_colors(self.h, _ptr(out, u8p)))
        return out

    def generate_esdf(self, config=None):
        """cblox::TsdfEsdfSubmap::generateEsdf() on the device; returns global passes used."""
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_submap_generate_esdf(
            self.h, C.byref(config) if config is not None else None, C.byref(n)))
        return n.value

    def num_blocks(self):
        return self.ctx.lib.vgx_submap_num_blocks(self.h)

    def block_index(self):
        bi = np.zeros((self.num_blocks(), 3), np.int32)
        self.ctx.check(self.ctx.lib.vgx_submap_block_index(self.h, _ptr(bi, i32p)))
        return bi

    def download_layers(self, vps):
        n = self.num_blocks()
        td = np.zeros((n, vps ** 3), np.float32)
        tw = np.zeros((n, vps ** 3), np.float32)
        ed = np.zeros((n, vps ** 3), np.float32)
        eo = np.zeros((n, vps ** 3), np.uint8)
        self.ctx.check(self.ctx.lib.vgx_submap_download_layers(
            self.h, _ptr(td, f32p), _ptr(tw, f32p), _ptr(ed, f32p), _ptr(eo, u8p)))
        return td, tw, ed, eo

    def set_points(self, point_type, xyz, distance, weight, flags=POINTS_KEEP_ORDER):
        xyz = _f32(xyz).reshape(-1, 3)
        d, w = _f32(distance), _f32(weight)
        self.ctx.check(self.ctx.lib.vgx_submap_set_points(
            self.h, point_type, xyz.shape[0], _ptr(xyz, f32p), _ptr(d, f32p), _ptr(w, f32p), flags))

    def extract_voxel_points(self, min_voxel_weight=1.0, max_voxel_distance=0.3,
                             use_esdf_distance=True):
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_submap_extract_voxel_points(
            self.h, min_voxel_weight, max_voxel_distance, int(use_esdf_distance), C.byref(n)))
        return n.value

    def extract_isosurface_points(self, min_voxel_weight=1.0):
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_submap_extract_isosurface_points(
            self.h, min_voxel_weight, C.byref(n)))
        return n.value

    def surface_obb(self):
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self.ctx.check(self.ctx.lib.vgx_submap_surface_obb(self.h, _ptr(mn, f32p), _ptr(mx, f32p)))
        return mn, mx

    def mission_surface_aabb(self, pose):
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self.ctx.check(self.ctx.lib.vgx_submap_mission_surface_aabb(
            self.h, _ptr(_f64(pose), f64p), _ptr(mn, f32p), _ptr(mx, f32p)))
        return mn, mx

    def num_points(self, point_type):
        return self.ctx.lib.vgx_submap_num_points(self.h, point_type)

    def point_order(self, point_type):
        n = self.num_points(point_type)
        order = np.zeros(max(n, 0), np.int64)
        self.ctx.check(self.ctx.lib.vgx_submap_point_order(self.h, point_type, _ptr(order, i64p)))
        return order

    def download_points(self, point_type):
        n = self.num_points(point_type)
        xyz = np.zeros((n, 3), np.float32)
        d = np.zeros(n, np.float32)
        w = np.zeros(n, np.float32)
        self.ctx.check(self.ctx.lib.vgx_submap_download_points(
            self.h, point_type, _ptr(xyz, f32p), _ptr(d, f32p), _ptr(w, f32p)))
        return xyz, d, w

    def generate_mesh(self, mesh=None, min_weight=1e-4):
        """MeshIntegrator::generateMesh(false, false) over the submap's raw TSDF layer, in the submap frame
        (vgx_submap_generate_mesh).  Returns the Mesh (a new one when mesh is None)."""
        mesh = mesh if mesh is not None else Mesh(self.ctx)
        cfg = MeshConfig(float(min_weight))
        self.ctx.check(self.ctx.lib.vgx_submap_generate_mesh(self.h, C.byref(cfg), mesh.h))
        return mesh

    def generate_mesh_colored(self, mesh=None, min_weight=1e-4):
        """generate_mesh plus one TSDF colour per soup vertex, MeshIntegratorConfig::use_color
        (vgx_submap_generate_mesh_colored; a submap without colours raises).  Returns the Mesh."""
        mesh = mesh if mesh is not None else Mesh(self.ctx)
        cfg = MeshConfig(float(min_weight))
        self.ctx.check(self.ctx.lib.vgx_submap_generate_mesh_colored(self.h, C.byref(cfg), mesh.h))
        return mesh

    def _query_args(self, layer, interpolate, gradient, pose, weight):
        lay = {"esdf": EVAL_LAYER_ESDF, "tsdf": EVAL_LAYER_TSDF}.get(layer, layer)
        flags = (QUERY_INTERPOLATE if interpolate else 0) | (QUERY_GRADIENT if gradient else 0)
        T = None if pose is None else np.ascontiguousarray(pose, np.float32).reshape(7)
        return int(lay), flags, T

    def query(self, points, layer="esdf", interpolate=True, gradient=False, pose=None, weight=False):
        """voxblox's EsdfMap / TsdfMap lookups at points [n][3] (vgx_submap_query): layer "esdf" or "tsdf", interpolate
        (getInterpDistance; else the nearest voxel), gradient (getGradient), pose T_Q_S [7] (qw,qx,qy,qz, tx,ty,tz: the
        points are in frame Q; None: the submap frame), weight (TSDF only).  Returns MapQuery(distance [n], gradient [n][3]
        or None, weight [n] or None, valid [n] bool); an invalid query has valid False and zeros elsewhere."""
        lay, flags, T = self._query_args(layer, interpolate, gradient, pose, weight)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        d = np.zeros(n, np.float32)
        g = np.zeros((n, 3), np.float32) if gradient else None
        w = np.zeros(n, np.float32) if weight else None
        v = np.zeros(n, np.uint8)
        self.ctx.check(self.ctx.lib.vgx_submap_query(self.h, lay, flags, _ptr(T, f32p), n, _ptr(pts, f32p), _ptr(d, f32p),
                                                     _ptr(g, f32p), _ptr(w, f32p), _ptr(v, u8p)))
        return MapQuery(d, g, w, v.view(np.bool_))

    def query_device(self, points, layer="esdf", interpolate=True, gradient=False, pose=None, weight=False, sync=True):
        """query() over torch tensors on the context's device (vgx_submap_query_device): points float32 [n][3] ->
        MapQuery of tensors (valid as uint8).  The caller's current stream is waited for first; sync=False returns once the
        work is queued on the context's registration stream (ctx.synchronize() waits for it)."""
        import torch
        lay, flags, T = self._query_args(layer, interpolate, gradient, pose, weight)
        pts = points.to(torch.float32).contiguous().reshape(-1, 3)
        n = pts.shape[0]
        d = torch.empty(n, dtype=torch.float32, device=pts.device)
        g = torch.empty((n, 3), dtype=torch.float32, device=pts.device) if gradient else None
        w = torch.empty(n, dtype=torch.float32, device=pts.device) if weight else None
        v = torch.empty(n, dtype=torch.uint8, device=pts.device)
        torch.cuda.current_stream(pts.device).synchronize()
        self.ctx.check(self.ctx.lib.vgx_submap_query_device(
            self.h, lay, flags, _ptr(T, f32p), n, vp(pts.data_ptr()), vp(d.data_ptr()),
            vp(g.data_ptr()) if g is not None else None, vp(w.data_ptr()) if w is not None else None, vp(v.data_ptr())))
        if sync:
            self.ctx.synchronize()
        return MapQuery(d, g, w, v)

    def layer_cloud(self, layer="esdf", config=None, cloud=None):
        """The point-cloud view of the raw ESDF or TSDF layer (vgx_submap_layer_cloud; config: cloud_config(...)).
        Returns the Cloud (a new one when cloud is None)."""
        cloud = cloud if cloud is not None else Cloud(self.ctx)
        which = {"esdf": EVAL_LAYER_ESDF, "tsdf": EVAL_LAYER_TSDF}.get(layer, layer)
        self.ctx.check(self.ctx.lib.vgx_submap_layer_cloud(self.h, int(which), None if config is None else C.byref(config),
                                                           cloud.h))
        return cloud

    def layer_planar_map(self, layer, config, planar_map=None):
        """The planar map of the raw ESDF or TSDF layer's height band (vgx_submap_layer_planar_map; config:
        planar_map_config(z_min=..., z_max=..., ...)).  Returns the PlanarMap (a new one when planar_map is None)."""
        planar_map = planar_map if planar_map is not None else PlanarMap(self.ctx)
        which = {"esdf": EVAL_LAYER_ESDF, "tsdf": EVAL_LAYER_TSDF}.get(layer, layer)
        self.ctx.check(self.ctx.lib.vgx_submap_layer_planar_map(self.h, int(which), None if config is None else C.byref(config),
                                                                planar_map.h))
        return planar_map

    def layer_elevation_map(self, layer, config, elevation_map=None):
        """The elevation map of the raw ESDF or TSDF layer's height band (vgx_submap_layer_elevation_map; config:
        elevation_map_config(z_min=..., z_max=..., ...)).  Returns the ElevationMap (a new one when elevation_map is None)."""
        elevation_map = elevation_map if elevation_map is not None else ElevationMap(self.ctx)
        which = {"esdf": EVAL_LAYER_ESDF, "tsdf": EVAL_LAYER_TSDF}.get(layer, layer)
        self.ctx.check(self.ctx.lib.vgx_submap_layer_elevation_map(self.h, int(which), None if config is None else C.byref(config),
                                                                   elevation_map.h))
        return elevation_map

    def serialize_layer(self, layer="tsdf", msg=None):
        """voxblox::serializeLayerAsMsg of the raw TSDF or ESDF layer (vgx_submap_serialize_layer).  Returns the MapMsg
        (a new one when msg is None)."""
        msg = msg if msg is not None else MapMsg(self.ctx)
        which = {"esdf": EVAL_LAYER_ESDF, "tsdf": EVAL_LAYER_TSDF}.get(layer, layer)
        self.ctx.check(self.ctx.lib.vgx_submap_serialize_layer(self.h, int(which), msg.h))
        return msg

    def surface_msg(self, point_type=POINTS_ISOSURFACE, T=None, msg=None):
        """The data bytes of publishSubmapSurfacePointcloud's PointXYZI cloud (vgx_submap_surface_msg); T: a row-major
        3 x 4 f32 affine or None.  Returns the MapMsg (a new one when msg is None)."""
        msg = msg if msg is not None else MapMsg(self.ctx)
        t = None if T is None else np.ascontiguousarray(T, np.float32).reshape(12)
        self.ctx.check(self.ctx.lib.vgx_submap_surface_msg(self.h, int(point_type), _ptr(t, f32p), msg.h))
        return msg

    def render_view(self, view, T_S_C, dirs, n=None):
        """The view of this submap's raw TSDF layer from sensor pose T_S_C (submap frame) along dirs [n][3]
        (vgx_submap_render_view / _device: a numpy array, a torch device tensor, or a device address with n).  Returns
        the View."""
        lib = self.ctx.lib
        return _render_view(self.ctx, lib.vgx_submap_render_view, lib.vgx_submap_render_view_device, self, view, T_S_C, dirs, n)

    def release_raw_layers(self):
        self.ctx.check(self.ctx.lib.vgx_submap_release_raw_layers(self.h))

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_submap_destroy(self.h)
            self.h = None


def default_config(**kw):
    cfg = RegConfig()
    load().vgx_reg_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


class RegistrationCostFunction:
    """Mirror of voxgraph::RegistrationCostFunction over the C ABI.

    Evaluate(parameters, residuals, jacobians) follows ceres::CostFunction::Evaluate
    (registration_cost_function.h:47-48): parameters = [ref_pose[4], read_pose[4]],
    residuals = f64[N], jacobians = None or [f64[N,4] or None, f64[N,4] or None].
    Returns True/False like the reference.
    """

    def __init__(self, ctx, reference_submap, reading_submap, config=None):
        self.ctx = ctx
        self.config = config if config is not None else default_config()
        h = vp()
        ctx.check(ctx.lib.vgx_reg_create(ctx.h, reference_submap.h, reading_submap.h,
                                         C.byref(self.config), C.byref(h)))
        self.h = h
        self._keep = (reference_submap, reading_submap)

    def num_residuals(self):
        return self.ctx.lib.vgx_reg_num_residuals(self.h)

    def Evaluate(self, parameters, residuals, jacobians):
        ref = _f64(parameters[0])
        read = _f64(parameters[1])
        jr = je = None
        if jacobians is not None:
            jr, je = jacobians[0], jacobians[1]
        for a in (residuals, jr, je):
            assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous)
        rc = self.ctx.check(self.ctx.lib.vgx_reg_evaluate(
            self.h, _ptr(ref, f64p), _ptr(read, f64p), _ptr(residuals, f64p), _ptr(jr, f64p),
            _ptr(je, f64p)))
        return rc == OK

    def evaluate_visuals(self, parameters, residuals, jacobians, visuals, want_residual_cloud=True, want_gradients=True):
        """Evaluate plus the cost-function visuals of that same evaluation (vgx_reg_evaluate_visuals): the rows come
        back as in Evaluate, `visuals` (a RegVisuals) is left holding the residual cloud and -- when Jacobians were
        asked for -- the Jacobian markers.  `visuals` may be None only to see the call refused."""
        ref = _f64(parameters[0])
        read = _f64(parameters[1])
        jr = je = None
        if jacobians is not None:
            jr, je = jacobians[0], jacobians[1]
        for a in (residuals, jr, je):
            assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous)
        rc = self.ctx.check(self.ctx.lib.vgx_reg_evaluate_visuals(
            self.h, _ptr(ref, f64p), _ptr(read, f64p), _ptr(residuals, f64p), _ptr(jr, f64p), _ptr(je, f64p),
            1 if want_residual_cloud else 0, 1 if want_gradients else 0, visuals.h if visuals is not None else None))
        return rc == OK

    def evaluate_device_f32(self, ref_pose, read_pose, d_residuals, d_jac_ref, d_jac_read):
        """Device pointers (ints); asynchronous on the context's stream."""
        rc = self.ctx.check(self.ctx.lib.vgx_reg_evaluate_device_f32(
            self.h, _ptr(_f64(ref_pose), f64p), _ptr(_f64(read_pose), f64p), vp(d_residuals),
            vp(d_jac_ref) if d_jac_ref else None, vp(d_jac_read) if d_jac_read else None))
        return rc == OK

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_reg_destroy(self.h)
            self.h = None


Registration = RegistrationCostFunction


class RegVisuals:
    """The cost-function visuals of one evaluation on the GPU (vgx_reg_visuals): the residual cloud as 32-byte
    pcl::PointXYZI records and the Jacobian markers' points; reused from call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_reg_visuals_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """(residual points, Jacobians) of the last evaluation into this handle"""
        n, m = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_reg_visuals_stats(self.h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def download(self):
        """(cloud bytes [n][32] u8, arrow points [2m][3] f64, origin points [m][3] f64, factor)"""
        n, m = self.stats()
        cloud = np.zeros((n, 32), np.uint8)
        arrows = np.zeros((2 * m, 3), np.float64)
        origins = np.zeros((m, 3), np.float64)
        factor = C.c_double()
        self.ctx.check(self.ctx.lib.vgx_reg_visuals_download(self.h, cloud.ctypes.data_as(vp), _ptr(arrows, f64p),
                                                             _ptr(origins, f64p), C.byref(factor)))
        return cloud, arrows, origins, factor.value

    def device_pointers(self):
        """(cloud, arrow points, origin points) device addresses as ints (None for an array with 0 rows)"""
        p = [vp(), vp(), vp()]
        self.ctx.check(self.ctx.lib.vgx_reg_visuals_device_pointers(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_reg_visuals_destroy(self.h)
            self.h = None


class RegistrationBatch:
    """All registration constraints of a pose graph, evaluated in one launch."""

    def __init__(self, ctx, cost_functions, node_pair, global_index=None, n_global=None):
        self.ctx = ctx
        self.n = len(cost_functions)
        arr = (vp * max(self.n, 1))(*[cf.h for cf in cost_functions])
        np_pair = np.ascontiguousarray(node_pair, dtype=np.int32).reshape(-1, 2)
        gi = None if global_index is None else np.ascontiguousarray(global_index, np.int32)
        h = vp()
        ctx.check(ctx.lib.vgx_reg_batch_create(
            ctx.h, self.n, arr, _ptr(np_pair, i32p), _ptr(gi, i32p),
            self.n if n_global is None else n_global, C.byref(h)))
        self.h = h
        self.n_global = self.n if n_global is None else n_global
        self._keep = list(cost_functions)

    def num_residuals(self):
        return self.ctx.lib.vgx_reg_batch_num_residuals(self.h)

    def row_offsets(self):
        ro = np.zeros(self.n + 1, np.int64)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_row_offsets(self.h, _ptr(ro, i64p)))
        return ro

    def evaluate_points(self, poses, d_residuals, d_jac_ref, d_jac_read):
        poses = _f64(poses).reshape(-1, 4)
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_evaluate_points(
            self.h, _ptr(poses, f64p), poses.shape[0], vp(d_residuals),
            vp(d_jac_ref) if d_jac_ref else None, vp(d_jac_read) if d_jac_read else None,
            _ptr(status, i32p)))
        return status[:self.n]

    def evaluate_points_f64(self, poses, d_residuals, d_jac_ref, d_jac_read):
        """vgx_reg_batch_evaluate_points_f64: the same rows as f64 (Ceres' own types) into device arrays"""
        poses = _f64(poses).reshape(-1, 4)
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_evaluate_points_f64(
            self.h, _ptr(poses, f64p), poses.shape[0], vp(d_residuals),
            vp(d_jac_ref) if d_jac_ref else None, vp(d_jac_read) if d_jac_read else None,
            _ptr(status, i32p)))
        return status[:self.n]

    def evaluate_rows_f64(self, poses, want_jac_ref=True, want_jac_read=True):
        """vgx_reg_batch_evaluate_rows_f64: f64 rows kept by the batch -> status per constraint"""
        poses = _f64(poses).reshape(-1, 4)
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_evaluate_rows_f64(self.h, _ptr(poses, f64p), poses.shape[0], int(want_jac_ref),
                                                                    int(want_jac_read), _ptr(status, i32p)))
        return status[:self.n]

    def fetch_rows_f64(self, c, n, want_jac_ref=True, want_jac_read=True):
        """vgx_reg_batch_fetch_rows_f64: constraint c's slice (n = its residuals) -> (residuals, jac_ref or None, jac_read or None)"""
        r = np.full(n, np.nan)
        jo = np.full((n, 4), np.nan) if want_jac_ref else None
        je = np.full((n, 4), np.nan) if want_jac_read else None
        self.ctx.check(self.ctx.lib.vgx_reg_batch_fetch_rows_f64(self.h, int(c), _ptr(r, f64p), _ptr(jo, f64p), _ptr(je, f64p)))
        return r, jo, je

    def blocked_layout(self):
        """vgx_reg_batch_blocked_layout -> (bytes, rows per block, first_block [n + 1])"""
        nbytes, rows = C.c_int64(), C.c_int32()
        first = np.zeros(self.n + 1, np.int64)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_blocked_layout(self.h, C.byref(nbytes), C.byref(rows),
                                                                 first.ctypes.data_as(C.POINTER(C.c_int64))))
        return int(nbytes.value), int(rows.value), first

    def evaluate_points_blocked(self, poses, d_blocks):
        poses = _f64(poses).reshape(-1, 4)
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_evaluate_points_blocked(self.h, _ptr(poses, f64p), poses.shape[0], vp(d_blocks),
                                                                          _ptr(status, i32p)))
        return status[:self.n]

    def choose_outputs(self, poses, d_residuals, d_jac_ref, d_jac_read, launches=3):
        """vgx_reg_batch_choose_outputs: lists of candidate device pointers (d_jac_ref / d_jac_read may be None) ->
        (chosen [3], ms per launch of the chosen combination, ms of every trial)"""
        poses = _f64(poses).reshape(-1, 4)
        n = len(d_residuals)
        arr = lambda ps: (vp * n)(*[vp(int(x)) for x in ps]) if ps is not None else None
        a_r, a_jr, a_je = arr(d_residuals), arr(d_jac_ref), arr(d_jac_read)
        chosen = np.zeros(3, np.int32)
        ms = C.c_float()
        trials = (C.c_float * (4 * n))()
        self.ctx.check(self.ctx.lib.vgx_reg_batch_choose_outputs(
            self.h, _ptr(poses, f64p), poses.shape[0], n, a_r, a_jr, a_je, int(launches), _ptr(chosen, i32p),
            C.byref(ms), trials))
        return [int(x) for x in chosen], float(ms.value), [float(x) for x in trials]

    def alloc_outputs(self, poses, n_candidates=4, want_jac_ref=True, want_jac_read=True):
        """vgx_reg_batch_alloc_outputs -> (residuals, jac_ref, jac_read device pointers (0 where not wanted), ms per launch)"""
        poses = _f64(poses).reshape(-1, 4)
        r, jo, je, ms = vp(), vp(), vp(), C.c_float()
        self.ctx.check(self.ctx.lib.vgx_reg_batch_alloc_outputs(self.h, _ptr(poses, f64p), poses.shape[0], int(n_candidates),
                                                                int(want_jac_ref), int(want_jac_read), C.byref(r), C.byref(jo),
                                                                C.byref(je), C.byref(ms)))
        return (r.value or 0), (jo.value or 0), (je.value or 0), float(ms.value)

    def free_outputs(self, r, jo, je):
        self.ctx.check(self.ctx.lib.vgx_reg_batch_free_outputs(self.h, vp(r) if r else None, vp(jo) if jo else None,
                                                               vp(je) if je else None))

    def evaluate_normal(self, poses, d_normal=None, to_host=True):
        poses = _f64(poses).reshape(-1, 4)
        status = np.zeros(max(self.n, 1), np.int32)
        host = np.zeros((self.n, NORMAL_SIZE), np.float64) if to_host else None
        self.ctx.check(self.ctx.lib.vgx_reg_batch_evaluate_normal(
            self.h, _ptr(poses, f64p), poses.shape[0], vp(d_normal) if d_normal else None,
            _ptr(host, f64p), _ptr(status, i32p)))
        return status[:self.n], host

    def evaluate_cost(self, poses, d_cost=None, to_host=True):
        """cost-only fused pass (vgx_reg_batch_evaluate_cost): -> (status, cost[n] f64 or None)"""
        poses = _f64(poses).reshape(-1, 4)
        status = np.zeros(max(self.n, 1), np.int32)
        host = np.zeros(self.n, np.float64) if to_host else None
        self.ctx.check(self.ctx.lib.vgx_reg_batch_evaluate_cost(
            self.h, _ptr(poses, f64p), poses.shape[0], vp(d_cost) if d_cost else None,
            _ptr(host, f64p), _ptr(status, i32p)))
        return status[:self.n], host

    def count_live(self, poses, unique=False):
        """residuals whose points the fused pass reads at these poses (chunk culling applied);
        with unique=True also the number of distinct points behind them"""
        poses = _f64(poses).reshape(-1, 4)
        n, u = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_reg_batch_count_live(self.h, _ptr(poses, f64p), poses.shape[0],
                                                             C.byref(n), C.byref(u) if unique else None))
        return (n.value, u.value) if unique else n.value

    def count_live_each(self, poses):
        """count_live per constraint (batch order)"""
        poses = _f64(poses).reshape(-1, 4)
        out = np.zeros(max(self.n, 1), np.int64)
        self.ctx.check(self.ctx.lib.vgx_reg_batch_count_live_each(self.h, _ptr(poses, f64p), poses.shape[0],
                                                                  out.ctypes.data_as(i64p)))
        return out[:self.n]

    def launch_order(self, points_pass):
        """1: constraints sharing a reference submap run side by side on one XCD (points shared in its
        L2); 0: constraint-major; -1: that pass has not run yet (vgx_reg_batch_launch_order)"""
        g = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_reg_batch_launch_order(self.h, int(bool(points_pass)), C.byref(g)))
        return g.value

    def assemble(self, n_nodes, d_fused, d_normal=None, zero_first=True):
        self.ctx.check(self.ctx.lib.vgx_reg_batch_assemble(
            self.h, vp(d_normal) if d_normal else None, n_nodes, vp(d_fused), int(zero_first)))

    def brick_layout(self):
        """BRICKS_APRON / BRICKS_QUAD: the bricks this batch reads (quad on demand when all its constraints sample)"""
        return int(self.ctx.lib.vgx_reg_batch_brick_layout(self.h))

    def scatter_normal(self, d_normal_all, d_normal=None, zero_first=True):
        """this shard's [n][45] blocks into rows global_index[c] of the DEVICE [n_global][45] array"""
        self.ctx.check(self.ctx.lib.vgx_reg_batch_scatter_normal(
            self.h, vp(d_normal) if d_normal else None, vp(d_normal_all), int(zero_first)))

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_reg_batch_destroy(self.h)
            self.h = None


def pose_graph_options(**kw):
    """vgx_pose_graph_options with the defaults of pose_graph.cpp:85-106, overridden by keyword"""
    o = PoseGraphOptions()
    load().vgx_pose_graph_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(k)
        setattr(o, k, v)
    return o


def pose_graph_edge(a, b, t_obs, yaw_obs, sqrt_information):
    e = PoseGraphEdge()
    e.a, e.b, e.yaw_obs = int(a), int(b), float(yaw_obs)
    e.t_obs[:] = [float(v) for v in t_obs]
    e.sqrt_information[:] = [float(v) for v in np.asarray(sqrt_information, np.float64).reshape(16)]
    return e


def dense_spd_solve(ctx, A, b, want_factor=True):
    """vgx_dense_spd_solve -> (x, L or None); raises VgxError(ERR_NOT_POSITIVE_DEFINITE) at a bad pivot"""
    A, b = _f64(A), _f64(b)
    n = len(b)
    x = np.zeros(n)
    L = np.zeros((n, n)) if want_factor else None
    ctx.check(ctx.lib.vgx_dense_spd_solve(ctx.h, n, _ptr(A, f64p), _ptr(b, f64p), _ptr(x, f64p), _ptr(L, f64p)))
    return x, L


def dense_spd_solve_many(ctx, A, B, want_factor=False):
    """vgx_dense_spd_solve_many: A X = B for B [n][m] -> (X [n][m], L or None); raises as dense_spd_solve does"""
    A, B = _f64(A), _f64(B)
    n, m = B.shape
    X = np.zeros((n, m))
    L = np.zeros((n, n)) if want_factor else None
    ctx.check(ctx.lib.vgx_dense_spd_solve_many(ctx.h, n, _ptr(A, f64p), m, _ptr(B, f64p), _ptr(X, f64p), _ptr(L, f64p)))
    return X, L


def tile_pattern(n_free_nodes, pairs, ordering=ORDER_NATURAL, permutation=None):
    """vgx_pose_graph_tile_pattern (host only, no context) -> (order [n_free_nodes], L tiles [n][2] as (row, column) sorted
    by (column, row)); pairs: the joined free nodes.  Raises ValueError where the library answers VGX_ERR_INVALID."""
    lib = load()
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    perm = None if permutation is None else np.ascontiguousarray(permutation, np.int32)
    if perm is not None and len(perm) != n_free_nodes:
        raise ValueError("tile_pattern: the permutation's length is not n_free_nodes")
    order = np.zeros(max(int(n_free_nodes), 1), np.int32)
    n = C.c_int32()
    args = (int(n_free_nodes), len(pr), _ptr(pr, i32p) if len(pr) else None, int(ordering), _ptr(perm, i32p))
    if lib.vgx_pose_graph_tile_pattern(*args, _ptr(order, i32p), 0, None, C.byref(n)) != OK:
        raise ValueError("vgx_pose_graph_tile_pattern refused its input")
    tiles = np.zeros((n.value, 2), np.int32)
    if lib.vgx_pose_graph_tile_pattern(*args, None, n.value, _ptr(tiles, i32p), None) != OK:
        raise ValueError("vgx_pose_graph_tile_pattern refused its input")
    return order[:n_free_nodes], tiles


def block_spd_solve(ctx, n_block_rows, bi, bj, values, b, want_factor=True):
    """vgx_block_spd_solve -> (x, stats dict, tile_index [n][2] or None, tile_values [n][64][64] or None); raises as
    dense_spd_solve does"""
    bi, bj = np.ascontiguousarray(bi, np.int32), np.ascontiguousarray(bj, np.int32)
    values, b = _f64(values), _f64(b)
    assert values.size == 16 * len(bi) == 16 * len(bj) and len(b) == 4 * n_block_rows
    x = np.zeros(4 * n_block_rows)
    stats = PoseGraphStructureStats()
    index = tiles = None
    if want_factor:
        pairs = np.stack([bi, bj], 1)
        inside = bool(len(pairs)) and pairs.min() >= 0 and pairs.max() < n_block_rows
        n_tiles = len(tile_pattern(n_block_rows, pairs)[1]) if inside else 1
        index, tiles = np.zeros((n_tiles, 2), np.int32), np.zeros((n_tiles, 64, 64))
    ctx.check(ctx.lib.vgx_block_spd_solve(ctx.h, int(n_block_rows), len(bi), _ptr(bi, i32p), _ptr(bj, i32p), _ptr(values, f64p),
                                          _ptr(b, f64p), _ptr(x, f64p), C.byref(stats), _ptr(index, i32p), _ptr(tiles, f64p)))
    return x, stats.as_dict(), index, tiles


def block_spd_solve_many(ctx, n_block_rows, bi, bj, values, B, in_place=False):
    """vgx_block_spd_solve_many: A X = B for B [4 n_block_rows][m] -> X [4 n_block_rows][m]; in_place: X is B's own array
    (B must then be a C-contiguous float64 array).  Raises as block_spd_solve does"""
    bi, bj = np.ascontiguousarray(bi, np.int32), np.ascontiguousarray(bj, np.int32)
    values = _f64(values)
    if in_place:
        assert isinstance(B, np.ndarray) and B.dtype == np.float64 and B.flags.c_contiguous
    else:
        B = _f64(B)
    n, m = B.shape
    assert values.size == 16 * len(bi) == 16 * len(bj) and n == 4 * n_block_rows
    X = B if in_place else np.zeros((n, m))
    ctx.check(ctx.lib.vgx_block_spd_solve_many(ctx.h, int(n_block_rows), len(bi), _ptr(bi, i32p), _ptr(bj, i32p), _ptr(values, f64p),
                                               m, _ptr(B, f64p), _ptr(X, f64p)))
    return X


class PoseGraph:
    """vgx_pose_graph: PoseGraph::optimize() on the device (include/voxgraph_amd.h, "Pose graph: the solve").
    linear_solver: LINEAR_SOLVER_DENSE (None: vgx_pose_graph_create) or LINEAR_SOLVER_TILE_SPARSE with an ordering."""

    def __init__(self, ctx, n_nodes, constant=None, linear_solver=None, ordering=ORDER_NATURAL, permutation=None):
        self.ctx, self.n_nodes = ctx, int(n_nodes)
        flags = None if constant is None else np.ascontiguousarray(constant, np.int32)
        h = vp()
        if linear_solver is None:
            ctx.check(ctx.lib.vgx_pose_graph_create(ctx.h, self.n_nodes, _ptr(flags, i32p), C.byref(h)))
        else:
            perm = None if permutation is None else np.ascontiguousarray(permutation, np.int32)
            ctx.check(ctx.lib.vgx_pose_graph_create_with_solver(ctx.h, self.n_nodes, _ptr(flags, i32p), int(linear_solver),
                                                                int(ordering), _ptr(perm, i32p), C.byref(h)))
        self.h = h
        self.n_free = self.n_nodes - 1 if constant is None else int(np.count_nonzero(np.asarray(constant) == 0))

    def set_linear_solver(self, solver, ordering=ORDER_NATURAL, permutation=None):
        perm = None if permutation is None else np.ascontiguousarray(permutation, np.int32)
        if perm is not None and len(perm) != self.n_free:
            raise VgxError(ERR_INVALID, "set_linear_solver: the permutation's length is not the number of free nodes")
        self.ctx.check(self.ctx.lib.vgx_pose_graph_set_linear_solver(self.h, int(solver), int(ordering), _ptr(perm, i32p)))

    def structure(self):
        """vgx_pose_graph_structure -> dict"""
        stats = PoseGraphStructureStats()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_structure(self.h, C.byref(stats)))
        return stats.as_dict()

    def order(self):
        """vgx_pose_graph_order -> [free nodes]: position -> free node"""
        out = np.zeros(max(self.n_free, 1), np.int32)
        self.ctx.check(self.ctx.lib.vgx_pose_graph_order(self.h, _ptr(out, i32p)))
        return out[:self.n_free]

    def download_gradient(self):
        """-> g [N] of the last full evaluation (the call vgx_pose_graph_download_system(graph, NULL, NULL, g))"""
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_download_system(self.h, C.byref(n), None, None))
        g = np.zeros(n.value)
        self.ctx.check(self.ctx.lib.vgx_pose_graph_download_system(self.h, None, None, _ptr(g, f64p)))
        return g

    def set_registration(self, batch):
        self.ctx.check(self.ctx.lib.vgx_pose_graph_set_registration(self.h, batch.h if batch is not None else None))

    def set_edges(self, edges):
        """edges: PoseGraphEdge items (pose_graph_edge(...))"""
        arr = (PoseGraphEdge * max(len(edges), 1))(*edges)
        self.ctx.check(self.ctx.lib.vgx_pose_graph_set_edges(self.h, len(edges), arr))

    def optimize(self, poses, options=None, **kw):
        """-> (poses [n_nodes][4], summary dict); keywords override the default options"""
        opts = options if options is not None else pose_graph_options(**kw)
        x = np.array(poses, np.float64).reshape(self.n_nodes, 4).copy()
        s = PoseGraphSummary()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_optimize(self.h, C.byref(opts), _ptr(x, f64p), C.byref(s)))
        d = s.as_dict()
        d["termination"] = TERMINATION_NAMES[s.termination_reason]
        return x, d

    def history(self):
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_history(self.h, 0, None, C.byref(n)))
        arr = (PoseGraphIteration * max(n.value, 1))()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_history(self.h, n.value, arr, None))
        return [{name: getattr(arr[k], name) for name, _ in PoseGraphIteration._fields_} for k in range(n.value)]

    def download_system(self):
        """-> (H [N][N], g [N]) of the last full evaluation, N = 4 x free nodes"""
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_download_system(self.h, C.byref(n), None, None))
        H, g = np.zeros((n.value, n.value)), np.zeros(n.value)
        self.ctx.check(self.ctx.lib.vgx_pose_graph_download_system(self.h, None, _ptr(H, f64p), _ptr(g, f64p)))
        return H, g

    def covariance(self, poses, pairs, exclude_registration=False):
        """vgx_pose_graph_covariance -> [n_pairs][4][4]: block (a, b) of H^-1 at `poses` per pair (a, b) of node indices;
        raises VgxError(ERR_NOT_POSITIVE_DEFINITE) on a rank-deficient graph"""
        x = np.array(poses, np.float64).reshape(self.n_nodes, 4)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros((len(pr), 4, 4))
        self.ctx.check(self.ctx.lib.vgx_pose_graph_covariance(self.h, _ptr(x, f64p), int(bool(exclude_registration)), len(pr),
                                                              _ptr(pr, i32p), _ptr(out, f64p)))
        return out

    def covariance_sparse(self, poses, pairs, exclude_registration=False, max_solve_bytes=0):
        """vgx_pose_graph_covariance_sparse -> ([n_pairs][4][4], stats dict): covariance()'s blocks from the tile-sparse
        factor, the solved columns cut into slabs of at most max_solve_bytes (0: 1 GiB); the graph's solver must be
        LINEAR_SOLVER_TILE_SPARSE"""
        x = np.array(poses, np.float64).reshape(self.n_nodes, 4)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros((len(pr), 4, 4))
        stats = PoseGraphCovarianceStats()
        self.ctx.check(self.ctx.lib.vgx_pose_graph_covariance_sparse(self.h, _ptr(x, f64p), int(bool(exclude_registration)), len(pr),
                                                                     _ptr(pr, i32p), int(max_solve_bytes), _ptr(out, f64p),
                                                                     C.byref(stats)))
        return out, stats.as_dict()

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_pose_graph_destroy(self.h)
            self.h = None


class RegistrationAssembler:
    """vgx_reg_assembler: the whole constraint list's node structure on one context; builds the fused buffer from
    the complete [n][45] array in list order (the sharding-independent assembly, include/voxgraph_amd.h)."""

    def __init__(self, ctx, node_pair):
        self.ctx = ctx
        np_pair = np.ascontiguousarray(node_pair, dtype=np.int32).reshape(-1, 2)
        self.n = len(np_pair)
        h = vp()
        ctx.check(ctx.lib.vgx_reg_assembler_create(ctx.h, self.n, _ptr(np_pair, i32p), C.byref(h)))
        self.h = h

    def assemble(self, d_normal_all, n_nodes, d_fused):
        self.ctx.check(self.ctx.lib.vgx_reg_assembler_assemble(self.h, vp(d_normal_all) if d_normal_all else None,
                                                               n_nodes, vp(d_fused)))

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_reg_assembler_destroy(self.h)
            self.h = None


def lpt_shards(weights, n_shards):
    """vgx_lpt_shards: shard index per constraint (greedy longest-processing-time)."""
    w = np.ascontiguousarray(weights, np.int64)
    out = np.zeros(len(w), np.int32)
    rc = load().vgx_lpt_shards(len(w), _ptr(w, i64p), int(n_shards), _ptr(out, i32p))
    if rc != OK:
        raise VgxError(rc, "vgx_lpt_shards")
    return out


def contiguous_shards(weights, n_shards):
    """vgx_contiguous_shards: the list cut into n_shards consecutive runs of (nearly) equal weight"""
    w = np.ascontiguousarray(weights, np.int64)
    out = np.zeros(len(w), np.int32)
    rc = load().vgx_contiguous_shards(len(w), _ptr(w, i64p), int(n_shards), _ptr(out, i32p))
    if rc != OK:
        raise VgxError(rc, "vgx_contiguous_shards")
    return out


class RegistrationMulti:
    """vgx_reg_multi: the constraint list sharded over several contexts of this process."""

    def __init__(self, ctxs, cost_functions, node_pair):
        self.ctxs, self.n = list(ctxs), len(cost_functions)
        carr = (vp * len(self.ctxs))(*[c.h for c in self.ctxs])
        rarr = (vp * max(self.n, 1))(*[cf.h for cf in cost_functions])
        np_pair = np.ascontiguousarray(node_pair, dtype=np.int32).reshape(-1, 2)
        h = vp()
        self.ctxs[0].check(self.ctxs[0].lib.vgx_reg_multi_create(len(self.ctxs), carr, self.n, rarr,
                                                                 _ptr(np_pair, i32p), C.byref(h)))
        self.h = h
        self._keep = list(cost_functions)

    def shard_of(self):
        out = np.zeros(max(self.n, 1), np.int32)
        self.ctxs[0].check(self.ctxs[0].lib.vgx_reg_multi_shard_of(self.h, _ptr(out, i32p)))
        return out[:self.n]

    def evaluate_fused(self, poses):
        poses = _f64(poses).reshape(-1, 4)
        out = np.zeros(fused_size(poses.shape[0], self.n))
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctxs[0].check(self.ctxs[0].lib.vgx_reg_multi_evaluate_fused(
            self.h, _ptr(poses, f64p), poses.shape[0], _ptr(out, f64p), _ptr(status, i32p)))
        return out, status[:self.n]

    def set_reduction(self, rccl):
        """False: the blocks gathered over peer mappings (default); True: one ncclAllReduce per evaluation"""
        self.ctxs[0].check(self.ctxs[0].lib.vgx_reg_multi_set_reduction(self.h, 1 if rccl else 0))

    def evaluate_normal(self, poses):
        poses = _f64(poses).reshape(-1, 4)
        out = np.zeros((self.n, NORMAL_SIZE))
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctxs[0].check(self.ctxs[0].lib.vgx_reg_multi_evaluate_normal(
            self.h, _ptr(poses, f64p), poses.shape[0], _ptr(out, f64p), _ptr(status, i32p)))
        return out, status[:self.n]

    def evaluate_cost(self, poses):
        poses = _f64(poses).reshape(-1, 4)
        out = np.zeros(self.n)
        status = np.zeros(max(self.n, 1), np.int32)
        self.ctxs[0].check(self.ctxs[0].lib.vgx_reg_multi_evaluate_cost(
            self.h, _ptr(poses, f64p), poses.shape[0], _ptr(out, f64p), _ptr(status, i32p)))
        return out, status[:self.n]

    def destroy(self):
        if self.h:
            self.ctxs[0].lib.vgx_reg_multi_destroy(self.h)
            self.h = None


def atomic_roundtrip_ns(ctx, table_bytes=8 << 20, waves=1, chain=2000):
    """bench tooling (vgx_bench_atomic_roundtrip): ns per step of a chain of dependent device-scope exchanges"""
    out = C.c_float()
    ctx.check(ctx.lib.vgx_bench_atomic_roundtrip(ctx.h, table_bytes, waves, chain, C.byref(out)))
    return out.value


def alloc_scattered(ctx, nbytes, chunk_bytes, seed):
    """bench tooling (vgx_bench_alloc_scattered): device pointer of a range whose physical chunks are mapped in shuffled order"""
    out = vp()
    ctx.check(ctx.lib.vgx_bench_alloc_scattered(ctx.h, int(nbytes), int(chunk_bytes), int(seed), C.byref(out)))
    return int(out.value)


def free_scattered(ctx, ptr):
    ctx.check(ctx.lib.vgx_bench_free_scattered(ctx.h, vp(int(ptr))))


def stream_ceiling_ms(ctx, d_src, read_bytes, d_dst, write_bytes, launches=5):
    """bench tooling (vgx_bench_stream_ceiling): ms per launch that streams read_bytes in and write_bytes out"""
    out = C.c_float()
    ctx.check(ctx.lib.vgx_bench_stream_ceiling(ctx.h, d_src, int(read_bytes) & ~15, d_dst, int(write_bytes) & ~15,
                                               launches, C.byref(out)))
    return out.value


def synth_city_scan(ctx, sensor_pose, n_az, n_el, el_span, max_range, seed, d_points):
    """Benchmark tooling: sphere-traced LiDAR scan of the analytic city (sensor frame)."""
    ctx.check(ctx.lib.vgx_synth_city_scan(ctx.h, _ptr(_f64(sensor_pose), f64p), n_az, n_el,
                                          float(el_span), float(max_range), seed, vp(d_points)))


def find_overlapping_pairs(ctx, submaps, poses, max_pairs=None):
    """PoseGraphInterface::updateOverlappingSubmapList -> [(i, j)] with i < j."""
    n = len(submaps)
    arr = (vp * max(n, 1))(*[s.h for s in submaps])
    poses = _f64(poses).reshape(-1, 4)
    max_pairs = n * (n - 1) // 2 if max_pairs is None else max_pairs
    pairs = np.zeros((max(max_pairs, 1), 2), np.int32)
    k = C.c_int32()
    ctx.check(ctx.lib.vgx_find_overlapping_pairs(ctx.h, n, arr, _ptr(poses, f64p), _ptr(pairs, i32p),
                                                 max_pairs, C.byref(k)))
    return [tuple(int(x) for x in p) for p in pairs[:k.value]]


def compress_normal(normal45):
    """45-number normal block -> (r_c[9], J_c[9,8]) with identical normal equations."""
    nb = _f64(normal45)
    r, J = np.zeros(9), np.zeros((9, 8))
    rc = load().vgx_reg_compress_normal(_ptr(nb, f64p), _ptr(r, f64p), _ptr(J, f64p))
    if rc != OK:
        raise VgxError(rc, "vgx_reg_compress_normal")
    return r, J


def fused_size(n_nodes, n_global):
    return load().vgx_reg_fused_size(n_nodes, n_global)


# ----------------------------------------------------------------------------
# TSDF path
# ----------------------------------------------------------------------------
def esdf_config(**kw):
    cfg = EsdfConfig()
    load().vgx_esdf_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def tsdf_config(**kw):
    cfg = TsdfConfig()
    load().vgx_tsdf_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def voxgraph_tsdf_config(**kw):
    """voxgraph/config/voxgraph_mapper.yaml:21-28 over voxblox's defaults."""
    base = dict(default_truncation_distance=0.60, max_ray_length_m=16.0, use_const_weight=1,
                use_weight_dropoff=1, use_sparsity_compensation_factor=1,
                sparsity_compensation_factor=20.0)
    base.update(kw)
    return tsdf_config(**base)


class TsdfLayer:
    """voxblox::Layer<TsdfVoxel> of the active submap, resident on the GPU."""

    def __init__(self, ctx, voxel_size, vps, lut_min=None, lut_dim=None, max_blocks=0):
        """lut_min / lut_dim / max_blocks are only an initial reservation: the layer grows."""
        self.ctx, self.vps, self.voxel_size = ctx, vps, float(voxel_size)
        mn = None if lut_min is None else np.ascontiguousarray(lut_min, np.int32)
        dm = None if lut_dim is None else np.ascontiguousarray(lut_dim, np.int32)
        h = vp()
        ctx.check(ctx.lib.vgx_tsdf_layer_create(ctx.h, float(voxel_size), vps, _ptr(mn, i32p),
                                                _ptr(dm, i32p), max_blocks, C.byref(h)))
        self.h = h

    def growths(self):
        return int(self.ctx.lib.vgx_tsdf_layer_growths(self.h))

    def clear_dropped(self):
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_clear_dropped(self.h))

    def reserve(self, origin, reach_m):
        o = _f32(origin)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_reserve(self.h, _ptr(o, f32p), float(reach_m)))

    def upload(self, block_index, distance, weight, rgba=None):
        bi = np.ascontiguousarray(block_index, np.int32).reshape(-1, 3)
        d, w = _f32(distance), _f32(weight)
        c = None if rgba is None else np.ascontiguousarray(rgba, np.uint8)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_upload(self.h, bi.shape[0], _ptr(bi, i32p), _ptr(d, f32p),
                                                          _ptr(w, f32p), _ptr(c, u8p)))

    def stats(self):
        n, d = C.c_int32(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_stats(self.h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def merge_submaps(self, submaps, T_L_S):
        """voxblox::mergeLayerAintoLayerB(submap TSDF layer, T_L_S[i], this layer) for each submap in array order
        (T_L_S [n][7] qw,qx,qy,qz,tx,ty,tz); returns the layer's block count afterwards."""
        n = len(submaps)
        arr = (vp * max(n, 1))(*[s.h for s in submaps])
        T = np.ascontiguousarray(T_L_S, np.float32).reshape(n, 7)
        nb = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_merge_submaps(self.h, n, arr, _ptr(T, f32p), C.byref(nb)))
        return nb.value

    def transform_submap(self, submap, T_L_S):
        """voxblox::transformLayer(submap TSDF layer, T_L_S, this layer) into this EMPTY layer
        (vgx_tsdf_layer_transform_submap: interpolated voxels copied, not merged); returns the layer's block count."""
        T = np.ascontiguousarray(T_L_S, np.float32).reshape(7)
        nb = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_transform_submap(self.h, submap.h, _ptr(T, f32p), C.byref(nb)))
        return nb.value

    def generate_mesh(self, mesh=None, min_weight=1e-4):
        """MeshIntegrator::generateMesh(false, false) over this layer (vgx_tsdf_layer_generate_mesh).  Returns the Mesh
        (a new one when mesh is None)."""
        mesh = mesh if mesh is not None else Mesh(self.ctx)
        cfg = MeshConfig(float(min_weight))
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_generate_mesh(self.h, C.byref(cfg), mesh.h))
        return mesh

    def generate_mesh_colored(self, mesh=None, min_weight=1e-4):
        """generate_mesh plus one TSDF colour per soup vertex, MeshIntegratorConfig::use_color
        (vgx_tsdf_layer_generate_mesh_colored).  Returns the Mesh."""
        mesh = mesh if mesh is not None else Mesh(self.ctx)
        cfg = MeshConfig(float(min_weight))
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_generate_mesh_colored(self.h, C.byref(cfg), mesh.h))
        return mesh

    def cloud(self, config=None, cloud=None):
        """The point-cloud view of this layer, colours included (vgx_tsdf_layer_cloud; config: cloud_config(...)).
        Returns the Cloud (a new one when cloud is None)."""
        cloud = cloud if cloud is not None else Cloud(self.ctx)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_cloud(self.h, None if config is None else C.byref(config), cloud.h))
        return cloud

    def planar_map(self, config, planar_map=None):
        """The planar map of this layer's height band (vgx_tsdf_layer_planar_map; config: planar_map_config(z_min=...,
        z_max=..., ...)).  Returns the PlanarMap (a new one when planar_map is None)."""
        planar_map = planar_map if planar_map is not None else PlanarMap(self.ctx)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_planar_map(self.h, None if config is None else C.byref(config), planar_map.h))
        return planar_map

    def elevation_map(self, config, elevation_map=None):
        """The elevation map of this layer's height band (vgx_tsdf_layer_elevation_map; config: elevation_map_config(
        z_min=..., z_max=..., ...)).  Returns the ElevationMap (a new one when elevation_map is None)."""
        elevation_map = elevation_map if elevation_map is not None else ElevationMap(self.ctx)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_elevation_map(self.h, None if config is None else C.byref(config), elevation_map.h))
        return elevation_map

    def render_view(self, view, T_L_C, dirs, n=None):
        """The view of this layer from sensor pose T_L_C along dirs [n][3] (vgx_tsdf_layer_render_view / _device: a numpy
        array, a torch device tensor, or a device address with n), behind every scan queued.  Returns the View."""
        lib = self.ctx.lib
        return _render_view(self.ctx, lib.vgx_tsdf_layer_render_view, lib.vgx_tsdf_layer_render_view_device, self, view, T_L_C, dirs, n)

    def serialize(self, msg=None):
        """voxblox::serializeLayerAsMsg of this layer, colours included (vgx_tsdf_layer_serialize).  Returns the MapMsg
        (a new one when msg is None)."""
        msg = msg if msg is not None else MapMsg(self.ctx)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_serialize(self.h, msg.h))
        return msg

    def deserialize(self, action, block_index, words, voxel_size=None, vps=None, layer_type=EVAL_LAYER_TSDF):
        """voxblox::deserializeMsgToLayer from host arrays (vgx_tsdf_layer_deserialize): block_index [n][3], words
        [n][vps^3 * 3] u32; voxel_size / vps: the message's (default: this layer's)."""
        bi = np.ascontiguousarray(block_index, np.int32).reshape(-1, 3)
        w = np.ascontiguousarray(words, np.uint32)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_deserialize(
            self.h, int(action), int(layer_type), self.voxel_size if voxel_size is None else float(voxel_size),
            self.vps if vps is None else int(vps), bi.shape[0], _ptr(bi, i32p), _ptr(w, u32p), w.size))

    def deserialize_msg(self, action, msg):
        """the same from a MapMsg that holds a TSDF layer message: the words never leave the device"""
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_deserialize_msg(self.h, int(action), msg.h))

    def download(self):
        n, _ = self.stats()
        nv = self.vps ** 3
        bi = np.zeros((n, 3), np.int32)
        d = np.zeros((n, nv), np.float32)
        w = np.zeros((n, nv), np.float32)
        rgba = np.zeros((n, nv, 4), np.uint8)
        self.ctx.check(self.ctx.lib.vgx_tsdf_layer_download(self.h, _ptr(bi, i32p), _ptr(d, f32p),
                                                            _ptr(w, f32p), _ptr(rgba, u8p)))
        return bi, d, w, rgba

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_tsdf_layer_destroy(self.h)
            self.h = None


def projected_map(ctx, submaps, poses, layer):
    """cblox::SubmapCollection::getProjectedMap() into `layer` (emptied first): the submaps merged in ascending
    vgx_submap_id order (the collection's std::map order) at poses[i] = submaps[i].getPose() ([n][7] qw,qx,qy,qz,
    tx,ty,tz).  Returns the layer."""
    ids = [int(ctx.lib.vgx_submap_id(s.h)) for s in submaps]
    order = sorted(range(len(submaps)), key=lambda i: ids[i])
    poses = np.ascontiguousarray(poses, np.float32).reshape(len(submaps), 7)
    layer.upload(np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    layer.merge_submaps([submaps[i] for i in order], poses[order])
    return layer


def combined_mesh(ctx, submaps, poses, layer, mesh=None, min_weight=1e-4, use_color=False):
    """cblox SubmapMesher::generateCombinedMesh: projected_map(ctx, submaps, poses, layer), then the layer's mesh
    (use_color: with one TSDF colour per vertex -- the submaps must carry colours for it to be more than zeros).
    Returns the Mesh."""
    projected_map(ctx, submaps, poses, layer)
    return layer.generate_mesh_colored(mesh, min_weight) if use_color else layer.generate_mesh(mesh, min_weight)


DEFAULT_COLOR_CYCLE_LENGTH = 20  # cblox::kDefaultColorCycleLength [recalled]


def rainbow_color_map(h):
    """voxblox rainbowColorMap(h) [recalled]: an HSV blend at s = v = 1 in double, each channel truncated to uint8,
    a = 255.  Returns [r, g, b, a] uint8."""
    h = float(h)
    h -= math.floor(h)
    h *= 6.0
    i = int(math.floor(h))
    f = h - i
    if not (i & 1):
        f = 1.0 - f
    v, m, n = 1.0, 0.0, 1.0 - f
    rgb = {0: (v, n, m), 6: (v, n, m), 1: (n, v, m), 2: (m, v, n), 3: (m, n, v), 4: (n, m, v), 5: (v, m, n)}.get(i)
    if rgb is None:
        return np.array([255, 127, 127, 255], np.uint8)
    return np.array([int(255 * c) for c in rgb] + [255], np.uint8)


def submap_color(submap_id):
    """voxgraph's colour of a submap's mesh: rainbowColorMap(id / kDefaultColorCycleLength)
    (VoxgraphMapper::publishActiveSubmapMeshCallback)"""
    return rainbow_color_map(float(submap_id) / float(DEFAULT_COLOR_CYCLE_LENGTH))


def separated_mesh(ctx, submaps, poses, colors=None, mesh=None, min_weight=1e-4):
    """cblox SubmapMesher::generateSeparatedMesh: every submap meshed in its own frame, coloured, moved to its pose and
    appended into one mesh keyed by block index; the submaps in ascending vgx_submap_id order (the collection's std::map
    order) at poses[i] ([n][7] qw,qx,qy,qz, tx,ty,tz), coloured colors[i] ([n][4] uint8; default submap_color(id)).
    Returns the Mesh (a new one when mesh is None), which has colours."""
    ids = [int(ctx.lib.vgx_submap_id(s.h)) for s in submaps]
    order = sorted(range(len(submaps)), key=lambda i: ids[i])
    poses = np.ascontiguousarray(poses, np.float32).reshape(len(submaps), 7)
    if colors is None:
        colors = np.array([submap_color(i) for i in ids], np.uint8).reshape(len(submaps), 4)
    colors = np.ascontiguousarray(colors, np.uint8).reshape(len(submaps), 4)
    mesh = mesh if mesh is not None else Mesh(ctx)
    return mesh.generate_separated([submaps[i] for i in order], poses[order], colors[order], min_weight)


def evaluate_layers_rmse(gt, test, layer=EVAL_LAYER_ESDF, mode=EVAL_IGNORE_BEHIND_TEST, error_layer=False):
    """voxblox::utils::evaluateLayersRmse(gt layer, test layer, mode, &details[, &error_layer]) over two finished submaps
    (vgx_evaluate_layers_rmse).  Returns the details as a dict; with error_layer=True, (details, (block_index [m][3],
    distance [m][vps^3], set [m][vps^3])) -- one error block per test block with a gt counterpart, in test-slot order."""
    ctx = gt.ctx
    det = EvaluationDetails()
    if not error_layer:
        ctx.check(ctx.lib.vgx_evaluate_layers_rmse(gt.h, test.h, int(layer), int(mode), C.byref(det), None, None, None,
                                                   None))
        return det.as_dict()
    n, nv = test.num_blocks(), test.vps ** 3
    bi = np.zeros((n, 3), np.int32)
    d = np.zeros((n, nv), np.float32)
    st = np.zeros((n, nv), np.uint8)
    m = C.c_int32()
    ctx.check(ctx.lib.vgx_evaluate_layers_rmse(gt.h, test.h, int(layer), int(mode), C.byref(det), _ptr(bi, i32p),
                                               _ptr(d, f32p), _ptr(st, u8p), C.byref(m)))
    m = m.value
    return det.as_dict(), (bi[:m], d[:m], st[:m])


def cloud_config(**kw):
    """vgx_cloud_config_default() with fields overridden: kind, surface_distance, min_weight, slice_axis, slice_value."""
    cfg = CloudConfig()
    load().vgx_cloud_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


class Cloud:
    """A layer's point cloud on the GPU (vgx_cloud): voxel centres, intensity = distance, optionally colours; reused from
    call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_cloud_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """(points, has_colors)"""
        n, has = C.c_int64(), C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_cloud_stats(self.h, C.byref(n), C.byref(has)))
        return n.value, bool(has.value)

    def download(self):
        """(xyz [n][3] f32, intensity [n] f32, rgba [n][4] uint8 or None)"""
        n, has = self.stats()
        xyz = np.zeros((n, 3), np.float32)
        inten = np.zeros(n, np.float32)
        rgba = np.zeros((n, 4), np.uint8) if has else None
        self.ctx.check(self.ctx.lib.vgx_cloud_download(self.h, _ptr(xyz, f32p), _ptr(inten, f32p), _ptr(rgba, u8p)))
        return xyz, inten, rgba

    def device_pointers(self):
        """(xyz, intensity, rgba) device addresses as ints (None where the cloud has none)"""
        p = [vp(), vp(), vp()]
        self.ctx.check(self.ctx.lib.vgx_cloud_device_pointers(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_cloud_destroy(self.h)
            self.h = None


def planar_map_config(**kw):
    """vgx_planar_map_config_default() with fields overridden: z_min, z_max (both required by the producing calls),
    occupied_distance, min_weight, min_free_voxels, unknown_is_obstacle, max_distance_m, use_box, cell_min, cell_dim."""
    cfg = PlanarMapConfig()
    load().vgx_planar_map_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        if k in ("cell_min", "cell_dim"):
            v = (C.c_int32 * 2)(int(v[0]), int(v[1]))
        setattr(cfg, k, v)
    return cfg


class PlanarMap:
    """A layer's height band as a 2D grid on the GPU (vgx_planar_map): state, occupancy, clearance, height and the
    clipped planar distance per cell, row-major with x fastest; reused from call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_planar_map_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """((x0, y0), (W, H), voxel_size, (unknown, free, occupied) cell counts)"""
        mn, dim, vs, counts = (C.c_int32 * 2)(), (C.c_int32 * 2)(), C.c_float(), (C.c_int64 * 3)()
        self.ctx.check(self.ctx.lib.vgx_planar_map_stats(self.h, mn, dim, C.byref(vs), counts))
        return (mn[0], mn[1]), (dim[0], dim[1]), vs.value, tuple(counts)

    def download(self):
        """(state [H][W] u8, occupancy [H][W] i8, clearance, height, distance [H][W] f32)"""
        _, (w, h), _, _ = self.stats()
        state = np.zeros((h, w), np.uint8)
        occupancy = np.zeros((h, w), np.int8)
        clearance, height, distance = (np.zeros((h, w), np.float32) for _ in range(3))
        self.ctx.check(self.ctx.lib.vgx_planar_map_download(self.h, _ptr(state, u8p), _ptr(occupancy, C.POINTER(C.c_int8)),
                                                            _ptr(clearance, f32p), _ptr(height, f32p), _ptr(distance, f32p)))
        return state, occupancy, clearance, height, distance

    def set_timing(self, enable=True):
        """record events between the passes of the producing calls from now on (off by default)"""
        self.ctx.check(self.ctx.lib.vgx_planar_map_set_timing(self.h, 1 if enable else 0))

    def pass_ms(self):
        """device milliseconds of the last producing call, with set_timing(True): (box, gather, row pass, column pass)"""
        ms = (C.c_float * 4)()
        self.ctx.check(self.ctx.lib.vgx_planar_map_pass_ms(self.h, ms))
        return tuple(ms)

    def device_pointers(self):
        """(state, occupancy, clearance, height, distance) device addresses as ints (None while the map holds 0 cells)"""
        p = [vp() for _ in range(5)]
        self.ctx.check(self.ctx.lib.vgx_planar_map_device_pointers(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_planar_map_destroy(self.h)
            self.h = None


def elevation_map_config(**kw):
    """vgx_elevation_map_config_default() with fields overridden: z_min, z_max (both required by the producing calls),
    min_weight, min_free_voxels, pick, step_radius_cells, min_support, max_slope, max_step_m, min_headroom_voxels,
    hole_is_obstacle, unknown_is_obstacle, max_distance_m, use_box, cell_min, cell_dim."""
    cfg = ElevationMapConfig()
    load().vgx_elevation_map_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        if k in ("cell_min", "cell_dim"):
            v = (C.c_int32 * 2)(int(v[0]), int(v[1]))
        setattr(cfg, k, v)
    return cfg


class ElevationMap:
    """A layer's height band as a 2.5D surface on the GPU (vgx_elevation_map): state, height, headroom, crossings,
    support, step, gradient, slope, class and the clipped planar distance per cell, row-major with x fastest; reused from
    call to call."""
    FIELDS = (("state", np.uint8), ("height", np.float32), ("headroom", np.int32), ("crossings", np.uint8), ("support", np.uint16),
              ("step", np.float32), ("grad", np.float32), ("slope", np.float32), ("slope_valid", np.uint8), ("cls", np.uint8),
              ("distance", np.float32))

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_elevation_map_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """((x0, y0), (W, H), voxel_size, (unknown, surface, hole, blocked) cell counts, (unknown, traversable,
        not traversable) cell counts)"""
        mn, dim, vs, states, classes = (C.c_int32 * 2)(), (C.c_int32 * 2)(), C.c_float(), (C.c_int64 * 4)(), (C.c_int64 * 3)()
        self.ctx.check(self.ctx.lib.vgx_elevation_map_stats(self.h, mn, dim, C.byref(vs), states, classes))
        return (mn[0], mn[1]), (dim[0], dim[1]), vs.value, tuple(states), tuple(classes)

    def download(self):
        """the eleven arrays in FIELDS' order, [H][W] each (grad: [H][W][2])"""
        _, (w, h), _, _, _ = self.stats()
        out = [np.zeros((h, w, 2) if name == "grad" else (h, w), dt) for name, dt in self.FIELDS]
        self.ctx.check(self.ctx.lib.vgx_elevation_map_download(self.h, *[a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))
                                                                         for a in out]))
        return tuple(out)

    def set_timing(self, enable=True):
        """record events between the passes of the producing calls from now on (off by default)"""
        self.ctx.check(self.ctx.lib.vgx_elevation_map_set_timing(self.h, 1 if enable else 0))

    def pass_ms(self):
        """device milliseconds of the last producing call, with set_timing(True): (box, gather, step row pass, step
        column pass with slope and class, distance row pass, distance column pass)"""
        ms = (C.c_float * 6)()
        self.ctx.check(self.ctx.lib.vgx_elevation_map_pass_ms(self.h, ms))
        return tuple(ms)

    def device_pointers(self):
        """the eleven arrays' device addresses as ints, in FIELDS' order (None while the map holds 0 cells)"""
        p = [vp() for _ in range(11)]
        self.ctx.check(self.ctx.lib.vgx_elevation_map_device_pointers(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_elevation_map_destroy(self.h)
            self.h = None


class MapMsg:
    """A map message on the GPU (vgx_map_msg): a serialised TSDF / ESDF layer (block indices and block words) or a
    submap's surface cloud (PointXYZI bytes); reused from call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_map_msg_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """(kind, blocks or points, words per voxel, payload bytes)"""
        kind, n, wpv, nb = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_map_msg_stats(self.h, C.byref(kind), C.byref(n), C.byref(wpv), C.byref(nb)))
        return kind.value, n.value, wpv.value, nb.value

    def layer_geometry(self):
        """(voxel_size, voxels_per_side) of the layer a layer message was made from"""
        vs, vps = C.c_float(), C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_map_msg_layer_geometry(self.h, C.byref(vs), C.byref(vps)))
        return vs.value, vps.value

    def download(self):
        """a layer message: (block_index [n][3] i32, words [n][vps^3 * W] u32); a surface cloud: bytes [n][32] uint8"""
        kind, n, wpv, _ = self.stats()
        if kind == MSG_SURFACE_CLOUD:
            data = np.zeros((n, 32), np.uint8)
            self.ctx.check(self.ctx.lib.vgx_map_msg_download(self.h, None, vp(data.ctypes.data)))
            return data
        bi = np.zeros((n, 3), np.int32)
        words = np.zeros((n, self.layer_geometry()[1] ** 3 * wpv if kind != MSG_NONE else 0), np.uint32)
        self.ctx.check(self.ctx.lib.vgx_map_msg_download(self.h, _ptr(bi, i32p), vp(words.ctypes.data)))
        return bi, words

    def device_pointers(self):
        """(block_index, payload) device addresses as ints (None where the message has none)"""
        p = [vp(), vp()]
        self.ctx.check(self.ctx.lib.vgx_map_msg_device_pointers(self.h, C.byref(p[0]), C.byref(p[1])))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_map_msg_destroy(self.h)
            self.h = None


def surface_msg_layout(n):
    """the vgx_scan_layout of a surface cloud of n points: pcl::PointXYZI as pcl::toROSMsg lays it out"""
    return scan_layout(width=int(n), height=1, point_step=32, offset_x=0, offset_y=4, offset_z=8,
                       color_kind=SCAN_COLOR_INTENSITY, color_offset=16)


def scan_layout(**kw):
    """A vgx_scan_layout from keywords (fields not given are 0; row_step defaults to width * point_step)."""
    lay = ScanLayout()
    for k, v in kw.items():
        if not hasattr(lay, k):
            raise AttributeError(k)
        setattr(lay, k, v)
    if "row_step" not in kw:
        lay.row_step = lay.width * lay.point_step
    return lay


def scan_config(intensity_min=None, intensity_max=None, constant_rgba=None):
    """vgx_scan_config_default() with fields overridden."""
    cfg = ScanConfig()
    load().vgx_scan_config_default(C.byref(cfg))
    if intensity_min is not None:
        cfg.intensity_min = intensity_min
    if intensity_max is not None:
        cfg.intensity_max = intensity_max
    if constant_rgba is not None:
        cfg.constant_rgba[:] = [int(v) for v in constant_rgba]
    return cfg


def scan_layout_check(layout, n_bytes):
    """vgx_scan_layout_check (host only): OK, or the code a decode of n_bytes bytes in this layout is refused with"""
    return load().vgx_scan_layout_check(None if layout is None else C.byref(layout), int(n_bytes))


def scan_time_field(kind, offset, scale=1.0, offset_s=0.0):
    """A vgx_scan_time_field: t = offset_s + raw * scale of the SCAN_TIME_* field at byte `offset` of a point."""
    return ScanTimeField(int(kind), int(offset), float(scale), float(offset_s))


def scan_track_view(knot_time, knot_T):
    """A vgx_scan_track over host arrays (converted to contiguous f64 [K] / f32 [K][7]).  Returns (view, arrays): keep
    the arrays alive as long as the view is used."""
    kt = np.ascontiguousarray(knot_time, np.float64).reshape(-1)
    kT = np.ascontiguousarray(knot_T, np.float32).reshape(-1, 7)
    if len(kt) != len(kT):
        raise ValueError("knot_time and knot_T differ in length")
    return ScanTrackView(len(kt), kt.ctypes.data_as(C.POINTER(C.c_double)), kT.ctypes.data_as(C.POINTER(C.c_float))), (kt, kT)


def scan_undistort_check(layout, time_field, knot_time, knot_T, n_bytes):
    """vgx_scan_undistort_check (host only); knot_time None: a NULL track"""
    view, keep = (None, None) if knot_time is None else scan_track_view(knot_time, knot_T)
    return load().vgx_scan_undistort_check(None if layout is None else C.byref(layout), None if time_field is None else C.byref(time_field),
                                           None if view is None else C.byref(view), int(n_bytes))


def depth_image_layout(**kw):
    """A vgx_depth_image_layout from keywords (fields not given are 0; row_step and color_row_step default to width *
    bytes per pixel of the encoding / colour kind)."""
    lay = DepthImageLayout()
    for k, v in kw.items():
        if not hasattr(lay, k):
            raise AttributeError(k)
        setattr(lay, k, v)
    if "row_step" not in kw:
        lay.row_step = lay.width * DEPTH_BYTES_PER_PIXEL.get(lay.encoding, 0)
    if "color_row_step" not in kw:
        lay.color_row_step = lay.width * IMAGE_COLOR_BYTES_PER_PIXEL.get(lay.color_kind, 0)
    return lay


def depth_camera(**kw):
    """vgx_depth_camera_default() with fields overridden by keyword (fx and fy have no default)."""
    cam = DepthCamera()
    load().vgx_depth_camera_default(C.byref(cam))
    for k, v in kw.items():
        if not hasattr(cam, k):
            raise AttributeError(k)
        setattr(cam, k, v)
    return cam


def depth_row_time(scale, offset_s=0.0):
    """A vgx_depth_row_time: t = offset_s + v * scale of image row v."""
    return DepthRowTime(float(scale), float(offset_s))


def depth_image_check(layout, camera, depth_n_bytes, color_n_bytes=0, row_time=None, knot_time=None, knot_T=None):
    """vgx_depth_image_check (host only): OK, or the code a decode of these byte counts is refused with; with a row time
    or knots given, vgx_depth_image_undistort_check (either may then be None: a NULL argument)"""
    lay, cam = (None if o is None else C.byref(o) for o in (layout, camera))
    if row_time is None and knot_time is None:
        return load().vgx_depth_image_check(lay, cam, int(depth_n_bytes), int(color_n_bytes))
    view, keep = (None, None) if knot_time is None else scan_track_view(knot_time, knot_T)
    return load().vgx_depth_image_undistort_check(lay, cam, None if row_time is None else C.byref(row_time),
                                                  None if view is None else C.byref(view), int(depth_n_bytes), int(color_n_bytes))


def projective_box(layout, camera, config, T_G_C, voxel_size, vps):
    """vgx_tsdf_projective_box (host only): (code, lo [3], hi [3]) -- the candidate block box of a projectively integrated
    frame; layout / camera / config may be None (a NULL argument)"""
    T = _f32(T_G_C)
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    lay, cam, cfg = (None if o is None else C.byref(o) for o in (layout, camera, config))
    rc = load().vgx_tsdf_projective_box(lay, cam, cfg, _ptr(T, f32p), float(voxel_size), int(vps), _ptr(lo, i32p), _ptr(hi, i32p))
    return rc, lo, hi


def lidar_model(**kw):
    """A vgx_lidar_model from keywords (fields not given are 0)."""
    m = LidarModel()
    for k, v in kw.items():
        if not hasattr(m, k):
            raise AttributeError(k)
        setattr(m, k, v)
    return m


def lidar_beam_model(width, row_elevation_rad, row_azimuth_offset_rad=None, azimuth_first_rad=0.0, azimuth_clockwise=0,
                     row_half_extent_max_rad=float("inf"), height=None):
    """A vgx_lidar_beam_model; height defaults to the table's length.  The f32 copies of the two arrays hang on the
    structure, so they live as long as it does."""
    m = LidarBeamModel()
    el = np.ascontiguousarray(row_elevation_rad, np.float32).reshape(-1)
    off = None if row_azimuth_offset_rad is None else np.ascontiguousarray(row_azimuth_offset_rad, np.float32).reshape(-1)
    m.width, m.height = int(width), len(el) if height is None else int(height)
    m.azimuth_first_rad, m.azimuth_clockwise, m.row_half_extent_max_rad = azimuth_first_rad, int(azimuth_clockwise), row_half_extent_max_rad
    m.row_elevation_rad = _ptr(el, f32p)
    m.row_azimuth_offset_rad = None if off is None else _ptr(off, f32p)
    m._keep = (el, off)
    return m


def range_image_check_beams(model):
    """vgx_range_image_check_beams (host only): OK, or the code the model is refused with; None: a NULL argument"""
    return load().vgx_range_image_check_beams(None if model is None else C.byref(model))


def range_image_pixel_beams(model, x, y, z):
    """vgx_range_image_pixel_beams (host only): (code, u, v); u = v = -1 outside the rows"""
    u, v = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = load().vgx_range_image_pixel_beams(None if model is None else C.byref(model), float(x), float(y), float(z), _ptr(u, i32p),
                                            _ptr(v, i32p))
    return rc, int(u[0]), int(v[0])


def range_image_box_beams(model, image_counts, config, T_G_S, voxel_size, vps):
    """vgx_tsdf_range_image_box_beams (host only): as range_image_box, for a LidarBeamModel"""
    T = _f32(T_G_S)
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    if isinstance(image_counts, dict):
        image_counts = range_image_counts(**image_counts)
    m, ic, cfg = (None if o is None else C.byref(o) for o in (model, image_counts, config))
    rc = load().vgx_tsdf_range_image_box_beams(m, ic, cfg, _ptr(T, f32p), float(voxel_size), int(vps), _ptr(lo, i32p), _ptr(hi, i32p))
    return rc, lo, hi


def view_rays_lidar_beams(model):
    """vgx_view_rays_lidar_beams (host only): unit directions [height * width][3] f32 through the pixel centres, row-major"""
    dirs = np.zeros((model.height * model.width, 3), np.float32)
    rc = load().vgx_view_rays_lidar_beams(C.byref(model), _ptr(dirs, f32p))
    if rc != OK:
        raise VgxError(rc, "vgx_view_rays_lidar_beams: the model is refused")
    return dirs


def range_image_check(model):
    """vgx_range_image_check (host only): OK, or the code the model is refused with; None: a NULL argument"""
    return load().vgx_range_image_check(None if model is None else C.byref(model))


def atan2_rule(y, x):
    """vgx_atan2_rule (host only) of f32 arrays, element by element"""
    fn = load().vgx_atan2_rule
    y, x = np.broadcast_arrays(np.asarray(y, np.float32), np.asarray(x, np.float32))
    return np.array([fn(float(a), float(b)) for a, b in zip(y.ravel(), x.ravel())], np.float32).reshape(y.shape)


def range_image_pixel(model, x, y, z):
    """vgx_range_image_pixel (host only): (code, u, v); v = -1 outside the rows"""
    u, v = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = load().vgx_range_image_pixel(None if model is None else C.byref(model), float(x), float(y), float(z), _ptr(u, i32p), _ptr(v, i32p))
    return rc, int(u[0]), int(v[0])


def _counts_dict(c):
    out = {}
    for k, t in type(c)._fields_:
        if k != "pad_":
            v = getattr(c, k)
            out[k] = np.array(v[:], np.float32) if hasattr(v, "__len__") else v
    return out


def range_image_counts(**kw):
    """A vgx_range_image_counts from keywords (as RangeImage.stats() returns them)"""
    c = RangeImageCounts()
    for k, v in kw.items():
        if hasattr(getattr(c, k), "__len__"):
            v = (C.c_float * 3)(*[float(x) for x in v])
        setattr(c, k, v)
    return c


def range_image_box(model, image_counts, config, T_G_S, voxel_size, vps):
    """vgx_tsdf_range_image_box (host only): (code, lo [3], hi [3]); image_counts a dict (RangeImage.stats()) or a
    RangeImageCounts; model / image_counts / config may be None (a NULL argument)"""
    T = _f32(T_G_S)
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    if isinstance(image_counts, dict):
        image_counts = range_image_counts(**image_counts)
    m, ic, cfg = (None if o is None else C.byref(o) for o in (model, image_counts, config))
    rc = load().vgx_tsdf_range_image_box(m, ic, cfg, _ptr(T, f32p), float(voxel_size), int(vps), _ptr(lo, i32p), _ptr(hi, i32p))
    return rc, lo, hi


class RangeImage:
    """A LiDAR scan gathered into a spherical range image on the GPU (vgx_range_image): per pixel the nearest return, its
    colour and its point index; reused from scan to scan.  FastTsdfIntegrator.integrate_range_image consumes it."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_range_image_create(ctx.h, C.byref(h)))
        self.h = h

    def build(self, model, scan, count=True):
        """from a decoded Scan; returns the counts as a dict, count=False: None and the build is queued"""
        out = RangeImageCounts()
        fn = self.ctx.lib.vgx_range_image_build_beams if isinstance(model, LidarBeamModel) else self.ctx.lib.vgx_range_image_build
        self.ctx.check(fn(self.h, C.byref(model), scan.h, C.byref(out) if count else None))
        return _counts_dict(out) if count else None

    def build_device(self, model, d_points, d_rgba, n, count=True):
        """from device arrays (f32 [n][3], u32 [n] or None) ready with respect to the TSDF stream"""
        out = RangeImageCounts()
        lib = self.ctx.lib
        fn = lib.vgx_range_image_build_beams_device if isinstance(model, LidarBeamModel) else lib.vgx_range_image_build_device
        self.ctx.check(fn(self.h, C.byref(model), vp(d_points) if d_points else None, vp(d_rgba) if d_rgba else None, int(n),
                          C.byref(out) if count else None))
        return _counts_dict(out) if count else None

    def stats(self):
        """the counts of the image held, as a dict (waits for a queued build)"""
        out = RangeImageCounts()
        self.ctx.check(self.ctx.lib.vgx_range_image_stats(self.h, C.byref(out), None))
        return _counts_dict(out)

    def model(self):
        """the uniform model the image was built for; of a table image a summary: the shared fields and the table's first
        and last elevation (beams() gives the table)"""
        m = LidarModel()
        self.ctx.check(self.ctx.lib.vgx_range_image_stats(self.h, None, C.byref(m)))
        return m

    def beams(self):
        """vgx_range_image_beams: None for a uniform image, else (row_elevation [h], row_azimuth_offset [h], limit)"""
        h = self.model().height
        is_table, limit = np.zeros(1, np.int32), np.zeros(1, np.float32)
        el, off = np.zeros(h, np.float32), np.zeros(h, np.float32)
        self.ctx.check(self.ctx.lib.vgx_range_image_beams(self.h, _ptr(is_table, i32p), _ptr(el, f32p), _ptr(off, f32p), _ptr(limit, f32p)))
        return (el, off, float(limit[0])) if is_table[0] else None

    def download(self):
        """(range [h][w] f32, rgba [h][w][4] u8, point_index [h][w] i32)"""
        m = self.model()
        rng = np.zeros((m.height, m.width), np.float32)
        rgba = np.zeros((m.height, m.width, 4), np.uint8)
        idx = np.zeros((m.height, m.width), np.int32)
        self.ctx.check(self.ctx.lib.vgx_range_image_download(self.h, _ptr(rng, f32p), _ptr(rgba, u8p), _ptr(idx, i32p)))
        return rng, rgba, idx

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_range_image_destroy(self.h)
            self.h = None


def _image_bytes(image):
    """(pointer or None, byte count) of an image's bytes: bytes, bytearray or a contiguous array; None: no image"""
    if image is None:
        return None, 0
    buf = np.frombuffer(image, np.uint8)
    return (vp(buf.ctypes.data) if buf.size else None), buf.size


class ScanTrack:
    """Samples (t, T_fixed_sensor) of a sensor's pose and the vgx_scan_track they make for one scan -- the same
    arithmetic as GpuScanTrack (voxgraph_amd/cpp/gpu_pointcloud_integrator.h), all of it f64, one rounding per operation:
      r      the reference's inverse rotation: n = sqrt(((w w + x x) + y y) + z z) of q_ref, r = (w / n, -x / n, -y / n, -z / n)
      q_rel  r (x) q_k, Hamilton product, every component summed left to right:
             w = rw kw - rx kx - ry ky - rz kz        x = rw kx + rx kw + ry kz - rz ky
             y = rw ky - rx kz + ry kw + rz kx        z = rw kz + rx ky - ry kx + rz kw
             then divided by m = sqrt(((w w + x x) + y y) + z z)
      t_rel  r applied to d = t_k - t_ref as the library applies a transform: uv = r.v x d, uv += uv, cc = r.v x uv,
             t_rel = (d + rw uv) + cc
      knot_time[k] = t_k - stamp; knot_T[k] = (q_rel, t_rel) cast to f32."""

    def __init__(self):
        self.times, self.poses = [], []

    def add(self, t, T_fixed_sensor):
        """T_fixed_sensor: qw,qx,qy,qz, tx,ty,tz of the sensor at time t in any fixed frame; times strictly ascending"""
        self.times.append(float(t))
        self.poses.append(np.asarray(T_fixed_sensor, np.float64).reshape(7).copy())

    def relative_to(self, T_fixed_sensor_ref, stamp=0.0):
        """-> (knot_time [K] f64, knot_T [K][7] f32): T_ref^-1 * T_k and t_k - stamp"""
        ref = np.asarray(T_fixed_sensor_ref, np.float64).reshape(7)
        P = np.array(self.poses, np.float64).reshape(-1, 7)
        w, x, y, z = ref[:4]
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        rw, rx, ry, rz = w / n, -x / n, -y / n, -z / n
        kw, kx, ky, kz = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
        qw = rw * kw - rx * kx - ry * ky - rz * kz
        qx = rw * kx + rx * kw + ry * kz - rz * ky
        qy = rw * ky - rx * kz + ry * kw + rz * kx
        qz = rw * kz + rx * ky - ry * kx + rz * kw
        m = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        dx, dy, dz = P[:, 4] - ref[4], P[:, 5] - ref[5], P[:, 6] - ref[6]
        ux, uy, uz = ry * dz - rz * dy, rz * dx - rx * dz, rx * dy - ry * dx
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        cx, cy, cz = ry * uz - rz * uy, rz * ux - rx * uz, rx * uy - ry * ux
        T = np.stack([qw / m, qx / m, qy / m, qz / m, (dx + rw * ux) + cx, (dy + rw * uy) + cy, (dz + rw * uz) + cz], 1)
        return np.array(self.times, np.float64) - np.float64(stamp), T.astype(np.float32)


class Scan:
    """A raw PointCloud2 -- or a depth image with its camera model -- decoded on the GPU (vgx_scan): the kept points and
    their colours in message / image order; reused from message to message.  FastTsdfIntegrator.integrate_scan /
    integrate_merged_scan consume it."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_scan_create(ctx.h, C.byref(h)))
        self.h = h

    def decode_msg(self, layout, data, config=None):
        """data: the message's bytes (bytes, bytearray or a contiguous array).  Returns (points, dropped)."""
        buf = np.frombuffer(data, np.uint8)
        self.ctx.check(self.ctx.lib.vgx_scan_decode_msg(self.h, C.byref(layout), None if config is None else C.byref(config),
                                                        vp(buf.ctypes.data) if buf.size else None, buf.size))
        return self.stats()

    def decode_msg_device(self, layout, d_data, n_bytes, config=None):
        """the same with the message at device address d_data (ready with respect to the TSDF stream)"""
        self.ctx.check(self.ctx.lib.vgx_scan_decode_msg_device(self.h, C.byref(layout), None if config is None else C.byref(config),
                                                               vp(d_data) if d_data else None, int(n_bytes)))
        return self.stats()

    def decode_undistorted(self, layout, data, time_field, knot_time, knot_T, config=None):
        """decode_msg with every point moved into the reference frame by the track (vgx_scan_decode_msg_undistorted):
        knot_time [K] f64 ascending, knot_T [K][7] f32 = T_ref_sensor at the knot times.  Returns (points, dropped)."""
        buf = np.frombuffer(data, np.uint8)
        view, keep = scan_track_view(knot_time, knot_T)
        self.ctx.check(self.ctx.lib.vgx_scan_decode_msg_undistorted(
            self.h, C.byref(layout), None if config is None else C.byref(config), C.byref(time_field), C.byref(view),
            vp(buf.ctypes.data) if buf.size else None, buf.size))
        return self.stats()

    def decode_undistorted_device(self, layout, d_data, n_bytes, time_field, knot_time, knot_T, config=None):
        """the same with the message at device address d_data (ready with respect to the TSDF stream)"""
        view, keep = scan_track_view(knot_time, knot_T)
        self.ctx.check(self.ctx.lib.vgx_scan_decode_msg_undistorted_device(
            self.h, C.byref(layout), None if config is None else C.byref(config), C.byref(time_field), C.byref(view),
            vp(d_data) if d_data else None, int(n_bytes)))
        return self.stats()

    def decode_depth_image(self, layout, camera, depth, color=None, config=None, row_time=None, knot_time=None, knot_T=None):
        """A depth image and its registered colour image (host bytes: bytes, bytearray or contiguous arrays; color None
        for IMAGE_COLOR_NONE) unprojected, filtered and coloured (vgx_scan_decode_depth_image); with row_time (a
        DepthRowTime) and knots, every point moved into the reference frame by the track
        (vgx_scan_decode_depth_image_undistorted).  Returns (points, dropped)."""
        (dp, dn), (cp, cn) = _image_bytes(depth), _image_bytes(color)
        cfg = None if config is None else C.byref(config)
        if row_time is None:
            self.ctx.check(self.ctx.lib.vgx_scan_decode_depth_image(self.h, C.byref(layout), C.byref(camera), cfg, dp, dn, cp, cn))
        else:
            view, keep = scan_track_view(knot_time, knot_T)
            self.ctx.check(self.ctx.lib.vgx_scan_decode_depth_image_undistorted(
                self.h, C.byref(layout), C.byref(camera), cfg, C.byref(row_time), C.byref(view), dp, dn, cp, cn))
        return self.stats()

    def decode_depth_image_device(self, layout, camera, d_depth, depth_n_bytes, d_color=None, color_n_bytes=0, config=None,
                                  row_time=None, knot_time=None, knot_T=None):
        """the same with the images at device addresses (ready with respect to the TSDF stream)"""
        dp, cp = (vp(a) if a else None for a in (d_depth, d_color))
        cfg = None if config is None else C.byref(config)
        if row_time is None:
            self.ctx.check(self.ctx.lib.vgx_scan_decode_depth_image_device(self.h, C.byref(layout), C.byref(camera), cfg, dp,
                                                                           int(depth_n_bytes), cp, int(color_n_bytes)))
        else:
            view, keep = scan_track_view(knot_time, knot_T)
            self.ctx.check(self.ctx.lib.vgx_scan_decode_depth_image_undistorted_device(
                self.h, C.byref(layout), C.byref(camera), cfg, C.byref(row_time), C.byref(view), dp, int(depth_n_bytes), cp,
                int(color_n_bytes)))
        return self.stats()

    def stats(self):
        """(points, dropped)"""
        n, d = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_scan_stats(self.h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def depth_stats(self):
        """(candidates, invalid, out_of_range, overflowed) of the last decode; zeros after a PointCloud2 decode"""
        v = [C.c_int64() for _ in range(4)]
        self.ctx.check(self.ctx.lib.vgx_scan_depth_stats(self.h, *(C.byref(x) for x in v)))
        return tuple(x.value for x in v)

    def undistort_stats(self):
        """(bad_time, overflowed, clamped) of the last decode; zeros after a plain one"""
        b, o, c = C.c_int64(), C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_scan_undistort_stats(self.h, C.byref(b), C.byref(o), C.byref(c)))
        return b.value, o.value, c.value

    def set_age(self, epoch, tickets):
        """test tooling: the decode's chain clock (vgx_scan_set_age)"""
        self.ctx.check(self.ctx.lib.vgx_scan_set_age(self.h, int(epoch), int(tickets)))

    def get_age(self):
        """test tooling: (epoch, tickets) of the decode's chain clock"""
        e, t = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_scan_get_age(self.h, C.byref(e), C.byref(t)))
        return e.value, t.value

    def download(self):
        """(points [n][3] f32, rgba [n][4] uint8)"""
        n, _ = self.stats()
        pts = np.zeros((n, 3), np.float32)
        rgba = np.zeros((n, 4), np.uint8)
        self.ctx.check(self.ctx.lib.vgx_scan_download(self.h, _ptr(pts, f32p), _ptr(rgba, u8p)))
        return pts, rgba

    def device_pointers(self):
        """(points, rgba) device addresses as ints (None for a scan of 0 points)"""
        p = [vp(), vp()]
        self.ctx.check(self.ctx.lib.vgx_scan_device_pointers(self.h, C.byref(p[0]), C.byref(p[1])))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_scan_destroy(self.h)
            self.h = None


def scan_registration_config(max_abs_distance_m, **kw):
    """vgx_scan_registration_config: the defaults, max_abs_distance_m (which has none) and fields overridden by keyword"""
    cfg = ScanRegistrationConfig()
    load().vgx_scan_registration_config_default(C.byref(cfg))
    cfg.max_abs_distance_m = max_abs_distance_m
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


class ScanRegistration:
    """Scan-to-map registration (vgx_scan_registration): a scan's sensor pose T_S_C refined against the active TSDF layer
    on the TSDF stream -- `T, usable = reg.refine(layer, T_prior)[:2]`, then integrate at T."""

    def __init__(self, ctx, config):
        self.ctx = ctx
        self._keep = None            # a borrowed source stays alive with the handle
        h = vp()
        ctx.check(ctx.lib.vgx_scan_registration_create(ctx.h, None if config is None else C.byref(config), C.byref(h)))
        self.h = h

    def set_points(self, points, n=None):
        """points: a numpy array [n][3] (copied), a torch device tensor [n][3] f32 (borrowed), a device address as an int
        with n (borrowed), or a capi.Scan (borrowed: its points at each evaluation)"""
        lib = self.ctx.lib
        if isinstance(points, Scan):
            self.ctx.check(lib.vgx_scan_registration_set_scan(self.h, points.h))
            self._keep = points
        elif isinstance(points, int):
            self.ctx.check(lib.vgx_scan_registration_set_points_device(self.h, vp(points) if points else None, int(n)))
            self._keep = None
        elif hasattr(points, "data_ptr"):
            if not points.is_cuda or str(points.dtype) != "torch.float32" or not points.is_contiguous():
                raise TypeError("a contiguous float32 device tensor [n][3]")
            m = points.numel() // 3
            self.ctx.check(lib.vgx_scan_registration_set_points_device(self.h, vp(points.data_ptr()) if m else None, m))
            self._keep = points
        else:
            p = _f32(points).reshape(-1, 3)
            self.ctx.check(lib.vgx_scan_registration_set_points(self.h, _ptr(p, f32p) if len(p) else None, len(p)))
            self._keep = None

    def evaluate(self, layer, T_S_C_prior, delta=(0.0, 0.0, 0.0, 0.0)):
        """-> (out [15]: sum r r, sum J_k r [4], sum J_k J_l [10]; n_valid; n_candidates)"""
        T, d, out = _f32(T_S_C_prior), _f64(delta), np.zeros(15)
        nv, nc = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_evaluate(self.h, layer.h, _ptr(T, f32p), _ptr(d, f64p), _ptr(out, f64p),
                                                                   C.byref(nv), C.byref(nc)))
        return out, nv.value, nc.value

    def refine(self, layer, T_S_C_prior, options=None, **kw):
        """-> (T_refined [7] f32, usable, delta [4], summary dict); keywords override the default pose-graph options"""
        opts = options if options is not None else pose_graph_options(**kw)
        T, out, delta, s = _f32(T_S_C_prior), np.zeros(7, np.float32), np.zeros(4), ScanRegistrationSummary()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_refine(self.h, layer.h, _ptr(T, f32p), C.byref(opts), _ptr(out, f32p),
                                                                 _ptr(delta, f64p), C.byref(s)))
        d = s.as_dict()
        d["termination"] = TERMINATION_NAMES[s.termination_reason]
        return out, bool(s.usable), delta, d

    def history(self):
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_history(self.h, 0, None, C.byref(n)))
        arr = (PoseGraphIteration * max(n.value, 1))()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_history(self.h, n.value, arr, None))
        return [{name: getattr(arr[k], name) for name, _ in PoseGraphIteration._fields_} for k in range(n.value)]

    # ---- scan localisation (vgx_scan_registration_*_map, _score_poses, _localize): posed finished submaps ----
    def set_map(self, submaps, poses=None, config=None):
        """submaps: capi.Submap handles (at most 64, none clears the map); poses T_M_S [n][7]; config: scan_map_config(...)"""
        n = len(submaps)
        hs = (vp * max(n, 1))(*[sm.h for sm in submaps])
        T = _f32(poses if n else np.zeros((0, 7))).reshape(-1, 7)
        if len(T) != n:
            raise ValueError("one pose per submap")
        self.ctx.check(self.ctx.lib.vgx_scan_registration_set_map(self.h, None if config is None else C.byref(config), n,
                                                                  hs if n else None, _ptr(T, f32p) if n else None))

    def evaluate_map(self, T_M_C_prior, delta=(0.0, 0.0, 0.0, 0.0)):
        """-> (out [15], n_terms, n_points_valid, n_candidates)"""
        T, d, out = _f32(T_M_C_prior), _f64(delta), np.zeros(15)
        nt, nv, nc = C.c_int64(), C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_evaluate_map(self.h, _ptr(T, f32p), _ptr(d, f64p), _ptr(out, f64p),
                                                                       C.byref(nt), C.byref(nv), C.byref(nc)))
        return out, nt.value, nv.value, nc.value

    def refine_map(self, T_M_C_prior, options=None, **kw):
        """-> (T_refined [7] f32, usable, delta [4], summary dict); keywords override the default pose-graph options"""
        opts = options if options is not None else pose_graph_options(**kw)
        T, out, delta, s = _f32(T_M_C_prior), np.zeros(7, np.float32), np.zeros(4), ScanRegistrationSummary()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_refine_map(self.h, _ptr(T, f32p), C.byref(opts), _ptr(out, f32p),
                                                                     _ptr(delta, f64p), C.byref(s)))
        d = s.as_dict()
        d["termination"] = TERMINATION_NAMES[s.termination_reason]
        return out, bool(s.usable), delta, d

    def score_poses(self, poses):
        """poses T_M_C [m][7] -> (cost [m] f64, n_terms [m], n_points_valid [m], n_candidates [m]) at delta = 0"""
        T = _f32(poses).reshape(-1, 7)
        m = len(T)
        cost = np.zeros(m)
        counts = [np.zeros(m, np.int64) for _ in range(3)]
        self.ctx.check(self.ctx.lib.vgx_scan_registration_score_poses(self.h, m, _ptr(T, f32p) if m else None, _ptr(cost, f64p),
                                                                      *[_ptr(c, i64p) for c in counts]))
        return (cost, *counts)

    def localize(self, poses, options=None, **kw):
        """-> (best_index, T_refined [7] f32, usable, delta [4], summary dict): the hypotheses scored, the best one refined"""
        opts = options if options is not None else pose_graph_options(**kw)
        T = _f32(poses).reshape(-1, 7)
        best, out, delta, s = C.c_int32(), np.zeros(7, np.float32), np.zeros(4), ScanRegistrationSummary()
        self.ctx.check(self.ctx.lib.vgx_scan_registration_localize(self.h, len(T), _ptr(T, f32p) if len(T) else None, C.byref(opts),
                                                                   C.byref(best), _ptr(out, f32p), _ptr(delta, f64p), C.byref(s)))
        d = s.as_dict()
        d["termination"] = TERMINATION_NAMES[s.termination_reason]
        return best.value, out, bool(s.usable), delta, d

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_scan_registration_destroy(self.h)
            self.h = None


def scan_map_config(**kw):
    """vgx_scan_map_config: the defaults and fields overridden by keyword; layer takes "esdf" / "tsdf" too"""
    cfg = ScanMapConfig()
    load().vgx_scan_map_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, {"esdf": EVAL_LAYER_ESDF, "tsdf": EVAL_LAYER_TSDF}.get(v, v) if k == "layer" else v)
    return cfg


def view_config(s_max, min_step, unknown_step, max_bracket, **kw):
    """vgx_view_config: the defaults, the four fields that have none and fields overridden by keyword (s_min, step_scale,
    image_width, flags)"""
    cfg = ViewConfig()
    load().vgx_view_config_default(C.byref(cfg))
    cfg.s_max, cfg.min_step, cfg.unknown_step, cfg.max_bracket = s_max, min_step, unknown_step, max_bracket
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def view_config_check(config):
    """vgx_view_config_check (host only): OK, or the code vgx_view_create refuses this config with"""
    return load().vgx_view_config_check(None if config is None else C.byref(config))


def view_rays_pinhole(width, height, fx, fy, cx, cy):
    """vgx_view_rays_pinhole (host only): unit directions [height * width][3] f32, row-major"""
    dirs = np.zeros((int(height) * int(width), 3), np.float32)
    rc = load().vgx_view_rays_pinhole(int(width), int(height), float(fx), float(fy), float(cx), float(cy), _ptr(dirs, f32p))
    if rc != OK:
        raise VgxError(rc, "vgx_view_rays_pinhole: width or height < 1, a parameter not finite, or a zero focal length")
    return dirs


def view_rays_lidar(width, height, elevation_min, elevation_max, azimuth_offset=0.0):
    """vgx_view_rays_lidar (host only): unit directions [height * width][3] f32, row-major (one row per elevation)"""
    dirs = np.zeros((int(height) * int(width), 3), np.float32)
    rc = load().vgx_view_rays_lidar(int(width), int(height), float(elevation_min), float(elevation_max), float(azimuth_offset),
                                    _ptr(dirs, f32p))
    if rc != OK:
        raise VgxError(rc, "vgx_view_rays_lidar: width or height < 1, or a parameter not finite")
    return dirs


ViewImage = collections.namedtuple("ViewImage", ["range", "status", "points", "gradient", "weight", "rgba", "n_samples"])


def _render_view(ctx, host_call, device_call, source, view, T, dirs, n):
    """dirs: a numpy array [n][3] (copied), a torch device tensor [n][3] f32, or a device address as an int with n"""
    T = _f32(T)
    if isinstance(dirs, int):
        ctx.check(device_call(source.h, view.h, _ptr(T, f32p), int(n), vp(dirs) if dirs else None))
    elif hasattr(dirs, "data_ptr"):
        if not dirs.is_cuda or str(dirs.dtype) != "torch.float32" or not dirs.is_contiguous():
            raise TypeError("a contiguous float32 device tensor [n][3]")
        m = dirs.numel() // 3
        ctx.check(device_call(source.h, view.h, _ptr(T, f32p), m, vp(dirs.data_ptr()) if m else None))
    else:
        d = _f32(dirs).reshape(-1, 3)
        ctx.check(host_call(source.h, view.h, _ptr(T, f32p), len(d), _ptr(d, f32p) if len(d) else None))
    return view


class View:
    """A rendered view on the GPU (vgx_view): per ray range, status and -- by the config's flags -- sensor-frame point,
    gradient, weight, colour and sample count; reused from call to call."""

    def __init__(self, ctx, config):
        self.ctx = ctx
        self.flags = 0 if config is None else int(config.flags)
        h = vp()
        ctx.check(ctx.lib.vgx_view_create(ctx.h, None if config is None else C.byref(config), C.byref(h)))
        self.h = h

    def stats(self):
        """the counts of the view held now: n_rays, n_hit, n_hit_unsampled, n_miss, n_inside, n_bad, n_samples"""
        c = ViewCounts()
        self.ctx.check(self.ctx.lib.vgx_view_stats(self.h, C.byref(c)))
        return c.as_dict()

    def download(self):
        """ViewImage(range [n] f32, status [n] u8, points [n][3], gradient [n][3], weight [n], rgba [n][4] u8, n_samples
        [n] i32); None for an output the flags do not hold"""
        n, f = self.stats()["n_rays"], self.flags
        rng, status = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        points = np.zeros((n, 3), np.float32) if f & VIEW_POINTS else None
        gradient = np.zeros((n, 3), np.float32) if f & VIEW_GRADIENT else None
        weight = np.zeros(n, np.float32) if f & VIEW_WEIGHT else None
        rgba = np.zeros((n, 4), np.uint8) if f & VIEW_RGBA else None
        samples = np.zeros(n, np.int32) if f & VIEW_N_SAMPLES else None
        self.ctx.check(self.ctx.lib.vgx_view_download(self.h, _ptr(rng, f32p), _ptr(status, u8p), _ptr(points, f32p),
                                                      _ptr(gradient, f32p), _ptr(weight, f32p), _ptr(rgba, u32p),
                                                      _ptr(samples, i32p)))
        return ViewImage(rng, status, points, gradient, weight, rgba, samples)

    def device_pointers(self):
        """ViewImage of device addresses as ints (None where the view holds none)"""
        p = [vp() for _ in range(7)]
        self.ctx.check(self.ctx.lib.vgx_view_device_pointers(self.h, *[C.byref(x) for x in p]))
        return ViewImage(*[x.value for x in p])

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_view_destroy(self.h)
            self.h = None


def evaluate_layers_rmse_cloud(gt, test, layer=EVAL_LAYER_ESDF, mode=EVAL_IGNORE_BEHIND_TEST, config=None, cloud=None):
    """evaluateLayersRmse and the point-cloud view of its error layer in one call (vgx_evaluate_layers_rmse_cloud): the
    error layer never leaves the device.  Returns (details dict, Cloud)."""
    ctx = gt.ctx
    cloud = cloud if cloud is not None else Cloud(ctx)
    det = EvaluationDetails()
    ctx.check(ctx.lib.vgx_evaluate_layers_rmse_cloud(gt.h, test.h, int(layer), int(mode), C.byref(det),
                                                     None if config is None else C.byref(config), cloud.h))
    return det.as_dict(), cloud


def decoupled_exp_pose(pose4):
    """Transformation::exp((x, y, z, 0, 0, yaw)) as [qw,qx,qy,qz, tx,ty,tz] f64: minkindr's decoupled exp (the
    translation is taken as it is, the rotation is about z) -- map_evaluation.cpp:155-159.  Formed in f64; the library
    rounds it to f32, as gpu_map_evaluation.h does."""
    x, y, z, yaw = (float(v) for v in pose4)
    return np.array([math.cos(0.5 * yaw), 0.0, 0.0, math.sin(0.5 * yaw), x, y, z])


def pose7_inverse(T):
    """T.inverse() of [qw,qx,qy,qz, tx,ty,tz] (f64): conjugate rotation, translation -(q^-1 t)."""
    T = np.asarray(T, np.float64)
    w, v = T[0], -T[1:4]
    t = T[4:7]
    uv = 2.0 * np.cross(v, t)
    r = t + w * uv + np.cross(v, uv)
    return np.concatenate([[w], v, -r])


def map_evaluation(ctx, submaps, poses, gt_submap, align, voxel_size=None, vps=None, error_layer=False,
                   min_voxel_weight=1.0, max_voxel_distance=0.3, cloud=None):
    """MapEvaluation::evaluate (map_evaluation.cpp:59-114) on the device.  submaps / poses ([n][7]) are the collection,
    gt_submap the ground truth (a submap holding its raw TSDF layer, identity pose).  Steps: the projected map; both
    finished (ESDF, kVoxels points); pose4 = align(reference = projected map, reading = ground truth) -- the caller's
    solver over a RegistrationCostFunction(reference, reading) with the reference constant at 0, as
    alignSubmapAtoSubmapB does; the ground truth resampled by T = Transformation::exp(x, y, z, 0, 0, yaw)
    (vgx_tsdf_layer_transform_submap) and its ESDF regenerated; evaluateLayersRmse(gt ESDF, projected ESDF,
    kIgnoreErrorBehindTestSurface).  Returns {"details", "pose4", "T_ground_truth__reading" (= T.inverse(), [7] f64)}
    and, with error_layer=True, "error_layer".  cloud=cloud_config(...): the evaluation goes through
    vgx_evaluate_layers_rmse_cloud instead and "error_cloud" holds the Cloud of the error layer (the caller destroys it);
    the details are the same bit for bit."""
    vs = float(voxel_size if voxel_size is not None else gt_submap.voxel_size)
    vps = int(vps if vps is not None else gt_submap.vps)
    proj_layer = TsdfLayer(ctx, vs, vps)
    gt_layer = TsdfLayer(ctx, vs, vps)
    proj = gt_t = None
    try:
        projected_map(ctx, submaps, poses, proj_layer)
        proj = Submap.from_tsdf_layer(ctx, proj_layer, 1)
        for sm in (proj, gt_submap):       # finishSubmap()
            sm.generate_esdf()
            sm.extract_voxel_points(min_voxel_weight, max_voxel_distance)
        pose4 = np.asarray(align(proj, gt_submap), np.float64).reshape(4)
        T = decoupled_exp_pose(pose4)
        gt_layer.transform_submap(gt_submap, T)           # transformSubmap(T): transformLayer, then finishSubmap()
        gt_t = Submap.from_tsdf_layer(ctx, gt_layer, int(ctx.lib.vgx_submap_id(gt_submap.h)))
        gt_t.generate_esdf()
        out = {"pose4": pose4, "T_ground_truth__reading": pose7_inverse(T)}
        if cloud is not None:
            if error_layer:
                raise ValueError("map_evaluation: error_layer and cloud are alternatives")
            out["details"], out["error_cloud"] = evaluate_layers_rmse_cloud(gt_t, proj, EVAL_LAYER_ESDF,
                                                                            EVAL_IGNORE_BEHIND_TEST, cloud)
            return out
        res = evaluate_layers_rmse(gt_t, proj, EVAL_LAYER_ESDF, EVAL_IGNORE_BEHIND_TEST, error_layer)
        if error_layer:
            out["details"], out["error_layer"] = res
        else:
            out["details"] = res
        return out
    finally:
        for o in (gt_t, proj, gt_layer, proj_layer):
            if o is not None:
                o.destroy()


MESH_COLORS_NONE, MESH_COLORS_PER_TRIANGLE, MESH_COLORS_PER_VERTEX = 0, 1, 2


class Mesh:
    """A voxblox MeshLayer on the GPU (vgx_mesh): per allocated block, in ascending block-index order, a range of
    triangles; reused from call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_mesh_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """(blocks, triangles)"""
        nb, nt = C.c_int32(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_mesh_stats(self.h, C.byref(nb), C.byref(nt)))
        return nb.value, nt.value

    def download(self):
        """(block_index [nb][3] int32, first [nb+1] int64, vertices [T][3][3] f32, normals [T][3] f32)"""
        nb, nt = self.stats()
        bi = np.zeros((nb, 3), np.int32)
        first = np.zeros(nb + 1, np.int64)
        v = np.zeros((nt, 3, 3), np.float32)
        n = np.zeros((nt, 3), np.float32)
        self.ctx.check(self.ctx.lib.vgx_mesh_download(self.h, _ptr(bi, i32p), _ptr(first, i64p), _ptr(v, f32p),
                                                      _ptr(n, f32p)))
        return bi, first, v, n

    def has_colors(self):
        """True after a separated mesh or a coloured mesh (vgx_mesh_has_colors)"""
        has = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_mesh_has_colors(self.h, C.byref(has)))
        return bool(has.value)

    def color_layout(self):
        """MESH_COLORS_NONE / _PER_TRIANGLE / _PER_VERTEX (vgx_mesh_color_layout)"""
        layout = C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_mesh_color_layout(self.h, C.byref(layout)))
        return layout.value

    def download_vertex_colors(self):
        """rgba [T][3][4] uint8, one colour per soup vertex (vgx_mesh_download_vertex_colors; any other layout raises)"""
        _, nt = self.stats()
        out = np.zeros((nt, 3, 4), np.uint8)
        self.ctx.check(self.ctx.lib.vgx_mesh_download_vertex_colors(self.h, _ptr(out, u8p)))
        return out

    def download_colors(self):
        """rgba [T][4] uint8, one colour per triangle (vgx_mesh_download_colors; a mesh without colours raises)"""
        _, nt = self.stats()
        out = np.zeros((nt, 4), np.uint8)
        self.ctx.check(self.ctx.lib.vgx_mesh_download_colors(self.h, _ptr(out, u8p)))
        return out

    def generate_separated(self, submaps, poses, colors, min_weight=1e-4):
        """vgx_submaps_generate_separated_mesh in ARRAY order: submaps[i] at poses[i] ([n][7] qw,qx,qy,qz, tx,ty,tz)
        coloured colors[i] ([n][4] uint8).  Returns self."""
        n = len(submaps)
        arr = (vp * max(n, 1))(*[s.h for s in submaps])
        T = np.ascontiguousarray(poses, np.float32).reshape(n, 7)
        rgba = np.ascontiguousarray(colors, np.uint8).reshape(n, 4)
        cfg = MeshConfig(float(min_weight))
        self.ctx.check(self.ctx.lib.vgx_submaps_generate_separated_mesh(self.ctx.h, n, arr, _ptr(T, f32p), _ptr(rgba, u8p),
                                                                        C.byref(cfg), self.h))
        return self

    def write_ply(self, path):
        self.ctx.check(self.ctx.lib.vgx_mesh_write_ply(self.h, os.fsencode(path)))

    def connect(self, threshold=1e-10, out=None):
        """voxblox createConnectedMesh over this mesh's triangle soup (vgx_mesh_connect): vertices in the same cell of a
        grid of pitch `threshold` (an f32; voxblox's default 1e-10f) become one.  Returns the ConnectedMesh (a new one
        when out is None)."""
        out = out if out is not None else ConnectedMesh(self.ctx)
        self.ctx.check(self.ctx.lib.vgx_mesh_connect(self.h, C.c_float(threshold), out.h))
        return out

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_mesh_destroy(self.h)
            self.h = None


class ConnectedMesh:
    """A voxblox connected Mesh on the GPU (vgx_connected_mesh): unique vertices in order of first occurrence, with the
    normal (and colour) of their first triangle, and [T][3] indices; reused from call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_connected_mesh_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """(vertices, triangles, has_colors)"""
        nv, nt, has = C.c_int64(), C.c_int64(), C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_connected_mesh_stats(self.h, C.byref(nv), C.byref(nt), C.byref(has)))
        return nv.value, nt.value, bool(has.value)

    def download(self):
        """(vertices [V][3] f32, normals [V][3] f32, rgba [V][4] uint8 or None, indices [T][3] uint32)"""
        nv, nt, has = self.stats()
        v = np.zeros((nv, 3), np.float32)
        n = np.zeros((nv, 3), np.float32)
        c = np.zeros((nv, 4), np.uint8) if has else None
        idx = np.zeros((nt, 3), np.uint32)
        self.ctx.check(self.ctx.lib.vgx_connected_mesh_download(self.h, _ptr(v, f32p), _ptr(n, f32p),
                                                                None if c is None else _ptr(c, u8p), _ptr(idx, u32p)))
        return v, n, c, idx

    def write_ply(self, path):
        self.ctx.check(self.ctx.lib.vgx_connected_mesh_write_ply(self.h, os.fsencode(path)))

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_connected_mesh_destroy(self.h)
            self.h = None


class MeshMarker:
    """marker.points and marker.colors of a mesh's visualization_msgs/Marker on the GPU (vgx_mesh_marker): [3T][3] f64
    and [3T][4] f32 in soup order; reused from call to call."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = vp()
        ctx.check(ctx.lib.vgx_mesh_marker_create(ctx.h, C.byref(h)))
        self.h = h

    def stats(self):
        """(points, color mode of the last accepted fill)"""
        n, mode = C.c_int64(), C.c_int32()
        self.ctx.check(self.ctx.lib.vgx_mesh_marker_stats(self.h, C.byref(n), C.byref(mode)))
        return n.value, mode.value

    def download(self):
        """(points [n][3] f64, colors [n][4] f32)"""
        n, _ = self.stats()
        points = np.zeros((n, 3), np.float64)
        colors = np.zeros((n, 4), np.float32)
        self.ctx.check(self.ctx.lib.vgx_mesh_marker_download(self.h, _ptr(points, f64p), _ptr(colors, f32p)))
        return points, colors

    def device_pointers(self):
        """(points, colors) device addresses as ints (None when the marker holds no points)"""
        p = [vp(), vp()]
        self.ctx.check(self.ctx.lib.vgx_mesh_marker_device_pointers(self.h, C.byref(p[0]), C.byref(p[1])))
        return tuple(x.value for x in p)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_mesh_marker_destroy(self.h)
            self.h = None


def mesh_marker_config(**kw):
    """vgx_mesh_marker_config_default with fields replaced: color_mode, opacity, use_constant_color, constant_rgba"""
    cfg = MeshMarkerConfig()
    load().vgx_mesh_marker_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k == "constant_rgba":
            cfg.constant_rgba = (C.c_uint8 * 4)(*[int(x) for x in v])
        else:
            setattr(cfg, k, v)
    return cfg


def fill_marker(mesh, color_mode=MARKER_LAMBERT_COLOR, opacity=1.0, constant_rgba=None, out=None):
    """voxblox_ros fillMarkerWithMesh over `mesh` (a Mesh) in `color_mode` (vgx_mesh_fill_marker), `opacity` in every
    alpha; constant_rgba: cblox colorMeshLayer(constant_rgba) first.  Returns the MeshMarker (a new one when out is
    None)."""
    cfg = mesh_marker_config(color_mode=int(color_mode), opacity=float(opacity))
    if constant_rgba is not None:
        cfg = mesh_marker_config(color_mode=int(color_mode), opacity=float(opacity), use_constant_color=1,
                                 constant_rgba=constant_rgba)
    out = out if out is not None else MeshMarker(mesh.ctx)
    mesh.ctx.check(mesh.ctx.lib.vgx_mesh_fill_marker(mesh.h, C.byref(cfg), out.h))
    return out


def mc_triangle_table():
    """the [256][16] int8 triangle table the mesh kernels read (vgx_mesh_triangle_table; no device needed)"""
    out = np.zeros((256, 16), np.int8)
    rc = load().vgx_mesh_triangle_table(out.ctypes.data_as(C.POINTER(C.c_int8)))
    if rc != OK:
        raise VgxError(rc, "vgx_mesh_triangle_table")
    return out


class FastTsdfIntegrator:
    """Mirror of voxblox::FastTsdfIntegrator as voxgraph drives it
    (pointcloud_integrator.cpp:66-83): ctor(config, layer), setLayer, integratePointCloud."""

    def __init__(self, ctx, config, layer):
        self.ctx, self.config, self.layer = ctx, config, layer
        h = vp()
        ctx.check(ctx.lib.vgx_tsdf_integrator_create(ctx.h, C.byref(config), layer.h, C.byref(h)))
        self.h = h

    def setLayer(self, layer):
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_set_layer(self.h, layer.h))
        self.layer = layer

    def integratePointCloud(self, T_G_C, points_C, colors=None, freespace_points=False, count=True):
        """count=False: n_updates == NULL, voxblox's void call -- uncounted, returns with the scan queued"""
        T = _f32(T_G_C)
        pts = _f32(points_C).reshape(-1, 3)
        col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate(self.h, _ptr(T, f32p), _ptr(pts, f32p),
                                                       _ptr(col, u8p), pts.shape[0],
                                                       int(freespace_points), C.byref(n) if count else None))
        return n.value

    def integratePointCloudMerged(self, T_G_C, points_C, colors=None, freespace_points=False):
        """voxblox::MergedTsdfIntegrator::integratePointCloud (same config / layer)"""
        T = _f32(T_G_C)
        pts = _f32(points_C).reshape(-1, 3)
        col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        n = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_merged(self.h, _ptr(T, f32p), _ptr(pts, f32p),
                                                              _ptr(col, u8p), pts.shape[0],
                                                              int(freespace_points), C.byref(n)))
        return n.value

    def integrate_merged_device(self, T_G_C, d_points, d_rgba, n, freespace_points=False, count=False):
        T = _f32(T_G_C)
        out = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_merged_device(
            self.h, _ptr(T, f32p), vp(d_points), vp(d_rgba) if d_rgba else None, n,
            int(freespace_points), C.byref(out) if count else None))
        return out.value

    def integrate_device(self, T_G_C, d_points, d_rgba, n, freespace_points=False, count=False):
        T = _f32(T_G_C)
        out = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_device(
            self.h, _ptr(T, f32p), vp(d_points), vp(d_rgba) if d_rgba else None, n,
            int(freespace_points), C.byref(out) if count else None))
        return out.value

    def integrate_scan(self, T_G_C, scan, freespace_points=False, count=True):
        """integratePointCloud of a decoded Scan (vgx_tsdf_integrate_scan); count=False: returns with the scan queued"""
        T = _f32(T_G_C)
        out = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_scan(self.h, _ptr(T, f32p), scan.h, int(freespace_points),
                                                            C.byref(out) if count else None))
        return out.value

    def integrate_depth_image(self, T_G_C, layout, camera, depth, color=None, count=True):
        """Projective integration of a depth image and its registered colour image (host bytes; color None for
        IMAGE_COLOR_NONE): vgx_tsdf_integrate_depth_image.  Returns the frame's counts as a dict; count=False: None, and
        the call returns with the frame queued."""
        T = _f32(T_G_C)
        (dp, dn), (cp, cn) = _image_bytes(depth), _image_bytes(color)
        out = ProjectiveCounts()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_depth_image(self.h, _ptr(T, f32p), C.byref(layout), C.byref(camera), dp, dn,
                                                                   cp, cn, C.byref(out) if count else None))
        return {k: getattr(out, k) for k, _ in ProjectiveCounts._fields_} if count else None

    def integrate_depth_image_device(self, T_G_C, layout, camera, d_depth, depth_n_bytes, d_color=None, color_n_bytes=0, count=True):
        """the same with the images at device addresses (ready with respect to the TSDF stream)"""
        T = _f32(T_G_C)
        dp, cp = (vp(a) if a else None for a in (d_depth, d_color))
        out = ProjectiveCounts()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_depth_image_device(
            self.h, _ptr(T, f32p), C.byref(layout), C.byref(camera), dp, int(depth_n_bytes), cp, int(color_n_bytes),
            C.byref(out) if count else None))
        return {k: getattr(out, k) for k, _ in ProjectiveCounts._fields_} if count else None

    def integrate_range_image(self, T_G_S, image, count=True):
        """Projective integration of a RangeImage (vgx_tsdf_integrate_range_image).  Returns the frame's counts as a dict;
        count=False: None, and the call returns with the frame queued."""
        T = _f32(T_G_S)
        out = ProjectiveCounts()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_range_image(self.h, _ptr(T, f32p), image.h, C.byref(out) if count else None))
        return {k: getattr(out, k) for k, _ in ProjectiveCounts._fields_} if count else None

    def integrate_merged_scan(self, T_G_C, scan, freespace_points=False, count=True):
        """MergedTsdfIntegrator::integratePointCloud of a decoded Scan (vgx_tsdf_integrate_merged_scan)"""
        T = _f32(T_G_C)
        out = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrate_merged_scan(self.h, _ptr(T, f32p), scan.h, int(freespace_points),
                                                                   C.byref(out) if count else None))
        return out.value

    def set_cloud_width(self, width):
        """organised clouds: points per row (sensor_msgs/PointCloud2.width); 0 = unorganised"""
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_set_cloud_width(self.h, int(width)))

    def set_speculation(self, depth=32, threshold=8 << 20):
        """test tooling (reproducible mode): write rays out `depth` steps deep at first when a scan's complete
        walks exceed `threshold` steps; the layer does not depend on either"""
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_set_speculation(self.h, depth, threshold))

    def set_projective_age(self, epoch, tickets):
        """test tooling: the chain clock of the projective frames (vgx_tsdf_integrator_set_projective_age)"""
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_set_projective_age(self.h, int(epoch), int(tickets)))

    def get_projective_age(self):
        """test tooling: (epoch, tickets) of the projective frames' chain clock"""
        e, t = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_get_projective_age(self.h, C.byref(e), C.byref(t)))
        return e.value, t.value

    def set_reproducible_age(self, epoch):
        """test tooling: the epoch of the reproducible-mode scratch (vgx_tsdf_integrator_set_reproducible_age)"""
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_set_reproducible_age(self.h, int(epoch)))

    def get_reproducible_age(self):
        """test tooling: the epoch of the reproducible-mode scratch"""
        e = C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_get_reproducible_age(self.h, C.byref(e)))
        return e.value

    def read_trace(self, max_workgroups):
        """last counted racing scan -> [workgroups][16] float64: four stamps in microseconds relative to the first start,
        then rays, rounds, per-voxel folds, longest chain of repeated folds, and the workgroup's eight statistics"""
        buf = np.zeros((int(max_workgroups), 16), np.int64)
        n, khz = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_read_trace(self.h, _ptr(buf, i64p), int(max_workgroups),
                                                                   C.byref(n), C.byref(khz)))
        t = buf[:min(n.value, int(max_workgroups))].astype(np.float64)
        if len(t):
            t0 = t[:, 0].min()
            t[:, :4] = (t[:, :4] - t0) * 1e3 / max(khz.value, 1)
        return t

    def walk_stats(self):
        """bench tooling, last counted racing scan (include/voxgraph_amd_bench.h): dict of the seven numbers"""
        out = (C.c_int64 * 7)()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_walk_stats(self.h, out))
        names = ("longest_chain", "exchanges", "colour_blends", "peeks", "voxel_folds", "cas_retries", "overrun_exchanges")
        return {k: int(v) for k, v in zip(names, out)}

    def set_event_trace(self, capacity_words):
        """test tooling: racing scans from now on run the event-logging form of the shipped kernel (0: off)"""
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_set_event_trace(self.h, int(capacity_words)))
        self._trace_cap = int(capacity_words)

    def read_event_trace(self):
        """-> (uint64 words of the log since the last read, events lost to a full log); empties the log"""
        buf = np.zeros(self._trace_cap, np.uint64)
        n, lost = C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_read_event_trace(
            self.h, _ptr(buf, C.POINTER(C.c_uint64)), len(buf), C.byref(n), C.byref(lost)))
        return buf[:n.value].copy(), int(lost.value)

    def download_sets(self):
        """-> (start set, observed set: uint64[2^20] each, (start offset, observed offset, scans since the last reset))"""
        a, b = np.zeros(1 << 20, np.uint64), np.zeros(1 << 20, np.uint64)
        st = (C.c_int64 * 3)()
        self.ctx.check(self.ctx.lib.vgx_tsdf_integrator_download_sets(
            self.h, _ptr(a, C.POINTER(C.c_uint64)), _ptr(b, C.POINTER(C.c_uint64)), st))
        return a, b, tuple(int(x) for x in st)

    def destroy(self):
        if self.h:
            self.ctx.lib.vgx_tsdf_integrator_destroy(self.h)
            self.h = None


# ------------------------------------------------------------------ saved maps
FILE_CBLOX_COLLECTION, FILE_VOXBLOX_LAYER = 0, 1


class MapFile:
    """A cblox submap-collection file (voxgraph's save_to_file) or a voxblox layer file.
    Host-only except load_submap()."""

    def __init__(self, path, fmt=FILE_CBLOX_COLLECTION):
        self.lib = load()
        h = vp()
        rc = self.lib.vgx_map_file_open(os.fsencode(path), fmt, C.byref(h))
        if rc != 0:
            raise VgxError(rc, self.lib.vgx_map_file_last_error(None).decode())
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise VgxError(rc, self.lib.vgx_map_file_last_error(self.h).decode())

    def __len__(self):
        return int(self.lib.vgx_map_file_num_submaps(self.h))

    def info(self, i):
        info = MapFileSubmapInfo()
        self._check(self.lib.vgx_map_file_get_submap_info(self.h, i, C.byref(info)))
        return info

    def read_submap(self, i, want_rgba=False):
        """-> dict(block_index, tsdf_distance, tsdf_weight, [tsdf_rgba], esdf_distance, esdf_observed)"""
        info = self.info(i)
        nb, vox = info.n_tsdf_blocks, info.voxels_per_side ** 3
        out = dict(block_index=np.zeros((nb, 3), np.int32), tsdf_distance=np.zeros((nb, vox), np.float32),
                   tsdf_weight=np.zeros((nb, vox), np.float32),
                   tsdf_rgba=np.zeros((nb, vox, 4), np.uint8) if want_rgba else None,
                   esdf_distance=np.zeros((nb, vox), np.float32), esdf_observed=np.zeros((nb, vox), np.uint8))
        self._check(self.lib.vgx_map_file_read_submap(
            self.h, i, _ptr(out["block_index"], i32p), _ptr(out["tsdf_distance"], f32p),
            _ptr(out["tsdf_weight"], f32p), _ptr(out["tsdf_rgba"], u8p),
            _ptr(out["esdf_distance"], f32p), _ptr(out["esdf_observed"], u8p)))
        return out

    def load_submap(self, ctx, i):
        """VoxgraphSubmap::LoadFromStream onto the device (not yet finished)."""
        sm = Submap.__new__(Submap)
        sm.ctx = ctx
        h = vp()
        self._check(self.lib.vgx_map_file_load_submap(ctx.h, self.h, i, C.byref(h)))
        sm.h = h
        return sm

    def close(self):
        if getattr(self, "h", None):
            self.lib.vgx_map_file_close(self.h)
            self.h = None

    __del__ = close


def write_map_file(path, fmt, voxel_size, vps, submaps):
    """submaps: list of dict(id, T_M_S[7], block_index, tsdf_distance, tsdf_weight,
    tsdf_rgba=None, esdf_distance=None, esdf_observed=None)"""
    lib = load()
    arr = (MapFileSubmapData * len(submaps))()
    keep = []
    for k, s in enumerate(submaps):
        bi = np.ascontiguousarray(s["block_index"], np.int32).reshape(-1, 3)
        td, tw = _f32(s["tsdf_distance"]), _f32(s["tsdf_weight"])
        rgba = None if s.get("tsdf_rgba") is None else np.ascontiguousarray(s["tsdf_rgba"], np.uint8)
        ed = _f32(s.get("esdf_distance"))
        eo = None if s.get("esdf_observed") is None else np.ascontiguousarray(s["esdf_observed"], np.uint8)
        keep += [bi, td, tw, rgba, ed, eo]
        arr[k].id = int(s.get("id", k))
        for a, v in enumerate(s.get("T_M_S", (1, 0, 0, 0, 0, 0, 0))):
            arr[k].T_M_S[a] = float(v)
        arr[k].n_blocks = bi.shape[0]
        arr[k].block_index, arr[k].tsdf_distance, arr[k].tsdf_weight = _ptr(bi, i32p), _ptr(td, f32p), _ptr(tw, f32p)
        arr[k].tsdf_rgba, arr[k].esdf_distance, arr[k].esdf_observed = _ptr(rgba, u8p), _ptr(ed, f32p), _ptr(eo, u8p)
    rc = lib.vgx_map_file_write(os.fsencode(path), fmt, float(voxel_size), int(vps), len(submaps), arr)
    if rc != 0:
        raise VgxError(rc, lib.vgx_map_file_last_error(None).decode())
