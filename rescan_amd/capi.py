"""ctypes binding of include/rescan_hip.h (librescan_hip.so) and a thin Python mirror of the
reference's operator names for the hot path (icp_align, alignment scores, arrangement_to_labels).

There is deliberately no CPU fallback here: if the HIP extension is missing, or no HIP device
is usable, every call raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librescan_hip.so")

f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
i8p = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")

# name -> (restype, argtypes); kept in one table so the symbol test can walk it.
SIGNATURES = {
    "rs_hip_init": (C.c_int, [C.c_int]),
    "rs_hip_last_error": (C.c_char_p, []),
    "rs_hip_set_stream": (C.c_int, [C.c_void_p]),
    "rs_hip_synchronize": (C.c_int, []),
    "rs_hip_stream_cu_mask": (C.c_int, [C.c_void_p, C.c_int32]),
    "rs_hip_get_stream": (C.c_void_p, []),
    "rs_hip_version": (C.c_char_p, []),
    "rs_hip_switch_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_double)]),
    "rs_hip_profile_enable": (C.c_int, [C.c_int]),
    "rs_hip_profile_reset": (C.c_int, []),
    "rs_hip_profile_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "rs_hip_cloud_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float]),
    "rs_hip_cloud_create_many": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rs_hip_cloud_many_single_above": (C.c_int32, [C.c_int32]),
    "rs_hip_cloud_destroy": (None, [C.c_void_p]),
    "rs_hip_profile_marker": (C.c_int, []),
    "rs_hip_cloud_size": (C.c_int32, [C.c_void_p]),
    "rs_hip_cloud_tiles": (C.c_int32, [C.c_void_p]),
    "rs_hip_cloud_bytes": (C.c_int64, [C.c_void_p]),
    "rs_hip_cloud_layout": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rs_hip_cloud_build_seconds": (C.c_int64, [C.POINTER(C.c_double), C.c_int32]),
    "rs_hip_radius_search": (C.c_int, [C.c_void_p, f32p, C.c_int64, C.c_float, C.c_int32, f32p, i32p, u64p,
                                       C.POINTER(C.c_uint64)]),
    "rs_hip_knn_grid_create": (C.c_void_p, [C.c_void_p, C.c_float, C.c_int32]),
    "rs_hip_knn_grid_destroy": (None, [C.c_void_p]),
    "rs_hip_knn_grid_geometry": (C.c_int, [C.c_void_p, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.POINTER(C.c_double), f32p]),
    "rs_hip_knn_geometry": (C.c_int, [f32p, C.c_int64, C.c_float, C.c_int32, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"),
                                      C.POINTER(C.c_double), f32p]),
    "rs_hip_knn_search": (C.c_int, [C.c_void_p, f32p, C.c_int64, C.c_int32, f32p, i32p, u64p, C.POINTER(C.c_uint64)]),
    "rs_hip_icp_align": (C.c_int, [C.c_void_p, C.c_void_p, f32p, f32p, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "rs_hip_icp_align_traced": (C.c_int, [C.c_void_p, C.c_void_p, f32p, f32p, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_float), C.POINTER(C.c_int32), f32p]),
    "rs_hip_icp_trace_begin": (C.c_int, [f32p, f32p, i32p, i32p, C.c_int32, C.c_int32]),
    "rs_hip_icp_trace_end": (C.c_int, []),
    "rs_hip_icp_reference_order_below": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_replay_below": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_lane_chains_below": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_lane_chains_sequential": (C.c_int64, []),
    "rs_hip_icp_stop_guard_redone": (C.c_int64, []),
    "rs_hip_icp_stop_guard": (C.c_float, [C.c_float]),
    "rs_hip_icp_early_plain": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_plain_from_records": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_update_fenced": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_state_layout": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rs_hip_icp_replay_redone": (C.c_int32, []),
    "rs_hip_icp_faith_redone": (C.c_int32, []),
    "rs_hip_icp_faith_guess": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_exact_centroids": (C.c_int32, [C.c_int32]),
    "rs_hip_score_scene_space_from": (C.c_int64, [C.c_int64]),
    "rs_hip_icp_chains_retry_after": (C.c_int32, [C.c_int32]),
    "rs_hip_icp_chains_gave_up": (C.c_int32, []),
    "rs_hip_icp_align_batch": (C.c_int, [C.c_void_p, C.c_void_p, f32p, C.c_int32, f32p, C.c_float, C.c_float,
                                         C.c_int32, C.c_int32, f32p, i32p]),
    "rs_hip_icp_align_multi": (C.c_int, [C.c_void_p, C.c_void_p, f32p, C.c_int32, f32p, C.c_float, C.c_float,
                                         C.c_int32, C.c_int32, f32p, i32p]),
    "rs_hip_icp_find_corrs": (C.c_int, [C.c_void_p, C.c_void_p, f32p, f32p, C.c_float, C.c_float,
                                        f32p, f32p, f32p, f32p, f32p, C.POINTER(C.c_int32)]),
    "rs_hip_alignment_scores": (C.c_int, [C.c_void_p, C.c_void_p, f32p, C.c_int32, C.c_float, C.c_int32, f32p]),
    "rs_hip_assign_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, i8p, f32p]),
    "rs_hip_label_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int]),
    "rs_hip_combine_label_rows": (None, [f32p, C.c_int32, C.c_int64, C.c_int32, i8p, f32p]),
    "rs_hip_label_partial_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rs_hip_fold_label_partials_device": (C.c_int, [C.c_void_p, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"),
                                                    C.c_int32, C.c_int64, i8p, f32p, C.c_void_p]),
    "rs_hip_fold_label_rows_device": (C.c_int, [C.c_void_p, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS"), C.c_int32,
                                                C.c_int64, C.c_int32, i8p, f32p, C.c_int32, C.c_void_p]),
    "rs_hip_arrangement_to_labels": (C.c_int, [C.c_void_p, f32p, C.c_void_p, i32p, i32p, C.c_int32, C.c_float,
                                               C.c_int, i8p, f32p, i32p]),
    "rs_hip_arrangement_to_ids": (C.c_int, [C.c_void_p, f32p, C.c_void_p, i32p, i32p, i32p, C.c_int32, C.c_float, C.c_int, C.c_int32,
                                            i32p, i32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_gather_attributes": (C.c_int, [i32p, C.c_int32, C.c_int32, C.c_void_p, i32p, C.c_void_p, C.c_int32]),
    "rs_hip_compute_neighborhood": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, i32p, i32p, f32p,
                                              C.c_int64, C.POINTER(C.c_int64)]),
    "rs_hip_coverage_create": (C.c_void_p, [f32p, f32p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_float]),
    "rs_hip_coverage_destroy": (None, [C.c_void_p]),
    "rs_hip_coverage_info": (C.c_int, [C.c_void_p, i32p, f32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rs_hip_coverage_scene_grid": (C.c_int, [C.c_void_p, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]),
    "rs_hip_coverage_scores": (C.c_int, [C.c_void_p, C.c_void_p, f32p, i32p, i32p, C.c_int32, f32p, C.c_void_p]),
    "rs_hip_coverage_extensions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_coverage_lds_budget": (C.c_int32, [C.c_int32]),
    "rs_hip_coverage_extension_routes": (None, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "rs_hip_arrange_release": (C.c_int, []),
    "rs_hip_coverage_footprints": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "rs_hip_footprints_from_arrays": (C.c_void_p, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]),
    "rs_hip_footprints_destroy": (None, [C.c_void_p]),
    "rs_hip_footprints_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rs_hip_footprints_arrays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_footprints_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rs_hip_coverage_footprint_routes": (None, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "rs_hip_voxel_grid_shape": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_scene_saliency": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    "rs_hip_cloud_create_level": (C.c_void_p, [C.c_void_p, C.c_float, C.c_int32, C.c_float, i32p, C.POINTER(C.c_int32)]),
    "rs_hip_level_samples": (C.c_int, [C.c_void_p, C.c_float, C.c_int32, i32p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rs_hip_level_samples_many": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "rs_hip_cloud_create_levels_many": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_cloud_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_resample_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "rs_hip_uniform_resample": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 7),
    "rs_hip_cloud_create_resampled": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.POINTER(C.c_int64)]),
    "rs_hip_vertex_normals": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "rs_hip_cloud_create_from_mesh": (C.c_void_p, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.POINTER(C.c_int64)]),
    "rs_hip_shuffle_plan": (C.c_int, [C.c_int64, C.c_uint32, C.c_void_p]),
    "rs_hip_shuffle_permutation": (C.c_int, [C.c_int64, C.c_uint32, C.c_void_p]),
    "rs_hip_select_by_ids": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]),
    "rs_hip_merge_shuffled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_cloud_create_fused": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                               C.c_float, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "rs_hip_fuse_seconds": (None, [C.c_void_p, C.c_int32]),
    "rs_hip_shuffle_permutations": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p]),
    "rs_hip_merge_shuffled_multi": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_cloud_fuse_arrangement": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "rs_hip_split_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "rs_hip_instance_table": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "rs_hip_split_by_instance": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "rs_hip_segment_centroids": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rs_hip_scan_to_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "rs_hip_cloud_split_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "rs_hip_split_layout": (None, [C.POINTER(C.c_int32)] * 4),
    "rs_hip_split_lds_ranks": (C.c_int32, [C.c_int32]),
    "rs_hip_split_chains_form": (C.c_int32, [C.c_int32]),
    "rs_hip_split_chains_sequential": (C.c_int64, []),
    "rs_hip_split_seconds": (None, [C.c_void_p, C.c_int32]),
    "rs_hip_plane_hypotheses": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_plane_votes": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "rs_hip_detect_planes": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "rs_hip_gather_plane_inliers": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "rs_hip_relabel_walls_and_floors": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    "rs_hip_plane_votes_form": (C.c_int32, [C.c_int32]),
    "rs_hip_pose_grid_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "rs_hip_propose_poses": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                       C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_cell_best": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rs_hip_verify_marks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "rs_hip_propose_release": (C.c_int, []),
    "rs_hip_overlap_factors": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "rs_hip_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    "rs_hip_isect_lds_budget": (C.c_int32, [C.c_int32]),
    "rs_hip_isect_pairs": (None, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "rs_hip_mat4_inverse": (None, [f32p, f32p]),
    "rs_hip_sincosf_model": (None, [f32p, C.c_int64, f32p, f32p]),
    "rs_hip_mat4_mul": (None, [f32p, f32p, f32p]),
    "rs_hip_icp_estimate_pt2pl": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int32, f32p, C.POINTER(C.c_float)]),
}


class RescanHipError(RuntimeError):
    pass


class IsectShape(C.Structure):
    """rs_hip_isect_shape_t: (boundary cloud, extent cloud) of one object."""
    _fields_ = [("boundary", C.c_void_p), ("extent", C.c_void_p)]


class ProposeTrace(C.Structure):
    """rs_hip_propose_trace_t"""
    _fields_ = [("n_scored", C.c_void_p), ("n_kept", C.c_void_p), ("n_proposed", C.c_void_p)]


class Layout(C.Structure):
    """rs_hip_layout_t"""
    ARRAYS = ("cell_start", "order", "qorder", "tiles", "by_orig", "pos", "qpos", "nor", "qnor")
    _fields_ = ([("min", C.c_float * 3), ("cell", C.c_float), ("inv_cell", C.c_float), ("dims", C.c_int32 * 3),
                 ("n", C.c_int64), ("n_cells", C.c_int64), ("occupied", C.c_int64), ("extent_limit", C.c_float),
                 ("n_tiles", C.c_int32), ("has_normals", C.c_int32)] + [(k, C.c_void_p) for k in ARRAYS])


class Placement(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("object", C.c_void_p), ("radius", C.c_float)]


_lib = None


def load():
    """dlopen librescan_hip.so and attach signatures.  Raises if the extension was not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RS_HIP_LIB", LIB_PATH)       # kernel A/B experiments (tools/variant.sh)
    if not os.path.exists(path):
        raise RescanHipError(
            f"{path} is missing: build it with `python -m rescan_amd.build` "
            "(there is no CPU fallback for the hot path)")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if "RS_HIP_LIB" in os.environ:        # an A/B build of an older tree may predate an entry point
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise RescanHipError(f"librescan_hip error {rc}: {load().rs_hip_last_error().decode()}")


def init(device=0):
    _check(load().rs_hip_init(int(device)))


def set_stream(stream_handle):
    _check(load().rs_hip_set_stream(C.c_void_p(stream_handle) if stream_handle else None))


def synchronize():
    _check(load().rs_hip_synchronize())


def stream_cu_mask(bits):
    """Restrict the calling thread's stream to the CUs whose entries in `bits` (sequence of 0/1, CU 0 first) are set; None: back
    to an unrestricted stream."""
    if bits is None:
        _check(load().rs_hip_stream_cu_mask(None, 0))
        return
    b = np.asarray(bits, np.uint8)
    words = np.zeros((len(b) + 31) // 32, np.uint32)
    for k, v in enumerate(b):
        if v:
            words[k // 32] |= np.uint32(1 << (k % 32))
    _check(load().rs_hip_stream_cu_mask(words.ctypes.data, len(words)))


def get_stream():
    """The HIP stream (an integer handle) the calling thread's launches go to."""
    return load().rs_hip_get_stream()


def profile_enable(on=True):
    load().rs_hip_profile_enable(1 if on else 0)


def profile_reset():
    load().rs_hip_profile_reset()


def profile_read(name):
    n = C.c_int64(); ms = C.c_double()
    load().rs_hip_profile_read(name.encode(), C.byref(n), C.byref(ms))
    return n.value, ms.value


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


IDENTITY = np.eye(4, dtype=np.float32).ravel()


class Cloud:
    """A device-resident cloud level + its grid index (rs_hip_cloud_t)."""

    def __init__(self, pos, nor=None, cell_size=-1.0):
        """cell_size > 0: explicit grid cell; < 0 (default): from the sampling density; 0: brute-tile layout."""
        lib = load()
        pos = _f32(pos).reshape(-1, 3)
        self.n = len(pos)
        self._pos = pos
        self._nor = None if nor is None else _f32(nor).reshape(-1, 3)
        self.handle = lib.rs_hip_cloud_create(
            pos.ctypes.data_as(C.c_void_p),
            None if self._nor is None else self._nor.ctypes.data_as(C.c_void_p),
            self.n, float(cell_size))
        if not self.handle:
            raise RescanHipError("rs_hip_cloud_create failed: " + lib.rs_hip_last_error().decode())

    @classmethod
    def many(cls, clouds, cell_size=-1.0):
        """Cloud(pos, nor, cell_size) for every (pos, nor_or_None) pair of `clouds`, built together in one call
        (rs_hip_cloud_create_many): each cloud is, to the byte, what Cloud(...) makes of its pair.  cell_size: one value for all, or
        one per cloud.  Returns the list of clouds; all or nothing."""
        lib = load()
        pairs = [(_f32(p).reshape(-1, 3), None if n is None else _f32(n).reshape(-1, 3)) for p, n in clouds]
        k = len(pairs)
        cells = np.full(k, cell_size, np.float32) if np.ndim(cell_size) == 0 else np.ascontiguousarray(cell_size, np.float32).ravel()
        if len(cells) != k:
            raise ValueError("one cell size per cloud")
        pos = (C.c_void_p * max(k, 1))(*[p.ctypes.data for p, _ in pairs])
        nor = (C.c_void_p * max(k, 1))(*[None if n is None else n.ctypes.data for _, n in pairs])
        counts = np.array([len(p) for p, _ in pairs], np.int32)
        handles = (C.c_void_p * max(k, 1))()
        any_nor = any(n is not None for _, n in pairs)
        _check(lib.rs_hip_cloud_create_many(C.addressof(pos), C.addressof(nor) if any_nor else None, counts.ctypes.data, cells.ctypes.data,
                                            k, C.addressof(handles)))
        made = []
        for j, (p, n) in enumerate(pairs):
            self = cls.__new__(cls)
            self.handle = handles[j]; self.n = len(p); self._pos = p; self._nor = n
            made.append(self)
        return made

    @classmethod
    def level_of(cls, base, radius, max_n_neigh, cell_size=-1.0):
        """The level of `base` as a cloud of its own, built on the device (rs_hip_cloud_create_level).
        Returns (cloud, sample indices)."""
        lib = load()
        idx = np.zeros(max(base.n, 1), np.int32); m = C.c_int32()
        h = lib.rs_hip_cloud_create_level(base.handle, float(radius), int(max_n_neigh), float(cell_size), idx, C.byref(m))
        if not h:
            raise RescanHipError("rs_hip_cloud_create_level failed: " + lib.rs_hip_last_error().decode())
        self = cls.__new__(cls)
        self.handle = h; self.n = m.value
        idx = idx[:m.value].copy()
        self._pos = base._pos[idx]
        self._nor = None if base._nor is None else base._nor[idx]
        return self, idx

    @classmethod
    def levels_many(cls, bases, levels, cell_size=-1.0):
        """Every level of `levels` = [(radius, max_n_neigh), ...] of every base in one call (rs_hip_cloud_create_levels_many): each
        is, to the byte, what level_of(base, radius, max_n_neigh, cell_size) makes.  cell_size: one value for all, or one per level.
        Returns [[(cloud, sample indices), ...per level], ...per base]; all or nothing."""
        lib = load()
        nc, nl, radii, caps, handles, idx, ptrs = _levels_many_args(bases, levels)
        cells = np.full(nl, cell_size, np.float32) if np.ndim(cell_size) == 0 else np.ascontiguousarray(cell_size, np.float32).ravel()
        if len(cells) != nl:
            raise ValueError("one cell size per level")
        made = (C.c_void_p * max(1, nc * nl))()
        counts = np.zeros(max(1, nc * nl), np.int32)
        _check(lib.rs_hip_cloud_create_levels_many(C.addressof(handles), nc, radii.ctypes.data, caps.ctypes.data, cells.ctypes.data, nl,
                                                   C.addressof(made), C.addressof(ptrs), counts.ctypes.data))
        out = []
        for c, base in enumerate(bases):
            row = []
            for l in range(nl):
                p = c * nl + l
                self = cls.__new__(cls)
                ind = idx[p][:counts[p]].copy()
                self.handle = made[p]; self.n = int(counts[p])
                self._pos = base._pos[ind]
                self._nor = None if base._nor is None else base._nor[ind]
                row.append((self, ind))
            out.append(row)
        return out

    @classmethod
    def resampled(cls, pos, nor, faces, cell_size=-1.0):
        """The level-0 cloud of a mesh (rs_pointcloud_uniform_resample), sampled and indexed on the device
        (rs_hip_cloud_create_resampled).  nor may be None."""
        lib = load()
        pos = _f32(pos).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        nor = None if nor is None else _f32(nor).reshape(-1, 3)
        n = C.c_int64()
        h = lib.rs_hip_cloud_create_resampled(pos.ctypes.data, None if nor is None else nor.ctypes.data, len(pos),
                                              faces.ctypes.data, len(faces), float(cell_size), C.byref(n))
        if not h:
            raise RescanHipError("rs_hip_cloud_create_resampled failed: " + lib.rs_hip_last_error().decode())
        self = cls.__new__(cls)
        self.handle = h; self.n = n.value
        self._pos = np.zeros((self.n, 3), np.float32)
        self._nor = None if nor is None else np.zeros((self.n, 3), np.float32)
        _check(lib.rs_hip_cloud_points(h, self._pos.ctypes.data, None if nor is None else self._nor.ctypes.data))
        return self

    @classmethod
    def from_mesh(cls, pos, faces, cell_size=-1.0):
        """The level-0 cloud of a mesh that comes without normals (rs_hip_cloud_create_from_mesh): vertex normals from the faces
        with the loader's pass (vertex_normals(.., loader_pass=True)), then what resampled() does with them, all on the device."""
        lib = load()
        pos = _f32(pos).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        n = C.c_int64()
        h = lib.rs_hip_cloud_create_from_mesh(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces), float(cell_size), C.byref(n))
        if not h:
            raise RescanHipError("rs_hip_cloud_create_from_mesh failed: " + lib.rs_hip_last_error().decode())
        self = cls.__new__(cls)
        self.handle = h; self.n = n.value
        self._pos = np.zeros((self.n, 3), np.float32); self._nor = np.zeros((self.n, 3), np.float32)
        _check(lib.rs_hip_cloud_points(h, self._pos.ctypes.data, self._nor.ctypes.data))
        return self

    @classmethod
    def fused(cls, scan, scan_instance_ids, uidx, model, pose, refine=True, max_dist=0.05, max_angle=np.float32(10.0 * 0.005555555556 * np.pi),
              cell_size=-1.0):
        """One placement of rsdu_augment_database on the device (rs_hip_cloud_create_fused): the scan's points with instance id
        uidx, aligned to `model` from inverse(pose) when refine, moved into the model's frame, merged with it and shuffled.
        Returns (cloud, info) with info = dict(xform, icp_err, source, scan_index, n_extracted); source[i] < n_extracted names
        extracted point source[i] (scan point scan_index[source[i]]), otherwise model point source[i] - n_extracted.
        (None, info) when no point carries uidx."""
        lib = load()
        ids = np.ascontiguousarray(scan_instance_ids, np.int32).ravel()
        if len(ids) != scan.n:
            raise ValueError("scan_instance_ids: one entry per scan point")
        pose = _f32(pose).ravel()
        xform = np.zeros(16, np.float32); err = C.c_float(); n_ext = C.c_int64()
        source = np.zeros(scan.n + model.n, np.int32); scan_index = np.zeros(max(scan.n, 1), np.int32)
        h = lib.rs_hip_cloud_create_fused(scan.handle, ids.ctypes.data, int(uidx), model.handle, pose.ctypes.data, int(bool(refine)),
                                          float(max_dist), float(max_angle), float(cell_size), xform.ctypes.data, C.byref(err),
                                          source.ctypes.data, scan_index.ctypes.data, C.byref(n_ext))
        na = n_ext.value
        info = dict(xform=xform, icp_err=err.value, source=source[:na + model.n if h else 0].copy(), scan_index=scan_index[:na].copy(),
                    n_extracted=na)
        if not h:
            msg = lib.rs_hip_last_error().decode()
            if msg:
                raise RescanHipError("rs_hip_cloud_create_fused failed: " + msg)
            return None, info
        self = cls.__new__(cls)
        self.handle = h; self.n = na + model.n
        self._pos = np.zeros((self.n, 3), np.float32); self._nor = np.zeros((self.n, 3), np.float32)
        _check(lib.rs_hip_cloud_points(h, self._pos.ctypes.data, self._nor.ctypes.data))
        return self, info

    @classmethod
    def fuse_arrangement(cls, scan, scan_instance_ids, placements, max_dist=0.05, max_angle=np.float32(10.0 * 0.005555555556 * np.pi), cell_size=-1.0):
        """rsdu_augment_database's loop over all placements of an arrangement in one call (rs_hip_cloud_fuse_arrangement).
        placements: dicts with uidx, pose, and model (a Cloud) or model_from (the index of an earlier placement whose resulting
        shape is the model; default -1: `model`); refine defaults to True.  Returns one (cloud, info) per placement, exactly what
        Cloud.fused returns for it alone given the same model; (None, info) where no scan point carries the uidx."""
        lib = load()
        ids = np.ascontiguousarray(scan_instance_ids, np.int32).ravel()
        if len(ids) != scan.n:
            raise ValueError("scan_instance_ids: one entry per scan point")
        P = len(placements)
        recs = (FusePlacement * max(P, 1))(); outs = (FuseResult * max(P, 1))()
        keep, sources, indices, n_model, n_shape, counts = [], [], [], [], [], {}
        for p, pl in enumerate(placements):
            frm = int(pl.get("model_from", -1)); model = pl.get("model")
            pose = _f32(pl["pose"]).ravel()
            recs[p].uidx = int(pl["uidx"]); recs[p].refine = int(bool(pl.get("refine", True))); recs[p].model_from = frm
            recs[p].model = model.handle if (frm == -1 and model is not None) else None
            recs[p].pose[:] = pose.tolist()
            keep.append(model)
            # the sizes follow from the ids alone; they only size the arrays handed in (the library judges the arguments itself)
            if recs[p].uidx not in counts:
                counts[recs[p].uidx] = int(np.count_nonzero(ids == recs[p].uidx))
            n_ext = counts[recs[p].uidx]
            nm = (model.n if model is not None else 0) if not 0 <= frm < p else n_shape[frm]
            n_model.append(nm); n_shape.append(n_ext + nm if n_ext else nm)
            sources.append(np.zeros(max(n_ext + nm, 1), np.int32)); indices.append(np.zeros(max(n_ext, 1), np.int32))
            outs[p].source = sources[p].ctypes.data; outs[p].scan_index = indices[p].ctypes.data
        _check(lib.rs_hip_cloud_fuse_arrangement(scan.handle, ids.ctypes.data, C.addressof(recs), P, float(max_dist), float(max_angle), float(cell_size),
                                                 C.addressof(outs)))
        made = []
        for p in range(P):
            na = int(outs[p].n_extracted); h = outs[p].cloud
            info = dict(xform=np.array(outs[p].xform[:], np.float32), icp_err=float(outs[p].icp_err), source=sources[p][:na + n_model[p] if h else 0].copy(),
                        scan_index=indices[p][:na].copy(), n_extracted=na)
            cloud = None
            if h:
                cloud = cls.__new__(cls)
                cloud.handle = h; cloud.n = na + n_model[p]
                cloud._pos = np.zeros((cloud.n, 3), np.float32); cloud._nor = np.zeros((cloud.n, 3), np.float32)
            made.append((cloud, info))
        for cloud, _ in made:
            if cloud is not None:
                _check(lib.rs_hip_cloud_points(cloud.handle, cloud._pos.ctypes.data, cloud._nor.ctypes.data))
        return made

    def split_objects(self, class_ids, instance_ids, static_classes=(), cell_size=-1.0):
        """seg2rsdb's pointcloud_to_rsdb on this level-0 cloud with normals (rs_hip_cloud_split_objects): one indexed cloud per
        instance, in order of first appearance, the dynamic ones centred; the points never visit the host on the way.  Returns
        (clouds, info), info as split_plan() returns it without out_pos / out_nor."""
        lib = load()
        cls = np.ascontiguousarray(class_ids, np.int32).ravel(); ids = np.ascontiguousarray(instance_ids, np.int32).ravel()
        if len(cls) != self.n or len(ids) != self.n:
            raise ValueError("one class id and instance id per point")
        static = np.ascontiguousarray(static_classes, np.int32).ravel()
        handles = (C.c_void_p * _split_room(self.n))()
        info = _split_call(lib.rs_hip_cloud_split_objects, self.n, False, False, self.handle, cls.ctypes.data, ids.ctypes.data,
                           static.ctypes.data if len(static) else None, len(static), float(cell_size), C.addressof(handles))
        clouds = []
        for k in range(info["n_instances"]):
            c = Cloud.__new__(Cloud)
            c.handle = handles[k]; c.n = int(info["counts"][k])
            c._pos = np.zeros((c.n, 3), np.float32); c._nor = np.zeros((c.n, 3), np.float32)
            clouds.append(c)
        for c in clouds:
            _check(lib.rs_hip_cloud_points(c.handle, c._pos.ctypes.data, c._nor.ctypes.data))
        return clouds, info

    def detect_planes(self, dot_threshold=0.8, dist_threshold=0.033, count_threshold=250, floor_iters=2500, wall_iters=5000, capacity=64,
                      trace=False):
        """rspf__detect_floor then rspf__detect_walls on this cloud (the reference: level 2), see detect_planes()."""
        return detect_planes(self, dot_threshold, dist_threshold, count_threshold, floor_iters, wall_iters, capacity, trace)

    def layout(self):
        """The two layouts as the build left them (rs_hip_cloud_layout): a dict of the scalars min, cell, inv_cell, dims, n, n_cells,
        occupied, extent_limit, n_tiles and the arrays cell_start, order, qorder, tiles, by_orig, pos, qpos — the records as (n, 4)
        uint32 — with nor and qnor for a cloud with normals."""
        lib = load()
        L = Layout()
        _check(lib.rs_hip_cloud_layout(self.handle, C.addressof(L)))
        n, dt = int(L.n), {"order": np.int32, "qorder": np.int32, "by_orig": np.int32}
        shapes = dict(cell_start=(L.n_cells + 1,), order=(n,), qorder=(n,), tiles=(L.n_tiles + 1,), by_orig=(n,), pos=(n, 4), qpos=(n, 4))
        if L.has_normals:
            shapes.update(nor=(n, 4), qnor=(n, 4))
        out = {k: np.zeros(shape, dt.get(k, np.uint32)) for k, shape in shapes.items()}
        for k, a in out.items():
            setattr(L, k, a.ctypes.data)
        _check(lib.rs_hip_cloud_layout(self.handle, C.addressof(L)))
        out.update(min=np.array(L.min[:], np.float32), cell=np.float32(L.cell), inv_cell=np.float32(L.inv_cell), dims=np.array(L.dims[:], np.int32),
                   n=n, n_cells=int(L.n_cells), occupied=int(L.occupied), extent_limit=np.float32(L.extent_limit), n_tiles=int(L.n_tiles))
        return out

    @property
    def n_tiles(self):
        """query tiles of the cloud (rs_hip_cloud_tiles): what one wave of a search takes"""
        return int(load().rs_hip_cloud_tiles(self.handle))

    @property
    def nbytes(self):
        return load().rs_hip_cloud_bytes(self.handle)

    def close(self):
        if getattr(self, "handle", None):
            load().rs_hip_cloud_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def radius_search(target, query, radius, k):
    """msh_hash_grid_radius_search: rows of the k nearest within radius, ascending."""
    query = _f32(query).reshape(-1, 3)
    nq = len(query)
    d = np.zeros((nq, k), np.float32); i = np.zeros((nq, k), np.int32); nn = np.zeros(nq, np.uint64)
    tot = C.c_uint64()
    _check(load().rs_hip_radius_search(target.handle, query, nq, float(radius), int(k), d, i, nn, C.byref(tot)))
    return d, i, nn.astype(np.int64), tot.value


def resample_plan(pos, faces, table=True):
    """The host part of the mesh resampler (rs_hip_resample_plan; no device needed): (n_samples, total_area, prob, alias), the
    last two None when table is False."""
    pos = _f32(pos).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n, total = C.c_int64(), C.c_double()
    prob = np.zeros(len(faces), np.float64) if table else None
    alias = np.zeros(len(faces), np.int32) if table else None
    _check(load().rs_hip_resample_plan(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces), C.byref(n), C.byref(total),
                                       prob.ctypes.data if table else None, alias.ctypes.data if table else None))
    return n.value, total.value, prob, alias


def vertex_normals(pos, faces, loader_pass=False, counts=False):
    """rs_pointcloud__compute_normals on the device (rs_hip_vertex_normals): the (n, 3) vertex normals of a mesh from its faces;
    loader_pass adds rs_pointcloud__load_ply's pass over them.  counts: also the number of corners that name each vertex."""
    pos = _f32(pos).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nor = np.zeros((len(pos), 3), np.float32)
    cnt = np.zeros(len(pos), np.int32) if counts else None
    _check(load().rs_hip_vertex_normals(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces), int(bool(loader_pass)), nor.ctypes.data,
                                        cnt.ctypes.data if counts else None))
    return (nor, cnt) if counts else nor


def uniform_resample(pos, faces, nor=None, col=None, radii=None, class_ids=None, instance_ids=None, first=0, count=None):
    """rs_pointcloud_uniform_resample on the device: samples first .. first + count - 1 of the reference's sequence (count None: to
    the end).  Returns a dict: n_samples, pos, face, and nor / col / radii / class_ids / instance_ids for the attributes given."""
    pos = _f32(pos).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n_samples = resample_plan(pos, faces, table=False)[0]
    if count is None:
        count = n_samples - first
    ins = dict(nor=None if nor is None else _f32(nor).reshape(-1, 3), col=None if col is None else _f32(col).reshape(-1, 3),
               radii=None if radii is None else _f32(radii).ravel(),
               class_ids=None if class_ids is None else np.ascontiguousarray(class_ids, np.int32).ravel(),
               instance_ids=None if instance_ids is None else np.ascontiguousarray(instance_ids, np.int32).ravel())
    m = max(int(count), 0)
    out = dict(n_samples=n_samples, pos=np.zeros((m, 3), np.float32), face=np.zeros(m, np.int32))
    for k, v in ins.items():
        if v is not None:
            if len(v) != len(pos):
                raise ValueError(f"{k}: one entry per vertex")
            out[k] = np.zeros((m, 3), np.float32) if v.ndim == 2 else np.zeros(m, v.dtype)
    ptr = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    _check(load().rs_hip_uniform_resample(pos.ctypes.data, *[ptr(ins[k]) for k in ("nor", "col", "radii", "class_ids", "instance_ids")],
                                          len(pos), faces.ctypes.data, len(faces), int(first), int(count), out["pos"].ctypes.data,
                                          *[ptr(out.get(k)) for k in ("nor", "col", "radii", "class_ids", "instance_ids")],
                                          out["face"].ctypes.data))
    return out


SEED_MERGE = 12346      # rs_pointcloud_merge's shuffle (lib/rs/rs_pointcloud.h:428)


def shuffle_plan(n, seed=SEED_MERGE):
    """The permutation of rs_pointcloud_merge's shuffle over n elements, by the reference's loop on the host
    (rs_hip_shuffle_plan; no device needed): perm[i] = the index in "A then B" of the element that ends at i."""
    perm = np.zeros(max(int(n), 0), np.int32)
    _check(load().rs_hip_shuffle_plan(int(n), int(seed), perm.ctypes.data))
    return perm


def shuffle_permutation(n, seed=SEED_MERGE):
    """The same permutation made on the device (rs_hip_shuffle_permutation)."""
    perm = np.zeros(max(int(n), 0), np.int32)
    _check(load().rs_hip_shuffle_permutation(int(n), int(seed), perm.ctypes.data))
    return perm


def select_by_ids(point_ids, ids):
    """rs_pointcloud_copy_by_ids' selection (rs_hip_select_by_ids): the indices i, increasing, with point_ids[i] in ids."""
    point_ids = np.ascontiguousarray(point_ids, np.int32).ravel(); ids = np.ascontiguousarray(ids, np.int32).ravel()
    index = np.zeros(max(len(point_ids), 1), np.int32); count = C.c_int64()
    _check(load().rs_hip_select_by_ids(point_ids.ctypes.data, len(point_ids), ids.ctypes.data, len(ids), index.ctypes.data, C.byref(count)))
    return index[:count.value].copy()


def merge_shuffled(a_pos, a_nor, xform, b_pos, b_nor, seed=SEED_MERGE):
    """rs_pointcloud_transform of A by xform, then rs_pointcloud_merge( A, B ) (rs_hip_merge_shuffled): (pos, nor, source)."""
    a_pos = _f32(a_pos).reshape(-1, 3); a_nor = _f32(a_nor).reshape(-1, 3); b_pos = _f32(b_pos).reshape(-1, 3); b_nor = _f32(b_nor).reshape(-1, 3)
    if len(a_nor) != len(a_pos) or len(b_nor) != len(b_pos):
        raise ValueError("one normal per point")
    xform = _f32(xform).ravel()
    n = len(a_pos) + len(b_pos)
    pos = np.zeros((n, 3), np.float32); nor = np.zeros((n, 3), np.float32); source = np.zeros(n, np.int32)
    _check(load().rs_hip_merge_shuffled(a_pos.ctypes.data, a_nor.ctypes.data, len(a_pos), xform.ctypes.data, b_pos.ctypes.data, b_nor.ctypes.data,
                                        len(b_pos), int(seed), pos.ctypes.data, nor.ctypes.data, source.ctypes.data))
    return pos, nor, source


def fuse_seconds(enable=True):
    """rs_hip_fuse_seconds: (extraction, ICP, permutation, merge, index build) seconds of Cloud.fused on this thread since the
    last call; enable: whether the next calls keep the clock."""
    out = np.zeros(5, np.float64)
    load().rs_hip_fuse_seconds(out.ctypes.data, int(bool(enable)))
    return out


class FusePlacement(C.Structure):
    """rs_hip_fuse_placement_t"""
    _fields_ = [("uidx", C.c_int32), ("refine", C.c_int32), ("model_from", C.c_int32), ("reserved", C.c_int32), ("model", C.c_void_p), ("pose", C.c_float * 16)]


class FuseResult(C.Structure):
    """rs_hip_fuse_result_t"""
    _fields_ = [("cloud", C.c_void_p), ("n_extracted", C.c_int64), ("xform", C.c_float * 16), ("icp_err", C.c_float), ("reserved", C.c_int32),
                ("source", C.c_void_p), ("scan_index", C.c_void_p)]


def shuffle_permutations(sizes, seed=SEED_MERGE):
    """The permutations of len(sizes) independent shuffles in one device pass (rs_hip_shuffle_permutations), concatenated; each
    slice holds local indices: the slice of placement p equals shuffle_plan(sizes[p], seed)."""
    n = np.ascontiguousarray(sizes, np.int64).ravel()
    perm = np.zeros(max(int(n.clip(min=0).sum()), 0) if len(n) else 0, np.int32)
    _check(load().rs_hip_shuffle_permutations(n.ctypes.data if len(n) else None, len(n), int(seed), perm.ctypes.data if len(perm) else None))
    return perm


def merge_shuffled_multi(parts, seed=SEED_MERGE):
    """merge_shuffled for every (a_pos, a_nor, xform, b_pos, b_nor) of parts in one permutation pass and one merge launch
    (rs_hip_merge_shuffled_multi): a list of (pos, nor, source), one per part."""
    P = len(parts)
    arrays = [[_f32(x).reshape(-1, 3) for x in (a_pos, a_nor, b_pos, b_nor)] for a_pos, a_nor, _, b_pos, b_nor in parts]
    for a_pos, a_nor, b_pos, b_nor in arrays:
        if len(a_nor) != len(a_pos) or len(b_nor) != len(b_pos):
            raise ValueError("one normal per point")
    xforms = np.ascontiguousarray(np.stack([_f32(x[2]).ravel() for x in parts]) if P else np.zeros((0, 16)), np.float32)
    n_a = np.array([len(a[0]) for a in arrays], np.int64); n_b = np.array([len(a[2]) for a in arrays], np.int64)
    ptrs = [(C.c_void_p * max(P, 1))(*[a[k].ctypes.data if len(a[k]) else None for a in arrays]) for k in range(4)]
    sizes = n_a + n_b; total = int(sizes.sum())
    pos = np.zeros((total, 3), np.float32); nor = np.zeros((total, 3), np.float32); source = np.zeros(total, np.int32)
    _check(load().rs_hip_merge_shuffled_multi(P, C.addressof(ptrs[0]), C.addressof(ptrs[1]), n_a.ctypes.data, xforms.ctypes.data, C.addressof(ptrs[2]),
                                              C.addressof(ptrs[3]), n_b.ctypes.data, int(seed), pos.ctypes.data if total else None,
                                              nor.ctypes.data if total else None, source.ctypes.data if total else None))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return [(pos[off[p]:off[p + 1]], nor[off[p]:off[p + 1]], source[off[p]:off[p + 1]]) for p in range(P)]


class SplitOut(C.Structure):
    """rs_hip_split_out_t"""
    _fields_ = [(k, C.c_void_p) for k in ("n_instances", "inst_ids", "counts", "first", "offsets", "order", "class_of", "is_static", "sums",
                                          "centroids", "xforms", "poses", "out_pos", "out_nor")]


def split_layout():
    """rs_hip_split_layout: dict(tile, lds_ranks, max_instances, chain_block)."""
    v = [C.c_int32() for _ in range(4)]
    load().rs_hip_split_layout(*[C.byref(x) for x in v])
    return dict(tile=v[0].value, lds_ranks=v[1].value, max_instances=v[2].value, chain_block=v[3].value)


def split_lds_ranks(ranks=-1):
    """The largest instance count of the partition's LDS route (rs_hip_split_lds_ranks; 0 forces the sort route); returns the previous."""
    return load().rs_hip_split_lds_ranks(int(ranks))


def split_chains_form(form=-1):
    """0: the centroid chains' block step, 1: a lone lane per chain (rs_hip_split_chains_form); returns the previous."""
    return load().rs_hip_split_chains_form(int(form))


def split_chains_sequential():
    """Addends the centroid chains of the last call added one by one (rs_hip_split_chains_sequential)."""
    return load().rs_hip_split_chains_sequential()


def split_seconds(enable=True):
    """rs_hip_split_seconds: (table, partition, chains, transform, index builds) seconds of scan_to_objects / Cloud.split_objects on
    this thread since the last call; enable: whether the next calls keep the clock."""
    out = np.zeros(5, np.float64)
    load().rs_hip_split_seconds(out.ctypes.data, int(bool(enable)))
    return out


def _split_room(n):
    return min(max(int(n), 1), split_layout()["max_instances"])


def instance_table(instance_ids):
    """The distinct instance ids in order of first appearance, on the device (rs_hip_instance_table): (inst_ids, counts, first)."""
    ids = np.ascontiguousarray(instance_ids, np.int32).ravel()
    m = _split_room(len(ids))
    inst = np.zeros(m, np.int32); counts = np.zeros(m, np.int64); first = np.zeros(m, np.int64); k = C.c_int32()
    _check(load().rs_hip_instance_table(ids.ctypes.data, len(ids), inst.ctypes.data, counts.ctypes.data, first.ctypes.data, C.byref(k)))
    return inst[:k.value].copy(), counts[:k.value].copy(), first[:k.value].copy()


def split_by_instance(instance_ids):
    """The stable multiway partition of a scan by instance id, on the device (rs_hip_split_by_instance): (inst_ids, offsets, order)."""
    ids = np.ascontiguousarray(instance_ids, np.int32).ravel()
    m = _split_room(len(ids))
    inst = np.zeros(m, np.int32); offsets = np.zeros(m + 1, np.int64); order = np.zeros(max(len(ids), 1), np.int32); k = C.c_int32()
    _check(load().rs_hip_split_by_instance(ids.ctypes.data, len(ids), inst.ctypes.data, offsets.ctypes.data, order.ctypes.data, C.byref(k)))
    return inst[:k.value].copy(), offsets[:k.value + 1].copy(), order[:len(ids)].copy()


def segment_centroids(pos, order, offsets):
    """rs_pointcloud_centroid's sequential fp64 chains per segment, on the device (rs_hip_segment_centroids): (sums, centroids), each
    (n_instances, 3); the centroids before y = 0."""
    pos = _f32(pos).reshape(-1, 3); order = np.ascontiguousarray(order, np.int32).ravel(); offsets = np.ascontiguousarray(offsets, np.int64).ravel()
    k = max(len(offsets) - 1, 0)
    sums = np.zeros((k, 3), np.float64); cen = np.zeros((k, 3), np.float32)
    _check(load().rs_hip_segment_centroids(pos.ctypes.data, len(pos), order.ctypes.data, offsets.ctypes.data, k, sums.ctypes.data, cen.ctypes.data))
    return sums, cen


def _split_call(fn, n, with_points, with_normals, *args):
    """Allocates every array of rs_hip_split_out_t for n points, calls fn( *args, out ) and trims the arrays to the instances found."""
    m = _split_room(n)
    k = C.c_int32()
    a = dict(inst_ids=np.zeros(m, np.int32), counts=np.zeros(m, np.int64), first=np.zeros(m, np.int64), offsets=np.zeros(m + 1, np.int64),
             order=np.zeros(max(n, 1), np.int32), class_of=np.zeros(m, np.int32), is_static=np.zeros(m, np.int32), sums=np.zeros((m, 3), np.float64),
             centroids=np.zeros((m, 3), np.float32), xforms=np.zeros((m, 16), np.float32), poses=np.zeros((m, 16), np.float32))
    if with_points:
        a["out_pos"] = np.zeros((max(n, 1), 3), np.float32)
    if with_normals:
        a["out_nor"] = np.zeros((max(n, 1), 3), np.float32)
    out = SplitOut(n_instances=C.addressof(k), **{key: v.ctypes.data for key, v in a.items()})
    _check(fn(*args, C.addressof(out)))
    i = k.value
    r = {key: (v[:n] if key in ("order", "out_pos", "out_nor") else v[:i + 1] if key == "offsets" else v[:i]).copy() for key, v in a.items()}
    r["n_instances"] = i
    return r


def _split_inputs(pos, nor, class_ids, instance_ids, static_classes):
    pos = _f32(pos).reshape(-1, 3)
    nor = None if nor is None else _f32(nor).reshape(-1, 3)
    cls = np.ascontiguousarray(class_ids, np.int32).ravel(); ids = np.ascontiguousarray(instance_ids, np.int32).ravel()
    if len(cls) != len(pos) or len(ids) != len(pos) or (nor is not None and len(nor) != len(pos)):
        raise ValueError("one class id, instance id and normal per point")
    static = np.ascontiguousarray(static_classes, np.int32).ravel()
    return pos, nor, cls, ids, static


def split_plan(pos, nor, class_ids, instance_ids, static_classes=()):
    """seg2rsdb's pointcloud_to_rsdb by the reference's loops on the host (rs_hip_split_plan; no device needed): a dict of
    n_instances, inst_ids, counts, first, offsets, order, class_of, is_static, sums, centroids (y = 0), xforms, poses, out_pos and,
    with normals, out_nor."""
    pos, nor, cls, ids, static = _split_inputs(pos, nor, class_ids, instance_ids, static_classes)
    return _split_call(load().rs_hip_split_plan, len(pos), True, nor is not None, pos.ctypes.data, None if nor is None else nor.ctypes.data,
                       cls.ctypes.data, ids.ctypes.data, len(pos), static.ctypes.data if len(static) else None, len(static))


def scan_to_objects(pos, nor, class_ids, instance_ids, static_classes=()):
    """The same on the device end to end (rs_hip_scan_to_objects)."""
    pos, nor, cls, ids, static = _split_inputs(pos, nor, class_ids, instance_ids, static_classes)
    return _split_call(load().rs_hip_scan_to_objects, len(pos), True, nor is not None, pos.ctypes.data, None if nor is None else nor.ctypes.data,
                       cls.ctypes.data, ids.ctypes.data, len(pos), static.ctypes.data if len(static) else None, len(static))


KNN_MAX_K = 64          # RS_HIP_KNN_MAX_K


SEED_PLANES = 12346     # rspf__detect_floor / rspf__detect_walls (lib/rs/rs_pointcloud_filters.cpp:154,217)


class PlaneTrace(C.Structure):
    """rs_hip_plane_trace_t"""
    _fields_ = [("capacity_rounds", C.c_int32), ("max_iters", C.c_int32), ("n_rounds", C.c_int32), ("idx", C.c_void_p), ("valid", C.c_void_p),
                ("counts", C.c_void_p), ("best", C.c_void_p), ("n_iters", C.c_void_p), ("mask_before", C.c_void_p), ("mask_after", C.c_void_p)]


def plane_hypotheses(pos, active, n_iter, distinct, seed=SEED_PLANES):
    """One RANSAC round's sampling on the host (rs_hip_plane_hypotheses; no device needed): (idx (n_iter, 3), center, normal)."""
    pos = _f32(pos).reshape(-1, 3); active = np.ascontiguousarray(active, np.uint8).ravel()
    if len(active) != len(pos):
        raise ValueError("active: one entry per point")
    idx = np.zeros((n_iter, 3), np.int32); center = np.zeros((n_iter, 3), np.float32); normal = np.zeros((n_iter, 3), np.float32)
    _check(load().rs_hip_plane_hypotheses(pos.ctypes.data, len(pos), active.ctypes.data, int(n_iter), int(bool(distinct)), int(seed),
                                          idx.ctypes.data, center.ctypes.data, normal.ctypes.data))
    return idx, center, normal


def plane_votes(pos, active, center, normal, dist_threshold, valid=None):
    """evaluate_plane_model for every hypothesis at once (rs_hip_plane_votes): int32 counts, 0 where valid[h] == 0."""
    pos = _f32(pos).reshape(-1, 3); active = np.ascontiguousarray(active, np.uint8).ravel()
    center = _f32(center).reshape(-1, 3); normal = _f32(normal).reshape(-1, 3)
    if len(active) != len(pos) or len(center) != len(normal):
        raise ValueError("active: one entry per point; center and normal: one row per hypothesis")
    valid = None if valid is None else np.ascontiguousarray(valid, np.uint8).ravel()
    counts = np.zeros(len(center), np.int32)
    _check(load().rs_hip_plane_votes(pos.ctypes.data, len(pos), active.ctypes.data, center.ctypes.data, normal.ctypes.data,
                                     None if valid is None else valid.ctypes.data, len(center), float(dist_threshold), counts.ctypes.data))
    return counts


def plane_votes_form(form=-1):
    """rs_hip_plane_votes_form: 0 the LDS tile (default), 1 wave-uniform global loads; < 0 only reads.  Returns the previous form."""
    return load().rs_hip_plane_votes_form(int(form))


def detect_planes(cloud, dot_threshold=0.8, dist_threshold=0.033, count_threshold=250, floor_iters=2500, wall_iters=5000, capacity=64,
                  trace=False, trace_rounds=32):
    """rs_hip_detect_planes: dict(centers, normals, n_inliers, n_floors, n_walls) and, with trace, trace = dict(n_rounds, idx, valid,
    counts, best, n_iters, mask_before, mask_after), one leading entry per recorded round (round 0: the floor)."""
    centers = np.zeros((capacity, 3), np.float32); normals = np.zeros((capacity, 3), np.float32); n_inl = np.zeros(capacity, np.int64)
    nf, nw, nm = C.c_int32(), C.c_int32(), C.c_int32()
    t = None
    if trace:
        mi = max(int(floor_iters), int(wall_iters), 1); r = int(trace_rounds)
        arrays = dict(idx=np.zeros((r, mi, 3), np.int32), valid=np.zeros((r, mi), np.uint8), counts=np.zeros((r, mi), np.int32),
                      best=np.full(r, -2, np.int32), n_iters=np.zeros(r, np.int32), mask_before=np.zeros((r, cloud.n), np.uint8),
                      mask_after=np.zeros((r, cloud.n), np.uint8))
        t = PlaneTrace(r, mi, 0, *[arrays[k].ctypes.data for k in ("idx", "valid", "counts", "best", "n_iters", "mask_before", "mask_after")])
    _check(load().rs_hip_detect_planes(cloud.handle, float(dot_threshold), float(dist_threshold), int(count_threshold), int(floor_iters),
                                       int(wall_iters), int(capacity), centers.ctypes.data, normals.ctypes.data, n_inl.ctypes.data,
                                       C.byref(nf), C.byref(nw), C.byref(nm), C.addressof(t) if t is not None else None))
    m = nm.value
    out = dict(centers=centers[:m].copy(), normals=normals[:m].copy(), n_inliers=n_inl[:m].copy(), n_floors=nf.value, n_walls=nw.value)
    if trace:
        k = min(t.n_rounds, r)
        out["trace"] = dict(n_rounds=t.n_rounds, **{key: a[:k] for key, a in arrays.items()})
    return out


def _plane_models(centers, normals, axes=None, extends=None, valid=None, normal_up_dot=None):
    centers = _f32(centers).reshape(-1, 3); m = len(centers)
    normals = _f32(normals).reshape(-1, 3)
    axes = None if axes is None else _f32(axes).reshape(-1, 9)
    extends = None if extends is None else _f32(extends).reshape(-1, 4)
    valid = None if valid is None else np.ascontiguousarray(valid, np.int8).ravel()
    up = None if normal_up_dot is None else _f32(normal_up_dot).ravel()
    for a in (normals, axes, extends, valid, up):
        if a is not None and len(a) != m:
            raise ValueError("plane models: every array has one row per model")
    return m, [None if a is None else a.ctypes.data for a in (centers, normals, axes, extends, valid, up)], (centers, normals, axes, extends, valid, up)


def gather_plane_inliers(cloud, centers, normals, axes=None, extends=None, valid=None, dot_threshold=0.8, dist_threshold=0.05,
                         check_validity=False, check_extends=False):
    """rspf__gather_model_inliers (rs_hip_gather_plane_inliers): a list with one increasing int32 index array per model.  axes: (M, 9)
    column-major, extends (M, 4), valid (M,)."""
    m, ptrs, keep = _plane_models(centers, normals, axes, extends, valid)
    lib = load()
    offsets = np.zeros(m + 1, np.int64)
    capacity = max(cloud.n, 1)
    while True:
        index = np.zeros(capacity, np.int32)
        rc = lib.rs_hip_gather_plane_inliers(cloud.handle, *ptrs[:5], m, float(dot_threshold), float(dist_threshold), int(bool(check_validity)),
                                             int(bool(check_extends)), index.ctypes.data, capacity, offsets.ctypes.data)
        if rc == -4 and capacity < m * max(cloud.n, 1) and b"capacity" in lib.rs_hip_last_error():
            capacity = m * max(cloud.n, 1)
            continue
        _check(rc)
        return [index[offsets[k]:offsets[k + 1]].copy() for k in range(m)]


def relabel_walls_and_floors(cloud, centers, normals, axes, extends, valid, normal_up_dot, floor_idx, wall_idx, unlabelled_idx, class_ids, instance_ids):
    """rspf_relabel_walls_and_floors on a level-1 cloud (rs_hip_relabel_walls_and_floors): the rewritten (class_ids, instance_ids)."""
    m, ptrs, keep = _plane_models(centers, normals, axes, extends, valid, normal_up_dot)
    cls = np.array(class_ids, np.int32).ravel(); inst = np.array(instance_ids, np.int32).ravel()
    if len(cls) != cloud.n or len(inst) != cloud.n:
        raise ValueError("class_ids, instance_ids: one entry per point")
    _check(load().rs_hip_relabel_walls_and_floors(cloud.handle, *ptrs, m, int(floor_idx), int(wall_idx), int(unlabelled_idx), cls.ctypes.data, inst.ctypes.data))
    return cls, inst


class KnnGrid:
    """msh_hash_grid_knn_search's own grid (geometry from the init radius) over a device cloud's points (rs_hip_knn_grid_t).
    dim = 2: a cloud of (x, y, 0) points, as msh_hash_grid_init_2d keeps them."""

    def __init__(self, cloud, radius, dim=3):
        lib = load()
        self.dim = int(dim)
        self.handle = lib.rs_hip_knn_grid_create(cloud.handle, float(radius), self.dim)
        if not self.handle:
            raise RescanHipError("rs_hip_knn_grid_create failed: " + lib.rs_hip_last_error().decode())

    def geometry(self):
        """((w, h, d), cell, min_pt) of the grid."""
        dims = np.zeros(3, np.int64); cell = C.c_double(); mn = np.zeros(3, np.float32)
        _check(load().rs_hip_knn_grid_geometry(self.handle, dims, C.byref(cell), mn))
        return tuple(int(x) for x in dims), cell.value, mn

    def close(self):
        if getattr(self, "handle", None):
            load().rs_hip_knn_grid_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def knn_geometry(points, radius, dim=3):
    """The k-NN grid's ((w, h, d), cell, min_pt) for these points, computed on the host (no device needed)."""
    pts = _f32(points).reshape(-1, 3)
    dims = np.zeros(3, np.int64); cell = C.c_double(); mn = np.zeros(3, np.float32)
    _check(load().rs_hip_knn_geometry(pts, len(pts), float(radius), int(dim), dims, C.byref(cell), mn))
    return tuple(int(x) for x in dims), cell.value, mn


def knn_search(grid, query, k):
    """msh_hash_grid_knn_search: the reference's k-NN rows (k <= KNN_MAX_K), ascending; entries past a row's count are 0.
    Returns (d², idx, n_neighbors, total) like radius_search."""
    query = _f32(query).reshape(-1, 3)
    nq = len(query)
    d = np.zeros((nq, k), np.float32); i = np.zeros((nq, k), np.int32); nn = np.zeros(nq, np.uint64)
    tot = C.c_uint64()
    _check(load().rs_hip_knn_search(grid.handle, query, nq, int(k), d, i, nn, C.byref(tot)))
    return d, i, nn.astype(np.int64), tot.value


def profile_marker():
    """A named no-op kernel on the calling thread's stream (marks a step's start in a rocprofv3 kernel trace)."""
    _check(load().rs_hip_profile_marker())


def cloud_build_seconds(reset=False):
    """(diagnostics) seconds spent building clouds since the last reset: (host copy, upload + bounds, cell index, Hilbert order + tiles), clouds counted."""
    out = (C.c_double * 4)()
    n = load().rs_hip_cloud_build_seconds(out, 1 if reset else 0)
    return [float(x) for x in out], int(n)


def cloud_many_single_above(n=-1):
    """Clouds of more than n points inside a Cloud.many batch are built alone (rs_hip_cloud_many_single_above; the result is the
    same).  n < 0 only reads.  Returns the previous value."""
    return int(load().rs_hip_cloud_many_single_above(int(n)))


def switch_get(name):
    """The value the library would use now for an environment switch of its table (rescan_amd/csrc/rs_switches.h): a flag gives 0.0 or
    1.0.  Raises for a name that is not in the table.  Needs no device."""
    v = C.c_double(0.0)
    _check(load().rs_hip_switch_get(name.encode(), C.byref(v)))
    return float(v.value)


# The setters of the switches that have one: (wrapper, its argument and default, result type, what it sets).  Each forwards to
# rs_hip_<wrapper>: a negative argument only reads, the previous value comes back.
_SETTERS = [
    ("icp_reference_order_below", "n_points", -1, int,
     "Sources of at most n_points points run the estimator in the reference's accumulation order (bit-identical results)."),
    ("icp_replay_below", "n_points", -1, int,
     "Threshold up to which sources above the reference-order threshold get the reference's sums computed in parallel (same bits)."),
    ("icp_lane_chains_below", "n_points", -1, int,
     "Sources above the two thresholds before and of at most n_points points: the reference's centroid chains by one wave per chain "
     "+ fp64 moments (any number of problems side by side)."),
    ("icp_early_plain", "on", -1, int, "Plain (chain-free) early iterations of the lane / grid chain estimators (default on)."),
    ("icp_plain_from_records", "on", -1, int,
     "1: plain iterations read the searches' 48-byte records again (default 0: moments from the matches, no records written)."),
    ("icp_update_fenced", "on", -1, int,
     "1: the launch that ends an iteration hands its sums over by two full fences again (default 0: agent-scope atomics; the same bits)."),
    ("icp_stop_guard", "guard", -1.0, float, "Width of the stop test's guard (0: off; default 1.5e-6)."),
    ("icp_exact_centroids", "on", -1, int,
     "Sources above both thresholds: centre the fp64 step on the reference's own fp32 centroid chains (default on)."),
    ("icp_chains_retry_after", "calls", -1, int,
     "After a source's centroid chains gave up, its next `calls` ICP calls go straight to the replay (default 15; 0: every call tries "
     "the chains first)."),
    ("score_scene_space_from", "n_queries", -1, int,
     "Score batches of at least n_queries (poses x object points) take the scene-space route (queries sorted by scene block)."),
    ("icp_faith_guess", "permille", -1, int,
     "Test switch of the sequential estimator's guessed cut (1000: as made, 0: three passes, else scaled)."),
]
# ... and the counters next to them: (wrapper, what it counts)
_COUNTERS = [
    ("icp_lane_chains_sequential", "(diagnostics) addends the lane chains have added one by one in fp32 since init."),
    ("icp_stop_guard_redone", "(diagnostics) problems run again in the reference's order because a stop test was decided inside the guard, since init."),
    ("icp_chains_gave_up", "Calls the grid chains gave up and the replay's pass 2 redid (include/rescan_hip.h)."),
    ("icp_replay_redone", "Segments the last call's replay walks had to re-add one addend after the other (include/rescan_hip.h)."),
    ("icp_faith_redone", "Iterations of the sequential estimator whose one-pass statistics + centroids had to be summed again (cumulative)."),
]


def _setter(name, arg, default, kind, doc):
    def f(value=default):
        return kind(getattr(load(), "rs_hip_" + name)(kind(value)))
    f.__name__ = f.__qualname__ = name
    f.__doc__ = f"{doc}  {arg} < 0 only reads.  Returns the previous value."
    return f


def _counter(name, doc):
    def f():
        return int(getattr(load(), "rs_hip_" + name)())
    f.__name__ = f.__qualname__ = name
    f.__doc__ = doc
    return f


for _row in _SETTERS:
    globals()[_row[0]] = _setter(*_row)
for _row in _COUNTERS:
    globals()[_row[0]] = _counter(*_row)


def icp_state_layout():
    """(words of loop state per problem, largest state block in words that rides in the fill launch's argument block)."""
    a, b = C.c_int32(0), C.c_int32(0)
    load().rs_hip_icp_state_layout(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def icp_align(source, target, T1, T2=IDENTITY, max_dist=0.1, max_angle=np.deg2rad(60.0), max_iter=100,
              fixed_iters=False):
    """icp_align (lib/rs/icp.h:416-500).  Returns (err, T1_new, n_iters)."""
    T = _f32(T1).ravel().copy()
    err = C.c_float(); it = C.c_int32()
    _check(load().rs_hip_icp_align(source.handle, target.handle, T, _f32(T2).ravel(), float(max_dist),
                                   float(np.float32(max_angle)), int(max_iter), int(bool(fixed_iters)),
                                   C.byref(err), C.byref(it)))
    return err.value, T, it.value


def icp_align_traced(source, target, T1, T2=IDENTITY, max_dist=0.1, max_angle=np.deg2rad(60.0), max_iter=100, fixed_iters=False):
    """icp_align, also returning the error after every iteration (what the reference prints with verbose = true).
    Returns (err, T1_new, n_iters, errs[n_iters])."""
    T = _f32(T1).ravel().copy()
    err = C.c_float(); it = C.c_int32()
    errs = np.zeros(max(1, int(max_iter)), np.float32)
    _check(load().rs_hip_icp_align_traced(source.handle, target.handle, T, _f32(T2).ravel(), float(max_dist),
                                          float(np.float32(max_angle)), int(max_iter), int(bool(fixed_iters)),
                                          C.byref(err), C.byref(it), errs))
    return err.value, T, it.value, errs[: it.value].copy()


# rs_hip_icp_trace_begin's estimator codes (include/rescan_hip.h: RS_HIP_ICP_STEP_*)
ICP_STEP_NONE, ICP_STEP_REF_ORDER, ICP_STEP_REPLAY, ICP_STEP_LANE_CHAINS, ICP_STEP_GRID_CHAINS, ICP_STEP_PLAIN, \
    ICP_STEP_RECORDS, ICP_STEP_MOMENTS = -1, 0, 1, 2, 3, 4, 5, 6
ICP_STEP_NAMES = {-1: "none", 0: "ref_order", 1: "replay", 2: "lane_chains", 3: "grid_chains", 4: "plain", 5: "records",
                  6: "moments"}


class IcpTrace:
    """The calling thread's ICP calls inside ``with IcpTrace(max_iter, n_problems) as tr:`` leave, per problem p and
    iteration i, the pose after the iteration (tr.poses[p, i], 16 floats), its error (tr.errs[p, i]) and the estimator step
    that ran (tr.kinds[p, i], ICP_STEP_*; ICP_STEP_NONE where no iteration ran); tr.redone[p] = 1 where the stop test's
    guard ran the problem again in the reference's order (rs_hip_icp_trace_begin)."""

    def __init__(self, max_iter, n_problems):
        self.poses = np.zeros((int(n_problems), int(max_iter), 16), np.float32)
        self.errs = np.zeros((int(n_problems), int(max_iter)), np.float32)
        self.kinds = np.zeros((int(n_problems), int(max_iter)), np.int32)
        self.redone = np.zeros(int(n_problems), np.int32)

    def __enter__(self):
        _check(load().rs_hip_icp_trace_begin(self.poses.reshape(-1), self.errs.reshape(-1), self.kinds.reshape(-1),
                                              self.redone, self.poses.shape[1], self.poses.shape[0]))
        return self

    def __exit__(self, *exc):
        _check(load().rs_hip_icp_trace_end())
        return False


def icp_align_batch(source, target, T1s, T2=IDENTITY, max_dist=0.1, max_angle=np.deg2rad(60.0), max_iter=100,
                    fixed_iters=False):
    T = _f32(T1s).reshape(-1, 16).copy()
    n = len(T)
    errs = np.zeros(n, np.float32); its = np.zeros(n, np.int32)
    _check(load().rs_hip_icp_align_batch(source.handle, target.handle, T, n, _f32(T2).ravel(), float(max_dist),
                                         float(np.float32(max_angle)), int(max_iter), int(bool(fixed_iters)),
                                         errs, its))
    return errs, T, its


def icp_align_multi(sources, target, T1s, T2=IDENTITY, max_dist=0.1, max_angle=np.deg2rad(60.0), max_iter=100, fixed_iters=False):
    """rs_hip_icp_align_multi: problem p aligns sources[p] (a Cloud each) to `target` from T1s[p] — one call."""
    T = _f32(T1s).reshape(-1, 16).copy()
    n = len(T)
    assert n == len(sources)
    handles = (C.c_void_p * max(1, n))(*[s_.handle for s_ in sources])
    errs = np.zeros(n, np.float32); its = np.zeros(n, np.int32)
    _check(load().rs_hip_icp_align_multi(C.addressof(handles), target.handle, T, n, _f32(T2).ravel(), float(max_dist),
                                         float(np.float32(max_angle)), int(max_iter), int(bool(fixed_iters)), errs, its))
    return errs, T, its


def icp_find_corrs(source, target, T1, T2=IDENTITY, max_dist=0.1, max_angle=np.deg2rad(60.0)):
    n1 = source.n
    out = [np.zeros((max(n1, 1), 3), np.float32) for _ in range(4)]
    w = np.zeros(max(n1, 1), np.float32)
    nc = C.c_int32()
    _check(load().rs_hip_icp_find_corrs(source.handle, target.handle, _f32(T1).ravel(), _f32(T2).ravel(),
                                        float(max_dist), float(np.float32(max_angle)), *out, w, C.byref(nc)))
    return [o[:nc.value] for o in out] + [w[:nc.value]]


def icp_estimate_pt2pl(p1, p2, n2, w, T1):
    T = _f32(T1).ravel().copy(); err = C.c_float()
    _check(load().rs_hip_icp_estimate_pt2pl(_f32(p1), _f32(p2), _f32(n2), _f32(w), len(w), T, C.byref(err)))
    return err.value, T


def alignment_scores(obj, scene, poses, radius=0.1, max_n_neigh=64):
    """mgs_compute_object_alignment_score for a batch of poses."""
    poses = _f32(poses).reshape(-1, 16)
    out = np.zeros(len(poses), np.float32)
    _check(load().rs_hip_alignment_scores(obj.handle, scene.handle, poses, len(poses), float(radius),
                                          int(max_n_neigh), out))
    return out


def pose_grid_plan(bbox_min, bbox_max, spacing, angle_delta, tables=True):
    """The host part of the pose search (rs_hip_pose_grid_plan; no device needed): (ox, oz, yaw) — the cell offsets along x and z
    and one 16-float rotation per yaw step, by the reference's float loops as written; tables=False: the three counts only."""
    lo, hi = _f32(bbox_min).ravel(), _f32(bbox_max).ravel()
    nx, nz, ny = C.c_int32(), C.c_int32(), C.c_int32()
    lib = load()
    _check(lib.rs_hip_pose_grid_plan(lo.ctypes.data, hi.ctypes.data, float(spacing), float(angle_delta), C.byref(nx), C.byref(nz), C.byref(ny),
                                     None, 0, None, 0, None, 0))
    if not tables:
        return nx.value, nz.value, ny.value
    ox, oz, yaw = np.zeros(nx.value, np.float32), np.zeros(nz.value, np.float32), np.zeros((ny.value, 16), np.float32)
    _check(lib.rs_hip_pose_grid_plan(lo.ctypes.data, hi.ctypes.data, float(spacing), float(angle_delta), C.byref(nx), C.byref(nz), C.byref(ny),
                                     ox.ctypes.data, len(ox), oz.ctypes.data, len(oz), yaw.ctypes.data, len(yaw)))
    return ox, oz, yaw


def propose_poses(objects, scene, bbox_min, bbox_max, spacing, angle_delta, height, thresholds, radius, max_n_neigh, capacity=None,
                  trace=False):
    """mgs_propose_poses on the device (rs_hip_propose_poses).  objects: one sequence of level clouds per object, coarsest first,
    all of the same length as thresholds; scene: the cloud that is searched.  Returns a list of (poses (n, 16), scores (n,)) per
    object, with trace a dict of n_scored / n_kept (n_objects, n_levels) and n_proposed (n_objects) as well.  capacity (entries
    per object) defaults to the number of cells, which no list can exceed; a smaller one that does not suffice raises."""
    thresholds = _f32(thresholds).ravel()
    n_levels, n_obj = len(thresholds), len(objects)
    if any(len(o) != n_levels for o in objects):
        raise ValueError("propose_poses: every object needs one cloud per threshold")
    lo, hi = _f32(bbox_min).ravel(), _f32(bbox_max).ravel()
    if capacity is None:
        nx, nz, _ = pose_grid_plan(lo, hi, spacing, angle_delta, tables=False)
        capacity = nx * nz
    handles = (C.c_void_p * max(1, n_obj * n_levels))(*[c.handle for o in objects for c in o])
    counts = np.zeros(max(1, n_obj), np.int32)
    poses, scores = np.zeros((max(1, n_obj), capacity, 16), np.float32), np.zeros((max(1, n_obj), capacity), np.float32)
    tr, t = None, None
    if trace:
        t = dict(n_scored=np.zeros((n_obj, n_levels), np.int32), n_kept=np.zeros((n_obj, n_levels), np.int32), n_proposed=np.zeros(n_obj, np.int32))
        tr = ProposeTrace(t["n_scored"].ctypes.data, t["n_kept"].ctypes.data, t["n_proposed"].ctypes.data)
    _check(load().rs_hip_propose_poses(handles, n_obj, n_levels, scene.handle, lo.ctypes.data, hi.ctypes.data, float(spacing), float(angle_delta),
                                       float(height), thresholds.ctypes.data, float(radius), int(max_n_neigh), int(capacity), counts.ctypes.data,
                                       poses.ctypes.data, scores.ctypes.data, C.byref(tr) if trace else None))
    out = [(poses[o, :counts[o]].copy(), scores[o, :counts[o]].copy()) for o in range(n_obj)]
    return (out, t) if trace else out


def cell_best(scores, threshold):
    """The per-cell judgement of the grid search on host scores (n_cells, n_yaw) (rs_hip_cell_best): best_yaw (-1: none), best_score
    and keep — the cell's slot in the proposal list, -1 where it proposes nothing."""
    scores = _f32(scores)
    n_cells, n_yaw = scores.shape
    by, bs, keep = np.zeros(n_cells, np.int32), np.zeros(n_cells, np.float32), np.zeros(n_cells, np.int32)
    _check(load().rs_hip_cell_best(scores.ctypes.data, n_cells, n_yaw, float(threshold), by.ctypes.data, bs.ctypes.data, keep.ctypes.data))
    return by, bs, keep


def verify_marks(old_scores, new_scores, threshold):
    """A verification level's marks on host scores (rs_hip_verify_marks): old > 0 ? (new > threshold ? new : -1) : old."""
    old, new = _f32(old_scores).ravel(), _f32(new_scores).ravel()
    if len(old) != len(new):
        raise ValueError("verify_marks: one new score per old one")
    out = np.zeros(len(old), np.float32)
    _check(load().rs_hip_verify_marks(old.ctypes.data, new.ctypes.data, len(old), float(threshold), out.ctypes.data))
    return out


def propose_release():
    """Frees the pose search's buffers of the calling thread."""
    _check(load().rs_hip_propose_release())


def _placements(poses, objects, radii):
    n = len(objects)
    arr = (Placement * max(1, n))()
    poses = _f32(poses).reshape(-1, 16)
    for i in range(n):
        arr[i].pose[:] = [float(x) for x in poses[i]]
        arr[i].object = objects[i].handle
        arr[i].radius = float(radii[i])
    return arr


def assign_labels(scene, poses, objects, radii, labels, min_dists, label_base=0):
    arr = _placements(poses, objects, radii)
    _check(load().rs_hip_assign_labels(scene.handle, C.addressof(arr), len(objects), int(label_base), labels, min_dists))
    return labels, min_dists


def label_rows(scene, poses, objects, radii, out_device_ptr=None, query_order=False):
    """Per-placement unary rows.  With out_device_ptr the rows stay on the GPU (for an all-gather): indexed by scene point
    in input order, or — query_order — by the scene cloud's query slot (what the kernel writes, no re-ordering pass)."""
    arr = _placements(poses, objects, radii)
    n = len(objects)
    if out_device_ptr is not None:
        _check(load().rs_hip_label_rows(scene.handle, C.addressof(arr), n, C.c_void_p(out_device_ptr), 2 if query_order else 1))
        return None
    rows = np.zeros((n, scene.n), np.float32)
    _check(load().rs_hip_label_rows(scene.handle, C.addressof(arr), n, rows.ctypes.data_as(C.c_void_p), 0))
    return rows


def label_partial_device(scene, poses, objects, radii, label_base, min_dists_ptr, labels_ptr):
    """The (min_dist, label) partial of a contiguous run of the sorted arrangement, written to device memory (query order)."""
    arr = _placements(poses, objects, radii)
    _check(load().rs_hip_label_partial_device(scene.handle, C.addressof(arr), len(objects), int(label_base), C.c_void_p(min_dists_ptr), C.c_void_p(labels_ptr)))


def fold_label_partials_device(base_ptr, min_offsets, label_offsets, scene_n, labels=None, min_dists=None, query_order_of=None):
    """Ordered fold of gathered per-rank partials (min_dists at base + 4*min_offsets[r], int8 labels at base + label_offsets[r])."""
    mo = np.ascontiguousarray(min_offsets, np.int64); lo = np.ascontiguousarray(label_offsets, np.int64)
    if labels is None or min_dists is None:
        labels = np.empty(int(scene_n), np.int8); min_dists = np.empty(int(scene_n), np.float32)
    _check(load().rs_hip_fold_label_partials_device(C.c_void_p(base_ptr), mo, lo, len(mo), int(scene_n), labels, min_dists,
                                                    query_order_of.handle if query_order_of is not None else None))
    return labels, min_dists


def combine_label_rows(rows, labels, min_dists, label_base=0):
    rows = _f32(rows)
    load().rs_hip_combine_label_rows(rows, rows.shape[0], rows.shape[1], int(label_base), labels, min_dists)
    return labels, min_dists


def fold_label_rows_device(rows_device_ptr, row_offsets, scene_n, labels=None, min_dists=None, label_base=0, fresh=None, query_order_of=None):
    """Ordered arg-min over rows that sit in device memory (row k at rows_device_ptr + 4*row_offsets[k]).
    fresh (default: when no labels / min_dists are given): the fold starts from the loop's initial state (label 0, 1e9)
    on the device; labels / min_dists, if given, only receive the result (e.g. pinned buffers that are reused).
    query_order_of: the scene Cloud whose query order the rows are in (label_rows(..., query_order=True)); the result is
    returned in input order either way."""
    off = np.ascontiguousarray(row_offsets, np.int64)
    if fresh is None:
        fresh = labels is None or min_dists is None
    if labels is None or min_dists is None:
        labels = np.empty(int(scene_n), np.int8); min_dists = np.empty(int(scene_n), np.float32)
    _check(load().rs_hip_fold_label_rows_device(C.c_void_p(rows_device_ptr), off, len(off), int(scene_n), int(label_base),
                                                labels, min_dists, 1 if fresh else 0,
                                                query_order_of.handle if query_order_of is not None else None))
    return labels, min_dists


def arrangement_to_labels(scene, poses, objects, is_static, class_idx, radius=0.05, prioritize_static=False):
    """rspf_arrangement_to_labels ordering + both passes.  Returns dict(labels, min_dists, order)."""
    n = len(objects)
    handles = (C.c_void_p * max(1, n))(*[o.handle for o in objects])
    labels = np.zeros(scene.n, np.int8); mind = np.zeros(scene.n, np.float32); order = np.zeros(max(1, n), np.int32)
    _check(load().rs_hip_arrangement_to_labels(
        scene.handle, _f32(poses).reshape(-1, 16), C.addressof(handles),
        np.ascontiguousarray(is_static, np.int32), np.ascontiguousarray(class_idx, np.int32), n,
        float(radius), int(bool(prioritize_static)), labels, mind, order))
    return dict(labels=labels, min_dists=mind, order=order[:n])


def arrangement_to_ids(scene, poses, objects, is_static, class_idx, uidx, radius=0.05, prioritize_static=False, unlabelled_class_idx=0):
    """rspf_arrangement_to_labels including its tail (:851-869).  Returns dict(class_ids, instance_ids, labels, min_dists, order)."""
    n = len(objects)
    handles = (C.c_void_p * max(1, n))(*[o.handle for o in objects])
    cls = np.zeros(scene.n, np.int32); inst = np.zeros(scene.n, np.int32)
    labels = np.zeros(scene.n, np.int8); mind = np.zeros(scene.n, np.float32); order = np.zeros(max(1, n), np.int32)
    _check(load().rs_hip_arrangement_to_ids(
        scene.handle, _f32(poses).reshape(-1, 16), C.addressof(handles), np.ascontiguousarray(is_static, np.int32),
        np.ascontiguousarray(class_idx, np.int32), np.ascontiguousarray(uidx, np.int32), n, float(radius), int(bool(prioritize_static)),
        int(unlabelled_class_idx), cls, inst, labels.ctypes.data_as(C.c_void_p), mind.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p)))
    return dict(class_ids=cls, instance_ids=inst, labels=labels, min_dists=mind, order=order[:n])


def gather_attributes(sample_idx, arrays):
    """dst[a][i] = arrays[a][sample_idx[i]] on the device (the level builder's attribute gathers); arrays: list of 2-D or 1-D
    float32 / int32 arrays over the base level's points."""
    idx = np.ascontiguousarray(sample_idx, np.int32)
    srcs = [np.ascontiguousarray(a) for a in arrays]
    for a in srcs:
        assert a.dtype.itemsize == 4
    words = np.array([int(np.prod(a.shape[1:])) if a.ndim > 1 else 1 for a in srcs], np.int32)
    outs = [np.empty((len(idx),) + a.shape[1:], a.dtype) for a in srcs]
    sp = (C.c_void_p * len(srcs))(*[a.ctypes.data for a in srcs]); dp = (C.c_void_p * len(srcs))(*[o.ctypes.data for o in outs])
    _check(load().rs_hip_gather_attributes(idx, len(idx), len(srcs[0]) if srcs else 0, C.addressof(sp), words, C.addressof(dp), len(srcs)))
    return outs


def mat4_inverse(m):
    o = np.empty(16, np.float32); load().rs_hip_mat4_inverse(_f32(m).ravel(), o); return o


def level_samples(cloud, radius, max_n_neigh):
    """rs_pointcloud__compute_level_poisson (lib/rs/rs_pointcloud.h:984-1106): (sample indices, rounds)."""
    out = np.zeros(max(cloud.n, 1), np.int32)
    n = C.c_int32(); r = C.c_int32()
    _check(load().rs_hip_level_samples(cloud.handle, float(radius), int(max_n_neigh), out, C.byref(n), C.byref(r)))
    return out[:n.value].copy(), r.value


def _levels_many_args(bases, levels):
    nc, nl = len(bases), len(levels)
    radii = np.array([r for r, _ in levels], np.float32)
    caps = np.array([k for _, k in levels], np.int32)
    handles = (C.c_void_p * max(1, nc))(*[b.handle for b in bases])
    idx = [np.zeros(max(b.n, 1), np.int32) for b in bases for _ in range(nl)]
    ptrs = (C.c_void_p * max(1, nc * nl))(*[a.ctypes.data for a in idx])
    return nc, nl, radii, caps, handles, idx, ptrs


def level_samples_many(bases, levels):
    """rs_hip_level_samples for every level of `levels` = [(radius, max_n_neigh), ...] of every base, decided in one call
    (rs_hip_level_samples_many): ([[sample indices, ...per level], ...per base], rounds)."""
    nc, nl, radii, caps, handles, idx, ptrs = _levels_many_args(bases, levels)
    counts = np.zeros(max(1, nc * nl), np.int32); r = C.c_int32()
    _check(load().rs_hip_level_samples_many(C.addressof(handles), nc, radii.ctypes.data, caps.ctypes.data, nl, C.addressof(ptrs), counts.ctypes.data,
                                            C.byref(r)))
    return [[idx[c * nl + l][:counts[c * nl + l]].copy() for l in range(nl)] for c in range(nc)], r.value


def sincosf_model(x):
    """The device's sinf/cosf evaluated on the host (tests: must equal the machine's libm)."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    s = np.empty_like(x); c = np.empty_like(x)
    load().rs_hip_sincosf_model(x, len(x), s, c)
    return s, c


def mat4_mul(a, b):
    o = np.empty(16, np.float32); load().rs_hip_mat4_mul(_f32(a).ravel(), _f32(b).ravel(), o); return o


def compute_neighborhood(cloud, max_nn=8, radius_sq=0.05 * 0.05, dist_exp=15.0, angle_exp=16.0):
    """rspf_compute_neighborhood: unique weighted edges (idx1, idx2, weight) of the K-nearest self-search."""
    cap = max(1, cloud.n * max_nn)
    a = np.zeros(cap, np.int32); b = np.zeros(cap, np.int32); w = np.zeros(cap, np.float32)
    m = C.c_int64()
    _check(load().rs_hip_compute_neighborhood(cloud.handle, int(max_nn), float(np.float32(radius_sq)), float(dist_exp),
                                              float(angle_exp), a, b, w, cap, C.byref(m)))
    return a[:m.value].copy(), b[:m.value].copy(), w[:m.value].copy()


class Coverage:
    """Scene voxel grid + coverage scores (rsao__compute_scene_coverage_score)."""

    def __init__(self, bbox_min, bbox_max, scene_pos, quality=None, voxel_size=0.05, threshold=0.5):
        pos = np.ascontiguousarray(scene_pos, np.float32)
        q = None if quality is None else np.ascontiguousarray(quality, np.float32)
        self.handle = load().rs_hip_coverage_create(np.ascontiguousarray(bbox_min, np.float32), np.ascontiguousarray(bbox_max, np.float32),
                                                    float(voxel_size), pos.ctypes.data if len(pos) else None,
                                                    None if q is None else q.ctypes.data, len(pos), float(threshold))
        if not self.handle:
            raise RescanHipError(f"coverage_create failed: {load().rs_hip_last_error().decode()}")
        res = np.zeros(3, np.int32); org = np.zeros(3, np.float32); n = C.c_int64(); v = C.c_int64()
        _check(load().rs_hip_coverage_info(self.handle, res, org, C.byref(n), C.byref(v)))
        self.res, self.origin, self.n_cells, self.valid_cells = res, org, n.value, v.value

    def scene_grid(self):
        data = np.zeros(self.n_cells, np.uint8)
        _check(load().rs_hip_coverage_scene_grid(self.handle, data))
        return data

    def scores(self, arrangements):
        """arrangements: list of lists of (Cloud, pose16, is_static).  Returns (scores f32, agree i32)."""
        flat = [p for a in arrangements for p in a]
        first = np.zeros(len(arrangements) + 1, np.int32)
        first[1:] = np.cumsum([len(a) for a in arrangements])
        n = len(flat)
        objs = (C.c_void_p * max(1, n))(*[p[0].handle for p in flat])
        poses = np.ascontiguousarray(np.array([np.asarray(p[1], np.float32).ravel() for p in flat], np.float32).reshape(-1, 16)) if n else np.zeros((1, 16), np.float32)
        stat = np.array([int(p[2]) for p in flat] or [0], np.int32)
        sc = np.zeros(len(arrangements), np.float32); ag = np.zeros(len(arrangements), np.int32)
        _check(load().rs_hip_coverage_scores(self.handle, C.addressof(objs), poses, stat, first, len(arrangements), sc, ag.ctypes.data))
        return sc, ag

    def extensions(self, base, candidates):
        """rsao_greedy_step's trial arrangements in one call (rs_hip_coverage_extensions).  base: list of (Cloud, pose16, is_static)
        — a static placement's Cloud may be None; candidates: list of (Cloud, pose16).  Returns (scores f32 [C], agree i32 [C],
        the base's own agreeing-voxel count): candidate k scored as the arrangement base + [candidate k]."""
        for k, p in enumerate(base):
            if len(p) != 3 or (not p[2] and p[0] is None) or np.size(p[1]) != 16:
                raise ValueError(f"extensions: base placement {k} is not (Cloud, pose16, is_static)")
        for k, p in enumerate(candidates):
            if len(p) != 2 or p[0] is None or np.size(p[1]) != 16:
                raise ValueError(f"extensions: candidate {k} is not (Cloud, pose16)")
        nb, nc = len(base), len(candidates)
        bo = (C.c_void_p * max(1, nb))(*[None if p[0] is None else p[0].handle for p in base])
        co = (C.c_void_p * max(1, nc))(*[p[0].handle for p in candidates])
        bp = _f32(np.array([np.asarray(p[1], np.float32).ravel() for p in base], np.float32).reshape(-1, 16)) if nb else np.zeros((1, 16), np.float32)
        cp = _f32(np.array([np.asarray(p[1], np.float32).ravel() for p in candidates], np.float32).reshape(-1, 16)) if nc else np.zeros((1, 16), np.float32)
        bs = np.array([int(bool(p[2])) for p in base] or [0], np.int32)
        sc, ag, ba = np.zeros(max(1, nc), np.float32), np.zeros(max(1, nc), np.int32), C.c_int32()
        _check(load().rs_hip_coverage_extensions(self.handle, C.addressof(bo), bp.ctypes.data, bs.ctypes.data, nb, C.addressof(co), cp.ctypes.data, nc,
                                                 sc.ctypes.data, ag.ctypes.data, C.addressof(ba)))
        return sc[:nc], ag[:nc], ba.value

    def footprints(self, placements):
        """The scene-active cells of every placement in one call (rs_hip_coverage_footprints).  placements: list of (Cloud, pose16,
        is_static) — a static placement's Cloud may be None.  Returns a Footprints, which scores arrangements of these placements
        on the host."""
        for k, p in enumerate(placements):
            if len(p) != 3 or (not p[2] and p[0] is None) or np.size(p[1]) != 16:
                raise ValueError(f"footprints: placement {k} is not (Cloud, pose16, is_static)")
        n = len(placements)
        objs = (C.c_void_p * max(1, n))(*[None if p[0] is None else p[0].handle for p in placements])
        poses = _f32(np.array([np.asarray(p[1], np.float32).ravel() for p in placements], np.float32).reshape(-1, 16)) if n else np.zeros((1, 16), np.float32)
        stat = np.array([int(bool(p[2])) for p in placements] or [0], np.int32)
        h = load().rs_hip_coverage_footprints(self.handle, C.addressof(objs), poses.ctypes.data, stat.ctypes.data, n)
        if not h:
            raise RescanHipError(f"coverage_footprints failed: {load().rs_hip_last_error().decode()}")
        return Footprints(h)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                load().rs_hip_coverage_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class Footprints:
    """Per placement, the sorted scene-active cells it hits (Coverage.footprints, or Footprints.from_arrays); scores arrangements
    of these placements as unions, on the host, bit for bit rsao__compute_scene_coverage_score.  One thread at a time per object."""

    def __init__(self, handle):
        self.handle = handle
        n, nc, v, t = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        _check(load().rs_hip_footprints_info(self.handle, C.byref(n), C.byref(nc), C.byref(v), C.byref(t)))
        self.n_placements, self.n_cells, self.valid_cells, self.total_cells = n.value, nc.value, v.value, t.value
        self.offsets = np.zeros(n.value + 1, np.int64)
        self._cells = np.zeros(t.value, np.int32)
        _check(load().rs_hip_footprints_arrays(self.handle, self.offsets.ctypes.data, self._cells.ctypes.data if t.value else None))

    @classmethod
    def from_arrays(cls, n_cells, valid_cells, offsets, cells):
        """Host only.  offsets: n + 1 values from 0; placement k's cells = cells[offsets[k]:offsets[k+1]], ascending, no duplicates."""
        off = np.ascontiguousarray(offsets, np.int64)
        ce = np.ascontiguousarray(cells, np.int32)
        if off.ndim != 1 or len(off) < 1 or ce.ndim != 1 or len(ce) < int(off[-1]):
            raise ValueError("from_arrays: offsets is not n + 1 values, or there are fewer cells than offsets[-1]")
        h = load().rs_hip_footprints_from_arrays(int(n_cells), int(valid_cells), off.ctypes.data, ce.ctypes.data if len(ce) else None, len(off) - 1)
        if not h:
            raise RescanHipError(f"footprints_from_arrays failed: {load().rs_hip_last_error().decode()}")
        return cls(h)

    def cells(self, k):
        """Placement k's cells: int32, ascending."""
        if not 0 <= k < self.n_placements:
            raise IndexError(k)
        return self._cells[self.offsets[k]:self.offsets[k + 1]].copy()

    def scores(self, arrangements):
        """arrangements: list of lists of placement indices.  Returns (scores f32, agree i32)."""
        first = np.zeros(len(arrangements) + 1, np.int32)
        first[1:] = np.cumsum([len(a) for a in arrangements])
        members = np.array([m for a in arrangements for m in a] or [0], np.int32)
        na = len(arrangements)
        sc, ag = np.zeros(max(1, na), np.float32), np.zeros(max(1, na), np.int32)
        _check(load().rs_hip_footprints_scores(self.handle, members.ctypes.data, first.ctypes.data, na, sc.ctypes.data, ag.ctypes.data))
        return sc[:na], ag[:na]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                load().rs_hip_footprints_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def coverage_lds_budget(nbytes=-1):
    """Candidates of Coverage.extensions whose bit sub-box fits `nbytes` of LDS keep it there, larger ones use global memory (0: all of
    them); returns the previous budget."""
    return load().rs_hip_coverage_lds_budget(int(nbytes))


def coverage_extension_routes(reset=False):
    """(candidates scored on the LDS route, on the slab route) since the last reset."""
    a, b = C.c_int64(), C.c_int64()
    load().rs_hip_coverage_extension_routes(C.byref(a), C.byref(b), int(bool(reset)))
    return a.value, b.value


def coverage_footprint_routes(reset=False):
    """(placements footprinted on the LDS route, on the slab route) since the last reset."""
    a, b = C.c_int64(), C.c_int64()
    load().rs_hip_coverage_footprint_routes(C.byref(a), C.byref(b), int(bool(reset)))
    return a.value, b.value


def arrange_release():
    """Frees the buffers Coverage.extensions, Coverage.footprints and scene_saliency keep for the calling thread (a thread that ends calls this first)."""
    _check(load().rs_hip_arrange_release())


def voxel_grid_shape(bbox_min, bbox_max, voxel_size):
    """isect_grid3d_init for a box (host only): (res int32[3], origin float32[3], n_cells)."""
    res, org, n = np.zeros(3, np.int32), np.zeros(3, np.float32), C.c_int64()
    _check(load().rs_hip_voxel_grid_shape(_f32(bbox_min).ctypes.data, _f32(bbox_max).ctypes.data, float(np.float32(voxel_size)),
                                          res.ctypes.data, org.ctypes.data, C.addressof(n)))
    return res, org, n.value


def scene_saliency(bbox_min, bbox_max, objects, prop_object, prop_poses, prop_static, scene_pos, scene_class, wall_class, floor_class,
                   voxel_size=0.15, want_grid=False):
    """rsao_compute_scene_saliency for one scene (rs_hip_scene_saliency).  objects: list of level-2 Clouds (None where no proposal
    names the object); proposal k places objects[prop_object[k]] at prop_poses[k], prop_static[k] = the object is static;
    scene_pos / scene_class: the scene's level-0 points and class ids; wall_class / floor_class: -1 where the class is absent.
    Returns quality float32 [n] (0 or 1), and the grid as the reference's byte array if want_grid."""
    bmin, bmax = _f32(bbox_min).ravel(), _f32(bbox_max).ravel()
    po = np.ascontiguousarray(prop_object, np.int32).ravel()
    pp = _f32(prop_poses).reshape(-1, 16)
    ps = np.ascontiguousarray(prop_static, np.int32).ravel()
    pos = _f32(scene_pos).reshape(-1, 3)
    cls = np.ascontiguousarray(scene_class, np.int32).ravel()
    if len(bmin) != 3 or len(bmax) != 3 or not float(voxel_size) > 0:
        raise ValueError("scene_saliency: a box of two 3-vectors and a voxel size > 0")
    if not (len(pp) == len(po) == len(ps)) or len(cls) != len(pos):
        raise ValueError("scene_saliency: proposal or scene arrays of different lengths")
    if len(po) and (po.min() < 0 or po.max() >= len(objects) or any(objects[o] is None for o in po)):
        raise ValueError("scene_saliency: a proposal names an object outside the list or without a cloud")
    objs = (C.c_void_p * max(1, len(objects)))(*[None if o is None else o.handle for o in objects])
    quality = np.zeros(max(1, len(pos)), np.float32)
    grid, cap = None, 0
    if want_grid:
        cap = voxel_grid_shape(bmin, bmax, voxel_size)[2]
        grid = np.zeros(cap, np.uint8)
    _check(load().rs_hip_scene_saliency(bmin.ctypes.data, bmax.ctypes.data, float(np.float32(voxel_size)), C.addressof(objs), len(objects),
                                        po.ctypes.data, pp.ctypes.data, ps.ctypes.data, len(po), pos.ctypes.data, cls.ctypes.data, len(pos),
                                        int(wall_class), int(floor_class), quality.ctypes.data, None if grid is None else grid.ctypes.data, cap))
    return (quality[:len(pos)], grid) if want_grid else quality[:len(pos)]


def _isect_shapes(shapes):
    arr = (IsectShape * len(shapes))()
    for k, (b, e) in enumerate(shapes):
        arr[k].boundary, arr[k].extent = b.handle, e.handle
    return arr


def overlap_factors(shapes, shape_a, poses_a, shape_b, poses_b, voxel_size=0.1, voxelize_inside=True, normalize_by_smaller=False):
    """isect_get_overlap_factor for a batch of pairs (rs_hip_overlap_factors).  shapes: list of (boundary Cloud, extent Cloud);
    pair k places shapes[shape_a[k]] by poses_a[k] and shapes[shape_b[k]] by poses_b[k].  Returns (overlap float32 [n],
    counts int32 [n, 3] = count_a, count_b, both)."""
    arr = _isect_shapes(shapes)
    ia, ib = np.ascontiguousarray(shape_a, np.int32), np.ascontiguousarray(shape_b, np.int32)
    pa, pb = _f32(poses_a).reshape(-1, 16), _f32(poses_b).reshape(-1, 16)
    n = len(ia)
    assert len(ib) == n and len(pa) == n and len(pb) == n
    ov, cnt = np.zeros(n, np.float32), np.zeros((n, 3), np.int32)
    _check(load().rs_hip_overlap_factors(C.addressof(arr), len(shapes), ia.ctypes.data, pa.ctypes.data, ib.ctypes.data, pb.ctypes.data, n,
                                         float(np.float32(voxel_size)), int(bool(voxelize_inside)), int(bool(normalize_by_smaller)),
                                         ov.ctypes.data, cnt.ctypes.data))
    return ov, cnt


def nms(shape, centroid, poses, scores, dist_threshold=0.2):
    """mgs_non_maxima_suppresion of one object's proposals (rs_hip_nms).  shape: (boundary Cloud, extent Cloud); centroid: the
    object's level-0 centroid as the reference caches it.  Returns (marks int32 [n]: 1 keep / 2 discard, keep_idx ascending, rounds)."""
    arr = _isect_shapes([shape])
    c = _f32(centroid).ravel()
    p, s = _f32(poses).reshape(-1, 16), _f32(scores).ravel()
    n = len(s)
    assert len(p) == n and len(c) == 3
    marks, keep = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    nk, nr = C.c_int32(), C.c_int32()
    _check(load().rs_hip_nms(C.addressof(arr), c.ctypes.data, p.ctypes.data, s.ctypes.data, n, float(np.float32(dist_threshold)),
                             marks.ctypes.data, keep.ctypes.data, C.addressof(nk), C.addressof(nr)))
    return marks[:n], keep[:nk.value].copy(), nr.value


def isect_lds_budget(nbytes=-1):
    """Pairs whose bit planes fit `nbytes` of LDS keep them there, larger ones use global memory (0: all of them); returns the previous budget."""
    return load().rs_hip_isect_lds_budget(int(nbytes))


def isect_pairs(reset=False):
    """(pairs rasterised, pairs rs_hip_nms settled without) since the last reset."""
    a, b = C.c_int64(), C.c_int64()
    load().rs_hip_isect_pairs(C.byref(a), C.byref(b), int(bool(reset)))
    return a.value, b.value
