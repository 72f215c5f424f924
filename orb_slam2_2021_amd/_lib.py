"""ctypes binding of liborbfe.so (include/orbfe.h, orbfe_match_batch.h, orbfe_debug.h, orbfe_synth.h,
orbfe_vocab.h, orbfe_stereo.h, orbfe_frustum.h, orbfe_keyframe.h, orbfe_pack.h, orbfe_c3.h,
orbfe_kfdb.h, orbfe_sim3.h, orbfe_triangulate.h, orbfe_pnp.h, orbfe_poseopt.h,
orbfe_optsim3.h, orbfe_lba.h, orbfe_essgraph.h, orbfe_gba.h, orbfe_init.h, orbfe_covis.h, orbfe_localmap.h,
orbfe_mapcorr.h, orbfe_frame.h, orbfe_gridmap.h).

The shared library is the product: every compute call below runs the HIP kernels in it. There is
no CPU fallback -- if the library is missing, or no HIP device is present when a compute handle is
created, the call raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, byref, Structure, c_char, c_char_p, c_double, c_float, c_int, c_int32,
                    c_size_t, c_uint8, c_uint32, c_uint64, c_void_p)

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBFE_LIB", os.path.join(_PKG_DIR, "lib", "liborbfe.so"))

ORBFE_OK = 0
ORBFE_ERR_ARG = -1
ORBFE_ERR_CAPACITY = -2
ORBFE_ERR_HIP = -3
ORBFE_ERR_STATE = -4
ORBFE_RESIZE_SIMD128 = 0
ORBFE_RESIZE_SCALAR = 1
ORBFE_MP_NONE, ORBFE_MP_PRESENT, ORBFE_MP_OBSERVED = 0, 1, 2
ORBFE_MP_BAD = 3  # orbfe_keyframe.h: non-NULL MapPoint with isBad()
MPF_TRACK_IN_VIEW, MPF_BAD, MPF_OBSERVED, MPF_PRESENT, MPF_OUTLIER = 1, 2, 4, 8, 16
MPF_SEEN = 32  # orbfe_frustum.h: mnLastFrameSeen == CurrentFrame.mnId
MPF_SKIP = 64  # orbfe_keyframe.h: already found / in the KeyFrame / already matched

# cv::KeyPoint field order (28 bytes), = orbfe_keypoint
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28


class OrbfeError(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what} failed with status {status}: {last_error()}")
        self.status = status


class LibraryMissing(ImportError):
    pass


class frame_view(Structure):
    _fields_ = [("n", c_int32), ("keys_un", c_void_p), ("u_right", c_void_p),
                ("descriptors", c_void_p), ("mp_state", c_void_p), ("nlevels", c_int32),
                ("scale_factors", c_void_p), ("level_sigma2", c_void_p),
                ("min_x", c_float), ("max_x", c_float), ("min_y", c_float), ("max_y", c_float),
                ("grid_inv_w", c_float), ("grid_inv_h", c_float),
                ("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float),
                ("bf", c_float), ("b", c_float),
                ("grid_origin_set", c_int32), ("grid_min_x", c_float), ("grid_min_y", c_float)]


class feature_vector(Structure):
    _fields_ = [("n_nodes", c_int32), ("node_ids", c_void_p), ("offsets", c_void_p),
                ("indices", c_void_p)]


class local_mappoints(Structure):
    _fields_ = [("m", c_int32), ("flags", c_void_p), ("proj_x", c_void_p), ("proj_y", c_void_p),
                ("proj_xr", c_void_p), ("level", c_void_p), ("view_cos", c_void_p),
                ("descriptors", c_void_p)]


class lastframe_mappoints(Structure):
    _fields_ = [("n", c_int32), ("flags", c_void_p), ("world_pos", c_void_p),
                ("descriptors", c_void_p), ("octave", c_void_p), ("angle", c_void_p),
                ("tcw_last", c_float * 12)]


class mappoint_geometry(Structure):
    _fields_ = [("m", c_int32), ("flags", c_void_p), ("world_pos", c_void_p), ("normal", c_void_p),
                ("min_distance", c_void_p), ("max_distance", c_void_p), ("descriptors", c_void_p)]


class frustum_out(Structure):
    _fields_ = [("flags", c_void_p), ("proj_x", c_void_p), ("proj_y", c_void_p),
                ("proj_xr", c_void_p), ("level", c_void_p), ("view_cos", c_void_p)]


class sft_pair(Structure):
    _fields_ = [("kf1", frame_view), ("kf2", frame_view), ("fv1", feature_vector),
                ("fv2", feature_vector), ("f12", c_float * 9), ("ex", c_float), ("ey", c_float),
                ("match12", c_void_p), ("nmatches", c_void_p), ("kf1_n_dev", c_void_p),
                ("kf2_n_dev", c_void_p), ("fv1_nodes_dev", c_void_p), ("fv2_nodes_dev", c_void_p)]


class c3_set(Structure):  # orbfe_c3.h
    _fields_ = [("kps", c_void_p), ("desc", c_void_p), ("counts", c_void_p), ("fv_node_ids", c_void_p),
                ("fv_offsets", c_void_p), ("fv_indices", c_void_p), ("fv_n_nodes", c_void_p),
                ("bow_words", c_void_p), ("bow_weights", c_void_p), ("bow_n", c_void_p),
                ("u_right", c_void_p), ("depth", c_void_p), ("matcher", c_void_p), ("pairs", c_void_p)]


class c3_config(Structure):
    _fields_ = [("n_images", c_int), ("rows", c_int), ("cols", c_int), ("cap", c_int), ("n_vocab", c_int),
                ("levelsup", c_int), ("n_stereo", c_int), ("mbf", c_float), ("mb", c_float),
                ("stereo_on_match", c_int), ("n_pairs", c_int)]


class kfdb_query(Structure):  # orbfe_kfdb.h
    _fields_ = [("mode", c_int), ("n", c_int), ("words", c_void_p), ("weights", c_void_p),
                ("on_device", c_int), ("d_n", c_void_p), ("stream", c_void_p), ("min_score", c_float),
                ("excluded", c_void_p), ("n_excluded", c_int)]


class kfdb_result(Structure):
    _fields_ = [("capacity", c_int), ("n_sharing", c_int), ("max_common", c_int), ("min_common", c_int),
                ("kf_ids", c_void_p), ("common_words", c_void_p), ("scored", c_void_p),
                ("scores", c_void_p), ("n_candidates", c_int), ("candidates", c_void_p)]


class covis_connections(Structure):  # orbfe_covis.h
    _fields_ = [("capacity", c_int), ("n_counter", c_void_p), ("counter_ids", c_void_p),
                ("counter_weights", c_void_p), ("n_ordered", c_void_p), ("ordered_ids", c_void_p),
                ("ordered_weights", c_void_p), ("nmax", c_void_p), ("kf_max", c_void_p), ("unchanged", c_void_p)]


class covis_votes(Structure):
    _fields_ = [("capacity", c_int), ("n", c_void_p), ("kf_ids", c_void_p), ("counts", c_void_p),
                ("max", c_void_p), ("kf_max", c_void_p)]


class covis_local_map(Structure):
    _fields_ = [("point_capacity", c_int), ("fixed_capacity", c_int), ("edge_capacity", c_int),
                ("n_points", c_int), ("n_fixed", c_int), ("n_edges", c_int), ("point_ids", c_void_p),
                ("fixed_ids", c_void_p), ("edge_begin", c_void_p), ("edge_kf", c_void_p), ("edge_slot", c_void_p)]


class covis_cull(Structure):
    _fields_ = [("decision", c_void_p), ("n_mps", c_void_p), ("n_redundant", c_void_p), ("bad_begin", c_void_p),
                ("bad_points", c_void_p), ("bad_capacity", c_int)]


class covis_points(Structure):  # orbfe_localmap.h
    _fields_ = [("point_capacity", c_int), ("n_points", c_int), ("point_ids", c_void_p)]


class covis_local_geometry(Structure):
    _fields_ = [("point_capacity", c_int), ("n_points", c_int), ("n_missing", c_int), ("point_ids", c_void_p),
                ("geometry", mappoint_geometry)]


class sim3_solver(Structure):  # orbfe_sim3.h
    _fields_ = [("n", c_int), ("x3dc1", c_void_p), ("x3dc2", c_void_p), ("sigma2_1", c_void_p),
                ("sigma2_2", c_void_p), ("k1", c_float * 4), ("k2", c_float * 4), ("fix_scale", c_int),
                ("min_inliers", c_int), ("max_iterations", c_int), ("probability", c_double),
                ("n_hyp", c_int), ("rand_idx", c_void_p), ("hyp_t12", c_void_p), ("hyp_t21", c_void_p)]


class sim3_result(Structure):
    _fields_ = [("hyp_capacity", c_int), ("mask_words", c_int), ("n_inliers", c_void_p), ("t12", c_void_p),
                ("t21", c_void_p), ("r12", c_void_p), ("tr12", c_void_p), ("s12", c_void_p),
                ("inlier_mask", c_void_p), ("n_evaluated", c_int), ("ransac_max_its", c_int),
                ("accepted", c_int), ("accepted_inliers", c_int), ("best", c_int), ("best_inliers", c_int),
                ("no_more", c_int)]


class sim3_state(Structure):
    _fields_ = [("iterations", c_int), ("best_inliers", c_int), ("best", c_int)]


class sim3_iterate(Structure):
    _fields_ = [("mask_words", c_int), ("inlier_mask", c_void_p), ("accepted", c_int), ("t12", c_float * 12),
                ("no_more", c_int), ("n_inliers", c_int)]


class pnp_solver(Structure):  # orbfe_pnp.h
    _fields_ = [("n", c_int), ("p3dw", c_void_p), ("p2d", c_void_p), ("sigma2", c_void_p), ("k", c_float * 4),
                ("probability", c_double), ("min_inliers", c_int), ("max_iterations", c_int), ("min_set", c_int),
                ("epsilon", c_float), ("th2", c_float), ("n_hyp", c_int), ("rand_idx", c_void_p)]


class pnp_result(Structure):
    _fields_ = [("hyp_capacity", c_int), ("rec_capacity", c_int), ("mask_words", c_int),
                ("n_inliers", c_void_p), ("inlier_mask", c_void_p), ("r", c_void_p), ("t", c_void_p),
                ("tcw", c_void_p), ("n_chosen", c_void_p), ("flags", c_void_p),
                ("records", c_void_p), ("refined_inliers", c_void_p), ("refined_mask", c_void_p),
                ("refined_r", c_void_p), ("refined_t", c_void_p), ("refined_tcw", c_void_p),
                ("refined_n_chosen", c_void_p), ("refined_flags", c_void_p),
                ("n_records", c_int), ("n_evaluated", c_int), ("ransac_max_its", c_int),
                ("ransac_min_inliers", c_int), ("ransac_epsilon", c_float),
                ("accepted", c_int), ("accepted_inliers", c_int), ("best", c_int), ("best_inliers", c_int),
                ("no_more", c_int)]


class pnp_state(Structure):
    _fields_ = [("iterations", c_int), ("best_inliers", c_int), ("best", c_int)]


class pnp_iterate(Structure):
    _fields_ = [("mask_words", c_int), ("inlier_mask", c_void_p), ("returned", c_int), ("accepted", c_int),
                ("tcw", c_float * 12), ("no_more", c_int), ("n_inliers", c_int)]


PNP_FLAG_SVD_NULL, PNP_FLAG_QR_SINGULAR = 1, 2  # orbfe_pnp.h: deviation flags of one hypothesis


class init_problem(Structure):  # orbfe_init.h
    _fields_ = [("n1", c_int), ("n2", c_int), ("keys1", c_void_p), ("keys2", c_void_p), ("matches12", c_void_p),
                ("k", c_float * 4), ("sigma", c_float), ("min_parallax", c_float), ("n_hyp", c_int),
                ("rand_idx", c_void_p)]


class init_result(Structure):
    _fields_ = [("hyp_capacity", c_int), ("mask_words", c_int), ("p3d", c_void_p), ("triangulated", c_void_p),
                ("score_h", c_void_p), ("score_f", c_void_p), ("mask_h", c_void_p), ("mask_f", c_void_p),
                ("ok", c_int), ("r21", c_float * 9), ("t21", c_float * 3), ("n_matches", c_int), ("flags", c_uint32),
                ("sh", c_float), ("sf", c_float), ("rh", c_float), ("model", c_int), ("best_h", c_int),
                ("best_f", c_int), ("h21", c_float * 9), ("f21", c_float * 9), ("n_motions", c_int),
                ("n_good", c_int * 8), ("cos_parallax", c_float * 8), ("candidate", c_int), ("motion", c_int),
                ("parallax", c_float)]


INIT_FLAG_TOO_FEW, INIT_FLAG_NO_MODEL = 1, 2  # orbfe_init.h: deviation flags of one problem
INIT_MODEL_NONE, INIT_MODEL_H, INIT_MODEL_F = -1, 0, 1


class poseopt_problem(Structure):  # orbfe_poseopt.h
    _fields_ = [("n", c_int), ("valid", c_void_p), ("xw", c_void_p), ("kp_un", c_void_p), ("u_right", c_void_p),
                ("inv_sigma2", c_void_p), ("k", c_float * 4), ("bf", c_float), ("tcw", c_float * 12)]


class poseopt_round(Structure):
    _fields_ = [("n_active", c_int), ("iterations", c_int), ("trials", c_int), ("rejected_trials", c_int),
                ("stop", c_int), ("n_bad", c_int), ("lam", c_double), ("chi2", c_double)]


class poseopt_result(Structure):
    _fields_ = [("mask_words", c_int), ("outlier_mask", c_void_p), ("tcw", c_float * 12),
                ("pose_q_t", c_double * 7), ("n_initial", c_int), ("n_bad", c_int), ("n_inliers", c_int),
                ("rounds_run", c_int), ("flags", c_uint32), ("rounds", poseopt_round * 4)]


class optsim3_problem(Structure):  # orbfe_optsim3.h
    _fields_ = [("n", c_int), ("valid", c_void_p), ("p3d1c", c_void_p), ("p3d2c", c_void_p), ("kp_un1", c_void_p),
                ("kp_un2", c_void_p), ("inv_sigma2_1", c_void_p), ("inv_sigma2_2", c_void_p), ("k1", c_float * 4),
                ("k2", c_float * 4), ("r12", c_float * 9), ("t12", c_float * 3), ("s12", c_float), ("th2", c_float),
                ("fix_scale", c_int), ("has_kf2", c_int), ("r2w", c_float * 9), ("t2w", c_float * 3)]


class optsim3_result(Structure):
    _fields_ = [("mask_words", c_int), ("removed_mask", c_void_p), ("n_correspondences", c_int), ("n_bad", c_int),
                ("n_inliers", c_int), ("rounds_run", c_int), ("flags", c_uint32), ("sim3_q_t_s", c_double * 8),
                ("s12_rt", c_float * 12), ("scw", c_float * 12), ("rounds", poseopt_round * 2)]


class lba_problem(Structure):  # orbfe_lba.h
    _fields_ = [("n_kf", c_int), ("n_points", c_int), ("n_edges", c_int), ("tcw", c_void_p), ("k", c_void_p),
                ("bf", c_void_p), ("fixed", c_void_p), ("xw", c_void_p), ("edge_begin", c_void_p), ("edge_kf", c_void_p),
                ("kp_un", c_void_p), ("u_right", c_void_p), ("inv_sigma2", c_void_p), ("stop_flag", c_void_p),
                ("stop_at_poll", c_int)]


class lba_round(Structure):
    _fields_ = [("n_active", c_int), ("iterations", c_int), ("trials", c_int), ("rejected_trials", c_int),
                ("stop", c_int), ("n_flagged", c_int), ("lam", c_double), ("chi2", c_double)]


class lba_result(Structure):
    _fields_ = [("tcw", c_void_p), ("xw", c_void_p), ("mask_words", c_int), ("erase_mask", c_void_p),
                ("level1_mask", c_void_p), ("n_erase", c_int), ("rounds_run", c_int), ("flags", c_uint32),
                ("polls", c_int), ("rounds", lba_round * 2)]


LBA_MAX_FREE_KF, LBA_MAX_KF, LBA_MAX_POINTS, LBA_MAX_EDGES = 128, 512, 16384, 131072  # orbfe_lba.h


class gba_problem(Structure):  # orbfe_gba.h
    _fields_ = [("n_kf", c_int), ("n_points", c_int), ("n_edges", c_int), ("tcw", c_void_p), ("k", c_void_p),
                ("bf", c_void_p), ("fixed", c_void_p), ("xw", c_void_p), ("edge_begin", c_void_p), ("edge_kf", c_void_p),
                ("kp_un", c_void_p), ("u_right", c_void_p), ("inv_sigma2", c_void_p), ("n_iterations", c_int),
                ("robust", c_int), ("stop_flag", c_void_p), ("stop_at_poll", c_int)]


class gba_trace(Structure):
    _fields_ = [("n_active", c_int), ("iterations", c_int), ("trials", c_int), ("rejected_trials", c_int),
                ("stop", c_int), ("lam", c_double), ("chi2", c_double), ("env_blocks", c_int), ("schur_blocks", c_int),
                ("flags", c_uint32), ("polls", c_int)]


class gba_result(Structure):
    _fields_ = [("tcw", c_void_p), ("xw", c_void_p), ("trace", gba_trace)]


GBA_MAX_KF, GBA_MAX_POINTS, GBA_MAX_EDGES, GBA_MAX_ENV_BLOCKS = 4096, 524288, 4194304, 2097152  # orbfe_gba.h
GBA_MAX_ITERATIONS = 64
GBA_FLAG_LARGE_STEP, GBA_FLAG_NONFINITE = 1, 2
GBA_STOP_ALL, GBA_STOP_TERMINATE, GBA_STOP_NBAD, GBA_STOP_NO_EDGE, GBA_STOP_FLAG = 0, 1, 2, 3, 4


class mapcorr_points(Structure):  # orbfe_mapcorr.h
    _fields_ = [("n_points", c_int), ("n_obs", c_int), ("n_levels", c_int), ("scale_factors", c_void_p),
                ("xw", c_void_p), ("bad", c_void_p), ("obs_begin", c_void_p), ("obs_kf", c_void_p),
                ("ref_kf", c_void_p), ("ref_level", c_void_p)]


class mapcorr_normals(Structure):
    _fields_ = [("normal", c_void_p), ("max_dist", c_void_p), ("min_dist", c_void_p), ("updated", c_void_p)]


class mapcorr_normals_problem(Structure):
    _fields_ = [("n_kf", c_int), ("ow", c_void_p), ("points", mapcorr_points)]


class mapcorr_loop_problem(Structure):
    _fields_ = [("n_kf", c_int), ("tcw", c_void_p), ("n_connected", c_int), ("connected_kf", c_void_p), ("cur", c_int),
                ("scw", c_void_p), ("n_slots", c_int), ("row_begin", c_void_p), ("row_point", c_void_p),
                ("points", mapcorr_points)]


class mapcorr_loop_result(Structure):
    _fields_ = [("noncorrected_sim3", c_void_p), ("corrected_sim3", c_void_p), ("tcw_out", c_void_p),
                ("xw_out", c_void_p), ("corrected_by", c_void_p), ("normals", mapcorr_normals)]


class mapcorr_gba_problem(Structure):
    _fields_ = [("n_kf", c_int), ("tcw", c_void_p), ("tcw_gba", c_void_p), ("optimised", c_void_p),
                ("parent", c_void_p), ("n_points", c_int), ("xw", c_void_p), ("bad", c_void_p),
                ("pt_optimised", c_void_p), ("xw_gba", c_void_p), ("ref_kf", c_void_p)]


class mapcorr_gba_result(Structure):
    _fields_ = [("tcw_out", c_void_p), ("propagated", c_void_p), ("xw_out", c_void_p), ("pt_changed", c_void_p),
                ("levels", c_int)]


MAPCORR_MAX_KF, MAPCORR_MAX_POINTS, MAPCORR_MAX_EDGES, MAPCORR_MAX_LEVELS = 8192, 1048576, 16777216, 64  # orbfe_mapcorr.h


class essgraph_problem(Structure):  # orbfe_essgraph.h
    _fields_ = [("n_vertices", c_int), ("tcw", c_void_p), ("fixed_vertex", c_int), ("fix_scale", c_int),
                ("n_corrected", c_int), ("corrected_idx", c_void_p), ("corrected_sim3", c_void_p),
                ("n_noncorrected", c_int), ("noncorrected_idx", c_void_p), ("noncorrected_sim3", c_void_p),
                ("n_edges", c_int), ("edge_i", c_void_p), ("edge_j", c_void_p), ("edge_kind", c_void_p),
                ("n_points", c_int), ("xw", c_void_p), ("point_ref", c_void_p)]


class essgraph_trace(Structure):
    _fields_ = [("iterations", c_int), ("trials", c_int), ("rejected_trials", c_int), ("stop", c_int),
                ("lam", c_double), ("chi2", c_double), ("env_blocks", c_int), ("flags", c_uint32)]


class essgraph_result(Structure):
    _fields_ = [("tcw", c_void_p), ("xw", c_void_p), ("trace", essgraph_trace)]


ESSGRAPH_MAX_VERTICES, ESSGRAPH_MAX_EDGES, ESSGRAPH_MAX_ENV_BLOCKS, ESSGRAPH_MAX_POINTS = 8192, 65536, 524288, 1048576
ESSGRAPH_FLAG_LARGE_STEP, ESSGRAPH_FLAG_NONFINITE = 1, 2
ESSGRAPH_STOP_ALL, ESSGRAPH_STOP_TERMINATE, ESSGRAPH_STOP_NBAD, ESSGRAPH_STOP_NO_EDGE = 0, 1, 2, 3
LBA_FLAG_LARGE_STEP, LBA_FLAG_NONFINITE = 1, 2
LBA_STOP_ALL, LBA_STOP_TERMINATE, LBA_STOP_NBAD, LBA_STOP_NO_EDGE, LBA_STOP_FLAG = 0, 1, 2, 3, 4

POSEOPT_FLAG_LARGE_STEP, POSEOPT_FLAG_NONFINITE = 1, 2  # orbfe_poseopt.h: deviation flags of one problem
POSEOPT_STOP_ALL, POSEOPT_STOP_TERMINATE, POSEOPT_STOP_NBAD, POSEOPT_STOP_NO_EDGE = 0, 1, 2, 3


class tri_keyframe(Structure):  # orbfe_triangulate.h
    _fields_ = [("tcw", c_float * 12), ("ow", c_float * 3), ("depth", c_void_p), ("keys_xy", c_void_p)]


class tri_pair(Structure):
    _fields_ = [("kf1", frame_view), ("kf2", frame_view), ("t1", tri_keyframe), ("t2", tri_keyframe),
                ("match12", c_void_p), ("kf1_n_dev", c_void_p), ("status", c_void_p), ("x3d", c_void_p),
                ("nnew", c_void_p), ("mark1", c_void_p), ("mark2", c_void_p)]


class tri_neighbour(Structure):
    _fields_ = [("kf", frame_view), ("t", tri_keyframe), ("fv", feature_vector), ("f12", c_float * 9),
                ("ex", c_float), ("ey", c_float)]


# orbfe_triangulate.h: status codes of one match
TRI_NO_MATCH, TRI_TRIANGULATED, TRI_STEREO1, TRI_STEREO2 = 0, 1, 2, 3
TRI_REJ_PARALLAX, TRI_REJ_W_ZERO, TRI_REJ_Z1, TRI_REJ_Z2, TRI_REJ_REPROJ1, TRI_REJ_REPROJ2 = -1, -2, -3, -4, -5, -6
TRI_REJ_DIST_ZERO, TRI_REJ_SCALE, TRI_REJ_UNPROJECT, TRI_REJ_BAD_MATCH, TRI_REJ_BAD_OCTAVE = -7, -8, -9, -10, -11
TRI_MAX_KEYS, TRI_MAX_KF2_KEYS, TRI_MAX_PAIRS, TRI_MAX_NEIGHBOURS = 8192, 16384, 4096, 64


GRAY_SHIFT15, GRAY_SHIFT14 = 0, 1  # orbfe_frame.h: cvtColor's 4.x / 2.4-3.x tables
DEPTH_U16, DEPTH_F32 = 0, 1
# orbfe_rectify.h: one destination pixel of a rectification plan
RECTIFY_ENTRY_DTYPE = np.dtype([("ix", "<i2"), ("iy", "<i2"), ("alpha", "<u2"), ("outside", "<u2")])


class camera(Structure):  # orbfe_frame.h
    _fields_ = [("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float), ("dist", c_float * 5),
                ("n_dist", c_int32), ("bf", c_float)]


def make_camera(fx, fy, cx, cy, dist, bf) -> camera:
    """mK, mDistCoef (k1, k2, p1, p2[, k3]) and mbf as an orbfe_camera."""
    d = [float(v) for v in np.asarray(dist, np.float32).reshape(-1)]
    if len(d) not in (4, 5):
        raise ValueError("mDistCoef has 4 or 5 entries")
    c = camera(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), n_dist=len(d), bf=float(bf))
    for i, v in enumerate(d):
        c.dist[i] = v
    return c


GRIDMAP_REFERENCE, GRIDMAP_INTENDED = 0, 1  # orbfe_gridmap.h: the two rule sets
GRIDMAP_SEGMENT, GRIDMAP_MAX_KEYFRAMES, GRIDMAP_MAX_POINTS = 64, 4096, 8192


class gridmap_geometry(Structure):  # orbfe_gridmap.h
    _fields_ = [("scale_factor", c_int32), ("min_x", c_float), ("max_x", c_float), ("min_z", c_float),
                ("max_z", c_float), ("visit_threshold", c_int32)]


class gridmap_stats(Structure):
    _fields_ = [("beams", ctypes.c_int64), ("visits", ctypes.c_int64), ("dropped", ctypes.c_int64),
                ("points_cut", ctypes.c_int64), ("kf_outside", c_int32), ("row0", c_int32), ("row1", c_int32)]


# name -> (restype, argtypes)
_SIGNATURES = {
    "orbfe_last_error": (c_char_p, []),
    "orbfe_version": (c_char_p, []),
    "orbfe_extractor_create": (c_int, [c_int, c_float, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_extractor_destroy": (c_int, [c_void_p]),
    "orbfe_extractor_set_resize_mode": (c_int, [c_void_p, c_int]),
    "orbfe_get_scale_tables": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "orbfe_max_keypoints": (c_int, [c_void_p, c_int, c_int]),
    "orbfe_extract": (c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_void_p, c_int, c_void_p,
                              POINTER(c_int)]),
    "orbfe_extract_batch": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_size_t, c_void_p,
                                    c_void_p, c_int, c_void_p]),
    "orbfe_extract_batch_device": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_int, c_int,
                                           c_size_t, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "orbfe_get_level": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p), POINTER(c_int),
                                POINTER(c_int), POINTER(c_size_t)]),
    "orbfe_get_level_device": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p), POINTER(c_int),
                                       POINTER(c_int), POINTER(c_size_t)]),
    "orbfe_extractor_set_host_pyramid": (c_int, [c_void_p, c_int]),
    "orbfe_extractor_set_graphs": (c_int, [c_void_p, c_int]),
    "orbfe_debug_graph_stats": (c_int, [c_void_p, c_void_p]),
    "orbfe_ktimer_select": (c_int, [ctypes.c_char_p]),
    "orbfe_ktimer_read": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, POINTER(c_int)]),
    "orbfe_ktimer_reset": (c_int, []),
    "orbfe_ktimer_calibrate": (c_int, [c_int, c_int, POINTER(c_double)]),
    "orbfe_extractor_stream": (c_void_p, [c_void_p]),
    "orbfe_extractor_pyramid_event": (c_void_p, [c_void_p]),
    "orbfe_stream_wait_event": (c_int, [c_void_p, c_void_p]),
    "orbfe_event_create": (c_int, [c_int, POINTER(c_void_p)]),
    "orbfe_event_record": (c_int, [c_void_p, c_void_p]),
    "orbfe_event_destroy": (c_int, [c_void_p]),
    "orbfe_event_query": (c_int, [c_void_p]),
    "orbfe_matcher_set_profiling": (c_int, [c_void_p, c_int]),
    "orbfe_matcher_last_device_ms": (c_int, [c_void_p, POINTER(c_float)]),
    "orbfe_debug_matcher_sweep_stats": (c_int, [c_void_p, c_void_p]),
    "orbfe_debug_matcher_set_sweep": (c_int, [c_void_p, c_int, c_int, c_int]),
    "orbfe_host_register": (c_int, [c_void_p, c_size_t]),
    "orbfe_host_unregister": (c_int, [c_void_p]),
    "orbfe_stream_create": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "orbfe_stream_create_masked": (c_int, [c_int, c_void_p, c_int, POINTER(c_void_p)]),
    "orbfe_stream_destroy": (c_int, [c_void_p]),
    "orbfe_matcher_create": (c_int, [c_float, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_matcher_destroy": (c_int, [c_void_p]),
    "orbfe_matcher_stream": (c_void_p, [c_void_p]),
    "orbfe_matcher_last_stats": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "orbfe_matcher_set_max_rounds": (c_int, [c_void_p, c_int]),
    "orbfe_descriptor_distance": (c_int, [c_void_p, c_void_p]),
    "orbfe_descriptor_distance_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "orbfe_search_by_projection_local": (c_int, [c_void_p, POINTER(frame_view),
                                                 POINTER(local_mappoints), c_float, c_void_p,
                                                 POINTER(c_int)]),
    "orbfe_search_by_projection_lastframe": (c_int, [c_void_p, POINTER(frame_view),
                                                     POINTER(lastframe_mappoints), c_void_p,
                                                     c_float, c_int, c_void_p, POINTER(c_int)]),
    "orbfe_search_for_triangulation": (c_int, [c_void_p, POINTER(frame_view), POINTER(frame_view),
                                               POINTER(feature_vector), POINTER(feature_vector),
                                               c_void_p, c_float, c_float, c_int, c_void_p,
                                               POINTER(c_int)]),
    "orbfe_search_for_triangulation_batch_device": (c_int, [c_void_p, c_int, c_void_p, c_int,
                                                            c_void_p]),
    "orbfe_debug_get_candidates": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, POINTER(c_int)]),
    "orbfe_debug_candidate_total": (c_int, [c_void_p, POINTER(ctypes.c_longlong)]),
    "orbfe_debug_get_level_keys": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, POINTER(c_int)]),
    "orbfe_debug_get_blurred": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int]),
    "orbfe_debug_geometry": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int]),
    "orbfe_debug_set_octree_key_cap": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_fast_side_levels": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_octree_split": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_latency_schedule": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_octree_threads": (c_int, [c_void_p, c_int, c_int]),
    "orbfe_debug_set_octree_threads_l0": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_octree_serial": (c_int, [c_void_p, c_int, c_int]),
    "orbfe_debug_set_pyramid_tiles": (c_int, [c_void_p, c_int, c_int, c_int, c_int]),
    "orbfe_debug_set_zero_copy": (c_int, [c_void_p, c_int, c_int]),
    "orbfe_debug_set_schedule_autotune": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_fast_side_merge": (c_int, [c_void_p, c_int]),
    "orbfe_debug_schedule_choice": (c_int, [c_void_p, c_int]),
    "orbfe_debug_set_octree_lds": (c_int, [c_void_p, c_int, c_int]),
    "orbfe_debug_set_fast_wpb": (c_int, [c_void_p, c_int, c_int]),
    "orbfe_debug_set_inline_side": (c_int, [c_void_p, c_int]),
    "orbfe_set_side_stream": (c_int, [c_void_p, c_void_p]),
    "orbfe_debug_set_blur_mode": (c_int, [c_void_p, c_int]),
    "orbfe_debug_get_umax": (c_int, [c_void_p, c_void_p]),
    "orbfe_debug_steer_trig": (c_int, [c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
    "orbfe_vocab_create": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_int, POINTER(c_void_p)]),
    "orbfe_vocab_load_text": (c_int, [c_char_p, c_int, POINTER(c_void_p)]),
    "orbfe_vocab_load_binary": (c_int, [c_char_p, c_int, POINTER(c_void_p)]),
    "orbfe_vocab_get_info": (c_int, [c_void_p, c_void_p]),
    "orbfe_vocab_export": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "orbfe_vocab_destroy": (c_int, [c_void_p]),
    # orbfe_pack.h
    "orbfe_packed_bytes": (c_size_t, [c_int, ctypes.c_longlong]),
    "orbfe_pack_keypoints_device": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                            c_size_t, c_void_p, c_void_p]),
    "orbfe_vocab_transform": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                      POINTER(c_int), c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "orbfe_vocab_transform_batch_device": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p,
                                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "orbfe_compute_stereo_matches_batch_device": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p,
                                                          c_void_p, c_void_p, c_int, c_float,
                                                          c_float, c_void_p, c_void_p, c_void_p]),
    "orbfe_compute_stereo_matches": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p,
                                             c_void_p, c_int, c_void_p, c_void_p, c_int, c_float,
                                             c_float, c_void_p, c_void_p]),
    "orbfe_stereo_frame": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_size_t, c_float,
                                   c_float, c_void_p, c_void_p, POINTER(c_int), c_void_p, c_void_p,
                                   POINTER(c_int), c_int, c_void_p, c_void_p]),
    # orbfe_frame.h
    "orbfe_image_bounds": (c_int, [POINTER(camera), c_int, c_int, c_void_p]),
    "orbfe_gray_batch_device": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_size_t, c_int, c_int, c_int, c_int,
                                        c_int, c_void_p, c_size_t, c_size_t, c_void_p]),
    "orbfe_frame_finish_batch_device": (c_int, [c_void_p, c_int, POINTER(camera), c_void_p, c_void_p, c_int,
                                                c_void_p, c_size_t, c_size_t, c_int, c_float, c_int, c_int,
                                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "orbfe_undistort_keypoints_host": (c_int, [POINTER(camera), c_void_p, c_int, c_void_p]),
    "orbfe_stereo_from_depth_host": (c_int, [POINTER(camera), c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int,
                                             c_float, c_int, c_int, c_void_p, c_void_p]),
    "orbfe_mono_frame": (c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_int, c_int, c_int, POINTER(camera),
                                 c_void_p, c_void_p, POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p]),
    "orbfe_rgbd_frame": (c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_int, c_int, c_int, c_void_p,
                                 c_size_t, c_int, c_float, POINTER(camera), c_void_p, c_void_p, POINTER(c_int),
                                 c_int, c_void_p, c_void_p, c_void_p]),
    "orbfe_rectify_maps_host": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                        c_void_p]),
    "orbfe_remap_host": (c_int, [c_void_p, c_int, c_int, c_size_t, c_int, c_void_p, c_void_p, c_size_t, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    "orbfe_rectify_entries_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "orbfe_rectify_plan_create": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_int, POINTER(c_void_p)]),
    "orbfe_rectify_plan_destroy": (None, [c_void_p]),
    "orbfe_rectify_plan_read": (c_int, [c_void_p, c_int, c_void_p]),
    "orbfe_rectify_batch_device": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_int,
                                           c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_size_t,
                                           c_void_p]),
    "orbfe_rectified_stereo_frame": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_size_t, c_int,
                                             c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                             POINTER(c_int), c_void_p, c_void_p, POINTER(c_int), c_int, c_void_p,
                                             c_void_p]),
    "orbfe_is_in_frustum": (c_int, [c_void_p, POINTER(frame_view), POINTER(mappoint_geometry),
                                    c_void_p, c_float, c_float, POINTER(frustum_out),
                                    POINTER(c_int)]),
    "orbfe_search_local_points": (c_int, [c_void_p, POINTER(frame_view),
                                          POINTER(mappoint_geometry), c_void_p, c_float, c_float,
                                          c_float, c_void_p, POINTER(c_int), POINTER(frustum_out),
                                          POINTER(c_int)]),
    "orbfe_synth_frame": (c_int, [c_uint64, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t]),
    "orbfe_synth_sequence_frame": (c_int, [c_uint64, ctypes.c_longlong, c_int, c_int, c_float, c_float, c_float,
                                           c_float, c_float, c_float, c_void_p, c_void_p, c_size_t]),
    # orbfe_keyframe.h
    "orbfe_search_by_bow_kf_frame": (c_int, [c_void_p, POINTER(frame_view), POINTER(feature_vector),
                                             POINTER(frame_view), POINTER(feature_vector), c_void_p,
                                             POINTER(c_int)]),
    "orbfe_search_by_bow_kf_frame_multi": (c_int, [c_void_p, c_int, c_void_p, c_void_p,
                                                   POINTER(frame_view), POINTER(feature_vector),
                                                   c_void_p, c_void_p]),
    "orbfe_search_by_bow_kf_kf": (c_int, [c_void_p, POINTER(frame_view), POINTER(feature_vector),
                                          POINTER(frame_view), POINTER(feature_vector), c_void_p,
                                          POINTER(c_int)]),
    "orbfe_search_by_projection_keyframe": (c_int, [c_void_p, POINTER(frame_view), c_void_p,
                                                    POINTER(mappoint_geometry), c_void_p, c_float,
                                                    c_float, c_int, c_void_p, POINTER(c_int)]),
    "orbfe_search_by_projection_sim3": (c_int, [c_void_p, POINTER(frame_view), c_void_p,
                                                POINTER(mappoint_geometry), c_float, c_int,
                                                c_void_p, POINTER(c_int)]),
    "orbfe_fuse": (c_int, [c_void_p, POINTER(frame_view), c_void_p, c_void_p,
                           POINTER(mappoint_geometry), c_float, c_float, c_void_p, POINTER(c_int)]),
    "orbfe_fuse_sim3": (c_int, [c_void_p, POINTER(frame_view), c_void_p, POINTER(mappoint_geometry),
                                c_float, c_float, c_void_p, POINTER(c_int)]),
    "orbfe_search_by_sim3": (c_int, [c_void_p, POINTER(frame_view), POINTER(frame_view),
                                     POINTER(mappoint_geometry), POINTER(mappoint_geometry),
                                     c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_float,
                                     c_float, c_float, c_void_p, POINTER(c_int)]),
    "orbfe_search_for_initialization": (c_int, [c_void_p, POINTER(frame_view), POINTER(frame_view),
                                                c_void_p, c_int, c_void_p, POINTER(c_int)]),
    "orbfe_compute_distinctive_descriptors": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "orbfe_compute_distinctive_descriptors_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p,
                                                             c_void_p, c_void_p]),
    "orbfe_predict_scale_thresholds": (c_int, [c_float, c_int, c_void_p]),
    # orbfe_c3.h
    "orbfe_c3_create": (c_int, [POINTER(c3_config), c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                c_void_p, c_int, POINTER(c_void_p)]),
    "orbfe_c3_run": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]),
    "orbfe_c3_finish": (c_int, [c_void_p, c_int, c_void_p]),
    "orbfe_c3_match_stream": (c_void_p, [c_void_p, c_int]),
    "orbfe_c3_destroy": (c_int, [c_void_p]),
    # orbfe_kfdb.h
    "orbfe_kfdb_create": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_kfdb_destroy": (c_int, [c_void_p]),
    "orbfe_kfdb_add": (c_int, [c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int]),
    "orbfe_kfdb_add_batch_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int, c_void_p]),
    "orbfe_kfdb_erase": (c_int, [c_void_p, ctypes.c_int64]),
    "orbfe_kfdb_clear": (c_int, [c_void_p]),
    "orbfe_kfdb_size": (c_int, [c_void_p, POINTER(c_int)]),
    "orbfe_kfdb_set_covisible": (c_int, [c_void_p, ctypes.c_int64, c_void_p, c_int]),
    "orbfe_kfdb_query": (c_int, [c_void_p, POINTER(kfdb_query), POINTER(kfdb_result)]),
    # orbfe_sim3.h
    "orbfe_sim3_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_sim3_destroy": (c_int, [c_void_p]),
    "orbfe_sim3_solve_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "orbfe_sim3_iterate": (c_int, [c_void_p, c_int, c_int, POINTER(sim3_state), POINTER(sim3_iterate)]),
    # orbfe_pnp.h
    "orbfe_pnp_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_pnp_destroy": (c_int, [c_void_p]),
    "orbfe_pnp_solve_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "orbfe_pnp_iterate": (c_int, [c_void_p, c_int, c_int, POINTER(pnp_state), POINTER(pnp_iterate)]),
    # orbfe_init.h
    "orbfe_init_create": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_init_destroy": (c_int, [c_void_p]),
    "orbfe_init_solve_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    # orbfe_covis.h
    "orbfe_covis_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_covis_destroy": (c_int, [c_void_p]),
    "orbfe_covis_set_keyframe": (c_int, [c_void_p, ctypes.c_int64, c_uint64, c_int, c_void_p]),
    "orbfe_covis_set_slots": (c_int, [c_void_p, ctypes.c_int64, c_int, c_void_p, c_void_p]),
    "orbfe_covis_erase_keyframe": (c_int, [c_void_p, ctypes.c_int64]),
    "orbfe_covis_set_points_bad": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "orbfe_covis_clear": (c_int, [c_void_p]),
    "orbfe_covis_size": (c_int, [c_void_p, POINTER(c_int)]),
    "orbfe_covis_update_connections": (c_int, [c_void_p, c_int, c_void_p, c_int, POINTER(covis_connections)]),
    "orbfe_covis_vote": (c_int, [c_void_p, c_int, c_void_p, c_void_p, POINTER(covis_votes)]),
    "orbfe_covis_local_map": (c_int, [c_void_p, c_int, c_void_p, POINTER(covis_local_map)]),
    "orbfe_covis_set_keyframe_attrs": (c_int, [c_void_p, ctypes.c_int64, c_int, c_void_p]),
    "orbfe_covis_cull_keyframes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, POINTER(covis_cull)]),
    "orbfe_covis_cull_points": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64,
                                        c_int, c_void_p]),
    # orbfe_localmap.h
    "orbfe_covis_distinct_points": (c_int, [c_void_p, c_int, c_void_p, POINTER(covis_points)]),
    "orbfe_covis_set_point_geometry": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p]),
    "orbfe_covis_local_geometry": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p,
                                           POINTER(covis_local_geometry)]),
    # orbfe_gridmap.h
    "orbfe_gridmap_default_geometry": (c_int, [POINTER(gridmap_geometry)]),
    "orbfe_gridmap_dims": (c_int, [POINTER(gridmap_geometry), POINTER(c_int32), POINTER(c_int32), POINTER(c_float),
                                   POINTER(c_float)]),
    "orbfe_gridmap_create": (c_int, [c_int, POINTER(gridmap_geometry), c_int, POINTER(c_void_p)]),
    "orbfe_gridmap_destroy": (c_int, [c_void_p]),
    "orbfe_gridmap_reset": (c_int, [c_void_p]),
    "orbfe_gridmap_update": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, POINTER(gridmap_stats)]),
    "orbfe_gridmap_update_resident": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(gridmap_stats),
                                              POINTER(c_int32)]),
    "orbfe_gridmap_build": (c_int, [c_void_p, c_int]),
    "orbfe_gridmap_download": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "orbfe_gridmap_download_counters": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "orbfe_gridmap_upload_counters": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "orbfe_gridmap_probability": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "orbfe_gridmap_host_update": (c_int, [POINTER(gridmap_geometry), c_int, c_void_p, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, POINTER(gridmap_stats)]),
    "orbfe_gridmap_host_build": (c_int, [POINTER(gridmap_geometry), c_void_p, c_void_p, c_int, c_int, c_void_p,
                                         c_void_p]),
    # orbfe_poseopt.h
    "orbfe_poseopt_create": (c_int, [c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_poseopt_destroy": (c_int, [c_void_p]),
    "orbfe_poseopt_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    # orbfe_lba.h
    "orbfe_lba_create": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_lba_destroy": (c_int, [c_void_p]),
    "orbfe_lba_solve": (c_int, [c_void_p, c_void_p, c_void_p]),
    # orbfe_gba.h
    "orbfe_gba_create": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_gba_destroy": (c_int, [c_void_p]),
    "orbfe_gba_solve": (c_int, [c_void_p, c_void_p, c_void_p]),
    "orbfe_gba_envelope": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    # orbfe_mapcorr.h
    "orbfe_mapcorr_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_mapcorr_destroy": (c_int, [c_void_p]),
    "orbfe_mapcorr_update_normal_depth": (c_int, [c_void_p, c_void_p, c_void_p]),
    "orbfe_mapcorr_correct_loop": (c_int, [c_void_p, c_void_p, c_void_p]),
    "orbfe_mapcorr_apply_gba": (c_int, [c_void_p, c_void_p, c_void_p]),
    # orbfe_essgraph.h
    "orbfe_essgraph_create": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_essgraph_destroy": (c_int, [c_void_p]),
    "orbfe_essgraph_solve": (c_int, [c_void_p, c_void_p, c_void_p]),
    # orbfe_optsim3.h
    "orbfe_optsim3_create": (c_int, [c_int, c_int, c_int, POINTER(c_void_p)]),
    "orbfe_optsim3_destroy": (c_int, [c_void_p]),
    "orbfe_optsim3_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    # orbfe_triangulate.h
    "orbfe_triangulate_matches": (c_int, [c_void_p, POINTER(frame_view), POINTER(tri_keyframe),
                                          POINTER(frame_view), POINTER(tri_keyframe), c_void_p, c_void_p,
                                          c_void_p, POINTER(c_int)]),
    "orbfe_triangulate_batch_device": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "orbfe_create_new_mappoints_device": (c_int, [c_void_p, POINTER(frame_view), POINTER(tri_keyframe),
                                                  POINTER(feature_vector), c_int, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# symbols declared in include/*.h (checked by tests/test_library.py)
EXPORTED = sorted(_SIGNATURES)

_lib = None


def lib() -> ctypes.CDLL:
    """Load liborbfe.so once (raises LibraryMissing if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (or make -C orb_slam2_2021_amd/csrc)")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        ab_build = "ORBFE_LIB" in os.environ  # an A/B build may predate newer entry points
        for name, (res, args) in _SIGNATURES.items():
            if ab_build and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    try:
        s = lib().orbfe_last_error()
    except Exception:  # pragma: no cover
        return "<no library>"
    return s.decode() if s else ""


def check(status: int, what: str) -> int:
    if status < 0:
        raise OrbfeError(status, what)
    return status


def ptr(a) -> c_void_p:
    """Address of a numpy array (contiguous) or an int device pointer."""
    if a is None:
        return c_void_p(0)
    if isinstance(a, int):
        return c_void_p(a)
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):  # torch tensor (device plumbing)
        return c_void_p(a.data_ptr())
    raise TypeError(f"cannot take the address of {type(a)}")


# ---- process-wide kernel timer (orbfe_ktimer_*, include/orbfe.h) ----------------------------------
def ktimer_select(kernels) -> None:
    """Time these kernels' launches by their own dispatch interval (what rocprofv3's kernel trace
    reports): an iterable of names ("k_fast", ...), "*" / True for every kernel, None / False /
    empty for none."""
    if kernels is True:
        v = "*"
    elif not kernels:
        v = ""
    elif isinstance(kernels, str):
        v = kernels
    else:
        v = ",".join(kernels)
    check(lib().orbfe_ktimer_select(v.encode()), "ktimer_select")


def ktimer_read() -> dict:
    """{kernel: (total ms, launches)} of every kernel timed so far (synchronises)."""
    cap, name_len = 64, 48
    names = ctypes.create_string_buffer(cap * name_len)
    total = np.zeros(cap, np.float64)
    launches = np.zeros(cap, np.int64)
    n = c_int()
    check(lib().orbfe_ktimer_read(names, name_len, ptr(total), ptr(launches), cap, ctypes.byref(n)),
          "ktimer_read")
    out = {}
    for k in range(n.value):
        nm = names.raw[k * name_len:(k + 1) * name_len].split(b"\0", 1)[0].decode()
        if launches[k] > 0:
            out[nm] = (float(total[k]), int(launches[k]))
    return out


def ktimer_reset() -> None:
    check(lib().orbfe_ktimer_reset(), "ktimer_reset")


def ktimer_calibrate(device: int = 0, n: int = 64) -> float:
    """The timer's per-dispatch overhead in microseconds (orbfe_ktimer_calibrate)."""
    v = c_double()
    check(lib().orbfe_ktimer_calibrate(int(device), int(n), byref(v)), "ktimer_calibrate")
    return float(v.value)
