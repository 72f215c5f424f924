"""orb_slam2_2021_amd -- MI355X-native ORB front-end for ORB-SLAM2 (lreithmayr/ORB_SLAM2_2021).

The product is liborbfe.so (HIP kernels for gfx950 behind the C ABI in include/orbfe.h); this
package is its host-side mirror of the reference's ORBextractor / ORBmatcher interfaces.
"""
from ._lib import (KEYPOINT_DTYPE, LIB_PATH, LibraryMissing, OrbfeError, ORBFE_MP_BAD, ORBFE_MP_NONE,
                   ORBFE_MP_OBSERVED, ORBFE_MP_PRESENT, ORBFE_RESIZE_SCALAR, ORBFE_RESIZE_SIMD128,
                   MPF_BAD, MPF_OBSERVED, MPF_OUTLIER, MPF_PRESENT, MPF_SEEN, MPF_SKIP,
                   MPF_TRACK_IN_VIEW)
from .covisibility import CovisibilityGraph
from .essential_graph import EssentialGraphOptimizer, OptimizeEssentialGraph, problem_of_essential_graph
from .extractor import ORBextractor, register_host, synth_frame, synth_sequence_frame, unregister_host
from .frames import (DeviceTriKeyFrame, FeatureVector, Frame, KeyFrame, KeyFrameMapPoints, LastFrameMapPoints,
                     LocalMapPoints, MapPointGeometry, ResidentLocalMap, TriKeyFrame)
from .initializer import Initializer, InitializerBatch
from .keyframe_database import KeyFrameDatabase, SharingList
from .global_bundle_adjustment import GlobalBundleAdjuster, GlobalBundleAdjustment, problem_of_map
from .local_bundle_adjustment import LocalBundleAdjuster, LocalBundleAdjustment, problem_of_local_map
from .map_correction import (ApplyGlobalBundleAdjustment, CorrectLoopPoses, MapCorrector, UpdateNormalAndDepth,
                             gba_update_problem_of_map, loop_problem_of_map, normals_problem_of_map)
from .matcher import ORBmatcher
from .occupancy_grid import GridStats, OccupancyGrid
from .rectify import StereoRectifier, rectify_entries_host, rectify_maps_host, remap_host
from .pnp_solver import PnPBatch, PnPsolver
from .pose_optimization import PoseOptimization, PoseOptimizer
from .sim3_optimization import OptimizeSim3, Sim3Optimizer, problem_of_keyframes
from .sim3_solver import Sim3Batch, Sim3Solver, solve_batch

__all__ = ["StereoRectifier", "rectify_maps_host", "remap_host", "rectify_entries_host", "OccupancyGrid", "GridStats", "ORBextractor", "ORBmatcher", "KeyFrameDatabase", "SharingList", "CovisibilityGraph", "Sim3Solver", "Sim3Batch", "solve_batch", "PnPsolver", "PnPBatch", "Initializer", "InitializerBatch", "PoseOptimizer", "PoseOptimization", "Sim3Optimizer", "OptimizeSim3", "problem_of_keyframes", "LocalBundleAdjuster", "LocalBundleAdjustment", "problem_of_local_map", "GlobalBundleAdjuster", "GlobalBundleAdjustment", "problem_of_map", "EssentialGraphOptimizer", "OptimizeEssentialGraph", "problem_of_essential_graph", "MapCorrector", "UpdateNormalAndDepth", "CorrectLoopPoses", "ApplyGlobalBundleAdjustment", "normals_problem_of_map", "loop_problem_of_map", "gba_update_problem_of_map", "Frame", "KeyFrame",
           "TriKeyFrame", "DeviceTriKeyFrame",
           "FeatureVector", "LocalMapPoints", "LastFrameMapPoints", "MapPointGeometry", "ResidentLocalMap", "KeyFrameMapPoints", "KEYPOINT_DTYPE",
           "synth_frame", "synth_sequence_frame", "register_host", "unregister_host", "OrbfeError", "LibraryMissing"]
