/*
 * orbfe_mapcorr.h -- the map corrections that follow an optimiser, on the GPU (liborbfe.so, gfx950): new
 * poses applied to a map's points, and the points' viewing normal and scale-invariance distances
 * refreshed.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   MapPoint::UpdateNormalAndDepth                                     src/MapPoint.cc:360-401
 *   LoopClosing::CorrectLoop, from mvpCurrentConnectedKFs to SetPose   src/LoopClosing.cc:453-535
 *     (without the two UpdateConnections: orbfe_covis_update_connections; without the fusion: Fuse)
 *   LoopClosing::RunGlobalBundleAdjustment's map update                src/LoopClosing.cc:705-766
 *   KeyFrame::SetPose's Twc and Ow                                     src/KeyFrame.cc
 * The float algebra is cv::Mat's (DESIGN.md sections 15 and 16: the double-accumulating CV_32F gemm with
 * alpha and C, cv::norm with double squares, Mat / scalar as a product with (float)(1.0 / s)); the Sim3
 * algebra is g2o's over Eigen, as in orbfe_optsim3.h and orbfe_essgraph.h. Every result is defined bit
 * for bit by orb_slam2_2021_amd/csrc/orbfe_mapcorr_core.h.
 *
 * Keyframes and points are indices into the caller's arrays (INTEGRATION.md section 20 has the gathers).
 *
 * Carried as written:
 *  - UpdateNormalAndDepth returns early for a bad point and for a point without an observation: updated
 *    = 0 and normal / max_dist / min_dist keep what the caller's arrays held (the three are in/out);
 *  - the normal is summed from +0.0f over the point's observers in the order of its segment, which stands
 *    for the iteration of std::map<KeyFrame*, size_t>; a point at an observer's centre has norm 0, 1 / 0 =
 *    inf, 0 * inf = NaN, and the NaN stays in the normal;
 *  - ref_level is mvKeysUn[observations[pRefKF]].octave: when the reference keyframe is not an observer
 *    operator[] inserts slot 0, and the caller passes keypoint 0's octave;
 *  - CorrectLoop corrects a point once, by the first keyframe in the iteration order of CorrectedSim3 (the
 *    order of connected_kf) whose row holds it; the corrected position is computed from the input xw;
 *  - UpdateNormalAndDepth at LoopClosing.cc:519 runs inside the loop of list position r, before r's
 *    SetPose: for a point corrected at position r an observer (and likewise the reference keyframe) shows
 *    its new camera centre only if it is a connected keyframe at a position strictly below r, and its old
 *    centre otherwise, keyframe r itself included;
 *  - Sim3 never normalises its quaternion: corrected_sim3 holds Quaterniond(R) of the widened floats and
 *    products of such, tcw_out their toRotationMatrix() and t * (1. / s), narrowed per element;
 *  - RunGlobalBundleAdjustment propagates (Tcw_child * Twc_parent) * TcwGBA_parent in that association,
 *    Twc_parent from the parent's old pose, TcwGBA_parent the parent's possibly propagated value; a point
 *    that GBA did not optimise moves with its reference keyframe (Rcw_bef * X + tcw_bef, then Rwc * Xc +
 *    twc of the new pose's stored inverse).
 *
 * Deviations, deliberate: none in the arithmetic. The fourth row of a pose is taken as [0 0 0 1] (the
 * reference computes it; it is that for finite poses). mnCorrectedByKF is not read: every point counts as
 * not yet corrected by the current keyframe when the call begins.
 *
 * Out of scope, with the caller: the mnCorrectedByKF / mnCorrectedReference / mnBAGlobalForKF
 * bookkeeping, UpdateConnections, the fusion, the mutexes, InformNewBigChange.
 *
 * Bounds: 8,192 keyframes, 1,048,576 points, 16,777,216 observation entries and as many row slots, 64
 * pyramid levels. A handle holds device and pinned host memory for its own bounds: together about 0.7 KB
 * per keyframe, 160 bytes per point and 16 per edge. A handle is not thread-safe. Every call is one upload,
 * its kernels on the handle's one stream and one result copy with one synchronisation; no graph capture,
 * no environment setting.
 */
#ifndef ORBFE_MAPCORR_H
#define ORBFE_MAPCORR_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_mapcorr orbfe_mapcorr;

#define ORBFE_MAPCORR_MAX_KF 8192
#define ORBFE_MAPCORR_MAX_POINTS 1048576
#define ORBFE_MAPCORR_MAX_EDGES 16777216
#define ORBFE_MAPCORR_MAX_LEVELS 64

/* device < 0: a host-only handle (argument checks work, a call that gets past them returns
 * ORBFE_ERR_STATE). ORBFE_ERR_ARG below 1 or past the hard caps above. max_edges bounds the observation
 * entries and the row slots of a call, each. */
int orbfe_mapcorr_create(int device, int max_kf, int max_points, int max_edges, orbfe_mapcorr** out);
int orbfe_mapcorr_destroy(orbfe_mapcorr* h);

/* The points' side of UpdateNormalAndDepth, shared by calls 1 and 2 */
typedef struct {
  int n_points, n_obs, n_levels;
  const float* scale_factors;  /* [n_levels] mvScaleFactors */
  const float* xw;             /* [n_points*3] GetWorldPos() */
  const uint8_t* bad;          /* [n_points] isBad() */
  const int* obs_begin;        /* [n_points+1] point p's observers are obs_begin[p] .. obs_begin[p+1]-1 */
  const int* obs_kf;           /* [n_obs] index of the observing keyframe, in mObservations' order */
  const int* ref_kf;           /* [n_points] index of mpRefKF */
  const int* ref_level;        /* [n_points] mvKeysUn[observations[pRefKF]].octave */
} orbfe_mapcorr_points_t;

typedef struct {
  float* normal;     /* in/out [n_points*3] mNormalVector, written where updated */
  float* max_dist;   /* in/out [n_points] mfMaxDistance */
  float* min_dist;   /* in/out [n_points] mfMinDistance */
  uint8_t* updated;  /* out [n_points] */
} orbfe_mapcorr_normals_t;

/* Call 1: UpdateNormalAndDepth for every point. */
typedef struct {
  int n_kf;
  const float* ow;  /* [n_kf*3] GetCameraCenter() */
  orbfe_mapcorr_points_t points;
} orbfe_mapcorr_normals_problem_t;

/* ORBFE_ERR_CAPACITY past the handle's bounds; ORBFE_ERR_ARG for a null array, n_levels outside 1 .. 64,
 * an obs_begin that is not a CSR over n_obs, a keyframe index out of range and, on a point that is not bad
 * and has an observer, a ref_kf or a ref_level out of range. Nothing is written on an error. */
int orbfe_mapcorr_update_normal_depth(orbfe_mapcorr* h, const orbfe_mapcorr_normals_problem_t* problem,
                                      orbfe_mapcorr_normals_t* result);

/* Call 2: CorrectLoop. */
typedef struct {
  int n_kf;
  const float* tcw;         /* [n_kf*12] rows 0..2 of GetPose(), row-major */
  int n_connected;          /* 1 .. n_kf */
  const int* connected_kf;  /* [n_connected] mvpCurrentConnectedKFs in the iteration order of CorrectedSim3 */
  int cur;                  /* the position of mpCurrentKF in connected_kf */
  const double* scw;        /* [8] mg2oScw: q (x y z w), t, s */
  int n_slots;
  const int* row_begin;     /* [n_connected+1] position i's GetMapPointMatches() is row_begin[i] .. row_begin[i+1]-1 */
  const int* row_point;     /* [n_slots] point index, -1: none */
  orbfe_mapcorr_points_t points;
} orbfe_mapcorr_loop_problem_t;

typedef struct {
  double* noncorrected_sim3;  /* out [n_connected*8] as orbfe_essgraph_problem_t takes them */
  double* corrected_sim3;     /* out [n_connected*8] */
  float* tcw_out;             /* out [n_connected*12] what SetPose receives */
  float* xw_out;              /* out [n_points*3] what SetWorldPos receives; a point that is not corrected: its input */
  int* corrected_by;          /* out [n_points] list position of the correcting keyframe, -1: not corrected */
  orbfe_mapcorr_normals_t normals;  /* updated = 1 for a corrected point with an observer */
} orbfe_mapcorr_loop_result_t;

/* ORBFE_ERR_ARG in addition for n_connected outside 1 .. n_kf, a connected keyframe listed twice or out
 * of range, cur out of range, a row_begin that is not a CSR over n_slots, a row_point outside
 * -1 .. n_points-1. */
int orbfe_mapcorr_correct_loop(orbfe_mapcorr* h, const orbfe_mapcorr_loop_problem_t* problem,
                               orbfe_mapcorr_loop_result_t* result);

/* Call 3: the map update after GlobalBundleAdjustemnt. */
typedef struct {
  int n_kf;
  const float* tcw;          /* [n_kf*12] GetPose(): it becomes mTcwBefGBA */
  const float* tcw_gba;      /* [n_kf*12] mTcwGBA, read only where optimised */
  const uint8_t* optimised;  /* [n_kf] mnBAGlobalForKF == nLoopKF */
  const int* parent;         /* [n_kf] index of the spanning tree's parent, -1: in mvpKeyFrameOrigins */
  int n_points;
  const float* xw;              /* [n_points*3] */
  const uint8_t* bad;           /* [n_points] */
  const uint8_t* pt_optimised;  /* [n_points] mnBAGlobalForKF == nLoopKF */
  const float* xw_gba;          /* [n_points*3] mPosGBA, read only where pt_optimised */
  const int* ref_kf;            /* [n_points] index of GetReferenceKeyFrame(), -1: not in the list */
} orbfe_mapcorr_gba_problem_t;

typedef struct {
  float* tcw_out;       /* out [n_kf*12] what SetPose receives, for every keyframe */
  uint8_t* propagated;  /* out [n_kf] 1 where :716-721 ran */
  float* xw_out;        /* out [n_points*3]; an unchanged point: its input */
  uint8_t* pt_changed;  /* out [n_points] */
  int levels;           /* out: dependent steps of the propagation (1 + the longest run of keyframes that are not optimised) */
} orbfe_mapcorr_gba_result_t;

/* ORBFE_ERR_ARG for a null array, a parent or ref_kf out of range, a cycle or a self-parent, an origin
 * that is not optimised (the reference would SetPose an empty matrix). */
int orbfe_mapcorr_apply_gba(orbfe_mapcorr* h, const orbfe_mapcorr_gba_problem_t* problem,
                            orbfe_mapcorr_gba_result_t* result);

#ifdef __cplusplus
}
#endif
#endif
