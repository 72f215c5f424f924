/*
 * orbfe_lba.h -- Optimizer::LocalBundleAdjustment on the GPU (liborbfe.so, gfx950): the Levenberg-
 * Marquardt of one local map with the points marginalised by a Schur complement.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   Optimizer::LocalBundleAdjustment, from the optimizer's set-up on   src/Optimizer.cc:508-781
 *   Converter::toSE3Quat / toVector3d / toCvMat                        src/Converter.cc
 * and what it runs of g2o: VertexSE3Expmap, VertexSBAPointXYZ, EdgeSE3ProjectXYZ and
 * EdgeStereoSE3ProjectXYZ (computeError, linearizeOplus, isDepthPositive, cam_project),
 * BaseBinaryEdge::constructQuadraticForm, RobustKernelHuber, BlockSolver_6_3 (buildSystem, setLambda,
 * restoreDiagonal, the Schur branch of solve), OptimizationAlgorithmLevenberg (solve,
 * computeLambdaInit, computeScale) and SparseOptimizer (initializeOptimization(level), optimize, push,
 * pop, discardTop, update, activeRobustChi2). BundleAdjustment / GlobalBundleAdjustemnt, whose reduced
 * system is not dense-solvable, is orbfe_gba.h. OptimizeEssentialGraph is orbfe_essgraph.h.
 *
 * The caller performs the gather of Optimizer.cc:456-656: the keyframes
 * (local ones, then fixed cameras, each ascending in mnId) with GetPose(), fx fy cx cy, mbf and
 * fixed = (a fixed camera, or mnId == 0); the local map points ascending in mnId with GetWorldPos();
 * per point its observations, contiguous (edge_begin is a CSR over the points), each with the
 * keyframe's index, mvKeysUn[].pt, mvuRight[] (< 0: a monocular edge) and mvInvLevelSigma2[octave].
 *
 * Carried as written: the BA edges' Jacobians divide by z and z_2; an edge to a fixed keyframe adds to
 * its point's Hll and b only; round 1 is optimize(5) under Huber (deltas float(sqrt(5.991)),
 * float(sqrt(7.815))), then every edge with chi2 > 5.991 / 7.815 (double, >, so a NaN chi2 keeps the
 * edge) or a non-positive depth goes to level 1 and every kernel is removed, then optimize(10) over the
 * level-0 edges with lambda, _ni and _nBad re-initialised; a vertex without a level-0 edge is not in
 * round 2's system and keeps its estimate; chi2() reads the error of the last computeActiveErrors that
 * covered the edge (the round's last evaluated trial, accepted or not; round 1's for a level-1 edge)
 * while isDepthPositive reads the current estimates; the stop flag is polled where the reference polls.
 *
 * Deviations, deliberate:
 *  - fixed summation order (g2o's follows pointer-ordered containers): per point, sums run over its
 *    edges in the caller's order from +0.0; across points, point p belongs to lane p % 64, a lane adds in
 *    ascending p from +0.0, the lanes are combined by s[l] += s[l + stride], stride = 32 .. 1 (Hpp(i,i),
 *    bp_i, each Schur block, bschur, the total chi2, computeScale's point part; its pose part is added in
 *    pose order and the total is poses + points). S = (Hpp + lambda on the diagonal) - C is formed once.
 *  - the reduced system is solved by a dense, unpivoted LDL^T in natural order on the upper triangle
 *    (the reference: Eigen's sparse SimplicialLDLT with AMD ordering). A trial fails when a d_j is 0.
 *  - ORBFE_LBA_FLAG_NONFINITE: a non-finite entry of S, bschur, a Dinv or a d_j fails the trial;
 *    computeLambdaInit skips a NaN diagonal entry.
 *  - sin / cos and pow(., 3) as in orbfe_poseopt.h (ORBFE_LBA_FLAG_LARGE_STEP); x is zero before a
 *    round's first successful solve and keeps the last successful solve's value after a failed one.
 *  - an edge's error is zero before the first computeActiveErrors (g2o leaves it uninitialised): this
 *    shows only when the stop flag ends round 1 before its first iteration.
 *  - no free keyframe, or no edge: ORBFE_OK with rounds_run = 0 and the inputs as bits.
 *
 * Bounds: 128 free keyframes, 512 keyframes, 16,384 points, 131,072 edges. A handle is not thread-safe.
 */
#ifndef ORBFE_LBA_H
#define ORBFE_LBA_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_lba orbfe_lba;

#define ORBFE_LBA_MAX_FREE_KF 128
#define ORBFE_LBA_MAX_KF 512
#define ORBFE_LBA_MAX_POINTS 16384
#define ORBFE_LBA_MAX_EDGES 131072

#define ORBFE_LBA_FLAG_LARGE_STEP 1u
#define ORBFE_LBA_FLAG_NONFINITE 2u

/* why a round's optimize() ended */
#define ORBFE_LBA_STOP_ALL 0        /* ran all its iterations */
#define ORBFE_LBA_STOP_TERMINATE 1  /* 10 trials in one iteration, or rho == 0 */
#define ORBFE_LBA_STOP_NBAD 2       /* three iterations in a row gained less than 1e-3 of their chi2 */
#define ORBFE_LBA_STOP_NO_EDGE 3    /* no level-0 edge: optimize() returned without a step */
#define ORBFE_LBA_STOP_FLAG 4       /* the stop flag read true */

/* device < 0: a host-only handle (argument checks work, a solve that gets past them returns
 * ORBFE_ERR_STATE). ORBFE_ERR_ARG past the hard caps above. */
int orbfe_lba_create(int device, int max_free_kf, int max_kf, int max_points, int max_edges, orbfe_lba** out);
int orbfe_lba_destroy(orbfe_lba* h);

typedef struct {
  int n_kf, n_points, n_edges;
  const float* tcw;               /* [n_kf*12] upper 3x4 of GetPose(), row-major */
  const float* k;                 /* [n_kf*4] fx fy cx cy */
  const float* bf;                /* [n_kf] mbf */
  const uint8_t* fixed;           /* [n_kf] a fixed camera, or a local keyframe with mnId == 0 */
  const float* xw;                /* [n_points*3] GetWorldPos() */
  const int* edge_begin;          /* [n_points+1] point p's edges are edge_begin[p] .. edge_begin[p+1]-1 */
  const int* edge_kf;             /* [n_edges] index of the observing keyframe */
  const float* kp_un;             /* [n_edges*2] mvKeysUn[].pt */
  const float* u_right;           /* [n_edges] mvuRight[]; < 0: monocular */
  const float* inv_sigma2;        /* [n_edges] mvInvLevelSigma2[octave] */
  const volatile int* stop_flag;  /* optional: pbStopFlag */
  int stop_at_poll;               /* -1: off; k: poll k (counted from 0) and every later one read true */
} orbfe_lba_problem_t;

typedef struct {
  int n_active;         /* level-0 edges of the round */
  int iterations;       /* solve() calls */
  int trials;           /* Levenberg trials over all iterations */
  int rejected_trials;
  int stop;             /* ORBFE_LBA_STOP_* */
  int n_flagged;        /* round 1: edges sent to level 1; the last round run: n_erase */
  double lambda;        /* _currentLambda at the end */
  double chi2;          /* the last currentChi */
} orbfe_lba_round_t;

typedef struct {
  float* tcw;             /* out [n_kf*12]: what SetPose receives; a fixed keyframe's input bits */
  float* xw;              /* out [n_points*3]: what SetWorldPos receives */
  int mask_words;         /* in: 64-bit words each mask holds (>= ceil(n_edges/64)) */
  uint64_t* erase_mask;   /* out: bit e%64 of word e/64 = edge e is in vToErase */
  uint64_t* level1_mask;  /* out: the edges round 2 left out */
  int n_erase;
  int rounds_run;         /* 0: stopped at the first poll (or nothing to optimise), 1, 2 */
  uint32_t flags;         /* ORBFE_LBA_FLAG_* */
  int polls;              /* stop-flag polls made */
  orbfe_lba_round_t rounds[2];
} orbfe_lba_result_t;

/* ORBFE_ERR_CAPACITY past the handle's bounds (or mask_words too small); ORBFE_ERR_ARG for a null
 * array, an edge_begin that is not a CSR over n_edges, a keyframe index out of range or a keyframe
 * listed twice under one point. The Levenberg control flow runs on the host: one small record is read
 * back per linearisation and per trial; every kernel is launched on the handle's one stream. */
int orbfe_lba_solve(orbfe_lba* h, const orbfe_lba_problem_t* problem, orbfe_lba_result_t* result);

#ifdef __cplusplus
}
#endif
#endif
