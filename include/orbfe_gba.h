/*
 * orbfe_gba.h -- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt on the GPU (liborbfe.so, gfx950):
 * the Levenberg-Marquardt of a whole map, the points marginalised by a Schur complement formed over the
 * covisible keyframe pairs only, the reduced pose system held and factorised as a 6x6 block envelope.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   Optimizer::BundleAdjustment, from the optimizer's set-up on        src/Optimizer.cc:51-240
 *   Converter::toSE3Quat / toVector3d / toCvMat                        src/Converter.cc
 * and what it runs of g2o: the routines listed in orbfe_lba.h (the two BA edges, constructQuadraticForm,
 * RobustKernelHuber, BlockSolver_6_3 with the Schur branch of solve, OptimizationAlgorithmLevenberg,
 * SparseOptimizer's initializeOptimization, optimize, push, pop, discardTop, update, removeVertex).
 * Its two callers: LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:679: 10 iterations, not robust)
 * and Tracking::CreateInitialMapMonocular (Tracking.cc:707: 20 iterations, robust).
 *
 * The caller performs the gather of Optimizer.cc:70-186: the keyframes that
 * are not bad, ascending in mnId, with GetPose(), fx fy cx cy, mbf and fixed = (mnId == 0); the map points
 * that are not bad, ascending in mnId, with GetWorldPos(); per point its observations by a listed
 * keyframe, contiguous (edge_begin is a CSR over the points), each with the keyframe's index,
 * mvKeysUn[].pt, mvuRight[] (< 0: a monocular edge) and mvInvLevelSigma2[octave].
 *
 * Carried as written: one optimize(n_iterations) over all edges (no second round, no chi2 or depth
 * classification, no erase mask); the Huber deltas are float(sqrt(5.99)) (mono: 5.99, not
 * LocalBundleAdjustment's 5.991) and float(sqrt(7.815)); with robust == 0 no kernel is set; a point
 * without an edge is removed from the graph (vbNotIncludedMP) and its output is its input bits; every
 * keyframe is written out through toSE3Quat -> toCvMat, the fixed and the edgeless ones included; a
 * keyframe with no edge to an included point is not in the system and keeps its estimate; an edge to a
 * fixed keyframe adds to its point's Hll and b only; the stop flag is polled only inside optimize()
 * (before each iteration and between the trials of one), with no check before it.
 *
 * Deviations, deliberate:
 *  - the fixed summation order of orbfe_lba.h (per point in edge order; across points the 64-lane rule
 *    and its tree), for Hpp, bp, every Schur block, bschur, chi2 and computeScale. S is formed once per
 *    trial with lambda on the diagonal.
 *  - the reduced system is solved by an unpivoted LDL^T in natural (slot) order over the block envelope
 *    (the reference: Eigen's sparse SimplicialLDLT with AMD ordering): v = A_ij; v -= (L_ik d_k) L_jk for
 *    k ascending; L_ij = v / d_j. Row s of the envelope starts at the smallest slot that shares a point
 *    with s; blocks inside it without a shared point start as +0.0 and fill in. A trial fails when a d_j
 *    is 0.
 *  - ORBFE_GBA_FLAG_NONFINITE: a non-finite entry of S, bschur, a Dinv or a d_j fails the trial;
 *    computeLambdaInit skips a NaN diagonal entry.
 *  - sin / cos and pow(., 3) as in orbfe_poseopt.h (ORBFE_GBA_FLAG_LARGE_STEP); x is zero before the
 *    first successful solve and keeps the last successful solve's value after a failed one.
 *  - no free keyframe, or no edge: ORBFE_OK with iterations = 0 and the inputs as bits.
 *
 * Out of scope, with the caller: the nLoopKF bookkeeping (SetPose against mTcwGBA / mnBAGlobalForKF);
 * LoopClosing::RunGlobalBundleAdjustment's spanning-tree propagation and map-point correction
 * (LoopClosing.cc:705-766); MapPoint::UpdateNormalAndDepth.
 *
 * Bounds: 4,096 keyframes, 524,288 points, 4,194,304 edges, 2,097,152 envelope blocks. The device
 * workspace of a handle at all four caps is about 3.0 GB: 534 bytes per edge (2.2 GB; the per-edge
 * products alone are 58 doubles), 288 bytes per envelope block and 16 per structural pair (0.65 GB),
 * 277 bytes per point (0.15 GB). A handle is not thread-safe.
 */
#ifndef ORBFE_GBA_H
#define ORBFE_GBA_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_gba orbfe_gba;

#define ORBFE_GBA_MAX_KF 4096
#define ORBFE_GBA_MAX_POINTS 524288
#define ORBFE_GBA_MAX_EDGES 4194304
#define ORBFE_GBA_MAX_ENV_BLOCKS 2097152
#define ORBFE_GBA_MAX_ITERATIONS 64

#define ORBFE_GBA_FLAG_LARGE_STEP 1u
#define ORBFE_GBA_FLAG_NONFINITE 2u

/* why optimize() ended */
#define ORBFE_GBA_STOP_ALL 0        /* ran all its iterations */
#define ORBFE_GBA_STOP_TERMINATE 1  /* 10 trials in one iteration, or rho == 0 */
#define ORBFE_GBA_STOP_NBAD 2       /* three iterations in a row gained less than 1e-3 of their chi2 */
#define ORBFE_GBA_STOP_NO_EDGE 3    /* not reached: without an edge the solve returns before optimize() */
#define ORBFE_GBA_STOP_FLAG 4       /* the stop flag read true */

/* device < 0: a host-only handle (argument checks and the plan work, a solve that gets past them returns
 * ORBFE_ERR_STATE). ORBFE_ERR_ARG below 1 or past the hard caps above. */
int orbfe_gba_create(int device, int max_kf, int max_points, int max_edges, int max_env_blocks, orbfe_gba** out);
int orbfe_gba_destroy(orbfe_gba* h);

typedef struct {
  int n_kf, n_points, n_edges;
  const float* tcw;               /* [n_kf*12] upper 3x4 of GetPose(), row-major */
  const float* k;                 /* [n_kf*4] fx fy cx cy */
  const float* bf;                /* [n_kf] mbf */
  const uint8_t* fixed;           /* [n_kf] mnId == 0; any set, none included, is accepted */
  const float* xw;                /* [n_points*3] GetWorldPos() */
  const int* edge_begin;          /* [n_points+1] point p's edges are edge_begin[p] .. edge_begin[p+1]-1 */
  const int* edge_kf;             /* [n_edges] index of the observing keyframe */
  const float* kp_un;             /* [n_edges*2] mvKeysUn[].pt */
  const float* u_right;           /* [n_edges] mvuRight[]; < 0: monocular */
  const float* inv_sigma2;        /* [n_edges] mvInvLevelSigma2[octave] */
  int n_iterations;               /* nIterations, 1 .. 64 */
  int robust;                     /* bRobust */
  const volatile int* stop_flag;  /* optional: pbStopFlag */
  int stop_at_poll;               /* -1: off; k: poll k (counted from 0) and every later one read true */
} orbfe_gba_problem_t;

typedef struct {
  int n_active;         /* level-0 edges: all of them */
  int iterations;       /* solve() calls */
  int trials;           /* Levenberg trials over all iterations */
  int rejected_trials;
  int stop;             /* ORBFE_GBA_STOP_* */
  double lambda;        /* _currentLambda at the end */
  double chi2;          /* the last currentChi */
  int env_blocks;       /* 6x6 blocks of the envelope */
  int schur_blocks;     /* structural keyframe pairs s1 <= s2 (those that share a point) */
  uint32_t flags;       /* ORBFE_GBA_FLAG_* */
  int polls;            /* stop-flag polls made */
} orbfe_gba_trace_t;

typedef struct {
  float* tcw;  /* out [n_kf*12]: what SetPose / mTcwGBA receives, for every keyframe */
  float* xw;   /* out [n_points*3]: what SetWorldPos / mPosGBA receives; a point without an edge: its input */
  orbfe_gba_trace_t trace;
} orbfe_gba_result_t;

/* ORBFE_ERR_CAPACITY past the handle's bounds (the envelope's blocks among them); ORBFE_ERR_ARG for a
 * null array, n_iterations outside 1 .. 64, an edge_begin that is not a CSR over n_edges, a keyframe
 * index out of range or a keyframe listed twice under one point. The Levenberg control flow runs on the
 * host: one small record is read back per linearisation and per trial; every kernel is launched on the
 * handle's one stream, and no kernel waits on another. */
int orbfe_gba_solve(orbfe_gba* h, const orbfe_gba_problem_t* problem, orbfe_gba_result_t* result);

/* Host only: the argument checks of orbfe_gba_solve (against the hard caps) and the plan. *env_blocks and
 * *schur_blocks are what a handle needs as max_env_blocks and what the trace will report. */
int orbfe_gba_envelope(const orbfe_gba_problem_t* problem, int* env_blocks, int* schur_blocks);

#ifdef __cplusplus
}
#endif
#endif
