/*
 * orbfe_poseopt.h -- Optimizer::PoseOptimization on the GPU (liborbfe.so, gfx950): the motion-only
 * Levenberg-Marquardt of one frame, or of every surviving relocalisation candidate, in one launch.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   Optimizer::PoseOptimization                                 src/Optimizer.cc:242-452
 *   Converter::toSE3Quat / toCvMat                              src/Converter.cc:37-53
 * and what it runs of g2o: VertexSE3Expmap::oplusImpl, EdgeSE3ProjectXYZOnlyPose and
 * EdgeStereoSE3ProjectXYZOnlyPose (types_six_dof_expmap.{h,cpp}), SE3Quat (se3quat.h),
 * BaseUnaryEdge::constructQuadraticForm, RobustKernelHuber::robustify,
 * OptimizationAlgorithmLevenberg::solve, SparseOptimizer::initializeOptimization / optimize /
 * activeRobustChi2, BlockSolver::buildSystem / setLambda / restoreDiagonal / solve (non-Schur) and
 * LinearSolverDense::solve (Eigen's LDLT).
 * Called by Tracking::TrackReferenceKeyFrame, TrackWithMotionModel, TrackLocalMap (one problem) and
 * Tracking::Relocalization (one problem per candidate, up to three times).
 *
 * A problem is indexed by the frame's keypoints, so bit i of the outlier mask is mvbOutlier[i]. The
 * caller gathers, per keypoint i: valid[i] = (mvpMapPoints[i] != NULL), the map point's GetWorldPos(),
 * mvKeysUn[i].pt, mvuRight[i] (< 0: monocular edge) and mvInvLevelSigma2[mvKeysUn[i].octave]; and fx,
 * fy, cx, cy, mbf and the upper 3x4 of mTcw.
 *
 * Carried as written: every round restarts from mTcw; the Huber kernel is removed after round 2; an
 * active edge is classified by the error of the round's last evaluated trial, accepted or not, a
 * flagged one is recomputed at the final estimate; chi2 is narrowed to float and compared with >, so
 * a NaN chi2 is an inlier; 3..9 correspondences run one round, fewer than 3 return 0 with the pose
 * untouched; a round without an active edge takes no step.
 *
 * Deviations, deliberate:
 *  - the sum over edges has a fixed order (g2o's follows a std::set of pointers): edge i belongs to
 *    lane i % 64, a lane adds its active edges in ascending i from +0.0, the 64 lanes are combined by
 *    s[l] += s[l + stride], stride = 32 .. 1. Eigen's small fixed-size products are taken in plain
 *    left-to-right scalar order.
 *  - sin / cos of SE3Quat::exp are a Cody-Waite reduction and fixed polynomials in + - * / (within
 *    2 ulp of libm on [1e-5, pi]); pow(theta, 3) and pow(2 rho - 1, 3) are x * x * x. A rotation step
 *    above pi sets ORBFE_POSEOPT_FLAG_LARGE_STEP; the functions stay defined there.
 *  - ORBFE_POSEOPT_FLAG_NONFINITE: a non-finite entry of H + lambda I or b makes the trial fail as a
 *    non-positive factorisation does (tempChi = DBL_MAX, rejected); Eigen's pivot search is not
 *    followed over NaN.
 *  - the increment x is zero before a round's first successful solve; g2o leaves it as allocated.
 *
 * Bounds: max_problems <= 64, max_obs <= 4096 keypoints per problem. A handle is not thread-safe: one
 * call at a time.
 */
#ifndef ORBFE_POSEOPT_H
#define ORBFE_POSEOPT_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_poseopt orbfe_poseopt;

#define ORBFE_POSEOPT_MAX_PROBLEMS 64
#define ORBFE_POSEOPT_MAX_OBS 4096

#define ORBFE_POSEOPT_FLAG_LARGE_STEP 1u
#define ORBFE_POSEOPT_FLAG_NONFINITE 2u

/* why a round's optimize() ended */
#define ORBFE_POSEOPT_STOP_ALL 0        /* ran all 10 iterations */
#define ORBFE_POSEOPT_STOP_TERMINATE 1  /* 10 trials in one iteration, or rho == 0 */
#define ORBFE_POSEOPT_STOP_NBAD 2       /* three iterations in a row gained less than 1e-3 of their chi2 */
#define ORBFE_POSEOPT_STOP_NO_EDGE 3    /* no active edge: optimize() returned -1 without a step */

/* device < 0: a host-only handle (argument checks work, a solve returns ORBFE_ERR_STATE). */
int orbfe_poseopt_create(int device, int max_problems, int max_obs, orbfe_poseopt** out);
int orbfe_poseopt_destroy(orbfe_poseopt* h);

typedef struct {
  int n;                    /* the frame's keypoints (pFrame->N) */
  const uint8_t* valid;     /* [n] mvpMapPoints[i] != NULL */
  const float* xw;          /* [n*3] GetWorldPos() (read where valid) */
  const float* kp_un;       /* [n*2] mvKeysUn[i].pt */
  const float* u_right;     /* [n] mvuRight; < 0: monocular */
  const float* inv_sigma2;  /* [n] mvInvLevelSigma2[mvKeysUn[i].octave] */
  float k[4];               /* fx, fy, cx, cy */
  float bf;                 /* mbf */
  float tcw[12];            /* upper 3x4 of mTcw, row-major */
} orbfe_poseopt_problem_t;

typedef struct {
  int n_active;             /* level-0 edges the round optimised */
  int iterations;           /* solve() calls */
  int trials;               /* Levenberg trials over all iterations */
  int rejected_trials;
  int stop;                 /* ORBFE_POSEOPT_STOP_* */
  int n_bad;                /* nBad after the round's classification */
  double lambda;            /* _currentLambda at the end */
  double chi2;              /* the last currentChi */
} orbfe_poseopt_round_t;

typedef struct {
  int mask_words;           /* in: 64-bit words outlier_mask holds (>= ceil(n/64)) */
  uint64_t* outlier_mask;   /* in, optional: bit i%64 of word i/64 = mvbOutlier[i]; 0 for invalid entries */
  float tcw[12];            /* what SetPose receives; the input pose, as bits, when n_initial < 3 */
  double pose_q_t[7];       /* the recovered SE3Quat: x y z w, then t */
  int n_initial;            /* nInitialCorrespondences */
  int n_bad;
  int n_inliers;            /* the return value */
  int rounds_run;
  uint32_t flags;           /* ORBFE_POSEOPT_FLAG_* */
  orbfe_poseopt_round_t rounds[4];
} orbfe_poseopt_result_t;

/* Optimises problems[0..n_problems): one upload, one launch of k_poseopt (one wavefront per problem,
 * all four rounds inside), one result copy, one stream synchronisation. ORBFE_ERR_CAPACITY when
 * n_problems or a problem's n exceeds the handle's bounds, or mask_words is below ceil(n/64). */
int orbfe_poseopt_batch(orbfe_poseopt* h, const orbfe_poseopt_problem_t* problems, int n_problems,
                        orbfe_poseopt_result_t* results);

#ifdef __cplusplus
}
#endif
#endif
