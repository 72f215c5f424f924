/*
 * orbfe_optsim3.h -- Optimizer::OptimizeSim3 on the GPU (liborbfe.so, gfx950): the 7-DoF
 * Levenberg-Marquardt of every loop candidate's Sim3 in one launch.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   Optimizer::OptimizeSim3                                     src/Optimizer.cc:1050-1250
 *   Converter::toCvMat(g2o::Sim3)                               src/Converter.cc:55-61
 *   gScm / gSmw / mScw of LoopClosing::ComputeSim3              src/LoopClosing.cc:341-354
 * and what it runs of g2o: Sim3 (sim3.h), VertexSim3Expmap::oplusImpl, EdgeSim3ProjectXYZ and
 * EdgeInverseSim3ProjectXYZ (types_seven_dof_expmap.h), BaseBinaryEdge::linearizeOplus (numeric) and
 * constructQuadraticForm, RobustKernelHuber::robustify, OptimizationAlgorithmLevenberg::solve,
 * SparseOptimizer::optimize / activeRobustChi2, BlockSolver (non-Schur) and LinearSolverDense::solve.
 *
 * A problem is indexed by KF1's keypoints, so bit i of the removal mask is "vpMatches1[i] was set to
 * NULL". The caller gathers, per keypoint i of KF1: valid[i] = (vpMatches1[i] and KF1's map point i
 * exist, neither isBad(), i2 = GetIndexInKeyFrame(KF2) >= 0), P3D1c = R1w * P3D1w + t1w and P3D2c
 * (cv::Mat float arithmetic), mvKeysUn[i].pt of KF1 and mvKeysUn[i2].pt of KF2, and the two
 * mvInvLevelSigma2 entries; per problem K1, K2, the Sim3Solver's R, t, s, th2 and bFixScale.
 *
 * Carried as written: the Jacobians are numeric (oplus(+-1e-9 e_d) per dimension, column =
 * (1 / 2e-9) * (e+ - e-)); Sim3(update)'s four branches, quaternions never normalised; with fix_scale
 * update[6] is zeroed in place; round 2 continues from round 1's estimate with the Huber kernel on;
 * a correspondence is removed when e12->chi2() > th2 || e21->chi2() > th2 on the errors of the round's
 * last evaluated trial, accepted or not, so a NaN chi2 keeps it; fewer than 10 correspondences after
 * round 1 return 0 with the Sim3 untouched and round 1's removals applied; no correspondence takes
 * no step.
 *
 * Deviations, deliberate (as orbfe_poseopt.h):
 *  - the sum over edges has a fixed order: correspondence i belongs to lane i % 64, a lane adds e12
 *    then e21 in ascending i from +0.0, the 64 lanes are combined by s[l] += s[l + stride],
 *    stride = 32 .. 1. Eigen's small fixed-size products are taken in plain left-to-right scalar order.
 *  - exp, sin and cos of Sim3(update) are Cody-Waite reductions and fixed polynomials in + - * /
 *    (exp within 1 ulp of libm on [-1, 1]); pow(2 rho - 1, 3) is x * x * x. A rotation step above pi
 *    sets ORBFE_OPTSIM3_FLAG_LARGE_STEP.
 *  - ORBFE_OPTSIM3_FLAG_NONFINITE: a non-finite entry of H + lambda I or b makes the trial fail as a
 *    non-positive factorisation does (tempChi = DBL_MAX, rejected).
 *  - the increment x is zero before a round's first successful solve; g2o leaves it as allocated.
 *
 * Bounds: max_problems <= 64, max_obs <= 4096 keypoints per problem. A handle is not thread-safe: one
 * call at a time.
 */
#ifndef ORBFE_OPTSIM3_H
#define ORBFE_OPTSIM3_H
#include <stdint.h>

#include "orbfe.h"
#include "orbfe_poseopt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_optsim3 orbfe_optsim3;

#define ORBFE_OPTSIM3_MAX_PROBLEMS 64
#define ORBFE_OPTSIM3_MAX_OBS 4096

#define ORBFE_OPTSIM3_FLAG_LARGE_STEP ORBFE_POSEOPT_FLAG_LARGE_STEP
#define ORBFE_OPTSIM3_FLAG_NONFINITE ORBFE_POSEOPT_FLAG_NONFINITE

/* device < 0: a host-only handle (argument checks work, a solve returns ORBFE_ERR_STATE). */
int orbfe_optsim3_create(int device, int max_problems, int max_obs, orbfe_optsim3** out);
int orbfe_optsim3_destroy(orbfe_optsim3* h);

typedef struct {
  int n;                      /* KF1's keypoints (vpMatches1.size()) */
  const uint8_t* valid;       /* [n] the correspondence enters the optimisation (:1110-1145) */
  const float* p3d1c;         /* [n*3] R1w * P3D1w + t1w (read where valid) */
  const float* p3d2c;         /* [n*3] R2w * P3D2w + t2w of vpMatches1[i] */
  const float* kp_un1;        /* [n*2] KF1's mvKeysUn[i].pt */
  const float* kp_un2;        /* [n*2] KF2's mvKeysUn[i2].pt */
  const float* inv_sigma2_1;  /* [n] KF1's mvInvLevelSigma2[kpUn1.octave] */
  const float* inv_sigma2_2;  /* [n] KF2's mvInvLevelSigma2[kpUn2.octave] */
  float k1[4], k2[4];         /* fx, fy, cx, cy of each keyframe */
  float r12[9], t12[3], s12;  /* the start: what orbfe_sim3_result_t returns */
  float th2;
  int fix_scale;
  int has_kf2;                /* r2w / t2w are given: the result's scw is filled */
  float r2w[9], t2w[3];       /* KF2's GetRotation() / GetTranslation() */
} orbfe_optsim3_problem_t;

typedef struct {
  int mask_words;             /* in: 64-bit words removed_mask holds (>= ceil(n/64)) */
  uint64_t* removed_mask;     /* in, optional: bit i%64 of word i/64 = vpMatches1[i] set to NULL */
  int n_correspondences;      /* nCorrespondences */
  int n_bad;                  /* correspondences removed by both classifications */
  int n_inliers;              /* the return value: nIn, or 0 on the early return */
  int rounds_run;             /* 1: returned after round 1 (fewer than 10 left), 2 otherwise */
  uint32_t flags;             /* ORBFE_OPTSIM3_FLAG_* */
  double sim3_q_t_s[8];       /* g2oS12 afterwards: q xyzw, t, s; the start as constructed on the early return */
  float s12_rt[12];           /* Converter::toCvMat(g2oS12): float(s R | t), row-major 3x4 */
  float scw[12];              /* has_kf2: toCvMat(g2oS12 * Sim3(R2w, t2w, 1.0)); else 0 */
  orbfe_poseopt_round_t rounds[2];
} orbfe_optsim3_result_t;

/* Optimises problems[0..n_problems): one upload, one launch of k_optsim3 (one wavefront per problem,
 * both rounds inside), one result copy, one stream synchronisation. ORBFE_ERR_CAPACITY when
 * n_problems or a problem's n exceeds the handle's bounds, or removed_mask is given and mask_words is
 * below ceil(n/64). With removed_mask NULL no mask is written and mask_words is only checked for >= 0. */
int orbfe_optsim3_batch(orbfe_optsim3* h, const orbfe_optsim3_problem_t* problems, int n_problems,
                        orbfe_optsim3_result_t* results);

#ifdef __cplusplus
}
#endif
#endif
