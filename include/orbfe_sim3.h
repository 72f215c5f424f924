/*
 * orbfe_sim3.h -- Sim3Solver on the GPU (liborbfe.so, gfx950): the RANSAC hypotheses of every
 * loop-closure candidate are generated, checked against all correspondences and selected in one
 * device pass.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   Sim3Solver::SetRansacParameters / iterate / find          src/Sim3Solver.cc:113-212
 *   ComputeCentroid / ComputeSim3 (Horn 1987)                 :214-336
 *   CheckInliers / Project / FromCameraToImage                :338-420
 * called by LoopClosing::ComputeSim3 (LoopClosing.cc:290-343) between the per-candidate
 * SearchByBoW (orbfe_search_by_bow_kf_kf) and SearchBySim3 (orbfe_search_by_sim3), whose
 * s12 / r12 / t12 arguments are this solver's s12 / r12 / tr12 as they stand.
 *
 * The caller does what the constructor does (:61-101): it filters the correspondences and passes
 * mvX3Dc1 / mvX3Dc2 and each keypoint's mvLevelSigma2 entry. The library derives the error
 * thresholds ((size_t)(9.210 * sigma2), truncated, compared as float) and mRansacMaxIts
 * (:124-134; a quotient that does not fit an int converts as x86 does, to INT_MIN, so the result
 * is 1).
 *
 * Random draws: the caller draws. rand_idx holds the raw values DUtils::Random::RandomInt(0,
 * vAvailableIndices.size() - 1) returned, three per iteration, iteration k at rand_idx[3k..3k+2];
 * draw i of an iteration must lie in 0 .. n-1-i. The library runs the swap-remove selection
 * (:162-176) on them.
 * Deviation, deliberate: the caller draws all of a call's samples up front, so after an early
 * acceptance it has consumed more rand() values than the reference would have. For given draws
 * the result is identical.
 *
 * Every hypothesis is evaluated whether or not an earlier one is accepted; the reference's
 * order-dependent acceptance (best replaced when count >= best, return at the first count >
 * minInliers, bNoMore once mnIterations >= mRansacMaxIts) is replayed from the per-hypothesis
 * inlier counts, on the device for find() and on the host by orbfe_sim3_iterate.
 *
 * Bounds: max_solvers <= 64, max_corr <= 4096 correspondences per solver, max_hyp <= 1024
 * hypotheses per solver (the reference uses 300). A solver with n < min_inliers is not launched
 * (bNoMore, no result); any other solver needs n >= 3.
 * A handle is not thread-safe: one call at a time.
 */
#ifndef ORBFE_SIM3_H
#define ORBFE_SIM3_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_sim3 orbfe_sim3;

#define ORBFE_SIM3_MAX_SOLVERS 64
#define ORBFE_SIM3_MAX_CORR 4096
#define ORBFE_SIM3_MAX_HYP 1024

/* device < 0: a host-only handle (argument checks and orbfe_sim3_iterate's bookkeeping work, a
 * solve returns ORBFE_ERR_STATE). */
int orbfe_sim3_create(int device, int max_solvers, int max_corr, int max_hyp, orbfe_sim3** out);
int orbfe_sim3_destroy(orbfe_sim3* h);

typedef struct {
  int n;                    /* correspondences that survived the constructor's filter */
  const float* x3dc1;       /* [n*3] mvX3Dc1 */
  const float* x3dc2;       /* [n*3] mvX3Dc2 */
  const float* sigma2_1;    /* [n] pKF1->mvLevelSigma2[kp1.octave] */
  const float* sigma2_2;    /* [n] pKF2->mvLevelSigma2[kp2.octave] */
  float k1[4], k2[4];       /* fx, fy, cx, cy of mK1 / mK2 */
  int fix_scale;            /* mbFixScale */
  int min_inliers;          /* SetRansacParameters(probability, minInliers, maxIterations) */
  int max_iterations;
  double probability;
  int n_hyp;                /* iterations drawn */
  const int32_t* rand_idx;  /* [3*n_hyp]; may be NULL when hyp_t12 / hyp_t21 are given */
  /* optional, both or neither: caller-computed hypotheses, the upper 3x4 of mT12i / mT21i
   * row-major. Hypothesis generation is skipped; r12 and s12 of the result are then 0 and tr12 is
   * hyp_t12's last column. */
  const float* hyp_t12;     /* [n_hyp*12] */
  const float* hyp_t21;     /* [n_hyp*12] */
} orbfe_sim3_solver_t;

typedef struct {
  int hyp_capacity;         /* in: hypotheses each array below holds (>= min(n_hyp, max_iterations) is enough) */
  int mask_words;           /* in: 64-bit words per hypothesis in inlier_mask (>= ceil(n/64)) */
  /* per evaluated hypothesis k; an array that is NULL is not filled */
  int32_t* n_inliers;       /* [k] mnInliersi */
  float* t12;               /* [k*12] upper 3x4 of mT12i, row-major */
  float* t21;               /* [k*12] upper 3x4 of mT21i */
  float* r12;               /* [k*9] mR12i, row-major */
  float* tr12;              /* [k*3] mt12i */
  float* s12;               /* [k] ms12i */
  uint64_t* inlier_mask;    /* [k*mask_words] bit i%64 of word i/64: mvbInliersi[i] */
  /* out */
  int n_evaluated;          /* min(n_hyp, mRansacMaxIts); 0 when n < min_inliers */
  int ransac_max_its;       /* mRansacMaxIts */
  /* find() over the evaluated hypotheses */
  int accepted;             /* hypothesis find() returns, or -1 */
  int accepted_inliers;     /* nInliers (0 without an accepted hypothesis) */
  int best;                 /* hypothesis behind mBestT12 (-1: none yet) */
  int best_inliers;         /* mnBestInliers */
  int no_more;              /* bNoMore (1 also when n < min_inliers) */
} orbfe_sim3_result_t;

/* Solves solvers[0..n_solvers): one upload, three kernels, one result copy, one stream
 * synchronisation. ORBFE_ERR_CAPACITY when a solver's n or evaluated hypothesis count exceeds the
 * handle's bounds or a result's capacities. */
int orbfe_sim3_solve_batch(orbfe_sim3* h, const orbfe_sim3_solver_t* solvers, int n_solvers,
                           orbfe_sim3_result_t* results);

typedef struct {
  int iterations;           /* mnIterations */
  int best_inliers;         /* mnBestInliers */
  int best;                 /* hypothesis behind mBestT12, -1: none. Start from {0, 0, -1}. */
} orbfe_sim3_state_t;

typedef struct {
  int mask_words;           /* in: words inlier_mask holds (>= ceil(n/64)) */
  uint64_t* inlier_mask;    /* in, optional: the accepted hypothesis' mvbInliersi over the solver's n
                             * (zeroed when nothing is accepted). Scattering through mvnIndices1 is
                             * the caller's. */
  int accepted;             /* hypothesis whose mT12i iterate returns, or -1 (an empty cv::Mat) */
  float t12[12];            /* its upper 3x4, when accepted */
  int no_more;              /* bNoMore */
  int n_inliers;            /* nInliers */
} orbfe_sim3_iterate_t;

/* iterate(nIterations) (:139-206) of solver `solver_index` of the last orbfe_sim3_solve_batch,
 * replayed on the host from its inlier counts (no device work). The walk also stops when the
 * solver's evaluated hypotheses run out. */
int orbfe_sim3_iterate(orbfe_sim3* h, int solver_index, int n_iterations, orbfe_sim3_state_t* state,
                       orbfe_sim3_iterate_t* out);

#ifdef __cplusplus
}
#endif
#endif
