/*
 * orbfe_pnp.h -- PnPsolver on the GPU (liborbfe.so, gfx950): the EPnP RANSAC hypotheses of every
 * relocalisation candidate are generated, checked against all correspondences, refined and selected
 * in one device pass.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   PnPsolver::SetRansacParameters / find / iterate / Refine    src/PnPsolver.cc:127-316
 *   CheckInliers                                                :318-349
 *   EPnP: compute_pose and everything below it                  :385-1009
 * called by Tracking::Relocalization (Tracking.cc:1368-1560) between the per-candidate SearchByBoW
 * (orbfe_search_by_bow) and PoseOptimization.
 *
 * The caller does what the constructor does (:66-117): it filters the matches and passes mvP3Dw,
 * mvP2D (mvKeysUn[i].pt), each keypoint's mvLevelSigma2 entry and fx, fy, cx, cy. The library derives
 * mRansacMinInliers, the adjusted epsilon, mRansacMaxIts (:140-163; a quotient that does not fit an
 * int converts as x86 does, to INT_MIN, so the result is 1) and mvMaxError[i] = sigma2[i] * th2 in
 * float.
 *
 * Random draws: the caller draws. rand_idx holds the raw values DUtils::Random::RandomInt(0,
 * vAvailableIndices.size() - 1) returned, four per iteration, iteration k at rand_idx[4k..4k+3];
 * draw i of an iteration must lie in 0 .. n-1-i. The library runs the swap-remove selection
 * (:199-212) on them.
 *
 * Every drawn hypothesis is evaluated whether or not an earlier one is accepted. Hypothesis k is a
 * record when its count is >= mRansacMinInliers and above every earlier such count; Refine() is
 * deterministic in mvbBestInliers, so it has one result per record, and the iteration the reference
 * accepts is the first record whose refinement has more than mRansacMinInliers inliers. find() is
 * replayed on the device, iterate() on the host by orbfe_pnp_iterate.
 *
 * Deviations, deliberate:
 *  - the caller draws all samples up front, so after an early acceptance it has consumed more rand()
 *    values than the reference would have. For given draws the result is identical.
 *  - min_set must be 4 (ORBFE_ERR_ARG otherwise): the reference never uses another value.
 *  - ORBFE_PNP_FLAG_SVD_NULL: a singular value <= DBL_MIN scales its left singular vector by 0 as it
 *    stands; OpenCV refills that vector from its RNG.
 *  - ORBFE_PNP_FLAG_QR_SINGULAR: qr_solve's singular early return (:934-939) leaves x unset; x is 0
 *    before the first Gauss-Newton step and keeps the previous step's value later. Nothing is printed.
 *  - at most ORBFE_PNP_MAX_RECORDS records per solver are refined; a solve that meets more returns
 *    ORBFE_ERR_CAPACITY.
 *
 * Bounds: max_solvers <= 64, max_corr <= 4096 correspondences per solver, max_hyp <= 1024 hypotheses
 * per solver (Relocalization draws 300). A solver with n < mRansacMinInliers is not launched (bNoMore,
 * no result). A handle is not thread-safe: one call at a time.
 */
#ifndef ORBFE_PNP_H
#define ORBFE_PNP_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_pnp orbfe_pnp;

#define ORBFE_PNP_MAX_SOLVERS 64
#define ORBFE_PNP_MAX_CORR 4096
#define ORBFE_PNP_MAX_HYP 1024
#define ORBFE_PNP_MAX_RECORDS 16

#define ORBFE_PNP_FLAG_SVD_NULL 1u
#define ORBFE_PNP_FLAG_QR_SINGULAR 2u

/* device < 0: a host-only handle (argument checks and orbfe_pnp_iterate work, a solve returns
 * ORBFE_ERR_STATE). */
int orbfe_pnp_create(int device, int max_solvers, int max_corr, int max_hyp, orbfe_pnp** out);
int orbfe_pnp_destroy(orbfe_pnp* h);

typedef struct {
  int n;                    /* correspondences that survived the constructor's filter */
  const float* p3dw;        /* [n*3] mvP3Dw */
  const float* p2d;         /* [n*2] mvP2D */
  const float* sigma2;      /* [n] mvSigma2 */
  float k[4];               /* fx, fy, cx, cy */
  double probability;       /* SetRansacParameters(probability, minInliers, maxIterations, minSet, */
  int min_inliers;          /*                     epsilon, th2)                                    */
  int max_iterations;
  int min_set;              /* must be 4 */
  float epsilon;
  float th2;
  int n_hyp;                /* iterations drawn */
  const int32_t* rand_idx;  /* [4*n_hyp] */
} orbfe_pnp_solver_t;

typedef struct {
  int hyp_capacity;         /* in: hypotheses each per-hypothesis array holds (>= n_hyp) */
  int rec_capacity;         /* in: records each per-record array holds (>= min(n_hyp, ORBFE_PNP_MAX_RECORDS)) */
  int mask_words;           /* in: 64-bit words per mask (>= ceil(n/64)) */
  /* per evaluated hypothesis k; an array that is NULL is not filled */
  int32_t* n_inliers;       /* [k] mnInliersi */
  uint64_t* inlier_mask;    /* [k*mask_words] bit i%64 of word i/64: mvbInliersi[i] */
  double* r;                /* [k*9] mRi, row-major */
  double* t;                /* [k*3] mti */
  float* tcw;               /* [k*12] upper 3x4 of the Tcw :228-234 builds, row-major */
  int32_t* n_chosen;        /* [k] the N of :533-535 */
  uint32_t* flags;          /* [k] ORBFE_PNP_FLAG_* */
  /* per record j (in hypothesis order); an array that is NULL is not filled */
  int32_t* records;         /* [j] the record's hypothesis index */
  int32_t* refined_inliers; /* [j] mnRefinedInliers */
  uint64_t* refined_mask;   /* [j*mask_words] mvbRefinedInliers */
  double* refined_r;        /* [j*9] */
  double* refined_t;        /* [j*3] */
  float* refined_tcw;       /* [j*12] upper 3x4 of mRefinedTcw */
  int32_t* refined_n_chosen;
  uint32_t* refined_flags;
  /* out */
  int n_records;
  int n_evaluated;          /* n_hyp; 0 when n < mRansacMinInliers */
  int ransac_max_its;       /* mRansacMaxIts */
  int ransac_min_inliers;   /* mRansacMinInliers */
  float ransac_epsilon;     /* mRansacEpsilon */
  /* find() from a fresh state, over the first min(n_evaluated, mRansacMaxIts) hypotheses */
  int accepted;             /* the record whose refined pose find() returns, or -1 */
  int accepted_inliers;     /* its mnRefinedInliers (0 without one) */
  int best;                 /* hypothesis behind mBestTcw (-1: none yet) */
  int best_inliers;         /* mnBestInliers */
  int no_more;              /* bNoMore (1 also when n < mRansacMinInliers) */
} orbfe_pnp_result_t;

/* Solves solvers[0..n_solvers): one upload, six kernels on one stream, one result copy, one stream
 * synchronisation. ORBFE_ERR_CAPACITY when a solver's n or n_hyp exceeds the handle's bounds or a
 * result's capacities. */
int orbfe_pnp_solve_batch(orbfe_pnp* h, const orbfe_pnp_solver_t* solvers, int n_solvers,
                          orbfe_pnp_result_t* results);

typedef struct {
  int iterations;           /* mnIterations */
  int best_inliers;         /* mnBestInliers */
  int best;                 /* hypothesis behind mBestTcw, -1: none. Start from {0, 0, -1}. */
} orbfe_pnp_state_t;

typedef struct {
  int mask_words;           /* in: words inlier_mask holds (>= ceil(n/64)) */
  uint64_t* inlier_mask;    /* in, optional: mvbRefinedInliers (returned == 1) or mvbBestInliers
                             * (returned == 2) over the solver's n, zeroed otherwise. Scattering through
                             * mvKeyPointIndices is the caller's. */
  int returned;             /* 0: an empty cv::Mat; 1: mRefinedTcw of record `accepted`; 2: mBestTcw,
                             * unrefined (:252-266) */
  int accepted;             /* the accepted record's hypothesis index, or -1 */
  float tcw[12];            /* upper 3x4 of the returned pose */
  int no_more;              /* bNoMore */
  int n_inliers;            /* nInliers */
} orbfe_pnp_iterate_t;

/* iterate(nIterations) (:176-269) of solver `solver_index` of the last orbfe_pnp_solve_batch,
 * replayed on the host (no device work), with the loop condition as written:
 * mnIterations < mRansacMaxIts || nCurrentIterations < nIterations. The walk also stops when the
 * solver's evaluated hypotheses run out. */
int orbfe_pnp_iterate(orbfe_pnp* h, int solver_index, int n_iterations, orbfe_pnp_state_t* state,
                      orbfe_pnp_iterate_t* out);

#ifdef __cplusplus
}
#endif
#endif
