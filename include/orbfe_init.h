/*
 * orbfe_init.h -- Initializer on the GPU (liborbfe.so, gfx950): the 2 x n_hyp eight-point hypotheses
 * of the monocular bootstrap are generated, scored against every match and selected, and the 8 or 4
 * motion hypotheses of the chosen model are triangulated and judged, in one device pass per batch.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021), src/Initializer.cc:
 *   Initialize                                   :44-121
 *   FindHomography / FindFundamental             :123-221
 *   ComputeH21 / ComputeF21                      :223-300
 *   CheckHomography / CheckFundamental           :302-468
 *   ReconstructF / ReconstructH / DecomposeE     :470-798, :986-1006
 *   Triangulate / Normalize / CheckRT            :800-984
 * called by Tracking::MonocularInitialization between ORBmatcher::SearchForInitialization and
 * Tracking::CreateInitialMapMonocular.
 *
 * One problem is one Initializer object plus one Initialize call: keys1 / keys2 are mvKeysUn[i].pt of
 * the reference and the current frame, matches12 is vMatches12 (-1 or an index into keys2), k is fx,
 * fy, cx, cy of mK, sigma and n_hyp are the constructor's sigma and iterations.
 *
 * Random draws: the caller draws. rand_idx holds the raw values DUtils::Random::RandomInt(0,
 * vAvailableIndices.size() - 1) returned, eight per iteration, iteration k at rand_idx[8k..8k+7]; draw
 * j of an iteration must lie in 0 .. N-1-j, N the number of matches. The library runs the swap-remove
 * selection (:82-97) on them.
 *
 * Deviations, deliberate:
 *  - all n_hyp hypotheses of both models are always evaluated (so does the reference).
 *  - ORBFE_INIT_FLAG_TOO_FEW: a problem with N < 8 is not launched; the reference would index past
 *    the end of vAvailableIndices. The result is false.
 *  - ORBFE_INIT_FLAG_NO_MODEL: no hypothesis of the chosen model scored above 0, so its matrix is an
 *    empty cv::Mat in the reference and the next product throws. The result is false.
 *  - RH of SH + SF == 0 is NaN; RH > 0.40 is then false and the F branch is taken, as written.
 *  - the parallax is acos(c) * 180 / CV_PI in the reference. The device returns the selected cosine c
 *    = vCosParallax[min(50, size - 1)]; the library's host side takes acosf of it, forms the degrees
 *    and makes the > minParallax (F) / >= minParallax (H) decision. No transcendental runs on the
 *    device.
 *  - the sorted vCosParallax is read at one index only, so it is selected, not sorted, under the IEEE
 *    total order of the bit patterns (-0 before +0, NaNs at the ends). std::sort on a NaN is
 *    unspecified in the reference.
 *  - when the result is false the reference leaves R21, t21, vP3D and vbTriangulated as the caller
 *    passed them; here they are zero-filled.
 *  - vn, the plane normals of ReconstructH, is never read by the reference and is not formed.
 *
 * Bounds: max_problems <= 16, max_keys <= 8192 keypoints per frame, max_matches <= 8192, max_hyp <=
 * 1024 hypotheses per model (the reference draws 200). A handle is not thread-safe: one call at a
 * time.
 */
#ifndef ORBFE_INIT_H
#define ORBFE_INIT_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_init orbfe_init;

#define ORBFE_INIT_MAX_PROBLEMS 16
#define ORBFE_INIT_MAX_KEYS 8192
#define ORBFE_INIT_MAX_MATCHES 8192
#define ORBFE_INIT_MAX_HYP 1024

#define ORBFE_INIT_FLAG_TOO_FEW 1u
#define ORBFE_INIT_FLAG_NO_MODEL 2u

#define ORBFE_INIT_MODEL_NONE (-1)
#define ORBFE_INIT_MODEL_H 0
#define ORBFE_INIT_MODEL_F 1

/* device < 0: a host-only handle (argument checks work, a solve returns ORBFE_ERR_STATE). */
int orbfe_init_create(int device, int max_problems, int max_keys, int max_matches, int max_hyp, orbfe_init** out);
int orbfe_init_destroy(orbfe_init* h);

typedef struct {
  int n1, n2;                /* keypoints of the reference / current frame (each >= 1) */
  const float* keys1;        /* [n1*2] mvKeysUn[i].pt of the reference frame */
  const float* keys2;        /* [n2*2] of the current frame */
  const int32_t* matches12;  /* [n1] -1 or an index into keys2 */
  float k[4];                /* fx, fy, cx, cy */
  float sigma;               /* Initializer(ReferenceFrame, sigma, iterations) */
  float min_parallax;        /* ReconstructH / ReconstructF's minParallax: Initialize passes 1.0 */
  int n_hyp;                 /* iterations drawn */
  const int32_t* rand_idx;   /* [8*n_hyp] */
} orbfe_init_problem_t;

typedef struct {
  int hyp_capacity;          /* in: hypotheses score_h / score_f hold (>= n_hyp) */
  int mask_words;            /* in: 64-bit words per mask (>= ceil(N/64)) */
  /* the reference's outputs; every array is required */
  float* p3d;                /* [n1*3] vP3D */
  uint8_t* triangulated;     /* [n1] vbTriangulated */
  /* diagnostics; an array that is NULL is not filled */
  float* score_h;            /* [n_hyp] CheckHomography's score of iteration k */
  float* score_f;            /* [n_hyp] CheckFundamental's */
  uint64_t* mask_h;          /* [mask_words] bit i%64 of word i/64: vbMatchesInliersH[i] over the N matches */
  uint64_t* mask_f;          /* [mask_words] vbMatchesInliersF */
  /* out */
  int ok;                    /* Initialize's return value */
  float r21[9], t21[3];      /* R21 row-major, t21 */
  int n_matches;             /* N = mvMatches12.size() */
  uint32_t flags;            /* ORBFE_INIT_FLAG_* */
  float sh, sf, rh;          /* SH, SF, RH */
  int model;                 /* ORBFE_INIT_MODEL_*: the branch RH took (NONE when not launched) */
  int best_h, best_f;        /* the iteration behind H / F, -1: none scored */
  float h21[9], f21[9];      /* H, F (zeros without one) */
  int n_motions;             /* 8 (H), 4 (F), 0 when ReconstructH returned at :654 or nothing ran */
  int n_good[8];             /* CheckRT's nGood per motion hypothesis */
  float cos_parallax[8];     /* vCosParallax[min(50, size-1)] after the sort; 0 where nGood == 0 */
  int candidate;             /* the motion hypothesis that passed every gate but the parallax, or -1 */
  int motion;                /* the winning motion hypothesis (candidate when ok), or -1 */
  float parallax;            /* the candidate's parallax in degrees (0 without one) */
} orbfe_init_result_t;

/* Solves problems[0..n): one upload, six kernels on one stream, one result copy, one stream
 * synchronisation. ORBFE_ERR_CAPACITY when a problem exceeds the handle's bounds or a result's
 * capacities; ORBFE_ERR_ARG for a null array, a draw out of range or a matches12 entry >= n2. */
int orbfe_init_solve_batch(orbfe_init* h, const orbfe_init_problem_t* problems, int n, orbfe_init_result_t* results);

#ifdef __cplusplus
}
#endif
#endif
