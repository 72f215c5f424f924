/*
 * orbfe_triangulate.h -- the geometry of LocalMapping::CreateNewMapPoints on MI355X (liborbfe.so):
 * SearchForTriangulation's matches in, map points out.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   the per-match loop of LocalMapping::CreateNewMapPoints      src/LocalMapping.cc:290-456
 *   KeyFrame::UnprojectStereo                                    src/KeyFrame.cc:632-648
 *   and, in orbfe_create_new_mappoints_device, the neighbour loop around them (:241-457) with the
 *   AddMapPoint that makes the next neighbour's search skip a keypoint (:445-446).
 * The caller keeps the baseline test (:248-265) and CheckNewKeyFrames() (:243): it leaves a skipped
 * neighbour out. It also keeps the map mutation (new MapPoint, AddObservation,
 * ComputeDistinctiveDescriptors, UpdateNormalAndDepth, mpMap->AddMapPoint): the calls return what
 * the reference would have created.
 *
 * A KeyFrame is an orbfe_frame_view (orbfe.h) plus an orbfe_tri_keyframe. Of the view the
 * triangulation reads n, keys_un, u_right, nlevels, scale_factors, level_sigma2, fx, fy, cx, cy, bf
 * and b; descriptors and mp_state are read by the search only. invfx / invfy are 1.0f / fx and
 * 1.0f / fy (Frame.cc / KeyFrame.cc), Rwc is the exact transpose of tcw's rotation, Twc's last
 * column is ow, ratioFactor is 1.5f * scale_factors[1] of KF1 (1.5f with a single level), and KF2's
 * stereo reprojection uses KF1's bf, as the reference does (:411).
 *
 * Outputs are dense over KF1's keypoints: entry idx1 belongs to the reference's pair
 * (idx1, match12[idx1]), which it walks in ascending idx1.
 *   status[n1]   int8, one of ORBFE_TRI_* below: the statement of :290-456 that ended the match
 *   x3d[n1 * 3]  the world point where status > 0; every other entry is left as it was
 *   nnew[1]      the number of entries with status > 0
 * Comparisons keep C semantics for NaN, exactly as the source writes them.
 *
 * Deviations from the reference, both on inputs it cannot survive:
 *   - UnprojectStereo returns an empty Mat for depth <= 0 (KeyFrame.cc:646-647) and the caller's
 *     x3D.t() / dot() would then throw; here the match ends with ORBFE_TRI_REJ_UNPROJECT.
 *   - match12[idx1] >= KF2's n, or a keypoint octave outside 0..nlevels-1, would read out of range;
 *     here the match ends with ORBFE_TRI_REJ_BAD_MATCH / ORBFE_TRI_REJ_BAD_OCTAVE before any of the
 *     reference's own tests. A negative match12 entry is "no match".
 */
#ifndef ORBFE_TRIANGULATE_H
#define ORBFE_TRIANGULATE_H
#include <stdint.h>

#include "orbfe.h"
#include "orbfe_match_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_TRI_NO_MATCH 0
#define ORBFE_TRI_TRIANGULATED 1   /* linear triangulation (:326-343) */
#define ORBFE_TRI_STEREO1 2        /* mpCurrentKeyFrame->UnprojectStereo(idx1) (:347) */
#define ORBFE_TRI_STEREO2 3        /* pKF2->UnprojectStereo(idx2) (:351) */
#define ORBFE_TRI_REJ_PARALLAX -1  /* no stereo and very low parallax (:354) */
#define ORBFE_TRI_REJ_W_ZERO -2    /* x3D.at<float>(3) == 0 (:338) */
#define ORBFE_TRI_REJ_Z1 -3        /* z1 <= 0 (:360) */
#define ORBFE_TRI_REJ_Z2 -4        /* z2 <= 0 (:364) */
#define ORBFE_TRI_REJ_REPROJ1 -5   /* reprojection error in KF1 (:379, :390) */
#define ORBFE_TRI_REJ_REPROJ2 -6   /* reprojection error in KF2 (:405, :416) */
#define ORBFE_TRI_REJ_DIST_ZERO -7 /* dist1 == 0 || dist2 == 0 (:427) */
#define ORBFE_TRI_REJ_SCALE -8     /* scale consistency (:436) */
#define ORBFE_TRI_REJ_UNPROJECT -9 /* UnprojectStereo's empty Mat: depth <= 0 (deviation, above) */
#define ORBFE_TRI_REJ_BAD_MATCH -10  /* match12[idx1] >= KF2's n (deviation, above) */
#define ORBFE_TRI_REJ_BAD_OCTAVE -11 /* a keypoint octave outside the level tables (deviation) */

#define ORBFE_TRI_MAX_KEYS 8192        /* keypoints of KF1 (the matcher's per-frame limit) */
#define ORBFE_TRI_MAX_KF2_KEYS 16384   /* keypoints of KF2 (SearchForTriangulation's limit) */
#define ORBFE_TRI_MAX_PAIRS 4096       /* pairs of one orbfe_triangulate_batch_device call */
#define ORBFE_TRI_MAX_NEIGHBOURS 64    /* neighbours of one orbfe_create_new_mappoints_device call */
#define ORBFE_TRI_MAX_LEVELS 32

/* What the triangulation reads of a KeyFrame beyond its orbfe_frame_view. */
typedef struct orbfe_tri_keyframe {
  float tcw[12];         /* GetPose() rows 0..2 (3x4, row-major) */
  float ow[3];           /* GetCameraCenter() */
  const float* depth;    /* mvDepth, n floats */
  const float* keys_xy;  /* optional mvKeys[i].pt, n x 2 floats: UnprojectStereo reads the distorted
                            keys (KeyFrame.cc:637-638). NULL = use keys_un. */
} orbfe_tri_keyframe;

/* One KeyFrame pair of orbfe_triangulate_batch_device. Every pointer, those inside kf1, kf2, t1 and
 * t2 included, is a DEVICE pointer. */
typedef struct orbfe_tri_pair {
  orbfe_frame_view kf1, kf2;
  orbfe_tri_keyframe t1, t2;
  const int32_t* match12;    /* kf1.n entries: idx2 or negative */
  const int32_t* kf1_n_dev;  /* optional device-side KF1 keypoint count (NULL = kf1.n); a value
                                above kf1.n is clamped to kf1.n, which sizes the launch */
  int8_t* status;            /* out: kf1.n */
  float* x3d;                /* out: kf1.n x 3 */
  int32_t* nnew;             /* out: 1 */
  uint8_t* mark1;            /* optional: KF1's mp_state, kf1.n bytes */
  uint8_t* mark2;            /* optional: KF2's mp_state, kf2.n bytes */
} orbfe_tri_pair;

/* The triangulation loop (:290-456) of one KeyFrame pair over host buffers; blocks until the
 * results are back (conventions of orbfe_keyframe.h). match12[kf1->n] as
 * orbfe_search_for_triangulation returns it. */
int orbfe_triangulate_matches(orbfe_matcher* m, const orbfe_frame_view* kf1,
                              const orbfe_tri_keyframe* t1, const orbfe_frame_view* kf2,
                              const orbfe_tri_keyframe* t2, const int32_t* match12, int8_t* status,
                              float* x3d, int* nnew);

/* n_pairs independent pairs, asynchronous on `stream` (NULL = the matcher's stream). The struct
 * array is host memory and is copied on every call, like orbfe_sft_pair; it reads the match12 that
 * orbfe_search_for_triangulation_batch_device wrote earlier on the same stream. With mark1 / mark2
 * set, every accepted match stores ORBFE_MP_OBSERVED at mark1[idx1] and mark2[idx2]: the
 * AddMapPoint (:445-446) that a later search of either KeyFrame must see. */
int orbfe_triangulate_batch_device(orbfe_matcher* m, int n_pairs, const orbfe_tri_pair* pairs,
                                   void* stream);

/* One neighbour of orbfe_create_new_mappoints_device (all pointers device memory). kf.mp_state is
 * written (cast from const): it must be the neighbour's own, writable array. */
typedef struct orbfe_tri_neighbour {
  orbfe_frame_view kf;
  orbfe_tri_keyframe t;
  orbfe_feature_vector fv;
  float f12[9];   /* ComputeF12(mpCurrentKeyFrame, pKF2), row-major */
  float ex, ey;   /* epipole of KF1 in the neighbour (ORBmatcher.cc:678-684) */
} orbfe_tri_neighbour;

/* CreateNewMapPoints' neighbour loop (:241-457) for one KF1 against n_nb neighbours in the caller's
 * order, asynchronous on `stream`: per neighbour SearchForTriangulation(KF1, nb, F12, ., false) and
 * then the triangulation with marking on, everything on one stream with no synchronisation and no
 * host copy in between. kf1->mp_state and every neighbour's kf.mp_state are read by the searches
 * and written by the marking, so neighbour j + 1 sees what neighbour j added. A neighbour whose
 * mp_state or keys_un pointer equals KF1's or an earlier neighbour's is rejected (ORBFE_ERR_ARG).
 * Device outputs, neighbour j at row j: match12[n_nb x kf1->n], status[n_nb x kf1->n],
 * x3d[n_nb x kf1->n x 3], nmatches[n_nb] (the search's return value), nnew[n_nb]. */
int orbfe_create_new_mappoints_device(orbfe_matcher* m, const orbfe_frame_view* kf1,
                                      const orbfe_tri_keyframe* t1, const orbfe_feature_vector* fv1,
                                      int n_nb, const orbfe_tri_neighbour* nbs, int32_t* match12,
                                      int8_t* status, float* x3d, int32_t* nmatches, int32_t* nnew,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
