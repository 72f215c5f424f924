/*
 * orbfe_localmap.h -- the local map on the GPU (liborbfe.so, gfx950), over an orbfe_covis handle:
 * the ordered distinct union of keyframes' mvpMapPoints rows as a device pass, a per-point geometry
 * store beside the covisibility table, and the gather of the union from the store into an
 * orbfe_mappoint_geometry that never leaves HBM.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021), the three walks that collect "the points
 * of these keyframes, each once":
 *   Tracking::UpdateLocalPoints                           src/Tracking.cc:1228-1252
 *   LocalMapping::SearchInNeighbors, vpFuseCandidates     src/LocalMapping.cc:500-521
 *   LoopClosing::ComputeSim3, mvpLoopMapPoints            src/LoopClosing.cc:371-391
 * In each a stamp member of the MapPoint (mnTrackReferenceForFrame, mnFuseCandidateForKF,
 * mnLoopPointForKF) makes a point appear once, at its first occurrence in (keyframe list, slot)
 * order. The keyframe lists themselves come from graph state, which stays with the caller
 * (orb_slam2_2021_amd/covisibility.py: update_local_keyframes, fuse_targets, loop_map_points).
 *
 * Deviation, deliberate: the stamps start at 0 in the reference (MapPoint.cc:37-41), so a current
 * Frame / KeyFrame with mnId == 0 finds every point already stamped and collects nothing. That
 * artefact is not reproduced: every call behaves as though its stamp differs from all earlier ones
 * (as orbfe_kfdb.h does for mnRelocQuery / mnLoopQuery).
 *
 * Determinism. The device decides each point's first occurrence with an atomic minimum over the keys
 * (list position << 13 | slot) and places the winners with an order-preserving scan, so the result
 * is the same from run to run and equal to the serial walk.
 *
 * Cost. A per-frame call: every kernel and copy is proportional to the named rows' slots (list
 * entries x the longest named row, in 256-slot blocks) or to the result. Nothing runs over the
 * point-id range, except once per handle when the 4-byte-per-id scratch array is allocated and
 * filled, and after a call that a HIP error cut short (the scratch is then refilled whole).
 *
 * The inverse. These calls read rows and bad flags only: they neither need nor rebuild the inverse
 * of orbfe_covis.h and do not mark it stale.
 *
 * Bounds. A keyframe list holds 1 to 4096 entries (repeats count) and a row at most 8192 slots, so a
 * call sees at most 2^25 slots; a key has 25 bits and no further bound on the total is needed or
 * made. A seen list holds at most 8192 entries. All outputs are integers and byte copies, exact.
 */
#ifndef ORBFE_LOCALMAP_H
#define ORBFE_LOCALMAP_H
#include <stdint.h>

#include "orbfe.h"
#include "orbfe_covis.h"
#include "orbfe_frustum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_LOCALMAP_MAX_KEYFRAMES 4096
#define ORBFE_LOCALMAP_MAX_SEEN 8192

/* The ordered distinct union of rows. kf_ids: n_kf stored keyframe ids in the caller's order; an id
 * may repeat (SearchInNeighbors' vpTargetKFs can hold a second neighbour twice): a repeat adds
 * nothing and is no error. point_ids: every point that sits in a slot of a named row, is not -1 and
 * is not flagged bad, once, ordered by its first occurrence in (list position, slot) order -- the
 * order of the reference's push_backs.
 * point_capacity below the result: ORBFE_ERR_CAPACITY, n_points set to what is needed, point_ids
 * untouched. n_kf outside 1..4096: ORBFE_ERR_ARG below, ORBFE_ERR_CAPACITY above. An id that is not
 * stored: ORBFE_ERR_ARG, before any device work. A host-only handle: ORBFE_ERR_STATE after these
 * checks. Blocking: two synchronisations (the count, then the ids). */
typedef struct {
  int point_capacity;  /* in */
  int n_points;        /* out */
  int32_t* point_ids;  /* [point_capacity] */
} orbfe_covis_points_t;

int orbfe_covis_distinct_points(orbfe_covis* h, int n_kf, const int64_t* kf_ids, orbfe_covis_points_t* result);

/* The geometry store: 64 bytes per point id and one state byte, allocated for max_point_id ids by the
 * first set_point_geometry on a device handle. set_point_geometry creates or overwrites the entries of
 * n points from host arrays (world_pos n x 3, normal n x 3, min_distance n, max_distance n, descriptors
 * n x 32): SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors as the caller mirrors
 * them. flags: the bits to hand on with the point (ORBFE_MPF_OBSERVED, ...); ORBFE_MPF_BAD,
 * ORBFE_MPF_SEEN and ORBFE_MPF_TRACK_IN_VIEW belong to the calls below and are refused. An id outside
 * [0, max_point_id), an id named twice or a refused flag bit: ORBFE_ERR_ARG, nothing touched. The
 * upload goes through the handle's pinned staging, 65536 points at a time. orbfe_covis_clear empties
 * the store. On a host-only handle the checks run and nothing is stored. */
int orbfe_covis_set_point_geometry(orbfe_covis* h, int n, const int32_t* point_ids, const uint8_t* flags,
                                   const float* world_pos, const float* normal, const float* min_distance,
                                   const float* max_distance, const uint8_t* descriptors);

/* distinct_points, then the gather of those points from the store on the device.
 * geometry: m = n_points and six device pointers into buffers the handle owns, valid until the next
 *   call on the handle; entry i describes point_ids[i]. flags[i] = the stored bits, with ORBFE_MPF_SEEN
 *   when the point is in seen_point_ids (the Frame's mvpMapPoints: mnLastFrameSeen == mnId,
 *   Tracking.cc:1180, :1193; -1, bad ids and ids outside the result are skipped; at most 8192 entries,
 *   else ORBFE_ERR_CAPACITY; an id below -1: ORBFE_ERR_ARG, at or above max_point_id:
 *   ORBFE_ERR_CAPACITY). ORBFE_MPF_BAD is never set: bad points are not in the list.
 * point_ids comes back to the host too (to map best_idx to points), under the capacity protocol
 *   above; when the capacity is too small no geometry is returned (m = 0, NULL pointers).
 * A point of the result whose geometry was never set: ORBFE_ERR_STATE, n_missing = how many (counted
 *   on the device, read back with n_points), no geometry returned; n_points is still set.
 * Blocking: the handle's stream is synchronised before the call returns, so the view can go straight
 * into orbfe_search_local_points / orbfe_is_in_frustum, which read it on the matcher's own stream.
 * The buffers grow geometrically with the bound on m that is known before the kernels run (the named
 * rows' slots, at most max_point_id) and are not reallocated per call. */
typedef struct {
  int point_capacity;  /* in */
  int n_points;        /* out */
  int n_missing;       /* out */
  int32_t* point_ids;  /* [point_capacity], host */
  orbfe_mappoint_geometry geometry;  /* out: device pointers */
} orbfe_covis_local_geometry_t;

int orbfe_covis_local_geometry(orbfe_covis* h, int n_kf, const int64_t* kf_ids, int n_seen,
                               const int32_t* seen_point_ids, orbfe_covis_local_geometry_t* result);

#ifdef __cplusplus
}
#endif
#endif
