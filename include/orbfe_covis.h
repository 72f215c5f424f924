/*
 * orbfe_covis.h -- the covisibility walks on the GPU (liborbfe.so, gfx950): the keyframes'
 * mvpMapPoints rows stay on the device, the observations are derived from them there, and
 * UpdateConnections, UpdateLocalKeyFrames' vote and LocalBundleAdjustment's gather run over them.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   KeyFrame::UpdateConnections, the counting and ordering   src/KeyFrame.cc:304-378
 *   Tracking::UpdateLocalKeyFrames, first half               src/Tracking.cc:1257-1303
 *   Optimizer::LocalBundleAdjustment, the gather             src/Optimizer.cc:471-506
 * The graph state those calls write (mConnectedKeyFrameWeights, the ordered lists, the spanning
 * tree) stays with the caller: orb_slam2_2021_amd/covisibility.py keeps it for Python, the C++
 * adapter keeps the reference's own KeyFrame members.
 *
 * The table. One row per stored keyframe: the point id (MapPoint::mnId, used directly as an array
 * index, 0 <= id < max_point_id) in each keypoint slot, -1 for none; one bad flag per point id.
 * The inverse (point -> observing keyframes and slot, the reference's mObservations) is not an
 * input: it is derived on the device from the rows and rebuilt by the next query after a mutation.
 * The cullings at the end of this header (LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag's
 * EraseObservation cascade, LocalMapping::MapPointCulling) walk the same state and prune it in place.
 * Rules of that derivation:
 *   - A point's observers are the distinct keyframes whose row holds it, ascending in keyframe
 *     mnId. The slot recorded for a keyframe is the lowest one holding the point (the reference's
 *     map has one index per keyframe).
 *   - A point that occupies two slots of the querying row votes twice, as the loop at
 *     KeyFrame.cc:317-336 does. A point that occupies two slots of another keyframe's row counts
 *     once for that keyframe.
 *   - Only live keyframes are stored: where the reference's SetBadFlag erases a keyframe's
 *     observations, the caller calls orbfe_covis_erase_keyframe.
 *   - A bad point is skipped wherever the reference tests isBad(): as a slot of the querying row,
 *     as an entry of a vote list, as a point of a local row.
 *   - The rebuilt inverse is identical from run to run: every point's segment is put in
 *     (keyframe mnId, slot) order after the atomics have filled it.
 *   - Observations() (MapPoint::nObs) is derived too: the sum, over a point's distinct live
 *     observers, of 1 + STEREO(the observer's attribute byte at its recorded (lowest) slot). The
 *     octave KeyFrameCulling reads for an observer is the one at that same recorded slot.
 *
 * Attributes. One byte per row slot beside the rows (orbfe_covis_set_keyframe_attrs): what the two
 * cullings read of a keypoint. They are never part of the inverse; the three queries below do not
 * read them.
 *
 * The tie key. The reference orders keyframes by KeyFrame* (std::map<KeyFrame*, int> iteration,
 * sort of pair<int, KeyFrame*>), so equal weights are ordered by pointer value. tie_key stands for
 * that pointer: a uint64, unique among the stored keyframes (a duplicate: ORBFE_ERR_ARG). The C++
 * adapter passes the pointer, Python passes mnId. Every order below is stated in tie_key.
 *
 * Bounds: max_keyframes <= 4096, max_slots <= 8192, max_point_id <= 2^24 (13 bytes of device
 * memory per id); a vote list holds at most 8192 entries. A handle is not thread-safe.
 * All outputs are integers and exact.
 */
#ifndef ORBFE_COVIS_H
#define ORBFE_COVIS_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_covis orbfe_covis;

#define ORBFE_COVIS_MAX_KEYFRAMES 4096
#define ORBFE_COVIS_MAX_SLOTS 8192
#define ORBFE_COVIS_MAX_POINT_ID (1 << 24)

/* device < 0: a host-only handle (bookkeeping and argument checks work, the queries and the two
 * cullings return ORBFE_ERR_STATE after their argument checks). */
int orbfe_covis_create(int device, int max_keyframes, int max_slots, int max_point_id,
                       orbfe_covis** out);
int orbfe_covis_destroy(orbfe_covis* h);

/* Mutations: small host-to-device copies; each leaves the inverse stale until the next query.
 * Argument errors touch nothing. A point id >= max_point_id: ORBFE_ERR_CAPACITY; below -1:
 * ORBFE_ERR_ARG.
 *
 * set_keyframe: add a keyframe, or replace the whole row (and the tie key) of a stored one.
 *   n_slots > max_slots or a full store: ORBFE_ERR_CAPACITY; a tie key another keyframe holds:
 *   ORBFE_ERR_ARG.
 * set_slots: AddMapPoint / EraseMapPointMatch (-1) / ReplaceMapPointMatch on n slots of a stored
 *   row, applied in order (a slot named twice keeps the last id). A slot outside the row:
 *   ORBFE_ERR_ARG; an id that is not stored: ORBFE_ERR_STATE.
 * erase_keyframe: an id that is not stored: ORBFE_ERR_STATE.
 * set_points_bad: SetBadFlag (bad != 0) of n points, or its undoing. */
int orbfe_covis_set_keyframe(orbfe_covis* h, int64_t kf_id, uint64_t tie_key, int n_slots,
                             const int32_t* point_ids);
int orbfe_covis_set_slots(orbfe_covis* h, int64_t kf_id, int n, const int32_t* slots,
                          const int32_t* point_ids);
int orbfe_covis_erase_keyframe(orbfe_covis* h, int64_t kf_id);
int orbfe_covis_set_points_bad(orbfe_covis* h, int n, const int32_t* point_ids, int bad);
int orbfe_covis_clear(orbfe_covis* h);
int orbfe_covis_size(const orbfe_covis* h, int* n);

/* UpdateConnections of n keyframes (KeyFrame.cc:304-378). The counts depend on the table only,
 * never on graph state, so the loops at LoopClosing.cc:465-535 and :567-587 are one call each.
 * Query q writes entries q*capacity.. of the per-entry arrays:
 *   counter: KFcounter, every keyframe sharing at least one point with the query, the query
 *     itself excluded, ascending in tie_key (the map's iteration order; it becomes
 *     mConnectedKeyFrameWeights).
 *   ordered: the entries with weight >= th, descending in (weight, tie_key) (sort ascending, then
 *     push_front). If none reaches th: the single entry (nmax, kf_max).
 *   nmax, kf_max: the maximal weight and the first keyframe holding it in ascending tie_key (the
 *     strict > at :352).
 *   unchanged: 1, with everything else empty / 0 / -1, when KFcounter is empty (the early return
 *     at :339: the caller leaves the keyframe's state as it was).
 * One device pass, one synchronisation, one result copy for the whole batch. A query with more
 * counter entries than `capacity`: ORBFE_ERR_CAPACITY, the result arrays untouched
 * (orbfe_covis_size - 1 is always enough). A kf id that is not stored: ORBFE_ERR_ARG. */
typedef struct {
  int capacity;              /* in: entries per query */
  int32_t* n_counter;        /* [n] */
  int64_t* counter_ids;      /* [n * capacity] */
  int32_t* counter_weights;  /* [n * capacity] */
  int32_t* n_ordered;        /* [n] */
  int64_t* ordered_ids;      /* [n * capacity] */
  int32_t* ordered_weights;  /* [n * capacity] */
  int32_t* nmax;             /* [n] */
  int64_t* kf_max;           /* [n] */
  uint8_t* unchanged;        /* [n] */
} orbfe_covis_connections_t;

int orbfe_covis_update_connections(orbfe_covis* h, int n, const int64_t* kf_ids, int th,
                                   orbfe_covis_connections_t* result);

/* The vote of Tracking::UpdateLocalKeyFrames (Tracking.cc:1257-1303) for n_queries Frames: query q
 * is point_ids[begin[q] .. begin[q+1]) (the Frame's mvpMapPoints; -1 and bad points are skipped, a
 * point listed twice votes twice; at most 8192 entries per query). Per query: the voted keyframes
 * ascending in tie_key with their counts (mvpLocalKeyFrames' initial content and order), max and
 * kf_max by the same strict > rule. Nothing is excluded; an empty counter gives n = 0, max = 0,
 * kf_max = -1. Capacity as above (orbfe_covis_size is always enough). */
typedef struct {
  int capacity;      /* in: entries per query */
  int32_t* n;        /* [n_queries] */
  int64_t* kf_ids;   /* [n_queries * capacity] */
  int32_t* counts;   /* [n_queries * capacity] */
  int32_t* max;      /* [n_queries] */
  int64_t* kf_max;   /* [n_queries] */
} orbfe_covis_votes_t;

int orbfe_covis_vote(orbfe_covis* h, int n_queries, const int32_t* begin, const int32_t* point_ids,
                     orbfe_covis_votes_t* result);

/* The gather of LocalBundleAdjustment (Optimizer.cc:471-506) from lLocalKeyFrames (the keyframe and
 * its GetVectorCovisibleKeyFrames(), read from the caller's graph state; each id stored and named
 * once, else ORBFE_ERR_ARG), in the order orbfe_lba_problem_t wants:
 *   point_ids: the non-bad points in any local row, each once, ascending.
 *   fixed_ids: the observers of a local point that are not local, ascending in mnId.
 *   edge_begin[n_points + 1]: a CSR over the points; per edge the observing keyframe's index in
 *     (local ascending in mnId, then fixed ascending in mnId) and the observing slot. A point's
 *     edges are ascending in the observer's mnId.
 * A capacity below what the gather finds: ORBFE_ERR_CAPACITY, the arrays untouched and n_points,
 * n_fixed, n_edges set to what is needed. Two synchronisations: the counts, then the arrays. */
typedef struct {
  int point_capacity, fixed_capacity, edge_capacity;  /* in */
  int n_points, n_fixed, n_edges;
  int32_t* point_ids;   /* [point_capacity] */
  int64_t* fixed_ids;   /* [fixed_capacity] */
  int32_t* edge_begin;  /* [point_capacity + 1] */
  int32_t* edge_kf;     /* [edge_capacity] */
  int32_t* edge_slot;   /* [edge_capacity] */
} orbfe_covis_local_map_t;

int orbfe_covis_local_map(orbfe_covis* h, int n_local, const int64_t* local_kf_ids,
                          orbfe_covis_local_map_t* result);

/* The per-slot attributes of a stored keyframe: bits 0-4 mvKeysUn[i].octave, bit 5 mvuRight[i] >= 0,
 * bit 6 mvDepth[i] > mThDepth || mvDepth[i] < 0 as the caller evaluates it in float. n_slots other than
 * the stored row's length, or bit 7 set: ORBFE_ERR_ARG; an id that is not stored: ORBFE_ERR_STATE.
 * A keyframe's keypoints never change: set_keyframe on a stored keyframe keeps the attributes when the
 * row's length is unchanged and drops them when it differs; erase_keyframe and clear drop them. */
#define ORBFE_COVIS_ATTR_OCTAVE 0x1f
#define ORBFE_COVIS_ATTR_STEREO 0x20
#define ORBFE_COVIS_ATTR_FAR 0x40
int orbfe_covis_set_keyframe_attrs(orbfe_covis* h, int64_t kf_id, int n_slots, const uint8_t* attrs);

/* LocalMapping::KeyFrameCulling (LocalMapping.cc:640-706) over kf_ids, the current keyframe's
 * GetVectorCovisibleKeyFrames() in the caller's order, with what KeyFrame::SetBadFlag does to the map's
 * observations (KeyFrame.cc:486-488, MapPoint.cc:141-198). Candidates are decided in order and each sees
 * the culls before it:
 *   - a slot counts towards nMPs when it holds a point that is not bad and, unless monocular, its FAR
 *     bit is clear; it is redundant when Observations() > 3 (the candidate included) and at least 3
 *     other observers have octave <= the slot's octave + 1;
 *   - n_redundant > 0.9 * n_mps (an int against a double product) culls; n_mps == 0 keeps;
 *   - mnId 0 is skipped (3); a redundant candidate with not_erase[i] != 0 is reported (2, the
 *     reference's mbToBeErased) and changes nothing;
 *   - a culled keyframe leaves the table as by erase_keyframe; each point its row holds (at the first
 *     slot holding it, bad points skipped) loses the observer, and one whose Observations() falls to
 *     <= 2 gets the bad flag, is listed, and its id at the recorded slot of every remaining observer's
 *     row becomes -1 (EraseMapPointMatch(mit->second): that slot alone).
 * The inverse is left stale. Dependent device steps: keyframes culled + 1, each one 4-byte read-back.
 * Checks, before any device work: each id stored and named once, else ORBFE_ERR_ARG; every stored
 * keyframe has attributes, else ORBFE_ERR_STATE; bad_capacity, else ORBFE_ERR_CAPACITY. */
typedef struct {
  uint8_t* decision;     /* [n] 0 kept, 1 culled, 2 redundant but not_erase (mbToBeErased), 3 skipped (mnId 0) */
  int32_t* n_mps;        /* [n] nMPs as the reference counts it at this candidate's turn */
  int32_t* n_redundant;  /* [n] nRedundantObservations at this candidate's turn */
  int32_t* bad_begin;    /* [n + 1] CSR over the candidates into bad_points */
  int32_t* bad_points;   /* [bad_capacity] the points a culled candidate's EraseObservation made bad, in slot order */
  int bad_capacity;      /* in: >= the sum of the candidates' row lengths, else ORBFE_ERR_CAPACITY before anything runs */
} orbfe_covis_cull_t;

int orbfe_covis_cull_keyframes(orbfe_covis* h, int n, const int64_t* kf_ids, const uint8_t* not_erase,
                               int monocular, orbfe_covis_cull_t* result);

/* LocalMapping::MapPointCulling (LocalMapping.cc:174-209) over mlpRecentAddedMapPoints, one point each:
 *   1 leaves (was bad); 2 set bad: (float)found / visible < 0.25f (0/0 is NaN and is not <);
 *   3 set bad: (int)current - (int)first >= 2 and Observations() <= (monocular ? 2 : 3);
 *   4 leaves: the age >= 3; 0 stays in the list.
 * Actions 2 and 3 flag the point and write -1 at its observers' recorded slots, as above; the inverse is
 * left stale then. One launch, one result copy. A point named twice, an id outside [0, max_point_id),
 * a keyframe id outside [0, 2^31): ORBFE_ERR_ARG, nothing touched; a stored keyframe without
 * attributes: ORBFE_ERR_STATE. */
int orbfe_covis_cull_points(orbfe_covis* h, int n, const int32_t* point_ids, const int32_t* found,
                            const int32_t* visible, const int64_t* first_kf_id, int64_t current_kf_id,
                            int monocular, uint8_t* action);

#ifdef __cplusplus
}
#endif
#endif
