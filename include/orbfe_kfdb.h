/*
 * orbfe_kfdb.h -- KeyFrameDatabase on the GPU (liborbfe.so, gfx950): the keyframes' BowVectors
 * stay on the device and the two place-recognition queries run there.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   KeyFrameDatabase ctor / add / erase / clear              src/KeyFrameDatabase.cc:33-72
 *   DetectLoopCandidates(KeyFrame*, float minScore)          :74-199
 *   DetectRelocalizationCandidates(Frame*)                   :201-315
 *   L1Scoring::score            Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
 * called by LoopClosing::DetectLoop and Tracking::Relocalization between ComputeBoW
 * (orbfe_vocab_transform*) and the per-candidate SearchByBoW (orbfe_search_by_bow_kf_frame_multi).
 *
 * A query returns the keyframes the reference returns, in its order, with bit-equal float scores:
 *   - score: the common words' terms fabs(vi - wi) - fabs(vi) - fabs(wi) (vi the query's weight)
 *     are summed in double, strictly left to right in ascending word order, then -score / 2.0,
 *     narrowed to float.
 *   - lKFsSharingWords order: ascending (smallest common word id, add sequence); an erased and
 *     re-added keyframe takes a new, later sequence number. Every later list inherits it.
 *   - minCommonWords = (int)(maxCommonWords * 0.8f); scored iff words > minCommonWords.
 *   - The covisibility accumulation reads the neighbour table set with orbfe_kfdb_set_covisible
 *     (GetBestCovisibilityKeyFrames(10) order). A neighbour id that is not stored does not count.
 *     RELOC counts every neighbour in the sharing list and adds its mRelocScore, which persists
 *     from the last query that scored it (:278-281); LOOP counts a neighbour iff it was scored in
 *     this query (:161), also when minScore dropped it from lScoreAndMatch.
 *   - LOOP: the excluded ids (GetConnectedKeyFrames) never enter the sharing list.
 * Deviations, both deliberate:
 *   - The reference never initialises mRelocScore (KeyFrame.cc:35). Here it is 0.0f from add.
 *   - Every query behaves as though its id differs from all earlier ones. The reference's
 *     artefact for a Frame / KeyFrame with mnId == 0 (mnRelocQuery / mnLoopQuery start at 0, so
 *     such a query finds nothing) is not reproduced.
 * The neighbour table belongs to the stored keyframe: erase drops it, add starts it empty.
 *
 * Only L1 scoring (ORBvoc's) is implemented. Bounds: max_keyframes <= 16384 (the sharing list is
 * sorted inside one workgroup's LDS), max_words_per_kf and the query <= 8192 words.
 * A handle is not thread-safe: one call at a time (the reference holds mMutex).
 */
#ifndef ORBFE_KFDB_H
#define ORBFE_KFDB_H
#include <stdint.h>

#include "orbfe.h"
#include "orbfe_vocab.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_kfdb orbfe_kfdb;

#define ORBFE_KFDB_MAX_KEYFRAMES 16384
#define ORBFE_KFDB_MAX_WORDS 8192
#define ORBFE_KFDB_COVISIBLE 10

enum { ORBFE_KFDB_RELOC = 0, ORBFE_KFDB_LOOP = 1 };

/* device < 0: a host-only handle (bookkeeping and argument checks work, queries and the device
 * add return ORBFE_ERR_STATE). The vocabulary gives n_words and must score with L1. */
int orbfe_kfdb_create(const orbfe_vocabulary* voc, int max_keyframes, int max_words_per_kf,
                      int device, orbfe_kfdb** out);
int orbfe_kfdb_destroy(orbfe_kfdb* db);

/* add(pKF): the keyframe's BowVector from host memory. words ascending and < n_words,
 * n <= max_words_per_kf. A kf_id already stored: ORBFE_ERR_STATE; a full store: ORBFE_ERR_CAPACITY. */
int orbfe_kfdb_add(orbfe_kfdb* db, int64_t kf_id, const uint32_t* words, const double* weights,
                   int n);
/* n keyframes straight from orbfe_vocab_transform_batch_device's output (image i at
 * d_bow_words + i*cap, d_bow_weights + i*cap, count d_bow_n[i]), with no host copy of the
 * vectors. stream: where the transform was enqueued (NULL: its output is complete). All or
 * nothing; a count above max_words_per_kf: ORBFE_ERR_CAPACITY. Returns after the copy. */
int orbfe_kfdb_add_batch_device(orbfe_kfdb* db, int n, const int64_t* kf_ids_host,
                                const uint32_t* d_bow_words, const double* d_bow_weights,
                                const int32_t* d_bow_n, int cap, void* stream);
/* erase(pKF) (an id that is not stored: ORBFE_ERR_STATE), clear(), number of stored keyframes */
int orbfe_kfdb_erase(orbfe_kfdb* db, int64_t kf_id);
int orbfe_kfdb_clear(orbfe_kfdb* db);
int orbfe_kfdb_size(const orbfe_kfdb* db, int* n);
/* pKF->GetBestCovisibilityKeyFrames(10), in that order (n <= 10; ids need not be stored). */
int orbfe_kfdb_set_covisible(orbfe_kfdb* db, int64_t kf_id, const int64_t* ids, int n);

typedef struct {
  int mode;                 /* ORBFE_KFDB_RELOC / ORBFE_KFDB_LOOP */
  int n;                    /* words in the query BowVector (<= 8192); with d_n: their bound */
  const uint32_t* words;    /* ascending */
  const double* weights;
  int on_device;            /* words / weights are device pointers (not checked) */
  const int32_t* d_n;       /* on_device only, optional: device count (d_bow_n + i) */
  void* stream;             /* on_device only: where the vectors were produced (NULL: complete) */
  float min_score;          /* LOOP: minScore */
  const int64_t* excluded;  /* LOOP: pKF->GetConnectedKeyFrames() (ids not stored are ignored) */
  int n_excluded;
} orbfe_kfdb_query_t;

typedef struct {
  int capacity;             /* in: entries each array below holds (>= orbfe_kfdb_size is enough) */
  /* stage 1: lKFsSharingWords in discovery order */
  int n_sharing;
  int max_common, min_common;
  int64_t* kf_ids;          /* [capacity] */
  int32_t* common_words;    /* mnRelocWords / mnLoopWords */
  uint8_t* scored;          /* 1: common_words > min_common */
  float* scores;            /* si where scored, else 0 */
  /* stage 2: vpRelocCandidates / vpLoopCandidates */
  int n_candidates;
  int64_t* candidates;      /* [capacity] */
} orbfe_kfdb_result_t;

/* One query: one device pass, one host synchronisation, the result back in one copy. Both stages
 * are always produced; an adapter that keeps the live covisibility graph on the host reads
 * stage 1 and accumulates itself. */
int orbfe_kfdb_query(orbfe_kfdb* db, const orbfe_kfdb_query_t* query, orbfe_kfdb_result_t* result);

#ifdef __cplusplus
}
#endif
#endif
