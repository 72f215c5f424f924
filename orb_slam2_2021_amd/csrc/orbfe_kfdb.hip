// orbfe_kfdb.hip -- KeyFrameDatabase on gfx950: the stored keyframes' BowVectors as a device
// forward index, DetectRelocalizationCandidates / DetectLoopCandidates as two kernels.
//
// Reference: src/KeyFrameDatabase.cc:33-315, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
// (L1Scoring::score). include/orbfe_kfdb.h lists the semantics that are reproduced.
//
// Device layout: slot s of max_keyframes holds a keyframe's sorted (word, weight) run at
// words + s*W, weights + s*W (W = max_words_per_kf), its count n[s] (-1: free / erased), its
// order position pos[s] and its persistent mRelocScore reloc[s]. Positions are handed out in add
// order from a counter below 2*max_keyframes (slot_at_pos is the inverse table); when the counter
// runs out the live slots are renumbered in order, so (first common word, pos) is the
// reference's discovery order and fits one 64-bit sort key. An erase only writes n[s] = -1.
//
// k_kfdb_sweep: the query's words staged in LDS (<= 32 KiB); one wave per slot walks the slot's
//   run 64 words at a time, each lane looks its word up in the query (branch-free lower bound) and
//   forms the word's term; the wave then adds the hit lanes' terms into one double strictly in lane
//   order = ascending word order (the reference's summation order; no tree reduction). Per slot:
//   common-word count, index of the first common word in the query, float score.
// k_kfdb_finish: one workgroup. Collects the slots with common > 0, bitonic-sorts their keys in
//   LDS, applies minCommonWords = (int)(max * 0.8f), writes stage 1 and mRelocScore where the
//   reference assigns it, accumulates over the neighbour table (float, neighbour order, strict >),
//   takes bestAccScore, and emits each pBestKF once in list order.
// k_kfdb_add: copies BowVectors (device batch layout or the host staging) into their slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <functional>
#include <queue>
#include <unordered_map>
#include <vector>

#include "../../include/orbfe.h"
#include "../../include/orbfe_kfdb.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_stage.h"

#define KFDB_SWEEP_THREADS 256
#define KFDB_FIN_THREADS 1024
#define KFDB_NEIGH ORBFE_KFDB_COVISIBLE

struct KfdbStore {
  uint32_t* words;     // [M * W]
  double* weights;     // [M * W]
  int32_t* n;          // [M] words in the slot, -1: free
  uint32_t* pos;       // [M] order position
  int32_t* slot_at_pos;  // [2M]
  float* reloc;        // [M] mRelocScore
  int W;
};

struct KfdbAddArgs {
  KfdbStore st;
  const int32_t* slots;  // [n] destination slot
  const uint32_t* poss;  // [n] its order position
  const uint32_t* src_words;
  const double* src_weights;
  const int32_t* src_n;
  int cap;               // source stride
  int32_t* counts_out;   // [n] the source counts, for the host's check
};

// One workgroup per keyframe. A count outside 0..min(W, cap) leaves the slot free.
__global__ __launch_bounds__(256) void k_kfdb_add(KfdbAddArgs a) {
  const int i = blockIdx.x;
  const int slot = a.slots[i];
  const int cnt = a.src_n[i];
  const bool ok = cnt >= 0 && cnt <= a.st.W && cnt <= a.cap;
  if (ok) {
    const uint32_t* sw = a.src_words + (size_t)i * a.cap;
    const double* sv = a.src_weights + (size_t)i * a.cap;
    uint32_t* dw = a.st.words + (size_t)slot * a.st.W;
    double* dv = a.st.weights + (size_t)slot * a.st.W;
    for (int k = threadIdx.x; k < cnt; k += blockDim.x) {
      dw[k] = sw[k];
      dv[k] = sv[k];
    }
  }
  if (threadIdx.x == 0) {
    a.counts_out[i] = cnt;
    a.st.n[slot] = ok ? cnt : -1;
    a.st.pos[slot] = a.poss[i];
    a.st.slot_at_pos[a.poss[i]] = slot;
    a.st.reloc[slot] = 0.0f;
  }
}

struct KfdbSweepArgs {
  KfdbStore st;
  int hi;                    // slots 0..hi-1 have been used
  const uint32_t* q_words;
  const double* q_weights;
  const int32_t* q_n_dev;    // optional device count
  int q_n;                   // count, or its bound with q_n_dev
  const int32_t* excl;       // sorted slots of the LOOP query's connected set
  int n_excl;
  int32_t* common;           // [hi] out
  uint32_t* first;           // [hi] out: query index of the smallest common word
  float* si;                 // [hi] out
};

__global__ __launch_bounds__(KFDB_SWEEP_THREADS) void k_kfdb_sweep(KfdbSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_q[];  // q_n words
  const int qn = a.q_n_dev ? max(0, min(*a.q_n_dev, a.q_n)) : a.q_n;
  for (int i = threadIdx.x; i < qn; i += KFDB_SWEEP_THREADS) s_q[i] = a.q_words[i];
  __syncthreads();
  const int lane = lane_id();
  const int nwaves = (int)gridDim.x * (KFDB_SWEEP_THREADS / 64);
  for (int s = (int)blockIdx.x * (KFDB_SWEEP_THREADS / 64) + wave_id(); s < a.hi; s += nwaves) {
    const int n = min(a.st.n[s], a.st.W);
    bool skip = n <= 0;
    if (!skip && a.n_excl > 0) {  // connected keyframes never enter the sharing list (:95)
      int lo = 0, hi = a.n_excl;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.excl[mid] < s) lo = mid + 1; else hi = mid;
      }
      skip = lo < a.n_excl && a.excl[lo] == s;
    }
    int common = 0;
    uint32_t first = 0;
    double score = 0.0;
    if (!skip) {
      const uint32_t* kw = a.st.words + (size_t)s * a.st.W;
      const double* kv = a.st.weights + (size_t)s * a.st.W;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool hit = false;
        double term = 0.0;
        int j = 0;
        if (i < n) {
          const uint32_t w = kw[i];
          // number of query words < w
          for (int step = ORBFE_KFDB_MAX_WORDS; step > 0; step >>= 1) {
            const int t = j + step;
            if (t <= qn && s_q[t - 1] < w) j = t;
          }
          if (j < qn && s_q[j] == w) {
            hit = true;
            const double vi = a.q_weights[j], wi = kv[i];
            term = fabs(vi - wi) - fabs(vi) - fabs(wi);  // ScoringObject.cpp:41
          }
        }
        uint64_t m = wave_ballot(hit);
        if (m) {
          if (common == 0) first = (uint32_t)__shfl(j, __ffsll((unsigned long long)m) - 1, 64);
          common += __popcll(m);
          while (m) {  // one add per common word, ascending: the order is the result
            score += __shfl(term, __ffsll((unsigned long long)m) - 1, 64);
            m &= m - 1;
          }
        }
      }
    }
    if (lane == 0) {
      a.common[s] = common;
      a.first[s] = first;
      a.si[s] = (float)(-score / 2.0);  // :65, then `float si =`
    }
  }
}

struct KfdbFinishArgs {
  int hi, mode;
  float min_score;
  const int32_t* common;
  const uint32_t* first;
  const float* si;
  const uint32_t* pos;
  const int32_t* slot_at_pos;
  const int32_t* neigh;   // [hi * 10] neighbour slots, -1: none / not stored
  float* reloc;
  int32_t* first_idx;     // [hi] scratch: first list index naming the slot as pBestKF
  float* acc;             // [hi] scratch per list entry
  int32_t* best;          // [hi] scratch per list entry: pBestKF's slot, -1: not in lScoreAndMatch
  // result (one buffer): hdr {n_sharing, max_common, min_common, n_candidates}, then hi-strided
  int32_t* hdr;
  int32_t* r_slot;
  int32_t* r_common;
  int32_t* r_scored;
  float* r_score;
  int32_t* r_cand;
};

__global__ __launch_bounds__(KFDB_FIN_THREADS) void k_kfdb_finish(KfdbFinishArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];  // pow2 >= hi
  __shared__ int s_cnt, s_max, s_base;
  __shared__ int s_wtot[KFDB_FIN_THREADS / 64];
  __shared__ float s_wbest[KFDB_FIN_THREADS / 64];
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  if (tid == 0) {
    s_cnt = 0;
    s_max = 0;
    s_base = 0;
  }
  __syncthreads();
  // lKFsSharingWords (unordered) and maxCommonWords
  int lmax = 0;
  for (int s = tid; s < a.hi; s += KFDB_FIN_THREADS) {
    const int c = a.common[s];
    if (c > 0) {
      const int k = atomicAdd(&s_cnt, 1);
      s_keys[k] = ((unsigned long long)a.first[s] << 32) | a.pos[s];
      lmax = max(lmax, c);
    }
  }
  lmax = wave_max(lmax);
  if (lane == 0) atomicMax(&s_max, lmax);
  __syncthreads();
  const int S = s_cnt;
  if (S == 0) {  // :106 / :226
    if (tid < 4) a.hdr[tid] = 0;
    return;
  }
  int P2 = 64;
  while (P2 < S) P2 <<= 1;
  for (int i = S + tid; i < P2; i += KFDB_FIN_THREADS) s_keys[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += KFDB_FIN_THREADS) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long u = s_keys[i], v = s_keys[x];
          if ((u > v) == ((i & k) == 0)) {
            s_keys[i] = v;
            s_keys[x] = u;
          }
        }
      }
      __syncthreads();
    }
  }
  const int maxc = s_max;
  const int minc = (int)((float)maxc * 0.8f);  // int minCommonWords = maxCommonWords * 0.8f
  const bool loop = a.mode == ORBFE_KFDB_LOOP;
  // stage 1 in list order; mRelocScore where :254 assigns it
  for (int i = tid; i < S; i += KFDB_FIN_THREADS) {
    const int slot = a.slot_at_pos[(uint32_t)s_keys[i]];
    const int c = a.common[slot];
    const bool scored = c > minc;
    const float sc = scored ? a.si[slot] : 0.0f;
    a.r_slot[i] = slot;
    a.r_common[i] = c;
    a.r_scored[i] = scored ? 1 : 0;
    a.r_score[i] = sc;
    a.first_idx[slot] = INT_MAX;
    if (!loop && scored) a.reloc[slot] = sc;
    s_keys[i] = (unsigned long long)slot;
  }
  __threadfence();
  __syncthreads();
  // accumulate by covisibility (:148-175 / :265-292)
  float lbest = loop ? a.min_score : 0.0f;
  for (int i = tid; i < S; i += KFDB_FIN_THREADS) {
    const int slot = (int)s_keys[i];
    const float s0 = a.si[slot];
    bool in_list = a.common[slot] > minc;
    if (loop && !(s0 >= a.min_score)) in_list = false;  // :137
    int bslot = -1;
    if (in_list) {
      float acc = s0, bs = s0;
      bslot = slot;
      for (int t = 0; t < KFDB_NEIGH; t++) {
        const int nb = a.neigh[(size_t)slot * KFDB_NEIGH + t];
        if (nb < 0) continue;
        const int cn = a.common[nb];
        if (loop ? !(cn > minc) : !(cn > 0)) continue;  // :161 / :278
        const float sn = loop ? a.si[nb] : a.reloc[nb];
        acc += sn;
        if (sn > bs) {
          bslot = nb;
          bs = sn;
        }
      }
      a.acc[i] = acc;
      if (acc > lbest) lbest = acc;
    }
    a.best[i] = bslot;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lbest = fmaxf(lbest, __shfl_xor(lbest, o, 64));
  if (lane == 0) s_wbest[wave] = lbest;
  __syncthreads();
  float best_acc = s_wbest[0];
  for (int w = 1; w < KFDB_FIN_THREADS / 64; w++) best_acc = fmaxf(best_acc, s_wbest[w]);
  const float min_retain = 0.75f * best_acc;
  // each pBestKF once, first occurrence first
  for (int i = tid; i < S; i += KFDB_FIN_THREADS) {
    const int b = a.best[i];
    if (b >= 0 && a.acc[i] > min_retain) atomicMin(&a.first_idx[b], i);
  }
  __threadfence();
  __syncthreads();
  for (int c0 = 0; c0 < S; c0 += KFDB_FIN_THREADS) {
    const int i = c0 + tid;
    bool emit = false;
    int b = -1;
    if (i < S) {
      b = a.best[i];
      emit = b >= 0 && a.acc[i] > min_retain &&
             __hip_atomic_load(&a.first_idx[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i;
    }
    const uint64_t m = wave_ballot(emit);
    if (lane == 0) s_wtot[wave] = __popcll(m);
    __syncthreads();
    int off = s_base, total = 0;
    for (int w = 0; w < KFDB_FIN_THREADS / 64; w++) {
      if (w < wave) off += s_wtot[w];
      total += s_wtot[w];
    }
    if (emit) a.r_cand[off + prefix_in_wave(m)] = b;
    __syncthreads();
    if (tid == 0) s_base += total;
    __syncthreads();
  }
  if (tid == 0) {
    a.hdr[0] = S;
    a.hdr[1] = maxc;
    a.hdr[2] = minc;
    a.hdr[3] = s_base;
  }
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_kfdb : OrbfeDev {
  int n_words = 0;
  int M = 0, W = 0;
  // bookkeeping (also on a host-only handle)
  std::unordered_map<int64_t, int> slot_of;
  std::vector<int64_t> id_of;                 // [M], valid where live
  std::vector<uint8_t> live;                  // [M]
  std::vector<uint32_t> pos;                  // [M]
  std::vector<std::vector<int64_t>> covis;    // [M]
  std::priority_queue<int, std::vector<int>, std::greater<int>> free_slots;  // below hi
  int hi = 0;             // slots ever used
  uint32_t next_pos = 0;  // < 2M
  bool neigh_dirty = true;
  // device
  hipEvent_t ev = nullptr;
  KfdbStore st{};
  int32_t* d_neigh = nullptr;      // [M * 10]
  int32_t* d_common = nullptr;     // [M]
  uint32_t* d_first = nullptr;     // [M]
  float* d_si = nullptr;           // [M]
  int32_t* d_first_idx = nullptr;  // [M]
  float* d_acc = nullptr;          // [M]
  int32_t* d_best = nullptr;       // [M]
  int32_t* d_res = nullptr;        // 4 + 5M
  int32_t* h_res = nullptr;        // pinned
  uint8_t* d_stage = nullptr;      // upload staging: a query / a host add / slot lists
  uint8_t* h_stage = nullptr;      // pinned
  size_t stage_bytes = 0;
  std::vector<int32_t> neigh_host;
};


static void kfdb_reset_host(orbfe_kfdb* db) {
  db->slot_of.clear();
  db->id_of.assign(db->M, 0);
  db->live.assign(db->M, 0);
  db->pos.assign(db->M, 0);
  db->covis.assign(db->M, {});
  db->free_slots = {};
  db->hi = 0;
  db->next_pos = 0;
  db->neigh_dirty = true;
}

extern "C" int orbfe_kfdb_create(const orbfe_vocabulary* voc, int max_keyframes,
                                 int max_words_per_kf, int device, orbfe_kfdb** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_create: bad argument");
  *out = nullptr;
  orbfe_vocab_info info;
  if (!voc || orbfe_vocab_get_info(voc, &info) != ORBFE_OK)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_create: no vocabulary");
  if (info.scoring != ORBFE_VOC_L1_NORM)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_kfdb_create: only L1_NORM scoring (ORBvoc's) is implemented");
  if (max_keyframes < 1 || max_keyframes > ORBFE_KFDB_MAX_KEYFRAMES || max_words_per_kf < 1 ||
      max_words_per_kf > ORBFE_KFDB_MAX_WORDS)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_kfdb_create: max_keyframes in 1..16384, max_words_per_kf in 1..8192");
  orbfe_kfdb* db = new orbfe_kfdb();
  db->n_words = info.n_words;
  db->M = max_keyframes;
  db->W = max_words_per_kf;
  db->st.W = db->W;
  kfdb_reset_host(db);
  if (device < 0) {
    *out = db;
    return ORBFE_OK;
  }
  const int open_st = orbfe_dev_open(db, device, "orbfe_kfdb_create");
  if (open_st != ORBFE_OK) {
    orbfe_kfdb_destroy(db);
    return open_st;
  }
  const size_t M = (size_t)db->M, W = (size_t)db->W;
  // staging: a query (words, weights, excluded slots) or a host add (words, weights, count) or
  // a device batch (slots, positions, counts back)
  db->stage_bytes = orbfe_al256(4 * (size_t)ORBFE_KFDB_MAX_WORDS) + orbfe_al256(8 * (size_t)ORBFE_KFDB_MAX_WORDS) +
                    3 * orbfe_al256(4 * M) + 256;
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipEventCreateWithFlags(&db->ev, hipEventDisableTiming));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->st.words, 4 * M * W));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->st.weights, 8 * M * W));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->st.n, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->st.pos, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->st.slot_at_pos, 4 * 2 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->st.reloc, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_neigh, 4 * M * KFDB_NEIGH));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_common, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_first, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_si, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_first_idx, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_acc, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_best, 4 * M));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_res, 4 * (4 + 5 * M)));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipHostMalloc(&db->h_res, 4 * (4 + 5 * M), hipHostMallocDefault));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMalloc(&db->d_stage, db->stage_bytes));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipHostMalloc(&db->h_stage, db->stage_bytes, hipHostMallocDefault));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMemsetAsync(db->st.n, 0xff, 4 * M, db->stream));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipMemsetAsync(db->st.slot_at_pos, 0, 4 * 2 * M, db->stream));
  // k_kfdb_finish sorts up to 16384 64-bit keys in LDS (128 KiB of the CU's 160 KiB)
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy,
                   hipFuncSetAttribute((const void*)k_kfdb_finish, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       8 * ORBFE_KFDB_MAX_KEYFRAMES));
  ORBFE_CREATE_HIP(db, orbfe_kfdb_destroy, hipStreamSynchronize(db->stream));
  *out = db;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_destroy(orbfe_kfdb* db) {
  if (!db) return ORBFE_OK;
  if (orbfe_dev_close(db)) {
    hipFree(db->st.words);
    hipFree(db->st.weights);
    hipFree(db->st.n);
    hipFree(db->st.pos);
    hipFree(db->st.slot_at_pos);
    hipFree(db->st.reloc);
    hipFree(db->d_neigh);
    hipFree(db->d_common);
    hipFree(db->d_first);
    hipFree(db->d_si);
    hipFree(db->d_first_idx);
    hipFree(db->d_acc);
    hipFree(db->d_best);
    hipFree(db->d_res);
    hipFree(db->d_stage);
    if (db->h_res) hipHostFree(db->h_res);
    if (db->h_stage) hipHostFree(db->h_stage);
    if (db->ev) hipEventDestroy(db->ev);
  }
  delete db;
  return ORBFE_OK;
}

// Positions for n more keyframes. When the counter would pass 2M the live slots are renumbered
// 0.. in their order (at most M live, so at least M adds separate two renumberings).
static int kfdb_reserve_positions(orbfe_kfdb* db, int n) {
  if ((size_t)db->next_pos + (size_t)n <= 2 * (size_t)db->M) return ORBFE_OK;
  std::vector<int> order;
  for (int s = 0; s < db->hi; s++)
    if (db->live[s]) order.push_back(s);
  std::sort(order.begin(), order.end(), [&](int x, int y) { return db->pos[x] < db->pos[y]; });
  std::vector<int32_t> inv(2 * (size_t)db->M, 0);
  for (size_t r = 0; r < order.size(); r++) {
    db->pos[order[r]] = (uint32_t)r;
    inv[r] = order[r];
  }
  db->next_pos = (uint32_t)order.size();
  if (db->device >= 0) {
    ORBFE_HIP_CHECK(hipStreamSynchronize(db->stream));
    ORBFE_HIP_CHECK(hipMemcpy(db->st.pos, db->pos.data(), 4 * (size_t)db->M, hipMemcpyHostToDevice));
    ORBFE_HIP_CHECK(hipMemcpy(db->st.slot_at_pos, inv.data(), 4 * inv.size(), hipMemcpyHostToDevice));
  }
  return ORBFE_OK;
}

static int kfdb_take_slot(orbfe_kfdb* db) {
  if (!db->free_slots.empty()) {
    const int s = db->free_slots.top();
    db->free_slots.pop();
    return s;
  }
  return db->hi++;
}

static void kfdb_commit(orbfe_kfdb* db, int slot, int64_t id, uint32_t pos) {
  db->slot_of[id] = slot;
  db->id_of[slot] = id;
  db->live[slot] = 1;
  db->pos[slot] = pos;
  db->covis[slot].clear();
  db->neigh_dirty = true;
}

static void kfdb_release(orbfe_kfdb* db, int slot) {
  db->slot_of.erase(db->id_of[slot]);
  db->live[slot] = 0;
  db->covis[slot].clear();
  db->free_slots.push(slot);
  db->neigh_dirty = true;
}

extern "C" int orbfe_kfdb_add(orbfe_kfdb* db, int64_t kf_id, const uint32_t* words,
                              const double* weights, int n) {
  if (!db || n < 0 || (n > 0 && (!words || !weights)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_add: bad argument");
  if (n > db->W) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_kfdb_add: more words than max_words_per_kf");
  for (int i = 0; i < n; i++) {
    if (words[i] >= (uint32_t)db->n_words)
      return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_add: word id >= the vocabulary's n_words");
    if (i > 0 && words[i] <= words[i - 1])
      return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_add: word ids must be strictly ascending");
  }
  if (db->slot_of.count(kf_id)) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_kfdb_add: keyframe id already stored");
  if ((int)db->slot_of.size() >= db->M) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_kfdb_add: the store is full");
  int st = kfdb_reserve_positions(db, 1);
  if (st) return st;
  const int slot = kfdb_take_slot(db);
  const uint32_t pos = db->next_pos++;
  if (db->device >= 0) {
    hipSetDevice(db->device);
    // staging: words | weights | {slot, pos, n, count back}
    const size_t o_w = 0, o_v = orbfe_al256(4 * (size_t)ORBFE_KFDB_MAX_WORDS);
    const size_t o_m = o_v + orbfe_al256(8 * (size_t)ORBFE_KFDB_MAX_WORDS);
    if (n > 0) {
      memcpy(db->h_stage + o_w, words, 4 * (size_t)n);
      memcpy(db->h_stage + o_v, weights, 8 * (size_t)n);
    }
    int32_t* hm = reinterpret_cast<int32_t*>(db->h_stage + o_m);
    hm[0] = slot;
    hm[1] = (int32_t)pos;
    hm[2] = n;
    hipError_t e = hipSuccess;
    if (n > 0) {
      e = hipMemcpyAsync(db->d_stage + o_w, db->h_stage + o_w, 4 * (size_t)n, hipMemcpyHostToDevice, db->stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(db->d_stage + o_v, db->h_stage + o_v, 8 * (size_t)n, hipMemcpyHostToDevice, db->stream);
    }
    if (e == hipSuccess)
      e = hipMemcpyAsync(db->d_stage + o_m, hm, 12, hipMemcpyHostToDevice, db->stream);
    if (e == hipSuccess) {
      KfdbAddArgs a;
      a.st = db->st;
      int32_t* dm = reinterpret_cast<int32_t*>(db->d_stage + o_m);
      a.slots = dm;
      a.poss = reinterpret_cast<const uint32_t*>(dm + 1);
      a.src_n = dm + 2;
      a.counts_out = dm + 3;
      a.src_words = reinterpret_cast<const uint32_t*>(db->d_stage + o_w);
      a.src_weights = reinterpret_cast<const double*>(db->d_stage + o_v);
      a.cap = ORBFE_KFDB_MAX_WORDS;
      ORBFE_LAUNCH("k_kfdb_add", k_kfdb_add, dim3(1), dim3(256), 0, db->stream, a);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) {
      db->free_slots.push(slot);
      return orbfe_set_hip_error(e, "orbfe_kfdb_add");
    }
  }
  kfdb_commit(db, slot, kf_id, pos);
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_add_batch_device(orbfe_kfdb* db, int n, const int64_t* kf_ids_host,
                                           const uint32_t* d_bow_words, const double* d_bow_weights,
                                           const int32_t* d_bow_n, int cap, void* stream) {
  if (db && db->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "keyframe database is host-only (device < 0)");
  if (!db || n < 0 || cap < 1 || cap > ORBFE_KFDB_MAX_WORDS ||
      (n > 0 && (!kf_ids_host || !d_bow_words || !d_bow_weights || !d_bow_n)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_add_batch_device: bad argument");
  if (n == 0) return ORBFE_OK;
  for (int i = 0; i < n; i++) {
    if (db->slot_of.count(kf_ids_host[i]))
      return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_kfdb_add_batch_device: keyframe id already stored");
    for (int k = 0; k < i; k++)
      if (kf_ids_host[k] == kf_ids_host[i])
        return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_add_batch_device: an id appears twice");
  }
  if ((size_t)db->slot_of.size() + (size_t)n > (size_t)db->M)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_kfdb_add_batch_device: the store is full");
  hipSetDevice(db->device);
  int st = kfdb_reserve_positions(db, n);
  if (st) return st;
  // staging: slots | positions | counts back (each n <= M ints)
  const size_t b = orbfe_al256(4 * (size_t)db->M);
  int32_t* hs = reinterpret_cast<int32_t*>(db->h_stage);
  int32_t* hp = reinterpret_cast<int32_t*>(db->h_stage + b);
  int32_t* hc = reinterpret_cast<int32_t*>(db->h_stage + 2 * b);
  std::vector<int> slots(n);
  for (int i = 0; i < n; i++) {
    slots[i] = kfdb_take_slot(db);
    hs[i] = slots[i];
    hp[i] = (int32_t)(db->next_pos + (uint32_t)i);
  }
  auto give_back = [&]() {
    for (int s : slots) db->free_slots.push(s);
  };
  hipError_t e = hipSuccess;
  if (stream) {  // the BowVectors are complete once `stream` reaches this point
    e = hipEventRecord(db->ev, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(db->stream, db->ev, 0);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(db->d_stage, hs, 4 * (size_t)n, hipMemcpyHostToDevice, db->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(db->d_stage + b, hp, 4 * (size_t)n, hipMemcpyHostToDevice, db->stream);
  if (e == hipSuccess) {
    KfdbAddArgs a;
    a.st = db->st;
    a.slots = reinterpret_cast<const int32_t*>(db->d_stage);
    a.poss = reinterpret_cast<const uint32_t*>(db->d_stage + b);
    a.src_words = d_bow_words;
    a.src_weights = d_bow_weights;
    a.src_n = d_bow_n;
    a.cap = cap;
    a.counts_out = reinterpret_cast<int32_t*>(db->d_stage + 2 * b);
    ORBFE_LAUNCH("k_kfdb_add", k_kfdb_add, dim3(n), dim3(256), 0, db->stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hc, db->d_stage + 2 * b, 4 * (size_t)n, hipMemcpyDeviceToHost, db->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
  if (e != hipSuccess) {
    give_back();
    return orbfe_set_hip_error(e, "orbfe_kfdb_add_batch_device");
  }
  bool ok = true;
  for (int i = 0; i < n; i++) ok = ok && hc[i] >= 0 && hc[i] <= db->W && hc[i] <= cap;
  if (!ok) {  // all or nothing: free the slots the kernel filled
    for (int s : slots) hipMemsetAsync(db->st.n + s, 0xff, 4, db->stream);
    hipStreamSynchronize(db->stream);
    give_back();
    return orbfe_set_error(ORBFE_ERR_CAPACITY,
                           "orbfe_kfdb_add_batch_device: a BowVector has more words than max_words_per_kf");
  }
  for (int i = 0; i < n; i++) kfdb_commit(db, slots[i], kf_ids_host[i], db->next_pos + (uint32_t)i);
  db->next_pos += (uint32_t)n;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_erase(orbfe_kfdb* db, int64_t kf_id) {
  if (!db) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_erase: bad argument");
  auto it = db->slot_of.find(kf_id);
  if (it == db->slot_of.end()) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_kfdb_erase: keyframe id not stored");
  const int slot = it->second;
  if (db->device >= 0) {
    hipSetDevice(db->device);
    ORBFE_HIP_CHECK(hipMemsetAsync(db->st.n + slot, 0xff, 4, db->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(db->stream));
  }
  kfdb_release(db, slot);
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_clear(orbfe_kfdb* db) {
  if (!db) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_clear: bad argument");
  if (db->device >= 0) {
    hipSetDevice(db->device);
    ORBFE_HIP_CHECK(hipMemsetAsync(db->st.n, 0xff, 4 * (size_t)db->M, db->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(db->stream));
  }
  kfdb_reset_host(db);
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_size(const orbfe_kfdb* db, int* n) {
  if (!db || !n) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_size: bad argument");
  *n = (int)db->slot_of.size();
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_set_covisible(orbfe_kfdb* db, int64_t kf_id, const int64_t* ids, int n) {
  if (!db || n < 0 || n > KFDB_NEIGH || (n > 0 && !ids))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_set_covisible: bad argument (n in 0..10)");
  auto it = db->slot_of.find(kf_id);
  if (it == db->slot_of.end())
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_kfdb_set_covisible: keyframe id not stored");
  db->covis[it->second].assign(ids, ids + n);
  db->neigh_dirty = true;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_query(orbfe_kfdb* db, const orbfe_kfdb_query_t* q, orbfe_kfdb_result_t* r) {
  if (!db || !q || !r || (q->mode != ORBFE_KFDB_RELOC && q->mode != ORBFE_KFDB_LOOP) || q->n < 0 ||
      q->n > ORBFE_KFDB_MAX_WORDS || (q->n > 0 && (!q->words || !q->weights)) || q->n_excluded < 0 ||
      (q->n_excluded > 0 && !q->excluded) || r->capacity < 0 ||
      (r->capacity > 0 && (!r->kf_ids || !r->common_words || !r->scored || !r->scores || !r->candidates)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_query: bad argument");
  if (!q->on_device) {
    for (int i = 0; i < q->n; i++) {
      if (q->words[i] >= (uint32_t)db->n_words)
        return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_query: word id >= the vocabulary's n_words");
      if (i > 0 && q->words[i] <= q->words[i - 1])
        return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_kfdb_query: word ids must be strictly ascending");
    }
  }
  if (db->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "keyframe database is host-only (device < 0)");
  r->n_sharing = r->max_common = r->min_common = r->n_candidates = 0;
  const int hi = db->hi;
  if (hi == 0 || q->n == 0) return ORBFE_OK;  // nothing can share a word
  hipSetDevice(db->device);
  // staging: words | weights | excluded slots
  const size_t o_w = 0, o_v = orbfe_al256(4 * (size_t)ORBFE_KFDB_MAX_WORDS);
  const size_t o_x = o_v + orbfe_al256(8 * (size_t)ORBFE_KFDB_MAX_WORDS);
  int32_t* hx = reinterpret_cast<int32_t*>(db->h_stage + o_x);
  int n_excl = 0;
  if (q->mode == ORBFE_KFDB_LOOP) {
    for (int i = 0; i < q->n_excluded; i++) {
      auto it = db->slot_of.find(q->excluded[i]);
      if (it != db->slot_of.end() && n_excl < db->M) hx[n_excl++] = it->second;
    }
    std::sort(hx, hx + n_excl);
    n_excl = (int)(std::unique(hx, hx + n_excl) - hx);
  }
  if (q->on_device && q->stream) {
    ORBFE_HIP_CHECK(hipEventRecord(db->ev, (hipStream_t)q->stream));
    ORBFE_HIP_CHECK(hipStreamWaitEvent(db->stream, db->ev, 0));
  }
  if (!q->on_device) {
    memcpy(db->h_stage + o_w, q->words, 4 * (size_t)q->n);
    memcpy(db->h_stage + o_v, q->weights, 8 * (size_t)q->n);
    ORBFE_HIP_CHECK(hipMemcpyAsync(db->d_stage + o_w, db->h_stage + o_w, 4 * (size_t)q->n, hipMemcpyHostToDevice, db->stream));
    ORBFE_HIP_CHECK(hipMemcpyAsync(db->d_stage + o_v, db->h_stage + o_v, 8 * (size_t)q->n, hipMemcpyHostToDevice, db->stream));
  }
  if (n_excl > 0)
    ORBFE_HIP_CHECK(hipMemcpyAsync(db->d_stage + o_x, hx, 4 * (size_t)n_excl, hipMemcpyHostToDevice, db->stream));
  if (db->neigh_dirty) {  // neighbour ids -> slots, as of now
    db->neigh_host.assign((size_t)hi * KFDB_NEIGH, -1);
    for (int s = 0; s < hi; s++) {
      if (!db->live[s]) continue;
      int k = 0;
      for (int64_t id : db->covis[s]) {
        auto it = db->slot_of.find(id);
        if (it != db->slot_of.end()) db->neigh_host[(size_t)s * KFDB_NEIGH + k++] = it->second;
      }
    }
    ORBFE_HIP_CHECK(hipMemcpyAsync(db->d_neigh, db->neigh_host.data(), 4 * db->neigh_host.size(),
                                   hipMemcpyHostToDevice, db->stream));
    // neigh_host stays untouched until this call's synchronise
    db->neigh_dirty = false;
  }
  KfdbSweepArgs sa;
  sa.st = db->st;
  sa.hi = hi;
  sa.q_words = q->on_device ? q->words : reinterpret_cast<const uint32_t*>(db->d_stage + o_w);
  sa.q_weights = q->on_device ? q->weights : reinterpret_cast<const double*>(db->d_stage + o_v);
  sa.q_n_dev = q->on_device ? q->d_n : nullptr;
  sa.q_n = q->n;
  sa.excl = reinterpret_cast<const int32_t*>(db->d_stage + o_x);
  sa.n_excl = n_excl;
  sa.common = db->d_common;
  sa.first = db->d_first;
  sa.si = db->d_si;
  const int wpb = KFDB_SWEEP_THREADS / 64;
  const int grid = std::min((hi + wpb - 1) / wpb, 2048);
  ORBFE_LAUNCH("k_kfdb_sweep", k_kfdb_sweep, dim3(grid), dim3(KFDB_SWEEP_THREADS), 4 * (size_t)q->n, db->stream, sa);
  KfdbFinishArgs fa;
  fa.hi = hi;
  fa.mode = q->mode;
  fa.min_score = q->min_score;
  fa.common = db->d_common;
  fa.first = db->d_first;
  fa.si = db->d_si;
  fa.pos = db->st.pos;
  fa.slot_at_pos = db->st.slot_at_pos;
  fa.neigh = db->d_neigh;
  fa.reloc = db->st.reloc;
  fa.first_idx = db->d_first_idx;
  fa.acc = db->d_acc;
  fa.best = db->d_best;
  fa.hdr = db->d_res;
  fa.r_slot = db->d_res + 4;
  fa.r_common = fa.r_slot + hi;
  fa.r_scored = fa.r_common + hi;
  fa.r_score = reinterpret_cast<float*>(fa.r_scored + hi);
  fa.r_cand = fa.r_scored + 2 * (size_t)hi;
  int P2 = 64;
  while (P2 < hi) P2 <<= 1;
  ORBFE_LAUNCH("k_kfdb_finish", k_kfdb_finish, dim3(1), dim3(KFDB_FIN_THREADS), 8 * (size_t)P2, db->stream, fa);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(db->h_res, db->d_res, 4 * (4 + 5 * (size_t)hi), hipMemcpyDeviceToHost, db->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(db->stream));
  const int32_t* h = db->h_res;
  const int S = h[0], nc = h[3];
  if (S < 0 || S > hi || nc < 0 || nc > S) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_kfdb_query: corrupt result");
  if (S > r->capacity) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_kfdb_query: result capacity below the sharing list");
  r->n_sharing = S;
  r->max_common = h[1];
  r->min_common = h[2];
  r->n_candidates = nc;
  const int32_t* hs = h + 4;
  for (int i = 0; i < S; i++) {
    r->kf_ids[i] = db->id_of[hs[i]];
    r->common_words[i] = hs[hi + i];
    r->scored[i] = (uint8_t)hs[2 * (size_t)hi + i];
  }
  memcpy(r->scores, hs + 3 * (size_t)hi, 4 * (size_t)S);
  for (int i = 0; i < nc; i++) r->candidates[i] = db->id_of[hs[4 * (size_t)hi + i]];
  return ORBFE_OK;
}
