// orbfe_localmap_core.h -- the host side of include/orbfe_localmap.h: argument and capacity checks, the
// index arithmetic the kernels of orbfe_covis.hip share with the host (the first-occurrence key, the
// tagged output index, the block numbering of the order-preserving compaction, the 64-byte store record),
// and the serial composition of that scheme on the host (lm_host_distinct). Plain C++ unless compiled by
// hipcc: orbfe_covis.hip includes it, and tests/cpp/localmap_core_test.cpp exercises it alone.
// tests/local_map_ref.py reaches the same lists a second way, with the reference's stamps and push_backs.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "orbfe_covis_core.h"

#if defined(__HIPCC__)
#define LM_HD __host__ __device__
#else
#define LM_HD
#endif

namespace orbfe_localmap_core {

namespace cc = orbfe_covis_core;

constexpr int kMaxList = 4096;   // keyframe list entries: 12 bits of a key
constexpr int kMaxSeen = 8192;   // as a vote list
constexpr int kBlock = 256;      // slots per workgroup of the three row passes
constexpr int kSetChunk = 65536; // points per staging pass of set_point_geometry
constexpr int kRecord = 64;      // bytes per stored point: descriptor 32 | pos 12 | normal 12 | min 4 | max 4

// flag bits (include/orbfe.h, orbfe_frustum.h) the store refuses; LM_PRESENT takes ORBFE_MPF_BAD's place in
// the state byte (bad points never reach a result, so the bit is free there) and is masked off on the way out
constexpr uint8_t kRefusedFlags = 1u | 2u | 32u;  // TRACK_IN_VIEW | BAD | SEEN
constexpr uint8_t kPresent = 2u;

// first[p] between calls. A key is position << 13 | slot < 2^25; an output index is tagged with bit 31 so
// that it equals no key (the thread that reads first[p] == its own key is the first occurrence, whatever
// the winner has written back meanwhile) and, being below 2^31 - 1, never the all-ones value either.
constexpr uint32_t kNone = 0xffffffffu;
LM_HD inline uint32_t lm_key(int pos, int slot) { return ((uint32_t)pos << 13) | (uint32_t)slot; }
LM_HD inline uint32_t lm_tag(int idx) { return 0x80000000u | (uint32_t)idx; }
LM_HD inline bool lm_is_index(uint32_t v) { return v != kNone && (v >> 31) != 0; }
LM_HD inline int lm_index(uint32_t v) { return (int)(v & 0x7fffffffu); }
// workgroup (bx, position) of a grid (nbx, n_kf): ascending in (position, slot)
LM_HD inline int lm_block(int pos, int bx, int nbx) { return pos * nbx + bx; }

// What one call launches, from the stored lengths of the named rows.
struct Plan {
  int max_row = 0;        // the longest named row
  int nbx = 0;            // 256-slot blocks per list position
  int n_blocks = 0;       // nbx * n_kf <= 4096 * 32
  int64_t named_slots = 0;  // sum of the named rows' lengths, repeats included: <= 2^25
  int bound = 0;          // on the result: min(named_slots, max_point_id)
};

// kf list -> rows (repeats allowed) and the plan
inline cc::Status check_list(const cc::Core& c, int n_kf, const int64_t* kf_ids, std::vector<int32_t>* rows, Plan* plan) {
  if (n_kf < 1 || !kf_ids) return {cc::ERR_ARG, "a keyframe list holds 1 to 4096 entries"};
  if (n_kf > kMaxList) return {cc::ERR_CAPACITY, "a keyframe list of more than 4096 entries"};
  cc::Status st = c.rows_of(n_kf, kf_ids, rows);
  if (st) return st;
  Plan p;
  for (int i = 0; i < n_kf; i++) {
    const int len = std::min(std::max(c.row_n[(*rows)[i]], 0), c.S);
    p.max_row = std::max(p.max_row, len);
    p.named_slots += len;
  }
  p.nbx = (p.max_row + kBlock - 1) / kBlock;
  p.n_blocks = p.nbx * n_kf;
  p.bound = (int)std::min<int64_t>(p.named_slots, c.P);
  *plan = p;
  return cc::ok();
}

// the Frame's mvpMapPoints as a seen list: -1 or 0..P-1, at most 8192 entries
inline cc::Status check_seen(const cc::Core& c, int n_seen, const int32_t* ids) {
  if (n_seen < 0 || (n_seen > 0 && !ids)) return {cc::ERR_ARG, "bad argument"};
  if (n_seen > kMaxSeen) return {cc::ERR_CAPACITY, "a seen list of more than 8192 entries"};
  int top = 0;
  return c.check_points(n_seen, ids, &top);
}

inline cc::Status check_geometry(const cc::Core& c, int n, const int32_t* ids, const uint8_t* flags, const float* pos,
                                 const float* normal, const float* min_d, const float* max_d, const uint8_t* desc) {
  if (n < 0 || (n > 0 && (!ids || !flags || !pos || !normal || !min_d || !max_d || !desc)))
    return {cc::ERR_ARG, "bad argument"};
  for (int i = 0; i < n; i++) {
    if (ids[i] < 0 || ids[i] >= c.P) return {cc::ERR_ARG, "a point id outside 0 .. max_point_id - 1"};
    if (flags[i] & kRefusedFlags) return {cc::ERR_ARG, "flags must not carry BAD, SEEN or TRACK_IN_VIEW"};
  }
  std::vector<int32_t> s(ids, ids + n);
  std::sort(s.begin(), s.end());
  if (std::adjacent_find(s.begin(), s.end()) != s.end()) return {cc::ERR_ARG, "a point named twice"};
  return cc::ok();
}

// point i of the caller's arrays -> its 64-byte record
inline void pack_record(uint8_t* dst, int i, const float* pos, const float* normal, const float* min_d,
                        const float* max_d, const uint8_t* desc) {
  memcpy(dst, desc + 32 * (size_t)i, 32);
  memcpy(dst + 32, pos + 3 * (size_t)i, 12);
  memcpy(dst + 44, normal + 3 * (size_t)i, 12);
  memcpy(dst + 56, min_d + i, 4);
  memcpy(dst + 60, max_d + i, 4);
}

// ---- the serial composition on the host ------------------------------------------------------
// The device scheme step by step over host arrays: the minimum per point, the winners per block, the
// exclusive scan of the block counts, the emit with the index written back, the reset over the result.
// rows[i]: the row of list position i (point id per slot, -1: none); bad[P]; first[P]: all kNone on entry
// and on return. seen (may be empty) marks like k_lm_seen: seen_out[idx] = 1. Returns false when an
// argument is outside what the checks above admit.
inline bool lm_host_distinct(const std::vector<std::vector<int32_t>>& rows, const std::vector<uint8_t>& bad,
                             std::vector<uint32_t>* first, const std::vector<int32_t>& seen,
                             std::vector<int32_t>* out, std::vector<uint8_t>* seen_out) {
  const int n_kf = (int)rows.size(), P = (int)bad.size();
  if (n_kf < 1 || n_kf > kMaxList || (int)first->size() != P || (int)seen.size() > kMaxSeen) return false;
  int max_row = 0;
  for (const auto& r : rows) {
    if ((int)r.size() > cc::kMaxSlots) return false;
    max_row = std::max(max_row, (int)r.size());
    for (int p : r)
      if (p < -1 || p >= P) return false;
  }
  const int nbx = (max_row + kBlock - 1) / kBlock;
  auto live = [&](int pos, int s, int* p) {
    if (s >= (int)rows[pos].size()) return false;
    *p = rows[pos][s];
    return (unsigned)*p < (unsigned)P && !bad[*p];
  };
  int p;
  for (int pos = 0; pos < n_kf; pos++)  // k_lm_first
    for (int s = 0; s < nbx * kBlock; s++)
      if (live(pos, s, &p)) (*first)[p] = std::min((*first)[p], lm_key(pos, s));
  std::vector<int32_t> blk((size_t)nbx * n_kf + 1, 0);
  for (int pos = 0; pos < n_kf; pos++)  // k_lm_count
    for (int s = 0; s < nbx * kBlock; s++)
      if (live(pos, s, &p) && (*first)[p] == lm_key(pos, s)) blk[lm_block(pos, s / kBlock, nbx)]++;
  int run = 0;  // the scan
  for (size_t b = 0; b < blk.size(); b++) {
    const int x = blk[b];
    blk[b] = run;
    run += x;
  }
  const int n_points = run;
  out->assign(n_points, -1);
  for (int pos = 0; pos < n_kf; pos++)  // k_lm_emit
    for (int bx = 0; bx < nbx; bx++) {
      int rank = 0;
      for (int t = 0; t < kBlock; t++) {
        const int s = bx * kBlock + t;
        if (!live(pos, s, &p) || (*first)[p] != lm_key(pos, s)) continue;
        const int idx = blk[lm_block(pos, bx, nbx)] + rank++;
        if (idx >= n_points) return false;
        (*out)[idx] = p;
        (*first)[p] = lm_tag(idx);
      }
    }
  seen_out->assign(n_points, 0);
  for (int q : seen) {  // k_lm_seen
    if ((unsigned)q >= (unsigned)P) continue;
    const uint32_t v = (*first)[q];
    if (lm_is_index(v) && lm_index(v) < n_points) (*seen_out)[lm_index(v)] = 1;
  }
  for (int i = 0; i < n_points; i++) {  // k_lm_reset
    if ((unsigned)(*out)[i] >= (unsigned)P) return false;
    (*first)[(*out)[i]] = kNone;
  }
  return true;
}

}  // namespace orbfe_localmap_core
