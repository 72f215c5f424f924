// orbfe_covis_core.h -- host bookkeeping of the covisibility table (include/orbfe_covis.h): the id
// table, the tie-key and mnId ranks, stale tracking, argument and capacity checks. Plain C++, no
// HIP: orbfe_covis.hip includes it, and tests/cpp/covis_core_test.cpp exercises it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <map>
#include <queue>
#include <unordered_map>
#include <vector>

namespace orbfe_covis_core {

// the values of ORBFE_OK / ORBFE_ERR_* (include/orbfe.h)
enum { OK = 0, ERR_ARG = -1, ERR_CAPACITY = -2, ERR_HIP = -3, ERR_STATE = -4 };

constexpr int kMaxKeyframes = 4096;
constexpr int kMaxSlots = 8192;
constexpr int kMaxPointId = 1 << 24;

struct Status {
  int code;
  const char* msg;
  explicit operator bool() const { return code != OK; }
};
inline Status ok() { return {OK, ""}; }

struct Core {
  int M = 0, S = 0, P = 0;  // max_keyframes, max_slots, max_point_id
  std::unordered_map<int64_t, int> slot_of;  // mnId -> row
  std::map<uint64_t, int> slot_of_key;       // tie key -> row, ascending
  std::vector<int64_t> id_of;                // [M], valid where live
  std::vector<uint64_t> key_of;              // [M]
  std::vector<uint8_t> live;                 // [M]
  std::vector<int32_t> row_n;                // [M] slots of the row
  std::vector<uint8_t> has_attr;             // [M] the row's per-slot attributes are stored
  int n_attr = 0;                            // live rows with attributes
  std::priority_queue<int, std::vector<int>, std::greater<int>> free_rows;  // below hi
  int hi = 0;               // rows ever used
  int64_t total_slots = 0;  // sum of row_n over live rows: bounds the inverse's entries
  int p_hi = 0;             // 1 + the largest point id ever written: bounds every per-point pass
  bool stale = true;        // the inverse does not describe the rows
  bool ranks_dirty = true;  // the keyframe set or a tie key changed since ranks() last ran
  // ranks(): r is a rank by mnId, t a rank by tie key, both 0..n_live-1
  std::vector<int32_t> id_rank_of_row;          // [hi]
  std::vector<int32_t> row_at_id_rank;          // [n_live]
  std::vector<uint16_t> tie_rank_of_id_rank;    // [n_live]
  std::vector<int32_t> row_at_tie_rank;         // [n_live]
  std::vector<int32_t> tie_rank_of_row;         // [hi]

  static Status check_create(int max_keyframes, int max_slots, int max_point_id) {
    if (max_keyframes < 1 || max_keyframes > kMaxKeyframes || max_slots < 1 || max_slots > kMaxSlots ||
        max_point_id < 1 || max_point_id > kMaxPointId)
      return {ERR_ARG, "max_keyframes in 1..4096, max_slots in 1..8192, max_point_id in 1..2^24"};
    return ok();
  }

  void init(int max_keyframes, int max_slots, int max_point_id) {
    M = max_keyframes;
    S = max_slots;
    P = max_point_id;
    clear();
  }

  void clear() {
    slot_of.clear();
    slot_of_key.clear();
    id_of.assign(M, 0);
    key_of.assign(M, 0);
    live.assign(M, 0);
    row_n.assign(M, -1);
    has_attr.assign(M, 0);
    n_attr = 0;
    free_rows = {};
    hi = 0;
    total_slots = 0;
    p_hi = 0;
    stale = true;
    ranks_dirty = true;
  }

  int size() const { return (int)slot_of.size(); }

  // -1 or 0..P-1; returns 1 + the largest id through *top
  Status check_points(int n, const int32_t* ids, int* top) const {
    int t = 0;
    for (int i = 0; i < n; i++) {
      if (ids[i] < -1) return {ERR_ARG, "a point id below -1"};
      if (ids[i] >= P) return {ERR_CAPACITY, "a point id at or above max_point_id"};
      t = std::max(t, ids[i] + 1);
    }
    *top = t;
    return ok();
  }

  // Checks of set_keyframe; on success *row is the row to write (a new one is not yet committed).
  Status prepare_keyframe(int64_t kf_id, uint64_t tie_key, int n_slots, const int32_t* ids, int* row,
                          int* top) const {
    if (n_slots < 0 || (n_slots > 0 && !ids)) return {ERR_ARG, "bad argument"};
    if (n_slots > S) return {ERR_CAPACITY, "more slots than max_slots"};
    Status st = check_points(n_slots, ids, top);
    if (st) return st;
    auto it = slot_of.find(kf_id);
    auto kt = slot_of_key.find(tie_key);
    if (kt != slot_of_key.end() && (it == slot_of.end() || kt->second != it->second))
      return {ERR_ARG, "the tie key belongs to another keyframe"};
    if (it == slot_of.end() && size() >= M) return {ERR_CAPACITY, "the table is full"};
    *row = it != slot_of.end() ? it->second : (free_rows.empty() ? hi : free_rows.top());
    return ok();
  }

  void commit_keyframe(int row, int64_t kf_id, uint64_t tie_key, int n_slots, int top) {
    if (!live[row]) {
      if (row == hi) {
        hi++;
      } else {
        free_rows.pop();  // prepare_keyframe chose the top
      }
      live[row] = 1;
      id_of[row] = kf_id;
      slot_of[kf_id] = row;
      key_of[row] = tie_key;
      slot_of_key[tie_key] = row;
      ranks_dirty = true;
    } else {
      total_slots -= row_n[row];
      if (row_n[row] != n_slots) drop_attrs(row);  // other keypoints
      if (key_of[row] != tie_key) {
        slot_of_key.erase(key_of[row]);
        key_of[row] = tie_key;
        slot_of_key[tie_key] = row;
        ranks_dirty = true;
      }
    }
    row_n[row] = n_slots;
    total_slots += n_slots;
    p_hi = std::max(p_hi, top);
    stale = true;
  }

  // Checks of set_slots; writes the (slot, id) pairs to apply, a slot named twice keeping its last id.
  Status prepare_slots(int64_t kf_id, int n, const int32_t* slots, const int32_t* ids, int* row,
                       std::vector<int32_t>* out_slots, std::vector<int32_t>* out_ids, int* top) const {
    if (n < 0 || (n > 0 && (!slots || !ids))) return {ERR_ARG, "bad argument"};
    auto it = slot_of.find(kf_id);
    if (it == slot_of.end()) return {ERR_STATE, "keyframe id not stored"};
    *row = it->second;
    for (int i = 0; i < n; i++)
      if (slots[i] < 0 || slots[i] >= row_n[*row]) return {ERR_ARG, "a slot outside the keyframe's row"};
    Status st = check_points(n, ids, top);
    if (st) return st;
    out_slots->clear();
    out_ids->clear();
    std::unordered_map<int32_t, int> at;
    for (int i = 0; i < n; i++) {
      auto f = at.find(slots[i]);
      if (f == at.end()) {
        at[slots[i]] = (int)out_slots->size();
        out_slots->push_back(slots[i]);
        out_ids->push_back(ids[i]);
      } else {
        (*out_ids)[f->second] = ids[i];
      }
    }
    return ok();
  }

  void commit_slots(int n, int top) {
    if (n > 0) stale = true;
    p_hi = std::max(p_hi, top);
  }

  Status erase(int64_t kf_id, int* row) {
    auto it = slot_of.find(kf_id);
    if (it == slot_of.end()) return {ERR_STATE, "keyframe id not stored"};
    const int r = it->second;
    *row = r;
    slot_of.erase(it);
    slot_of_key.erase(key_of[r]);
    live[r] = 0;
    drop_attrs(r);
    total_slots -= row_n[r];
    row_n[r] = -1;
    free_rows.push(r);
    stale = true;
    ranks_dirty = true;
    return ok();
  }

  void drop_attrs(int row) {
    if (has_attr[row]) n_attr--;
    has_attr[row] = 0;
  }

  // Checks of set_keyframe_attrs
  Status prepare_attrs(int64_t kf_id, int n_slots, const uint8_t* attrs, int* row) const {
    if (n_slots < 0 || (n_slots > 0 && !attrs)) return {ERR_ARG, "bad argument"};
    auto it = slot_of.find(kf_id);
    if (it == slot_of.end()) return {ERR_STATE, "keyframe id not stored"};
    if (n_slots != row_n[it->second]) return {ERR_ARG, "n_slots differs from the stored row's length"};
    for (int i = 0; i < n_slots; i++)
      if (attrs[i] & 0x80) return {ERR_ARG, "bit 7 of an attribute byte is set"};
    *row = it->second;
    return ok();
  }

  void commit_attrs(int row) {
    if (!has_attr[row]) n_attr++;
    has_attr[row] = 1;
  }

  bool all_have_attrs() const { return n_attr == size(); }

  // Checks of cull_keyframes: the candidates' rows, and the bound on the bad list.
  Status prepare_cull(int n, const int64_t* kf_ids, const uint8_t* not_erase, int bad_capacity,
                      std::vector<int32_t>* rows) const {
    if (n > 0 && !not_erase) return {ERR_ARG, "bad argument"};
    Status st = local_rows(n, kf_ids, rows);
    if (st) return st;
    if (!all_have_attrs()) return {ERR_STATE, "a stored keyframe has no attributes"};
    int64_t need = 0;
    for (int i = 0; i < n; i++) need += row_n[(*rows)[i]];
    if (bad_capacity < need) return {ERR_CAPACITY, "bad_capacity below the sum of the candidates' row lengths"};
    return ok();
  }

  // Checks of cull_points
  Status prepare_cull_points(int n, const int32_t* ids, const int32_t* found, const int32_t* visible,
                             const int64_t* first_kf_id, int64_t current_kf_id, const uint8_t* action) const {
    if (n < 0 || (n > 0 && (!ids || !found || !visible || !first_kf_id || !action))) return {ERR_ARG, "bad argument"};
    const int64_t lim = (int64_t)1 << 31;
    if (current_kf_id < 0 || current_kf_id >= lim) return {ERR_ARG, "a keyframe id outside 0 .. 2^31 - 1"};
    std::vector<int32_t> s(ids, ids + n);
    for (int i = 0; i < n; i++) {
      if (ids[i] < 0 || ids[i] >= P) return {ERR_ARG, "a point id outside 0 .. max_point_id - 1"};
      if (first_kf_id[i] < 0 || first_kf_id[i] >= lim) return {ERR_ARG, "a keyframe id outside 0 .. 2^31 - 1"};
    }
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return {ERR_ARG, "a point named twice"};
    if (!all_have_attrs()) return {ERR_STATE, "a stored keyframe has no attributes"};
    return ok();
  }

  // The rank tables as of now.
  void ranks() {
    const int n = size();
    id_rank_of_row.assign(hi, -1);
    tie_rank_of_row.assign(hi, -1);
    row_at_id_rank.resize(n);
    row_at_tie_rank.resize(n);
    tie_rank_of_id_rank.resize(n);
    std::vector<std::pair<int64_t, int>> by_id;
    by_id.reserve(n);
    for (const auto& kv : slot_of) by_id.push_back({kv.first, kv.second});
    std::sort(by_id.begin(), by_id.end());
    for (int r = 0; r < n; r++) {
      row_at_id_rank[r] = by_id[r].second;
      id_rank_of_row[by_id[r].second] = r;
    }
    int t = 0;
    for (const auto& kv : slot_of_key) {
      row_at_tie_rank[t] = kv.second;
      tie_rank_of_row[kv.second] = t;
      t++;
    }
    for (int r = 0; r < n; r++) tie_rank_of_id_rank[r] = (uint16_t)tie_rank_of_row[row_at_id_rank[r]];
    ranks_dirty = false;
  }

  // ids of a query batch -> rows (duplicates allowed)
  Status rows_of(int n, const int64_t* kf_ids, std::vector<int32_t>* rows) const {
    if (n < 0 || (n > 0 && !kf_ids)) return {ERR_ARG, "bad argument"};
    rows->resize(n);
    for (int i = 0; i < n; i++) {
      auto it = slot_of.find(kf_ids[i]);
      if (it == slot_of.end()) return {ERR_ARG, "a keyframe id that is not stored"};
      (*rows)[i] = it->second;
    }
    return ok();
  }

  // lLocalKeyFrames -> rows: each stored, each once
  Status local_rows(int n, const int64_t* kf_ids, std::vector<int32_t>* rows) const {
    Status st = rows_of(n, kf_ids, rows);
    if (st) return st;
    std::vector<int32_t> s(*rows);
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return {ERR_ARG, "a local keyframe id named twice"};
    return ok();
  }

  // CSR of vote lists
  Status check_votes(int n_queries, const int32_t* begin, const int32_t* point_ids) const {
    if (n_queries < 0 || (n_queries > 0 && !begin)) return {ERR_ARG, "bad argument"};
    if (n_queries == 0) return ok();
    if (begin[0] != 0) return {ERR_ARG, "begin[0] must be 0"};
    for (int q = 0; q < n_queries; q++) {
      if (begin[q + 1] < begin[q]) return {ERR_ARG, "begin must not descend"};
      if (begin[q + 1] - begin[q] > kMaxSlots) return {ERR_CAPACITY, "a vote list of more than 8192 entries"};
    }
    if (begin[n_queries] > 0 && !point_ids) return {ERR_ARG, "bad argument"};
    int top = 0;
    return check_points(begin[n_queries], point_ids, &top);
  }
};

// One query's packed device result -> the caller's arrays. An entry is weight << 12 | tie rank.
inline int key_weight(uint32_t key) { return (int)(key >> 12); }
inline int key_rank(uint32_t key) { return (int)(key & 4095u); }

}  // namespace orbfe_covis_core
