// covis_core_test.cpp -- the covisibility table's host bookkeeping (orb_slam2_2021_amd/csrc/orbfe_covis_core.h)
// exercised alone: the id table, row reuse, tie-key and mnId ranks, stale tracking, every argument and capacity
// check. No library, no GPU; built with ASan + UBSan by tests/test_covis_core.py.
//
// With `--bench KF SLOTS OBSERVERS BATCH REPEATS` it instead times KeyFrame::UpdateConnections' counting and
// ordering (src/KeyFrame.cc:304-378) restated with the reference's own containers (std::map<KeyFrame*, int>, one
// std::map<KeyFrame*, size_t> of observations per map point) over a synthetic map of that shape: the host figure
// DESIGN.md §24 sets beside the device's. Build that one without the sanitizers.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <random>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_covis_core.h"

namespace cc = orbfe_covis_core;

static int g_fail = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      g_fail++;                                                         \
    }                                                                   \
  } while (0)

static int set_keyframe(cc::Core& c, int64_t id, uint64_t key, const std::vector<int32_t>& pts) {
  int row = -1, top = 0;
  cc::Status st = c.prepare_keyframe(id, key, (int)pts.size(), pts.data(), &row, &top);
  if (st) return st.code;
  c.commit_keyframe(row, id, key, (int)pts.size(), top);
  return cc::OK;
}

static void test_core() {
  CHECK(cc::Core::check_create(0, 1, 1).code == cc::ERR_ARG);
  CHECK(cc::Core::check_create(4097, 1, 1).code == cc::ERR_ARG);
  CHECK(cc::Core::check_create(1, 8193, 1).code == cc::ERR_ARG);
  CHECK(cc::Core::check_create(1, 1, (1 << 24) + 1).code == cc::ERR_ARG);
  CHECK(cc::Core::check_create(4096, 8192, 1 << 24).code == cc::OK);

  cc::Core c;
  c.init(4, 8, 100);
  CHECK(c.size() == 0 && c.stale && c.ranks_dirty);
  // ids out of order, tie keys reversing them
  CHECK(set_keyframe(c, 30, 5, {1, 2, -1, 99}) == cc::OK);
  CHECK(set_keyframe(c, 10, 9, {2}) == cc::OK);
  CHECK(set_keyframe(c, 20, 7, {}) == cc::OK);
  CHECK(c.size() == 3 && c.hi == 3 && c.total_slots == 5 && c.p_hi == 100);
  c.ranks();
  CHECK(!c.ranks_dirty);
  CHECK(c.row_at_id_rank == (std::vector<int32_t>{1, 2, 0}));   // 10, 20, 30
  CHECK(c.row_at_tie_rank == (std::vector<int32_t>{0, 2, 1}));  // keys 5, 7, 9
  CHECK(c.tie_rank_of_id_rank == (std::vector<uint16_t>{2, 1, 0}));
  CHECK(c.id_rank_of_row == (std::vector<int32_t>{2, 0, 1}));
  // argument and capacity checks touch nothing
  const int64_t slots_before = c.total_slots;
  c.stale = false;
  CHECK(set_keyframe(c, 40, 5, {1}) == cc::ERR_ARG);            // duplicate tie key
  CHECK(set_keyframe(c, 10, 5, {1}) == cc::ERR_ARG);            // ... also when replacing
  CHECK(set_keyframe(c, 40, 1, {100}) == cc::ERR_CAPACITY);     // id at max_point_id
  CHECK(set_keyframe(c, 40, 1, {-2}) == cc::ERR_ARG);
  CHECK(set_keyframe(c, 40, 1, std::vector<int32_t>(9, 1)) == cc::ERR_CAPACITY);  // more than max_slots
  CHECK(c.size() == 3 && c.total_slots == slots_before && !c.stale && !c.ranks_dirty);
  CHECK(set_keyframe(c, 40, 1, {3}) == cc::OK);
  CHECK(c.stale && c.ranks_dirty);
  CHECK(set_keyframe(c, 50, 2, {3}) == cc::ERR_CAPACITY);       // the table is full
  // replacing a row: same key keeps the ranks, another key dirties them
  c.ranks();
  c.stale = false;
  CHECK(set_keyframe(c, 10, 9, {4, 5, 6}) == cc::OK);
  CHECK(c.stale && !c.ranks_dirty && c.total_slots == slots_before + 1 + 2);
  CHECK(set_keyframe(c, 10, 8, {4, 5, 6}) == cc::OK);
  CHECK(c.ranks_dirty && c.slot_of_key.count(9) == 0 && c.slot_of_key.count(8) == 1);
  // set_slots
  int row = -1, top = 0;
  std::vector<int32_t> os, oi;
  const int32_t s1[] = {0, 2, 0}, p1[] = {7, 8, 9};
  CHECK(c.prepare_slots(10, 3, s1, p1, &row, &os, &oi, &top).code == cc::OK);
  CHECK(os == (std::vector<int32_t>{0, 2}) && oi == (std::vector<int32_t>{9, 8}) && top == 10);  // last id wins
  const int32_t s2[] = {3};
  CHECK(c.prepare_slots(10, 1, s2, p1, &row, &os, &oi, &top).code == cc::ERR_ARG);     // outside the row
  CHECK(c.prepare_slots(77, 1, s1, p1, &row, &os, &oi, &top).code == cc::ERR_STATE);   // not stored
  const int32_t p2[] = {100};
  CHECK(c.prepare_slots(10, 1, s1, p2, &row, &os, &oi, &top).code == cc::ERR_CAPACITY);
  c.stale = false;
  c.commit_slots(0, 0);
  CHECK(!c.stale);
  c.commit_slots(2, 10);
  CHECK(c.stale);
  // erase and re-add: the freed row is reused, lowest first
  CHECK(c.erase(77, &row).code == cc::ERR_STATE);
  CHECK(c.erase(30, &row).code == cc::OK && row == 0);
  CHECK(c.erase(20, &row).code == cc::OK && row == 2);
  CHECK(c.size() == 2 && c.row_n[0] == -1 && c.slot_of_key.count(5) == 0);
  CHECK(set_keyframe(c, 5, 5, {1, 1}) == cc::OK);
  CHECK(c.slot_of[5] == 0 && c.hi == 4);
  c.ranks();
  CHECK(c.row_at_id_rank == (std::vector<int32_t>{0, 1, 3}));   // 5, 10, 40
  CHECK(c.row_at_tie_rank == (std::vector<int32_t>{3, 0, 1}));  // keys 1, 5, 8
  CHECK(c.id_rank_of_row[2] == -1);
  // query lists
  std::vector<int32_t> rows;
  const int64_t q1[] = {10, 10, 5}, q2[] = {10, 20};
  CHECK(c.rows_of(3, q1, &rows).code == cc::OK && rows == (std::vector<int32_t>{1, 1, 0}));
  CHECK(c.rows_of(2, q2, &rows).code == cc::ERR_ARG);
  CHECK(c.local_rows(3, q1, &rows).code == cc::ERR_ARG);        // named twice
  CHECK(c.local_rows(1, q1, &rows).code == cc::OK);
  const int32_t b1[] = {0, 2, 2, 3}, v1[] = {5, -1, 99};
  CHECK(c.check_votes(3, b1, v1).code == cc::OK);
  const int32_t b2[] = {1, 2}, b3[] = {0, 2, 1}, v2[] = {5, 100, 3};
  CHECK(c.check_votes(1, b2, v1).code == cc::ERR_ARG);
  CHECK(c.check_votes(2, b3, v1).code == cc::ERR_ARG);
  CHECK(c.check_votes(3, b1, v2).code == cc::ERR_CAPACITY);
  const int32_t b4[] = {0, cc::kMaxSlots + 1};
  CHECK(c.check_votes(1, b4, nullptr).code == cc::ERR_CAPACITY);
  CHECK(cc::key_weight((8192u << 12) | 4095u) == 8192 && cc::key_rank((8192u << 12) | 4095u) == 4095);
  c.clear();
  CHECK(c.size() == 0 && c.hi == 0 && c.p_hi == 0 && c.stale && c.ranks_dirty);
  CHECK(set_keyframe(c, 1, 1, {0}) == cc::OK && c.slot_of[1] == 0);
}

// ---- the reference's containers, for the host figure ------------------------------------------------
struct KeyFrame;
struct MapPoint {
  std::map<KeyFrame*, size_t> mObservations;
  bool bad = false;
};
struct KeyFrame {
  long mnId = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  std::vector<int> mvOrderedWeights;
};

// KeyFrame.cc:304-385 without AddConnection's re-sort of the other keyframes (the device call returns the
// counts and the order; that side effect is host work on either path)
static size_t update_connections(KeyFrame* kf, int th) {
  std::map<KeyFrame*, int> KFcounter;
  std::vector<MapPoint*> vpMP = kf->mvpMapPoints;
  for (MapPoint* pMP : vpMP) {
    if (!pMP) continue;
    if (pMP->bad) continue;
    std::map<KeyFrame*, size_t> observations = pMP->mObservations;
    for (auto& o : observations) {
      if (o.first->mnId == kf->mnId) continue;
      KFcounter[o.first]++;
    }
  }
  if (KFcounter.empty()) return 0;
  int nmax = 0;
  KeyFrame* pKFmax = nullptr;
  std::vector<std::pair<int, KeyFrame*>> vPairs;
  vPairs.reserve(KFcounter.size());
  for (auto& m : KFcounter) {
    if (m.second > nmax) {
      nmax = m.second;
      pKFmax = m.first;
    }
    if (m.second >= th) vPairs.push_back({m.second, m.first});
  }
  if (vPairs.empty()) vPairs.push_back({nmax, pKFmax});
  std::sort(vPairs.begin(), vPairs.end());
  std::list<KeyFrame*> lKFs;
  std::list<int> lWs;
  for (auto& p : vPairs) {
    lKFs.push_front(p.second);
    lWs.push_front(p.first);
  }
  kf->mConnectedKeyFrameWeights = KFcounter;
  kf->mvpOrderedConnectedKeyFrames.assign(lKFs.begin(), lKFs.end());
  kf->mvOrderedWeights.assign(lWs.begin(), lWs.end());
  return KFcounter.size();
}

static int bench(int n_kf, int n_slots, int observers, int batch, int repeats) {
  // a track: keyframe t draws its points from a window that slides with t, so that a point is seen by about
  // `observers` keyframes (the same generator as profiles/covis.py)
  std::mt19937 rng(1);
  // a window holds a given id with probability ~0.39 (n_slots draws from 2 * n_slots ids)
  const int window = n_slots * 2, step = std::max((int)(window * 0.39 / std::max(observers, 1)), 1);
  std::vector<MapPoint> points((size_t)n_kf * step + window);
  std::vector<KeyFrame> kfs(n_kf);
  for (int t = 0; t < n_kf; t++) {
    kfs[t].mnId = t;
    kfs[t].mvpMapPoints.resize(n_slots);
    for (int s = 0; s < n_slots; s++) {
      MapPoint* p = &points[(size_t)t * step + rng() % window];
      kfs[t].mvpMapPoints[s] = p;
      p->mObservations.insert({&kfs[t], (size_t)s});
    }
  }
  size_t n_obs = 0, n_pts = 0;
  for (auto& p : points)
    if (!p.mObservations.empty()) {
      n_obs += p.mObservations.size();
      n_pts++;
    }
  std::vector<double> ms;
  size_t conn = 0;
  for (int r = 0; r < repeats + 2; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int q = 0; q < batch; q++) conn += update_connections(&kfs[(size_t)q * n_kf / batch], 15);
    const auto t1 = std::chrono::steady_clock::now();
    if (r >= 2) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());  // two warm-up rounds
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"host_update_connections_ms\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f, \"repeats\": %d}, "
              "\"keyframes\": %d, \"slots\": %d, \"batch\": %d, \"observers_per_point\": %.2f, \"connections\": %zu}\n",
              ms[ms.size() / 2], ms.front(), ms.back(), repeats, n_kf, n_slots, batch, (double)n_obs / (double)n_pts,
              conn / (size_t)(repeats + 2) / (size_t)batch);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !std::strcmp(argv[1], "--bench"))
    return bench(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
  test_core();
  if (g_fail) return 1;
  std::printf("OK covisibility core\n");
  return 0;
}
