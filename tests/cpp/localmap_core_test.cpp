// localmap_core_test -- orb_slam2_2021_amd/csrc/orbfe_localmap_core.h alone on the host, serially, built with
// ASan + UBSan by tests/test_localmap_core.py. Reads a case file the restatement (tests/local_map_ref.py) wrote and
// prints one line per case:
//   D n_points n_kf n_bad n_seen, then per list position `len id*len`, the bad ids, the seen ids
//       -> lm_host_distinct (the device scheme step by step): `n id*n | seen flags`, and the scratch must be all
//          ones again afterwards
//   C max_kf max_slots max_point_id n_stored (id len)*n_stored n_list id*n_list
//       -> check_list on a table of rows of those lengths: `status max_row nbx n_blocks named_slots bound`
//   G max_point_id n (id flag)*n  -> check_geometry: status
//   S max_point_id n id*n         -> check_seen: status
// A case the readers refuse: exit status 2.
// --bench n_kf slots observers repeats: Tracking::UpdateLocalPoints through the reference's containers
// (vector<MapPoint*> rows, the mnTrackReferenceForFrame stamp, push_back) on one core, as JSON.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_localmap_core.h"

namespace lm = orbfe_localmap_core;
namespace cc = orbfe_covis_core;

static int refuse(const char* why) {
  fprintf(stderr, "localmap_core_test: %s\n", why);
  return 2;
}

static int run_cases(const char* path) {
  std::ifstream in(path);
  if (!in) return refuse("cannot open the case file");
  std::string kind;
  while (in >> kind) {
    if (kind == "D") {
      int n_points, n_kf, n_bad, n_seen;
      if (!(in >> n_points >> n_kf >> n_bad >> n_seen)) return refuse("short D header");
      if (n_points < 1 || n_points > (1 << 24) || n_kf < 1 || n_kf > 4096 || n_bad < 0 || n_seen < 0 || n_seen > 8192)
        return refuse("D header out of range");
      std::vector<std::vector<int32_t>> rows(n_kf);
      for (int k = 0; k < n_kf; k++) {
        int len;
        if (!(in >> len) || len < 0 || len > 8192) return refuse("bad row length");
        rows[k].resize(len);
        for (int s = 0; s < len; s++)
          if (!(in >> rows[k][s]) || rows[k][s] < -1 || rows[k][s] >= n_points) return refuse("bad slot");
      }
      std::vector<uint8_t> bad(n_points, 0);
      for (int i = 0; i < n_bad; i++) {
        int p;
        if (!(in >> p) || p < 0 || p >= n_points) return refuse("bad point id");
        bad[p] = 1;
      }
      std::vector<int32_t> seen(n_seen);
      for (int i = 0; i < n_seen; i++)
        if (!(in >> seen[i]) || seen[i] < -1 || seen[i] >= n_points) return refuse("bad seen id");
      std::vector<uint32_t> first(n_points, lm::kNone);
      std::vector<int32_t> out;
      std::vector<uint8_t> seen_out;
      for (int pass = 0; pass < 2; pass++) {  // twice over one scratch: the reset leaves it usable
        if (!lm::lm_host_distinct(rows, bad, &first, seen, &out, &seen_out)) return refuse("lm_host_distinct refused");
        for (uint32_t v : first)
          if (v != lm::kNone) return refuse("the scratch was not reset");
      }
      printf("%zu", out.size());
      for (int p : out) printf(" %d", p);
      printf(" |");
      for (uint8_t s : seen_out) printf(" %d", s);
      printf("\n");
    } else if (kind == "C") {
      int M, S, P, n_stored, n_list;
      if (!(in >> M >> S >> P >> n_stored)) return refuse("short C header");
      if (cc::Core::check_create(M, S, P)) return refuse("C header out of range");
      cc::Core core;
      core.init(M, S, P);
      for (int k = 0; k < n_stored; k++) {
        long long id;
        int len;
        if (!(in >> id >> len) || len < 0 || len > S) return refuse("bad stored keyframe");
        std::vector<int32_t> row(len, -1);
        int r = -1, top = 0;
        if (core.prepare_keyframe(id, (uint64_t)id, len, row.data(), &r, &top)) return refuse("keyframe refused");
        core.commit_keyframe(r, id, (uint64_t)id, len, top);
      }
      if (!(in >> n_list) || n_list < 0 || n_list > 10000) return refuse("bad list length");
      std::vector<int64_t> ids(n_list);
      for (int i = 0; i < n_list; i++) {
        long long v;
        if (!(in >> v)) return refuse("short list");
        ids[i] = v;
      }
      std::vector<int32_t> rows;
      lm::Plan plan;
      const cc::Status st = lm::check_list(core, n_list, ids.data(), &rows, &plan);
      printf("%d %d %d %d %lld %d\n", st.code, plan.max_row, plan.nbx, plan.n_blocks, (long long)plan.named_slots,
             plan.bound);
    } else if (kind == "G" || kind == "S") {
      int P, n;
      if (!(in >> P >> n) || P < 1 || P > (1 << 24) || n < 0 || n > 100000) return refuse("short header");
      cc::Core core;
      core.init(1, 1, P);
      std::vector<int32_t> ids(n);
      std::vector<uint8_t> flags(n, 0);
      for (int i = 0; i < n; i++) {
        int f = 0;
        if (!(in >> ids[i])) return refuse("short ids");
        if (kind == "G" && (!(in >> f) || f < 0 || f > 255)) return refuse("bad flag");
        flags[i] = (uint8_t)f;
      }
      if (kind == "S") {
        printf("%d\n", lm::check_seen(core, n, ids.data()).code);
      } else {
        std::vector<float> f3(3 * (size_t)n + 1, 0.f), f1((size_t)n + 1, 0.f);
        std::vector<uint8_t> d(32 * (size_t)n + 1, 0);
        printf("%d\n", lm::check_geometry(core, n, ids.data(), flags.data(), f3.data(), f3.data(), f1.data(), f1.data(),
                                          d.data()).code);
      }
    } else {
      return refuse("unknown case kind");
    }
  }
  return 0;
}

// ---- the reference's containers ---------------------------------------------------------------
struct MP {
  long unsigned int mnTrackReferenceForFrame = 0;
  bool mbBad = false;
  bool isBad() const { return mbBad; }
};
struct KF {
  std::vector<MP*> mvpMapPoints;
  std::vector<MP*> GetMapPointMatches() const { return mvpMapPoints; }
};

static void update_local_points(const std::vector<KF*>& mvpLocalKeyFrames, long unsigned int frame_id,
                                std::vector<MP*>* mvpLocalMapPoints) {
  mvpLocalMapPoints->clear();
  for (KF* pKF : mvpLocalKeyFrames) {
    const std::vector<MP*> vpMPs = pKF->GetMapPointMatches();
    for (MP* pMP : vpMPs) {
      if (!pMP) continue;
      if (pMP->mnTrackReferenceForFrame == frame_id) continue;
      if (!pMP->isBad()) {
        mvpLocalMapPoints->push_back(pMP);
        pMP->mnTrackReferenceForFrame = frame_id;
      }
    }
  }
}

static int bench(int n_kf, int slots, int observers, int repeats) {
  if (n_kf < 1 || n_kf > 4096 || slots < 1 || slots > 8192 || observers < 1 || repeats < 1) return refuse("bench arguments");
  const int n_points = std::max(1, (int)((long long)n_kf * slots / observers));
  std::mt19937 rng(7);
  std::vector<MP> pts(n_points);
  std::vector<KF> kfs(n_kf);
  const int window = std::max(1, observers * slots / 2);
  for (int k = 0; k < n_kf; k++) {
    kfs[k].mvpMapPoints.resize(slots);
    const long long base = (long long)k * n_points / n_kf;
    for (int s = 0; s < slots; s++)
      kfs[k].mvpMapPoints[s] = (rng() % 10u) ? &pts[(size_t)((base + (long long)(rng() % (unsigned)window)) % n_points)] : nullptr;
  }
  std::vector<KF*> local;
  for (KF& k : kfs) local.push_back(&k);
  std::vector<MP*> out;
  std::vector<double> ms;
  for (int rep = 0; rep < repeats; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    update_local_points(local, (long unsigned int)(rep + 1), &out);
    const auto t1 = std::chrono::steady_clock::now();
    ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"host_update_local_points_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"points\": %zu, \"keyframes\": %d, "
         "\"slots\": %d}\n",
         ms[ms.size() / 2], ms.front(), ms.back(), out.size(), n_kf, slots);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && std::string(argv[1]) == "--bench")
    return bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
  if (argc != 2) return refuse("usage: localmap_core_test CASES | --bench n_kf slots observers repeats");
  return run_cases(argv[1]);
}
