// cull_core_test -- orb_slam2_2021_amd/csrc/orbfe_cull_core.h alone on the host, serially, built with
// ASan + UBSan by tests/test_cull_core.py. Reads a case file the restatement (tests/culling_ref.py) wrote and
// prints one line per case:
//   L n_red n_mps                                   -> cull_keyframe_redundant
//   P bad found visible cur first obs mono          -> cull_point_action
//   S mono n_kf n_points n_bad n_cand, then per keyframe `id len (point attr)*len`, the bad ids, and per
//     candidate `row not_erase`                     -> cull_host_keyframes: decisions, counts, bad lists
// A case the readers refuse: exit status 2.
// --bench n_kf slots observers n_cand repeats: KeyFrameCulling through the reference's containers
// (std::map<KeyFrame*, size_t> mObservations, nObs kept by Add/EraseObservation) on one core, as JSON.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_cull_core.h"

static int refuse(const char* why) {
  fprintf(stderr, "cull_core_test: %s\n", why);
  return 2;
}

static int run_cases(const char* path) {
  std::ifstream in(path);
  if (!in) return refuse("cannot open the case file");
  std::string kind;
  while (in >> kind) {
    if (kind == "L") {
      int n_red, n_mps;
      if (!(in >> n_red >> n_mps)) return refuse("short L case");
      printf("%d\n", cull_keyframe_redundant(n_red, n_mps) ? 1 : 0);
    } else if (kind == "P") {
      int bad, found, visible, obs, mono;
      long long cur, first;
      if (!(in >> bad >> found >> visible >> cur >> first >> obs >> mono)) return refuse("short P case");
      if (cur < 0 || cur >= (1ll << 31) || first < 0 || first >= (1ll << 31)) return refuse("keyframe id range");
      printf("%d\n", cull_point_action(bad, found, visible, cur, first, obs, mono));
    } else if (kind == "S") {
      int mono, n_kf, n_points, n_bad, n_cand;
      if (!(in >> mono >> n_kf >> n_points >> n_bad >> n_cand)) return refuse("short S header");
      if (n_kf < 0 || n_kf > 4096 || n_points < 0 || n_points > (1 << 24) || n_bad < 0 || n_cand < 0 || n_cand > n_kf)
        return refuse("S header out of range");
      CullHostTable t;
      t.bad.assign(n_points, 0);
      for (int k = 0; k < n_kf; k++) {
        long long id;
        int len;
        if (!(in >> id >> len) || len < 0 || len > 8192) return refuse("bad keyframe header");
        if (k > 0 && id <= t.ids.back()) return refuse("keyframes must ascend in mnId");
        t.ids.push_back(id);
        t.rows.emplace_back(len);
        t.attrs.emplace_back(len);
        t.live.push_back(1);
        for (int s = 0; s < len; s++) {
          int p, a;
          if (!(in >> p >> a) || p < -1 || p >= n_points || a < 0 || a > 127) return refuse("bad slot");
          t.rows[k][s] = p;
          t.attrs[k][s] = (uint8_t)a;
        }
      }
      for (int i = 0; i < n_bad; i++) {
        int p;
        if (!(in >> p) || p < 0 || p >= n_points) return refuse("bad point id");
        t.bad[p] = 1;
      }
      std::vector<int> cand;
      std::vector<uint8_t> ne, seen(n_kf, 0);
      for (int i = 0; i < n_cand; i++) {
        int r, e;
        if (!(in >> r >> e) || r < 0 || r >= n_kf || seen[r]) return refuse("bad candidate");
        seen[r] = 1;
        cand.push_back(r);
        ne.push_back(e ? 1 : 0);
      }
      CullHostResult out;
      cull_host_keyframes(&t, cand, ne, mono, &out);
      for (int i = 0; i < n_cand; i++) {
        printf("%d %d %d %d", out.decision[i], out.n_mps[i], out.n_redundant[i], out.bad_begin[i + 1] - out.bad_begin[i]);
        for (int j = out.bad_begin[i]; j < out.bad_begin[i + 1]; j++) printf(" %d", out.bad_points[j]);
        printf(i + 1 < n_cand ? " | " : "");
      }
      printf("\n");
    } else {
      return refuse("unknown case kind");
    }
  }
  return 0;
}

// ---- the reference's containers ---------------------------------------------------------------
struct KF;
struct MP {
  std::map<KF*, size_t> mObservations;
  int nObs = 0;
  bool mbBad = false;
};
struct KF {
  std::vector<MP*> mvpMapPoints;
  std::vector<int> octave;
  std::vector<float> mvuRight;
  bool mbBad = false;
};

static void add_observation(MP* p, KF* kf, size_t idx) {
  if (p->mObservations.count(kf)) return;
  p->mObservations[kf] = idx;
  p->nObs += kf->mvuRight[idx] >= 0 ? 2 : 1;
}

static void erase_observation(MP* p, KF* kf) {
  if (!p->mObservations.count(kf)) return;
  const size_t idx = p->mObservations[kf];
  p->nObs -= kf->mvuRight[idx] >= 0 ? 2 : 1;
  p->mObservations.erase(kf);
  if (p->nObs <= 2) {
    std::map<KF*, size_t> obs = p->mObservations;
    p->mbBad = true;
    p->mObservations.clear();
    for (auto& m : obs) m.first->mvpMapPoints[m.second] = nullptr;
  }
}

static int keyframe_culling(const std::vector<KF*>& local) {
  int culled = 0;
  for (KF* pKF : local) {
    const std::vector<MP*> vpMapPoints = pKF->mvpMapPoints;
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
      MP* pMP = vpMapPoints[i];
      if (!pMP || pMP->mbBad) continue;
      nMPs++;
      if (pMP->nObs > 3) {
        const int scaleLevel = pKF->octave[i];
        const std::map<KF*, size_t> observations = pMP->mObservations;
        int nObs = 0;
        for (auto& m : observations) {
          if (m.first == pKF) continue;
          if (m.first->octave[m.second] <= scaleLevel + 1) {
            nObs++;
            if (nObs >= 3) break;
          }
        }
        if (nObs >= 3) nRedundantObservations++;
      }
    }
    if (nRedundantObservations > 0.9 * nMPs) {
      for (MP* p : pKF->mvpMapPoints)
        if (p) erase_observation(p, pKF);
      pKF->mbBad = true;
      culled++;
    }
  }
  return culled;
}

static int bench(int n_kf, int slots, int observers, int n_cand, int repeats) {
  if (n_kf < 8 || slots < 1 || observers < 1 || n_cand < 1 || n_cand > n_kf || repeats < 1) return refuse("bench arguments");
  const int n_points = std::max(1, (int)((long long)n_kf * slots / observers));
  std::vector<double> ms;
  int culled = 0;
  for (int rep = 0; rep < repeats; rep++) {
    std::mt19937 rng(7);
    std::vector<MP> pts(n_points);
    std::vector<KF> kfs(n_kf);
    for (int k = 0; k < n_kf; k++) {
      KF& kf = kfs[k];
      kf.mvpMapPoints.resize(slots);
      kf.octave.resize(slots);
      kf.mvuRight.resize(slots);
      // a track: keyframe k sees a window of the points, so neighbours overlap; every fifth repeats its neighbour
      const int src = (k % 5 == 4) ? k - 1 : k;
      const long long base = (long long)src * n_points / n_kf;
      for (int s = 0; s < slots; s++) {
        const int p = (int)((base + (long long)(rng() % (unsigned)(observers * slots / 2 + 1))) % n_points);
        kf.mvpMapPoints[s] = &pts[p];
        kf.octave[s] = (int)(rng() % 4u);
        kf.mvuRight[s] = (rng() % 3u) ? -1.f : 10.f;
      }
      for (int s = 0; s < slots; s++) add_observation(kf.mvpMapPoints[s], &kf, (size_t)s);
    }
    std::vector<KF*> local;
    for (int i = 0; i < n_cand; i++) local.push_back(&kfs[(size_t)(n_kf / 2 - n_cand / 2 + i)]);
    const auto t0 = std::chrono::steady_clock::now();
    culled = keyframe_culling(local);
    const auto t1 = std::chrono::steady_clock::now();
    ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"host_keyframe_culling_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"culled\": %d, \"keyframes\": %d, "
         "\"slots\": %d, \"candidates\": %d}\n",
         ms[ms.size() / 2], ms.front(), ms.back(), culled, n_kf, slots, n_cand);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && std::string(argv[1]) == "--bench")
    return bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
  if (argc != 2) return refuse("usage: cull_core_test CASES | --bench n_kf slots observers n_cand repeats");
  return run_cases(argv[1]);
}
