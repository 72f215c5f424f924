// mapcorr_core_test.cpp -- orbfe_mapcorr_core.h composed serially on the host: the three map corrections
// over the cases of a text file, result bits printed for tests/test_mapcorr_core.py to compare with
// tests/mapcorr_ref.py. Built with -fsanitize=address,undefined; no GPU, no library.
//
// Input (tests/mapcorr_ref.py write_cases): the case count, then per case its kind (1 update_normal_depth,
// 2 correct_loop, 3 apply_gba), its counts and its arrays; every float is the hex bit pattern of a float (8
// digits), every double of a double (16 digits). Every index is checked as orbfe_mapcorr.hip checks it (exit
// status 2 otherwise). normal / max_dist / min_dist start at the bits 7fc12345. One output line per case.
//
//   mapcorr_core_test cases.txt
//   mapcorr_core_test --bench KEYFRAMES POINTS OBSERVERS CONNECTED REPEATS
// --bench: the host time of the three walks over a generated map, the median of REPEATS, as one JSON line
// (the CPU figure of profiles/mapcorr.py).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_mapcorr_core.h"

static bool read_float(FILE* f, float* out) {
  unsigned bits = 0;
  if (fscanf(f, "%x", &bits) != 1) return false;
  memcpy(out, &bits, 4);
  return true;
}
static bool read_double(FILE* f, double* out) {
  unsigned long long bits = 0;
  if (fscanf(f, "%llx", &bits) != 1) return false;
  memcpy(out, &bits, 8);
  return true;
}
static bool read_floats(FILE* f, std::vector<float>* v, size_t n) {
  v->resize(n);
  for (float& x : *v)
    if (!read_float(f, &x)) return false;
  return true;
}
static bool read_ints(FILE* f, std::vector<int>* v, size_t n) {
  v->resize(n);
  for (int& x : *v)
    if (fscanf(f, "%d", &x) != 1) return false;
  return true;
}
static bool read_bytes(FILE* f, std::vector<uint8_t>* v, size_t n) {
  v->resize(n);
  for (uint8_t& x : *v) {
    int t = 0;
    if (fscanf(f, "%d", &t) != 1 || t < 0 || t > 1) return false;
    x = (uint8_t)t;
  }
  return true;
}
static void put32(float v) {
  unsigned bits;
  memcpy(&bits, &v, 4);
  printf(" %08x", bits);
}
static void put64(double v) {
  unsigned long long bits;
  memcpy(&bits, &v, 8);
  printf(" %016llx", bits);
}

struct Points {
  int n_levels = 0, n_points = 0, n_obs = 0;
  std::vector<float> scale, xw, normal, max_dist, min_dist;
  std::vector<uint8_t> bad, updated;
  std::vector<int> ref_kf, ref_level, obs_begin, obs_kf;

  bool read(FILE* f, int n_kf) {
    if (n_levels < 1 || n_levels > 64 || n_points < 0 || n_points > 1048576 || n_obs < 0 || n_obs > 16777216) return false;
    if (!read_floats(f, &scale, n_levels) || !read_floats(f, &xw, 3 * (size_t)n_points) || !read_bytes(f, &bad, n_points) ||
        !read_ints(f, &ref_kf, n_points) || !read_ints(f, &ref_level, n_points) || !read_ints(f, &obs_begin, (size_t)n_points + 1) ||
        !read_ints(f, &obs_kf, n_obs))
      return false;
    if (obs_begin[0] != 0 || obs_begin[n_points] != n_obs) return false;
    for (int p = 0; p < n_points; p++) {
      if (obs_begin[p] > obs_begin[p + 1] || obs_begin[p] < 0 || obs_begin[p + 1] > n_obs) return false;
      if (!bad[p] && obs_begin[p + 1] > obs_begin[p] &&
          (ref_kf[p] < 0 || ref_kf[p] >= n_kf || ref_level[p] < 0 || ref_level[p] >= n_levels))
        return false;
    }
    for (int k : obs_kf)
      if (k < 0 || k >= n_kf) return false;
    float s;
    const unsigned bits = 0x7fc12345u;
    memcpy(&s, &bits, 4);
    normal.assign(3 * (size_t)n_points, s), max_dist.assign(n_points, s), min_dist.assign(n_points, s);
    updated.assign(n_points, 0);
    return true;
  }
  void bind(McNd* nd) {
    nd->scale = scale.data(), nd->n_levels = n_levels;
    nd->obs_begin = obs_begin.data(), nd->obs_kf = obs_kf.data(), nd->ref_kf = ref_kf.data(), nd->ref_level = ref_level.data();
    nd->normal = normal.data(), nd->max_dist = max_dist.data(), nd->min_dist = min_dist.data(), nd->updated = updated.data();
  }
  void print() const {
    for (uint8_t u : updated) printf(" %d", (int)u);
    for (float v : normal) put32(v);
    for (float v : max_dist) put32(v);
    for (float v : min_dist) put32(v);
  }
};

struct LoopCase {
  int n_kf = 0, n_connected = 0, cur = 0, n_slots = 0;
  std::vector<float> tcw, ow_old, ow_new, tcw_out, xw_out;
  std::vector<int> connected, pos_of_kf, row_begin, row_point, corrected_by;
  std::vector<double> scw, nonc, corr, swi;
  Points pts;

  bool check() {
    if (n_kf < 1 || n_kf > 8192 || n_connected < 1 || n_connected > n_kf || cur < 0 || cur >= n_connected || n_slots < 0) return false;
    pos_of_kf.assign(n_kf, -1);
    for (int i = 0; i < n_connected; i++) {
      const int k = connected[i];
      if (k < 0 || k >= n_kf || pos_of_kf[k] >= 0) return false;
      pos_of_kf[k] = i;
    }
    if (row_begin[0] != 0 || row_begin[n_connected] != n_slots) return false;
    for (int i = 0; i < n_connected; i++)
      if (row_begin[i] > row_begin[i + 1] || row_begin[i] < 0 || row_begin[i + 1] > n_slots) return false;
    for (int q : row_point)
      if (q < -1 || q >= pts.n_points) return false;
    return true;
  }
  McLoop bind() {
    const size_t nc = n_connected, np = pts.n_points;
    ow_old.assign(3 * (size_t)n_kf, 0.f), ow_new.assign(3 * nc, 0.f), tcw_out.assign(12 * nc, 0.f), xw_out.assign(3 * np, 0.f);
    corrected_by.assign(np, 0), nonc.assign(8 * nc, 0.0), corr.assign(8 * nc, 0.0), swi.assign(8 * nc, 0.0);
    McLoop w;
    memset(&w, 0, sizeof(w));
    pts.bind(&w.nd);
    w.nd.ow = ow_old.data(), w.nd.ow_new = ow_new.data(), w.nd.pos_of_kf = pos_of_kf.data();
    w.n_kf = n_kf, w.n_connected = n_connected, w.cur = cur, w.n_points = pts.n_points, w.n_slots = n_slots;
    w.tcw = tcw.data(), w.connected_kf = connected.data();
    for (int k = 0; k < 8; k++) w.scw[k] = scw[k];
    w.row_begin = row_begin.data(), w.row_point = row_point.data(), w.xw = pts.xw.data(), w.bad = pts.bad.data();
    w.ow_old = ow_old.data(), w.ow_new = ow_new.data(), w.nonc = nonc.data(), w.corr = corr.data(), w.swi = swi.data();
    w.tcw_out = tcw_out.data(), w.xw_out = xw_out.data(), w.corrected_by = corrected_by.data();
    return w;
  }
};

struct GbaCase {
  int n_kf = 0, n_points = 0;
  std::vector<float> tcw, tcw_gba, xw, xw_gba, tcw_out, ow_out, xw_out;
  std::vector<uint8_t> optimised, bad, pt_optimised, pt_changed;
  std::vector<int> parent, ref_kf;
  McGbaPlan plan;

  McGba bind() {
    tcw_out.assign(12 * (size_t)n_kf, 0.f), ow_out.assign(3 * (size_t)n_kf, 0.f), xw_out.assign(3 * (size_t)n_points, 0.f);
    pt_changed.assign(n_points, 0);
    McGba w;
    memset(&w, 0, sizeof(w));
    w.n_kf = n_kf, w.n_points = n_points, w.tcw = tcw.data(), w.tcw_gba = tcw_gba.data(), w.optimised = optimised.data();
    w.parent = parent.data(), w.order = plan.order.data(), w.xw = xw.data(), w.bad = bad.data(), w.pt_optimised = pt_optimised.data();
    w.xw_gba = xw_gba.data(), w.ref_kf = ref_kf.data(), w.tcw_out = tcw_out.data(), w.ow_out = ow_out.data();
    w.xw_out = xw_out.data(), w.pt_changed = pt_changed.data();
    return w;
  }
};

static int run_file(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  int count = 0;
  if (fscanf(f, "%d", &count) != 1 || count < 0 || count > 4096) return 2;
  for (int c = 0; c < count; c++) {
    int kind = 0;
    if (fscanf(f, "%d", &kind) != 1) return 2;
    if (kind == 1) {
      int n_kf = 0;
      Points P;
      std::vector<float> ow;
      if (fscanf(f, "%d %d %d %d", &n_kf, &P.n_levels, &P.n_points, &P.n_obs) != 4 || n_kf < 0 || n_kf > 8192) return 2;
      if (!read_floats(f, &ow, 3 * (size_t)n_kf) || !P.read(f, n_kf)) return 2;
      McNd nd;
      memset(&nd, 0, sizeof(nd));
      P.bind(&nd);
      nd.ow = ow.data();
      mc_host_normals(nd, P.n_points, P.xw.data(), P.bad.data());
      P.print();
    } else if (kind == 2) {
      LoopCase L;
      Points& P = L.pts;
      if (fscanf(f, "%d %d %d %d %d %d %d", &L.n_kf, &L.n_connected, &L.cur, &L.n_slots, &P.n_levels, &P.n_points, &P.n_obs) != 7) return 2;
      if (L.n_kf < 1 || L.n_kf > 8192 || L.n_connected < 1 || L.n_connected > L.n_kf || L.n_slots < 0 || L.n_slots > 16777216) return 2;
      L.scw.resize(8);
      if (!read_floats(f, &L.tcw, 12 * (size_t)L.n_kf) || !read_ints(f, &L.connected, L.n_connected)) return 2;
      for (double& v : L.scw)
        if (!read_double(f, &v)) return 2;
      if (!read_ints(f, &L.row_begin, (size_t)L.n_connected + 1) || !read_ints(f, &L.row_point, L.n_slots) || !P.read(f, L.n_kf)) return 2;
      if (!L.check()) return 2;
      const McLoop w = L.bind();
      mc_host_loop(w);
      for (double v : L.nonc) put64(v);
      for (double v : L.corr) put64(v);
      for (float v : L.tcw_out) put32(v);
      for (float v : L.xw_out) put32(v);
      for (int v : L.corrected_by) printf(" %d", v);
      P.print();
    } else if (kind == 3) {
      GbaCase G;
      if (fscanf(f, "%d %d", &G.n_kf, &G.n_points) != 2 || G.n_kf < 0 || G.n_kf > 8192 || G.n_points < 0 || G.n_points > 1048576) return 2;
      if (!read_floats(f, &G.tcw, 12 * (size_t)G.n_kf) || !read_floats(f, &G.tcw_gba, 12 * (size_t)G.n_kf) ||
          !read_bytes(f, &G.optimised, G.n_kf) || !read_ints(f, &G.parent, G.n_kf) || !read_floats(f, &G.xw, 3 * (size_t)G.n_points) ||
          !read_bytes(f, &G.bad, G.n_points) || !read_bytes(f, &G.pt_optimised, G.n_points) ||
          !read_floats(f, &G.xw_gba, 3 * (size_t)G.n_points) || !read_ints(f, &G.ref_kf, G.n_points))
        return 2;
      if (mc_gba_plan(G.n_kf, G.parent.data(), G.optimised.data(), &G.plan) != MC_PLAN_OK) return 2;
      for (int k : G.ref_kf)
        if (k < -1 || k >= G.n_kf) return 2;
      mc_host_gba(G.bind());
      printf(" %d", (int)G.plan.level_begin.size() - 1);
      for (float v : G.tcw_out) put32(v);
      for (int k = 0; k < G.n_kf; k++) printf(" %d", G.optimised[k] ? 0 : 1);
      for (float v : G.xw_out) put32(v);
      for (uint8_t v : G.pt_changed) printf(" %d", (int)v);
    } else {
      return 2;
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}

// The plan's own properties on hand-built trees
static int self_test() {
  McGbaPlan P;
  {  // origin(opt) -> a(non) -> b(non) -> c(opt) -> d(non)
    const int parent[5] = {-1, 0, 1, 2, 3};
    const uint8_t opt[5] = {1, 0, 0, 1, 0};
    if (mc_gba_plan(5, parent, opt, &P) != MC_PLAN_OK) return 1;
    const std::vector<int> order = {0, 3, 1, 4, 2}, begin = {0, 2, 4, 5};
    if (P.order != order || P.level_begin != begin) return 1;
  }
  {
    const int self[2] = {-1, 1}, cyc[3] = {-1, 2, 1}, far[2] = {-1, 2}, low[2] = {-1, -2}, opt_cycle[3] = {-1, 2, 1};
    const uint8_t opt[3] = {1, 0, 0}, all[3] = {1, 1, 1}, none[1] = {0};
    const int origin[1] = {-1};
    if (mc_gba_plan(2, self, opt, &P) != MC_PLAN_CYCLE || mc_gba_plan(3, cyc, opt, &P) != MC_PLAN_CYCLE ||
        mc_gba_plan(3, opt_cycle, all, &P) != MC_PLAN_CYCLE || mc_gba_plan(2, far, opt, &P) != MC_PLAN_PARENT ||
        mc_gba_plan(2, low, opt, &P) != MC_PLAN_PARENT || mc_gba_plan(1, origin, none, &P) != MC_PLAN_ORIGIN)
      return 1;
    if (mc_gba_plan(0, origin, none, &P) != MC_PLAN_OK || !P.order.empty() || P.level_begin.size() != 1) return 1;
  }
  return 0;
}

static unsigned long long g_rng = 88172645463325252ull;
static double rnd() {  // xorshift64, [0, 1)
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}

template <class F>
static double median_ms(int repeats, F&& fn) {
  std::vector<double> t;
  for (int r = 0; r < repeats; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    fn();
    t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

// A track: keyframe k at x = 0.1 k looking down +z with a small yaw; point p in front of keyframe
// p * n_kf / n_points, seen by the `observers` keyframes from there on.
static int bench(int n_kf, int n_points, int observers, int n_connected, int repeats) {
  if (n_kf < 2 || n_kf > 8192 || n_points < 1 || n_points > 1048576 || observers < 1 || observers > n_kf || n_connected < 1 ||
      n_connected > n_kf || repeats < 1 || (long long)n_points * observers > 16777216)
    return 2;
  LoopCase L;
  Points& P = L.pts;
  L.n_kf = n_kf, L.n_connected = n_connected, L.cur = n_connected - 1;
  L.tcw.resize(12 * (size_t)n_kf);
  std::vector<float> ow(3 * (size_t)n_kf);
  for (int k = 0; k < n_kf; k++) {
    const double a = 0.02 * (rnd() - 0.5), c = cos(a), s = sin(a);
    const float T[12] = {(float)c, 0.f, (float)s, (float)(-0.1 * k * c), 0.f, 1.f, 0.f, 0.f, (float)-s, 0.f, (float)c, (float)(0.1 * k * s)};
    memcpy(&L.tcw[12 * (size_t)k], T, sizeof(T));
    mc_centre(T, &ow[3 * (size_t)k]);
  }
  P.n_levels = 8, P.n_points = n_points, P.n_obs = n_points * observers;
  P.scale.resize(8);
  P.scale[0] = 1.0f;
  for (int l = 1; l < 8; l++) P.scale[l] = P.scale[l - 1] * 1.2f;
  P.xw.resize(3 * (size_t)n_points), P.bad.assign(n_points, 0), P.ref_kf.resize(n_points), P.ref_level.resize(n_points);
  P.obs_begin.resize((size_t)n_points + 1), P.obs_kf.resize(P.n_obs);
  std::vector<std::vector<int>> rows(n_kf);
  for (int p = 0; p < n_points; p++) {
    int first = (int)((long long)p * n_kf / n_points);
    if (first > n_kf - observers) first = n_kf - observers;
    P.xw[3 * (size_t)p] = (float)(0.1 * first + 4.0 * (rnd() - 0.5));
    P.xw[3 * (size_t)p + 1] = (float)(2.0 * (rnd() - 0.5));
    P.xw[3 * (size_t)p + 2] = (float)(4.0 + 8.0 * rnd());
    P.ref_kf[p] = first, P.ref_level[p] = (int)(8 * rnd()) & 7;
    P.obs_begin[p] = p * observers;
    for (int o = 0; o < observers; o++) {
      P.obs_kf[(size_t)p * observers + o] = first + o;
      rows[first + o].push_back(p);
    }
  }
  P.obs_begin[n_points] = P.n_obs;
  const unsigned bits = 0x7fc12345u;
  float s;
  memcpy(&s, &bits, 4);
  P.normal.assign(3 * (size_t)n_points, s), P.max_dist.assign(n_points, s), P.min_dist.assign(n_points, s), P.updated.assign(n_points, 0);
  // the connected keyframes: the last n_connected of the track, the current one last
  L.row_begin.assign(1, 0);
  for (int i = 0; i < n_connected; i++) {
    const int k = n_kf - n_connected + i;
    L.connected.push_back(k);
    L.row_point.insert(L.row_point.end(), rows[k].begin(), rows[k].end());
    L.row_begin.push_back((int)L.row_point.size());
  }
  L.n_slots = (int)L.row_point.size();
  L.scw.resize(8);
  {
    OsSim3 S, D = {{0.0, 0.01, 0.0, 1.0}, {0.3, 0.0, -0.2}, 1.05}, out;
    mc_sim3_of_pose(&L.tcw[12 * (size_t)(n_kf - 1)], &S);
    os_sim3_mul(D, S, &out);
    os_store_state(L.scw.data(), out);
  }
  if (!L.check()) return 2;
  GbaCase G;
  G.n_kf = n_kf, G.n_points = n_points, G.tcw = L.tcw, G.tcw_gba = L.tcw, G.xw = P.xw, G.xw_gba = P.xw, G.bad = P.bad, G.ref_kf = P.ref_kf;
  G.optimised.assign(n_kf, 1), G.parent.resize(n_kf), G.pt_optimised.assign(n_points, 1);
  for (int k = 0; k < n_kf; k++) {
    G.parent[k] = k - 1;
    if (k >= n_kf - 8 && k > 0) G.optimised[k] = 0;  // the keyframes inserted while the optimiser ran
    for (int j = 0; j < 12; j++) G.tcw_gba[12 * (size_t)k + j] += (j % 4 == 3) ? 0.01f : 0.0f;
  }
  for (int p = 0; p < n_points; p += 10) G.pt_optimised[p] = 0;

  McNd nd;
  memset(&nd, 0, sizeof(nd));
  P.bind(&nd);
  nd.ow = ow.data();
  const double t_normals = median_ms(repeats, [&] { mc_host_normals(nd, n_points, P.xw.data(), P.bad.data()); });
  const McLoop w = L.bind();
  const double t_loop = median_ms(repeats, [&] { mc_host_loop(w); });
  const double t_gba = median_ms(repeats, [&] {
    if (mc_gba_plan(n_kf, G.parent.data(), G.optimised.data(), &G.plan) != MC_PLAN_OK) abort();
    mc_host_gba(G.bind());
  });
  int corrected = 0;
  for (int v : L.corrected_by) corrected += v >= 0;
  printf("{\"keyframes\": %d, \"points\": %d, \"observers\": %d, \"connected\": %d, \"row_slots\": %d, \"corrected_points\": %d, "
         "\"repeats\": %d, \"host_update_normal_depth_ms\": %.4f, \"host_correct_loop_ms\": %.4f, \"host_apply_gba_ms\": %.4f}\n",
         n_kf, n_points, observers, n_connected, L.n_slots, corrected, repeats, t_normals, t_loop, t_gba);
  return 0;
}

int main(int argc, char** argv) {
  if (self_test() != 0) {
    fprintf(stderr, "the plan's self test failed\n");
    return 1;
  }
  if (argc == 7 && strcmp(argv[1], "--bench") == 0) return bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
  if (argc != 2) return 2;
  return run_file(argv[1]);
}
