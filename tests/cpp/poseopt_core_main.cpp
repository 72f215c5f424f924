// poseopt_core_main.cpp -- orbfe_poseopt_core.h on the host: PoseOptimization over the problems of a
// text file, result bits printed for tests/test_poseopt_ref.py to compare with tests/poseopt_ref.py.
// Built with -fsanitize=address,undefined; no GPU, no library.
//
// Input: the problem count, then per problem "n fx fy cx cy bf" and the 12 floats of tcw, then n lines
// "valid X Y Z u v ur invSigma2"; every real is the hex bit pattern of a float. Output per problem, one
// line: n_initial n_bad n_inliers rounds_run flags, the 12 floats of tcw, the 7 doubles of the pose,
// the mask words and, for each of the 4 rounds, n_active iterations trials rejected stop n_bad lambda
// chi2; then the number of edges whose flag would differ had the last round classified them at the
// final estimate. Reals as hex. With a second argument R the problems are solved R times over (timing).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_poseopt_core.h"

static bool read_float(FILE* f, float* out) {
  unsigned bits = 0;
  if (fscanf(f, "%x", &bits) != 1) return false;
  memcpy(out, &bits, 4);
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

struct Problem {
  int n = 0;
  float cam[5], tcw[12];
  std::vector<uint8_t> valid;
  std::vector<float> xw, kp, ur, is2;
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const int repeat = argc > 2 ? atoi(argv[2]) : 1;
  int count = 0;
  if (fscanf(f, "%d", &count) != 1 || count < 0 || count > 4096) return 2;
  std::vector<Problem> probs(count);
  for (Problem& p : probs) {
    if (fscanf(f, "%d", &p.n) != 1 || p.n < 0 || p.n > 4096) return 2;
    for (int i = 0; i < 5; i++)
      if (!read_float(f, &p.cam[i])) return 2;
    for (int i = 0; i < 12; i++)
      if (!read_float(f, &p.tcw[i])) return 2;
    p.valid.resize(p.n), p.xw.resize(3 * p.n), p.kp.resize(2 * p.n), p.ur.resize(p.n), p.is2.resize(p.n);
    for (int i = 0; i < p.n; i++) {
      int v = 0;
      if (fscanf(f, "%d", &v) != 1) return 2;
      p.valid[i] = (uint8_t)v;
      float r[7];
      for (int j = 0; j < 7; j++)
        if (!read_float(f, &r[j])) return 2;
      p.xw[3 * i] = r[0], p.xw[3 * i + 1] = r[1], p.xw[3 * i + 2] = r[2];
      p.kp[2 * i] = r[3], p.kp[2 * i + 1] = r[4];
      p.ur[i] = r[5];
      p.is2[i] = r[6];
    }
  }
  fclose(f);
  for (int rep = 0; rep < repeat; rep++)
    for (const Problem& p : probs) {
      PoProblem P;
      P.n = p.n;
      P.valid = p.valid.data(), P.xw = p.xw.data(), P.kp = p.kp.data(), P.ur = p.ur.data(), P.inv_sigma2 = p.is2.data();
      P.fx = p.cam[0], P.fy = p.cam[1], P.cx = p.cam[2], P.cy = p.cam[3], P.bf = p.cam[4];
      P.tcw = p.tcw;
      PoWork w;
      memset(&w, 0, sizeof(w));
      PoOut o;
      memset(&o, 0, sizeof(o));
      const int words = (p.n + 63) / 64;
      std::vector<uint64_t> mask(words > 0 ? words : 1, 0);
      po_optimize(PoHostGroup(), P, w, &o, mask.data());
      if (rep + 1 < repeat) continue;
      printf("%d %d %d %d %u", o.n_initial, o.n_bad, o.n_inliers, o.rounds_run, o.flags);
      for (int i = 0; i < 12; i++) put32(o.tcw[i]);
      for (int i = 0; i < 7; i++) put64(o.pose[i]);
      for (int i = 0; i < words; i++) printf(" %016llx", (unsigned long long)mask[i]);
      for (int it = 0; it < 4; it++) {
        const PoRound& r = o.rounds[it];
        printf(" %d %d %d %d %d %d", r.n_active, r.iterations, r.trials, r.rejected_trials, r.stop, r.n_bad);
        put64(r.lambda);
        put64(r.chi2);
      }
      // edges whose flag would differ had the last round classified them at the final estimate
      int stale = 0;
      PoSE3 est;
      for (int i = 0; i < 4; i++) est.q[i] = o.pose[i];
      for (int i = 0; i < 3; i++) est.t[i] = o.pose[4 + i];
      for (int i = 0; i < p.n && o.rounds_run > 0; i++) {
        if (!p.valid[i]) continue;
        PoEdge e;
        po_load_edge(P, i, &e);
        double pt[3], err[3];
        po_edge_error(P, e, est, pt, err);
        const bool flag = (float)po_edge_chi2(e, err) > (e.stereo ? 7.815f : 5.991f);
        if (flag != (bool)((mask[i >> 6] >> (i & 63)) & 1ull)) stale++;
      }
      printf(" %d\n", stale);
    }
  return 0;
}
