// gba_core_main.cpp -- orbfe_gba_core.h on the host: BundleAdjustment over the problems of a text file,
// result bits printed for tests/test_gba_ref.py to compare with tests/gba_ref.py. Built with
// -fsanitize=address,undefined; no GPU, no library.
//
// Input: the problem count, then per problem "nk np ne stop_at_poll n_iterations robust", nk lines
// "fixed" + 12 floats of tcw + fx fy cx cy bf, then per point "count X Y Z" followed by count lines
// "kf u v ur invSigma2"; every real is the hex bit pattern of a float. Output per problem, one line:
// n_active iterations trials rejected stop lambda chi2 env_blocks schur_blocks flags polls, the 12 nk
// floats of tcw, the 3 np floats of xw. Reals as hex. With a second argument R the problems are solved R
// times over and the wall time of each problem's last solve goes to stderr (timing).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_gba_core.h"

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
  int nk = 0, np = 0, ne = 0, stop_at = -1, n_it = 10, robust = 1;
  std::vector<float> tcw, k, bf, xw, kp, ur, is2;
  std::vector<uint8_t> fixed;
  std::vector<int> edge_begin, e_kf;
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
    if (fscanf(f, "%d %d %d %d %d %d", &p.nk, &p.np, &p.ne, &p.stop_at, &p.n_it, &p.robust) != 6) return 2;
    if (p.nk < 0 || p.nk > 4096 || p.np < 0 || p.np > 524288 || p.ne < 0 || p.ne > 4194304 || p.n_it < 1 || p.n_it > 64) return 2;
    p.tcw.resize(12 * p.nk), p.k.resize(4 * p.nk), p.bf.resize(p.nk), p.fixed.resize(p.nk);
    for (int i = 0; i < p.nk; i++) {
      int fx = 0;
      if (fscanf(f, "%d", &fx) != 1) return 2;
      p.fixed[i] = (uint8_t)fx;
      for (int j = 0; j < 12; j++)
        if (!read_float(f, &p.tcw[12 * i + j])) return 2;
      for (int j = 0; j < 4; j++)
        if (!read_float(f, &p.k[4 * i + j])) return 2;
      if (!read_float(f, &p.bf[i])) return 2;
    }
    p.xw.resize(3 * p.np), p.edge_begin.assign(p.np + 1, 0);
    p.e_kf.resize(p.ne), p.kp.resize(2 * p.ne), p.ur.resize(p.ne), p.is2.resize(p.ne);
    int e = 0;
    for (int i = 0; i < p.np; i++) {
      int c = 0;
      if (fscanf(f, "%d", &c) != 1 || c < 0 || e + c > p.ne) return 2;
      for (int j = 0; j < 3; j++)
        if (!read_float(f, &p.xw[3 * i + j])) return 2;
      for (int j = 0; j < c; j++, e++) {
        if (fscanf(f, "%d", &p.e_kf[e]) != 1 || p.e_kf[e] < 0 || p.e_kf[e] >= p.nk) return 2;
        if (!read_float(f, &p.kp[2 * e]) || !read_float(f, &p.kp[2 * e + 1]) || !read_float(f, &p.ur[e]) || !read_float(f, &p.is2[e]))
          return 2;
      }
      p.edge_begin[i + 1] = e;
    }
    if (e != p.ne) return 2;
  }
  fclose(f);
  for (int rep = 0; rep < repeat; rep++)
    for (const Problem& p : probs) {
      const auto t0 = std::chrono::steady_clock::now();
      GbaIn in = {{p.nk, p.np, p.ne, p.tcw.data(), p.k.data(), p.bf.data(), p.fixed.data(), p.xw.data(), p.edge_begin.data(),
                   p.e_kf.data(), p.kp.data(), p.ur.data(), p.is2.data(), nullptr, p.stop_at},
                  p.n_it,
                  p.robust};
      LbaPlan plan;
      lba_plan(in.l, &plan);
      LbaActive A;
      lba_active(in.l, plan, nullptr, &A);
      GbaEnvPlan E;
      gba_plan_envelope(in.l, plan, A, 2097152, &E);
      if (E.nblk > 2097152) return 3;
      GbaHostBackend b;
      GbaOut o;
      if (gba_run(b, in, plan, A, E, &o) != 0) return 3;
      if (rep + 1 < repeat) continue;
      if (repeat > 1)
        fprintf(stderr, "%d keyframes %d edges: %.3f ms\n", p.nk, p.ne,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      const GbaTrace& t = o.trace;
      printf("%d %d %d %d %d", t.n_active, t.iterations, t.trials, t.rejected_trials, t.stop);
      put64(t.lambda);
      put64(t.chi2);
      printf(" %d %d %u %d", t.env_blocks, t.schur_blocks, t.flags, t.polls);
      for (float v : o.tcw) put32(v);
      for (float v : o.xw) put32(v);
      printf("\n");
    }
  return 0;
}
