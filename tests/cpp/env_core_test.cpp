// The block-envelope LDL^T of orb_slam2_2021_amd/csrc/orbfe_env_core.h against the scalar rule it stands
// for, written out here: v = A_ij; v -= (L_ik d_k) L_jk, k ascending; L_ij = v / d_j; then
// y_i -= L_ik y_k (k ascending), y_i / d_i, x_i -= L_ki x_k (k descending). For B = 6 and B = 7 a small
// envelope (5 block rows, row_first = 0 0 1 1 3) is filled with diagonally dominant values from a fixed
// integer recurrence and solved both ways: d, every L entry inside the envelope and the solution must be
// equal on their bits. env_pivot_diag must report an exact zero pivot (1) and a NaN pivot (2) and leave L
// as it was. Stand-alone, CPU only; tests/test_env_core.py builds it with ASan + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_env_core.h"

static int g_failed = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      g_failed++;                                                 \
    }                                                             \
  } while (0)

static uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}

struct Rng {  // the fixed recurrence: 31-bit linear congruential
  uint32_t x;
  int next(int mod) {
    x = (x * 1103515245u + 12345u) & 0x7fffffffu;
    return (int)((x >> 16) % (uint32_t)mod);
  }
};

template <int B>
struct Env {
  EnvPlan plan;
  std::vector<double> L, d, y;
  EnvWs ws;
  Env() {
    plan.ns = 5;
    plan.row_first = {0, 0, 1, 1, 3};
    env_plan_structure(&plan, 1 << 20);
    L.assign((size_t)plan.nblk * B * B, 0.0), d.assign(B * plan.ns, 0.0), y.assign(B * plan.ns, 0.0);
    ws = {plan.ns, plan.row_first.data(), plan.row_off.data(), plan.col_begin.data(), plan.col_row.data(), L.data(), d.data(), y.data()};
  }
};

template <int B>
static void check_structure() {
  Env<B> e;
  const EnvPlan& p = e.plan;
  CHECK(p.nblk == 1 + 2 + 2 + 3 + 2);
  CHECK((p.row_off == std::vector<int>{0, 1, 3, 5, 8, 10}));
  CHECK((p.col_begin == std::vector<int>{0, 1, 3, 4, 5, 5}));  // column 0: row 1; 1: rows 2 3; 2: row 3; 3: row 4
  CHECK((p.col_row == std::vector<int>{1, 2, 3, 3, 4}));
  EnvPlan q;
  q.ns = 5, q.row_first = {0, 0, 1, 1, 3};
  env_plan_structure(&q, 9);  // above the capacity: the count only
  CHECK(q.nblk == 10 && q.row_off.empty() && q.col_begin.empty() && q.col_row.empty());
}

template <int B>
static void check_solve() {
  Env<B> e;
  const EnvWs& w = e.ws;
  const int ns = w.ns, n = B * ns;
  auto c0 = [&](int i) { return B * w.row_first[i / B]; };
  // the matrix, dense and symmetric, zero outside the envelope; the right-hand side
  std::vector<double> A((size_t)n * n, 0.0), rhs(n);
  Rng rng = {2021u + B};
  for (int i = 0; i < n; i++) {
    for (int j = c0(i); j < i; j++) A[(size_t)i * n + j] = A[(size_t)j * n + i] = (rng.next(201) - 100) / 64.0;
    A[(size_t)i * n + i] = 64.0 + rng.next(16) / 8.0;  // a row's off-diagonal sum is below 34 * 100 / 64
    rhs[i] = (rng.next(2001) - 1000) / 32.0;
  }
  for (int s = 0; s < ns; s++)
    for (int c = w.row_first[s]; c <= s; c++)
      for (int r = 0; r < B; r++)
        for (int cc = 0; cc < (c == s ? r + 1 : B); cc++) env_block<B>(w, s, c)[B * r + cc] = A[(size_t)(B * s + r) * n + B * c + cc];
  // the backends' order
  for (int b = 0; b < ns; b++) {
    double sD[B * B];
    CHECK(env_pivot_diag<B>(w, b, sD) == 0);
    const int nr = w.col_begin[b + 1] - w.col_begin[b];
    for (int t = 0; t < B * nr; t++) env_scale_row<B>(w, b, t, sD, w.d + B * b);
    CHECK(env_trailing_items(w, b, B) == (long long)nr * nr * B * B);
    for (long long t = 0; t < env_trailing_items(w, b, B); t++) env_trailing_item<B>(w, b, t, w.d + B * b);
  }
  for (int i = 0; i < n; i++) w.y[i] = rhs[i];
  for (int b = 0; b < ns; b++) {
    env_forward_diag<B>(w, b);
    const int nr = w.col_begin[b + 1] - w.col_begin[b];
    for (int t = 0; t < B * nr; t++) env_forward_row<B>(w, b, t);
  }
  for (int i = 0; i < n; i++) w.y[i] = w.y[i] / w.d[i];
  for (int s = ns - 1; s >= 0; s--) {
    env_backward_diag<B>(w, s);
    for (int t = 0; t < B * (s - w.row_first[s]); t++) env_backward_col<B>(w, s, t);
  }
  // the scalar rule, row by row
  std::vector<double> Lr((size_t)n * n, 0.0), dr(n), x(n);
  for (int i = 0; i < n; i++)
    for (int j = c0(i); j <= i; j++) {
      double v = A[(size_t)i * n + j];
      for (int k = c0(i) > c0(j) ? c0(i) : c0(j); k < j; k++) v = v - (Lr[(size_t)i * n + k] * dr[k]) * Lr[(size_t)j * n + k];
      if (j < i) Lr[(size_t)i * n + j] = v / dr[j];
      else dr[i] = v;
    }
  for (int i = 0; i < n; i++) {
    double v = rhs[i];
    for (int k = c0(i); k < i; k++) v = v - Lr[(size_t)i * n + k] * x[k];
    x[i] = v;
  }
  for (int i = 0; i < n; i++) x[i] = x[i] / dr[i];
  for (int k = n - 1; k >= 0; k--)
    for (int i = c0(k); i < k; i++) x[i] = x[i] - Lr[(size_t)k * n + i] * x[k];
  int entries = 0;
  for (int i = 0; i < n; i++) {
    CHECK(dr[i] > 0.0 && bits(w.d[i]) == bits(dr[i]));
    CHECK(bits(w.y[i]) == bits(x[i]));
    for (int j = c0(i); j < i; j++, entries++) CHECK(bits(env_block<B>(w, i / B, j / B)[B * (i % B) + j % B]) == bits(Lr[(size_t)i * n + j]));
  }
  CHECK(entries == 10 * B * B - ns * B * (B + 1) / 2);  // every block, less the diagonal blocks' upper halves
  // the solution solves the system: a residual far below the entries' size (not a bit-level claim)
  for (int i = 0; i < n; i++) {
    double r = -rhs[i];
    for (int j = 0; j < n; j++) r += A[(size_t)i * n + j] * x[j];
    CHECK(std::fabs(r) < 1e-9);
  }
}

template <int B>
static void check_bad_pivot(double bad, int want) {
  Env<B> e;
  const EnvWs& w = e.ws;
  for (int s = 0; s < w.ns; s++)
    for (int r = 0; r < B; r++) env_block<B>(w, s, s)[(B + 1) * r] = 1.0;
  double* blk = env_block<B>(w, 1, 1);
  // d_1 = 1 - (0.5 * 1) * 0.5 = 0.75, l_21 = 0.375 / 0.75 = 0.5, so d_2 = a_22 - (0.5 * 0.75) * 0.5 is an exact zero
  blk[B * 1 + 0] = 0.5, blk[B * 2 + 1] = 0.375;
  blk[(B + 1) * 2] = bad == 0.0 ? 0.1875 : bad;
  const std::vector<double> before = e.L;
  double sD[B * B];
  CHECK(env_pivot_diag<B>(w, 0, sD) == 0);
  CHECK(env_pivot_diag<B>(w, 1, sD) == want);
  CHECK(memcmp(before.data(), e.L.data(), 8 * before.size()) == 0);
}

int main() {
  check_structure<6>(), check_structure<7>();
  check_solve<6>(), check_solve<7>();
  check_bad_pivot<6>(0.0, 1), check_bad_pivot<7>(0.0, 1);
  check_bad_pivot<6>(std::numeric_limits<double>::quiet_NaN(), 2), check_bad_pivot<7>(std::numeric_limits<double>::quiet_NaN(), 2);
  check_bad_pivot<6>(std::numeric_limits<double>::infinity(), 2);
  if (g_failed) return 1;
  printf("OK envelope core\n");
  return 0;
}
