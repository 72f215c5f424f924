// orbfe_env_core.h -- the block envelope of a symmetric sparse system and its unpivoted LDL^T in natural
// order, written once for any block dimension B: the description (EnvWs), the structure pass over
// row_first (EnvPlan, env_plan_structure), the factorisation pivot block by pivot block and the two
// substitutions. Global BundleAdjustment (B = 6, orbfe_gba_core.h: one kernel per step) and
// OptimizeEssentialGraph (B = 7, orbfe_essgraph_core.h: one workgroup for all of it) both run these
// functions, on the device and in their host backends; tests/cpp/env_core_test.cpp holds them to the scalar
// rule. Depends on orbfe_lm_core.h alone (PO_HD, po_finite). Not part of the C ABI. Every operation is an
// IEEE double - * /, rounded separately.
//
// The envelope (DESIGN.md sections 21 and 22): row s of the lower triangle holds the blocks row_first[s]
// .. s; block (s, c) is at L[(row_off[s] + c - row_first[s]) * B * B], row-major. The factorisation is the
// scalar rule v = A_ij; v -= (L_ik d_k) L_jk for k ascending; L_ij = v / d_j, taken pivot block by pivot
// block: an entry takes its updates in ascending scalar pivot index and is divided by d_j when column j's
// block is the pivot, so any mapping of entries to threads gives the same bits; outside the envelope every
// entry is an exact zero. Every loop is capped by a count of the plan; every index read from memory was
// built by env_plan_structure.
#pragma once
#include "orbfe_lm_core.h"

#include <vector>

struct EnvWs {
  int ns;                // block rows
  const int* row_first;  // [ns] the first block column of row s
  const int* row_off;    // [ns + 1] blocks before row s; row s's last block is the diagonal one
  const int* col_begin;  // [ns + 1] the rows s > b whose envelope holds column b ...
  const int* col_row;    // ... ascending
  double* L;             // [nblk * B * B] the matrix, then its factor (strictly lower; the diagonal is d)
  double* d;             // [ns * B]
  double* y;             // [ns * B] the right-hand side, then the solution
};

template <int B>
PO_HD inline double* env_block(const EnvWs& e, int s, int c) {
  return e.L + ((size_t)e.row_off[s] + (c - e.row_first[s])) * (B * B);
}

// Pivot block b by one thread: d_p and the block's strictly lower part, p ascending; sD (B * B) keeps the
// factored block for env_scale_row. -> 0, 1 (a d_p == 0) or 2 (a d_p not finite)
template <int B>
PO_HD inline int env_pivot_diag(const EnvWs& e, int b, double* sD) {
  double* diag = env_block<B>(e, b, b);
  for (int r = 0; r < B; r++)
    for (int c = 0; c <= r; c++) sD[B * r + c] = diag[B * r + c];
  for (int p = 0; p < B; p++) {
    const double dp = sD[(B + 1) * p];
    if (!po_finite(dp)) return 2;
    if (dp == 0.0) return 1;
    e.d[B * (size_t)b + p] = dp;
    for (int r = p + 1; r < B; r++) sD[B * r + p] = sD[B * r + p] / dp;
    for (int r = p + 1; r < B; r++) {
      const double m = sD[B * r + p] * dp;
      for (int c = p + 1; c <= r; c++) sD[B * r + c] = sD[B * r + c] - m * sD[B * c + p];
    }
  }
  for (int r = 0; r < B; r++)
    for (int c = 0; c < r; c++) diag[B * r + c] = sD[B * r + c];
  return 0;
}

// Scalar row t (0 .. rows_below(b) * B - 1) of the column below pivot block b: its B entries, left to right.
// sd: the pivot block's B entries of d, e.d + B * b or a copy of them (a kernel's LDS)
template <int B>
PO_HD inline void env_scale_row(const EnvWs& e, int b, int t, const double* sD, const double* sd) {
  const int s = e.col_row[e.col_begin[b] + t / B];
  double* row = env_block<B>(e, s, b) + B * (t % B);
  double v[B];
  for (int c = 0; c < B; c++) v[c] = row[c];
  for (int c = 0; c < B; c++) {
    double a = v[c];
    for (int p = 0; p < c; p++) a = a - (v[p] * sd[p]) * sD[B * c + p];
    v[c] = a / sd[c];
  }
  for (int c = 0; c < B; c++) row[c] = v[c];
}

PO_HD inline long long env_trailing_items(const EnvWs& e, int b, int bdim) {
  const long long nr = e.col_begin[b + 1] - e.col_begin[b];
  return nr * nr * bdim * bdim;
}

// Item t (0 .. env_trailing_items - 1) of pivot block b's trailing update: one scalar of block (a, bb) of
// the column's rows, bb <= a, takes its B updates in ascending p. sd: as for env_scale_row
template <int B>
PO_HD inline void env_trailing_item(const EnvWs& e, int b, long long t, const double* sd) {
  const int c0 = e.col_begin[b], nr = e.col_begin[b + 1] - c0;
  const int a = (int)(t / ((long long)nr * (B * B))), rem = (int)(t % ((long long)nr * (B * B)));
  const int bb = rem / (B * B), idx = rem % (B * B), r = idx / B, c = idx % B;
  if (bb > a || (bb == a && c > r)) return;
  const int sa = e.col_row[c0 + a], sb = e.col_row[c0 + bb];
  const double* La = env_block<B>(e, sa, b) + B * r;
  const double* Lb = env_block<B>(e, sb, b) + B * c;
  double* dst = env_block<B>(e, sa, sb) + idx;
  double x = *dst;
  for (int p = 0; p < B; p++) x = x - (La[p] * sd[p]) * Lb[p];
  *dst = x;
}

// forward: y_i -= L_ik y_k, k ascending. The pivot block's own rows (one thread), then scalar row t below
template <int B>
PO_HD inline void env_forward_diag(const EnvWs& e, int b) {
  const double* diag = env_block<B>(e, b, b);
  double* yb = e.y + B * (size_t)b;
  for (int r = 1; r < B; r++) {
    double v = yb[r];
    for (int p = 0; p < r; p++) v = v - diag[B * r + p] * yb[p];
    yb[r] = v;
  }
}

template <int B>
PO_HD inline void env_forward_row(const EnvWs& e, int b, int t) {
  const int s = e.col_row[e.col_begin[b] + t / B], r = t % B;
  const double* row = env_block<B>(e, s, b) + B * r;
  const double* yb = e.y + B * (size_t)b;
  double v = e.y[B * (size_t)s + r];
  for (int p = 0; p < B; p++) v = v - row[p] * yb[p];
  e.y[B * (size_t)s + r] = v;
}

// backward: x_i -= L_ki x_k, k descending. Block row s's own part (one thread), then scalar column t
// (0 .. (s - row_first[s]) * B - 1) of the row's blocks left of the diagonal
template <int B>
PO_HD inline void env_backward_diag(const EnvWs& e, int s) {
  const double* diag = env_block<B>(e, s, s);
  double* ys = e.y + B * (size_t)s;
  for (int r = B - 1; r >= 1; r--) {
    const double xr = ys[r];
    for (int c = 0; c < r; c++) ys[c] = ys[c] - diag[B * r + c] * xr;
  }
}

template <int B>
PO_HD inline void env_backward_col(const EnvWs& e, int s, int t) {
  const int cb = t / B, cc = t % B;
  const double* blk = env_block<B>(e, s, e.row_first[s] + cb);
  const double* ys = e.y + B * (size_t)s;
  double* dst = e.y + B * (size_t)(e.row_first[s] + cb) + cc;
  double v = *dst;
  for (int r = B - 1; r >= 0; r--) v = v - blk[B * r + cc] * ys[r];
  *dst = v;
}

// ---- the structure, on the host -------------------------------------------------------------------------
struct EnvPlan {
  int ns = 0;
  long long nblk = 0;
  std::vector<int> row_first, row_off, col_begin, col_row;
};

// From ns and row_first: nblk and, unless it exceeds max_blocks (the plan stops at the count and the
// caller reports the capacity), row_off, col_begin and col_row
inline void env_plan_structure(EnvPlan* E, long long max_blocks) {
  const int ns = E->ns;
  E->nblk = 0;
  for (int s = 0; s < ns; s++) E->nblk += s - E->row_first[s] + 1;
  E->row_off.clear(), E->col_begin.clear(), E->col_row.clear();
  if (E->nblk > max_blocks) return;
  E->row_off.assign(ns + 1, 0);
  for (int s = 0; s < ns; s++) E->row_off[s + 1] = E->row_off[s] + (s - E->row_first[s] + 1);
  E->col_begin.assign(ns + 1, 0);
  for (int s = 0; s < ns; s++)
    for (int c = E->row_first[s]; c < s; c++) E->col_begin[c + 1]++;
  for (int s = 0; s < ns; s++) E->col_begin[s + 1] += E->col_begin[s];
  E->col_row.assign(E->col_begin[ns], 0);
  std::vector<int> cat(E->col_begin.begin(), E->col_begin.end() - 1);
  for (int s = 0; s < ns; s++)
    for (int c = E->row_first[s]; c < s; c++) E->col_row[cat[c]++] = s;
}
