// orbfe_gba_core.h -- Optimizer::BundleAdjustment's arithmetic (Optimizer.cc:51-240) on top of
// orbfe_lba_core.h: the BA edges, Huber, the per-point and per-pose sums, Dinv, the Schur lanes, the
// back-substitution, the update, the reduction and the Levenberg round are that header's, unchanged. New
// here: the plan of the reduced system as a 6x6 block envelope over the covisible keyframe pairs, the
// Schur blocks written into it, the block-envelope LDL^T with its two substitutions (templated on the
// block dimension), GbaHostBackend and gba_run (one optimize(nIterations), every keyframe written out).
// Used by orbfe_gba.hip and tests/cpp/gba_core_main.cpp; tests/gba_ref.py is the same code in Python. Not
// part of the C ABI. Every operation is an IEEE double + - * / sqrt, rounded separately.
//
// The envelope: slot s is the s-th free keyframe with an edge; row s of the lower
// triangle holds the blocks row_first[s] .. s, row_first[s] the smallest slot that shares a point with s;
// block (s, c) is at L[(row_off[s] + c - row_first[s]) * B * B], row-major. The factorisation is the
// scalar rule of orbfe_essgraph.h, v = A_ij; v -= (L_ik d_k) L_jk for k ascending; L_ij = v / d_j, taken
// pivot block by pivot block: inside the envelope it is orbfe_lba_core.h's dense lba_ldlt_dot, outside
// every entry is an exact zero. Every loop is capped by a count of the plan; every index read from memory
// was built by gba_plan_envelope or checked by orbfe_gba_solve.
#pragma once
#include "orbfe_lba_core.h"

#include <algorithm>

// ---- the block envelope: one description, any block dimension -------------------------------------------
struct EnvWs {
  int ns;                // block rows
  const int* row_first;  // [ns] the first block column of row s
  const int* row_off;    // [ns + 1] blocks before row s
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

// Scalar row t (0 .. rows_below(b) * B - 1) of the column below pivot block b: its B entries, left to right
template <int B>
PO_HD inline void env_scale_row(const EnvWs& e, int b, int t, const double* sD) {
  const int s = e.col_row[e.col_begin[b] + t / B];
  double* row = env_block<B>(e, s, b) + B * (t % B);
  const double* sd = e.d + B * (size_t)b;
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
// the column's rows, bb <= a, takes its B updates in ascending p
template <int B>
PO_HD inline void env_trailing_item(const EnvWs& e, int b, long long t) {
  const int c0 = e.col_begin[b], nr = e.col_begin[b + 1] - c0;
  const int a = (int)(t / ((long long)nr * (B * B))), rem = (int)(t % ((long long)nr * (B * B)));
  const int bb = rem / (B * B), idx = rem % (B * B), r = idx / B, c = idx % B;
  if (bb > a || (bb == a && c > r)) return;
  const int sa = e.col_row[c0 + a], sb = e.col_row[c0 + bb];
  const double* La = env_block<B>(e, sa, b) + B * r;
  const double* Lb = env_block<B>(e, sb, b) + B * c;
  const double* sd = e.d + B * (size_t)b;
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

// ---- the workspace ---------------------------------------------------------------------------------------
struct GbaWs {
  LbaWs l;  // S, Lm, Mm are not used: the reduced system is env; bs, d, y, xp are [6 nslot]
  EnvWs env;
  int npair;
  const int* pair_s1;  // [npair] the structural pairs s1 <= s2, sorted by (s2, s1)
  const int* pair_s2;
};

// Optimizer.cc:87-88: const float thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815)
inline void gba_set_deltas(LbaWs* w) { w->delta_mono = (double)(float)sqrt(5.99), w->delta_stereo = (double)(float)sqrt(7.815); }

// lba_schur_finish into the envelope: S(6 s1 + r, 6 s2 + c), s1 <= s2, is entry (c, r) of block (s2, s1);
// of a diagonal block the lower triangle is written. bschur on the diagonal pairs.
PO_HD inline void gba_schur_finish(const GbaWs& g, int s1, int s2, double lambda, const double* acc) {
  const LbaWs& w = g.l;
  const int f1 = w.free_of_slot[s1];
  double* blk = env_block<6>(g.env, s2, s1);
  bool ok = true;
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      if (s1 == s2 && r > c) continue;
      double h = 0.0;
      if (s1 == s2) h = w.hpp[21 * (size_t)f1 + lba_upper(r, c)];
      if (s1 == s2 && r == c) h = h + lambda;
      const double v = h - acc[6 * r + c];
      blk[6 * c + r] = v;
      ok = ok && po_finite(v);
    }
  if (s1 == s2)
    for (int r = 0; r < 6; r++) {
      const double v = w.bp[6 * (size_t)f1 + r] - acc[36 + r];
      w.bs[6 * (size_t)s1 + r] = v;
      ok = ok && po_finite(v);
    }
  if (!ok) lm_fail(w.rec, LM_FLAG_NONFINITE);
}

// ---- the host side ---------------------------------------------------------------------------------------
struct GbaIn {
  LbaIn l;
  int n_iterations, robust;
};

struct GbaTrace {
  int32_t n_active, iterations, trials, rejected_trials, stop;
  double lambda, chi2;
  int32_t env_blocks, schur_blocks;
  uint32_t flags;
  int32_t polls;
};

struct GbaOut {
  std::vector<float> tcw, xw;
  GbaTrace trace;
};

// The slots' envelope. A: lba_active(in, P, nullptr): the slots are the free keyframes with an edge.
struct GbaEnvPlan {
  int ns = 0;
  long long nblk = 0, npair = 0;
  std::vector<int> pair_s1, pair_s2, row_first, row_off, col_begin, col_row;
};

// max_blocks: the plan stops at the counts when nblk exceeds it (the caller reports the capacity)
inline void gba_plan_envelope(const LbaIn& in, const LbaPlan& P, const LbaActive& A, long long max_blocks, GbaEnvPlan* E) {
  const int ns = A.nslot;
  E->ns = ns;
  std::vector<uint64_t> keys;
  std::vector<int> slots;
  for (int p = 0; p < in.np; p++) {
    slots.clear();
    for (int e = in.edge_begin[p]; e < in.edge_begin[p + 1]; e++) {
      const int f = P.kf_free[in.e_kf[e]];
      if (f >= 0) slots.push_back(A.slot_of_free[f]);
    }
    for (size_t i = 0; i < slots.size(); i++)
      for (size_t j = 0; j < slots.size(); j++)
        if (slots[i] <= slots[j]) keys.push_back(((uint64_t)slots[j] << 32) | (uint32_t)slots[i]);
    if (keys.size() > (1u << 24)) {  // keep the list short while it is built
      std::sort(keys.begin(), keys.end());
      keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    }
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  E->npair = (long long)keys.size();
  E->row_first.resize(ns);
  for (int s = 0; s < ns; s++) E->row_first[s] = s;
  for (uint64_t k : keys) {
    const int s2 = (int)(k >> 32), s1 = (int)(k & 0xffffffffu);
    if (s1 < E->row_first[s2]) E->row_first[s2] = s1;
  }
  E->nblk = 0;
  for (int s = 0; s < ns; s++) E->nblk += s - E->row_first[s] + 1;
  E->pair_s1.clear(), E->pair_s2.clear(), E->row_off.clear(), E->col_begin.clear(), E->col_row.clear();
  if (E->nblk > max_blocks) return;
  E->pair_s1.resize(keys.size()), E->pair_s2.resize(keys.size());
  for (size_t i = 0; i < keys.size(); i++) E->pair_s2[i] = (int)(keys[i] >> 32), E->pair_s1[i] = (int)(keys[i] & 0xffffffffu);
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

// Optimizer.cc:189-238. B supplies start, begin_round, linearize, trial, accept, finish.
template <class B>
inline int gba_run(B& b, const GbaIn& gin, const LbaPlan& P, const LbaActive& A, const GbaEnvPlan& E, GbaOut* o) {
  const LbaIn& in = gin.l;
  o->tcw.assign(in.tcw, in.tcw + 12 * (size_t)in.nk);
  o->xw.assign(in.xw, in.xw + 3 * (size_t)in.np);
  memset(&o->trace, 0, sizeof(o->trace));
  o->trace.env_blocks = (int32_t)E.nblk, o->trace.schur_blocks = (int32_t)E.npair;
  if (P.nfree == 0 || in.ne == 0) return 0;  // deviation: nothing to optimise, the inputs as bits
  LbaPoller poll = {in.stop_flag, in.stop_at_poll, 0};
  int st = 0;
  if ((st = b.start(P, E))) return st;
  LbaRound r;
  uint32_t flags = 0;
  if ((st = lba_round(b, A, gin.robust != 0, gin.n_iterations, poll, &r, &flags))) return st;
  GbaTrace& t = o->trace;
  t.n_active = r.n_active, t.iterations = r.iterations, t.trials = r.trials, t.rejected_trials = r.rejected_trials;
  t.stop = r.stop, t.lambda = r.lambda, t.chi2 = r.chi2, t.flags = flags, t.polls = poll.polls;
  std::vector<double> T(7 * (size_t)in.nk), X(3 * (size_t)in.np);
  if ((st = b.finish(T.data(), X.data()))) return st;
  for (int i = 0; i < in.nk; i++) {  // :195-212: every keyframe, through toSE3Quat and toCvMat
    double m[9];
    po_quat_to_matrix(&T[7 * (size_t)i], m);
    for (int rr = 0; rr < 3; rr++) {
      for (int c = 0; c < 3; c++) o->tcw[12 * (size_t)i + 4 * rr + c] = (float)m[3 * rr + c];
      o->tcw[12 * (size_t)i + 4 * rr + 3] = (float)T[7 * (size_t)i + 4 + rr];
    }
  }
  for (int p = 0; p < in.np; p++)  // :215-238: vbNotIncludedMP keeps its input
    if (A.p_active[p])
      for (int k = 0; k < 3; k++) o->xw[3 * (size_t)p + k] = (float)X[3 * (size_t)p + k];
  return 0;
}

// The workspace in host memory, every stage a loop over the per-element functions
struct GbaHostBackend {
  GbaWs g;
  LmRec rec;
  LbaActive A;
  std::vector<double> est_T, tri_T, est_X, tri_X, e_err, e_prod, p_hll, p_bl, p_chi, p_dinv, p_db, p_xl, hpp, bp, bs, L, d, y, xp;

  int start(const LbaPlan& plan, const GbaEnvPlan& E) {
    memset(&g, 0, sizeof(g));
    LbaWs& w = g.l;
    const size_t nk = plan.nk, np = plan.np, ne = plan.ne, nf = plan.nfree, n = 6 * (size_t)E.ns;
    est_T = plan.T0, tri_T = plan.T0, est_X = plan.X0, tri_X = plan.X0;
    e_err.assign(3 * ne, 0.0), e_prod.assign(LBA_EDGE_DOUBLES * ne, 0.0);
    p_hll.assign(9 * np, 0.0), p_bl.assign(3 * np, 0.0), p_chi.assign(np, 0.0), p_dinv.assign(9 * np, 0.0);
    p_db.assign(3 * np, 0.0), p_xl.assign(3 * np, 0.0);
    hpp.assign(21 * nf, 0.0), bp.assign(6 * nf, 0.0), bs.assign(n, 0.0), L.assign(36 * (size_t)E.nblk, 0.0);
    d.assign(n, 0.0), y.assign(n, 0.0), xp.assign(n, 0.0);
    w.nk = (int)nk, w.nfree = (int)nf, w.np = (int)np, w.ne = (int)ne;
    w.cam = plan.cam.data(), w.kf_free = plan.kf_free.data(), w.e_pt = plan.e_pt.data(), w.e_obs = plan.e_obs.data();
    w.e_w = plan.e_w.data(), w.e_stereo = plan.e_stereo.data(), w.kl_begin = plan.kl_begin.data(), w.kl_edge = plan.kl_edge.data();
    w.est_T = est_T.data(), w.tri_T = tri_T.data(), w.est_X = est_X.data(), w.tri_X = tri_X.data();
    w.e_err = e_err.data(), w.e_prod = e_prod.data(), w.p_hll = p_hll.data(), w.p_bl = p_bl.data(), w.p_chi = p_chi.data();
    w.p_dinv = p_dinv.data(), w.p_db = p_db.data(), w.p_xl = p_xl.data(), w.hpp = hpp.data(), w.bp = bp.data();
    w.bs = bs.data(), w.d = d.data(), w.y = y.data(), w.xp = xp.data();
    w.edge_begin = plan.edge_begin, w.e_kf = plan.e_kf;
    w.rec = &rec;
    gba_set_deltas(&w);
    g.env = {E.ns, E.row_first.data(), E.row_off.data(), E.col_begin.data(), E.col_row.data(), L.data(), d.data(), y.data()};
    g.npair = (int)E.npair, g.pair_s1 = E.pair_s1.data(), g.pair_s2 = E.pair_s2.data();
    return 0;
  }

  int begin_round(const LbaActive& a, bool kernel_on) {
    A = a;
    LbaWs& w = g.l;
    w.e_active = A.e_active.data(), w.p_active = A.p_active.data();
    w.slot_of_free = A.slot_of_free.data(), w.free_of_slot = A.free_of_slot.data();
    w.nslot = A.nslot, w.kernel_on = kernel_on ? 1 : 0;
    for (double& v : xp) v = 0.0;  // deviation: x is zero before the first successful solve
    for (double& v : p_xl) v = 0.0;
    return 0;
  }

  void tree_reduce(int mode, double lambda, bool trial) {
    const LbaWs& w = g.l;
    for (int e = 0; e < w.ne; e++) trial ? lba_edge<false>(w, e, true) : lba_edge<true>(w, e, false);
    for (int p = 0; p < w.np; p++) trial ? lba_point_sum<false>(w, p) : lba_point_sum<true>(w, p);
    if (!trial)
      for (int s = 0; s < w.nslot; s++) {
        double acc[LBA_LANES][27];
        for (int l = 0; l < LBA_LANES; l++) lba_pose_lane(w, w.free_of_slot[s], l, acc[l]);
        PoHostGroup().reduce(acc);
        lba_pose_finish(w, w.free_of_slot[s], acc[0]);
      }
    double part[LBA_LANES][2];
    for (int l = 0; l < LBA_LANES; l++) lba_reduce_lane(w, l, mode, lambda, part[l]);
    if (!mode) {
      double mx = 0.0;
      for (int l = 0; l < LBA_LANES; l++) mx = part[l][1] > mx ? part[l][1] : mx;
      for (int l = 0; l < LBA_LANES; l++) part[l][1] = 0.0;
      PoHostGroup().reduce(part);
      part[0][1] = mx;
    } else {
      PoHostGroup().reduce(part);
    }
    lba_reduce_finish(w, mode, lambda, part[0][0], part[0][1]);
  }

  int linearize(LmRec* out) {
    memset(&rec, 0, sizeof(rec));
    tree_reduce(0, 0.0, false);
    *out = rec;
    return 0;
  }

  int trial(double lambda, LmRec* out) {
    memset(&rec, 0, sizeof(rec));
    const LbaWs& w = g.l;
    const EnvWs& env = g.env;
    const int ns = env.ns, n = 6 * ns;
    for (int p = 0; p < w.np; p++) lba_point_dinv(w, p, lambda);
    for (double& v : L) v = 0.0;  // blocks without a structural pair are +0.0 before the factorisation
    for (int i = 0; i < g.npair; i++) {
      const int s1 = g.pair_s1[i], s2 = g.pair_s2[i];
      double acc[LBA_LANES][42];
      for (int l = 0; l < LBA_LANES; l++) lba_schur_lane(w, w.free_of_slot[s1], w.free_of_slot[s2], l, acc[l]);
      PoHostGroup().reduce(acc);
      gba_schur_finish(g, s1, s2, lambda, acc[0]);
    }
    // a d_j that is 0, or not finite (deviation), fails the trial
    for (int b = 0; b < ns && !rec.fail; b++) {
      double sD[36];
      const int bad = env_pivot_diag<6>(env, b, sD);
      if (bad) {
        lm_fail(w.rec, bad == 2 ? LM_FLAG_NONFINITE : 0u);
        break;
      }
      const int nr = env.col_begin[b + 1] - env.col_begin[b];
      for (int t = 0; t < 6 * nr; t++) env_scale_row<6>(env, b, t, sD);
      const long long items = env_trailing_items(env, b, 6);
      for (long long t = 0; t < items; t++) env_trailing_item<6>(env, b, t);
    }
    if (!rec.fail) {
      for (int i = 0; i < n; i++) w.y[i] = w.bs[i];
      for (int b = 0; b < ns; b++) {
        env_forward_diag<6>(env, b);
        const int nr = env.col_begin[b + 1] - env.col_begin[b];
        for (int t = 0; t < 6 * nr; t++) env_forward_row<6>(env, b, t);
      }
      for (int i = 0; i < n; i++) w.y[i] = w.y[i] / w.d[i];
      for (int s = ns - 1; s >= 0; s--) {
        env_backward_diag<6>(env, s);
        for (int t = 0; t < 6 * (s - env.row_first[s]); t++) env_backward_col<6>(env, s, t);
      }
      for (int i = 0; i < n; i++) w.xp[i] = w.y[i];
      for (int p = 0; p < w.np; p++) lba_point_backsub(w, p);
    }
    for (int p = 0; p < w.np; p++) lba_update_point(w, p);
    for (int k = 0; k < w.nk; k++) lba_update_kf(w, k);
    const int fail = rec.fail;
    const uint32_t fl = rec.flags;
    tree_reduce(1, lambda, true);
    rec.fail = fail, rec.flags = fl;
    *out = rec;
    return 0;
  }

  int accept() {
    est_T.swap(tri_T), est_X.swap(tri_X);
    LbaWs& w = g.l;
    w.est_T = est_T.data(), w.tri_T = tri_T.data(), w.est_X = est_X.data(), w.tri_X = tri_X.data();
    return 0;
  }

  int finish(double* T, double* X) {
    memcpy(T, est_T.data(), 8 * est_T.size());
    memcpy(X, est_X.data(), 8 * est_X.size());
    return 0;
  }
};
