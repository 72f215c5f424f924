// orbfe_gba_core.h -- Optimizer::BundleAdjustment's arithmetic (Optimizer.cc:51-240) on top of
// orbfe_lba_core.h and orbfe_env_core.h: the BA edges, Huber, the per-point and per-pose sums, Dinv, the
// Schur lanes, the back-substitution, the update, the reduction, the Levenberg round and the host backend's
// base are the former's, unchanged; the block envelope, its structure pass, its LDL^T and its two
// substitutions are the latter's, at block dimension 6. New here: the plan of the reduced system as an
// envelope over the covisible keyframe pairs, the Schur blocks written into it, GbaHostBackend's trial and
// gba_run (one optimize(nIterations), every keyframe written out). Used by orbfe_gba.hip and
// tests/cpp/gba_core_main.cpp; tests/gba_ref.py is the same code in Python. Not part of the C ABI. Every
// operation is an IEEE double + - * / sqrt, rounded separately.
//
// The envelope: slot s is the s-th free keyframe with an edge; row_first[s] is the
// smallest slot that shares a point with s. Inside the envelope the factorisation is orbfe_lba_core.h's
// dense lba_ldlt_dot, outside every entry is an exact zero. Every loop is capped by a count of the plan;
// every index read from memory was built by gba_plan_envelope or checked by orbfe_gba_solve.
#pragma once
#include "orbfe_env_core.h"
#include "orbfe_lba_core.h"

#include <algorithm>

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
struct GbaEnvPlan : EnvPlan {  // ns, nblk, row_first, row_off, col_begin, col_row
  long long npair = 0;
  std::vector<int> pair_s1, pair_s2;
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
  E->pair_s1.clear(), E->pair_s2.clear();
  env_plan_structure(E, max_blocks);
  if (E->nblk > max_blocks) return;
  E->pair_s1.resize(keys.size()), E->pair_s2.resize(keys.size());
  for (size_t i = 0; i < keys.size(); i++) E->pair_s2[i] = (int)(keys[i] >> 32), E->pair_s1[i] = (int)(keys[i] & 0xffffffffu);
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
  for (int i = 0; i < in.nk; i++) lba_pose_out(&T[7 * (size_t)i], &o->tcw[12 * (size_t)i]);  // :195-212: every keyframe
  for (int p = 0; p < in.np; p++)  // :215-238: vbNotIncludedMP keeps its input
    if (A.p_active[p])
      for (int k = 0; k < 3; k++) o->xw[3 * (size_t)p + k] = (float)X[3 * (size_t)p + k];
  return 0;
}

// BaHostBackend with the envelope as the reduced system
struct GbaHostBackend : BaHostBackend {
  GbaWs g;  // g.l is a copy of w, taken per trial
  std::vector<double> L;

  int start(const LbaPlan& plan, const GbaEnvPlan& E) {
    BaHostBackend::start(plan, 6 * (size_t)E.ns);
    gba_set_deltas(&w);
    L.assign(36 * (size_t)E.nblk, 0.0);
    g.env = {E.ns, E.row_first.data(), E.row_off.data(), E.col_begin.data(), E.col_row.data(), L.data(), d.data(), y.data()};
    g.npair = (int)E.npair, g.pair_s1 = E.pair_s1.data(), g.pair_s2 = E.pair_s2.data();
    return 0;
  }

  int trial(double lambda, LmRec* out) {
    memset(&rec, 0, sizeof(rec));
    g.l = w;
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
      for (int t = 0; t < 6 * nr; t++) env_scale_row<6>(env, b, t, sD, env.d + 6 * b);
      const long long items = env_trailing_items(env, b, 6);
      for (long long t = 0; t < items; t++) env_trailing_item<6>(env, b, t, env.d + 6 * b);
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
    }
    return trial_tail(lambda, out);
  }
};
