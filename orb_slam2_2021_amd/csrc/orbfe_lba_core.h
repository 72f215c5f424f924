// orbfe_lba_core.h -- Optimizer::LocalBundleAdjustment's arithmetic (Optimizer.cc:508-781 and the g2o
// routines under it: the two BA edges of types_six_dof_expmap, BaseBinaryEdge::constructQuadraticForm,
// RobustKernelHuber, BlockSolver_6_3's buildSystem / setLambda / restoreDiagonal / Schur solve,
// OptimizationAlgorithmLevenberg, SparseOptimizer's optimize / push / pop / update) as host/device
// inline functions over one workspace of plain arrays (LbaWs). The kernels of orbfe_lba.hip call the
// per-element functions with one thread, or one wavefront lane, each; LbaHostBackend below loops the same
// functions on the host; lba_run is the two rounds over orbfe_lm_core.h's Levenberg driver
// (lm_host_optimize), on the host for both. Used by orbfe_lba.hip and tests/cpp/lba_core_main.cpp;
// tests/lba_ref.py is the same code in Python. Not part of the C ABI. The SE3 rules, po_sincos and the
// "EIGEN:" readings of orbfe_poseopt_core.h are reused; the flag and stop codes, the record (LmRec), the
// host group and po_finite are orbfe_lm_core.h's. Every operation is an IEEE double + - * / sqrt, rounded
// separately (-ffp-contract=off).
//
// Summation (the rule that defines the numbers):
//   per point   Hll, bl, cl and the point's share of the robust chi2 run over the point's active edges
//               in the caller's edge order, from +0.0;
//   over points point p belongs to lane p % 64; a lane adds its terms in ascending p from +0.0, absent
//               terms skipped; the lanes are combined by s[l] += s[l + stride], stride = 32 .. 1. This
//               is Hpp(i,i), bp_i, a Schur block's sum, bschur's sum, the total chi2 and the points'
//               part of computeScale.
// Every loop is capped by a count the host has checked; every index read from memory was checked by the
// host (orbfe_lba_solve) or built by it (lba_plan).
#pragma once
#include "orbfe_lm_core.h"
#include "orbfe_poseopt_core.h"  // SE3: PoSE3, po_se3_*, po_quat_to_matrix

#include <cstring>
#include <vector>

#define LBA_LANES 64
#define LBA_MAX_FREE 128
#define LBA_EDGE_DOUBLES 58 /* per-edge products: rho0, Hll 9, bl 3, Hpl 18, Hpp 21 (r <= c), bp 6 (e_prod) */
static_assert(LBA_EDGE_DOUBLES == 1 + 9 + 3 + 18 + 21 + 6, "e_prod layout");

struct LbaRound {
  int32_t n_active, iterations, trials, rejected_trials, stop, n_flagged;
  double lambda, chi2;
};

struct LbaWs {
  int nk, nfree, np, ne, nslot, kernel_on;
  double delta_mono, delta_stereo;  // RobustKernelHuber's deltas (lba_set_deltas; orbfe_gba_core.h sets its own)
  // the problem, widened to double
  const double* cam;        // [nk * 5] fx fy cx cy bf
  const int* kf_free;       // [nk] index among the free keyframes, or -1
  const int* edge_begin;    // [np + 1]
  const int* e_kf;          // [ne]
  const int* e_pt;          // [ne]
  const double* e_obs;      // [ne * 3] u v uR
  const double* e_w;        // [ne] invSigma2
  const uint8_t* e_stereo;  // [ne]
  const int* kl_begin;      // [nfree * 64 + 1]: free keyframe f's edges whose point is in lane l ...
  const int* kl_edge;       // ... in ascending point order
  // the active set of the round (level-0 edges and the vertices they touch)
  const uint8_t* e_active;  // [ne]
  const uint8_t* p_active;  // [np]
  const int* slot_of_free;  // [nfree] position in the reduced system, or -1
  const int* free_of_slot;  // [nslot]
  // estimates: accepted and trial
  double *est_T, *tri_T;  // [nk * 7] q (x y z w), t
  double *est_X, *tri_X;  // [np * 3]
  // per edge
  double* e_err;   // [ne * 3] _error of the last computeActiveErrors that covered the edge
  double* e_prod;  // [ne * LBA_EDGE_DOUBLES]
  // per point
  double* p_hll;   // [np * 9]
  double* p_bl;    // [np * 3]
  double* p_chi;   // [np]
  double* p_dinv;  // [np * 9]
  double* p_db;    // [np * 3]
  double* p_xl;    // [np * 3]
  // per free keyframe and the reduced system (n = 6 nslot)
  double* hpp;  // [nfree * 21] r <= c, row-major
  double* bp;   // [nfree * 6]
  double* S;    // [n * n] row-major, the upper triangle is read
  double* bs;   // [n]
  double* Lm;   // [n * n] Lm[k * n + i] = L_ik
  double* Mm;   // [n * n] Mm[k * n + i] = L_ik * d_k
  double* d;    // [n]
  double* y;    // [n]
  double* xp;   // [nfree * 6] by slot
  LmRec* rec;
};

PO_HD inline int lba_upper(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }  // r <= c

PO_HD inline void lba_load_T(const double* a, PoSE3* T) {
  for (int k = 0; k < 4; k++) T->q[k] = a[k];
  for (int k = 0; k < 3; k++) T->t[k] = a[4 + k];
}

PO_HD inline void lba_store_T(const PoSE3& T, double* a) {
  for (int k = 0; k < 4; k++) a[k] = T.q[k];
  for (int k = 0; k < 3; k++) a[4 + k] = T.t[k];
}

// computeError of EdgeSE3ProjectXYZ (project2d divides in double) and EdgeStereoSE3ProjectXYZ (const float
// invz = 1.0f / z: divided in double, narrowed): obs - cam_project(T.map(Xw))
PO_HD inline void lba_edge_error(const double* cam, bool stereo, const double* obs, const double* p, double* err) {
  if (stereo) {
    const double invz = (double)(float)(1.0 / p[2]);
    const double r0 = p[0] * invz * cam[0] + cam[2];
    const double r1 = p[1] * invz * cam[1] + cam[3];
    const double r2 = r0 - cam[4] * invz;
    err[0] = obs[0] - r0, err[1] = obs[1] - r1, err[2] = obs[2] - r2;
  } else {
    const double r0 = p[0] / p[2] * cam[0] + cam[2];
    const double r1 = p[1] / p[2] * cam[1] + cam[3];
    err[0] = obs[0] - r0, err[1] = obs[1] - r1, err[2] = 0.0;
  }
}

// EIGEN: _error.dot(information() * _error) with a diagonal information
PO_HD inline double lba_chi2(double wt, bool stereo, const double* err) {
  double s = err[0] * (wt * err[0]) + err[1] * (wt * err[1]);
  if (stereo) s = s + err[2] * (wt * err[2]);
  return s;
}

// linearizeOplus of the two BA edges, as written (types_six_dof_expmap.cpp:103-139, :188-234): divisions
// by z and z_2, not products with 1/z. A: rows of 3 (the point, vertex 0), B: rows of 6 (the pose).
// EIGEN: the mono _jacobianOplusXi = -1./z * tmp * R evaluates (-1./z * tmp) entry by entry, then the
// 2x3 * 3x3 product with k ascending, the zero entries of tmp included.
PO_HD inline void lba_jacobians(const double* cam, bool stereo, const double* q, const double* p, double* A, double* B) {
  const double fx = cam[0], fy = cam[1], bf = cam[4];
  const double x = p[0], y = p[1], z = p[2];
  const double z_2 = z * z;
  double R[9];
  po_quat_to_matrix(q, R);
  if (stereo) {
    for (int c = 0; c < 3; c++) {
      A[c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
      A[3 + c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
      A[6 + c] = A[c] - bf * R[6 + c] / z_2;
    }
  } else {
    const double s = -1. / z;
    const double t[6] = {s * fx, s * 0.0, s * (-x / z * fx), s * 0.0, s * fy, s * (-y / z * fy)};
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < 3; c++) A[3 * r + c] = (t[3 * r] * R[c] + t[3 * r + 1] * R[3 + c]) + t[3 * r + 2] * R[6 + c];
    A[6] = A[7] = A[8] = 0.0;
  }
  B[0] = x * y / z_2 * fx;
  B[1] = -(1 + (x * x / z_2)) * fx;
  B[2] = y / z * fx;
  B[3] = -1. / z * fx;
  B[4] = 0.0;
  B[5] = x / z_2 * fx;
  B[6] = (1 + y * y / z_2) * fy;
  B[7] = -x * y / z_2 * fy;
  B[8] = -x / z * fy;
  B[9] = 0.0;
  B[10] = -1. / z * fy;
  B[11] = y / z_2 * fy;
  if (stereo) {
    B[12] = B[0] - bf * y / z_2;
    B[13] = B[1] + bf * x / z_2;
    B[14] = B[2];
    B[15] = B[3];
    B[16] = 0.0;
    B[17] = B[5] - bf / z_2;
  } else {
    for (int c = 0; c < 6; c++) B[12 + c] = 0.0;
  }
}

PO_HD inline void lba_huber(double chi2, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  *rho0 = chi2, *rho1 = 1.0;
  if (!(chi2 <= dsqr)) {  // RobustKernelHuber::robustify
    const double sq = sqrt(chi2);
    *rho0 = 2 * sq * delta - dsqr;
    *rho1 = delta / sq;
  }
}

// computeError (+ the robust chi2 term) of one active edge at the accepted or the trial estimates and,
// with FULL, linearizeOplus + constructQuadraticForm into the edge's own products.
// EIGEN: omega_r = -(w e_k), times rho1 under a kernel; weightedOmega = rho1 w;
//   b_c += sum_k J_kc omega_r[k];  H_ab += sum_k (J_ka ww) J_kb;  Hpl_rc = sum_k (A_kc ww) B_kr
// (sum_k is k = 0, 1 and, for a stereo edge, 2, left to right).
template <bool FULL>
PO_HD inline void lba_edge(const LbaWs& w, int e, bool trial) {
  if (!w.e_active[e]) return;
  const int kf = w.e_kf[e], pt = w.e_pt[e];
  PoSE3 T;
  lba_load_T((trial ? w.tri_T : w.est_T) + 7 * (size_t)kf, &T);
  const double* X = (trial ? w.tri_X : w.est_X) + 3 * (size_t)pt;
  const double* cam = w.cam + 5 * (size_t)kf;
  const bool stereo = w.e_stereo[e] != 0;
  const double wt = w.e_w[e];
  double p[3], err[3];
  po_se3_map(T, X, p);
  lba_edge_error(cam, stereo, w.e_obs + 3 * (size_t)e, p, err);
  for (int k = 0; k < 3; k++) w.e_err[3 * (size_t)e + k] = err[k];
  const double chi2 = lba_chi2(wt, stereo, err);
  double rho0 = chi2, rho1 = 1.0;
  if (w.kernel_on) lba_huber(chi2, stereo ? w.delta_stereo : w.delta_mono, &rho0, &rho1);
  double* o = w.e_prod + LBA_EDGE_DOUBLES * (size_t)e;
  o[0] = rho0;
  if (!FULL) return;
  double A[9], B[18];
  lba_jacobians(cam, stereo, T.q, p, A, B);
  const int D = stereo ? 3 : 2;
  const double ww = w.kernel_on ? rho1 * wt : wt;
  double om[3];
  for (int k = 0; k < 3; k++) om[k] = w.kernel_on ? (-(wt * err[k])) * rho1 : -(wt * err[k]);
  double* hll = o + 1;
  double* bl = o + 10;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double s = A[a] * om[0];
    for (int k = 1; k < 3; k++)
        if (k < D) s = s + A[3 * k + a] * om[k];
    bl[a] = s;
#pragma unroll
    for (int b = 0; b < 3; b++) {
      double h = (A[a] * ww) * A[b];
      for (int k = 1; k < 3; k++)
        if (k < D) h = h + (A[3 * k + a] * ww) * A[3 * k + b];
      hll[3 * a + b] = h;
    }
  }
  if (w.kf_free[kf] < 0) return;  // a fixed keyframe: the point's Hll and b only
  double* hpl = o + 13;
  double* hpp = o + 31;
  double* bp = o + 52;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double s = B[r] * om[0];
    for (int k = 1; k < 3; k++)
        if (k < D) s = s + B[6 * k + r] * om[k];
    bp[r] = s;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double h = (A[c] * ww) * B[r];
      for (int k = 1; k < 3; k++)
        if (k < D) h = h + (A[3 * k + c] * ww) * B[6 * k + r];
      hpl[3 * r + c] = h;
    }
#pragma unroll
    for (int c = r; c < 6; c++) {
      double h = (B[r] * ww) * B[c];
      for (int k = 1; k < 3; k++)
        if (k < D) h = h + (B[6 * k + r] * ww) * B[6 * k + c];
      hpp[lba_upper(r, c)] = h;
    }
  }
}

// A point's Hll, bl and share of the robust chi2 over its active edges, in edge order
template <bool FULL>
PO_HD inline void lba_point_sum(const LbaWs& w, int p) {
  if (!w.p_active[p]) return;
  double chi = 0.0, h[9], b[3];
  for (int k = 0; k < 9; k++) h[k] = 0.0;
  for (int k = 0; k < 3; k++) b[k] = 0.0;
  for (int e = w.edge_begin[p]; e < w.edge_begin[p + 1]; e++) {
    if (!w.e_active[e]) continue;
    const double* o = w.e_prod + LBA_EDGE_DOUBLES * (size_t)e;
    chi = chi + o[0];
    if (FULL) {
      for (int k = 0; k < 9; k++) h[k] = h[k] + o[1 + k];
      for (int k = 0; k < 3; k++) b[k] = b[k] + o[10 + k];
    }
  }
  w.p_chi[p] = chi;
  if (FULL) {
    for (int k = 0; k < 9; k++) w.p_hll[9 * (size_t)p + k] = h[k];
    for (int k = 0; k < 3; k++) w.p_bl[3 * (size_t)p + k] = b[k];
  }
}

// One lane's part of Hpp(f,f) (21) and bp_f (6) over the free keyframe's active edges
PO_HD inline void lba_pose_lane(const LbaWs& w, int f, int lane, double* acc) {
  for (int k = 0; k < 27; k++) acc[k] = 0.0;
  for (int i = w.kl_begin[f * LBA_LANES + lane]; i < w.kl_begin[f * LBA_LANES + lane + 1]; i++) {
    const int e = w.kl_edge[i];
    if (!w.e_active[e]) continue;
    const double* o = w.e_prod + LBA_EDGE_DOUBLES * (size_t)e + 31;
    for (int k = 0; k < 27; k++) acc[k] = acc[k] + o[k];
  }
}

PO_HD inline void lba_pose_finish(const LbaWs& w, int f, const double* acc) {
  for (int k = 0; k < 21; k++) w.hpp[21 * f + k] = acc[k];
  for (int k = 0; k < 6; k++) w.bp[6 * f + k] = acc[21 + k];
}

// EIGEN: Matrix3d::inverse(): the cofactors times 1 / det, det = (c00 m00 + c10 m10) + c20 m20 over the
// first column's cofactors; no singularity test. Dinv = (Hll + lambda I)^-1, db = Dinv bl.
PO_HD inline void lba_inverse3(const double* m, double* inv) {
  double cf[9];  // cf[3 i + j] = cofactor<i, j>
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cf[3 * i + j] = m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
    }
  const double det = (cf[0] * m[0] + cf[3] * m[3]) + cf[6] * m[6];
  const double invdet = 1.0 / det;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) inv[3 * j + i] = cf[3 * i + j] * invdet;
}

PO_HD inline void lba_point_dinv(const LbaWs& w, int p, double lambda) {
  if (!w.p_active[p]) return;
  double m[9], inv[9];
  for (int k = 0; k < 9; k++) m[k] = w.p_hll[9 * (size_t)p + k];
  m[0] = m[0] + lambda, m[4] = m[4] + lambda, m[8] = m[8] + lambda;
  lba_inverse3(m, inv);
  bool ok = true;
  for (int k = 0; k < 9; k++) {
    w.p_dinv[9 * (size_t)p + k] = inv[k];
    ok = ok && po_finite(inv[k]);
  }
  const double* b = w.p_bl + 3 * (size_t)p;
  for (int r = 0; r < 3; r++) w.p_db[3 * (size_t)p + r] = (inv[3 * r] * b[0] + inv[3 * r + 1] * b[1]) + inv[3 * r + 2] * b[2];
  if (!ok) lm_fail(w.rec, LM_FLAG_NONFINITE);  // deviation: a non-finite Dinv fails the trial
}

// One lane's part of sum_p (B_f1 Dinv) B_f2^T (36) and, on the diagonal, of sum_p B_f db (6): the points
// both keyframes see through active edges, by a merge of the two lists (each ascending in p)
PO_HD inline void lba_schur_lane(const LbaWs& w, int f1, int f2, int lane, double* acc) {
  for (int k = 0; k < 42; k++) acc[k] = 0.0;
  int ia = w.kl_begin[f1 * LBA_LANES + lane], ib = w.kl_begin[f2 * LBA_LANES + lane];
  const int ea = w.kl_begin[f1 * LBA_LANES + lane + 1], eb = w.kl_begin[f2 * LBA_LANES + lane + 1];
  while (ia < ea && ib < eb) {  // at most (ea - ia) + (eb - ib) steps
    const int e1 = w.kl_edge[ia], e2 = w.kl_edge[ib];
    const int p1 = w.e_pt[e1], p2 = w.e_pt[e2];
    if (p1 < p2) {
      ia++;
      continue;
    }
    if (p2 < p1) {
      ib++;
      continue;
    }
    ia++, ib++;
    if (!w.e_active[e1] || !w.e_active[e2]) continue;
    const double* B1 = w.e_prod + LBA_EDGE_DOUBLES * (size_t)e1 + 13;
    const double* B2 = w.e_prod + LBA_EDGE_DOUBLES * (size_t)e2 + 13;
    const double* Di = w.p_dinv + 9 * (size_t)p1;
    for (int r = 0; r < 6; r++) {
      double bd[3];
      for (int c = 0; c < 3; c++) bd[c] = (B1[3 * r] * Di[c] + B1[3 * r + 1] * Di[3 + c]) + B1[3 * r + 2] * Di[6 + c];
      for (int c = 0; c < 6; c++)
        acc[6 * r + c] = acc[6 * r + c] + ((bd[0] * B2[3 * c] + bd[1] * B2[3 * c + 1]) + bd[2] * B2[3 * c + 2]);
    }
    if (f1 == f2) {
      const double* db = w.p_db + 3 * (size_t)p1;
      for (int r = 0; r < 6; r++) acc[36 + r] = acc[36 + r] + ((B1[3 * r] * db[0] + B1[3 * r + 1] * db[1]) + B1[3 * r + 2] * db[2]);
    }
  }
}

// S(s1,s2) = (Hpp + lambda on the diagonal) - C, formed once; bschur = bp - sum. Of a diagonal block only
// r <= c is read later, and checked here. Deviation: a non-finite entry fails the trial.
PO_HD inline void lba_schur_finish(const LbaWs& w, int s1, int s2, double lambda, const double* acc) {
  const int n = 6 * w.nslot;
  const int f1 = w.free_of_slot[s1];
  bool ok = true;
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double h = 0.0;
      if (s1 == s2 && r <= c) h = w.hpp[21 * f1 + lba_upper(r, c)];
      if (s1 == s2 && r == c) h = h + lambda;
      const double v = h - acc[6 * r + c];
      w.S[(size_t)(6 * s1 + r) * n + 6 * s2 + c] = v;
      if (s1 != s2 || r <= c) ok = ok && po_finite(v);
    }
  if (s1 == s2)
    for (int r = 0; r < 6; r++) {
      const double v = w.bp[6 * f1 + r] - acc[36 + r];
      w.bs[6 * s1 + r] = v;
      ok = ok && po_finite(v);
    }
  if (!ok) lm_fail(w.rec, LM_FLAG_NONFINITE);
}

// Deviation: the dense, unpivoted LDL^T in natural order that stands for LinearSolverEigen's sparse
// SimplicialLDLT. Element (i, j), i >= j, of the factorisation before the division by d_j:
// v = A_ij (read from the upper triangle); v = v - (L_ik d_k) L_jk for k ascending.
PO_HD inline double lba_ldlt_dot(const LbaWs& w, int n, int i, int j) {
  double v = w.S[(size_t)j * n + i];
  for (int k = 0; k < j; k++) v = v - w.Mm[(size_t)k * n + i] * w.Lm[(size_t)k * n + j];
  return v;
}

// cl = bl + sum_j B_j^T (-xp_j) over the point's active edges to free keyframes, in edge order
// (EIGEN: dest_c += sum_r B_rc src_r, r ascending); xl = Dinv cl. Only after a successful pose solve.
PO_HD inline void lba_point_backsub(const LbaWs& w, int p) {
  if (!w.p_active[p]) return;
  double cl[3];
  for (int k = 0; k < 3; k++) cl[k] = w.p_bl[3 * (size_t)p + k];
  for (int e = w.edge_begin[p]; e < w.edge_begin[p + 1]; e++) {
    if (!w.e_active[e]) continue;
    const int f = w.kf_free[w.e_kf[e]];
    if (f < 0) continue;
    const double* B = w.e_prod + LBA_EDGE_DOUBLES * (size_t)e + 13;
    const double* x = w.xp + 6 * w.slot_of_free[f];
    for (int c = 0; c < 3; c++) {
      double s = B[c] * -x[0];
      for (int r = 1; r < 6; r++) s = s + B[3 * r + c] * -x[r];
      cl[c] = cl[c] + s;
    }
  }
  const double* Di = w.p_dinv + 9 * (size_t)p;
  for (int r = 0; r < 3; r++) w.p_xl[3 * (size_t)p + r] = (Di[3 * r] * cl[0] + Di[3 * r + 1] * cl[1]) + Di[3 * r + 2] * cl[2];
}

// SparseOptimizer::update into the trial estimates: += for an active point, exp(x) * T for an active free
// keyframe; every other vertex's trial estimate is its accepted one (push / pop never touch it).
PO_HD inline void lba_update_point(const LbaWs& w, int p) {
  for (int k = 0; k < 3; k++) {
    const double v = w.est_X[3 * (size_t)p + k];
    w.tri_X[3 * (size_t)p + k] = w.p_active[p] ? v + w.p_xl[3 * (size_t)p + k] : v;
  }
}

PO_HD inline void lba_update_kf(const LbaWs& w, int kf) {
  PoSE3 T, d, o;
  lba_load_T(w.est_T + 7 * (size_t)kf, &T);
  const int f = w.kf_free[kf];
  const int s = f < 0 ? -1 : w.slot_of_free[f];
  if (s < 0) {
    lba_store_T(T, w.tri_T + 7 * (size_t)kf);
    return;
  }
  unsigned flags = 0;
  po_se3_exp(w.xp + 6 * s, &d, &flags);
  po_se3_mul(d, T, &o);
  lba_store_T(o, w.tri_T + 7 * (size_t)kf);
  lm_or(&w.rec->flags, flags);
}

// One lane's part of the sums over points: out[0] the robust chi2, out[1] computeScale's point partials
// (mode 1: x_j (lambda x_j + b_j) per vertex from +0.0) or max |Hll_jj| (mode 0, computeLambdaInit)
PO_HD inline void lba_reduce_lane(const LbaWs& w, int lane, int mode, double lambda, double* out) {
  double chi = 0.0, sc = 0.0;
  for (int p = lane; p < w.np; p += LBA_LANES) {
    if (!w.p_active[p]) continue;
    chi = chi + w.p_chi[p];
    if (mode) {
      double s = 0.0;
      for (int j = 0; j < 3; j++) {
        const double x = w.p_xl[3 * (size_t)p + j];
        s = s + x * (lambda * x + w.p_bl[3 * (size_t)p + j]);
      }
      sc = sc + s;
    } else {
      for (int j = 0; j < 3; j++) {
        const double a = fabs(w.p_hll[9 * (size_t)p + 4 * j]);
        sc = a > sc ? a : sc;  // std::max(fabs(H_jj), maxDiagonal); deviation: a NaN entry is skipped
      }
    }
  }
  out[0] = chi, out[1] = sc;
}

// lane 0 after the tree (the sums) or the maximum over the lanes: adds the poses' part
PO_HD inline void lba_reduce_finish(const LbaWs& w, int mode, double lambda, double chi, double pts) {
  w.rec->chi = chi;
  if (mode) {
    double poses = 0.0;
    for (int s = 0; s < w.nslot; s++) {
      const int f = w.free_of_slot[s];
      double v = 0.0;
      for (int j = 0; j < 6; j++) {
        const double x = w.xp[6 * s + j];
        v = v + x * (lambda * x + w.bp[6 * f + j]);
      }
      poses = poses + v;
    }
    w.rec->scale = poses + pts;
  } else {
    double mx = pts;
    for (int s = 0; s < w.nslot; s++) {
      const int f = w.free_of_slot[s];
      for (int j = 0; j < 6; j++) {
        const double a = fabs(w.hpp[21 * f + lba_upper(j, j)]);
        mx = a > mx ? a : mx;
      }
    }
    w.rec->maxdiag = mx;
  }
}

// Optimizer.cc:683 / :726: chi2() of the stored error (double, compared with the double literals by >, so
// a NaN chi2 keeps the edge) || !isDepthPositive() at the current estimates
PO_HD inline bool lba_edge_flag(const LbaWs& w, int e) {
  const bool stereo = w.e_stereo[e] != 0;
  const double chi2 = lba_chi2(w.e_w[e], stereo, w.e_err + 3 * (size_t)e);
  PoSE3 T;
  lba_load_T(w.est_T + 7 * (size_t)w.e_kf[e], &T);
  double p[3];
  po_se3_map(T, w.est_X + 3 * (size_t)w.e_pt[e], p);
  return chi2 > (stereo ? 7.815 : 5.991) || !(p[2] > 0.0);
}

// Optimizer.cc:520-521: const float thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815)
inline void lba_set_deltas(LbaWs* w) { w->delta_mono = (double)(float)sqrt(5.991), w->delta_stereo = (double)(float)sqrt(7.815); }

// ---- the host side: the plan, the Levenberg control flow, the host backend -------------------------
struct LbaIn {
  int nk, np, ne;
  const float* tcw;          // [nk * 12]
  const float* k;            // [nk * 4]
  const float* bf;           // [nk]
  const uint8_t* fixed;      // [nk]
  const float* xw;           // [np * 3]
  const int* edge_begin;     // [np + 1]
  const int* e_kf;           // [ne]
  const float* kp;           // [ne * 2]
  const float* ur;           // [ne]
  const float* is2;          // [ne]
  const volatile int* stop_flag;
  int stop_at_poll;
};

struct LbaOut {
  std::vector<float> tcw, xw;
  std::vector<uint8_t> erase, level1;
  int n_erase = 0, rounds_run = 0, polls = 0;
  uint32_t flags = 0;
  LbaRound rounds[2];
};

// The problem widened to double and the by-keyframe lists. The indices of `in` are checked by the caller.
struct LbaPlan {
  int nk = 0, nfree = 0, np = 0, ne = 0;
  std::vector<double> cam, e_obs, e_w, T0, X0;
  std::vector<int> kf_free, e_pt, kl_begin, kl_edge;
  std::vector<uint8_t> e_stereo;
  const int *edge_begin = nullptr, *e_kf = nullptr;  // the caller's arrays
};

inline void lba_plan(const LbaIn& in, LbaPlan* P) {
  P->nk = in.nk, P->np = in.np, P->ne = in.ne, P->nfree = 0;
  P->edge_begin = in.edge_begin, P->e_kf = in.e_kf;
  P->cam.resize(5 * (size_t)in.nk), P->T0.resize(7 * (size_t)in.nk), P->kf_free.resize(in.nk);
  for (int i = 0; i < in.nk; i++) {
    for (int k = 0; k < 4; k++) P->cam[5 * i + k] = (double)in.k[4 * i + k];
    P->cam[5 * i + 4] = (double)in.bf[i];
    PoSE3 T;
    po_se3_from_tcw(in.tcw + 12 * i, &T);
    lba_store_T(T, &P->T0[7 * (size_t)i]);
    P->kf_free[i] = in.fixed[i] ? -1 : P->nfree++;
  }
  P->X0.resize(3 * (size_t)in.np);
  for (size_t i = 0; i < 3 * (size_t)in.np; i++) P->X0[i] = (double)in.xw[i];
  P->e_obs.resize(3 * (size_t)in.ne), P->e_w.resize(in.ne), P->e_pt.resize(in.ne), P->e_stereo.resize(in.ne);
  std::vector<int> count((size_t)P->nfree * LBA_LANES + 1, 0);
  for (int p = 0; p < in.np; p++)
    for (int e = in.edge_begin[p]; e < in.edge_begin[p + 1]; e++) {
      P->e_pt[e] = p;
      P->e_stereo[e] = !(in.ur[e] < 0);  // mvuRight < 0: monocular
      P->e_obs[3 * (size_t)e] = (double)in.kp[2 * (size_t)e], P->e_obs[3 * (size_t)e + 1] = (double)in.kp[2 * (size_t)e + 1];
      P->e_obs[3 * (size_t)e + 2] = (double)in.ur[e];
      P->e_w[e] = (double)in.is2[e];
      const int f = P->kf_free[in.e_kf[e]];
      if (f >= 0) count[(size_t)f * LBA_LANES + p % LBA_LANES + 1]++;
    }
  for (size_t i = 1; i < count.size(); i++) count[i] += count[i - 1];
  P->kl_begin = count;
  P->kl_edge.assign(count.back(), 0);
  std::vector<int> at(count.begin(), count.end() - 1);
  for (int p = 0; p < in.np; p++)
    for (int e = in.edge_begin[p]; e < in.edge_begin[p + 1]; e++) {
      const int f = P->kf_free[in.e_kf[e]];
      if (f >= 0) P->kl_edge[at[(size_t)f * LBA_LANES + p % LBA_LANES]++] = e;
    }
}

// The level-0 edges' vertices (SparseOptimizer::initializeOptimization(level)): a point or a free keyframe
// without an active edge is not in the system.
struct LbaActive {
  std::vector<uint8_t> e_active, p_active;
  std::vector<int> slot_of_free, free_of_slot;
  int nslot = 0, n_edges = 0;
};

inline void lba_active(const LbaIn& in, const LbaPlan& P, const uint8_t* level1, LbaActive* A) {
  A->e_active.assign(in.ne, 0), A->p_active.assign(in.np, 0);
  A->slot_of_free.assign(P.nfree, -1), A->free_of_slot.clear();
  std::vector<uint8_t> used(P.nfree, 0);
  A->n_edges = 0;
  for (int e = 0; e < in.ne; e++) {
    if (level1 && level1[e]) continue;
    A->e_active[e] = 1, A->n_edges++;
    A->p_active[P.e_pt[e]] = 1;
    if (P.kf_free[in.e_kf[e]] >= 0) used[P.kf_free[in.e_kf[e]]] = 1;
  }
  for (int f = 0; f < P.nfree; f++)
    if (used[f]) A->slot_of_free[f] = (int)A->free_of_slot.size(), A->free_of_slot.push_back(f);
  A->nslot = (int)A->free_of_slot.size();
}

struct LbaPoller {
  const volatile int* flag;
  int at, polls;
  bool operator()() {
    const int k = polls++;
    if (at >= 0 && k >= at) return true;
    return flag && *flag;
  }
};

// One round: SparseOptimizer::optimize(max_it) by orbfe_lm_core.h's lm_host_optimize, lambda from the
// diagonal. A backend B supplies begin_round, linearize, trial, accept; each returns 0 or an error status
// that ends the run.
template <class B>
inline int lba_round(B& b, const LbaActive& A, bool kernel_on, int max_it, LbaPoller& poll, LbaRound* tr, uint32_t* flags) {
  LbaRound r = {A.n_edges, 0, 0, 0, LM_STOP_NO_EDGE, 0, 0.0, 0.0};
  if (A.n_edges > 0) {  // else _ivMap.size() == 0: optimize() returns -1 without a step
    int st = 0;
    LmTrace t;
    if ((st = b.begin_round(A, kernel_on))) return st;
    if ((st = lm_host_optimize(b, max_it, 0.0, poll, &t))) return st;
    r.iterations = t.iterations, r.trials = t.trials, r.rejected_trials = t.rejected_trials, r.stop = t.stop;
    r.lambda = t.lambda, r.chi2 = t.chi2;
    *flags |= t.flags;
  }
  *tr = r;
  return 0;
}

// A keyframe's state q (x y z w), t as the 12 floats of Tcw: to_homogeneous_matrix, narrowed by
// Converter::toCvMat. Which keyframes are written out is each caller's rule.
inline void lba_pose_out(const double* T, float* tcw) {
  double m[9];
  po_quat_to_matrix(T, m);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) tcw[4 * r + c] = (float)m[3 * r + c];
    tcw[4 * r + 3] = (float)T[4 + r];
  }
}

// Optimizer.cc:658-781. B also supplies start, classify and finish.
template <class B>
inline int lba_run(B& b, const LbaIn& in, const LbaPlan& P, LbaOut* o) {
  o->tcw.assign(in.tcw, in.tcw + 12 * (size_t)in.nk);
  o->xw.assign(in.xw, in.xw + 3 * (size_t)in.np);
  o->erase.assign(in.ne, 0), o->level1.assign(in.ne, 0);
  o->n_erase = o->rounds_run = o->polls = 0, o->flags = 0;
  memset(o->rounds, 0, sizeof(o->rounds));
  if (P.nfree == 0 || in.ne == 0) return 0;  // deviation: nothing to optimise, the inputs as bits
  LbaPoller poll = {in.stop_flag, in.stop_at_poll, 0};
  int st = 0;
  const bool stop0 = poll();  // :658
  if (!stop0) {
    LbaActive A;
    lba_active(in, P, nullptr, &A);
    if ((st = b.start(P))) return st;
    if ((st = lba_round(b, A, true, 5, poll, &o->rounds[0], &o->flags))) return st;
    o->rounds_run = 1;
    if (!poll()) {  // :667
      if ((st = b.classify(o->level1.data()))) return st;
      int n1 = 0;
      for (int e = 0; e < in.ne; e++) n1 += o->level1[e];
      o->rounds[0].n_flagged = n1;
      lba_active(in, P, o->level1.data(), &A);
      if ((st = lba_round(b, A, false, 10, poll, &o->rounds[1], &o->flags))) return st;
      o->rounds_run = 2;
    }
    if ((st = b.classify(o->erase.data()))) return st;
    for (int e = 0; e < in.ne; e++) o->n_erase += o->erase[e];
    o->rounds[o->rounds_run - 1].n_flagged = o->n_erase;
    std::vector<double> T(7 * (size_t)in.nk), X(3 * (size_t)in.np);
    if ((st = b.finish(T.data(), X.data()))) return st;
    for (int i = 0; i < in.nk; i++)  // a fixed keyframe's pose is not set (a local one with mnId 0: its input bits)
      if (!in.fixed[i]) lba_pose_out(&T[7 * (size_t)i], &o->tcw[12 * (size_t)i]);
    for (size_t i = 0; i < X.size(); i++) o->xw[i] = (float)X[i];
  }
  o->polls = poll.polls;
  return 0;
}

// The workspace in host memory, every stage a loop over the per-element functions: what the local and the
// global adjuster's host backends (LbaHostBackend below, GbaHostBackend of orbfe_gba_core.h) share. Each
// adds its reduced system's arrays and its trial: Dinv, its own Schur complement and solve into y, trial_tail.
struct BaHostBackend {
  LbaWs w;
  LmRec rec;
  LbaActive A;
  std::vector<double> est_T, tri_T, est_X, tri_X, e_err, e_prod, p_hll, p_bl, p_chi, p_dinv, p_db, p_xl, hpp, bp, bs, d, y, xp;

  // n: the bound on the reduced system's size; the caller sets its own arrays and deltas after it
  void start(const LbaPlan& plan, size_t n) {
    memset(&w, 0, sizeof(w));
    const size_t nk = plan.nk, np = plan.np, ne = plan.ne, nf = plan.nfree;
    est_T = plan.T0, tri_T = plan.T0, est_X = plan.X0, tri_X = plan.X0;
    e_err.assign(3 * ne, 0.0), e_prod.assign(LBA_EDGE_DOUBLES * ne, 0.0);
    p_hll.assign(9 * np, 0.0), p_bl.assign(3 * np, 0.0), p_chi.assign(np, 0.0), p_dinv.assign(9 * np, 0.0);
    p_db.assign(3 * np, 0.0), p_xl.assign(3 * np, 0.0);
    hpp.assign(21 * nf, 0.0), bp.assign(6 * nf, 0.0), bs.assign(n, 0.0), d.assign(n, 0.0), y.assign(n, 0.0), xp.assign(n, 0.0);
    w.nk = (int)nk, w.nfree = (int)nf, w.np = (int)np, w.ne = (int)ne;
    w.cam = plan.cam.data(), w.kf_free = plan.kf_free.data(), w.e_pt = plan.e_pt.data(), w.e_obs = plan.e_obs.data();
    w.e_w = plan.e_w.data(), w.e_stereo = plan.e_stereo.data(), w.kl_begin = plan.kl_begin.data(), w.kl_edge = plan.kl_edge.data();
    w.est_T = est_T.data(), w.tri_T = tri_T.data(), w.est_X = est_X.data(), w.tri_X = tri_X.data();
    w.e_err = e_err.data(), w.e_prod = e_prod.data(), w.p_hll = p_hll.data(), w.p_bl = p_bl.data(), w.p_chi = p_chi.data();
    w.p_dinv = p_dinv.data(), w.p_db = p_db.data(), w.p_xl = p_xl.data(), w.hpp = hpp.data(), w.bp = bp.data();
    w.bs = bs.data(), w.d = d.data(), w.y = y.data(), w.xp = xp.data();
    w.edge_begin = plan.edge_begin, w.e_kf = plan.e_kf;
    w.rec = &rec;
  }

  int begin_round(const LbaActive& a, bool kernel_on) {
    A = a;
    w.e_active = A.e_active.data(), w.p_active = A.p_active.data();
    w.slot_of_free = A.slot_of_free.data(), w.free_of_slot = A.free_of_slot.data();
    w.nslot = A.nslot, w.kernel_on = kernel_on ? 1 : 0;
    for (double& v : xp) v = 0.0;  // deviation: x is zero before a round's first successful solve
    for (double& v : p_xl) v = 0.0;
    return 0;
  }

  void tree_reduce(int mode, double lambda, bool trial) {
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

  // after the pose solve, y the solution unless the trial has failed: x and the points' back-substitution,
  // the update, the trial chi2
  int trial_tail(double lambda, LmRec* out) {
    if (!rec.fail) {
      for (int i = 0; i < 6 * w.nslot; i++) w.xp[i] = w.y[i];
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
    w.est_T = est_T.data(), w.tri_T = tri_T.data(), w.est_X = est_X.data(), w.tri_X = tri_X.data();
    return 0;
  }

  int finish(double* T, double* X) {
    memcpy(T, est_T.data(), 8 * est_T.size());
    memcpy(X, est_X.data(), 8 * est_X.size());
    return 0;
  }
};

struct LbaHostBackend : BaHostBackend {
  std::vector<double> S, Lm, Mm;

  int start(const LbaPlan& plan) {
    const size_t n = 6 * (size_t)plan.nfree;
    BaHostBackend::start(plan, n);
    S.assign(n * n, 0.0), Lm.assign(n * n, 0.0), Mm.assign(n * n, 0.0);
    w.S = S.data(), w.Lm = Lm.data(), w.Mm = Mm.data();
    lba_set_deltas(&w);
    return 0;
  }

  int trial(double lambda, LmRec* out) {
    memset(&rec, 0, sizeof(rec));
    const int n = 6 * w.nslot;
    for (int p = 0; p < w.np; p++) lba_point_dinv(w, p, lambda);
    for (int s1 = 0; s1 < w.nslot; s1++)
      for (int s2 = s1; s2 < w.nslot; s2++) {
        double acc[LBA_LANES][42];
        for (int l = 0; l < LBA_LANES; l++) lba_schur_lane(w, w.free_of_slot[s1], w.free_of_slot[s2], l, acc[l]);
        PoHostGroup().reduce(acc);
        lba_schur_finish(w, s1, s2, lambda, acc[0]);
      }
    // the factorisation by columns; a d_j that is 0 (SimplicialLDLT's rule, as remembered) or not finite
    // (deviation) fails the trial
    for (int j = 0; j < n && !rec.fail; j++) {
      const double dj = lba_ldlt_dot(w, n, j, j);
      w.d[j] = dj;
      if (!po_finite(dj)) lm_fail(w.rec, LM_FLAG_NONFINITE);
      else if (dj == 0.0) lm_fail(w.rec, 0);
      if (rec.fail) break;
      for (int i = j + 1; i < n; i++) {
        const double l = lba_ldlt_dot(w, n, i, j) / dj;
        w.Lm[(size_t)j * n + i] = l;
        w.Mm[(size_t)j * n + i] = l * dj;
      }
    }
    if (!rec.fail) {
      for (int i = 0; i < n; i++) w.y[i] = w.bs[i];
      for (int k = 0; k < n; k++)
        for (int i = k + 1; i < n; i++) w.y[i] = w.y[i] - w.Lm[(size_t)k * n + i] * w.y[k];
      for (int i = 0; i < n; i++) w.y[i] = w.y[i] / w.d[i];
      for (int k = n - 1; k >= 0; k--)
        for (int i = 0; i < k; i++) w.y[i] = w.y[i] - w.Lm[(size_t)i * n + k] * w.y[k];
    }
    return trial_tail(lambda, out);
  }

  int classify(uint8_t* flag) {
    for (int e = 0; e < w.ne; e++) flag[e] = lba_edge_flag(w, e) ? 1 : 0;
    return 0;
  }
};
