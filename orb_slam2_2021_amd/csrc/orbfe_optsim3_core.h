// orbfe_optsim3_core.h -- Optimizer::OptimizeSim3's arithmetic (Optimizer.cc:1050-1250 and the g2o
// routines under it: Sim3, VertexSim3Expmap::oplusImpl, EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ,
// BaseBinaryEdge's numeric linearizeOplus and constructQuadraticForm, RobustKernelHuber,
// OptimizationAlgorithmLevenberg, BlockSolver's non-Schur path, LinearSolverDense) as host/device
// inline functions. Used by k_optsim3 in orbfe_optsim3.hip and by the stand-alone host program
// tests/cpp/optsim3_core_main.cpp. Not part of the C ABI.
//
// Every operation is an IEEE double (or float) + - * / sqrt, rounded separately (-ffp-contract=off).
// No libm call: sin / cos are orbfe_poseopt_core.h's po_sincos, std::exp of Sim3(update) is restated
// below (os_exp), pow(x, 3) is a product. Every Eigen operation is restated by the rule DESIGN.md
// sections 18 and 19 record, marked "EIGEN:"; tests/optsim3_ref.py is the same code in Python, line by
// line.
//
// A problem is run by a group of PO_LANES lanes (orbfe_lm_core.h's group abstraction); the Levenberg
// controller (LmCtl) and the 7x7 LDLT (lm_ldlt<7>) are that header's too.
// Correspondence i (KF1's keypoint index) belongs to lane i % PO_LANES; a lane adds, in ascending i,
// first e12 then e21 of its active correspondences into OS_ACC accumulators that start at +0.0, and the
// lanes are combined by s[l] += s[l + stride], stride = 32 .. 1. The Jacobians are numeric, as in the
// reference: per linearisation the 14 perturbed estimates oplus(+-1e-9 e_d) and their inverses are
// built once into the work area's table (they do not depend on the edge) and every edge is evaluated
// at the 15 states of the table.
//
// Deviations from the reference, deliberate:
//  - the fixed order of the sum over edges above (g2o's follows a std::set of pointers), and Eigen's
//    small fixed-size products taken in plain left-to-right scalar order; the information matrix is
//    read as the diagonal it is (no 0 * e terms);
//  - exp, sin, cos from + - * / (os_exp within 1 ulp of libm on [-1, 1], po_sincos as section 18);
//    pow(2 rho - 1, 3) is a product (orbfe_lm_core.h). A rotation step above pi sets LM_FLAG_LARGE_STEP;
//  - LM_FLAG_NONFINITE: a non-finite entry of H + lambda I or b makes the trial fail as a non-positive
//    factorisation does (tempChi = DBL_MAX, rejected); Eigen's pivot search is not followed over NaN;
//  - the increment x is zero before a round's first successful solve; g2o leaves it as allocated.
//
// Every Levenberg decision is taken on values that are identical in all lanes, so control flow is
// uniform; every loop has a fixed cap (2 rounds, 10 iterations, 10 trials, 7 pivots, ceil(n / 64) <= 64
// correspondences per lane) and no computed value forms an address.
#pragma once
#include "orbfe_lm_core.h"
#include "orbfe_poseopt_core.h"  // po_sincos and the quaternion rules

#define OS_ACC 36     // 28 lower entries of H (row-major over r >= c), 7 of b, the robust chi2
#define OS_STATES 15  // the estimate, then oplus(+delta e_d), oplus(-delta e_d) for d = 0 .. 6
#define OS_STATE_DOUBLES 16  // a state and its inverse: q xyzw, t, s each

struct OsSim3 {
  double q[4];  // x y z w, not normalised (Sim3 never normalises)
  double t[3];
  double s;
};

// One problem as the kernel sees it: KF1-indexed arrays, the cameras and th2 widened to double.
struct OsProblem {
  int n;
  int fix_scale;
  int has_kf2;
  const uint8_t* valid;
  const float* p3d1c;  // [n*3]
  const float* p3d2c;  // [n*3]
  const float* kp1;    // [n*2]
  const float* kp2;    // [n*2]
  const float* is1;    // [n]
  const float* is2;    // [n]
  double k1[4], k2[4];  // fx fy cx cy
  double th2;
  const float* start;  // r12[9], t12[3], s12
  const float* kf2;    // r2w[9], t2w[3]
};

struct OsOut {
  double sim3[8];  // q xyzw, t, s
  float s12_rt[12];
  float scw[12];
  int32_t n_correspondences, n_bad, n_inliers, rounds_run;
  uint32_t flags, pad;
  PoRound rounds[2];
};

// The solve's working set and the perturbation table: LDS on the device.
struct OsWork {
  double A[49], x[7], rhs[7], temp[7];
  int tr[7];
  int positive;
  double S[OS_ACC];  // the sums of the current linearisation
  double J[14 * PO_LANES];  // an edge's Jacobian, entry k of lane l at J[k * PO_LANES + l]
  double tab[OS_STATES * OS_STATE_DOUBLES];
};

// ---- exp from + - * / ------------------------------------------------------------------------------
// Deviation: replaces std::exp. Cody-Waite reduction by ln 2 (k ln2_hi is exact for |k| < 2^11), the
// rational form of fdlibm's e_exp.c on the reduced argument, then k exact doublings or halvings.
PO_HD inline double os_exp(double x) {
  if (x != x) return x;
  if (x > 709.782712893384) return DBL_MAX * 2.0;  // +inf
  if (x < -745.2) return 0.0;
  const long long kk = (long long)(x * 1.44269504088896338700e+00 + (x < 0 ? -0.5 : 0.5));
  const double k = (double)kk;
  const double hi = x - k * 6.93147180369123816490e-01;
  const double lo = k * 1.90821492927058770002e-10;
  const double r = hi - lo;
  const double t = r * r;
  const double c =
      r - t * (1.66666666666666019037e-01 +
               t * (-2.77777777770155933842e-03 +
                    t * (6.61375632143793436117e-05 + t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
  double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
  const bool neg = kk < 0;
  const long long a = neg ? -kk : kk;  // <= 1076
  double p = neg ? 0.5 : 2.0;
#pragma unroll
  for (int j = 0; j < 11; j++) {  // y *= 2^(+-2^j) for the bits of |k|; the last factor is applied as two halves
    if (j < 10) {
      if ((a >> j) & 1) y = y * p;
      p = p * p;
    } else if ((a >> j) & 1) {
      const double h = neg ? 7.458340731200207e-155 : 1.3407807929942597e+154;  // 2^-512, 2^512
      y = y * h;
      y = y * h;
    }
  }
  return y;
}

// ---- Sim3 ------------------------------------------------------------------------------------------
// Sim3(const Vector7d&) (sim3.h:70-142). EIGEN: norm() is sqrt((x^2 + y^2) + z^2); a 3x3 product sums
// k ascending; a sum of three matrices is taken left to right per entry.
PO_HD inline void os_sim3_from_update(const double* u, OsSim3* S, unsigned* flags) {
  const double sigma = u[6];
  const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double O[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
  const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double O2[9], R[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
  const double s = os_exp(sigma);
  const double eps = 0.00001;
  double A, B, C;
  const bool small_theta = theta < eps;
  double sn = 0.0, cs = 1.0;
  if (!small_theta) po_sincos(theta, &sn, &cs, flags);
  if (fabs(sigma) < eps) {
    C = 1;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double a = s * sn;
      const double b = s * cs;
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  if (small_theta) {
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (I[i] + O[i]) + O2[i];
  } else {
    const double ra = sn / theta;
    const double rb = (1 - cs) / (theta * theta);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (I[i] + ra * O[i]) + rb * O2[i];
  }
  po_quat_from_matrix(R, S->q);  // r = Quaterniond(R): no normalisation
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double w0 = (A * O[3 * r] + B * O2[3 * r]) + C * I[3 * r];
    const double w1 = (A * O[3 * r + 1] + B * O2[3 * r + 1]) + C * I[3 * r + 1];
    const double w2 = (A * O[3 * r + 2] + B * O2[3 * r + 2]) + C * I[3 * r + 2];
    S->t[r] = (w0 * u[3] + w1 * u[4]) + w2 * u[5];
  }
  S->s = s;
}

// Sim3::operator*: r = a.r * b.r; t = a.s * (a.r * b.t) + a.t; s = a.s * b.s
PO_HD inline void os_sim3_mul(const OsSim3& a, const OsSim3& b, OsSim3* o) {
  double r[3];
  po_quat_rotate(a.q, b.t, r);
  po_quat_mul(a.q, b.q, o->q);
  o->t[0] = a.s * r[0] + a.t[0], o->t[1] = a.s * r[1] + a.t[1], o->t[2] = a.s * r[2] + a.t[2];
  o->s = a.s * b.s;
}

// Sim3::inverse: Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
PO_HD inline void os_sim3_inverse(const OsSim3& a, OsSim3* o) {
  o->q[0] = -a.q[0], o->q[1] = -a.q[1], o->q[2] = -a.q[2], o->q[3] = a.q[3];
  const double c = -1. / a.s;
  const double v[3] = {c * a.t[0], c * a.t[1], c * a.t[2]};
  po_quat_rotate(o->q, v, o->t);
  o->s = 1. / a.s;
}

// Sim3(Matrix3d, Vector3d, double) of widened floats (LoopClosing.cc:341, :350): r = Quaterniond(R)
PO_HD inline void os_sim3_from_floats(const float* r9, const float* t3, double s, OsSim3* S) {
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; i++) m[i] = (double)r9[i];
  po_quat_from_matrix(m, S->q);
  S->t[0] = (double)t3[0], S->t[1] = (double)t3[1], S->t[2] = (double)t3[2];
  S->s = s;
}

// VertexSim3Expmap::oplusImpl: update[6] = 0 in place with _fix_scale; Sim3(update) * estimate()
PO_HD inline void os_oplus(double* u, bool fix_scale, const OsSim3& est, OsSim3* o, unsigned* flags) {
  if (fix_scale) u[6] = 0;
  OsSim3 d;
  os_sim3_from_update(u, &d, flags);
  os_sim3_mul(d, est, o);
}

PO_HD inline void os_store_state(double* dst, const OsSim3& S) {
#pragma unroll
  for (int k = 0; k < 4; k++) dst[k] = S.q[k];
#pragma unroll
  for (int k = 0; k < 3; k++) dst[4 + k] = S.t[k];
  dst[7] = S.s;
}

// Converter::toCvMat(g2o::Sim3): float(s * R | t)
PO_HD inline void os_sim3_to_rt(const OsSim3& S, float* rt) {
  double m[9];
  po_quat_to_matrix(S.q, m);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) rt[4 * i + j] = (float)(S.s * m[3 * i + j]);
    rt[4 * i + 3] = (float)S.t[i];
  }
}

// ---- one edge --------------------------------------------------------------------------------------
// computeError of EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ at the state S (8 doubles: the
// estimate for e12, its inverse for e21): obs - cam_map(project(S.map(X))); map = s * (r * X) + t
PO_HD inline void os_edge_error(const double* S, const double* X, const double* obs, const double* cam, double* err) {
  double r[3];
  po_quat_rotate(S, X, r);
  const double p0 = S[7] * r[0] + S[4], p1 = S[7] * r[1] + S[5], p2 = S[7] * r[2] + S[6];
  err[0] = obs[0] - (p0 / p2 * cam[0] + cam[2]);
  err[1] = obs[1] - (p1 / p2 * cam[1] + cam[3]);
}

// EIGEN: _error.dot(information() * _error) with a diagonal information
PO_HD inline double os_edge_chi2(double w, const double* err) { return err[0] * (w * err[0]) + err[1] * (w * err[1]); }

// The data of edge `dir` (0: e12 = x1 from S12 * X2, 1: e21 = x2 from S21 * X1) of correspondence i
PO_HD inline void os_load_edge(const OsProblem& P, int i, int dir, double* X, double* obs, double* w) {
  const float* x = dir == 0 ? P.p3d2c : P.p3d1c;
  const float* kp = dir == 0 ? P.kp1 : P.kp2;
  X[0] = (double)x[3 * (size_t)i], X[1] = (double)x[3 * (size_t)i + 1], X[2] = (double)x[3 * (size_t)i + 2];
  obs[0] = (double)kp[2 * (size_t)i], obs[1] = (double)kp[2 * (size_t)i + 1];
  *w = (double)(dir == 0 ? P.is1 : P.is2)[i];
}

// const float deltaHuber = sqrt(th2); setDelta widens
PO_HD inline double os_huber_delta(double th2) { return (double)(float)sqrt(th2); }

// RobustKernelHuber::robustify -> rho[0]; *rho1 = rho[1]
PO_HD inline double os_huber(double chi2, double delta, double dsqr, double* rho1) {
  *rho1 = 1.0;
  if (chi2 <= dsqr) return chi2;
  const double sq = sqrt(chi2);
  *rho1 = delta / sq;
  return 2 * sq * delta - dsqr;
}

// computeError + activeRobustChi2's term of one edge at the state S
PO_HD inline void os_edge_chi_accumulate(double* acc, const OsProblem& P, int i, int dir, const double* S, double delta,
                                         double dsqr) {
  double X[3], obs[2], w, err[2], rho1;
  os_load_edge(P, i, dir, X, obs, &w);
  os_edge_error(S, X, obs, dir == 0 ? P.k1 : P.k2, err);
  acc[35] = acc[35] + os_huber(os_edge_chi2(w, err), delta, dsqr, &rho1);
}

// computeError, the numeric BaseBinaryEdge::linearizeOplus over the table (column d =
// (1 / (2 delta)) * (e(+d) - e(-d))) and the robust constructQuadraticForm of one edge.
// EIGEN: omega_r = -(w * e_k), omega_r *= rho1; b_r += B_0r * omega_r0 + B_1r * omega_r1;
//        H_rc += (B_0r * (rho1 * w)) * B_0c + (B_1r * (rho1 * w)) * B_1c, lower triangle only.
// Jl: the lane's column of OsWork::J; the loop over d stays rolled, so the table is read as it is needed.
PO_HD inline void os_edge_accumulate(double* acc, const OsProblem& P, int i, int dir, const double* tab, double* Jl,
                                     double delta, double dsqr) {
  double X[3], obs[2], w, err[2], rho1;
  os_load_edge(P, i, dir, X, obs, &w);
  const double* cam = dir == 0 ? P.k1 : P.k2;
  const int off = dir == 0 ? 0 : 8;
  os_edge_error(tab + off, X, obs, cam, err);
  acc[35] = acc[35] + os_huber(os_edge_chi2(w, err), delta, dsqr, &rho1);
  const double scalar = 1.0 / (2 * 1e-9);
  // Load-bearing: this loop must stay rolled and J must go through Jl (LDS). Unrolled, or with J kept in
  // registers across it, the compiler hoists the table's 30 x 8 loads out of the loop over the lane's
  // correspondences and k_optsim3 spills to scratch (1,452 bytes per lane measured). Check
  // -Rpass-analysis=kernel-resource-usage after any change here: scratch must stay 0.
#pragma unroll 1
  for (int d = 0; d < 7; d++) {
    double ep[2], em[2];
    os_edge_error(tab + (1 + 2 * d) * OS_STATE_DOUBLES + off, X, obs, cam, ep);
    os_edge_error(tab + (2 + 2 * d) * OS_STATE_DOUBLES + off, X, obs, cam, em);
    Jl[d * PO_LANES] = scalar * (ep[0] - em[0]);
    Jl[(7 + d) * PO_LANES] = scalar * (ep[1] - em[1]);
  }
  double J[14];
#pragma unroll
  for (int k = 0; k < 14; k++) J[k] = Jl[k * PO_LANES];
  const double or0 = -(w * err[0]) * rho1, or1 = -(w * err[1]) * rho1;
  const double ww = rho1 * w;
#pragma unroll
  for (int r = 0; r < 7; r++) {
    acc[28 + r] = acc[28 + r] + (J[r] * or0 + J[7 + r] * or1);
#pragma unroll
    for (int c = 0; c <= r; c++)
      acc[r * (r + 1) / 2 + c] = acc[r * (r + 1) / 2 + c] + ((J[r] * ww) * J[c] + (J[7 + r] * ww) * J[7 + c]);
  }
}

// The table of one linearisation: state 0 is the estimate, state 1 + 2 d + (0 | 1) is oplus(+delta e_d |
// -delta e_d); each followed by its inverse. Lanes 0 .. 14 build one state each.
template <class G>
PO_HD inline void os_build_table(const G& g, OsWork& w, const OsSim3& est, bool fix_scale) {
  g.sync();  // every lane has read the previous table
  for (int slot = 0; slot < G::slots; slot++) {
    const int vl = slot * G::width + g.lane();
    if (vl >= OS_STATES) continue;
    OsSim3 S = est, Si;
    if (vl > 0) {
      const int d = (vl - 1) >> 1;
      double u[7];
#pragma unroll
      for (int k = 0; k < 7; k++) u[k] = k == d ? (((vl - 1) & 1) ? -1e-9 : 1e-9) : 0.0;
      unsigned unused = 0;
      os_oplus(u, fix_scale, est, &S, &unused);
    }
    os_sim3_inverse(S, &Si);
    os_store_state(w.tab + vl * OS_STATE_DOUBLES, S);
    os_store_state(w.tab + vl * OS_STATE_DOUBLES + 8, Si);
  }
  g.sync();
}

// The sums over the active correspondences (valid and not removed): s[0] holds them in every lane.
// rem[slot]: bit c = the removal flag of correspondence (slot * width + lane) + 64 c.
template <class G>
PO_HD inline void os_sums_full(const G& g, const OsProblem& P, const uint64_t* rem, OsWork& w, double delta, double dsqr,
                               double (*s)[OS_ACC]) {
  for (int slot = 0; slot < G::slots; slot++) {
    const int vl = slot * G::width + g.lane();
    double acc[OS_ACC];
#pragma unroll
    for (int k = 0; k < OS_ACC; k++) acc[k] = 0.0;
    int c = 0;
    for (int i = vl; i < P.n; i += PO_LANES, c++) {  // at most ceil(n / 64) <= 64 correspondences
      if (!P.valid[i] || ((rem[slot] >> c) & 1ull)) continue;
      os_edge_accumulate(acc, P, i, 0, w.tab, w.J + g.lane(), delta, dsqr);
      os_edge_accumulate(acc, P, i, 1, w.tab, w.J + g.lane(), delta, dsqr);
    }
#pragma unroll
    for (int k = 0; k < OS_ACC; k++) s[slot][k] = acc[k];
  }
  g.reduce(s);
}

// activeRobustChi2 at the state T (8 doubles) and its inverse Ti
template <class G>
PO_HD inline void os_sums_chi(const G& g, const OsProblem& P, const uint64_t* rem, const double* T, const double* Ti,
                              double delta, double dsqr, double (*s)[1]) {
  for (int slot = 0; slot < G::slots; slot++) {
    const int vl = slot * G::width + g.lane();
    double acc[OS_ACC];
    acc[35] = 0.0;
    int c = 0;
    for (int i = vl; i < P.n; i += PO_LANES, c++) {
      if (!P.valid[i] || ((rem[slot] >> c) & 1ull)) continue;
      os_edge_chi_accumulate(acc, P, i, 0, T, delta, dsqr);
      os_edge_chi_accumulate(acc, P, i, 1, Ti, delta, dsqr);
    }
    s[slot][0] = acc[35];
  }
  g.reduce(s);
}

// ---- OptimizeSim3 ----------------------------------------------------------------------------------
// mask: ceil(n / 64) words, bit i % 64 of word i / 64 = "vpMatches1[i] was set to NULL". Lane 0 writes o
// and mask.
template <class G>
PO_HD inline void os_optimize(const G& g, const OsProblem& P, OsWork& w, OsOut* o, uint64_t* mask) {
  const int lane = g.lane();
  const int words = (P.n + 63) / 64;
  const bool fix_scale = P.fix_scale != 0;
  const double delta = os_huber_delta(P.th2);
  const double dsqr = delta * delta;
  uint64_t rem[G::slots], val[G::slots];
  for (int slot = 0; slot < G::slots; slot++) {
    const int vl = slot * G::width + lane;
    uint64_t v = 0;
    int c = 0;
    for (int i = vl; i < P.n; i += PO_LANES, c++)
      if (P.valid[i]) v |= 1ull << c;
    val[slot] = v;
    rem[slot] = 0;
  }
  int n_corr = 0;
  for (int c = 0; c < words; c++) n_corr += (int)__builtin_popcountll(g.ballot(val, c));
  OsSim3 start, est, eval;
  os_sim3_from_floats(P.start, P.start + 9, (double)P.start[12], &start);
  est = start;
  eval = est;
  unsigned flags = 0;
  int n_bad = 0, rounds_run = 0;
  if (lane == 0)
    for (int it = 0; it < 2; it++) {
      PoRound z = {0, 0, 0, 0, 0, 0, 0.0, 0.0};
      o->rounds[it] = z;
    }
  for (int it = 0; it < 2; it++) {
    if (it == 1 && n_corr - n_bad < 10) break;  // :1220: return 0, g2oS12 untouched
    const int max_iter = it == 0 ? 5 : (n_bad > 0 ? 10 : 5);
    const int n_active = n_corr - n_bad;
    int iterations = 0, trials = 0, rejected = 0, stop = LM_STOP_ALL;
    LmCtl lm = {0.0, 0.0, 0.0, 2.0, 0.0, 0, 0};
    if (n_active == 0) {
      stop = LM_STOP_NO_EDGE;
    } else {
      g.sync();
      if (lane == 0)
        for (int j = 0; j < 7; j++) w.x[j] = 0.0;  // deviation: zero before a round's first successful solve
      g.sync();
      for (int i = 0; i < 10; i++) {
        if (i >= max_iter) break;
        iterations++;
        os_build_table(g, w, est, fix_scale);
        {
          double S[G::slots][OS_ACC];
          os_sums_full(g, P, rem, w, delta, dsqr, S);
          if (lane == 0)
            for (int k = 0; k < OS_ACC; k++) w.S[k] = S[0][k];
          g.sync();
        }
        const double* s = w.S;  // read where needed: 36 doubles are not held across the trials
        double lambda_init = 0.0;
        if (i == 0) {
          double mx = 0.0;
#pragma unroll
          for (int j = 0; j < 7; j++) {
            const double a = fabs(s[j * (j + 1) / 2 + j]);
            mx = a < mx ? mx : a;  // std::max(fabs(H_jj), maxDiagonal)
          }
          lambda_init = 1e-5 * mx;
        }
        lm_begin_iteration(lm, s[35], i == 0, lambda_init);
        do {
          const double lambda = lm.lambda;
          // setLambda + LinearSolverDense::solve. Deviation: a non-finite entry gives ok2 = false
          bool ok2 = true;
#pragma unroll
          for (int k = 0; k < 35; k++) ok2 = ok2 && po_finite(s[k]);
          ok2 = ok2 && po_finite(lambda);
#pragma unroll
          for (int j = 0; j < 7; j++) ok2 = ok2 && po_finite(s[j * (j + 1) / 2 + j] + lambda);
          if (!ok2) flags |= LM_FLAG_NONFINITE;
          g.sync();
          if (lane == 0 && ok2) {
#pragma unroll
            for (int r = 0; r < 7; r++) {
#pragma unroll
              for (int c = 0; c <= r; c++) w.A[7 * r + c] = r == c ? s[r * (r + 1) / 2 + c] + lambda : s[r * (r + 1) / 2 + c];
              w.rhs[r] = s[28 + r];
            }
            w.positive = lm_ldlt<7>(w.A, w.tr, w.temp) ? 1 : 0;
            if (w.positive) lm_ldlt_solve<7>(w.A, w.tr, w.rhs, w.x);
          }
          g.sync();
          ok2 = ok2 && w.positive != 0;
          double x[7];
#pragma unroll
          for (int j = 0; j < 7; j++) x[j] = w.x[j];
          OsSim3 trial, trial_inv;
          os_oplus(x, fix_scale, est, &trial, &flags);  // zeroes x[6] with fix_scale: computeScale reads it so
          os_sim3_inverse(trial, &trial_inv);
          eval = trial;
          double T[8], Ti[8];
          os_store_state(T, trial);
          os_store_state(Ti, trial_inv);
          double C[G::slots][1];
          os_sums_chi(g, P, rem, T, Ti, delta, dsqr, C);
          double scale = 0.0;
#pragma unroll
          for (int j = 0; j < 7; j++) scale = scale + x[j] * (lambda * x[j] + s[28 + j]);
          trials++;
          if (lm_trial(lm, C[0][0], !ok2, scale)) est = trial;
          else rejected++;
        } while (lm_more_trials(lm));
        stop = lm_end_iteration(lm);
        if (stop != LM_STOP_ALL) break;
      }
    }
    // :1195-1212, :1229-1243: an active correspondence is removed when e12->chi2() > th2 ||
    // e21->chi2() > th2, both the errors of the last evaluated trial, accepted or not; a NaN keeps it
    OsSim3 eval_inv;
    os_sim3_inverse(eval, &eval_inv);
    double T[8], Ti[8];
    os_store_state(T, eval);
    os_store_state(Ti, eval_inv);
    for (int slot = 0; slot < G::slots; slot++) {
      const int vl = slot * G::width + lane;
      uint64_t nw = rem[slot];
      int c = 0;
      for (int i = vl; i < P.n; i += PO_LANES, c++) {
        if (!P.valid[i] || ((rem[slot] >> c) & 1ull)) continue;
        double X[3], obs[2], wgt, err[2];
        os_load_edge(P, i, 0, X, obs, &wgt);
        os_edge_error(T, X, obs, P.k1, err);
        const double c12 = os_edge_chi2(wgt, err);
        os_load_edge(P, i, 1, X, obs, &wgt);
        os_edge_error(Ti, X, obs, P.k2, err);
        const double c21 = os_edge_chi2(wgt, err);
        if (c12 > P.th2 || c21 > P.th2) nw |= 1ull << c;
      }
      rem[slot] = nw;
    }
    n_bad = 0;
    for (int c = 0; c < words; c++) n_bad += (int)__builtin_popcountll(g.ballot(rem, c));
    rounds_run = it + 1;
    if (lane == 0) {
      PoRound r = {n_active, iterations, trials, rejected, stop, n_bad, lm.lambda, lm.current};
      o->rounds[it] = r;
    }
  }
  for (int c = 0; c < words; c++) {
    const uint64_t word = g.ballot(rem, c);
    if (lane == 0) mask[c] = word;
  }
  if (lane == 0) {
    const OsSim3 out = rounds_run == 2 ? est : start;
    os_store_state(o->sim3, out);
    os_sim3_to_rt(out, o->s12_rt);
    for (int i = 0; i < 12; i++) o->scw[i] = 0.0f;
    if (P.has_kf2) {  // LoopClosing.cc:350-354: mScw = toCvMat(gScm * gSmw)
      OsSim3 smw, scw;
      os_sim3_from_floats(P.kf2, P.kf2 + 9, 1.0, &smw);
      os_sim3_mul(out, smw, &scw);
      os_sim3_to_rt(scw, o->scw);
    }
    o->n_correspondences = n_corr;
    o->n_bad = n_bad;
    o->n_inliers = rounds_run == 2 ? n_corr - n_bad : 0;
    o->rounds_run = rounds_run;
    o->flags = flags;
    o->pad = 0;
  }
}

// ------------------------------------------------------------------------------------------
// staging (host)

// One problem as the kernel sees it. in_* are byte offsets into the upload buffer, o_* into the result
// buffer.
struct OsDev {
  int n, fix_scale, has_kf2, pad;
  double cam[9];    // k1, k2 (fx, fy, cx, cy: float widened to double), th2
  float start[13];  // r12, t12, s12
  float kf2[12];    // r2w, t2w
  float pad2;
  unsigned long long in_valid, in_p1, in_p2, in_kp1, in_kp2, in_is1, in_is2, o_out, o_mask;
};

// The arrays of one problem with n correspondences, taken from the two blocks in the order the buffers
// hold them; fills d's offsets only. The one statement of the buffer plan: over counting blocks it sizes
// a handle (os_plan_bounds), over the real ones it places a batch.
inline void os_layout(OrbfeStage& in, OrbfeStage& res, size_t n, OsDev& d) {
  d.in_valid = in.take(n);
  d.in_p1 = in.take(12 * n);
  d.in_p2 = in.take(12 * n);
  d.in_kp1 = in.take(8 * n);
  d.in_kp2 = in.take(8 * n);
  d.in_is1 = in.take(4 * n);
  d.in_is2 = in.take(4 * n);
  d.o_out = res.take(sizeof(OsOut));
  d.o_mask = res.take(8 * ((n + 63) / 64));
}

// A handle's buffer sizes: the record table and S problems at the bound
inline void os_plan_bounds(size_t S, size_t C, size_t* in_bytes, size_t* res_bytes) {
  OrbfeStage in, res;
  OsDev d;
  in.take(sizeof(OsDev) * S);
  for (size_t s = 0; s < S; s++) os_layout(in, res, C, d);
  *in_bytes = in.off, *res_bytes = res.off;
}
