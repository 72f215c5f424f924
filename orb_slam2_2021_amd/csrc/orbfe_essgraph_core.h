// orbfe_essgraph_core.h -- Optimizer::OptimizeEssentialGraph's arithmetic (Optimizer.cc:784-1048 and the
// g2o routines under it: Sim3 with log(), VertexSim3Expmap::oplusImpl, EdgeSim3::computeError,
// BaseBinaryEdge's numeric linearizeOplus and constructQuadraticForm, BlockSolver_7_3's buildSystem /
// setLambda, OptimizationAlgorithmLevenberg with setUserLambdaInit, SparseOptimizer's optimize / push /
// pop / update) as host/device inline functions over one workspace of plain arrays (EgWs). The kernels of
// orbfe_essgraph.hip call the per-element functions with one thread or lane each; EgHostBackend below
// loops the same functions on the host; eg_run drives orbfe_lm_core.h's Levenberg control flow, on the host for both.
// Used by orbfe_essgraph.hip and tests/cpp/essgraph_core_main.cpp; tests/essgraph_ref.py is the same code
// in Python. Not part of the C ABI. The quaternion rules, po_sincos, os_exp and the Sim3 functions of
// orbfe_poseopt_core.h and orbfe_optsim3_core.h are reused; the flag and stop codes, the record (LmRec),
// the host group and po_finite are orbfe_lm_core.h's. Every operation is an IEEE double + - * / sqrt,
// rounded separately (-ffp-contract=off). "EIGEN:" marks a restated Eigen rule.
//
// Summation (the rule that defines the numbers):
//   per vertex   H_ii and b_i run over the vertex's incident edges in ascending edge index from +0.0;
//   per block    an off-diagonal block runs over its edges (duplicates allowed) in ascending edge index;
//   totals       edge e (chi2) and slot s (computeScale) belong to lane e % 64 / s % 64; a lane adds in
//                ascending index from +0.0; the lanes are combined by s[l] += s[l + stride], 32 .. 1.
// The linear solve is orbfe_env_core.h's unpivoted LDL^T in natural order over the 7x7 block envelope
// (env_*<7>): entry (i, j) is v = A_ij; v = v - (L_ik d_k) L_jk for k ascending inside both rows'
// envelopes; L_ij = v / d_j.
// Every loop is capped by a count the host has checked; every index read from memory was checked by the
// host (orbfe_essgraph_solve) or built by it (eg_plan).
#pragma once
#include "orbfe_env_core.h"
#include "orbfe_lm_core.h"
#include "orbfe_optsim3_core.h"  // Sim3: OsSim3, os_sim3_*, os_oplus, os_exp, po_sincos, the quaternion rules

#include <algorithm>
#include <cstring>
#include <vector>

#define EG_LANES 64
#define EG_STATES 29        /* the estimates, then 2 vertices x 7 dimensions x (+delta, -delta) */
#define EG_EDGE_DOUBLES 161 /* Ji^T Ji 49, Jj^T Jj 49, Ji^T Jj 49, b_i 7, b_j 7 */
#define EG_MAX_ITER 20

// ---- log and acos from + - * / sqrt ------------------------------------------------------------------
// Deviation: replaces std::log. x = m 2^k with m in [sqrt(1/2), sqrt(2)) by exact halvings / doublings,
// then fdlibm's e_log.c on f = m - 1: s = f / (2 + f), the two polynomials in s^2, and the compensated
// k ln2_hi + k ln2_lo sum. The branches fdlibm takes on the high word are taken on values here.
PO_HD inline double eg_log(double x) {
  if (x != x) return x;
  if (x < 0.0) return (x - x) / (x - x);       // NaN
  if (x == 0.0) return -(DBL_MAX * 2.0);        // -inf
  if (x > DBL_MAX) return x;                    // +inf
  double m = x;
  int k = 0;
  for (int it = 0; it < 1100 && m >= 1.4142135623730951; it++) m = m * 0.5, k++;
  for (int it = 0; it < 1100 && m < 0.70710678118654757; it++) m = m * 2.0, k--;
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  const double f = m - 1.0;
  const double dk = (double)k;
  if (fabs(f) < 9.5367431640625e-07) {  // |f| < 2^-20
    if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
  }
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  const double mo = m < 1.0 ? m * 2.0 : m;  // the mantissa in [1, 2): fdlibm's test on hx
  if (mo >= 1.3799991607666016 && mo < 1.4200000762939453) {
    const double hfsq = 0.5 * f * f;
    return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

PO_HD inline double eg_acos_r(double z) {
  const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
               qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
  const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
  return p / q;
}

// Deviation: replaces std::acos. fdlibm's e_acos.c; the head of sqrt(z) that it takes by clearing the
// low word is taken by Veltkamp's split (26 bits, so df * df is exact as there).
PO_HD inline double eg_acos(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
  if (x != x) return x;
  const double ax = fabs(x);
  if (ax >= 1.0) {
    if (ax == 1.0) return x > 0 ? 0.0 : pi + 2.0 * pio2_lo;
    return (x - x) / (x - x);  // NaN
  }
  if (ax < 0.5) {
    if (ax <= 6.938893903907228e-18) return pio2_hi + pio2_lo;  // 2^-57
    const double r = eg_acos_r(x * x);
    return pio2_hi - (x - (pio2_lo - x * r));
  }
  if (x < 0) {
    const double z = (1.0 + x) * 0.5;
    const double r = eg_acos_r(z);
    const double s = sqrt(z);
    const double w = r * s - pio2_lo;
    return pi - 2.0 * (s + w);
  }
  const double z = (1.0 - x) * 0.5;
  const double s = sqrt(z);
  const double t = s * 134217729.0;
  const double df = t - (t - s);
  const double c = (z - df * df) / (s + df);
  const double r = eg_acos_r(z);
  const double w = r * s + c;
  return 2.0 * (df + w);
}

// EIGEN: PartialPivLU<Matrix3d>::compute (unblocked) and solve. Column k: the pivot is the largest
// |entry| of rows k .. 2, the first maximum wins; the rows swap; a non-zero pivot divides the column
// below it; the rank-1 update a_ij -= l_ik u_kj. solve: P b, the unit lower solve by columns, the upper
// solve by columns from the last (x_i / u_ii, then x_r -= x_i u_ri above it).
PO_HD inline void eg_lu3_solve(const double* W, const double* t, double* x) {
  double a[9];
#pragma unroll
  for (int i = 0; i < 9; i++) a[i] = W[i];
  x[0] = t[0], x[1] = t[1], x[2] = t[2];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int big = k;
    double best = fabs(a[4 * k]);
#pragma unroll
    for (int i = k + 1; i < 3; i++)
      if (i > k && fabs(a[3 * i + k]) > best) big = i, best = fabs(a[3 * i + k]);
#pragma unroll
    for (int i = k + 1; i < 3; i++)
      if (i == big) {  // rows k and big swap, and P b with them
        double tmp;
#pragma unroll
        for (int c = 0; c < 3; c++) tmp = a[3 * k + c], a[3 * k + c] = a[3 * i + c], a[3 * i + c] = tmp;
        tmp = x[k], x[k] = x[i], x[i] = tmp;
      }
    if (best != 0.0) {
#pragma unroll
      for (int i = k + 1; i < 3; i++) a[3 * i + k] = a[3 * i + k] / a[4 * k];
    }
#pragma unroll
    for (int i = k + 1; i < 3; i++)
#pragma unroll
      for (int c = k + 1; c < 3; c++) a[3 * i + c] = a[3 * i + c] - a[3 * i + k] * a[3 * k + c];
  }
  x[1] = x[1] - x[0] * a[3];
  x[2] = x[2] - x[0] * a[6];
  x[2] = x[2] - x[1] * a[7];
  x[2] = x[2] / a[8];
  x[0] = x[0] - x[2] * a[2];
  x[1] = x[1] - x[2] * a[5];
  x[1] = x[1] / a[4];
  x[0] = x[0] - x[1] * a[1];
  x[0] = x[0] / a[0];
}

// Sim3::log() (sim3.h:148-230). EIGEN: d = 0.5 * (((R00 + R11) + R22) - 1); B * Omega * Omega is the
// product of (B Omega) with Omega, k ascending; the sum of three matrices left to right per entry.
PO_HD inline void eg_sim3_log(const OsSim3& S, double* res) {
  const double sigma = eg_log(S.s);
  double R[9];
  po_quat_to_matrix(S.q, R);
  const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR
  const double eps = 0.00001;
  double om[3], A, B, C;
  const bool near = d > 1 - eps;
  double theta = 0.0, sn = 0.0, cs = 1.0;
  if (near) {
    om[0] = 0.5 * dR[0], om[1] = 0.5 * dR[1], om[2] = 0.5 * dR[2];
  } else {
    theta = eg_acos(d);
    const double f = theta / (2 * sqrt(1 - d * d));
    om[0] = f * dR[0], om[1] = f * dR[1], om[2] = f * dR[2];
    unsigned unused = 0;
    po_sincos(theta, &sn, &cs, &unused);
  }
  if (fabs(sigma) < eps) {
    C = 1;
    if (near) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (near) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta2 = theta * theta;
      const double a = S.s * sn;
      const double b = S.s * cs;
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  const double O[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};  // skew
  const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double W[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double bo2 = ((B * O[3 * r]) * O[c] + (B * O[3 * r + 1]) * O[3 + c]) + (B * O[3 * r + 2]) * O[6 + c];
      W[3 * r + c] = (A * O[3 * r + c] + bo2) + C * I[3 * r + c];
    }
  double up[3];
  eg_lu3_solve(W, S.t, up);
  res[0] = om[0], res[1] = om[1], res[2] = om[2];
  res[3] = up[0], res[4] = up[1], res[5] = up[2];
  res[6] = sigma;
}

PO_HD inline void eg_load(const double* a, OsSim3* S) {
#pragma unroll
  for (int k = 0; k < 4; k++) S->q[k] = a[k];
#pragma unroll
  for (int k = 0; k < 3; k++) S->t[k] = a[4 + k];
  S->s = a[7];
}

// EdgeSim3::computeError: (C * v0.estimate() * v1.estimate().inverse()).log()
PO_HD inline void eg_error(const OsSim3& C, const OsSim3& Si, const OsSim3& Sj, double* err) {
  OsSim3 a, inv, b;
  os_sim3_mul(C, Si, &a);
  os_sim3_inverse(Sj, &inv);
  os_sim3_mul(a, inv, &b);
  eg_sim3_log(b, err);
}

// chi2 with the identity information: the sum of squares in index order
PO_HD inline double eg_chi2(const double* e) {
  double s = e[0] * e[0];
#pragma unroll
  for (int k = 1; k < 7; k++) s = s + e[k] * e[k];
  return s;
}

struct EgTrace {
  int32_t iterations, trials, rejected_trials, stop;
  double lambda, chi2;
  int32_t env_blocks;
  uint32_t flags;
};

struct EgWs {
  int nv, ne, ns, nblk, nob, np, fix_scale, fixed;
  // the problem
  const float* tcw;        // [nv * 12]
  const int* corr_of_v;    // [nv] index into corr, or -1
  const int* nonc_of_v;    // [nv] index into nonc, or -1
  const double* corr;      // [ncorr * 8]
  const double* nonc;      // [nnonc * 8]
  const int* e_i;          // [ne] vertex 0
  const int* e_j;          // [ne] vertex 1
  const uint8_t* e_kind;   // [ne]
  const float* xw;         // [np * 3]
  const int* p_ref;        // [np]
  // the structure (eg_plan)
  const int* slot_of_v;  // [nv] the vertex's block row, or -1 (the fixed vertex, a vertex without an edge)
  const int* v_of_slot;  // [ns]
  const int* ve_begin;   // [ns + 1] slot s's incident edges, ascending ...
  const int* ve_edge;    // ... as 2 e + side (side 1: the slot's vertex is the edge's vertex 1)
  const int* row_first;  // [ns] the first block column of row s
  const int* row_off;    // [ns + 1] row s's blocks are row_off[s] .. row_off[s + 1] - 1, the last the diagonal
  const int* ob_begin;   // [nob + 1] the off-diagonal blocks that have edges ...
  const int* ob_pos;     // [nob] ... their position in the envelope ...
  const int* ob_edge;    // ... and their edges, ascending, as 2 e + transposed
  const int* col_begin;  // [ns + 1] the rows s > b whose envelope holds column b ...
  const int* col_row;    // ... ascending
  // states: q (x y z w), t, s
  double* scw;   // [nv * 8] vScw: the start estimates
  double* mst;   // [nv * 8] the measurement-side state: NonCorrectedSim3 where the keyframe is in it
  double* est;   // [nv * 8] accepted
  double* tri;   // [nv * 8] trial
  double* meas;  // [ne * 8]
  // per edge
  double* e_state;  // [ne * EG_STATES * 7] the errors at the 29 states of one linearisation
  double* e_chi;    // [ne]
  double* e_prod;   // [ne * EG_EDGE_DOUBLES]
  // the system
  double* H;  // [nblk * 49] the envelope of the lower triangle, lambda not added
  double* L;  // [nblk * 49] H + lambda I, factored in place (unit lower, the diagonal unused after)
  double* b;  // [ns * 7]
  double* d;  // [ns * 7]
  double* y;  // [ns * 7]
  double* x;  // [ns * 7] the increment of the last successful solve
  float* out_tcw;  // [nv * 12]
  float* out_xw;   // [np * 3]
  LmRec* rec;
};

// ---- setup --------------------------------------------------------------------------------------------
// Optimizer.cc:812-847: vScw and the start estimate; the state the kind-1 measurements are taken from
PO_HD inline void eg_vertex_setup(const EgWs& w, int v) {
  OsSim3 S, M;
  if (w.corr_of_v[v] >= 0) {
    eg_load(w.corr + 8 * (size_t)w.corr_of_v[v], &S);
  } else {
    const float* T = w.tcw + 12 * (size_t)v;
    const float r9[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const float t3[3] = {T[3], T[7], T[11]};
    os_sim3_from_floats(r9, t3, 1.0, &S);
  }
  M = S;
  if (w.nonc_of_v[v] >= 0) eg_load(w.nonc + 8 * (size_t)w.nonc_of_v[v], &M);
  os_store_state(w.scw + 8 * (size_t)v, S);
  os_store_state(w.est + 8 * (size_t)v, S);
  os_store_state(w.tri + 8 * (size_t)v, S);
  os_store_state(w.mst + 8 * (size_t)v, M);
}

// :861-877 (kind 0: Sjw * Swi over vScw) and :894-984 (kind 1: over NonCorrectedSim3 where present)
PO_HD inline void eg_edge_setup(const EgWs& w, int e) {
  const double* src = w.e_kind[e] == 0 ? w.scw : w.mst;
  OsSim3 Si, Sj, inv, m;
  eg_load(src + 8 * (size_t)w.e_i[e], &Si);
  eg_load(src + 8 * (size_t)w.e_j[e], &Sj);
  os_sim3_inverse(Si, &inv);
  os_sim3_mul(Sj, inv, &m);
  os_store_state(w.meas + 8 * (size_t)e, m);
}

// ---- linearisation ------------------------------------------------------------------------------------
// The error of edge e at state k of BaseBinaryEdge::linearizeOplus: k = 0 the estimates; k = 1 + 14 side
// + 2 d + (0 | 1): vertex `side` at oplus(+delta e_d | -delta e_d). A fixed vertex's states are not
// computed (zeros stand in: its Jacobian is not used).
PO_HD inline void eg_edge_state(const EgWs& w, int e, int k, const double* est) {
  double* out = w.e_state + ((size_t)e * EG_STATES + k) * 7;
  const int vi = w.e_i[e], vj = w.e_j[e];
  OsSim3 C, Si, Sj;
  eg_load(w.meas + 8 * (size_t)e, &C);
  eg_load(est + 8 * (size_t)vi, &Si);
  eg_load(est + 8 * (size_t)vj, &Sj);
  if (k > 0) {
    const int side = (k - 1) / 14, dim = ((k - 1) % 14) >> 1;
    if ((side ? vj : vi) == w.fixed) {
#pragma unroll
      for (int c = 0; c < 7; c++) out[c] = 0.0;
      return;
    }
    double u[7];
#pragma unroll
    for (int c = 0; c < 7; c++) u[c] = c == dim ? (((k - 1) & 1) ? -1e-9 : 1e-9) : 0.0;
    unsigned unused = 0;
    OsSim3 P;
    os_oplus(u, w.fix_scale != 0, side ? Sj : Si, &P, &unused);
    if (side) Sj = P;
    else Si = P;
  }
  double err[7];
  eg_error(C, Si, Sj, err);
#pragma unroll
  for (int c = 0; c < 7; c++) out[c] = err[c];
  if (k == 0) w.e_chi[e] = eg_chi2(err);
}

// Entry c (0 .. 13: 7 side + d) of row k of the edge's Jacobian: (1 / (2 delta)) * (e+ - e-)
PO_HD inline double eg_jac(const double* st, int k, int c) {
  const double scalar = 1.0 / (2 * 1e-9);
  return scalar * (st[(1 + 2 * c) * 7 + k] - st[(2 + 2 * c) * 7 + k]);
}

// Entry idx of the edge's constructQuadraticForm products from its 7 x 14 Jacobian J (row k at J[14 k]).
// EIGEN: (J^T J)_rc = sum_k J_kr J_kc, b_r = sum_k J_kr (-e_k), k ascending, left to right.
PO_HD inline double eg_product(const double* J, const double* err, int idx) {
  int a, b = -1;
  if (idx < 49) a = idx / 7, b = idx % 7;
  else if (idx < 98) a = 7 + (idx - 49) / 7, b = 7 + (idx - 49) % 7;
  else if (idx < 147) a = (idx - 98) / 7, b = 7 + (idx - 98) % 7;
  else a = idx - 147;
  double s = b >= 0 ? J[a] * J[b] : J[a] * -err[0];
  for (int k = 1; k < 7; k++) s = b >= 0 ? s + J[14 * k + a] * J[14 * k + b] : s + J[14 * k + a] * -err[k];
  return s;
}

// ---- assembly -----------------------------------------------------------------------------------------
// Entry idx of slot s's diagonal block (0 .. 48) or of b_s (49 .. 55)
PO_HD inline void eg_diag_entry(const EgWs& w, int s, int idx) {
  double acc = 0.0;
  for (int it = w.ve_begin[s]; it < w.ve_begin[s + 1]; it++) {
    const int ent = w.ve_edge[it], e = ent >> 1, side = ent & 1;
    const double* o = w.e_prod + EG_EDGE_DOUBLES * (size_t)e;
    acc = acc + (idx < 49 ? o[49 * side + idx] : o[147 + 7 * side + (idx - 49)]);
  }
  if (idx < 49) w.H[((size_t)w.row_off[s + 1] - 1) * 49 + idx] = acc;
  else w.b[7 * (size_t)s + (idx - 49)] = acc;
}

// Entry idx of off-diagonal block o (row: the later slot): H_ij = Ji^T Jj, read transposed when the
// edge's vertex 0 is the earlier slot
PO_HD inline void eg_offdiag_entry(const EgWs& w, int o, int idx) {
  const int r = idx / 7, c = idx % 7;
  double acc = 0.0;
  for (int it = w.ob_begin[o]; it < w.ob_begin[o + 1]; it++) {
    const int ent = w.ob_edge[it], e = ent >> 1;
    acc = acc + w.e_prod[EG_EDGE_DOUBLES * (size_t)e + 98 + ((ent & 1) ? 7 * c + r : idx)];
  }
  w.H[(size_t)w.ob_pos[o] * 49 + idx] = acc;
}

// setLambda on a copy: L = H, then + lambda on slot s's diagonal entry r
PO_HD inline void eg_add_lambda(const EgWs& w, int s, int r, double lambda) {
  const size_t at = ((size_t)w.row_off[s + 1] - 1) * 49 + 8 * r;
  w.L[at] = w.H[at] + lambda;
}

// The envelope of the system as orbfe_env_core.h reads it: L is factored in place, y takes b before the
// forward substitution
PO_HD inline EnvWs eg_env(const EgWs& w) { return {w.ns, w.row_first, w.row_off, w.col_begin, w.col_row, w.L, w.d, w.y}; }

// ---- update, chi2, computeScale -----------------------------------------------------------------------
// SparseOptimizer::update into the trial estimate: oplus for a vertex in the system, a copy otherwise.
// oplusImpl zeroes the solver's x_6 in place with _fix_scale: computeScale reads it so.
PO_HD inline void eg_update_vertex(const EgWs& w, int v) {
  const int s = w.slot_of_v[v];
  OsSim3 S, o;
  eg_load(w.est + 8 * (size_t)v, &S);
  if (s < 0) {
    os_store_state(w.tri + 8 * (size_t)v, S);
    return;
  }
  double u[7];
#pragma unroll
  for (int k = 0; k < 7; k++) u[k] = w.x[7 * (size_t)s + k];
  unsigned flags = 0;
  os_oplus(u, w.fix_scale != 0, S, &o, &flags);
  w.x[7 * (size_t)s + 6] = u[6];
  os_store_state(w.tri + 8 * (size_t)v, o);
  lm_or(&w.rec->flags, flags);
}

PO_HD inline void eg_edge_chi(const EgWs& w, int e, const double* est) {
  OsSim3 C, Si, Sj;
  eg_load(w.meas + 8 * (size_t)e, &C);
  eg_load(est + 8 * (size_t)w.e_i[e], &Si);
  eg_load(est + 8 * (size_t)w.e_j[e], &Sj);
  double err[7];
  eg_error(C, Si, Sj, err);
  w.e_chi[e] = eg_chi2(err);
}

// One lane's part of the total chi2 (out[0]) and, with mode 1, of computeScale (out[1])
PO_HD inline void eg_reduce_lane(const EgWs& w, int lane, int mode, double lambda, double* out) {
  double chi = 0.0, sc = 0.0;
  for (int e = lane; e < w.ne; e += EG_LANES) chi = chi + w.e_chi[e];
  if (mode)
    for (int s = lane; s < w.ns; s += EG_LANES) {
      double v = 0.0;
      for (int j = 0; j < 7; j++) {
        const double x = w.x[7 * (size_t)s + j];
        v = v + x * (lambda * x + w.b[7 * (size_t)s + j]);
      }
      sc = sc + v;
    }
  out[0] = chi, out[1] = sc;
}

// ---- finish -------------------------------------------------------------------------------------------
// :997-1015: [R | t / s] narrowed as Converter::toCvSE3 narrows (eigt *= (1. / s))
PO_HD inline void eg_finish_vertex(const EgWs& w, int v) {
  OsSim3 S;
  eg_load(w.est + 8 * (size_t)v, &S);
  double m[9];
  po_quat_to_matrix(S.q, m);
  const double c = 1. / S.s;
  float* o = w.out_tcw + 12 * (size_t)v;
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) o[4 * r + k] = (float)m[3 * r + k];
    o[4 * r + 3] = (float)(S.t[r] * c);
  }
}

// :1036-1044: correctedSwr.map(Srw.map(P)), Srw the start estimate of the reference keyframe
PO_HD inline void eg_finish_point(const EgWs& w, int p) {
  const int v = w.p_ref[p];
  OsSim3 Srw, S, Swr;
  eg_load(w.scw + 8 * (size_t)v, &Srw);
  eg_load(w.est + 8 * (size_t)v, &S);
  os_sim3_inverse(S, &Swr);
  const double X[3] = {(double)w.xw[3 * (size_t)p], (double)w.xw[3 * (size_t)p + 1], (double)w.xw[3 * (size_t)p + 2]};
  double r[3], a[3], c[3];
  po_quat_rotate(Srw.q, X, r);
  for (int k = 0; k < 3; k++) a[k] = Srw.s * r[k] + Srw.t[k];
  po_quat_rotate(Swr.q, a, r);
  for (int k = 0; k < 3; k++) c[k] = Swr.s * r[k] + Swr.t[k];
  for (int k = 0; k < 3; k++) w.out_xw[3 * (size_t)p + k] = (float)c[k];
}

// ---- the host side: the plan, the Levenberg control flow, the host backend ----------------------------
struct EgIn {
  int nv, fixed, fix_scale;
  const float* tcw;
  int ncorr;
  const int* corr_idx;
  const double* corr;
  int nnonc;
  const int* nonc_idx;
  const double* nonc;
  int ne;
  const int* e_i;
  const int* e_j;
  const uint8_t* e_kind;
  int np;
  const float* xw;
  const int* p_ref;
};

struct EgOut {
  std::vector<float> tcw, xw;
  EgTrace trace;
};

struct EgPlan : EnvPlan {  // ns, nblk, row_first, row_off, col_begin, col_row
  int nv = 0, ne = 0, nob = 0, np = 0;
  std::vector<int> corr_of_v, nonc_of_v, slot_of_v, v_of_slot, ve_begin, ve_edge, ob_begin, ob_pos, ob_edge;
};

// The slots and the envelope: one pass over the edges, then env_plan_structure stopped at the count (a
// capacity of 0 blocks): the caller holds nblk against its own capacity before eg_plan_rest builds the
// rest. The indices of `in` are checked by the caller.
inline void eg_plan_envelope(const EgIn& in, EgPlan* P) {
  P->nv = in.nv, P->ne = in.ne, P->np = in.np;
  std::vector<uint8_t> used(in.nv, 0);
  for (int e = 0; e < in.ne; e++) used[in.e_i[e]] = used[in.e_j[e]] = 1;
  P->slot_of_v.assign(in.nv, -1), P->v_of_slot.clear();
  for (int v = 0; v < in.nv; v++)
    if (used[v] && v != in.fixed) P->slot_of_v[v] = (int)P->v_of_slot.size(), P->v_of_slot.push_back(v);
  P->ns = (int)P->v_of_slot.size();
  P->row_first.resize(P->ns);
  for (int s = 0; s < P->ns; s++) P->row_first[s] = s;
  for (int e = 0; e < in.ne; e++) {
    const int a = P->slot_of_v[in.e_i[e]], b = P->slot_of_v[in.e_j[e]];
    if (a < 0 || b < 0) continue;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo < P->row_first[hi]) P->row_first[hi] = lo;
  }
  env_plan_structure(P, 0);
}

// The rest of the structure; nblk fits the handle (checked by the caller between the two)
inline void eg_plan_rest(const EgIn& in, EgPlan* P) {
  const int ns = P->ns;
  env_plan_structure(P, P->nblk);
  P->corr_of_v.assign(in.nv, -1), P->nonc_of_v.assign(in.nv, -1);
  for (int k = 0; k < in.ncorr; k++) P->corr_of_v[in.corr_idx[k]] = k;
  for (int k = 0; k < in.nnonc; k++) P->nonc_of_v[in.nonc_idx[k]] = k;
  P->ve_begin.assign(ns + 1, 0);
  for (int e = 0; e < in.ne; e++) {
    const int a = P->slot_of_v[in.e_i[e]], b = P->slot_of_v[in.e_j[e]];
    if (a >= 0) P->ve_begin[a + 1]++;
    if (b >= 0) P->ve_begin[b + 1]++;
  }
  for (int s = 0; s < ns; s++) P->ve_begin[s + 1] += P->ve_begin[s];
  P->ve_edge.assign(P->ve_begin[ns], 0);
  std::vector<int> at(P->ve_begin.begin(), P->ve_begin.end() - 1);
  struct Ob {
    int hi, lo, ent;
  };
  std::vector<Ob> obs;
  for (int e = 0; e < in.ne; e++) {
    const int a = P->slot_of_v[in.e_i[e]], b = P->slot_of_v[in.e_j[e]];
    if (a >= 0) P->ve_edge[at[a]++] = 2 * e;
    if (b >= 0) P->ve_edge[at[b]++] = 2 * e + 1;
    if (a >= 0 && b >= 0) obs.push_back(a > b ? Ob{a, b, 2 * e} : Ob{b, a, 2 * e + 1});
  }
  std::stable_sort(obs.begin(), obs.end(), [](const Ob& x, const Ob& y) { return x.hi != y.hi ? x.hi < y.hi : x.lo < y.lo; });
  P->ob_begin.assign(1, 0), P->ob_pos.clear(), P->ob_edge.clear();
  for (size_t k = 0; k < obs.size(); k++) {
    if (k > 0 && (obs[k].hi != obs[k - 1].hi || obs[k].lo != obs[k - 1].lo)) P->ob_begin.push_back((int)k);
    if (k == 0 || obs[k].hi != obs[k - 1].hi || obs[k].lo != obs[k - 1].lo)
      P->ob_pos.push_back(P->row_off[obs[k].hi] + (obs[k].lo - P->row_first[obs[k].hi]));
    P->ob_edge.push_back(obs[k].ent);
  }
  if (!obs.empty()) P->ob_begin.push_back((int)obs.size());
  P->nob = (int)P->ob_pos.size();
}

// Optimizer.cc:784-1048 after the caller's gather: SparseOptimizer::optimize(20) by orbfe_lm_core.h's
// lm_host_optimize with setUserLambdaInit(1e-16) and no stop flag. A backend B supplies start, linearize,
// trial, accept and finish; each returns 0 or an error status that ends the run.
template <class B>
inline int eg_run(B& b, const EgIn& in, const EgPlan& P, EgOut* o) {
  o->tcw.assign(12 * (size_t)in.nv, 0.0f), o->xw.assign(3 * (size_t)in.np, 0.0f);
  const EgTrace none = {0, 0, 0, LM_STOP_NO_EDGE, 0.0, 0.0, (int)P.nblk, 0};
  o->trace = none;
  int st = 0;
  if ((st = b.start(in, P))) return st;
  if (in.ne > 0) {  // else _ivMap.size() == 0: optimize() returns -1 without a step
    LmTrace t;
    LmNoPoll poll;
    if ((st = lm_host_optimize(b, EG_MAX_ITER, 1e-16, poll, &t))) return st;
    const EgTrace r = {t.iterations, t.trials, t.rejected_trials, t.stop, t.lambda, t.chi2, (int)P.nblk, t.flags};
    o->trace = r;
  }
  return b.finish(o->tcw.data(), o->xw.data());
}

// The workspace in host memory, every stage a loop over the per-element functions
struct EgHostBackend {
  EgWs w;
  LmRec rec;
  std::vector<double> scw, mst, est, tri, meas, e_state, e_chi, e_prod, H, L, b, d, y, x;
  std::vector<float> out_tcw, out_xw;

  int start(const EgIn& in, const EgPlan& P) {
    memset(&w, 0, sizeof(w));
    const size_t nv = in.nv, ne = in.ne, ns = P.ns, nb = (size_t)P.nblk;
    scw.assign(8 * nv, 0.0), mst = scw, est = scw, tri = scw, meas.assign(8 * ne, 0.0);
    e_state.assign(EG_STATES * 7 * ne, 0.0), e_chi.assign(ne, 0.0), e_prod.assign(EG_EDGE_DOUBLES * ne, 0.0);
    H.assign(49 * nb, 0.0), L = H, b.assign(7 * ns, 0.0), d = b, y = b, x = b;  // deviation: x is zero before the first solve
    out_tcw.assign(12 * nv, 0.0f), out_xw.assign(3 * (size_t)in.np, 0.0f);
    w.nv = in.nv, w.ne = in.ne, w.ns = P.ns, w.nblk = (int)P.nblk, w.nob = P.nob, w.np = in.np;
    w.fix_scale = in.fix_scale, w.fixed = in.fixed;
    w.tcw = in.tcw, w.corr_of_v = P.corr_of_v.data(), w.nonc_of_v = P.nonc_of_v.data(), w.corr = in.corr, w.nonc = in.nonc;
    w.e_i = in.e_i, w.e_j = in.e_j, w.e_kind = in.e_kind, w.xw = in.xw, w.p_ref = in.p_ref;
    w.slot_of_v = P.slot_of_v.data(), w.v_of_slot = P.v_of_slot.data(), w.ve_begin = P.ve_begin.data();
    w.ve_edge = P.ve_edge.data(), w.row_first = P.row_first.data(), w.row_off = P.row_off.data();
    w.ob_begin = P.ob_begin.data(), w.ob_pos = P.ob_pos.data(), w.ob_edge = P.ob_edge.data();
    w.col_begin = P.col_begin.data(), w.col_row = P.col_row.data();
    w.scw = scw.data(), w.mst = mst.data(), w.est = est.data(), w.tri = tri.data(), w.meas = meas.data();
    w.e_state = e_state.data(), w.e_chi = e_chi.data(), w.e_prod = e_prod.data();
    w.H = H.data(), w.L = L.data(), w.b = b.data(), w.d = d.data(), w.y = y.data(), w.x = x.data();
    w.out_tcw = out_tcw.data(), w.out_xw = out_xw.data(), w.rec = &rec;
    for (int v = 0; v < w.nv; v++) eg_vertex_setup(w, v);
    for (int e = 0; e < w.ne; e++) eg_edge_setup(w, e);
    return 0;
  }

  void reduce(int mode, double lambda) {
    double part[EG_LANES][2];
    for (int l = 0; l < EG_LANES; l++) eg_reduce_lane(w, l, mode, lambda, part[l]);
    PoHostGroup().reduce(part);
    rec.chi = part[0][0], rec.scale = part[0][1];
  }

  int linearize(LmRec* out) {
    memset(&rec, 0, sizeof(rec));
    for (int e = 0; e < w.ne; e++) {
      for (int k = 0; k < EG_STATES; k++) eg_edge_state(w, e, k, w.est);
      const double* st = w.e_state + (size_t)e * EG_STATES * 7;
      double J[98];
      for (int k = 0; k < 7; k++)
        for (int c = 0; c < 14; c++) J[14 * k + c] = eg_jac(st, k, c);
      for (int idx = 0; idx < EG_EDGE_DOUBLES; idx++) e_prod[EG_EDGE_DOUBLES * (size_t)e + idx] = eg_product(J, st, idx);
    }
    for (double& v : H) v = 0.0;
    for (int s = 0; s < w.ns; s++)
      for (int idx = 0; idx < 56; idx++) eg_diag_entry(w, s, idx);
    for (int o = 0; o < w.nob; o++)
      for (int idx = 0; idx < 49; idx++) eg_offdiag_entry(w, o, idx);
    reduce(0, 0.0);
    *out = rec;
    return 0;
  }

  int trial(double lambda, LmRec* out) {
    memset(&rec, 0, sizeof(rec));
    const int n = 7 * w.ns;
    L = H;
    w.L = L.data();
    for (int s = 0; s < w.ns; s++)
      for (int r = 0; r < 7; r++) eg_add_lambda(w, s, r, lambda);
    // a d_j that is 0, or not finite (deviation), fails the trial
    const EnvWs env = eg_env(w);
    for (int b = 0; b < w.ns; b++) {
      double sD[49];
      const int bad = env_pivot_diag<7>(env, b, sD);
      if (bad) {
        lm_fail(w.rec, bad == 2 ? LM_FLAG_NONFINITE : 0u);
        break;
      }
      const int nr = env.col_begin[b + 1] - env.col_begin[b];
      for (int t = 0; t < 7 * nr; t++) env_scale_row<7>(env, b, t, sD, env.d + 7 * b);
      const long long items = env_trailing_items(env, b, 7);
      for (long long t = 0; t < items; t++) env_trailing_item<7>(env, b, t, env.d + 7 * b);
    }
    if (!rec.fail) {
      for (int i = 0; i < n; i++) w.y[i] = w.b[i];
      for (int b = 0; b < w.ns; b++) {
        env_forward_diag<7>(env, b);
        const int nr = env.col_begin[b + 1] - env.col_begin[b];
        for (int t = 0; t < 7 * nr; t++) env_forward_row<7>(env, b, t);
      }
      for (int i = 0; i < n; i++) w.y[i] = w.y[i] / w.d[i];
      for (int s = w.ns - 1; s >= 0; s--) {
        env_backward_diag<7>(env, s);
        for (int t = 0; t < 7 * (s - env.row_first[s]); t++) env_backward_col<7>(env, s, t);
      }
      for (int i = 0; i < n; i++) w.x[i] = w.y[i];
    }
    for (int v = 0; v < w.nv; v++) eg_update_vertex(w, v);
    for (int e = 0; e < w.ne; e++) eg_edge_chi(w, e, w.tri);
    const int fail = rec.fail;
    const uint32_t fl = rec.flags;
    reduce(1, lambda);
    rec.fail = fail, rec.flags = fl;
    *out = rec;
    return 0;
  }

  int accept() {
    est.swap(tri);
    w.est = est.data(), w.tri = tri.data();
    return 0;
  }

  int finish(float* tcw, float* xw) {
    for (int v = 0; v < w.nv; v++) eg_finish_vertex(w, v);
    for (int p = 0; p < w.np; p++) eg_finish_point(w, p);
    if (w.nv) memcpy(tcw, out_tcw.data(), 4 * out_tcw.size());
    if (w.np) memcpy(xw, out_xw.data(), 4 * out_xw.size());
    return 0;
  }
};
