// orbfe_poseopt_core.h -- Optimizer::PoseOptimization's arithmetic (Optimizer.cc:242-452 and the g2o
// routines under it: SE3Quat, the two *OnlyPose edges, RobustKernelHuber, BlockSolver's non-Schur path)
// as host/device inline functions. OptimizationAlgorithmLevenberg's decisions (LmCtl), LinearSolverDense's
// LDLT (lm_ldlt<6>), the lane group and the flag and stop codes are orbfe_lm_core.h's. Used by k_poseopt in
// orbfe_poseopt.hip and by the stand-alone host program tests/cpp/poseopt_core_main.cpp. Not part of
// the C ABI.
//
// Every operation is an IEEE double (or float) + - * / sqrt, rounded separately (-ffp-contract=off).
// No libm transcendental: sin / cos of SE3Quat::exp are restated below (po_sincos), pow(x, 3) is
// a product (orbfe_lm_core.h). Every Eigen operation is restated by the rule DESIGN.md section 18 records, marked
// "EIGEN:"; tests/poseopt_ref.py is the same code in Python, line by line.
//
// A problem is run by a group of PO_LANES lanes. Edge i (the frame's keypoint index) belongs to lane
// i % PO_LANES; a lane adds its active edges in ascending i into accumulators that start at +0.0 and
// the lanes are combined by s[l] += s[l + stride], stride = 32 .. 1. A group type G runs G::width of
// the lanes at once and G::slots = PO_LANES / G::width of them one after the other (the device: 64 and
// 1, the host: 1 and 64). Every Levenberg decision is taken on values that are identical in all lanes,
// so control flow is uniform; every loop has a fixed cap (4 rounds, 10 iterations, 10 trials, 6 pivots,
// ceil(n / 64) edges per lane) and no computed value forms an address.
#pragma once
#include "orbfe_lm_core.h"
#include "orbfe_stage.h"

#define PO_ACC 28  // 21 lower entries of H (row-major over r >= c), 6 of b, the robust chi2

struct PoSE3 {
  double q[4];  // x y z w
  double t[3];
};

// One problem as the kernel sees it: the frame's arrays and the camera widened to double.
struct PoProblem {
  int n;
  const uint8_t* valid;
  const float* xw;
  const float* kp;
  const float* ur;
  const float* inv_sigma2;
  double fx, fy, cx, cy, bf;
  const float* tcw;  // [12]
};

struct PoEdge {
  double X[3], obs[3], w, delta, dsqr;
  bool stereo;
};

struct PoOut {
  float tcw[12];
  double pose[7];
  int32_t n_initial, n_bad, n_inliers, rounds_run;
  uint32_t flags, pad;
  PoRound rounds[4];
};

// The solve's working set: LDS on the device, so the pivot indices may address it.
struct PoWork {
  double A[36], x[6], rhs[6], temp[6];
  int tr[6];
  int positive;
};

// ---- sin / cos from + - * / ------------------------------------------------------------------------
// sin(x + y) on [-pi/4, pi/4], y the tail of x
PO_HD inline double po_kernel_sin(double x, double y) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double z = x * x;
  const double w = z * z;
  const double r = (S2 + z * (S3 + z * S4)) + (z * w) * (S5 + z * S6);
  const double v = z * x;
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

// cos(x + y) on [-pi/4, pi/4]: the 1 - z/2 step compensated
PO_HD inline double po_kernel_cos(double x, double y) {
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double z = x * x;
  double w = z * z;
  const double r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
  const double hz = 0.5 * z;
  w = 1.0 - hz;
  return w + (((1.0 - w) - hz) + (z * r - x * y));
}

// Deviation: replaces libm's sin / cos. Cody-Waite reduction by pi/2 with the constant split in pieces
// of 33 bits (k * piece is exact for a small k; each subtraction's rounding error is carried into a
// tail), then the kernels by quadrant. Defined for every finite theta: above pi it sets LM_FLAG_LARGE_STEP,
// from 2^31 on it returns (0, 1). A non-finite theta gives NaN.
PO_HD inline void po_sincos(double theta, double* sn, double* cs, unsigned* flags) {
  const double nan = theta - theta;  // 0, or NaN for a non-finite theta
  if (nan != 0.0) {
    *sn = *cs = nan;
    return;
  }
  if (theta > 3.141592653589793) *flags |= LM_FLAG_LARGE_STEP;
  if (!(theta < 2147483648.0 && theta > -2147483648.0)) {
    *sn = 0.0;
    *cs = 1.0;
    return;
  }
  const long long kk = (long long)(theta * 6.36619772367581382433e-01 + 0.5);
  const double k = (double)kk;
  const double r0 = theta - k * 1.57079632673412561417e+00;
  const double w1 = k * 6.07710050630396597660e-11;
  const double r1 = r0 - w1;
  const double e1 = (r0 - r1) - w1;
  const double w2 = k * 2.02226624871116645580e-21;
  const double r2 = r1 - w2;
  const double e2 = (r1 - r2) - w2;
  const double tail = (e1 + e2) - k * 8.47842766036889956997e-32;
  const double r = r2 + tail;
  const double y = (r2 - r) + tail;
  const double s = po_kernel_sin(r, y), c = po_kernel_cos(r, y);
  const int q = (int)(kk & 3);
  *sn = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
  *cs = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}

// ---- Eigen's quaternion and 3x3 operations ---------------------------------------------------------
template <int I>
PO_HD inline void po_quat_diag(const double* m, double* q) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double t = sqrt(m[4 * I] - m[4 * J] - m[4 * K] + 1.0);
  q[I] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (m[3 * K + J] - m[3 * J + K]) * t;
  q[J] = (m[3 * J + I] + m[3 * I + J]) * t;
  q[K] = (m[3 * K + I] + m[3 * I + K]) * t;
}

// EIGEN: Quaterniond(Matrix3d): the trace branch if the trace is > 0, else the branch of the largest
// diagonal entry (a later entry wins only if strictly greater)
PO_HD inline void po_quat_from_matrix(const double* m, double* q) {
  double t = m[0] + m[4] + m[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    const bool one = m[4] > m[0];
    const bool two = m[8] > (one ? m[4] : m[0]);
    if (two) po_quat_diag<2>(m, q);
    else if (one) po_quat_diag<1>(m, q);
    else po_quat_diag<0>(m, q);
  }
}

// SE3Quat::normalizeRotation: w < 0 flips every coefficient, then
// EIGEN: normalize() divides each coefficient by sqrt(((x^2 + y^2) + z^2) + w^2) when that sum is > 0
PO_HD inline void po_normalize_rotation(double* q) {
  if (q[3] < 0) {
    q[0] = q[0] * -1.0, q[1] = q[1] * -1.0, q[2] = q[2] * -1.0, q[3] = q[3] * -1.0;
  }
  const double z = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  if (z > 0.0) {
    const double nrm = sqrt(z);
    q[0] = q[0] / nrm, q[1] = q[1] / nrm, q[2] = q[2] / nrm, q[3] = q[3] / nrm;
  }
}

// EIGEN: cross()
PO_HD inline void po_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// EIGEN: Quaterniond * Vector3d: uv = qv x v; uv += uv; v + w * uv + qv x uv
PO_HD inline void po_quat_rotate(const double* q, const double* v, double* o) {
  double uv[3], c2[3];
  po_cross(q, v, uv);
  uv[0] = uv[0] + uv[0], uv[1] = uv[1] + uv[1], uv[2] = uv[2] + uv[2];
  po_cross(q, uv, c2);
  o[0] = (v[0] + q[3] * uv[0]) + c2[0];
  o[1] = (v[1] + q[3] * uv[1]) + c2[1];
  o[2] = (v[2] + q[3] * uv[2]) + c2[2];
}

// EIGEN: the scalar quaternion product, term by term
PO_HD inline void po_quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// EIGEN: toRotationMatrix()
PO_HD inline void po_quat_to_matrix(const double* q, double* m) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  m[0] = 1.0 - (tyy + tzz), m[1] = txy - twz, m[2] = txz + twy;
  m[3] = txy + twz, m[4] = 1.0 - (txx + tzz), m[5] = tyz - twx;
  m[6] = txz - twy, m[7] = tyz + twx, m[8] = 1.0 - (txx + tyy);
}

// Converter::toSE3Quat: float -> double, SE3Quat(R, t)
PO_HD inline void po_se3_from_tcw(const float* tcw, PoSE3* T) {
  double m[9];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) m[3 * i + j] = (double)tcw[4 * i + j];
    T->t[i] = (double)tcw[4 * i + 3];
  }
  po_quat_from_matrix(m, T->q);
  po_normalize_rotation(T->q);
}

// SE3Quat::exp. EIGEN: a 3x3 product sums k ascending.
PO_HD inline void po_se3_exp(const double* u, PoSE3* T, unsigned* flags) {
  const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double O[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
  const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double O2[9], R[9], V[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
  if (theta < 0.00001) {
#pragma unroll
    for (int i = 0; i < 9; i++) V[i] = R[i] = (I[i] + O[i]) + O2[i];
  } else {
    double s, c;
    po_sincos(theta, &s, &c, flags);
    const double a = s / theta;
    const double b = (1.0 - c) / (theta * theta);
    const double d = (theta - s) / (theta * theta * theta);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      R[i] = (I[i] + a * O[i]) + b * O2[i];
      V[i] = (I[i] + b * O[i]) + d * O2[i];
    }
  }
  po_quat_from_matrix(R, T->q);
  po_normalize_rotation(T->q);
#pragma unroll
  for (int r = 0; r < 3; r++) T->t[r] = (V[3 * r] * u[3] + V[3 * r + 1] * u[4]) + V[3 * r + 2] * u[5];
}

// SE3Quat::operator*: t = a.t + a.q * b.t; q = a.q * b.q; normalizeRotation
PO_HD inline void po_se3_mul(const PoSE3& a, const PoSE3& b, PoSE3* o) {
  double r[3];
  po_quat_rotate(a.q, b.t, r);
  po_quat_mul(a.q, b.q, o->q);
  po_normalize_rotation(o->q);
  o->t[0] = a.t[0] + r[0], o->t[1] = a.t[1] + r[1], o->t[2] = a.t[2] + r[2];
}

PO_HD inline void po_se3_map(const PoSE3& T, const double* X, double* p) {
  double r[3];
  po_quat_rotate(T.q, X, r);
  p[0] = r[0] + T.t[0], p[1] = r[1] + T.t[1], p[2] = r[2] + T.t[2];
}

// ---- one edge --------------------------------------------------------------------------------------
PO_HD inline void po_load_edge(const PoProblem& P, int i, PoEdge* e) {
  const float ur = P.ur[i];
  e->stereo = !(ur < 0);  // mvuRight[i] < 0: monocular
  e->X[0] = (double)P.xw[3 * (size_t)i], e->X[1] = (double)P.xw[3 * (size_t)i + 1], e->X[2] = (double)P.xw[3 * (size_t)i + 2];
  e->obs[0] = (double)P.kp[2 * (size_t)i], e->obs[1] = (double)P.kp[2 * (size_t)i + 1], e->obs[2] = (double)ur;
  e->w = (double)P.inv_sigma2[i];
  e->delta = e->stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991);  // const float delta..., setDelta widens
  e->dsqr = e->delta * e->delta;
}

// computeError of the two *OnlyPose edges: obs - cam_project(T.map(Xw)); p = T.map(Xw)
PO_HD inline void po_edge_error(const PoProblem& P, const PoEdge& e, const PoSE3& T, double* p, double* err) {
  po_se3_map(T, e.X, p);
  if (e.stereo) {
    const double invz = (double)(float)(1.0 / p[2]);  // const float invz = 1.0f / z: divided in double, narrowed
    const double r0 = p[0] * invz * P.fx + P.cx;
    const double r1 = p[1] * invz * P.fy + P.cy;
    const double r2 = r0 - P.bf * invz;
    err[0] = e.obs[0] - r0, err[1] = e.obs[1] - r1, err[2] = e.obs[2] - r2;
  } else {
    const double r0 = p[0] / p[2] * P.fx + P.cx;  // project2d divides in double
    const double r1 = p[1] / p[2] * P.fy + P.cy;
    err[0] = e.obs[0] - r0, err[1] = e.obs[1] - r1, err[2] = 0.0;
  }
}

// EIGEN: _error.dot(information() * _error) with a diagonal information: sum_k e_k * (w * e_k)
PO_HD inline double po_edge_chi2(const PoEdge& e, const double* err) {
  double s = err[0] * (e.w * err[0]) + err[1] * (e.w * err[1]);
  if (e.stereo) s = s + err[2] * (e.w * err[2]);
  return s;
}

// computeError + activeRobustChi2's term and, with FULL, linearizeOplus + constructQuadraticForm of one
// active edge into a lane's accumulators.
// EIGEN: b_r -= sum_k ((rho1 * A_kr) * w) * e_k (without a kernel: (A_kr * w) * e_k);
//        H_rc += sum_k (A_kr * (rho1 * w)) * A_kc (without: A_kr * w), lower triangle only.
template <bool FULL>
PO_HD inline void po_edge_accumulate(double* acc, const PoProblem& P, const PoEdge& e, const PoSE3& T, bool kernel_on) {
  double p[3], err[3];
  po_edge_error(P, e, T, p, err);
  const double chi2 = po_edge_chi2(e, err);
  double rho0 = chi2, rho1 = 1.0;
  if (kernel_on && !(chi2 <= e.dsqr)) {  // RobustKernelHuber::robustify
    const double sq = sqrt(chi2);
    rho0 = 2 * sq * e.delta - e.dsqr;
    rho1 = e.delta / sq;
  }
  acc[27] = acc[27] + rho0;
  if (!FULL) return;
  const double x = p[0], y = p[1];
  const double invz = 1.0 / p[2];
  const double invz_2 = invz * invz;
  const double fx = P.fx, fy = P.fy, bf = P.bf;
  double J[18];
  J[0] = x * y * invz_2 * fx;
  J[1] = -(1 + (x * x * invz_2)) * fx;
  J[2] = y * invz * fx;
  J[3] = -invz * fx;
  J[4] = 0.0;
  J[5] = x * invz_2 * fx;
  J[6] = (1 + y * y * invz_2) * fy;
  J[7] = -x * y * invz_2 * fy;
  J[8] = -x * invz * fy;
  J[9] = 0.0;
  J[10] = -invz * fy;
  J[11] = y * invz_2 * fy;
  J[12] = J[0] - bf * y * invz_2;
  J[13] = J[1] + bf * x * invz_2;
  J[14] = J[2];
  J[15] = J[3];
  J[16] = 0.0;
  J[17] = J[5] - bf * invz_2;
  const double ww = kernel_on ? rho1 * e.w : e.w;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double s;
    if (kernel_on) {
      s = ((rho1 * J[r]) * e.w) * err[0];
      s = s + ((rho1 * J[6 + r]) * e.w) * err[1];
      if (e.stereo) s = s + ((rho1 * J[12 + r]) * e.w) * err[2];
    } else {
      s = (J[r] * e.w) * err[0];
      s = s + (J[6 + r] * e.w) * err[1];
      if (e.stereo) s = s + (J[12 + r] * e.w) * err[2];
    }
    acc[21 + r] = acc[21 + r] - s;
#pragma unroll
    for (int c = 0; c <= r; c++) {
      double h = (J[r] * ww) * J[c];
      h = h + (J[6 + r] * ww) * J[6 + c];
      if (e.stereo) h = h + (J[12 + r] * ww) * J[12 + c];
      acc[r * (r + 1) / 2 + c] = acc[r * (r + 1) / 2 + c] + h;
    }
  }
}

// The sums over the active edges (valid and not flagged) at pose T: s[0] holds them in every lane.
// out[slot]: bit c = the outlier flag of edge (slot * width + lane) + 64 c.
template <bool FULL, class G>
PO_HD inline void po_sums(const G& g, const PoProblem& P, const uint64_t* out, const PoSE3& T, bool kernel_on,
                          double (*s)[FULL ? PO_ACC : 1]) {
  for (int slot = 0; slot < G::slots; slot++) {
    const int vl = slot * G::width + g.lane();
    double acc[PO_ACC];
#pragma unroll
    for (int k = 0; k < PO_ACC; k++) acc[k] = 0.0;
    int c = 0;
    for (int i = vl; i < P.n; i += PO_LANES, c++) {  // at most ceil(n / 64) <= 64 edges
      if (!P.valid[i] || ((out[slot] >> c) & 1ull)) continue;
      PoEdge e;
      po_load_edge(P, i, &e);
      po_edge_accumulate<FULL>(acc, P, e, T, kernel_on);
    }
    if (FULL) {
#pragma unroll
      for (int k = 0; k < PO_ACC; k++) s[slot][k] = acc[k];
    } else {
      s[slot][0] = acc[27];
    }
  }
  g.reduce(s);
}

// ---- PoseOptimization ------------------------------------------------------------------------------
// mask: ceil(n / 64) words, bit i % 64 of word i / 64 = mvbOutlier[i]. Lane 0 writes o and mask.
template <class G>
PO_HD inline void po_optimize(const G& g, const PoProblem& P, PoWork& w, PoOut* o, uint64_t* mask) {
  const int lane = g.lane();
  const int words = (P.n + 63) / 64;
  uint64_t out[G::slots], val[G::slots];
  for (int slot = 0; slot < G::slots; slot++) {
    const int vl = slot * G::width + lane;
    uint64_t v = 0;
    int c = 0;
    for (int i = vl; i < P.n; i += PO_LANES, c++)
      if (P.valid[i]) v |= 1ull << c;
    val[slot] = v;
    out[slot] = 0;
  }
  int n_initial = 0;
  for (int c = 0; c < words; c++) n_initial += (int)__builtin_popcountll(g.ballot(val, c));
  PoSE3 T0, est, eval;
  po_se3_from_tcw(P.tcw, &T0);
  est = T0;
  unsigned flags = 0;
  int n_bad = 0, rounds_run = 0;
  if (lane == 0)
    for (int it = 0; it < 4; it++) {
      PoRound z = {0, 0, 0, 0, 0, 0, 0.0, 0.0};
      o->rounds[it] = z;
    }
  const int n_rounds = n_initial < 3 ? 0 : (n_initial < 10 ? 1 : 4);  // :365, :441: edges().size() counts all edges
  for (int it = 0; it < n_rounds; it++) {
    est = T0;  // :378: every round restarts from the frame's pose
    eval = est;
    const bool kernel_on = it < 3;  // :408: the kernel is removed after round 2
    int n_active = 0;
    for (int c = 0; c < words; c++) n_active += (int)__builtin_popcountll(g.ballot(val, c) & ~g.ballot(out, c));
    int iterations = 0, trials = 0, rejected = 0, stop = LM_STOP_ALL;
    LmCtl lm = {0.0, 0.0, 0.0, 2.0, 0.0, 0, 0};
    if (n_active == 0) {
      stop = LM_STOP_NO_EDGE;
    } else {
      g.sync();
      if (lane == 0)
        for (int j = 0; j < 6; j++) w.x[j] = 0.0;  // deviation: zero before a round's first successful solve
      g.sync();
      for (int i = 0; i < 10; i++) {
        iterations++;
        double S[G::slots][PO_ACC];
        po_sums<true>(g, P, out, est, kernel_on, S);
        const double* s = S[0];
        double lambda_init = 0.0;
        if (i == 0) {
          double mx = 0.0;
#pragma unroll
          for (int j = 0; j < 6; j++) {
            const double a = fabs(s[j * (j + 1) / 2 + j]);
            mx = a < mx ? mx : a;  // std::max(fabs(H_jj), maxDiagonal)
          }
          lambda_init = 1e-5 * mx;
        }
        lm_begin_iteration(lm, s[27], i == 0, lambda_init);
        do {
          const double lambda = lm.lambda;
          // setLambda + LinearSolverDense::solve. Deviation: a non-finite entry gives ok2 = false
          bool ok2 = true;
#pragma unroll
          for (int k = 0; k < 27; k++) ok2 = ok2 && po_finite(s[k]);
          ok2 = ok2 && po_finite(lambda);
#pragma unroll
          for (int j = 0; j < 6; j++) ok2 = ok2 && po_finite(s[j * (j + 1) / 2 + j] + lambda);
          if (!ok2) flags |= LM_FLAG_NONFINITE;
          g.sync();
          if (lane == 0 && ok2) {
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
              for (int c = 0; c <= r; c++) w.A[6 * r + c] = r == c ? s[r * (r + 1) / 2 + c] + lambda : s[r * (r + 1) / 2 + c];
              w.rhs[r] = s[21 + r];
            }
            w.positive = lm_ldlt<6>(w.A, w.tr, w.temp) ? 1 : 0;
            if (w.positive) lm_ldlt_solve<6>(w.A, w.tr, w.rhs, w.x);
          }
          g.sync();
          ok2 = ok2 && w.positive != 0;
          double x[6];
#pragma unroll
          for (int j = 0; j < 6; j++) x[j] = w.x[j];
          PoSE3 d, trial;
          po_se3_exp(x, &d, &flags);
          po_se3_mul(d, est, &trial);
          eval = trial;
          double C[G::slots][1];
          po_sums<false>(g, P, out, trial, kernel_on, C);
          double scale = 0.0;
#pragma unroll
          for (int j = 0; j < 6; j++) scale = scale + x[j] * (lambda * x[j] + s[21 + j]);
          trials++;
          if (lm_trial(lm, C[0][0], !ok2, scale)) est = trial;
          else rejected++;
        } while (lm_more_trials(lm));
        stop = lm_end_iteration(lm);
        if (stop != LM_STOP_ALL) break;
      }
    }
    // :383-439: an edge flagged before is recomputed at the final estimate, an active one keeps the
    // error of the last evaluated trial, accepted or not
    for (int slot = 0; slot < G::slots; slot++) {
      const int vl = slot * G::width + lane;
      uint64_t nw = 0;
      int c = 0;
      for (int i = vl; i < P.n; i += PO_LANES, c++) {
        if (!P.valid[i]) continue;
        PoEdge e;
        po_load_edge(P, i, &e);
        const bool flagged = (out[slot] >> c) & 1ull;
        PoSE3 T;
#pragma unroll
        for (int k = 0; k < 4; k++) T.q[k] = flagged ? est.q[k] : eval.q[k];
#pragma unroll
        for (int k = 0; k < 3; k++) T.t[k] = flagged ? est.t[k] : eval.t[k];
        double p[3], err[3];
        po_edge_error(P, e, T, p, err);
        const float chi2 = (float)po_edge_chi2(e, err);
        if (chi2 > (e.stereo ? 7.815f : 5.991f)) nw |= 1ull << c;
      }
      out[slot] = nw;
    }
    n_bad = 0;
    for (int c = 0; c < words; c++) n_bad += (int)__builtin_popcountll(g.ballot(out, c));
    rounds_run = it + 1;
    if (lane == 0) {
      PoRound r = {n_active, iterations, trials, rejected, stop, n_bad, lm.lambda, lm.current};
      o->rounds[it] = r;
    }
  }
  for (int c = 0; c < words; c++) {
    const uint64_t word = g.ballot(out, c);
    if (lane == 0) mask[c] = word;
  }
  if (lane == 0) {
    if (n_rounds == 0) {
      for (int i = 0; i < 12; i++) o->tcw[i] = P.tcw[i];
    } else {
      double m[9];
      po_quat_to_matrix(est.q, m);  // to_homogeneous_matrix, narrowed by Converter::toCvMat
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o->tcw[4 * i + j] = (float)m[3 * i + j];
        o->tcw[4 * i + 3] = (float)est.t[i];
      }
    }
    for (int i = 0; i < 4; i++) o->pose[i] = est.q[i];
    for (int i = 0; i < 3; i++) o->pose[4 + i] = est.t[i];
    o->n_initial = n_initial;
    o->n_bad = n_bad;
    o->n_inliers = n_rounds == 0 ? 0 : n_initial - n_bad;
    o->rounds_run = rounds_run;
    o->flags = flags;
    o->pad = 0;
  }
}

// ------------------------------------------------------------------------------------------
// staging (host)

// One problem as the kernel sees it. in_* are byte offsets into the upload buffer, o_* into the result
// buffer.
struct PoDev {
  int n, pad;
  double cam[5];  // fx, fy, cx, cy, bf: float widened to double
  float tcw[12];
  unsigned long long in_valid, in_xw, in_kp, in_ur, in_is2, o_out, o_mask;
};

// The arrays of one problem with n observations, taken from the two blocks in the order the buffers hold
// them; fills d's offsets only. The one statement of the buffer plan: over counting blocks it sizes a
// handle (po_plan_bounds), over the real ones it places a batch.
inline void po_layout(OrbfeStage& in, OrbfeStage& res, size_t n, PoDev& d) {
  d.in_valid = in.take(n);
  d.in_xw = in.take(12 * n);
  d.in_kp = in.take(8 * n);
  d.in_ur = in.take(4 * n);
  d.in_is2 = in.take(4 * n);
  d.o_out = res.take(sizeof(PoOut));
  d.o_mask = res.take(8 * ((n + 63) / 64));
}

// A handle's buffer sizes: the record table and S problems at the bound
inline void po_plan_bounds(size_t S, size_t C, size_t* in_bytes, size_t* res_bytes) {
  OrbfeStage in, res;
  PoDev d;
  in.take(sizeof(PoDev) * S);
  for (size_t s = 0; s < S; s++) po_layout(in, res, C, d);
  *in_bytes = in.off, *res_bytes = res.off;
}
