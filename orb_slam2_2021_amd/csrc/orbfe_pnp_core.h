// orbfe_pnp_core.h -- PnPsolver's arithmetic (PnPsolver.cc:199-212, :318-349, :385-1009) as
// host/device inline functions: the sample selection, EPnP (compute_pose) and one point of
// CheckInliers. Used by k_pnp_hypotheses / k_pnp_refine / k_pnp_inliers in orbfe_pnp.hip and by the
// stand-alone host program tests/cpp/pnp_core_main.cpp. Not part of the C ABI.
//
// Every operation is an IEEE double (or float) + - * / sqrt, rounded separately (-ffp-contract=off);
// every OpenCV call is restated by the rule DESIGN.md section 17 records, and a rule recalled from
// OpenCV's source carries "OPENCV:".
//
// compute_pose is written for a group of G::width lanes that share one PnpWork: a lane takes the
// elements lane, lane + width, ... of every element-wise step, every lane forms a sum it needs in
// the reference's order on its own (no cross-lane reduction), and the short serial chains run on
// lane 0. Control flow between two g.sync() calls never depends on data, so all lanes of a group
// (and all groups that share a barrier) reach every sync. On the host the group is one lane.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNP_HD __host__ __device__
#else
#define PNP_HD
#endif
#include <stdint.h>

#include <cfloat>
#include <cmath>

#include "orbfe_stage.h"

#define PNP_FLAG_SVD_NULL 1u     /* == ORBFE_PNP_FLAG_SVD_NULL */
#define PNP_FLAG_QR_SINGULAR 2u  /* == ORBFE_PNP_FLAG_QR_SINGULAR */

struct PnpHostGroup {
  static constexpr int width = 1;
  PNP_HD int lane() const { return 0; }
  PNP_HD void sync() const {}
  PNP_HD bool all(bool b) const { return b; }
};

// One hypothesis' (or one refinement's) working set: LDS on the device. Every array that is indexed
// at run time lives here, so a kernel keeps none in scratch.
struct PnpWork {
  double At[144], Vt[144], W[12];  // MtM, then the 12x12 SVD: row r of At is ut + 12*r
  double sa[36], sv[36], sw[6];    // the small SVDs (3x3, and N x 6 with N <= 5)
  double cws[12], ccs[12], ci[9];
  double l[60], rho[6], dv[72];
  double b5[5], betas[4];
  double ga[24], gb[6], gx[4], a1[4], a2[4];
  double pc0[3], pw0[3], abt[9];
  double Rs[27], ts[9], err[3];
  unsigned flags;
  int sign;
};

// The four correspondences of one iteration: swap-remove on a fresh 0..n-1 list (:199-212), kept as
// the (at most three) slots that no longer hold their own index. Needs n >= 4 and
// 0 <= draw[i] <= n - 1 - i; every index returned is then in 0..n-1.
PNP_HD inline void pnp_select4(int n, const int* draw, int* idx) {
  int key0 = -1, val0 = 0, key1 = -1, val1 = 0, key2 = -1, val2 = 0;
  for (int i = 0; i < 4; i++) {
    const int r = draw[i], last = n - 1 - i;
    const int at_r = r == key2 ? val2 : (r == key1 ? val1 : (r == key0 ? val0 : r));
    const int back = last == key2 ? val2 : (last == key1 ? val1 : (last == key0 ? val0 : last));
    idx[i] = at_r;
    if (i == 0) key0 = r, val0 = back;
    if (i == 1) key1 = r, val1 = back;
    if (i == 2) key2 = r, val2 = back;
  }
}

// OPENCV: JacobiSVDImpl_<double> calls the double hypot; restated as the square root of the sum of squares
PNP_HD inline double pnp_hypot(double a, double b) { return sqrt(a * a + b * b); }

// OPENCV: JacobiSVDImpl_<double>(At, W, Vt, m, n, n1 = n, minval = DBL_MIN, eps = 10 * DBL_EPSILON).
// At holds n rows of m elements (the transposed input); on return row i of At is the i-th left
// singular vector, W the singular values in descending order, Vt the right singular vectors as rows.
// One-sided Jacobi, at most max(m, 30) sweeps, so a NaN matrix ends. i, j, k come from the loops.
// Deviation (PNP_FLAG_SVD_NULL): a row whose singular value is <= DBL_MIN is scaled by 0 as it stands
// instead of being refilled from OpenCV's RNG.
template <class G>
PNP_HD inline void pnp_jacobi_svd(const G& g, double* At, int astep, double* W, double* Vt, int vstep, int m, int n,
                                  unsigned* flags) {
  const int lane = g.lane();
  const double eps = DBL_EPSILON * 10;
  for (int i = lane; i < n; i += G::width) {
    double sd = 0;
    for (int k = 0; k < m; k++) {
      const double t = At[i * astep + k];
      sd += t * t;
    }
    W[i] = sd;
    for (int k = 0; k < n; k++) Vt[i * vstep + k] = 0;
    Vt[i * vstep + i] = 1;
  }
  g.sync();
  const int max_iter = m > 30 ? m : 30;
  const int mn = m > n ? m : n;
  bool done = false;
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
    for (int i = 0; i < n - 1; i++)
      for (int j = i + 1; j < n; j++) {
        double* Ai = At + i * astep;
        double* Aj = At + j * astep;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
        const bool rot = !done && !(fabs(p) <= eps * sqrt(a * b));
        double c = 0, s = 0;
        if (rot) {
          p *= 2;
          const double beta = a - b, gamma = pnp_hypot(p, beta);
          if (beta < 0) {
            const double delta = (gamma - beta) * 0.5;
            s = sqrt(delta / gamma);
            c = p / (gamma * s * 2);
          } else {
            c = sqrt((gamma + beta) / (gamma * 2));
            s = p / (gamma * c * 2);
          }
        }
        g.sync();  // every lane has read rows i and j
        if (rot)
          for (int k = lane; k < mn; k += G::width) {
            if (k < m) {
              const double t0 = c * Ai[k] + s * Aj[k];
              const double t1 = -s * Ai[k] + c * Aj[k];
              Ai[k] = t0;
              Aj[k] = t1;
            }
            if (k < n) {
              double* Vi = Vt + i * vstep;
              double* Vj = Vt + j * vstep;
              const double t0 = c * Vi[k] + s * Vj[k];
              const double t1 = -s * Vi[k] + c * Vj[k];
              Vi[k] = t0;
              Vj[k] = t1;
            }
          }
        g.sync();
        if (rot) {
          a = b = 0;
          for (int k = 0; k < m; k++) {
            a += Ai[k] * Ai[k];
            b += Aj[k] * Aj[k];
          }
          if (lane == 0) W[i] = a, W[j] = b;
          changed = true;
        }
        g.sync();
      }
    if (!changed) done = true;
    if (g.all(done)) break;
  }
  if (lane == 0) {
    for (int i = 0; i < n; i++) {
      double sd = 0;
      for (int k = 0; k < m; k++) {
        const double t = At[i * astep + k];
        sd += t * t;
      }
      W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {  // OPENCV: descending selection sort, first maximum wins
      int j = i;
      for (int k = i + 1; k < n; k++)
        if (W[j] < W[k]) j = k;
      if (i != j) {
        double tmp = W[i];
        W[i] = W[j];
        W[j] = tmp;
        for (int k = 0; k < m; k++) tmp = At[i * astep + k], At[i * astep + k] = At[j * astep + k], At[j * astep + k] = tmp;
        for (int k = 0; k < n; k++) tmp = Vt[i * vstep + k], Vt[i * vstep + k] = Vt[j * vstep + k], Vt[j * vstep + k] = tmp;
      }
    }
    for (int i = 0; i < n; i++) {
      const double sd = W[i];
      if (sd <= DBL_MIN) *flags |= PNP_FLAG_SVD_NULL;
      const double s = sd > DBL_MIN ? 1 / sd : 0.;
      for (int k = 0; k < m; k++) At[i * astep + k] *= s;
    }
  }
  g.sync();
}

// OPENCV: SVBkSbImpl_<double>'s threshold: the sum of the singular values times 2 * DBL_EPSILON
PNP_HD inline double pnp_bksb_threshold(const double* w, int nm) {
  double threshold = 0;
  for (int i = 0; i < nm; i++) threshold += w[i];
  return threshold * (DBL_EPSILON * 2);
}

// OPENCV: cvSolve(A, b, x, CV_SVD) of a 6 x nn system after its SVD (sa: rows = left singular
// vectors, sv: Vt with stride nn): x += (u_i . b / w_i) * v_i for every w_i above the threshold
PNP_HD inline void pnp_solve_bksb(const PnpWork& w, int nn, double* x) {
  for (int j = 0; j < nn; j++) x[j] = 0;
  const double threshold = pnp_bksb_threshold(w.sw, nn);
  for (int i = 0; i < nn; i++) {
    double wi = w.sw[i];
    if (fabs(wi) <= threshold) continue;
    wi = 1 / wi;
    double s = 0;
    for (int j = 0; j < 6; j++) s += w.sa[6 * i + j] * w.rho[j];
    s *= wi;
    for (int j = 0; j < nn; j++) x[j] = x[j] + s * w.sv[nn * i + j];
  }
}

PNP_HD inline double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNP_HD inline double pnp_dist2(const double* p1, const double* p2) {
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// Element (row, col) of the 2n x 12 matrix fill_M (:448-464) builds. K = fu, fv, uc, vc.
PNP_HD inline double pnp_m_elem(const double* alphas, const double* us, const double* K, int row, int col) {
  const int i = row >> 1, h = row & 1, c = col / 3, d = col - 3 * c;
  const double as = alphas[4 * i + c];
  if (d == 2) return as * (K[2 + h] - us[2 * i + h]);
  if (d == h) return as * K[h];
  return 0.0;
}

// qr_solve (:903-1009) of the 6x4 system in w.ga / w.gb into w.gx. Returns false on its singular
// early return (:934-939), which leaves w.gx as it was.
PNP_HD inline bool pnp_qr_solve(PnpWork& w) {
  const int nr = 6, nc = 4;
  double* pA = w.ga;
  for (int k = 0; k < nc; k++) {
    // the scan as written: the pointer is advanced after the compare, so rows k .. nr-2 are seen
    double eta = fabs(pA[k * nc + k]);
    for (int i = k + 1; i < nr; i++) {
      const double elt = fabs(pA[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) {
      w.a1[k] = w.a2[k] = 0.0;
      return false;
    }
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; i++) {
      pA[i * nc + k] *= inv_eta;
      sum += pA[i * nc + k] * pA[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (pA[k * nc + k] < 0) sigma = -sigma;
    pA[k * nc + k] += sigma;
    w.a1[k] = sigma * pA[k * nc + k];
    w.a2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double s2 = 0;
      for (int i = k; i < nr; i++) s2 += pA[i * nc + k] * pA[i * nc + j];
      const double tau = s2 / w.a1[k];
      for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
    }
  }
  for (int j = 0; j < nc; j++) {  // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; i++) tau += pA[i * nc + j] * w.gb[i];
    tau /= w.a1[j];
    for (int i = j; i < nr; i++) w.gb[i] -= tau * pA[i * nc + j];
  }
  w.gx[nc - 1] = w.gb[nc - 1] / w.a2[nc - 1];  // X = R-1 b
  for (int i = nc - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * w.gx[j];
    w.gx[i] = (w.gb[i] - sum) / w.a2[i];
  }
  return true;
}

// gauss_newton (:882-901) on w.betas. Deviation (PNP_FLAG_QR_SINGULAR): x starts as 0, where the
// reference leaves it uninitialised until the first qr_solve that does not return early.
PNP_HD inline void pnp_gauss_newton(PnpWork& w) {
  for (int i = 0; i < 4; i++) w.gx[i] = 0.0;
  double* bt = w.betas;
  for (int k = 0; k < 5; k++) {
    for (int i = 0; i < 6; i++) {
      const double* rowL = w.l + i * 10;
      double* rowA = w.ga + i * 4;
      rowA[0] = 2 * rowL[0] * bt[0] + rowL[1] * bt[1] + rowL[3] * bt[2] + rowL[6] * bt[3];
      rowA[1] = rowL[1] * bt[0] + 2 * rowL[2] * bt[1] + rowL[4] * bt[2] + rowL[7] * bt[3];
      rowA[2] = rowL[3] * bt[0] + rowL[4] * bt[1] + 2 * rowL[5] * bt[2] + rowL[8] * bt[3];
      rowA[3] = rowL[6] * bt[0] + rowL[7] * bt[1] + rowL[8] * bt[2] + 2 * rowL[9] * bt[3];
      w.gb[i] = w.rho[i] - (rowL[0] * bt[0] * bt[0] + rowL[1] * bt[0] * bt[1] + rowL[2] * bt[1] * bt[1] +
                            rowL[3] * bt[0] * bt[2] + rowL[4] * bt[1] * bt[2] + rowL[5] * bt[2] * bt[2] +
                            rowL[6] * bt[0] * bt[3] + rowL[7] * bt[1] * bt[3] + rowL[8] * bt[2] * bt[3] +
                            rowL[9] * bt[3] * bt[3]);
    }
    if (!pnp_qr_solve(w)) w.flags |= PNP_FLAG_QR_SINGULAR;
    for (int i = 0; i < 4; i++) bt[i] += w.gx[i];
  }
}

// column r of L_6x10 that find_betas_approx_{1,2,3} (:692-795) copies into its system
PNP_HD inline int pnp_approx_col(int variant, int r) {
  if (variant == 1) return r == 2 ? 3 : (r == 3 ? 6 : r);
  return r;
}

// compute_pose (:492-540) over n correspondences. pws[3n] / us[2n] hold add_correspondence's doubles,
// alphas[4n] / pcs[3n] are work arrays, K = fu, fv, uc, vc. Lane 0 leaves R[9], t[3], the chosen N
// and the deviation flags; they are valid after the final sync.
template <class G>
PNP_HD inline void pnp_compute_pose(const G& g, PnpWork& w, int n, const double* pws, const double* us,
                                    double* alphas, double* pcs, const double* K, double* R, double* t, int* N_out,
                                    unsigned* flags_out) {
  const int lane = g.lane();
  if (lane == 0) w.flags = 0;
  // choose_control_points (:385-420): sums in row order
  for (int j = lane; j < 3; j += G::width) {
    double s = 0;
    for (int i = 0; i < n; i++) s += pws[3 * i + j];
    w.cws[j] = s / n;
  }
  g.sync();
  // OPENCV: cvMulTransposed(order = 1) on CV_64F: element (a, b), a <= b, is the double sum over the
  // rows in order, times scale 1; the lower triangle is copied from the upper
  for (int e = lane; e < 6; e += G::width) {
    const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e : (e < 5 ? e - 2 : 2);
    double s0 = 0;
    for (int i = 0; i < n; i++) s0 += (pws[3 * i + a] - w.cws[a]) * (pws[3 * i + b] - w.cws[b]);
    s0 = s0 * 1.0;
    w.sa[3 * a + b] = s0;
    w.sa[3 * b + a] = s0;
  }
  g.sync();
  // OPENCV: cvSVD(MODIFY_A | U_T): At = the transposed input; dc = W, row i of uct = row i of At
  pnp_jacobi_svd(g, w.sa, 3, w.sw, w.sv, 3, 3, 3, &w.flags);
  if (lane == 0) {
    for (int i = 1; i < 4; i++) {
      const double k = sqrt(w.sw[i - 1] / n);
      for (int j = 0; j < 3; j++) w.cws[3 * i + j] = w.cws[j] + k * w.sa[3 * (i - 1) + j];
    }
    // compute_barycentric_coordinates (:422-446): cc[3*i + j-1] = cws[j][i] - cws[0][i], transposed
    for (int i = 0; i < 3; i++)
      for (int j = 1; j < 4; j++) w.sa[3 * (j - 1) + i] = w.cws[3 * j + i] - w.cws[i];
  }
  g.sync();
  pnp_jacobi_svd(g, w.sa, 3, w.sw, w.sv, 3, 3, 3, &w.flags);
  if (lane == 0) {
    // OPENCV: cvInvert(CV_SVD) = SVD::backSubst without a right-hand side: inv[r][j] accumulates
    // Vt[i][r] * (U[j][i] * (1 / w_i)) over the w_i above the threshold, from 0
    for (int i = 0; i < 9; i++) w.ci[i] = 0;
    const double threshold = pnp_bksb_threshold(w.sw, 3);
    for (int i = 0; i < 3; i++) {
      double wi = w.sw[i];
      if (fabs(wi) <= threshold) continue;
      wi = 1 / wi;
      for (int r = 0; r < 3; r++) {
        const double s = w.sv[3 * i + r];
        for (int j = 0; j < 3; j++) w.ci[3 * r + j] = w.ci[3 * r + j] + s * (w.sa[3 * i + j] * wi);
      }
    }
  }
  g.sync();
  for (int i = lane; i < n; i += G::width) {
    const double* pi = pws + 3 * i;
    double* a = alphas + 4 * i;
    for (int j = 0; j < 3; j++)
      a[1 + j] = w.ci[3 * j] * (pi[0] - w.cws[0]) + w.ci[3 * j + 1] * (pi[1] - w.cws[1]) +
                 w.ci[3 * j + 2] * (pi[2] - w.cws[2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
  }
  g.sync();
  // MtM = cvMulTransposed(M, order = 1): 78 distinct entries, each the sum over M's 2n rows in order
  for (int e = lane; e < 78; e += G::width) {
    int a = 0, rem = e;
    while (rem >= 12 - a) rem -= 12 - a, a++;  // at most 11 steps
    const int b = a + rem;
    double s0 = 0;
    for (int r = 0; r < 2 * n; r++) s0 += pnp_m_elem(alphas, us, K, r, a) * pnp_m_elem(alphas, us, K, r, b);
    s0 = s0 * 1.0;
    w.At[12 * a + b] = s0;
    w.At[12 * b + a] = s0;
  }
  g.sync();
  pnp_jacobi_svd(g, w.At, 12, w.W, w.Vt, 12, 12, 12, &w.flags);
  const double* ut = w.At;
  if (lane == 0) {
    // compute_L_6x10 (:797-841), compute_rho (:843-851)
    for (int i = 0; i < 4; i++) {
      const double* v = ut + 12 * (11 - i);
      int a = 0, b = 1;
      for (int j = 0; j < 6; j++) {
        double* d = w.dv + 18 * i + 3 * j;
        d[0] = v[3 * a] - v[3 * b];
        d[1] = v[3 * a + 1] - v[3 * b + 1];
        d[2] = v[3 * a + 2] - v[3 * b + 2];
        b++;
        if (b > 3) a++, b = a + 1;
      }
    }
    for (int i = 0; i < 6; i++) {
      double* row = w.l + 10 * i;
      const double *d0 = w.dv + 3 * i, *d1 = w.dv + 18 + 3 * i, *d2 = w.dv + 36 + 3 * i, *d3 = w.dv + 54 + 3 * i;
      row[0] = pnp_dot(d0, d0);
      row[1] = 2.0f * pnp_dot(d0, d1);
      row[2] = pnp_dot(d1, d1);
      row[3] = 2.0f * pnp_dot(d0, d2);
      row[4] = 2.0f * pnp_dot(d1, d2);
      row[5] = pnp_dot(d2, d2);
      row[6] = 2.0f * pnp_dot(d0, d3);
      row[7] = 2.0f * pnp_dot(d1, d3);
      row[8] = 2.0f * pnp_dot(d2, d3);
      row[9] = pnp_dot(d3, d3);
    }
    w.rho[0] = pnp_dist2(w.cws, w.cws + 3);
    w.rho[1] = pnp_dist2(w.cws, w.cws + 6);
    w.rho[2] = pnp_dist2(w.cws, w.cws + 9);
    w.rho[3] = pnp_dist2(w.cws + 3, w.cws + 6);
    w.rho[4] = pnp_dist2(w.cws + 3, w.cws + 9);
    w.rho[5] = pnp_dist2(w.cws + 6, w.cws + 9);
  }
  g.sync();
  for (int variant = 1; variant <= 3; variant++) {
    const int nn = variant == 1 ? 4 : (variant == 2 ? 3 : 5);
    if (lane == 0)  // OPENCV: cvSolve(CV_SVD): At = the transposed 6 x nn system
      for (int r = 0; r < nn; r++)
        for (int i = 0; i < 6; i++) w.sa[6 * r + i] = w.l[10 * i + pnp_approx_col(variant, r)];
    g.sync();
    pnp_jacobi_svd(g, w.sa, 6, w.sw, w.sv, nn, 6, nn, &w.flags);
    if (lane == 0) {
      double* b = w.b5;
      double* betas = w.betas;
      pnp_solve_bksb(w, nn, b);
      if (variant == 1) {
        if (b[0] < 0) {
          betas[0] = sqrt(-b[0]);
          betas[1] = -b[1] / betas[0];
          betas[2] = -b[2] / betas[0];
          betas[3] = -b[3] / betas[0];
        } else {
          betas[0] = sqrt(b[0]);
          betas[1] = b[1] / betas[0];
          betas[2] = b[2] / betas[0];
          betas[3] = b[3] / betas[0];
        }
      } else {
        if (b[0] < 0) {
          betas[0] = sqrt(-b[0]);
          betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
        } else {
          betas[0] = sqrt(b[0]);
          betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
        }
        if (b[1] < 0) betas[0] = -betas[0];
        betas[2] = variant == 3 ? b[3] / betas[0] : 0.0;
        betas[3] = 0.0;
      }
      pnp_gauss_newton(w);
      // compute_ccs (:466-478)
      for (int i = 0; i < 12; i++) w.ccs[i] = 0.0f;
      for (int i = 0; i < 4; i++) {
        const double* v = ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
          for (int k = 0; k < 3; k++) w.ccs[3 * j + k] += betas[i] * v[3 * j + k];
      }
    }
    g.sync();
    // compute_pcs (:480-490)
    for (int i = lane; i < n; i += G::width) {
      const double* a = alphas + 4 * i;
      for (int j = 0; j < 3; j++)
        pcs[3 * i + j] = a[0] * w.ccs[j] + a[1] * w.ccs[3 + j] + a[2] * w.ccs[6 + j] + a[3] * w.ccs[9 + j];
    }
    g.sync();
    if (lane == 0) w.sign = pcs[2] < 0.0 ? 1 : 0;  // solve_for_sign (:659-674)
    g.sync();
    if (w.sign) {
      for (int i = lane; i < 12; i += G::width) w.ccs[i] = -w.ccs[i];
      for (int i = lane; i < 3 * n; i += G::width) pcs[i] = -pcs[i];
    }
    g.sync();
    // estimate_R_and_t (:586-650): sums in row order
    for (int e = lane; e < 6; e += G::width) {
      const double* src = e < 3 ? pcs : pws;
      const int j = e < 3 ? e : e - 3;
      double s = 0.0;
      for (int i = 0; i < n; i++) s += src[3 * i + j];
      s /= n;
      if (e < 3) w.pc0[j] = s; else w.pw0[j] = s;
    }
    g.sync();
    for (int e = lane; e < 9; e += G::width) {
      const int j = e / 3, c = e - 3 * j;
      double s = 0;  // cvSetZero
      for (int i = 0; i < n; i++) s += (pcs[3 * i + j] - w.pc0[j]) * (pws[3 * i + c] - w.pw0[c]);
      w.abt[e] = s;
    }
    g.sync();
    if (lane == 0)
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) w.sa[3 * r + c] = w.abt[3 * c + r];
    g.sync();
    // OPENCV: cvSVD(MODIFY_A) with U and V: U[i][k] = At[k][i], V[j][k] = Vt[k][j]
    pnp_jacobi_svd(g, w.sa, 3, w.sw, w.sv, 3, 3, 3, &w.flags);
    if (lane == 0) {
      double* Rv = w.Rs + 9 * (variant - 1);
      double* tv = w.ts + 3 * (variant - 1);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
          Rv[3 * i + j] = w.sa[i] * w.sv[j] + w.sa[3 + i] * w.sv[3 + j] + w.sa[6 + i] * w.sv[6 + j];
      const double det = Rv[0] * Rv[4] * Rv[8] + Rv[1] * Rv[5] * Rv[6] + Rv[2] * Rv[3] * Rv[7] -
                         Rv[2] * Rv[4] * Rv[6] - Rv[1] * Rv[3] * Rv[8] - Rv[0] * Rv[5] * Rv[7];
      if (det < 0) {
        Rv[6] = -Rv[6];
        Rv[7] = -Rv[7];
        Rv[8] = -Rv[8];
      }
      tv[0] = w.pc0[0] - pnp_dot(Rv, w.pw0);
      tv[1] = w.pc0[1] - pnp_dot(Rv + 3, w.pw0);
      tv[2] = w.pc0[2] - pnp_dot(Rv + 6, w.pw0);
      // reprojection_error (:566-584)
      double sum2 = 0.0;
      for (int i = 0; i < n; i++) {
        const double* pw = pws + 3 * i;
        const double Xc = pnp_dot(Rv, pw) + tv[0];
        const double Yc = pnp_dot(Rv + 3, pw) + tv[1];
        const double inv_Zc = 1.0 / (pnp_dot(Rv + 6, pw) + tv[2]);
        const double ue = K[2] + K[0] * Xc * inv_Zc;
        const double ve = K[3] + K[1] * Yc * inv_Zc;
        const double u = us[2 * i], v = us[2 * i + 1];
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
      }
      w.err[variant - 1] = sum2 / n;
    }
    g.sync();
  }
  if (lane == 0) {
    int N = 1;
    if (w.err[1] < w.err[0]) N = 2;
    if (w.err[2] < w.err[N - 1]) N = 3;
    for (int i = 0; i < 9; i++) R[i] = w.Rs[9 * (N - 1) + i];
    for (int i = 0; i < 3; i++) t[i] = w.ts[3 * (N - 1) + i];
    *N_out = N;
    *flags_out = w.flags;
  }
  g.sync();
}

// One correspondence of CheckInliers (:318-349). R, t: mRi / mti; K = fu, fv, uc, vc as double.
PNP_HD inline bool pnp_is_inlier(const double* R, const double* t, const double* K, float X, float Y, float Z, float u,
                                 float v, float max_error) {
  const float Xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
  const float Yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
  const float invZc = (float)(1 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
  const double ue = K[2] + K[0] * Xc * invZc;
  const double ve = K[3] + K[1] * Yc * invZc;
  const float distX = (float)(u - ue);
  const float distY = (float)(v - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < max_error;
}

// ------------------------------------------------------------------------------------------
// staging (host)

#define PNP_R 16           /* == ORBFE_PNP_MAX_RECORDS */
#define PNP_WS_DOUBLES 12  // per correspondence of a record: pws 3, us 2, alphas 4, pcs 3

// One launched solver, as the kernels see it. in_* are byte offsets into the upload buffer, o_* into
// the result buffer, ws into the refinement workspace.
struct PnpDev {
  int n, n_eval, min_inliers, max_its, words, pad0, pad1, pad2;
  double K[4];
  unsigned long long in_p3d, in_p2d, in_max, in_rand;
  unsigned long long o_mask, o_r, o_t, o_tcw, o_N, o_flags, o_cnt, o_slot;          // per hypothesis
  unsigned long long o_rec, o_rmask, o_rr, o_rt, o_rtcw, o_rN, o_rflags, o_rcnt;  // per record
  unsigned long long o_sel, ws;
};
// o_sel: accepted, accepted_inliers, best, best_inliers, no_more, n_records, overflow
#define PNP_SEL_INTS 8

// The arrays of one solver with n correspondences and e hypotheses, taken from the three blocks in the
// order the buffers hold them; fills d's offsets only. The one statement of the buffer plan: over counting
// blocks it sizes a handle (pnp_plan_bounds), over the real ones it places a solve. The workspace holds
// doubles only and is packed without the alignment step.
inline void pnp_layout(OrbfeStage& in, OrbfeStage& res, OrbfeStage& ws, size_t n, size_t e, PnpDev& d) {
  const size_t w = (n + 63) / 64, r = PNP_R;
  d.in_p3d = in.take(12 * n);
  d.in_p2d = in.take(8 * n);
  d.in_max = in.take(4 * n);
  d.in_rand = in.take(16 * e);
  d.o_mask = res.take(8 * w * e);
  d.o_r = res.take(72 * e);
  d.o_t = res.take(24 * e);
  d.o_tcw = res.take(48 * e);
  d.o_N = res.take(4 * e);
  d.o_flags = res.take(4 * e);
  d.o_cnt = res.take(4 * e);
  d.o_slot = res.take(4 * e);
  d.o_rec = res.take(4 * r);
  d.o_rmask = res.take(8 * w * r);
  d.o_rr = res.take(72 * r);
  d.o_rt = res.take(24 * r);
  d.o_rtcw = res.take(48 * r);
  d.o_rN = res.take(4 * r);
  d.o_rflags = res.take(4 * r);
  d.o_rcnt = res.take(4 * r);
  d.o_sel = res.take(4 * PNP_SEL_INTS);
  d.ws = ws.off;
  ws.off += r * PNP_WS_DOUBLES * 8 * n;
}

// A handle's buffer sizes: the record table and S solvers at the bounds
inline void pnp_plan_bounds(size_t S, size_t C, size_t H, size_t* in_bytes, size_t* res_bytes, size_t* ws_bytes) {
  OrbfeStage in, res, ws;
  PnpDev d;
  in.take(sizeof(PnpDev) * S);
  for (size_t s = 0; s < S; s++) pnp_layout(in, res, ws, C, H, d);
  *in_bytes = in.off, *res_bytes = res.off, *ws_bytes = ws.off;
}
