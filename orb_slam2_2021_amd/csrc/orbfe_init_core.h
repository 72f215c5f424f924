// orbfe_init_core.h -- Initializer's arithmetic (Initializer.cc:44-1006) as host/device inline
// functions: the sample selection, Normalize, ComputeH21 / ComputeF21 with OpenCV's Jacobi SVD and its
// fill-in, the 3x3 inverse / determinant / products, one match of CheckHomography / CheckFundamental,
// the motion hypotheses of ReconstructH / ReconstructF, one match of CheckRT and the two decisions.
// Used by the kernels of orbfe_init.hip and by the stand-alone host program
// tests/cpp/initializer_core_main.cpp. Not part of the C ABI.
//
// Every operation is an IEEE float or double + - * / sqrt, rounded separately (-ffp-contract=off);
// every OpenCV call is restated by the rule DESIGN.md section 23 records, and a rule recalled from
// OpenCV's source carries "OPENCV:". The rules orbfe_triangulate_core.h already states (the gemm's
// double sum with one rounding, cv::norm, lapack.cpp's hypot, the 4x4 SVD) are used from there.
// tests/initializer_ref.py mirrors this file function by function.
//
// The Jacobi SVD works on caller-provided memory whose element e sits at index e * es: LDS with
// es = the number of threads that share the block on the device (lane-interleaved, so the threads of
// a wavefront never meet in a bank), a plain array with es = 1 on the host.
#pragma once
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <cstring>

#include "orbfe_stage.h"
#include "orbfe_triangulate_core.h"

#define INIT_HD __host__ __device__

#define INIT_FLAG_TOO_FEW 1u   /* == ORBFE_INIT_FLAG_TOO_FEW */
#define INIT_FLAG_NO_MODEL 2u  /* == ORBFE_INIT_FLAG_NO_MODEL */
#define INIT_MODEL_H 0
#define INIT_MODEL_F 1

#define INIT_WORK_AT 144  // 9 rows of 16 (ComputeH21); ComputeF21 uses 9 rows of 9, a 3x3 SVD 3 of 3
#define INIT_WORK_VT 81
#define INIT_WORK_W 9

struct InitNorm {  // Normalize's result: T = [sx 0 -mx*sx; 0 sy -my*sy; 0 0 1]
  float mx, my, sx, sy;
};

// The eight matches of one iteration: swap-remove on a fresh 0..n-1 list (:82-97), kept as the (at
// most seven) slots that no longer hold their own index. Needs n >= 8 and 0 <= draw[j] <= n - 1 - j;
// every index returned is then in 0..n-1.
INIT_HD inline void init_select8(int n, const int* draw, int* idx) {
  int key[8], val[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int r = draw[i], last = n - 1 - i;
    int at_r = r, back = last;
#pragma unroll
    for (int q = 0; q < 8; q++)
      if (q < i) {  // a slot written twice holds the later value
        if (key[q] == r) at_r = val[q];
        if (key[q] == last) back = val[q];
      }
    idx[i] = at_r;
    key[i] = r;
    val[i] = back;
  }
}

// Normalize (:819-865) from its four running sums' results
INIT_HD inline InitNorm init_norm_of(float mx, float my, float dx, float dy) {
  InitNorm o;
  o.mx = mx;
  o.my = my;
  o.sx = (float)(1.0 / (double)dx);  // 1.0 / meanDevX: a double quotient, narrowed
  o.sy = (float)(1.0 / (double)dy);
  return o;
}

// Normalize over all n keys of a frame, the float sums in key order (the host's form; the kernel
// takes the same sums in the same order with a wavefront)
INIT_HD inline InitNorm init_normalize(const float* keys, int n) {
  float mx = 0, my = 0;
  for (int i = 0; i < n; i++) {
    mx = mx + keys[2 * (size_t)i];
    my = my + keys[2 * (size_t)i + 1];
  }
  mx = mx / (float)n;
  my = my / (float)n;
  float dx = 0, dy = 0;
  for (int i = 0; i < n; i++) {
    dx = dx + fabsf(keys[2 * (size_t)i] - mx);
    dy = dy + fabsf(keys[2 * (size_t)i + 1] - my);
  }
  dx = dx / (float)n;
  dy = dy / (float)n;
  return init_norm_of(mx, my, dx, dy);
}

INIT_HD inline void init_norm_point(const InitNorm& o, float x, float y, float* xn, float* yn) {
  *xn = (x - o.mx) * o.sx;
  *yn = (y - o.my) * o.sy;
}

INIT_HD inline void init_t_of(const InitNorm& o, float* T) {
  T[0] = o.sx, T[1] = 0, T[2] = (-o.mx) * o.sx;
  T[3] = 0, T[4] = o.sy, T[5] = (-o.my) * o.sy;
  T[6] = 0, T[7] = 0, T[8] = 1;
}

// OPENCV: CV_32F gemm: each element the double sum (tri_dot3_d), one rounding. 3x3 row-major.
INIT_HD inline void init_gemm3(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      C[3 * i + j] = (float)tri_dot3_d(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}

// OPENCV: (s * A) * B is one gemm with alpha = s: the double sum times alpha in double, one rounding
INIT_HD inline void init_gemm3_alpha(const float* A, const float* B, float alpha, float* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      C[3 * i + j] =
          (float)((double)alpha * tri_dot3_d(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]));
}

// A * x (+ c): the gemm rule, with C added in double before the one rounding
INIT_HD inline void init_gemv3(const float* A, const float* x, const float* c, float* y) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double s = tri_dot3_d(A[3 * i], A[3 * i + 1], A[3 * i + 2], x[0], x[1], x[2]);
    if (c) s = s + (double)c[i];
    y[i] = (float)s;
  }
}

INIT_HD inline void init_transpose3(const float* A, float* B) {
  B[0] = A[0], B[1] = A[3], B[2] = A[6], B[3] = A[1], B[4] = A[4], B[5] = A[7], B[6] = A[2], B[7] = A[5], B[8] = A[8];
}

// OPENCV: det3 on CV_32F: every product and sum in double, the first-row cofactor expansion
INIT_HD inline double init_det3_d(const float* f) {
  const double m0 = f[0], m1 = f[1], m2 = f[2], m3 = f[3], m4 = f[4], m5 = f[5], m6 = f[6], m7 = f[7], m8 = f[8];
  return m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6) + m2 * (m3 * m7 - m4 * m6);
}

// OPENCV: Mat::inv() (DECOMP_LU) of a 3x3 CV_32F: d = det3, zeros when d == 0, else the adjugate in
// double times 1/d, each element rounded once
INIT_HD inline void init_inv3(const float* f, float* o) {
  double d = init_det3_d(f);
  if (d == 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = 0;
    return;
  }
  d = 1.0 / d;
  const double s0 = f[0], s1 = f[1], s2 = f[2], s3 = f[3], s4 = f[4], s5 = f[5], s6 = f[6], s7 = f[7], s8 = f[8];
  o[0] = (float)((s4 * s8 - s5 * s7) * d);
  o[1] = (float)((s2 * s7 - s1 * s8) * d);
  o[2] = (float)((s1 * s5 - s2 * s4) * d);
  o[3] = (float)((s5 * s6 - s3 * s8) * d);
  o[4] = (float)((s0 * s8 - s2 * s6) * d);
  o[5] = (float)((s2 * s3 - s0 * s5) * d);
  o[6] = (float)((s3 * s7 - s4 * s6) * d);
  o[7] = (float)((s1 * s6 - s0 * s7) * d);
  o[8] = (float)((s0 * s4 - s1 * s3) * d);
}

// OPENCV: RNG::next(): state = (uint32)state * 4164903690 + (state >> 32); the low 32 bits are returned
INIT_HD inline uint64_t init_rng_next(uint64_t state) {
  return (uint64_t)(uint32_t)state * 4164903690ull + (state >> 32);
}

// OPENCV: JacobiSVDImpl_<float>(At, W, Vt, m, n, n1, minval = FLT_MIN, eps = FLT_EPSILON * 2).
// At holds n1 rows of m floats (rows >= n are filled here), Vt n rows of n, W n doubles; element e of
// each sits at index e * es. On return row i of At is the i-th left vector scaled by 1 / W[i] (rows
// i < n1 only), W the singular values in descending order, Vt the right vectors as rows. At most
// max(m, 30) sweeps, so a NaN matrix ends. *refills counts the refilled rows i < n (may be NULL).
INIT_HD inline void init_jacobi_svd(float* At, int astep, float* Vt, int vstep, double* W, int m, int n, int n1,
                                    int es, int* refills) {
#define IA(i, k) At[((i) * astep + (k)) * es]
#define IV(i, k) Vt[((i) * vstep + (k)) * es]
#define IW(i) W[(i) * es]
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) sd += (double)IA(i, k) * (double)IA(i, k);
    IW(i) = sd;
    for (int k = 0; k < n; k++) IV(i, k) = i == k ? 1.0f : 0.0f;
  }
  const float eps = FLT_EPSILON * 2;
  const int max_iter = m > 30 ? m : 30;  // OPENCV: at most max(m, 30) sweeps
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
    for (int i = 0; i < n - 1; i++)
      for (int j = i + 1; j < n; j++) {
        double a = IW(i), p = 0, b = IW(j);
        for (int k = 0; k < m; k++) p += (double)IA(i, k) * (double)IA(j, k);
        if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = tri_hypot_d(p, beta);
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)sqrt(delta / gamma);
          c = (float)(p / (gamma * (double)s * 2));
        } else {
          c = (float)sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * (double)c * 2));
        }
        a = b = 0;
        for (int k = 0; k < m; k++) {
          const float t0 = c * IA(i, k) + s * IA(j, k);
          const float t1 = -s * IA(i, k) + c * IA(j, k);
          IA(i, k) = t0;
          IA(j, k) = t1;
          a += (double)t0 * t0;
          b += (double)t1 * t1;
        }
        IW(i) = a;
        IW(j) = b;
        changed = true;
        for (int k = 0; k < n; k++) {
          const float t0 = c * IV(i, k) + s * IV(j, k);
          const float t1 = -s * IV(i, k) + c * IV(j, k);
          IV(i, k) = t0;
          IV(j, k) = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) sd += (double)IA(i, k) * (double)IA(i, k);
    IW(i) = sqrt(sd);
  }
  // OPENCV: descending selection sort (W[j] < W[k] on the doubles); rows of At and Vt go with them
  for (int i = 0; i < n - 1; i++) {
    int j = i;
    for (int k = i + 1; k < n; k++)
      if (IW(j) < IW(k)) j = k;
    if (i != j) {
      const double tw = IW(i);
      IW(i) = IW(j);
      IW(j) = tw;
      for (int k = 0; k < m; k++) {
        const float t = IA(i, k);
        IA(i, k) = IA(j, k);
        IA(j, k) = t;
      }
      for (int k = 0; k < n; k++) {
        const float t = IV(i, k);
        IV(i, k) = IV(j, k);
        IV(j, k) = t;
      }
    }
  }
  // OPENCV: the fill-in. A row i >= n, or a row whose singular value is <= FLT_MIN, is drawn from
  // RNG(0x12345678) as +-1/m, orthogonalised twice against rows 0..i-1 and normalised.
  uint64_t rng = 0x12345678ull;
  for (int i = 0; i < n1; i++) {
    double sd = i < n ? IW(i) : 0;
    for (int ii = 0; ii < 100 && sd <= (double)FLT_MIN; ii++) {
      if (i < n && refills) *refills += 1;
      const float val0 = (float)(1.0 / (double)m);
      for (int k = 0; k < m; k++) {
        rng = init_rng_next(rng);
        IA(i, k) = ((uint32_t)rng & 256u) != 0 ? val0 : -val0;  // OPENCV: (rng.next() & 256) != 0
      }
      for (int pass = 0; pass < 2; pass++)
        for (int j = 0; j < i; j++) {
          sd = 0;
          for (int k = 0; k < m; k++) sd += (double)(IA(i, k) * IA(j, k));  // OPENCV: a float product added to the double
          float asum = 0;
          for (int k = 0; k < m; k++) {
            const float t = (float)((double)IA(i, k) - sd * (double)IA(j, k));  // OPENCV: formed in double, narrowed
            IA(i, k) = t;
            asum = asum + fabsf(t);
          }
          asum = asum > eps * 100.0f ? 1.0f / asum : 0.0f;
          for (int k = 0; k < m; k++) IA(i, k) = IA(i, k) * asum;
        }
      sd = 0;
      for (int k = 0; k < m; k++) sd += (double)IA(i, k) * (double)IA(i, k);
      sd = sqrt(sd);
    }
    const float s = (float)(sd > (double)FLT_MIN ? 1.0 / sd : 0.0);
    for (int k = 0; k < m; k++) IA(i, k) = IA(i, k) * s;
  }
#undef IA
#undef IV
#undef IW
}

// cv::SVD::compute of a 3x3 CV_32F (m == n: JacobiSVDImpl_ on the transpose, n1 = 3): u's column i is
// row i of At. w[3], u[9], vt[9].
INIT_HD inline void init_svd3(const float* M, float* At, float* Vt, double* W, int es, float* w, float* u, float* vt,
                              int* refills) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) At[(3 * i + k) * es] = M[3 * k + i];
  init_jacobi_svd(At, 3, Vt, 3, W, 3, 3, 3, es, refills);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    w[i] = (float)W[i * es];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      u[3 * i + j] = At[(3 * j + i) * es];
      vt[3 * i + j] = Vt[(3 * i + j) * es];
    }
  }
}

// ComputeH21 (:223-263): A is 16x9, m > n: the SVD runs on the transpose (9 rows of 16); vt.row(8) is
// the last row of Vt. The fill-in only touches u, which is not used (n1 = 0). p1 / p2: 8 (x, y).
INIT_HD inline void init_compute_h21(const float* p1, const float* p2, float* At, float* Vt, double* W, int es,
                                     float* H) {
#define IA(i, k) At[((i) * 16 + (k)) * es]
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    const int r = 2 * i;
    IA(0, r) = 0, IA(1, r) = 0, IA(2, r) = 0, IA(3, r) = -u1, IA(4, r) = -v1, IA(5, r) = -1.0f;
    IA(6, r) = v2 * u1, IA(7, r) = v2 * v1, IA(8, r) = v2;
    IA(0, r + 1) = u1, IA(1, r + 1) = v1, IA(2, r + 1) = 1.0f, IA(3, r + 1) = 0, IA(4, r + 1) = 0, IA(5, r + 1) = 0;
    IA(6, r + 1) = (-u2) * u1, IA(7, r + 1) = (-u2) * v1, IA(8, r + 1) = -u2;
  }
#undef IA
  init_jacobi_svd(At, 16, Vt, 9, W, 16, 9, 0, es, nullptr);
#pragma unroll
  for (int k = 0; k < 9; k++) H[k] = Vt[(8 * 9 + k) * es];
}

// ComputeF21 (:265-300): A is 8x9, m < n: OpenCV swaps the roles, the rotations orthogonalise the 8
// rows of A itself and vt (FULL_UV, 9 rows) is At; row 8 comes from the fill-in. Then the rank-2
// step: a 3x3 SVD, w[2] = 0, u * diag(w) * vt as two gemms.
INIT_HD inline void init_compute_f21(const float* p1, const float* p2, float* At, float* Vt, double* W, int es,
                                     float* F, int* refills) {
#define IA(i, k) At[((i) * 9 + (k)) * es]
  for (int i = 0; i < 8; i++) {
    const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
    IA(i, 0) = u2 * u1, IA(i, 1) = u2 * v1, IA(i, 2) = u2;
    IA(i, 3) = v2 * u1, IA(i, 4) = v2 * v1, IA(i, 5) = v2;
    IA(i, 6) = u1, IA(i, 7) = v1, IA(i, 8) = 1.0f;
  }
  for (int k = 0; k < 9; k++) IA(8, k) = 0;
  init_jacobi_svd(At, 9, Vt, 8, W, 9, 8, 9, es, refills);
  float fpre[9];
#pragma unroll
  for (int k = 0; k < 9; k++) fpre[k] = IA(8, k);
#undef IA
  float w[3], u[9], vt[9], d[9], ud[9];
  init_svd3(fpre, At, Vt, W, es, w, u, vt, refills);
  w[2] = 0;
  d[0] = w[0], d[1] = 0, d[2] = 0, d[3] = 0, d[4] = w[1], d[5] = 0, d[6] = 0, d[7] = 0, d[8] = w[2];
  init_gemm3(u, d, ud);
  init_gemm3(ud, vt, F);
}

// One match of CheckHomography (:337-385): score += *t1 where *in1, += *t2 where *in2
INIT_HD inline void init_check_h_match(const float* H21, const float* H12, float u1, float v1, float u2, float v2,
                                       float inv_sigma2, bool* in1, float* t1, bool* in2, float* t2) {
  const float th = 5.991f;
  float w = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
  float a = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w;
  float b = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w;
  const float chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_sigma2;
  w = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
  a = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w;
  b = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w;
  const float chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_sigma2;
  *in1 = !(chi1 > th);
  *t1 = th - chi1;
  *in2 = !(chi2 > th);
  *t2 = th - chi2;
}

// One match of CheckFundamental (:413-465)
INIT_HD inline void init_check_f_match(const float* F, float u1, float v1, float u2, float v2, float inv_sigma2,
                                       bool* in1, float* t1, bool* in2, float* t2) {
  const float th = 3.841f, th_score = 5.991f;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_sigma2;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_sigma2;
  *in1 = !(chi1 > th);
  *t1 = th_score - chi1;
  *in2 = !(chi2 > th);
  *t2 = th_score - chi2;
}

INIT_HD inline void init_k_matrix(const float* k, float* K) {
  K[0] = k[0], K[1] = 0, K[2] = k[2], K[3] = 0, K[4] = k[1], K[5] = k[3], K[6] = 0, K[7] = 0, K[8] = 1;
}

// t / cv::norm(t). OPENCV: Mat / scalar multiplies by (float)(1.0 / s)
INIT_HD inline void init_unit3(const float* t, float* o) {
  const float inv = (float)(1.0 / tri_norm3_d(t[0], t[1], t[2]));
  o[0] = t[0] * inv, o[1] = t[1] * inv, o[2] = t[2] * inv;
}

// ReconstructF up to the four hypotheses (:486-494) with DecomposeE (:986-1006):
// (R1,t) (R2,t) (R1,-t) (R2,-t). R[4*9], t[4*3].
INIT_HD inline void init_motions_f(const float* F21, const float* K, float* At, float* Vt, double* W, int es, float* R,
                                   float* t, int* refills) {
  float Kt[9], KF[9], E[9], w[3], u[9], vt[9];
  init_transpose3(K, Kt);
  init_gemm3(Kt, F21, KF);
  init_gemm3(KF, K, E);
  init_svd3(E, At, Vt, W, es, w, u, vt, refills);
  const float u2[3] = {u[2], u[5], u[8]};
  float tt[3];
  init_unit3(u2, tt);
  const float Wm[9] = {0, -1.0f, 0, 1.0f, 0, 0, 0, 0, 1.0f};
  float Wt[9], uw[9], R1[9], R2[9];
  init_gemm3(u, Wm, uw);
  init_gemm3(uw, vt, R1);
  if (init_det3_d(R1) < 0)
#pragma unroll
    for (int i = 0; i < 9; i++) R1[i] = -R1[i];
  init_transpose3(Wm, Wt);
  init_gemm3(u, Wt, uw);
  init_gemm3(uw, vt, R2);
  if (init_det3_d(R2) < 0)
#pragma unroll
    for (int i = 0; i < 9; i++) R2[i] = -R2[i];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = R1[i], R[9 + i] = R2[i], R[18 + i] = R1[i], R[27 + i] = R2[i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = tt[i], t[3 + i] = tt[i], t[6 + i] = -tt[i], t[9 + i] = -tt[i];
}

// ReconstructH up to the eight hypotheses (:641-743): false for the early return of :654. vn is never
// read by the reference and is not formed. R[8*9], t[8*3].
INIT_HD inline bool init_motions_h(const float* H21, const float* K, float* At, float* Vt, double* W, int es, float* R,
                                   float* t, int* refills) {
  float invK[9], KH[9], A[9], w[3], U[9], V[9];
  init_inv3(K, invK);
  init_gemm3(invK, H21, KH);
  init_gemm3(KH, K, A);
  init_svd3(A, At, Vt, W, es, w, U, V, refills);
  const float s = (float)(init_det3_d(U) * init_det3_d(V));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_st = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float st[4] = {aux_st, -aux_st, -aux_st, aux_st};
  const float aux_sp = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sp[4] = {aux_sp, -aux_sp, -aux_sp, aux_sp};
  const float z = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float Rp[9] = {ct, 0, -st[i], 0, 1.0f, 0, st[i], 0, ct};
    float URp[9], tu[3];
    init_gemm3_alpha(U, Rp, s, URp);  // s * U * Rp * Vt: the scale rides on the first gemm
    init_gemm3(URp, V, R + 9 * i);
    const float tp[3] = {x1[i] * (d1 - d3), z * (d1 - d3), (-x3[i]) * (d1 - d3)};
    init_gemv3(U, tp, nullptr, tu);
    init_unit3(tu, t + 3 * i);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float Rp[9] = {cp, 0, sp[i], 0, -1.0f, 0, sp[i], 0, -cp};
    float URp[9], tu[3];
    init_gemm3_alpha(U, Rp, s, URp);
    init_gemm3(URp, V, R + 9 * (4 + i));
    const float tp[3] = {x1[i] * (d1 + d3), z * (d1 + d3), x3[i] * (d1 + d3)};
    init_gemv3(U, tp, nullptr, tu);
    init_unit3(tu, t + 3 * (4 + i));
  }
  return true;
}

// P2 = K * [R | t] (3x4, gemm) and O2 = -R.t() * t (:898-903)
INIT_HD inline void init_camera2(const float* R, const float* t, const float* K, float* P2, float* O2) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++)
      P2[4 * i + j] = (float)tri_dot3_d(K[3 * i], K[3 * i + 1], K[3 * i + 2], R[j], R[3 + j], R[6 + j]);
    P2[4 * i + 3] = (float)tri_dot3_d(K[3 * i], K[3 * i + 1], K[3 * i + 2], t[0], t[1], t[2]);
  }
  float Rt[9];
  init_transpose3(R, Rt);
#pragma unroll
  for (int i = 0; i < 9; i++) Rt[i] = -Rt[i];
  init_gemv3(Rt, t, nullptr, O2);
}

INIT_HD inline bool init_finite(float x) { return fabsf(x) <= FLT_MAX; }

// One inlier match of CheckRT (:912-970): true when the match passes every gate; then X is its
// vP3D entry, *cosp its cosParallax and *good its vbGood bit. k: fx, fy, cx, cy.
INIT_HD inline bool init_check_rt_match(const float* R, const float* t, const float* P2, const float* O2,
                                        const float* k, float x1, float y1, float x2, float y2, float th2, float* X,
                                        float* cosp, bool* good) {
  const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
  const float P1[12] = {fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1.0f, 0};
  float A[4][4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    // OPENCV: a * M.row(r) - M.row(q) is one scaled add on floats: fl(fl(a * m_r) - m_q)
    A[0][c] = x1 * P1[8 + c] - P1[c];
    A[1][c] = y1 * P1[8 + c] - P1[4 + c];
    A[2][c] = x2 * P2[8 + c] - P2[c];
    A[3][c] = y2 * P2[8 + c] - P2[4 + c];
  }
  float v[4];
  tri_svd4_vt_row3(A, v);
  const float inv = (float)(1.0 / (double)v[3]);  // OPENCV: Mat / scalar multiplies by (float)(1.0 / s)
  X[0] = v[0] * inv, X[1] = v[1] * inv, X[2] = v[2] * inv;
  *good = false;
  *cosp = 0;
  if (!(init_finite(X[0]) && init_finite(X[1]) && init_finite(X[2]))) return false;  // isfinite
  const float dist1 = (float)tri_norm3_d(X[0], X[1], X[2]);  // normal1 = p3dC1 - O1, O1 = 0
  const float n2[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};
  const float dist2 = (float)tri_norm3_d(n2[0], n2[1], n2[2]);
  const float c = (float)(tri_dot3_d(X[0], X[1], X[2], n2[0], n2[1], n2[2]) / (double)(dist1 * dist2));
  *cosp = c;
  const bool low = (double)c < 0.99998;
  if (X[2] <= 0 && low) return false;
  float X2[3];
  init_gemv3(R, X, t, X2);
  if (X2[2] <= 0 && low) return false;
  const float inv_z1 = (float)(1.0 / (double)X[2]);
  float ex = fx * X[0] * inv_z1 + cx - x1;
  float ey = fy * X[1] * inv_z1 + cy - y1;
  if (ex * ex + ey * ey > th2) return false;
  const float inv_z2 = (float)(1.0 / (double)X2[2]);
  ex = fx * X2[0] * inv_z2 + cx - x2;
  ey = fy * X2[1] * inv_z2 + cy - y2;
  if (ex * ex + ey * ey > th2) return false;
  *good = low;
  return true;
}

// The IEEE total order of a float as an unsigned key (-NaN < -inf < ... < -0 < +0 < ... < +NaN)
INIT_HD inline uint32_t init_order_key(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b < 0x80000000u ? (b ^ 0x80000000u) : ~b;
}
INIT_HD inline float init_key_value(uint32_t key) {
  const uint32_t b = key >= 0x80000000u ? (key ^ 0x80000000u) : ~key;
  float x;
  memcpy(&x, &b, 4);
  return x;
}

// ReconstructF's gates before the parallax (:546-567): the hypothesis the if-chain of :570-617 tests,
// or -1
INIT_HD inline int init_decide_f(const int* n_good, int n_inl) {
  int max_good = n_good[0];
#pragma unroll
  for (int i = 1; i < 4; i++) max_good = n_good[i] > max_good ? n_good[i] : max_good;
  const int n09 = (int)(0.9 * (double)n_inl);
  const int n_min_good = n09 > 50 ? n09 : 50;
  int nsimilar = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if ((double)n_good[i] > 0.7 * (double)max_good) nsimilar++;
  if (max_good < n_min_good || nsimilar > 1) return -1;
  int idx = -1;
#pragma unroll
  for (int i = 3; i >= 0; i--)
    if (n_good[i] == max_good) idx = i;
  return idx;
}

// ReconstructH's scan (:745-784) and the gates of :786-787 but the parallax: bestSolutionIdx when
// they pass, or -1
INIT_HD inline int init_decide_h(const int* n_good, int n_inl) {
  int best = 0, second = 0, idx = -1;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (n_good[i] > best) {
      second = best;
      best = n_good[i];
      idx = i;
    } else if (n_good[i] > second) {
      second = n_good[i];
    }
  }
  const bool ok = (double)second < 0.75 * (double)best && best > 50 && (double)best > 0.9 * (double)n_inl;
  return ok ? idx : -1;
}

// ------------------------------------------------------------------------------------------
// staging (host)

// What k_init_select, k_init_checkrt and k_init_decide leave per problem (in the result buffer)
struct InitSel {
  int best_h, best_f, model, n_motions, candidate, n_inl;
  unsigned flags;
  int pad;
  int n_good[8];
  float cosv[8];
  float SH, SF, RH, pad1;
  float H21[9], F21[9];
  float R[72], t[24];
};

// One launched problem, as the kernels see it. in_* are byte offsets into the upload buffer, o_*
// into the result buffer, w_* into the workspace.
struct InitDev {
  int n1, n2, N, n_hyp, words, pad0, pad1, pad2;
  float k[4];
  float sigma, inv_sigma2, th2, pad3;
  unsigned long long in_k1, in_k2, in_m1, in_m2, in_rand;
  unsigned long long o_nrm, o_sh, o_sf, o_sel, o_mh, o_mf, o_p3d, o_tri;
  unsigned long long w_models, w_masks, w_p3d, w_good, w_cos;
};

// The arrays of one problem with n1 and n2 keypoints, m matches and e hypotheses, taken from the three
// blocks in the order the buffers hold them; fills d's offsets only. The one statement of the buffer
// plan: over counting blocks it sizes a handle (init_plan_bounds), over the real ones it places a solve.
inline void init_layout(OrbfeStage& in, OrbfeStage& res, OrbfeStage& ws, size_t n1, size_t n2, size_t m, size_t e,
                        InitDev& d) {
  const size_t w = (m + 63) / 64;
  d.in_k1 = in.take(8 * n1);
  d.in_k2 = in.take(8 * n2);
  d.in_m1 = in.take(4 * m);
  d.in_m2 = in.take(4 * m);
  d.in_rand = in.take(32 * e);
  d.o_nrm = res.take(2 * sizeof(InitNorm));
  d.o_sh = res.take(4 * e);
  d.o_sf = res.take(4 * e);
  d.o_sel = res.take(sizeof(InitSel));
  d.o_mh = res.take(8 * w);
  d.o_mf = res.take(8 * w);
  d.o_p3d = res.take(12 * n1);
  d.o_tri = res.take(n1);
  d.w_models = ws.take(108 * e);
  d.w_masks = ws.take(16 * w * e);
  d.w_p3d = ws.take(96 * n1);
  d.w_good = ws.take(8 * n1);
  d.w_cos = ws.take(32 * m);
}

// A handle's buffer sizes: the record table and S problems at the bounds
inline void init_plan_bounds(size_t S, size_t K, size_t M, size_t H, size_t* in_bytes, size_t* res_bytes,
                             size_t* ws_bytes) {
  OrbfeStage in, res, ws;
  InitDev d;
  in.take(sizeof(InitDev) * S);
  for (size_t s = 0; s < S; s++) init_layout(in, res, ws, K, K, M, H, d);
  *in_bytes = in.off, *res_bytes = res.off, *ws_bytes = ws.off;
}
