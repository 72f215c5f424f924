// orbfe_sim3_core.h -- Sim3Solver's per-hypothesis arithmetic (Sim3Solver.cc:162-176, :214-336) as
// host/device inline functions: the sample selection and ComputeSim3. Used by k_sim3_hypotheses in
// orbfe_sim3.hip. Not part of the C ABI.
//
// Every float operation is rounded separately (-ffp-contract=off) and every OpenCV call is restated
// by the rule DESIGN.md section 15 records; a rule recalled from OpenCV's source carries "OPENCV:".
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "orbfe_stage.h"

#define SIM3_JACOBI_MAX_ROTATIONS (4 * 4 * 30)

// The three correspondences of one iteration: swap-remove on a fresh 0..n-1 list (:162-176), kept
// as the (at most two) slots that no longer hold their own index. Needs n >= 3 and
// 0 <= draw[i] <= n - 1 - i; every index returned is then in 0..n-1.
__host__ __device__ __forceinline__ void sim3_select3(int n, const int* draw, int* idx) {
  int key0 = -1, val0 = 0, key1 = -1, val1 = 0;
  auto get = [&](int j) { return j == key1 ? val1 : (j == key0 ? val0 : j); };
  for (int i = 0; i < 3; i++) {
    const int size = n - i;
    const int r = draw[i];
    idx[i] = get(r);
    const int back = get(size - 1);
    if (i == 0) {
      key0 = r;
      val0 = back;
    } else if (i == 1) {
      key1 = r;
      val1 = back;
    }
  }
}

// OPENCV: CV_32F gemm element: double accumulation left to right, one rounding
__host__ __device__ __forceinline__ double sim3_dot3_d(float a0, float a1, float a2, float b0, float b1, float b2) {
  double s = (double)a0 * (double)b0;
  s += (double)a1 * (double)b1;
  s += (double)a2 * (double)b2;
  return s;
}

// OPENCV: std::hypot(float, float) as sqrt of the double sum of squares, narrowed once
__host__ __device__ __forceinline__ float sim3_hypot(float a, float b) {
  return (float)sqrt((double)a * (double)a + (double)b * (double)b);
}

// OPENCV: cv::eigen on a symmetric 4x4 CV_32F (JacobiImpl_<float>): eigenvalues descending in W,
// eigenvectors as the rows of V. At most SIM3_JACOBI_MAX_ROTATIONS rotations, so a NaN matrix ends.
// indR[k] is in k+1..3 and indC[k] in 0..k-1 whatever the values, so every index is below 4.
__host__ __device__ inline void sim3_jacobi4(float A[4][4], float W[4], float V[4][4]) {
  const int n = 4;
  const float eps = FLT_EPSILON;
  int indR[4] = {0, 0, 0, 0}, indC[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i][j] = i == j ? 1.0f : 0.0f;
  auto row_max = [&](int k) {
    int m = k + 1;
    float mv = fabsf(A[k][m]);
    for (int i = k + 2; i < n; i++) {
      const float val = fabsf(A[k][i]);
      if (mv < val) mv = val, m = i;
    }
    return m;
  };
  auto col_max = [&](int k) {
    int m = 0;
    float mv = fabsf(A[0][k]);
    for (int i = 1; i < k; i++) {
      const float val = fabsf(A[i][k]);
      if (mv < val) mv = val, m = i;
    }
    return m;
  };
  for (int k = 0; k < n; k++) {
    W[k] = A[k][k];
    if (k < n - 1) indR[k] = row_max(k);
    if (k > 0) indC[k] = col_max(k);
  }
  for (int iters = 0; iters < SIM3_JACOBI_MAX_ROTATIONS; iters++) {
    int k = 0;
    float mv = fabsf(A[0][indR[0]]);
    for (int i = 1; i < n - 1; i++) {
      const float val = fabsf(A[i][indR[i]]);
      if (mv < val) mv = val, k = i;
    }
    int l = indR[k];
    for (int i = 1; i < n; i++) {
      const float val = fabsf(A[indC[i]][i]);
      if (mv < val) mv = val, k = indC[i], l = i;
    }
    const float p = A[k][l];
    if (fabsf(p) <= eps) break;
    const float y = (W[l] - W[k]) * 0.5f;
    float t = fabsf(y) + sim3_hypot(p, y);
    float s = sim3_hypot(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) s = -s, t = -t;
    A[k][l] = 0;
    W[k] -= t;
    W[l] += t;
    float a0, b0;
#define SIM3_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
    for (int i = 0; i < k; i++) SIM3_ROTATE(A[i][k], A[i][l]);
    for (int i = k + 1; i < l; i++) SIM3_ROTATE(A[k][i], A[i][l]);
    for (int i = l + 1; i < n; i++) SIM3_ROTATE(A[k][i], A[l][i]);
    for (int i = 0; i < n; i++) SIM3_ROTATE(V[k][i], V[l][i]);
#undef SIM3_ROTATE
    for (int j = 0; j < 2; j++) {
      const int idx = j == 0 ? k : l;
      if (idx < n - 1) indR[idx] = row_max(idx);
      if (idx > 0) indC[idx] = col_max(idx);
    }
  }
  for (int k = 0; k < n - 1; k++) {
    int m = k;
    for (int i = k + 1; i < n; i++)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      float tmp = W[m];
      W[m] = W[k];
      W[k] = tmp;
      for (int i = 0; i < n; i++) {
        tmp = V[m][i];
        V[m][i] = V[k][i];
        V[k][i] = tmp;
      }
    }
  }
}

// ComputeCentroid (:214-223): P holds one point per column, P[row][col]
__host__ __device__ __forceinline__ void sim3_centroid(const float P[3][3], float Pr[3][3], float C[3]) {
  for (int r = 0; r < 3; r++) {
    float c = (P[r][0] + P[r][1]) + P[r][2];  // OPENCV: cv::reduce(SUM) of a CV_32F row: float, left to right
    c = c * (float)(1.0 / 3);                 // OPENCV: C / P.cols multiplies by (float)(1.0 / 3)
    C[r] = c;
    for (int i = 0; i < 3; i++) Pr[r][i] = P[r][i] - c;
  }
}

// ComputeSim3 (:225-336). P1 / P2: the three sampled points of set 1 / 2, one per column.
// T12 / T21: the upper 3x4 of mT12i / mT21i, row-major. R row-major.
__host__ __device__ inline void sim3_compute(const float P1[3][3], const float P2[3][3], int fix_scale,
                                             float* T12, float* T21, float* R, float* t, float* s_out) {
  float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
  sim3_centroid(P1, Pr1, O1);
  sim3_centroid(P2, Pr2, O2);
  float M[3][3];  // Pr2 * Pr1.t()
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      M[i][j] = (float)sim3_dot3_d(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
  const float N11 = M[0][0] + M[1][1] + M[2][2];
  const float N12 = M[1][2] - M[2][1];
  const float N13 = M[2][0] - M[0][2];
  const float N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2];
  const float N23 = M[0][1] + M[1][0];
  const float N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2];
  const float N34 = M[1][2] + M[2][1];
  const float N44 = -M[0][0] - M[1][1] + M[2][2];
  float A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
  float W[4], V[4][4];
  sim3_jacobi4(A, W, V);
  const float q0 = V[0][0];
  float vec[3] = {V[0][1], V[0][2], V[0][3]};
  // OPENCV: cv::norm of CV_32F accumulates the squares in double; its double result is used as is
  const double nrm = sqrt((double)vec[0] * (double)vec[0] + (double)vec[1] * (double)vec[1] +
                          (double)vec[2] * (double)vec[2]);
  const double ang = atan2(nrm, (double)q0);
  const float alpha = (float)(2.0 * ang / nrm);  // OPENCV: 2*ang*vec/norm(vec) is one double alpha applied as a float scale
  for (int i = 0; i < 3; i++) vec[i] = vec[i] * alpha;
  // OPENCV: cv::Rodrigues, vector -> matrix, in double: identity below DBL_EPSILON, else
  // (c*I + (1-c)*r*rT) + s*[r]x element by element, narrowed to float
  {
    const double x = vec[0], y = vec[1], z = vec[2];
    const double theta = sqrt(x * x + y * y + z * z);
    if (theta < DBL_EPSILON) {
      for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    } else {
      const double c = cos(theta), sn = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
      const double r[3] = {x * it, y * it, z * it};
      const double rx[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          double e = c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j]);
          e = e + sn * rx[3 * i + j];
          R[3 * i + j] = (float)e;
        }
    }
  }
  float P3[3][3];  // R * Pr2
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      P3[i][j] = (float)sim3_dot3_d(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j]);
  float s = 1.0f;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        nom += (double)Pr1[i][j] * (double)P3[i][j];  // OPENCV: Mat::dot: double sum of the float pairs' products, row-major
        den += (double)(P3[i][j] * P3[i][j]);
      }
    s = (float)(nom / den);
  }
  // O1 - s*R*O2: one gemm with alpha -s and C = O1
  for (int i = 0; i < 3; i++) {
    double v = sim3_dot3_d(R[3 * i], R[3 * i + 1], R[3 * i + 2], O2[0], O2[1], O2[2]);
    v = (-(double)s) * v;
    v = v + (double)O1[i];
    t[i] = (float)v;
  }
  const float a_inv = (float)(1.0 / (double)s);
  float sRinv[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      T12[4 * i + j] = R[3 * i + j] * s;       // OPENCV: s*R multiplies by (float)alpha
      sRinv[3 * i + j] = R[3 * j + i] * a_inv;  // OPENCV: (1.0/s)*R.t() multiplies by (float)alpha
      T21[4 * i + j] = sRinv[3 * i + j];
    }
  for (int i = 0; i < 3; i++) {
    T12[4 * i + 3] = t[i];
    double v = sim3_dot3_d(sRinv[3 * i], sRinv[3 * i + 1], sRinv[3 * i + 2], t[0], t[1], t[2]);
    T21[4 * i + 3] = (float)(-1.0 * v);
  }
  *s_out = s;
}

// ------------------------------------------------------------------------------------------
// staging (host)

// One launched solver, as the kernels see it. in_* are byte offsets into the upload buffer, o_* into
// the result buffer.
struct Sim3Dev {
  int n, n_eval, fix_scale, min_inliers, max_its, has_hyp, words, pad;
  float k1[4], k2[4];
  unsigned long long in_x1, in_x2, in_max1, in_max2, in_rand, in_t12, in_t21;
  unsigned long long o_mask, o_t12, o_t21, o_r, o_t, o_s, o_cnt, o_sel;
};

// The arrays of one solver with n correspondences and e evaluated hypotheses, taken from the two blocks
// in the order the buffers hold them; fills d's offsets only. The one statement of the buffer plan: over
// counting blocks it sizes a handle (sim3_plan_bounds), over the real ones it places a solve.
inline void sim3_layout(OrbfeStage& in, OrbfeStage& res, size_t n, size_t e, bool has_hyp, Sim3Dev& d) {
  const size_t w = (n + 63) / 64;
  d.in_x1 = in.take(12 * n);
  d.in_x2 = in.take(12 * n);
  d.in_max1 = in.take(4 * n);
  d.in_max2 = in.take(4 * n);
  if (has_hyp) {
    d.in_t12 = in.take(48 * e);
    d.in_t21 = in.take(48 * e);
  } else {
    d.in_rand = in.take(12 * e);
  }
  d.o_mask = res.take(8 * w * e);
  d.o_t12 = res.take(48 * e);
  d.o_t21 = res.take(48 * e);
  d.o_r = res.take(36 * e);
  d.o_t = res.take(12 * e);
  d.o_s = res.take(4 * e);
  d.o_cnt = res.take(4 * e);
  d.o_sel = res.take(32);
}

// A handle's buffer sizes: the record table and S solvers at the bounds, in the larger of the two
// hypothesis modes
inline void sim3_plan_bounds(size_t S, size_t C, size_t H, size_t* in_bytes, size_t* res_bytes) {
  *in_bytes = *res_bytes = 0;
  for (int has_hyp = 0; has_hyp < 2; has_hyp++) {
    OrbfeStage in, res;
    Sim3Dev d;
    in.take(sizeof(Sim3Dev) * S);
    for (size_t s = 0; s < S; s++) sim3_layout(in, res, C, H, has_hyp != 0, d);
    *in_bytes = std::max(*in_bytes, in.off);
    *res_bytes = std::max(*res_bytes, res.off);
  }
}
