// orbfe_triangulate_core.h -- the per-match arithmetic of LocalMapping::CreateNewMapPoints
// (LocalMapping.cc:290-438) and KeyFrame::UnprojectStereo (KeyFrame.cc:632-648) as host/device
// inline functions. Used by k_triangulate in orbfe_triangulate.hip. Not part of the C ABI.
//
// Every float operation is rounded separately (-ffp-contract=off) and every OpenCV / libm call is
// restated by the rule DESIGN.md section 16 records; a rule recalled from OpenCV's source carries
// "OPENCV:", a C library call "LIBM:". tests/triangulate_ref.py mirrors each marked line.
//
// No array here is indexed by a run-time value: after unrolling every element of the 4x4 matrices
// is a scalar, so the kernel keeps them in registers (no scratch).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "../../include/orbfe_triangulate.h"

#define TRI_SVD_MAX_SWEEPS 30  // OPENCV: JacobiSVDImpl_ runs at most max(m, 30) sweeps (m = 4)

struct TriCam {  // of one KeyFrame
  float fx, fy, cx, cy, invfx, invfy, bf, b;
};
struct TriObs {  // of one keypoint
  float x, y;        // mvKeysUn[i].pt
  float ur;          // mvuRight[i]
  float depth;       // mvDepth[i]
  float kx, ky;      // mvKeys[i].pt (UnprojectStereo)
  float sigma2;      // mvLevelSigma2[octave]
  float scale;       // mvScaleFactors[octave]
};

// OPENCV: CV_32F gemm element / Mat::dot of three float pairs: double accumulation left to right
__host__ __device__ __forceinline__ double tri_dot3_d(float a0, float a1, float a2, float b0, float b1, float b2) {
  double s = (double)a0 * (double)b0;
  s += (double)a1 * (double)b1;
  s += (double)a2 * (double)b2;
  return s;
}

// OPENCV: cv::norm (NORM_L2) of a CV_32F 3x1: the squares accumulate in double; the double result
__host__ __device__ __forceinline__ double tri_norm3_d(float a0, float a1, float a2) {
  return sqrt(tri_dot3_d(a0, a1, a2, a0, a1, a2));
}

// OPENCV: lapack.cpp's own hypot template, instantiated for double by JacobiSVDImpl_'s hypot((double)p, beta)
__host__ __device__ __forceinline__ double tri_hypot_d(double a, double b) {
  a = fabs(a);
  b = fabs(b);
  if (a > b) {
    b /= a;
    return a * sqrt(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * sqrt(1 + a * a);
  }
  return 0;
}

// OPENCV: cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 CV_32F is JacobiSVDImpl_<float>
// on the transpose (At row i = column i of A) without LAPACK; v = vt.row(3) after the sort.
// A is row-major A[r][c].
__host__ __device__ inline void tri_svd4_vt_row3(const float A[4][4], float v[4]) {
  float At[4][4], Vt[4][4];
  double W[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float t = A[k][i];
      At[i][k] = t;
      sd += (double)t * t;  // OPENCV: row norms of At accumulate in double
      Vt[i][k] = i == k ? 1.0f : 0.0f;
    }
    W[i] = sd;
  }
  const float eps = FLT_EPSILON * 2;  // OPENCV: JacobiSVD(float*) passes eps = FLT_EPSILON * 2
  for (int iter = 0; iter < TRI_SVD_MAX_SWEEPS; iter++) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = i + 1; j < 4; j++) {  // OPENCV: column pairs in the fixed order i < j
        double a = W[i], p = 0, b = W[j];
#pragma unroll
        for (int k = 0; k < 4; k++) p += (double)At[i][k] * At[j][k];
        if (fabs(p) <= eps * sqrt(a * b)) continue;  // OPENCV: the skip test, eps * sqrt(a * b) in double
        p *= 2;
        const double beta = a - b, gamma = tri_hypot_d(p, beta);
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)sqrt(delta / gamma);
          c = (float)(p / (gamma * s * 2));
        } else {
          c = (float)sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * c * 2));
        }
        a = b = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float t0 = c * At[i][k] + s * At[j][k];
          const float t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0;
          At[j][k] = t1;
          a += (double)t0 * t0;
          b += (double)t1 * t1;
        }
        W[i] = a;
        W[j] = b;
        changed = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float t0 = c * Vt[i][k] + s * Vt[j][k];
          const float t1 = -s * Vt[i][k] + c * Vt[j][k];
          Vt[i][k] = t0;
          Vt[j][k] = t1;
        }
      }
    }
    if (!changed) break;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) sd += (double)At[i][k] * At[i][k];
    W[i] = sqrt(sd);
  }
  // OPENCV: singular values sorted descending by selection (W[j] < W[k] on the doubles), rows of Vt
  // swapped with them, signs as the rotations left them. The largest index is kept in a scalar.
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int j = i;
    double wj = W[i];
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (wj < W[k]) {
        j = k;
        wj = W[k];
      }
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (j == k) {
        const double tw = W[i];
        W[i] = W[k];
        W[k] = tw;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float tv = Vt[i][q];
          Vt[i][q] = Vt[k][q];
          Vt[k][q] = tv;
        }
      }
  }
#pragma unroll
  for (int q = 0; q < 4; q++) v[q] = Vt[3][q];
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:632-648) for depth z > 0. T / O: the KeyFrame's pose rows
// and camera centre (Twc = [Rcw^T | Ow]).
__host__ __device__ __forceinline__ void tri_unproject(const float* T, const float* O, const TriCam& c,
                                                       const TriObs& o, float* X) {
  const float z = o.depth;
  const float x = (o.kx - c.cx) * z * c.invfx;
  const float y = (o.ky - c.cy) * z * c.invfy;
  // OPENCV: Rwc * x3Dc + twc is one gemm with C: the double sum plus C in double, one rounding
  X[0] = (float)(tri_dot3_d(T[0], T[4], T[8], x, y, z) + (double)O[0]);
  X[1] = (float)(tri_dot3_d(T[1], T[5], T[9], x, y, z) + (double)O[1]);
  X[2] = (float)(tri_dot3_d(T[2], T[6], T[10], x, y, z) + (double)O[2]);
}

// The reprojection test of :367-392 / :394-418 in one KeyFrame. bf is always KF1's (:385, :411).
__host__ __device__ __forceinline__ bool tri_reproj_rejects(const float* T, const TriCam& c, const TriObs& o,
                                                            bool stereo, float bf, const float* X, float z) {
  const float x = (float)(tri_dot3_d(T[0], T[1], T[2], X[0], X[1], X[2]) + (double)T[3]);
  const float y = (float)(tri_dot3_d(T[4], T[5], T[6], X[0], X[1], X[2]) + (double)T[7]);
  const float invz = (float)(1.0 / (double)z);  // invz = 1.0 / z: a double quotient, narrowed
  const float u = c.fx * x * invz + c.cx;
  const float v = c.fy * y * invz + c.cy;
  const float ex = u - o.x;
  const float ey = v - o.y;
  if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)o.sigma2;  // a double comparison
  const float u_r = u - bf * invz;
  const float er = u_r - o.ur;
  return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)o.sigma2;  // a double comparison
}

// One match of :290-438. T1 / T2: GetPose() rows 0..2; O1 / O2: GetCameraCenter().
// X receives the world point when the returned status is > 0.
__host__ __device__ inline int tri_match(const float* T1, const float* O1, const TriCam& c1, const TriObs& o1,
                                         const float* T2, const float* O2, const TriCam& c2, const TriObs& o2,
                                         float ratio_factor, float* X) {
  const bool st1 = o1.ur >= 0, st2 = o2.ur >= 0;
  // OPENCV: Mat_<float>(3,1) << a, b, 1.0 stores each operand converted to float
  const float xn1[3] = {(o1.x - c1.cx) * c1.invfx, (o1.y - c1.cy) * c1.invfy, 1.0f};
  const float xn2[3] = {(o2.x - c2.cx) * c2.invfx, (o2.y - c2.cy) * c2.invfy, 1.0f};
  // ray = Rwc * xn, Rwc the transpose of the pose's rotation (gemm)
  const float r1[3] = {(float)tri_dot3_d(T1[0], T1[4], T1[8], xn1[0], xn1[1], xn1[2]),
                       (float)tri_dot3_d(T1[1], T1[5], T1[9], xn1[0], xn1[1], xn1[2]),
                       (float)tri_dot3_d(T1[2], T1[6], T1[10], xn1[0], xn1[1], xn1[2])};
  const float r2[3] = {(float)tri_dot3_d(T2[0], T2[4], T2[8], xn2[0], xn2[1], xn2[2]),
                       (float)tri_dot3_d(T2[1], T2[5], T2[9], xn2[0], xn2[1], xn2[2]),
                       (float)tri_dot3_d(T2[2], T2[6], T2[10], xn2[0], xn2[1], xn2[2])};
  // ray1.dot(ray2) / (norm(ray1) * norm(ray2)): all double, narrowed once
  const float cos_rays = (float)(tri_dot3_d(r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]) /
                                 (tri_norm3_d(r1[0], r1[1], r1[2]) * tri_norm3_d(r2[0], r2[1], r2[2])));
  float cos_st1 = cos_rays + 1, cos_st2 = cos_st1;
  // cos(2 * atan2(mb / 2, depth)) on floats under `using namespace std` (:316, :318):
  // LIBM: std::cos(float) is cosf
  // LIBM: std::atan2(float, float) is atan2f
  if (st1)
    cos_st1 = cosf(2 * atan2f(c1.b / 2, o1.depth));
  else if (st2)
    cos_st2 = cosf(2 * atan2f(c2.b / 2, o2.depth));
  const float cos_st = cos_st2 < cos_st1 ? cos_st2 : cos_st1;  // std::min(a, b): b < a ? b : a
  int status;
  if (cos_rays < cos_st && cos_rays > 0 && (st1 || st2 || (double)cos_rays < 0.9998)) {
    // OPENCV: a * M.row(r) - M.row(q) is one scaled add on floats: fl(fl(a * m_r) - m_q)
    float A[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      A[0][k] = xn1[0] * T1[8 + k] - T1[k];
      A[1][k] = xn1[1] * T1[8 + k] - T1[4 + k];
      A[2][k] = xn2[0] * T2[8 + k] - T2[k];
      A[3][k] = xn2[1] * T2[8 + k] - T2[4 + k];
    }
    float v[4];
    tri_svd4_vt_row3(A, v);
    if (v[3] == 0) return ORBFE_TRI_REJ_W_ZERO;
    const float inv = (float)(1.0 / (double)v[3]);  // OPENCV: Mat / scalar multiplies by (float)(1.0 / s)
    X[0] = v[0] * inv;
    X[1] = v[1] * inv;
    X[2] = v[2] * inv;
    status = ORBFE_TRI_TRIANGULATED;
  } else if (st1 && cos_st1 < cos_st2) {
    if (!(o1.depth > 0)) return ORBFE_TRI_REJ_UNPROJECT;
    tri_unproject(T1, O1, c1, o1, X);
    status = ORBFE_TRI_STEREO1;
  } else if (st2 && cos_st2 < cos_st1) {
    if (!(o2.depth > 0)) return ORBFE_TRI_REJ_UNPROJECT;
    tri_unproject(T2, O2, c2, o2, X);
    status = ORBFE_TRI_STEREO2;
  } else {
    return ORBFE_TRI_REJ_PARALLAX;
  }
  // Rcw.row(2).dot(x3Dt) + tcw(2): Mat::dot's double plus the float, narrowed by the assignment
  const float z1 = (float)(tri_dot3_d(T1[8], T1[9], T1[10], X[0], X[1], X[2]) + (double)T1[11]);
  if (z1 <= 0) return ORBFE_TRI_REJ_Z1;
  const float z2 = (float)(tri_dot3_d(T2[8], T2[9], T2[10], X[0], X[1], X[2]) + (double)T2[11]);
  if (z2 <= 0) return ORBFE_TRI_REJ_Z2;
  if (tri_reproj_rejects(T1, c1, o1, st1, c1.bf, X, z1)) return ORBFE_TRI_REJ_REPROJ1;
  if (tri_reproj_rejects(T2, c2, o2, st2, c1.bf, X, z2)) return ORBFE_TRI_REJ_REPROJ2;
  const float dist1 = (float)tri_norm3_d(X[0] - O1[0], X[1] - O1[1], X[2] - O1[2]);
  const float dist2 = (float)tri_norm3_d(X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]);
  if (dist1 == 0 || dist2 == 0) return ORBFE_TRI_REJ_DIST_ZERO;
  const float ratio_dist = dist2 / dist1;
  const float ratio_octave = o1.scale / o2.scale;
  if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor)
    return ORBFE_TRI_REJ_SCALE;
  return status;
}
