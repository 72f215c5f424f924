// orbfe_frame_core.h -- the per-pixel and per-keypoint rules of the monocular and RGB-D Frames
// (include/orbfe_frame.h), one host/device inline function per rule: cvtColor's 8-bit gray,
// convertTo's depth value, cv::undistortPoints(src, dst, K, D, noArray(), K) for one point,
// Frame::UndistortKeyPoints' early-out, Frame::ComputeStereoFromRGBD and Frame::ComputeImageBounds
// (Tracking.cc:226-283, Frame.cc:456-520, 702-723). Used by the kernels of orbfe_frame.hip, by the
// host entry points of orbfe_frame_host.cpp and by the stand-alone host program
// tests/cpp/frame_core_main.cpp. Not part of the C ABI. tests/sensor_ref.py reaches the same
// results a second way.
//
// OpenCV's rules are restated as of 4.5.x (DESIGN.md "Monocular and RGB-D Frames"). The undistortion
// runs in double in exactly the order written, every operation rounded on its own (the library is
// built with -ffp-contract=off); gray is integer; the depth rules are single float operations.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbfe_frame.h"

#if defined(__HIPCC__)
#define FRAME_HD __host__ __device__
#else
#define FRAME_HD
#endif

// cvtColor, 8-bit: R2Y G2Y B2Y of color_yuv / color_rgb (4.x: 15 fractional bits; 2.4 / 3.x: 14),
// rounded to nearest by the added half.
FRAME_HD inline uint8_t frame_gray(unsigned r, unsigned g, unsigned b, int mode) {
  if (mode == ORBFE_GRAY_SHIFT14) return (uint8_t)((4899u * r + 9617u * g + 1868u * b + (1u << 13)) >> 14);
  return (uint8_t)((9798u * r + 19235u * g + 3735u * b + (1u << 14)) >> 15);
}

// One interleaved pixel: channel 0 is R when rgb != 0 (mbRGB, Tracking.cc:236-247), else B; a fourth
// channel (alpha) is never read.
FRAME_HD inline uint8_t frame_gray_px(unsigned c0, unsigned c1, unsigned c2, int rgb, int mode) {
  return rgb ? frame_gray(c0, c1, c2, mode) : frame_gray(c2, c1, c0, mode);
}

// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:246-247) for the one value read:
// applied when the factor differs from 1 by more than 1e-5 (a float difference against the double
// literal) or the map is not float.
FRAME_HD inline bool frame_depth_converts(int depth_type, float factor) {
  const float d = factor - 1.0f;
  return (double)(d < 0 ? -d : d) > 1e-5 || depth_type != ORBFE_DEPTH_F32;
}
FRAME_HD inline float frame_depth_value(const void* row, int x, int depth_type, float factor) {
  if (depth_type == ORBFE_DEPTH_U16) return (float)static_cast<const uint16_t*>(row)[x] * factor;
  const float raw = static_cast<const float*>(row)[x];
  return frame_depth_converts(depth_type, factor) ? raw * factor : raw;
}

// mDistCoef.at<float>(0) == 0.0 (Frame.cc:458, :490): no undistortion at all, whatever the other
// coefficients hold; -0.0f compares equal.
FRAME_HD inline bool frame_distorted(const orbfe_camera& cam) { return !(cam.dist[0] == 0.0f); }

// The camera as cv::undistortPoints holds it: everything converted to double once.
struct FrameUndist {
  double fx, fy, cx, cy, ifx, ify;
  double k[12];  // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4; from k[5] on zero here
};
FRAME_HD inline FrameUndist frame_undist(const orbfe_camera& cam) {
  FrameUndist u;
  u.fx = (double)cam.fx;
  u.fy = (double)cam.fy;
  u.cx = (double)cam.cx;
  u.cy = (double)cam.cy;
  u.ifx = 1. / u.fx;
  u.ify = 1. / u.fy;
  for (int i = 0; i < 12; i++) u.k[i] = 0.;
  for (int i = 0; i < 5 && i < cam.n_dist; i++) u.k[i] = (double)cam.dist[i];
  return u;
}

// cvUndistortPointsInternal for one CV_32FC2 point with R = I, P = K and the default criteria
// (5 iterations, no epsilon test); the tilt matrices are the identity.
FRAME_HD inline void frame_undistort_point(const FrameUndist& c, float px, float py, float* ox, float* oy) {
  const double* k = c.k;
  double x = (double)px, y = (double)py;
  const double u = x, v = y;
  x = (x - c.cx) * c.ifx;
  y = (y - c.cy) * c.ify;
  const double x0 = x, y0 = y;
  for (int j = 0; j < 5; j++) {
    const double r2 = x * x + y * y;
    const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
    if (icdist < 0) {  // test: undistortPoints("bad" distortion): the point stays where it was
      x = (u - c.cx) * c.ifx;
      y = (v - c.cy) * c.ify;
      break;
    }
    const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
    const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  // the 3x3 product with [fx 0 cx; 0 fy cy; 0 0 1], the zero terms kept as OpenCV evaluates them
  const double xx = c.fx * x + 0. * y + c.cx;
  const double yy = 0. * x + c.fy * y + c.cy;
  const double ww = 1. / (0. * x + 0. * y + 1.);
  *ox = (float)(xx * ww);
  *oy = (float)(yy * ww);
}

// Frame::UndistortKeyPoints for one keypoint: kp = mvKeys[i] with pt replaced (Frame.cc:481-484).
FRAME_HD inline orbfe_keypoint frame_undistort_key(const orbfe_camera& cam, const FrameUndist& c,
                                                   const orbfe_keypoint& kp) {
  orbfe_keypoint o = kp;
  if (frame_distorted(cam)) frame_undistort_point(c, kp.x, kp.y, &o.x, &o.y);
  return o;
}

// Frame::ComputeStereoFromRGBD for one keypoint (Frame.cc:707-722): d = imDepth.at<float>(v, u) with
// the float coordinates of the DISTORTED key truncated; d > 0 fails for zero, negative and NaN.
// map == NULL (monocular) and a truncated position outside rows x cols give -1 / -1.
FRAME_HD inline void frame_stereo_from_depth(const void* map, size_t pitch, int depth_type, float factor,
                                             int rows, int cols, float kx, float ky, float kun_x, float bf,
                                             float* u_right, float* depth) {
  *u_right = -1.0f;
  *depth = -1.0f;
  if (!map) return;
  if (!(kx >= 0.0f && kx < (float)cols && ky >= 0.0f && ky < (float)rows)) return;
  const int u = (int)kx, v = (int)ky;
  const float d = frame_depth_value(static_cast<const uint8_t*>(map) + (size_t)v * pitch, u, depth_type, factor);
  if (d > 0) {
    *depth = d;
    *u_right = kun_x - bf / d;
  }
}

// Frame::ComputeImageBounds (Frame.cc:488-520): out = {mnMinX, mnMaxX, mnMinY, mnMaxY}.
// std::min(a, b) is (b < a) ? b : a and std::max(a, b) is (a < b) ? b : a, also for NaN.
FRAME_HD inline void frame_image_bounds(const orbfe_camera& cam, int rows, int cols, float out[4]) {
  if (!frame_distorted(cam)) {
    out[0] = 0.0f;
    out[1] = (float)cols;
    out[2] = 0.0f;
    out[3] = (float)rows;
    return;
  }
  const FrameUndist c = frame_undist(cam);
  const float sx[4] = {0.0f, (float)cols, 0.0f, (float)cols};
  const float sy[4] = {0.0f, 0.0f, (float)rows, (float)rows};
  float x[4], y[4];
  for (int i = 0; i < 4; i++) frame_undistort_point(c, sx[i], sy[i], &x[i], &y[i]);
  out[0] = (x[2] < x[0]) ? x[2] : x[0];
  out[1] = (x[1] < x[3]) ? x[3] : x[1];
  out[2] = (y[1] < y[0]) ? y[1] : y[0];
  out[3] = (y[2] < y[3]) ? y[3] : y[2];
}

FRAME_HD inline bool frame_camera_ok(const orbfe_camera* cam) {
  return cam && (cam->n_dist == 4 || cam->n_dist == 5);
}
