// orbfe_rectify_core.h -- the rules of stereo rectification (include/orbfe_rectify.h), one host/device
// inline function per rule: cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F) for one row, cv::remap's
// conversion of a float map pair to its fixed-point entry, its 8-bit bilinear blend, and BORDER_CONSTANT 0
// (Examples/Stereo/arducam_images.cpp:123-133, 229-275 of the reference). Used by the kernels of
// orbfe_rectify.hip, by the host entry points of orbfe_rectify_host.cpp and by the stand-alone host program
// tests/cpp/rectify_core_main.cpp. Not part of the C ABI. tests/rectify_ref.py reaches the same results a
// second way.
//
// OpenCV's rules are restated as of 4.5.x. The maps run in double in exactly the
// order written, every operation rounded on its own (-ffp-contract=off); the entry is one float product
// per coordinate, rounded half to even; the blend is integer.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbfe_rectify.h"
#include "orbfe_frame_core.h"

// One destination pixel of a plan: the top-left tap, the two 5-bit fractions (alpha = b * 32 + a) and
// whether the pixel is the border constant. 8 bytes, so that a pixel costs one load.
typedef orbfe_rectify_entry RectifyEntry;
static_assert(sizeof(RectifyEntry) == 8, "a plan entry is one 8-byte load");

// remap's fixed-point grid: INTER_BITS = 5, and source sizes the short taps can address.
#define RECTIFY_MAX_SRC 32766

// Rule 1, once per calibration: iR = inv(P3 * R). The product accumulates a0*b0 + a1*b1 + a2*b2 in that
// order; the inverse is OpenCV's closed form for n = 3 (d = 1./det3, each cofactor times d). False when
// the determinant is zero.
inline bool rectify_inverse(const double P3[9], const double R[9], double ir[9]) {
  double m[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = P3[3 * i] * R[j];
      s = s + P3[3 * i + 1] * R[3 + j];
      s = s + P3[3 * i + 2] * R[6 + j];
      m[3 * i + j] = s;
    }
  double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
             m[2] * (m[3] * m[7] - m[4] * m[6]);
  if (d == 0.) return false;
  d = 1. / d;
  ir[0] = (m[4] * m[8] - m[5] * m[7]) * d;
  ir[1] = (m[2] * m[7] - m[1] * m[8]) * d;
  ir[2] = (m[1] * m[5] - m[2] * m[4]) * d;
  ir[3] = (m[5] * m[6] - m[3] * m[8]) * d;
  ir[4] = (m[0] * m[8] - m[2] * m[6]) * d;
  ir[5] = (m[2] * m[3] - m[0] * m[5]) * d;
  ir[6] = (m[3] * m[7] - m[4] * m[6]) * d;
  ir[7] = (m[1] * m[6] - m[0] * m[7]) * d;
  ir[8] = (m[0] * m[4] - m[1] * m[3]) * d;
  return true;
}

// Rule 1, row i of the maps: the three homogeneous coordinates start at the row's own value and advance by
// running adds along the row (the scalar loop of initUndistortRectifyMap); k4 = k5 = k6 = 0, the thin-prism
// terms and the identity tilt are kept as the literal zeros and ones OpenCV multiplies by.
// k: k1 k2 p1 p2 k3. fx, fy, u0, v0: the entries of K.
inline void rectify_map_row(const double ir[9], const double k[5], double fx, double fy, double u0, double v0,
                            int i, int cols, float* m1, float* m2) {
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  const double k4 = 0., k5 = 0., k6 = 0., s1 = 0., s2 = 0., s3 = 0., s4 = 0., invProj = 1.;
  double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
  for (int j = 0; j < cols; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
    const double w = 1. / _w, x = _x * w, y = _y * w;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2);
    const double yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2);
    const double u = fx * invProj * xd + u0;
    const double v = fy * invProj * yd + v0;
    m1[j] = (float)u;
    m2[j] = (float)v;
  }
}

// Rules 2 and 4: one float map pair to its entry. cvRound(m * 32.f) is a float product rounded half to even
// (rintf in the default rounding mode; v_rndne_f32 on the device). A product that is not finite or does not
// fit an int has no defined conversion in the reference: it is the border constant here, with zero fields.
FRAME_HD inline int16_t rectify_sat_short(int v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }
FRAME_HD inline RectifyEntry rectify_entry(float m1, float m2, int src_rows, int src_cols) {
  RectifyEntry e;
  const float px = m1 * 32.f, py = m2 * 32.f;
  if (!(px >= -2147483648.f && px < 2147483648.f && py >= -2147483648.f && py < 2147483648.f)) {
    e.ix = e.iy = 0;
    e.alpha = 0;
    e.outside = 1;
    return e;
  }
  const int sx = (int)rintf(px), sy = (int)rintf(py);
  e.ix = rectify_sat_short(sx >> 5);
  e.iy = rectify_sat_short(sy >> 5);
  e.alpha = (uint16_t)((sy & 31) * 32 + (sx & 31));
  const int ix = e.ix, iy = e.iy;
  e.outside = (ix >= src_cols || ix + 1 < 0 || iy >= src_rows || iy + 1 < 0) ? 1 : 0;
  return e;
}

// Rule 3: the four weights 32(32-a)(32-b), 32a(32-b), 32(32-a)b, 32ab sum to 32768. OpenCV stores them as
// shorts, so for a = b = 0 it keeps 32767 and gives the missing 1 to a neighbour; for bytes p, q
// (32767 p + q + 16384) >> 15 == p, so the exact weights give the same 8-bit result.
FRAME_HD inline unsigned rectify_blend(unsigned p00, unsigned p01, unsigned p10, unsigned p11, unsigned a,
                                       unsigned b) {
  const unsigned na = 32u - a, nb = 32u - b;
  return (32u * na * nb * p00 + 32u * a * nb * p01 + 32u * na * b * p10 + 32u * a * b * p11 + (1u << 14)) >> 15;
}

// Rules 3 and 4 for channel c of one destination pixel that is not `outside`: a tap outside the source
// reads 0 with the same weights and rounding.
template <int C>
FRAME_HD inline unsigned rectify_channel(const uint8_t* src, size_t pitch, int rows, int cols, RectifyEntry e,
                                         int c) {
  const int x0 = e.ix, y0 = e.iy;
  const bool l = x0 >= 0, r = x0 + 1 < cols, t = y0 >= 0, d = y0 + 1 < rows;
  const ptrdiff_t sp = (ptrdiff_t)pitch, o = (ptrdiff_t)y0 * sp + (ptrdiff_t)x0 * C + c;  // only valid taps are read
  const unsigned p00 = (t && l) ? src[o] : 0u;
  const unsigned p01 = (t && r) ? src[o + C] : 0u;
  const unsigned p10 = (d && l) ? src[o + sp] : 0u;
  const unsigned p11 = (d && r) ? src[o + sp + C] : 0u;
  return rectify_blend(p00, p01, p10, p11, e.alpha & 31u, (unsigned)e.alpha >> 5);
}

// Rule 5 for output byte `xb` of a destination row: remap on the image as it comes, each channel rounded to
// its byte, then gray rule 1 of orbfe_frame_core.h on those bytes when GRAY. A GRAY row has one byte per
// pixel, a colour row C: rectify_pixel_of(xb) is the pixel whose entry `e` the byte needs.
template <int C, bool GRAY>
FRAME_HD inline int rectify_pixel_of(int xb) {
  return GRAY ? xb : xb / C;
}
template <int C, bool GRAY>
FRAME_HD inline uint8_t rectify_byte(const uint8_t* src, size_t pitch, int rows, int cols, RectifyEntry e, int xb,
                                     int rgb, int mode) {
  if (GRAY) {
    if (e.outside) return frame_gray_px(0, 0, 0, rgb, mode);
    return frame_gray_px(rectify_channel<C>(src, pitch, rows, cols, e, 0),
                         rectify_channel<C>(src, pitch, rows, cols, e, 1),
                         rectify_channel<C>(src, pitch, rows, cols, e, 2), rgb, mode);
  }
  if (e.outside) return 0;
  return (uint8_t)rectify_channel<C>(src, pitch, rows, cols, e, xb % C);
}

// What the entry points share: the arguments of a remap.
FRAME_HD inline bool rectify_gray_fused(int channels, int gray_out) { return channels != 1 && gray_out != 0; }
FRAME_HD inline int rectify_out_channels(int channels, int gray_out) {
  return rectify_gray_fused(channels, gray_out) ? 1 : channels;
}
inline bool rectify_sizes_ok(int src_rows, int src_cols, int dst_rows, int dst_cols) {
  return src_rows > 0 && src_cols > 0 && src_rows <= RECTIFY_MAX_SRC && src_cols <= RECTIFY_MAX_SRC && dst_rows > 0 &&
         dst_cols > 0;
}
inline bool rectify_format_ok(int channels, int gray_mode) {
  return (channels == 1 || channels == 3 || channels == 4) &&
         (gray_mode == ORBFE_GRAY_SHIFT15 || gray_mode == ORBFE_GRAY_SHIFT14);
}
