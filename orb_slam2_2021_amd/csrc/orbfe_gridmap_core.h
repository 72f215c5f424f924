// orbfe_gridmap_core.h -- the rules of the occupancy grid (include/orbfe_gridmap.h), one host/device
// inline function per rule: the grid of a geometry, the cell of a position, CastLaserBeam's swaps and
// its step, the flat index of a visit, and the message of a cell (GridMapping.cpp:72-154, 232-270).
// Used by the kernels of orbfe_gridmap.hip, by the host entry points of orbfe_gridmap_host.cpp and by
// the stand-alone host program tests/cpp/gridmap_core_main.cpp. Not part of the C ABI.
// tests/gridmap_ref.py reaches the same results a second way.
//
// The beam's error term accumulates in double, one add per step, and is compared with 0.5: that is
// not exact integer Bresenham (the first (dx, dy) at which the two differ is (10, 3)), so every user
// replays the same adds in the same order through gm_beam_step. The library is built with
// -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbfe_gridmap.h"

#if defined(__HIPCC__)
#define GM_HD __host__ __device__
#else
#define GM_HD
#endif

struct GmGrid {
  int32_t scale, rows, cols, visit_threshold;
  float min_x, min_z, norm_x, norm_z;
};

// InitGridMap (:72-107). A size is the float difference of its two ends.
inline int gm_grid_of(const orbfe_gridmap_geometry* g, GmGrid* out) {
  if (!g || !out || g->scale_factor < 1 || g->visit_threshold < 0) return ORBFE_ERR_ARG;
  if (!isfinite(g->min_x) || !isfinite(g->max_x) || !isfinite(g->min_z) || !isfinite(g->max_z)) return ORBFE_ERR_ARG;
  const float fc = g->max_x - g->min_x, fr = g->max_z - g->min_z;
  if (!(fc >= 1.0f) || !(fr >= 1.0f) || fc != floorf(fc) || fr != floorf(fr)) return ORBFE_ERR_ARG;
  if ((double)fc * (double)fr >= 2147483648.0) return ORBFE_ERR_CAPACITY;
  out->scale = g->scale_factor;
  out->cols = (int32_t)fc;
  out->rows = (int32_t)fr;
  out->visit_threshold = g->visit_threshold;
  out->min_x = g->min_x;
  out->min_z = g->min_z;
  out->norm_x = (float)(out->cols - 1) / (float)out->cols;
  out->norm_z = (float)(out->rows - 1) / (float)out->rows;
  return ORBFE_OK;
}

// One coordinate's cell (:111-114, :122-126), or -1 when it is outside [0, size). A NaN and a floored
// value beyond the int range are outside (the reference's conversion of those is undefined).
GM_HD inline int gm_cell(float p, int scale, float lo, float norm, int size) {
  const float g = p * (float)scale;
  const float c = (g - lo) * norm;
  const float f = floorf(c);
  if (!(f >= 0.0f && f < 2147483648.0f)) return -1;
  const int i = (int)f;
  return i < size ? i : -1;
}

// CastLaserBeam up to its loop (:234-252). x0, y0 are rewritten as the reference's by-reference
// arguments are: under REFERENCE rules they are the next beam's start.
struct GmBeam {
  int x, x1, y, ystep, steep;
  double deltaerr;
};
GM_HD inline int gm_iabs(int v) { return v < 0 ? -v : v; }
// the two swaps (:234-244): steep exchanges the axes, the second orders the ends; returns steep
GM_HD inline int gm_beam_swaps(int& x0, int& y0, int& x1, int& y1) {
  const int steep = gm_iabs(y1 - y0) > gm_iabs(x1 - x0);
  int t;
  if (steep) {
    t = x0, x0 = y0, y0 = t;
    t = x1, x1 = y1, y1 = t;
  }
  if (x0 > x1) {
    t = x0, x0 = x1, x1 = t;
    t = y0, y0 = y1, y1 = t;
  }
  return steep;
}
GM_HD inline GmBeam gm_beam_setup(int& x0, int& y0, int x1, int y1) {
  GmBeam b;
  b.steep = gm_beam_swaps(x0, y0, x1, y1);
  const int dx = x1 - x0, dy = gm_iabs(y1 - y0);
  b.deltaerr = (double)dy / (double)dx;  // a zero-length beam: 0 / 0, a NaN that never reaches 0.5
  b.x = x0;
  b.x1 = x1;
  b.y = y0;
  b.ystep = y0 < y1 ? 1 : -1;
  return b;
}
// cells the beam visits, both ends included
GM_HD inline int gm_beam_steps(const GmBeam& b) { return b.x1 - b.x + 1; }

// The flat index the visit at (x, y) addresses (:255-262), or -1 when it lies beyond the buffer.
GM_HD inline long long gm_visit_index(int x, int y, int steep, int rows, int cols) {
  const long long flat = steep ? (long long)x * cols + y : (long long)y * cols + x;
  return flat >= 0 && flat < (long long)rows * cols ? flat : -1;
}

// The loop body after the visit (:263-268).
GM_HD inline void gm_beam_step(int& y, double& error, double deltaerr, int ystep) {
  error = error + deltaerr;
  if (error >= 0.5) {
    y = y + ystep;
    error = error - 1.0;
  }
}

// BuildOccupancyGridMsg for one cell (:143-151).
GM_HD inline float gm_cell_data(int oc, int vc, int visit_threshold) {
  return vc <= visit_threshold ? 1.0f : 1.0f - (float)oc / (float)vc;
}
GM_HD inline int8_t gm_cell_msg(float data) {
  const float v = (1.0f - data) * 100.0f;
  return v >= 127.0f ? (int8_t)127 : v <= -128.0f ? (int8_t)-128 : (int8_t)(int)v;
}

// ---- the serial composition on the host --------------------------------------------------------

inline int gm_check_update(int n_kf, const float* centres, const int32_t* begin, const float* world_pos) {
  if (n_kf < 1 || !centres || !begin) return ORBFE_ERR_ARG;
  if (n_kf > ORBFE_GRIDMAP_MAX_KEYFRAMES) return ORBFE_ERR_CAPACITY;
  if (begin[0] != 0) return ORBFE_ERR_ARG;
  for (int k = 0; k < n_kf; k++)
    if (begin[k + 1] < begin[k]) return ORBFE_ERR_ARG;
  for (int k = 0; k < n_kf; k++)
    if (begin[k + 1] - begin[k] > ORBFE_GRIDMAP_MAX_POINTS) return ORBFE_ERR_CAPACITY;
  if (begin[n_kf] > 0 && !world_pos) return ORBFE_ERR_ARG;
  return ORBFE_OK;
}

struct GmTally {
  int64_t beams = 0, visits = 0, dropped = 0, points_cut = 0;
  int32_t kf_outside = 0, row0 = INT32_MAX, row1 = -1;  // rows touched: row0 .. row1 inclusive
  void touch(int row) {
    if (row < row0) row0 = row;
    if (row > row1) row1 = row;
  }
  void to(orbfe_gridmap_stats* s) const {
    s->beams = beams;
    s->visits = visits;
    s->dropped = dropped;
    s->points_cut = points_cut;
    s->kf_outside = kf_outside;
    s->row0 = row1 < 0 ? 0 : row0;
    s->row1 = row1 < 0 ? 0 : row1 + 1;
  }
};

// UpdateGridMap (:109-135) of one keyframe with n points.
inline void gm_host_keyframe(const GmGrid& g, int rules, const float* centre, const float* pos, int n, int32_t* occupied,
                             int32_t* visits, GmTally* t) {
  int kx = gm_cell(centre[0], g.scale, g.min_x, g.norm_x, g.cols);
  int kz = gm_cell(centre[2], g.scale, g.min_z, g.norm_z, g.rows);
  if (kx < 0 || kz < 0) {
    t->kf_outside++;
    return;
  }
  const int kx0 = kx, kz0 = kz;
  for (int i = 0; i < n; i++) {
    const int px = gm_cell(pos[3 * (size_t)i], g.scale, g.min_x, g.norm_x, g.cols);
    const int pz = gm_cell(pos[3 * (size_t)i + 2], g.scale, g.min_z, g.norm_z, g.rows);
    if (px < 0 || pz < 0) {
      if (rules == ORBFE_GRIDMAP_REFERENCE) {
        t->points_cut += n - i;
        return;
      }
      t->points_cut++;
      continue;
    }
    ++occupied[(size_t)pz * g.cols + px];
    t->touch(pz);
    if (rules != ORBFE_GRIDMAP_REFERENCE) kx = kx0, kz = kz0;
    GmBeam b = gm_beam_setup(kx, kz, px, pz);
    t->beams++;
    double error = 0;
    int y = b.y;
    for (int x = b.x; x <= b.x1; ++x) {
      const long long flat = gm_visit_index(x, y, b.steep, g.rows, g.cols);
      if (flat < 0) {
        t->dropped++;
      } else {
        ++visits[flat];
        t->visits++;
        t->touch((int)(flat / g.cols));
      }
      gm_beam_step(y, error, b.deltaerr, b.ystep);
    }
  }
}
