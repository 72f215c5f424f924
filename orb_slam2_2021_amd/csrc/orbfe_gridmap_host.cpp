// orbfe_gridmap_host.cpp -- the host entry points of include/orbfe_gridmap.h: the rules of
// orbfe_gridmap_core.h over host arrays, no device involved. Plain C++: compiled into liborbfe.so and,
// with ORBFE_GRIDMAP_STANDALONE, into the stand-alone test program tests/cpp/gridmap_core_main.cpp
// (where the library's error record is absent and a status is only returned).
#include "orbfe_gridmap_core.h"

#ifdef ORBFE_GRIDMAP_STANDALONE
static int orbfe_set_error(int code, const char*) { return code; }
#else
int orbfe_set_error(int code, const char* msg);  // orbfe_extract.hip
#endif

extern "C" int orbfe_gridmap_default_geometry(orbfe_gridmap_geometry* g) {
  if (!g) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_default_geometry: bad argument");
  g->scale_factor = 3;
  g->max_x = (float)(1000 * g->scale_factor);
  g->max_z = (float)(1600 * g->scale_factor);
  g->min_x = (float)(-1000 * g->scale_factor);
  g->min_z = (float)(-500 * g->scale_factor);
  g->visit_threshold = 0;
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_dims(const orbfe_gridmap_geometry* g, int32_t* rows, int32_t* cols, float* norm_x,
                                  float* norm_z) {
  GmGrid grid;
  const int st = gm_grid_of(g, &grid);
  if (st) return orbfe_set_error(st, "orbfe_gridmap_dims: bad geometry");
  if (rows) *rows = grid.rows;
  if (cols) *cols = grid.cols;
  if (norm_x) *norm_x = grid.norm_x;
  if (norm_z) *norm_z = grid.norm_z;
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_host_update(const orbfe_gridmap_geometry* g, int rules, int32_t* occupied,
                                         int32_t* visits, int n_kf, const float* centres, const int32_t* begin,
                                         const float* world_pos, orbfe_gridmap_stats* stats) {
  GmGrid grid;
  int st = gm_grid_of(g, &grid);
  if (st) return orbfe_set_error(st, "orbfe_gridmap_host_update: bad geometry");
  if (!occupied || !visits || (rules != ORBFE_GRIDMAP_REFERENCE && rules != ORBFE_GRIDMAP_INTENDED))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_host_update: bad argument");
  st = gm_check_update(n_kf, centres, begin, world_pos);
  if (st) return orbfe_set_error(st, "orbfe_gridmap_host_update: bad keyframe list");
  GmTally t;
  for (int k = 0; k < n_kf; k++)
    gm_host_keyframe(grid, rules, centres + 3 * (size_t)k, world_pos + 3 * (size_t)begin[k], begin[k + 1] - begin[k],
                     occupied, visits, &t);
  if (stats) t.to(stats);
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_host_build(const orbfe_gridmap_geometry* g, const int32_t* occupied,
                                        const int32_t* visits, int row0, int row1, int8_t* grid_out, float* data) {
  GmGrid grid;
  const int st = gm_grid_of(g, &grid);
  if (st) return orbfe_set_error(st, "orbfe_gridmap_host_build: bad geometry");
  if (!occupied || !visits || !grid_out || row0 < 0 || row1 < row0 || row1 > grid.rows)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_host_build: bad argument");
  const size_t lo = (size_t)row0 * grid.cols, hi = (size_t)row1 * grid.cols;
  for (size_t i = lo; i < hi; i++) {
    const float d = gm_cell_data(occupied[i], visits[i], grid.visit_threshold);
    if (data) data[i - lo] = d;
    grid_out[i - lo] = gm_cell_msg(d);
  }
  return ORBFE_OK;
}
