// orbfe_rectify_host.cpp -- the host entry points of include/orbfe_rectify.h: the rules of
// orbfe_rectify_core.h over host arrays, no device involved. Plain C++: compiled into liborbfe.so and,
// with ORBFE_RECTIFY_STANDALONE, into the stand-alone test program tests/cpp/rectify_core_main.cpp
// (where the library's error record is absent and a status is only returned).
#include <vector>

#include "orbfe_rectify_core.h"

#ifdef ORBFE_RECTIFY_STANDALONE
static int orbfe_set_error(int code, const char*) { return code; }
#else
int orbfe_set_error(int code, const char* msg);  // orbfe_extract.hip
#endif

extern "C" int orbfe_rectify_maps_host(const double* K, const double* D, int n_dist, const double* R,
                                       const double* P3, int rows, int cols, float* map1, float* map2) {
  if (!K || !D || (n_dist != 4 && n_dist != 5) || !P3 || rows <= 0 || cols <= 0 || !map1 || !map2)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_maps_host: bad argument");
  const double eye[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
  double ir[9], k[5] = {0., 0., 0., 0., 0.};
  if (!rectify_inverse(P3, R ? R : eye, ir))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_maps_host: P * R is singular");
  for (int i = 0; i < n_dist; i++) k[i] = D[i];
  for (int i = 0; i < rows; i++)
    rectify_map_row(ir, k, K[0], K[4], K[2], K[5], i, cols, map1 + (size_t)i * cols, map2 + (size_t)i * cols);
  return ORBFE_OK;
}

extern "C" int orbfe_rectify_entries_host(const float* map1, const float* map2, int rows, int cols, int src_rows,
                                          int src_cols, orbfe_rectify_entry* entries) {
  if (!map1 || !map2 || !entries || !rectify_sizes_ok(src_rows, src_cols, rows, cols))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_entries_host: bad argument");
  for (size_t i = 0; i < (size_t)rows * cols; i++) entries[i] = rectify_entry(map1[i], map2[i], src_rows, src_cols);
  return ORBFE_OK;
}

template <int C, bool GRAY>
static void remap_rows(const uint8_t* src, int src_rows, int src_cols, size_t src_pitch, const uint8_t* map1,
                       const uint8_t* map2, size_t map_pitch, int dst_cols, int row0, int row1, int rgb, int mode,
                       uint8_t* dst, size_t dst_pitch) {
  std::vector<RectifyEntry> ent((size_t)dst_cols);
  const int width = dst_cols * (GRAY ? 1 : C);
  for (int y = row0; y < row1; y++) {
    const float* m1 = reinterpret_cast<const float*>(map1 + (size_t)y * map_pitch);
    const float* m2 = reinterpret_cast<const float*>(map2 + (size_t)y * map_pitch);
    for (int x = 0; x < dst_cols; x++) ent[x] = rectify_entry(m1[x], m2[x], src_rows, src_cols);
    uint8_t* drow = dst + (size_t)(y - row0) * dst_pitch;
    for (int xb = 0; xb < width; xb++)
      drow[xb] = rectify_byte<C, GRAY>(src, src_pitch, src_rows, src_cols, ent[rectify_pixel_of<C, GRAY>(xb)], xb, rgb, mode);
  }
}

extern "C" int orbfe_remap_host(const uint8_t* src, int src_rows, int src_cols, size_t src_pitch, int channels,
                                const float* map1, const float* map2, size_t map_pitch, int dst_rows, int dst_cols,
                                int row0, int row1, int rgb, int gray_mode, int gray_out, uint8_t* dst,
                                size_t dst_pitch) {
  if (!src || !map1 || !map2 || !dst || !rectify_sizes_ok(src_rows, src_cols, dst_rows, dst_cols) ||
      !rectify_format_ok(channels, gray_mode) || src_pitch < (size_t)src_cols * channels ||
      map_pitch < (size_t)dst_cols * sizeof(float) || map_pitch % sizeof(float) != 0 || row0 < 0 || row1 < row0 ||
      row1 > dst_rows || dst_pitch < (size_t)dst_cols * rectify_out_channels(channels, gray_out))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_remap_host: bad argument");
  const uint8_t* b1 = reinterpret_cast<const uint8_t*>(map1);
  const uint8_t* b2 = reinterpret_cast<const uint8_t*>(map2);
#define REMAP_ROWS(C, G) \
  remap_rows<C, G>(src, src_rows, src_cols, src_pitch, b1, b2, map_pitch, dst_cols, row0, row1, rgb ? 1 : 0, gray_mode, dst, dst_pitch)
  const bool g = rectify_gray_fused(channels, gray_out);
  if (channels == 1)
    REMAP_ROWS(1, false);
  else if (channels == 3)
    g ? REMAP_ROWS(3, true) : REMAP_ROWS(3, false);
  else
    g ? REMAP_ROWS(4, true) : REMAP_ROWS(4, false);
#undef REMAP_ROWS
  return ORBFE_OK;
}
