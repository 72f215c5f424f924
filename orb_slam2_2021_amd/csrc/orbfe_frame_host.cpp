// orbfe_frame_host.cpp -- the host entry points of include/orbfe_frame.h: the rules of
// orbfe_frame_core.h over host arrays, no device involved. Plain C++: compiled into liborbfe.so and,
// with ORBFE_FRAME_STANDALONE, into the stand-alone test program tests/cpp/frame_core_main.cpp
// (where the library's error record is absent and a status is only returned).
#include "orbfe_frame_core.h"

#ifdef ORBFE_FRAME_STANDALONE
static int orbfe_set_error(int code, const char*) { return code; }
#else
int orbfe_set_error(int code, const char* msg);  // orbfe_extract.hip
#endif

static bool depth_args_ok(const void* map, size_t pitch, int type, int rows, int cols) {
  if (!map) return true;
  if (type != ORBFE_DEPTH_U16 && type != ORBFE_DEPTH_F32) return false;
  const size_t elem = type == ORBFE_DEPTH_U16 ? 2 : 4;
  return rows > 0 && cols > 0 && pitch >= (size_t)cols * elem && pitch % elem == 0;
}

extern "C" int orbfe_image_bounds(const orbfe_camera* cam, int rows, int cols, float out[4]) {
  if (!frame_camera_ok(cam) || !out || rows < 0 || cols < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_image_bounds: bad argument");
  frame_image_bounds(*cam, rows, cols, out);
  return ORBFE_OK;
}

extern "C" int orbfe_undistort_keypoints_host(const orbfe_camera* cam, const orbfe_keypoint* keys, int n,
                                              orbfe_keypoint* keys_un) {
  if (!frame_camera_ok(cam) || n < 0 || (n > 0 && (!keys || !keys_un)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_undistort_keypoints_host: bad argument");
  const FrameUndist c = frame_undist(*cam);
  for (int i = 0; i < n; i++) keys_un[i] = frame_undistort_key(*cam, c, keys[i]);
  return ORBFE_OK;
}

extern "C" int orbfe_stereo_from_depth_host(const orbfe_camera* cam, const orbfe_keypoint* keys,
                                            const orbfe_keypoint* keys_un, int n, const void* depth_map,
                                            size_t depth_pitch, int depth_type, float depth_factor, int rows,
                                            int cols, float* u_right, float* depth) {
  if (!frame_camera_ok(cam) || n < 0 || (n > 0 && (!keys || !keys_un || !u_right || !depth)) ||
      !depth_args_ok(depth_map, depth_pitch, depth_type, rows, cols))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_stereo_from_depth_host: bad argument");
  for (int i = 0; i < n; i++)
    frame_stereo_from_depth(depth_map, depth_pitch, depth_type, depth_factor, rows, cols, keys[i].x, keys[i].y,
                            keys_un[i].x, cam->bf, &u_right[i], &depth[i]);
  return ORBFE_OK;
}
