// orbfe_frame.hip -- the monocular and RGB-D Frames' per-frame steps for gfx950 (include/orbfe_frame.h):
//   k_gray          cvtColor(*2GRAY) of a batch of interleaved 3- or 4-channel images into the 8-bit
//                   planes the extractor takes (Tracking.cc:226-283).
//   k_frame_finish  Frame::UndistortKeyPoints and Frame::ComputeStereoFromRGBD for every keypoint of a
//                   batch in one launch (Frame.cc:456-486, 702-723).
// Both apply the rules of orbfe_frame_core.h, which the host entry points (orbfe_frame_host.cpp) share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/orbfe.h"
#include "../../include/orbfe_frame.h"
#include "orbfe_device.h"
#include "orbfe_frame_core.h"
#include "orbfe_internal.h"
#include "orbfe_ktimer.h"

namespace {

// ---- k_gray -------------------------------------------------------------------------------------
// Memory bound: C bytes in and one out per pixel. A lane owns four adjacent pixels whose output is one
// aligned dword of the destination row: it loads the aligned dwords that cover its 4*C source bytes
// (C of them, one more when the row's source address is not dword-aligned), shifts them into place
// and stores one dword. Neighbouring lanes read neighbouring 12- or 16-byte pieces, so a wave reads
// 768 or 1024 contiguous bytes and writes 256. The pixels in front of a row's first aligned
// destination dword and behind its last (at most three each) go bytewise through one lane per row.
// Every dword loaded holds at least one byte of the row, so no load leaves the dwords the image occupies.
constexpr int GRAY_ROWS = 4;  // rows per workgroup, one wave each

struct GrayArgs {
  const uint8_t* src;
  uint8_t* dst;
  long long src_stride, dst_stride, src_pitch, dst_pitch;
  int rows, cols, rgb, mode;
};

template <int C>
__global__ __launch_bounds__(64 * GRAY_ROWS) void k_gray(GrayArgs a) {
  const int row = blockIdx.y * GRAY_ROWS + threadIdx.y;
  if (row >= a.rows) return;
  const uint8_t* __restrict__ srow = a.src + (long long)blockIdx.z * a.src_stride + (long long)row * a.src_pitch;
  uint8_t* __restrict__ drow = a.dst + (long long)blockIdx.z * a.dst_stride + (long long)row * a.dst_pitch;
  const int head = min(a.cols, (int)((4u - (unsigned)((uintptr_t)drow & 3u)) & 3u));
  const int groups = (a.cols - head) >> 2;
  for (int u = blockIdx.x * 64 + threadIdx.x; u <= groups; u += gridDim.x * 64) {
    if (u < groups) {
      const int x = head + 4 * u;
      const uint8_t* p = srow + (long long)x * C;
      const unsigned sh = (unsigned)((uintptr_t)p & 3u);
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
      uint32_t w[C + 1], b[C];
#pragma unroll
      for (int k = 0; k < C; k++) w[k] = q[k];
      w[C] = sh ? q[C] : 0u;
#pragma unroll
      for (int k = 0; k < C; k++) b[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
      auto byte = [&](int i) { return (b[i >> 2] >> (8 * (i & 3))) & 255u; };
      uint32_t out = 0;
#pragma unroll
      for (int j = 0; j < 4; j++)
        out |= (uint32_t)frame_gray_px(byte(C * j), byte(C * j + 1), byte(C * j + 2), a.rgb, a.mode) << (8 * j);
      *reinterpret_cast<uint32_t*>(drow + x) = out;
    } else {
      auto one = [&](int x) {
        const uint8_t* p = srow + (long long)x * C;
        drow[x] = frame_gray_px(p[0], p[1], p[2], a.rgb, a.mode);
      };
      for (int x = 0; x < head; x++) one(x);
      for (int x = head + 4 * groups; x < a.cols; x++) one(x);
    }
  }
}

// ---- k_frame_finish -----------------------------------------------------------------------------
// One keypoint per lane: the five double-precision iterations are a short serial chain.
struct FinishArgs {
  orbfe_camera cam;
  FrameUndist und;
  const orbfe_keypoint* kps;
  const int32_t* counts;
  const uint8_t* maps;  // NULL: monocular
  long long map_stride, map_pitch;
  int cap, depth_type, rows, cols;
  float factor;
  orbfe_keypoint* keys_un;
  float* u_right;
  float* depth;
};

__global__ __launch_bounds__(256) void k_frame_finish(FinishArgs a) {
  const int img = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= min(a.counts[img], a.cap)) return;
  const long long o = (long long)img * a.cap + k;
  const orbfe_keypoint kp = a.kps[o];
  const orbfe_keypoint un = frame_undistort_key(a.cam, a.und, kp);
  float ur, dep;
  frame_stereo_from_depth(a.maps ? a.maps + (long long)img * a.map_stride : nullptr, (size_t)a.map_pitch,
                          a.depth_type, a.factor, a.rows, a.cols, kp.x, kp.y, un.x, a.cam.bf, &ur, &dep);
  a.keys_un[o] = un;
  a.u_right[o] = ur;
  a.depth[o] = dep;
}

bool depth_layout_ok(const void* map, size_t pitch, int type, int rows, int cols) {
  if (!map) return true;
  if (type != ORBFE_DEPTH_U16 && type != ORBFE_DEPTH_F32) return false;
  const size_t elem = type == ORBFE_DEPTH_U16 ? 2 : 4;
  return rows > 0 && cols > 0 && pitch >= (size_t)cols * elem && pitch % elem == 0 && (uintptr_t)map % elem == 0;
}

int launch_gray(int n, const uint8_t* d_src, size_t src_stride, size_t src_pitch, int channels, int rgb, int mode,
                int rows, int cols, uint8_t* d_dst, size_t dst_stride, size_t dst_pitch, hipStream_t s) {
  GrayArgs a;
  a.src = d_src;
  a.dst = d_dst;
  a.src_stride = (long long)src_stride;
  a.dst_stride = (long long)dst_stride;
  a.src_pitch = (long long)src_pitch;
  a.dst_pitch = (long long)dst_pitch;
  a.rows = rows;
  a.cols = cols;
  a.rgb = rgb ? 1 : 0;
  a.mode = mode;
  const dim3 grid((cols / 4 + 1 + 63) / 64, (rows + GRAY_ROWS - 1) / GRAY_ROWS, n), block(64, GRAY_ROWS);
  if (channels == 3)
    ORBFE_LAUNCH("k_gray", k_gray<3>, grid, block, 0, s, a);
  else
    ORBFE_LAUNCH("k_gray", k_gray<4>, grid, block, 0, s, a);
  ORBFE_HIP_CHECK(hipGetLastError());
  return ORBFE_OK;
}

int launch_finish(int n, const orbfe_camera& cam, const orbfe_keypoint* d_kps, const int32_t* d_counts, int cap,
                  const void* d_maps, size_t map_stride, size_t map_pitch, int depth_type, float factor, int rows,
                  int cols, orbfe_keypoint* d_un, float* d_ur, float* d_dep, hipStream_t s) {
  FinishArgs a;
  std::memset(&a, 0, sizeof(a));
  a.cam = cam;
  a.und = frame_undist(cam);
  a.kps = d_kps;
  a.counts = d_counts;
  a.maps = static_cast<const uint8_t*>(d_maps);
  a.map_stride = (long long)map_stride;
  a.map_pitch = (long long)map_pitch;
  a.cap = cap;
  a.depth_type = depth_type;
  a.rows = rows;
  a.cols = cols;
  a.factor = factor;
  a.keys_un = d_un;
  a.u_right = d_ur;
  a.depth = d_dep;
  ORBFE_LAUNCH("k_frame_finish", k_frame_finish, dim3((cap + 255) / 256, n), dim3(256), 0, s, a);
  ORBFE_HIP_CHECK(hipGetLastError());
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_gray_batch_device(orbfe_extractor* h, int n_images, const uint8_t* d_src,
                                       size_t src_image_stride, size_t src_pitch, int channels, int rgb,
                                       int gray_mode, int rows, int cols, uint8_t* d_dst,
                                       size_t dst_image_stride, size_t dst_pitch, void* stream) {
  if (!h || n_images < 0 || n_images > 65535 || !d_src || !d_dst || rows <= 0 || rows > 65535 * GRAY_ROWS ||
      cols <= 0 || (channels != 3 && channels != 4) || src_pitch < (size_t)cols * channels ||
      dst_pitch < (size_t)cols || (gray_mode != ORBFE_GRAY_SHIFT15 && gray_mode != ORBFE_GRAY_SHIFT14))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gray_batch_device: bad argument");
  if (n_images == 0) return ORBFE_OK;
  hipStream_t hs;
  hipSetDevice(orbfe_internal_device(h, &hs));
  return launch_gray(n_images, d_src, src_image_stride, src_pitch, channels, rgb, gray_mode, rows, cols, d_dst,
                     dst_image_stride, dst_pitch, stream ? (hipStream_t)stream : hs);
}

extern "C" int orbfe_frame_finish_batch_device(orbfe_extractor* h, int n_images, const orbfe_camera* cam,
                                               const orbfe_keypoint* d_kps, const int32_t* d_counts, int cap,
                                               const void* d_depth_maps, size_t depth_image_stride,
                                               size_t depth_pitch, int depth_type, float depth_factor, int rows,
                                               int cols, orbfe_keypoint* d_keys_un, float* d_u_right,
                                               float* d_depth, void* stream) {
  if (!h || n_images < 0 || n_images > 65535 || !frame_camera_ok(cam) || !d_kps || !d_counts || cap <= 0 ||
      !d_keys_un || !d_u_right || !d_depth || !depth_layout_ok(d_depth_maps, depth_pitch, depth_type, rows, cols) ||
      (d_depth_maps && n_images > 1 && depth_image_stride % (depth_type == ORBFE_DEPTH_U16 ? 2 : 4) != 0))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_frame_finish_batch_device: bad argument");
  if (n_images == 0) return ORBFE_OK;
  hipStream_t hs;
  hipSetDevice(orbfe_internal_device(h, &hs));
  return launch_finish(n_images, *cam, d_kps, d_counts, cap, d_depth_maps, depth_image_stride, depth_pitch,
                       depth_type, depth_factor, rows, cols, d_keys_un, d_u_right, d_depth,
                       stream ? (hipStream_t)stream : hs);
}

// ---- the blocking one-call Frames ---------------------------------------------------------------
struct OrbfeFrameScratch {
  uint8_t* d_src = nullptr;   // the caller's image as it came (colour or gray)
  size_t src_n = 0;
  uint8_t* d_gray = nullptr;  // k_gray's plane
  size_t gray_n = 0;
  uint8_t* d_map = nullptr;   // the raw depth map
  size_t map_n = 0;
  orbfe_keypoint* d_kps = nullptr;  // keys, then undistorted keys (slots each)
  uint8_t* d_desc = nullptr;
  float* d_out = nullptr;           // u_right, then depth
  int32_t* d_count = nullptr;
  size_t slots = 0;
};

void orbfe_internal_frame_free(OrbfeFrameScratch* s) {
  if (!s) return;
  hipFree(s->d_src);
  hipFree(s->d_gray);
  hipFree(s->d_map);
  hipFree(s->d_kps);
  hipFree(s->d_desc);
  hipFree(s->d_out);
  hipFree(s->d_count);
  delete s;
}

static int grow(uint8_t** p, size_t* have, size_t need) {
  if (need <= *have) return ORBFE_OK;
  hipFree(*p);
  *p = nullptr;
  *have = 0;
  ORBFE_HIP_CHECK(hipMalloc(p, need));
  *have = need;
  return ORBFE_OK;
}

static int frame_impl(const char* who, orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step,
                      int channels, int rgb, int gray_mode, const void* depth_map, size_t depth_step, int depth_type,
                      float depth_factor, const orbfe_camera* cam, orbfe_keypoint* kps, uint8_t* desc, int* n, int cap,
                      orbfe_keypoint* keys_un, float* u_right, float* depth) {
  if (!h || !n || !img || !frame_camera_ok(cam) || rows < 0 || cols < 0 ||
      (channels != 1 && channels != 3 && channels != 4) || step < (size_t)cols * channels ||
      (gray_mode != ORBFE_GRAY_SHIFT15 && gray_mode != ORBFE_GRAY_SHIFT14))
    return orbfe_set_error(ORBFE_ERR_ARG, who);
  *n = 0;
  if (rows == 0 || cols == 0) return ORBFE_OK;  // mvKeys.empty(): the constructor returns (Frame.cc:183-184)
  if (!depth_layout_ok(depth_map, depth_step, depth_type, rows, cols)) return orbfe_set_error(ORBFE_ERR_ARG, who);
  const int K = orbfe_max_keypoints(h, rows, cols);
  if (K < 0) return K;
  if (cap < K) return orbfe_set_error(ORBFE_ERR_CAPACITY, "cap < orbfe_max_keypoints");
  if (!kps || !desc || !keys_un || !u_right || !depth) return orbfe_set_error(ORBFE_ERR_ARG, who);
  hipStream_t s;
  hipSetDevice(orbfe_internal_device(h, &s));
  OrbfeFrameScratch** slot = orbfe_internal_frame_slot(h);
  if (!*slot) *slot = new OrbfeFrameScratch();
  OrbfeFrameScratch* S = *slot;
  const size_t src_bytes = (size_t)(rows - 1) * step + (size_t)cols * channels;
  int st = grow(&S->d_src, &S->src_n, src_bytes);
  if (st != ORBFE_OK) return st;
  const size_t gpitch = ((size_t)cols + 3) & ~(size_t)3;
  if (channels != 1 && (st = grow(&S->d_gray, &S->gray_n, gpitch * rows)) != ORBFE_OK) return st;
  const size_t map_bytes =
      depth_map ? (size_t)(rows - 1) * depth_step + (size_t)cols * (depth_type == ORBFE_DEPTH_U16 ? 2 : 4) : 0;
  if (depth_map && (st = grow(&S->d_map, &S->map_n, map_bytes)) != ORBFE_OK) return st;
  if ((size_t)K > S->slots) {
    hipFree(S->d_kps);
    hipFree(S->d_desc);
    hipFree(S->d_out);
    S->d_kps = nullptr;
    S->d_desc = nullptr;
    S->d_out = nullptr;
    S->slots = 0;
    ORBFE_HIP_CHECK(hipMalloc(&S->d_kps, 2 * (size_t)K * sizeof(orbfe_keypoint)));
    ORBFE_HIP_CHECK(hipMalloc(&S->d_desc, (size_t)K * ORBFE_DESC_BYTES));
    ORBFE_HIP_CHECK(hipMalloc(&S->d_out, 2 * (size_t)K * sizeof(float)));
    S->slots = (size_t)K;
  }
  if (!S->d_count) ORBFE_HIP_CHECK(hipMalloc(&S->d_count, sizeof(int32_t)));
  // image up, gray, ExtractORB(0, imGray), UndistortKeyPoints + ComputeStereoFromRGBD: one stream, one wait
  ORBFE_HIP_CHECK(hipMemcpyAsync(S->d_src, img, src_bytes, hipMemcpyHostToDevice, s));
  if (depth_map) ORBFE_HIP_CHECK(hipMemcpyAsync(S->d_map, depth_map, map_bytes, hipMemcpyHostToDevice, s));
  const uint8_t* plane = S->d_src;
  size_t pitch = step;
  if (channels != 1) {
    st = launch_gray(1, S->d_src, 0, step, channels, rgb, gray_mode, rows, cols, S->d_gray, 0, gpitch, s);
    if (st != ORBFE_OK) return st;
    plane = S->d_gray;
    pitch = gpitch;
  }
  st = orbfe_extract_batch_device(h, 1, plane, pitch * rows, rows, cols, pitch, S->d_kps, S->d_desc, K, S->d_count, s);
  if (st != ORBFE_OK) return st;
  orbfe_keypoint* d_un = S->d_kps + K;
  st = launch_finish(1, *cam, S->d_kps, S->d_count, K, depth_map ? S->d_map : nullptr, 0, depth_step, depth_type,
                     depth_factor, rows, cols, d_un, S->d_out, S->d_out + K, s);
  if (st != ORBFE_OK) return st;
  int32_t count = 0;
  ORBFE_HIP_CHECK(hipMemcpyAsync(&count, S->d_count, sizeof(count), hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipStreamSynchronize(s));
  count = std::min(count, K);
  *n = count;
  if (count == 0) return ORBFE_OK;
  ORBFE_HIP_CHECK(hipMemcpyAsync(kps, S->d_kps, sizeof(orbfe_keypoint) * count, hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipMemcpyAsync(desc, S->d_desc, (size_t)ORBFE_DESC_BYTES * count, hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipMemcpyAsync(keys_un, d_un, sizeof(orbfe_keypoint) * count, hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipMemcpyAsync(u_right, S->d_out, sizeof(float) * count, hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipMemcpyAsync(depth, S->d_out + K, sizeof(float) * count, hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipStreamSynchronize(s));
  return ORBFE_OK;
}

extern "C" int orbfe_mono_frame(orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step,
                                int channels, int rgb, int gray_mode, const orbfe_camera* cam, orbfe_keypoint* kps,
                                uint8_t* desc, int* n, int cap, orbfe_keypoint* keys_un, float* u_right,
                                float* depth) {
  return frame_impl("orbfe_mono_frame: bad argument", h, img, rows, cols, step, channels, rgb, gray_mode, nullptr, 0,
                    ORBFE_DEPTH_F32, 1.0f, cam, kps, desc, n, cap, keys_un, u_right, depth);
}

extern "C" int orbfe_rgbd_frame(orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step,
                                int channels, int rgb, int gray_mode, const void* depth_map, size_t depth_step,
                                int depth_type, float depth_factor, const orbfe_camera* cam, orbfe_keypoint* kps,
                                uint8_t* desc, int* n, int cap, orbfe_keypoint* keys_un, float* u_right,
                                float* depth) {
  if (!depth_map) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rgbd_frame: bad argument");
  return frame_impl("orbfe_rgbd_frame: bad argument", h, img, rows, cols, step, channels, rgb, gray_mode, depth_map,
                    depth_step, depth_type, depth_factor, cam, kps, desc, n, cap, keys_un, u_right, depth);
}
