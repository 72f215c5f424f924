// orbfe_rectify.hip -- stereo rectification of raw camera pairs for gfx950 (include/orbfe_rectify.h):
//   k_rectify_plan  cv::remap's conversion of a camera's float maps to fixed-point entries, once per calibration.
//   k_rectify       cv::remap(INTER_LINEAR, BORDER_CONSTANT 0), the crop to a row range and cvtColor(*2GRAY) of a
//                   batch of raw pairs in one launch (Examples/Stereo/arducam_images.cpp:123-133,
//                   Tracking.cc:183-208), into the planes the extractor and ComputeStereoMatches take.
// Both apply the rules of orbfe_rectify_core.h, which the host entry points (orbfe_rectify_host.cpp) share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/orbfe.h"
#include "../../include/orbfe_rectify.h"
#include "../../include/orbfe_stereo.h"
#include "orbfe_device.h"
#include "orbfe_internal.h"
#include "orbfe_ktimer.h"
#include "orbfe_rectify_core.h"
#include "orbfe_stage.h"

struct orbfe_rectify_plan {
  int device = 0;
  RectifyEntry* d_ent = nullptr;  // the left camera's dst_rows * dst_cols entries, then the right camera's
  int dst_rows = 0, dst_cols = 0, src_rows = 0, src_cols = 0;
};

namespace {

// ---- k_rectify_plan -----------------------------------------------------------------------------
// One entry per lane: two coalesced float loads, one 8-byte store.
__global__ __launch_bounds__(256) void k_rectify_plan(const float* __restrict__ m1, const float* __restrict__ m2,
                                                      long long n, int src_rows, int src_cols,
                                                      RectifyEntry* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const RectifyEntry e = rectify_entry(m1[i], m2[i], src_rows, src_cols);
  uint2 w;
  w.x = (uint32_t)(uint16_t)e.ix | ((uint32_t)(uint16_t)e.iy << 16);
  w.y = (uint32_t)e.alpha | ((uint32_t)e.outside << 16);
  *reinterpret_cast<uint2*>(out + i) = w;
}

// ---- k_rectify ----------------------------------------------------------------------------------
// k_gray's store shape: a lane owns one aligned dword of a destination row (four gray pixels, or four bytes of a
// colour row) and the bytes in front of a row's first aligned dword and behind its last go bytewise through one
// lane per row, so nothing outside a row's bytes is written. A pixel's plan entry is one 8-byte load, the same
// for every image of the batch (the table of one camera at 640 x 480 is 2.4 MB and stays in L2). Neighbouring
// destination pixels read neighbouring source pixels, so a wave's taps fall into a few 128-byte lines of two or
// three source rows and come through L1 / L2 as plain byte loads; every tap is bounds-checked (rule 4), so no
// load leaves the source image.
constexpr int RECT_ROWS = 4;  // rows per workgroup, one wave each

struct RectifyArgs {
  const uint8_t* src[2];    // the first pair's left and right image
  const RectifyEntry* ent;  // the plan
  uint8_t* dst;
  long long pair_stride, src_pitch, dst_stride, dst_pitch, ent_side;
  int n_pairs, src_rows, src_cols, dst_cols, row0, rows, rgb, mode;
};

__device__ inline RectifyEntry load_entry(const RectifyEntry* p) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);  // entries are 8 bytes apart from an aligned base
  RectifyEntry e;
  e.ix = (int16_t)(w.x & 0xffffu);
  e.iy = (int16_t)(w.x >> 16);
  e.alpha = (uint16_t)(w.y & 0xffffu);
  e.outside = (uint16_t)(w.y >> 16);
  return e;
}

template <int C, bool GRAY>
__global__ __launch_bounds__(64 * RECT_ROWS) void k_rectify(RectifyArgs a) {
  const int row = blockIdx.y * RECT_ROWS + threadIdx.y;
  if (row >= a.rows) return;
  const int side = (int)blockIdx.z >= a.n_pairs ? 1 : 0;  // the lefts, then the rights
  const int pair = (int)blockIdx.z - side * a.n_pairs;
  const uint8_t* __restrict__ src = a.src[side] + (long long)pair * a.pair_stride;
  const RectifyEntry* __restrict__ ent =
      a.ent + (long long)side * a.ent_side + (long long)(a.row0 + row) * a.dst_cols;
  uint8_t* __restrict__ drow = a.dst + (long long)blockIdx.z * a.dst_stride + (long long)row * a.dst_pitch;
  const int width = a.dst_cols * (GRAY ? 1 : C);
  auto value = [&](int xb) {
    return rectify_byte<C, GRAY>(src, (size_t)a.src_pitch, a.src_rows, a.src_cols,
                                 load_entry(ent + rectify_pixel_of<C, GRAY>(xb)), xb, a.rgb, a.mode);
  };
  const int head = min(width, (int)((4u - (unsigned)((uintptr_t)drow & 3u)) & 3u));
  const int groups = (width - head) >> 2;
  for (int u = blockIdx.x * 64 + threadIdx.x; u <= groups; u += gridDim.x * 64) {
    if (u < groups) {
      const int x = head + 4 * u;
      uint32_t out = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) out |= (uint32_t)value(x + j) << (8 * j);
      *reinterpret_cast<uint32_t*>(drow + x) = out;
    } else {
      for (int x = 0; x < head; x++) drow[x] = value(x);
      for (int x = head + 4 * groups; x < width; x++) drow[x] = value(x);
    }
  }
}

int launch_rectify(const orbfe_rectify_plan* P, int n_pairs, const uint8_t* d_left, const uint8_t* d_right,
                   size_t pair_stride, size_t src_pitch, int channels, int rgb, int mode, int gray_out, int row0,
                   int row1, uint8_t* d_dst, size_t dst_stride, size_t dst_pitch, hipStream_t s) {
  RectifyArgs a;
  a.src[0] = d_left;
  a.src[1] = d_right;
  a.ent = P->d_ent;
  a.dst = d_dst;
  a.pair_stride = (long long)pair_stride;
  a.src_pitch = (long long)src_pitch;
  a.dst_stride = (long long)dst_stride;
  a.dst_pitch = (long long)dst_pitch;
  a.ent_side = (long long)P->dst_rows * P->dst_cols;
  a.n_pairs = n_pairs;
  a.src_rows = P->src_rows;
  a.src_cols = P->src_cols;
  a.dst_cols = P->dst_cols;
  a.row0 = row0;
  a.rows = row1 - row0;
  a.rgb = rgb ? 1 : 0;
  a.mode = mode;
  const bool g = rectify_gray_fused(channels, gray_out);
  const long long width = (long long)P->dst_cols * rectify_out_channels(channels, gray_out);
  const dim3 grid((unsigned)std::min<long long>((width / 4 + 1 + 63) / 64, 65535),
                  (a.rows + RECT_ROWS - 1) / RECT_ROWS, 2 * n_pairs),
      block(64, RECT_ROWS);
  if (channels == 1)
    ORBFE_LAUNCH("k_rectify", (k_rectify<1, false>), grid, block, 0, s, a);
  else if (channels == 3 && g)
    ORBFE_LAUNCH("k_rectify", (k_rectify<3, true>), grid, block, 0, s, a);
  else if (channels == 3)
    ORBFE_LAUNCH("k_rectify", (k_rectify<3, false>), grid, block, 0, s, a);
  else if (g)
    ORBFE_LAUNCH("k_rectify", (k_rectify<4, true>), grid, block, 0, s, a);
  else
    ORBFE_LAUNCH("k_rectify", (k_rectify<4, false>), grid, block, 0, s, a);
  ORBFE_HIP_CHECK(hipGetLastError());
  return ORBFE_OK;
}

// what a batch call and the one-call Frame check alike
bool remap_args_ok(const orbfe_rectify_plan* P, size_t src_pitch, int channels, int gray_mode, int gray_out, int row0,
                   int row1, size_t dst_pitch) {
  return P && rectify_format_ok(channels, gray_mode) && src_pitch < ((size_t)1 << 40) &&
         src_pitch >= (size_t)P->src_cols * channels && row0 >= 0 && row1 >= row0 && row1 <= P->dst_rows &&
         row1 - row0 <= 65535 * RECT_ROWS &&
         (long long)P->dst_cols * rectify_out_channels(channels, gray_out) <= 0x7fffffffLL &&
         dst_pitch >= (size_t)P->dst_cols * rectify_out_channels(channels, gray_out);
}

}  // namespace

extern "C" int orbfe_rectify_plan_create(orbfe_extractor* h, const float* map1_l, const float* map2_l,
                                         const float* map1_r, const float* map2_r, int dst_rows, int dst_cols,
                                         int src_rows, int src_cols, orbfe_rectify_plan** plan) {
  if (!h || !map1_l || !map2_l || !map1_r || !map2_r || !plan ||
      !rectify_sizes_ok(src_rows, src_cols, dst_rows, dst_cols) || (long long)dst_rows * dst_cols > (1LL << 30))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_plan_create: bad argument");
  *plan = nullptr;
  hipStream_t s;
  const int device = orbfe_internal_device(h, &s);
  hipSetDevice(device);
  const size_t n = (size_t)dst_rows * dst_cols;
  orbfe_rectify_plan* P = new orbfe_rectify_plan();
  P->device = device;
  P->dst_rows = dst_rows;
  P->dst_cols = dst_cols;
  P->src_rows = src_rows;
  P->src_cols = src_cols;
  float* d_maps = nullptr;  // map1_l, map2_l, map1_r, map2_r
  auto build = [&]() -> int {
    ORBFE_HIP_CHECK(hipMalloc(&P->d_ent, 2 * n * sizeof(RectifyEntry)));
    ORBFE_HIP_CHECK(hipMalloc(&d_maps, 4 * n * sizeof(float)));
    const float* maps[4] = {map1_l, map2_l, map1_r, map2_r};
    for (int i = 0; i < 4; i++)
      ORBFE_HIP_CHECK(hipMemcpyAsync(d_maps + i * n, maps[i], n * sizeof(float), hipMemcpyHostToDevice, s));
    for (int side = 0; side < 2; side++)
      ORBFE_LAUNCH("k_rectify_plan", k_rectify_plan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                   d_maps + 2 * side * n, d_maps + (2 * side + 1) * n, (long long)n, src_rows, src_cols,
                   P->d_ent + side * n);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipStreamSynchronize(s));  // the maps may be pageable and short-lived
    return ORBFE_OK;
  };
  const int st = build();
  hipFree(d_maps);
  if (st != ORBFE_OK) {
    orbfe_rectify_plan_destroy(P);
    return st;
  }
  *plan = P;
  return ORBFE_OK;
}

extern "C" void orbfe_rectify_plan_destroy(orbfe_rectify_plan* plan) {
  if (!plan) return;
  hipSetDevice(plan->device);
  hipFree(plan->d_ent);
  delete plan;
}

extern "C" int orbfe_rectify_plan_read(orbfe_rectify_plan* plan, int right, orbfe_rectify_entry* entries) {
  if (!plan || !entries) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_plan_read: bad argument");
  hipSetDevice(plan->device);
  const size_t n = (size_t)plan->dst_rows * plan->dst_cols;
  ORBFE_HIP_CHECK(hipMemcpy(entries, plan->d_ent + (right ? n : 0), n * sizeof(RectifyEntry), hipMemcpyDeviceToHost));
  return ORBFE_OK;
}

extern "C" int orbfe_rectify_batch_device(orbfe_extractor* h, const orbfe_rectify_plan* plan, int n_pairs,
                                          const uint8_t* d_src_left, const uint8_t* d_src_right,
                                          size_t src_pair_stride, size_t src_pitch, int channels, int rgb,
                                          int gray_mode, int gray_out, int row0, int row1, uint8_t* d_dst,
                                          size_t dst_image_stride, size_t dst_pitch, void* stream) {
  if (!h || n_pairs < 0 || n_pairs > 32767 || !d_src_left || !d_src_right || !d_dst ||
      !remap_args_ok(plan, src_pitch, channels, gray_mode, gray_out, row0, row1, dst_pitch))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_batch_device: bad argument");
  if (n_pairs == 0 || row0 == row1) return ORBFE_OK;
  hipStream_t hs;
  const int device = orbfe_internal_device(h, &hs);
  if (device != plan->device)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_rectify_batch_device: the plan lives on another device");
  hipSetDevice(device);
  return launch_rectify(plan, n_pairs, d_src_left, d_src_right, src_pair_stride, src_pitch, channels, rgb, gray_mode,
                        gray_out, row0, row1, d_dst, dst_image_stride, dst_pitch, stream ? (hipStream_t)stream : hs);
}

// ---- the blocking one-call Frame ------------------------------------------------------------------
struct OrbfeRectifyScratch {
  uint8_t* d_src = nullptr;     // the raw pair as it came
  size_t src_n = 0;
  uint8_t* d_planes = nullptr;  // k_rectify's two planes
  size_t planes_n = 0;
  orbfe_keypoint* d_kps = nullptr;  // left, then right (slots each)
  uint8_t* d_desc = nullptr;
  float* d_out = nullptr;           // u_right, then depth
  int32_t* d_counts = nullptr;      // left, right
  size_t slots = 0;
};

void orbfe_internal_rectify_free(OrbfeRectifyScratch* s) {
  if (!s) return;
  hipFree(s->d_src);
  hipFree(s->d_planes);
  hipFree(s->d_kps);
  hipFree(s->d_desc);
  hipFree(s->d_out);
  hipFree(s->d_counts);
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

extern "C" int orbfe_rectified_stereo_frame(orbfe_extractor* h, const orbfe_rectify_plan* plan, const uint8_t* left,
                                            const uint8_t* right, int rows, int cols, size_t step, int channels,
                                            int rgb, int gray_mode, int row0, int row1, float mbf, float mb,
                                            orbfe_keypoint* kps_l, uint8_t* desc_l, int* n_l, orbfe_keypoint* kps_r,
                                            uint8_t* desc_r, int* n_r, int cap, float* u_right, float* depth) {
  const char* who = "orbfe_rectified_stereo_frame: bad argument";
  if (!h || !plan || !left || !right || !n_l || !n_r || rows < 0 || cols < 0) return orbfe_set_error(ORBFE_ERR_ARG, who);
  *n_l = *n_r = 0;
  if (rows == 0 || cols == 0 || row0 == row1) return ORBFE_OK;  // N = 0: the constructor returns early (Frame.cc:120-121)
  const size_t gpitch = ((size_t)plan->dst_cols + 3) & ~(size_t)3;
  if (rows != plan->src_rows || cols != plan->src_cols ||
      !remap_args_ok(plan, step, channels, gray_mode, 1, row0, row1, gpitch))
    return orbfe_set_error(ORBFE_ERR_ARG, who);
  const int out_rows = row1 - row0, out_cols = plan->dst_cols;
  const int K = orbfe_max_keypoints(h, out_rows, out_cols);
  if (K < 0) return K;
  if (cap < K) return orbfe_set_error(ORBFE_ERR_CAPACITY, "cap < orbfe_max_keypoints");
  if (!kps_l || !desc_l || !kps_r || !desc_r || !u_right || !depth) return orbfe_set_error(ORBFE_ERR_ARG, who);
  hipStream_t s;
  const int device = orbfe_internal_device(h, &s);
  if (device != plan->device) return orbfe_set_error(ORBFE_ERR_ARG, who);
  hipSetDevice(device);
  OrbfeRectifyScratch** slot = orbfe_internal_rectify_slot(h);
  if (!*slot) *slot = new OrbfeRectifyScratch();
  OrbfeRectifyScratch* S = *slot;
  // a side-by-side image (right = left + one image row's bytes, inside the same rows) goes up once
  const size_t row_bytes = (size_t)cols * channels;
  const bool side_by_side = right == left + row_bytes && step >= 2 * row_bytes;
  const size_t one = (size_t)(rows - 1) * step + row_bytes;
  const size_t right_off = side_by_side ? row_bytes : orbfe_al256(one);
  int st = grow(&S->d_src, &S->src_n, right_off + one);
  if (st != ORBFE_OK) return st;
  if ((st = grow(&S->d_planes, &S->planes_n, 2 * gpitch * out_rows)) != ORBFE_OK) return st;
  if ((size_t)K > S->slots) {
    hipFree(S->d_kps);
    hipFree(S->d_desc);
    hipFree(S->d_out);
    S->d_kps = nullptr;
    S->d_desc = nullptr;
    S->d_out = nullptr;
    S->slots = 0;
    ORBFE_HIP_CHECK(hipMalloc(&S->d_kps, 2 * (size_t)K * sizeof(orbfe_keypoint)));
    ORBFE_HIP_CHECK(hipMalloc(&S->d_desc, 2 * (size_t)K * ORBFE_DESC_BYTES));
    ORBFE_HIP_CHECK(hipMalloc(&S->d_out, 2 * (size_t)K * sizeof(float)));
    S->slots = (size_t)K;
  }
  if (!S->d_counts) ORBFE_HIP_CHECK(hipMalloc(&S->d_counts, 2 * sizeof(int32_t)));
  // pair up, remap + crop + gray, ExtractORB(0 / 1) as one batch, ComputeStereoMatches: one stream, one wait
  if (side_by_side) {
    ORBFE_HIP_CHECK(hipMemcpyAsync(S->d_src, left, right_off + one, hipMemcpyHostToDevice, s));
  } else {
    ORBFE_HIP_CHECK(hipMemcpyAsync(S->d_src, left, one, hipMemcpyHostToDevice, s));
    ORBFE_HIP_CHECK(hipMemcpyAsync(S->d_src + right_off, right, one, hipMemcpyHostToDevice, s));
  }
  st = launch_rectify(plan, 1, S->d_src, S->d_src + right_off, 0, step, channels, rgb, gray_mode, 1, row0, row1,
                      S->d_planes, gpitch * out_rows, gpitch, s);
  if (st != ORBFE_OK) return st;
  st = orbfe_extract_batch_device(h, 2, S->d_planes, gpitch * out_rows, out_rows, out_cols, gpitch, S->d_kps,
                                  S->d_desc, K, S->d_counts, s);
  if (st != ORBFE_OK) return st;
  st = orbfe_compute_stereo_matches_batch_device(h, 1, 0, 1, S->d_kps, S->d_desc, S->d_counts, K, mbf, mb, S->d_out,
                                                 S->d_out + K, s);
  if (st != ORBFE_OK) return st;
  int32_t counts[2] = {0, 0};
  ORBFE_HIP_CHECK(hipMemcpyAsync(counts, S->d_counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  ORBFE_HIP_CHECK(hipStreamSynchronize(s));
  const int nl = std::min(counts[0], K), nr = std::min(counts[1], K);
  *n_l = nl;
  *n_r = nr;
  if (nl > 0) {
    ORBFE_HIP_CHECK(hipMemcpyAsync(kps_l, S->d_kps, sizeof(orbfe_keypoint) * nl, hipMemcpyDeviceToHost, s));
    ORBFE_HIP_CHECK(hipMemcpyAsync(desc_l, S->d_desc, (size_t)ORBFE_DESC_BYTES * nl, hipMemcpyDeviceToHost, s));
    ORBFE_HIP_CHECK(hipMemcpyAsync(u_right, S->d_out, sizeof(float) * nl, hipMemcpyDeviceToHost, s));
    ORBFE_HIP_CHECK(hipMemcpyAsync(depth, S->d_out + K, sizeof(float) * nl, hipMemcpyDeviceToHost, s));
  }
  if (nr > 0) {
    ORBFE_HIP_CHECK(hipMemcpyAsync(kps_r, S->d_kps + K, sizeof(orbfe_keypoint) * nr, hipMemcpyDeviceToHost, s));
    ORBFE_HIP_CHECK(hipMemcpyAsync(desc_r, S->d_desc + (size_t)K * ORBFE_DESC_BYTES, (size_t)ORBFE_DESC_BYTES * nr,
                                   hipMemcpyDeviceToHost, s));
  }
  ORBFE_HIP_CHECK(hipStreamSynchronize(s));
  return ORBFE_OK;
}
