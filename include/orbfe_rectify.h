/*
 * orbfe_rectify.h -- stereo rectification of raw camera pairs on the GPU (liborbfe.so, gfx950).
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   cv::initUndistortRectifyMap in rectification()          Examples/Stereo/arducam_images.cpp:229-275
 *   the per-frame split, cv::remap(INTER_LINEAR) and crop   Examples/Stereo/arducam_images.cpp:123-133
 *                                                           Examples/Stereo/arducam_video.cpp:75-104
 *   cvtColor of both halves in Tracking::GrabImageStereo    src/Tracking.cc:183-208
 *
 * Every rule (the maps in double with running sums along a row, the float product rounded half to even
 * into the 1/32-pixel grid, the integer bilinear blend, BORDER_CONSTANT 0, gray after the blend) is
 * restated in orb_slam2_2021_amd/csrc/orbfe_rectify_core.h and used by both the kernels and the _host
 * functions; DESIGN.md section 30 records them. Results are bit-identical between the device and the
 * host entry points. Radial k1 k2 k3 and tangential p1 p2 only; bilinear only; 8-bit images only.
 */
#ifndef ORBFE_RECTIFY_H
#define ORBFE_RECTIFY_H
#include <stddef.h>
#include <stdint.h>

#include "orbfe.h"
#include "orbfe_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A calibration's fixed-point maps on the device, for both cameras. */
typedef struct orbfe_rectify_plan orbfe_rectify_plan;

/* One destination pixel of a plan: top-left tap (ix, iy), fractions alpha = (sy & 31) * 32 + (sx & 31),
 * outside != 0 when the pixel is the border constant (then ix = iy = alpha = 0 if the map value had no
 * int conversion). */
typedef struct orbfe_rectify_entry {
  int16_t ix, iy;
  uint16_t alpha;
  uint16_t outside;
} orbfe_rectify_entry;

/* cv::initUndistortRectifyMap(K, D, R, P, Size(cols, rows), CV_32F, map1, map2), row-major doubles as
 * the settings file holds them: K[9], D[n_dist] (k1 k2 p1 p2[ k3]; n_dist = 4 or 5), R[9] or NULL for
 * the identity, P3[9] = the left 3 x 3 of P. map1 / map2: rows x cols floats, contiguous. Host only:
 * no device, no handle. ORBFE_ERR_ARG also when P3 * R is singular. */
int orbfe_rectify_maps_host(const double* K, const double* D, int n_dist, const double* R,
                            const double* P3, int rows, int cols, float* map1, float* map2);

/* cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0), the crop to destination rows
 * [row0, row1) and cvtColor(*2GRAY), on host arrays. src: src_rows x src_cols pixels of `channels`
 * (1, 3 or 4) interleaved bytes, rows src_pitch bytes apart. map1 / map2: dst_rows x dst_cols floats,
 * rows map_pitch bytes apart (a multiple of 4). dst: row1 - row0 rows, dst_pitch bytes apart, of
 * dst_cols pixels: one byte each when gray_out != 0 and channels is 3 or 4 (channel 0 = R when
 * rgb != 0, gray_mode ORBFE_GRAY_*), else `channels` bytes each. Bytes of a destination row beyond
 * its pixels are not touched. Source sizes above 32766 are refused. */
int orbfe_remap_host(const uint8_t* src, int src_rows, int src_cols, size_t src_pitch, int channels,
                     const float* map1, const float* map2, size_t map_pitch, int dst_rows,
                     int dst_cols, int row0, int row1, int rgb, int gray_mode, int gray_out,
                     uint8_t* dst, size_t dst_pitch);

/* The fixed-point entries remap derives from float maps (rows x cols, contiguous) for a source of
 * src_rows x src_cols: what a plan holds. Host only. */
int orbfe_rectify_entries_host(const float* map1, const float* map2, int rows, int cols, int src_rows,
                               int src_cols, orbfe_rectify_entry* entries);

/* Converts the float maps of the left and the right camera (host memory, dst_rows x dst_cols,
 * contiguous; from orbfe_rectify_maps_host or the caller's own OpenCV) to fixed point on the device of
 * `h`, once: 8 bytes per pixel and camera. The plan lives as long as the calibration and serves every
 * frame and batch of handles on that device; it holds device memory only and is destroyed by
 * orbfe_rectify_plan_destroy. Blocking. */
int orbfe_rectify_plan_create(orbfe_extractor* h, const float* map1_l, const float* map2_l,
                              const float* map1_r, const float* map2_r, int dst_rows, int dst_cols,
                              int src_rows, int src_cols, orbfe_rectify_plan** plan);
void orbfe_rectify_plan_destroy(orbfe_rectify_plan* plan);

/* The plan's entries of one camera (right != 0: the right one) copied to host memory,
 * dst_rows x dst_cols of them. Blocking. */
int orbfe_rectify_plan_read(orbfe_rectify_plan* plan, int right, orbfe_rectify_entry* entries);

/* Rectifies n_pairs raw pairs on the device: pair p's left image at d_src_left + p*src_pair_stride and
 * its right image at d_src_right + p*src_pair_stride, both src_rows x src_cols of the plan, rows
 * src_pitch bytes apart (a side-by-side image: d_src_right = d_src_left + src_cols*channels). Writes
 * 2*n_pairs images of row1 - row0 rows, the lefts and then the rights (image i at
 * d_dst + i*dst_image_stride, rows dst_pitch bytes apart): with gray_out != 0 the 8-bit planes
 * orbfe_extract_batch_device and orbfe_compute_stereo_matches_batch_device take (left0 = 0,
 * right0 = n_pairs). Arguments as orbfe_remap_host. Bytes of a destination row beyond its pixels are
 * not touched. Any pitch and alignment. Async on `stream` (NULL: the handle's stream). */
int orbfe_rectify_batch_device(orbfe_extractor* h, const orbfe_rectify_plan* plan, int n_pairs,
                               const uint8_t* d_src_left, const uint8_t* d_src_right,
                               size_t src_pair_stride, size_t src_pitch, int channels, int rgb,
                               int gray_mode, int gray_out, int row0, int row1, uint8_t* d_dst,
                               size_t dst_image_stride, size_t dst_pitch, void* stream);

/* The stereo Frame from a raw pair (arducam_images.cpp:119-153 + Tracking.cc:183-208 + Frame.cc:80-125):
 * left / right are host images of rows x cols pixels (the plan's source size), `step` bytes between rows,
 * `channels` 1, 3 or 4. One upload each, remap + crop to rows [row0, row1) + gray in one launch,
 * ExtractORB of both planes as a batch, ComputeStereoMatches, one wait. Outputs and mbf / mb as
 * orbfe_stereo_frame (cap >= orbfe_max_keypoints(h, row1 - row0, the plan's dst_cols)). Blocking.
 * An empty image (rows or cols 0, or row0 == row1) gives zero counts. */
int orbfe_rectified_stereo_frame(orbfe_extractor* h, const orbfe_rectify_plan* plan,
                                 const uint8_t* left, const uint8_t* right, int rows, int cols,
                                 size_t step, int channels, int rgb, int gray_mode, int row0, int row1,
                                 float mbf, float mb, orbfe_keypoint* kps_l, uint8_t* desc_l, int* n_l,
                                 orbfe_keypoint* kps_r, uint8_t* desc_r, int* n_r, int cap,
                                 float* u_right, float* depth);

#ifdef __cplusplus
}
#endif
#endif
