/*
 * orbfe_frame.h -- the monocular and RGB-D Frame constructors' per-frame steps on the GPU
 * (liborbfe.so, gfx950).
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   cvtColor / convertTo of Tracking::GrabImageRGBD / GrabImageMonocular  src/Tracking.cc:226-283
 *   Frame::UndistortKeyPoints()                                           src/Frame.cc:456-486
 *   Frame::ComputeImageBounds()                                           src/Frame.cc:488-520
 *   Frame::ComputeStereoFromRGBD()                                        src/Frame.cc:702-723
 *   the RGB-D and monocular Frame constructors' hot path                  src/Frame.cc:154-214, 216-277
 *
 * Every rule (the two gray tables, convertTo's float product, cv::undistortPoints with P = K in
 * double, the k1 == 0 early-out) is restated in orb_slam2_2021_amd/csrc/orbfe_frame_core.h and
 * used by both the kernels and the _host functions; DESIGN.md "Monocular and RGB-D Frames" records
 * them. Results are bit-identical between the device and the host entry points.
 */
#ifndef ORBFE_FRAME_H
#define ORBFE_FRAME_H
#include <stddef.h>
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvtColor's 8-bit fixed-point tables: OpenCV 4.x (15 fractional bits, the default) or the
 * 2.4 / 3.x tables (14 bits). */
#define ORBFE_GRAY_SHIFT15 0
#define ORBFE_GRAY_SHIFT14 1

/* Raw type of a depth map (imDepth before convertTo). */
#define ORBFE_DEPTH_U16 0
#define ORBFE_DEPTH_F32 1

/* mK, mDistCoef (k1, k2, p1, p2[, k3]; n_dist = 4 or 5) and mbf. */
typedef struct orbfe_camera {
  float fx, fy, cx, cy;
  float dist[5];
  int32_t n_dist;
  float bf;
} orbfe_camera;

/* Frame::ComputeImageBounds: out = {mnMinX, mnMaxX, mnMinY, mnMaxY}. Host only. */
int orbfe_image_bounds(const orbfe_camera* cam, int rows, int cols, float out[4]);

/* cvtColor(RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY) of n_images interleaved 8-bit images on the
 * device of `h`: image i at d_src + i*src_image_stride, rows src_pitch bytes apart, `channels`
 * (3 or 4; alpha ignored) bytes per pixel, channel 0 = R when rgb != 0 (mbRGB) and B otherwise.
 * Writes the 8-bit planes orbfe_extract_batch_device takes: image i at d_dst + i*dst_image_stride,
 * rows dst_pitch bytes apart; bytes of a row beyond cols are not touched. Any pitch and alignment.
 * Async on `stream` (NULL: the handle's stream). */
int orbfe_gray_batch_device(orbfe_extractor* h, int n_images, const uint8_t* d_src,
                            size_t src_image_stride, size_t src_pitch, int channels, int rgb,
                            int gray_mode, int rows, int cols, uint8_t* d_dst,
                            size_t dst_image_stride, size_t dst_pitch, void* stream);

/* UndistortKeyPoints and ComputeStereoFromRGBD of a whole batch in one launch: the keypoints of
 * image i are d_kps + i*cap, d_counts[i] of them (the outputs of orbfe_extract_batch_device).
 * Writes d_keys_un (mvKeysUn: all seven fields, x and y undistorted), d_u_right (mvuRight) and
 * d_depth (mvDepth) at i*cap + k for k < d_counts[i]; entries at or beyond the count are not
 * touched. d_depth_maps: image i's raw depth map (depth_type ORBFE_DEPTH_*) at
 * d_depth_maps + i*depth_image_stride bytes, rows depth_pitch bytes apart, rows x cols values;
 * depth_factor is mDepthMapFactor already inverted (Tracking.cc:148-152). NULL d_depth_maps is the
 * monocular Frame: u_right and depth are -1. A keypoint whose truncated position lies outside
 * rows x cols (never an extractor's) gets -1 where the reference would read out of bounds.
 * Async on `stream` (NULL: the handle's stream). */
int orbfe_frame_finish_batch_device(orbfe_extractor* h, int n_images, const orbfe_camera* cam,
                                    const orbfe_keypoint* d_kps, const int32_t* d_counts, int cap,
                                    const void* d_depth_maps, size_t depth_image_stride,
                                    size_t depth_pitch, int depth_type, float depth_factor,
                                    int rows, int cols, orbfe_keypoint* d_keys_un,
                                    float* d_u_right, float* d_depth, void* stream);

/* The same rules on host arrays (no device, no handle), for callers whose keypoints are already
 * in host memory (the reference's constructor at Frame.cc:186-188): keys_un[n] from keys[n]
 * (keys_un == keys is allowed), then u_right[n] / depth[n] from the raw depth map sampled at the
 * distorted keys. depth_map NULL: both -1. */
int orbfe_undistort_keypoints_host(const orbfe_camera* cam, const orbfe_keypoint* keys, int n,
                                   orbfe_keypoint* keys_un);
int orbfe_stereo_from_depth_host(const orbfe_camera* cam, const orbfe_keypoint* keys,
                                 const orbfe_keypoint* keys_un, int n, const void* depth_map,
                                 size_t depth_pitch, int depth_type, float depth_factor, int rows,
                                 int cols, float* u_right, float* depth);

/* The monocular Frame (Frame.cc:216-277; Tracking.cc:257-283): gray conversion when channels is
 * 3 or 4 (channels == 1: the image is CV_8UC1 already), ExtractORB, UndistortKeyPoints, no stereo.
 * img is host memory, rows `step` bytes apart. kps / desc / keys_un / u_right / depth hold cap
 * entries (cap >= orbfe_max_keypoints(h, rows, cols)). Blocking. An empty image gives *n = 0. */
int orbfe_mono_frame(orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step,
                     int channels, int rgb, int gray_mode, const orbfe_camera* cam,
                     orbfe_keypoint* kps, uint8_t* desc, int* n, int cap, orbfe_keypoint* keys_un,
                     float* u_right, float* depth);

/* The RGB-D Frame (Frame.cc:154-214; Tracking.cc:226-255): the same plus ComputeStereoFromRGBD on
 * the raw depth map (host memory, rows depth_step bytes apart), whose values are converted where
 * they are sampled. */
int orbfe_rgbd_frame(orbfe_extractor* h, const uint8_t* img, int rows, int cols, size_t step,
                     int channels, int rgb, int gray_mode, const void* depth_map, size_t depth_step,
                     int depth_type, float depth_factor, const orbfe_camera* cam,
                     orbfe_keypoint* kps, uint8_t* desc, int* n, int cap, orbfe_keypoint* keys_un,
                     float* u_right, float* depth);

#ifdef __cplusplus
}
#endif
#endif
