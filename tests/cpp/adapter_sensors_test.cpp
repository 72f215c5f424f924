// adapter/Frame_sensors_gpu.cc over the test-only declarations (cvstub_sensors/Frame.h before cvstub/): one
// Frame with the TUM fr1 camera, a lattice of keypoints and a float depth map goes through
// UndistortKeyPoints, ComputeStereoFromRGBD and ComputeImageBounds, and must hold exactly what the host entry
// points of include/orbfe_frame.h give for the same arrays. Host only: no GPU is touched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <opencv2/core.hpp>

#include "Frame.h"
#include "orbfe_frame.h"

int main() {
  using ORB_SLAM2::Frame;
  const int rows = 480, cols = 640;
  const float dist[5] = {0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f};
  int failures = 0;
  for (int n_dist = 4; n_dist <= 5; n_dist++) {
    Frame F;
    F.mK = cv::Mat::eye(3, 3, CV_32F);
    F.mK.at<float>(0, 0) = 517.306408f;
    F.mK.at<float>(1, 1) = 516.469215f;
    F.mK.at<float>(0, 2) = 318.643040f;
    F.mK.at<float>(1, 2) = 255.313989f;
    F.mDistCoef = cv::Mat(n_dist, 1, CV_32F);
    for (int i = 0; i < n_dist; i++) F.mDistCoef.at<float>(i) = dist[i];
    F.mbf = 40.0f;
    for (int iy = 0; iy < 7; iy++)
      for (int ix = 0; ix < 9; ix++) {
        const int i = (int)F.mvKeys.size();
        F.mvKeys.emplace_back(ix * 79.6f + 0.3f, iy * 79.7f + 0.6f, 31.0f + i, 2.0f * i, 5.0f + i, i % 8, i - 2);
      }
    F.N = (int)F.mvKeys.size();
    // a depth map whose rows are 5 floats longer than the image; zero, negative and NaN values included
    std::vector<float> buf((size_t)rows * (cols + 5), -7.0f);
    cv::Mat depth(rows, cols, CV_32F, buf.data(), (size_t)(cols + 5) * sizeof(float));
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) {
        const int k = (x / 79 + y / 79) % 4;
        depth.at<float>(y, x) = k == 0 ? 0.0f : k == 1 ? 0.5f + 0.01f * x + 0.02f * y : k == 2 ? -1.0f : NAN;
      }
    for (int x = 0; x < cols; x++) depth.at<float>(0, x) = 1.25f + 0.001f * x;

    F.UndistortKeyPoints();
    F.ComputeStereoFromRGBD(depth);
    F.ComputeImageBounds(depth);

    orbfe_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.fx = 517.306408f;
    cam.fy = 516.469215f;
    cam.cx = 318.643040f;
    cam.cy = 255.313989f;
    cam.n_dist = n_dist;
    for (int i = 0; i < n_dist; i++) cam.dist[i] = dist[i];
    cam.bf = 40.0f;
    std::vector<orbfe_keypoint> un(F.N);
    std::vector<float> ur(F.N), dep(F.N);
    float b[4];
    const orbfe_keypoint* keys = reinterpret_cast<const orbfe_keypoint*>(F.mvKeys.data());
    if (orbfe_undistort_keypoints_host(&cam, keys, F.N, un.data()) != ORBFE_OK ||
        orbfe_stereo_from_depth_host(&cam, keys, un.data(), F.N, buf.data(), (size_t)(cols + 5) * sizeof(float),
                                     ORBFE_DEPTH_F32, 1.0f, rows, cols, ur.data(), dep.data()) != ORBFE_OK ||
        orbfe_image_bounds(&cam, rows, cols, b) != ORBFE_OK) {
      std::printf("host entry point failed: %s\n", orbfe_last_error());
      return 2;
    }
    int moved = 0, with_depth = 0, without = 0;
    for (int i = 0; i < F.N; i++) {
      if (std::memcmp(&F.mvKeysUn[i], &un[i], sizeof(orbfe_keypoint)) != 0) failures++;
      if (std::memcmp(&F.mvuRight[i], &ur[i], 4) != 0 || std::memcmp(&F.mvDepth[i], &dep[i], 4) != 0) failures++;
      moved += F.mvKeysUn[i].pt.x != F.mvKeys[i].pt.x;
      (F.mvDepth[i] > 0 ? with_depth : without)++;
      if (F.mvKeysUn[i].size != F.mvKeys[i].size || F.mvKeysUn[i].octave != F.mvKeys[i].octave ||
          F.mvKeysUn[i].class_id != F.mvKeys[i].class_id)
        failures++;
    }
    if ((int)F.mvKeysUn.size() != F.N || (int)F.mvuRight.size() != F.N || (int)F.mvDepth.size() != F.N) failures++;
    const float fb[4] = {Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY};
    if (std::memcmp(fb, b, sizeof(b)) != 0) failures++;
    if (moved == 0 || with_depth == 0 || without == 0) failures++;  // the frame exercises every branch
    std::printf("n_dist %d: %d keys, %d moved, %d with depth, bounds %.4f %.4f %.4f %.4f\n", n_dist, F.N, moved,
                with_depth, b[0], b[1], b[2], b[3]);
  }
  std::printf(failures ? "FAILED: %d\n" : "adapter_sensors_test OK\n", failures);
  return failures ? 1 : 0;
}
