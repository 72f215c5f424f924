// Frame_sensors_gpu.cc -- Frame::UndistortKeyPoints (src/Frame.cc:456-486), Frame::ComputeImageBounds
// (:488-520) and Frame::ComputeStereoFromRGBD (:702-723) of a GPU build of lreithmayr/ORB_SLAM2_2021, as
// drop-in bodies over the host entry points of include/orbfe_frame.h. At this point of the RGB-D and
// monocular constructors (Frame.cc:186-188, :247) the keypoints are in host memory (mvKeys, filled by
// ExtractORB), so the bodies run the shared rules on the host; the device path of the same rules is what
// orbfe_mono_frame / orbfe_rgbd_frame and the device batches use. The maintainer removes the three
// methods' bodies from src/Frame.cc and compiles this file beside it.
//
// Built only inside the reference's tree; anywhere else this translation
// unit is empty.
#if __has_include(<opencv2/core.hpp>) && __has_include("Frame.h")

#include <opencv2/core.hpp>

#include "Frame.h"
#include "orbfe.hpp"
#include "orbfe_frame.h"

namespace ORB_SLAM2 {

namespace {
// mK (3x3 CV_32F), mDistCoef (4x1 or 5x1 CV_32F, Tracking.cc:77-89) and mbf
orbfe_camera camera_of(const cv::Mat& K, const cv::Mat& distCoef, float bf) {
  orbfe_camera c{};
  c.fx = K.at<float>(0, 0);
  c.fy = K.at<float>(1, 1);
  c.cx = K.at<float>(0, 2);
  c.cy = K.at<float>(1, 2);
  c.n_dist = distCoef.rows * distCoef.cols;
  for (int i = 0; i < c.n_dist && i < 5; i++) c.dist[i] = distCoef.at<float>(i);
  c.bf = bf;
  return c;
}
}  // namespace

void Frame::UndistortKeyPoints() {
  mvKeysUn.resize(N);
  if (N == 0) return;
  const orbfe_camera cam = camera_of(mK, mDistCoef, mbf);
  const int st = orbfe_undistort_keypoints_host(&cam, reinterpret_cast<const orbfe_keypoint*>(mvKeys.data()), N,
                                                reinterpret_cast<orbfe_keypoint*>(mvKeysUn.data()));  // 28-byte cv::KeyPoint
  if (st != ORBFE_OK) throw orbfe::Error(st, "orbfe_undistort_keypoints_host");
}

void Frame::ComputeImageBounds(const cv::Mat& imLeft) {
  const orbfe_camera cam = camera_of(mK, mDistCoef, mbf);
  float b[4];
  const int st = orbfe_image_bounds(&cam, imLeft.rows, imLeft.cols, b);
  if (st != ORBFE_OK) throw orbfe::Error(st, "orbfe_image_bounds");
  mnMinX = b[0];
  mnMaxX = b[1];
  mnMinY = b[2];
  mnMaxY = b[3];
}

// imDepth is the CV_32F map Tracking::GrabImageRGBD converted (Tracking.cc:246-247): factor 1 here.
void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth) {
  mvuRight = std::vector<float>(N, -1);
  mvDepth = std::vector<float>(N, -1);
  if (N == 0) return;
  if (imDepth.type() != CV_32F) throw orbfe::Error(ORBFE_ERR_ARG, "ComputeStereoFromRGBD: imDepth is not CV_32F");
  const orbfe_camera cam = camera_of(mK, mDistCoef, mbf);
  const int st = orbfe_stereo_from_depth_host(&cam, reinterpret_cast<const orbfe_keypoint*>(mvKeys.data()),
                                              reinterpret_cast<const orbfe_keypoint*>(mvKeysUn.data()), N, imDepth.data,
                                              imDepth.step, ORBFE_DEPTH_F32, 1.0f, imDepth.rows, imDepth.cols,
                                              mvuRight.data(), mvDepth.data());
  if (st != ORBFE_OK) throw orbfe::Error(st, "orbfe_stereo_from_depth_host");
}

}  // namespace ORB_SLAM2

#endif
