// TEST-ONLY superset of cvstub/Frame.h for adapter/Frame_sensors_gpu.cc (tests/cpp/adapter_sensors_test.cpp):
// the same declaration plus what the RGB-D and monocular constructors' steps touch, with the reference's
// member names (include/Frame.h): UndistortKeyPoints, ComputeImageBounds, ComputeStereoFromRGBD and mDistCoef.
// This directory comes before cvstub/ on the include path; everything else is taken from cvstub/.
#ifndef ORBFE_TEST_STUB_SENSORS_FRAME_H
#define ORBFE_TEST_STUB_SENSORS_FRAME_H

#include <vector>

#include <opencv2/core.hpp>

#include "DBoW2/FeatureVector.h"
#include "ORBextractor.h"

namespace ORB_SLAM2 {

class MapPoint;

class Frame {
 public:
  void ExtractORB(int flag, const cv::Mat& im);
  void ComputeStereoMatches();
  void UndistortKeyPoints();
  void ComputeImageBounds(const cv::Mat& imLeft);
  void ComputeStereoFromRGBD(const cv::Mat& imDepth);

  ORBextractor *mpORBextractorLeft = nullptr, *mpORBextractorRight = nullptr;
  cv::Mat mK;
  cv::Mat mDistCoef;
  inline static float fx = 0.f;
  inline static float fy = 0.f;
  inline static float cx = 0.f;
  inline static float cy = 0.f;
  float mbf = 0.f;
  float mb = 0.f;
  int N = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<float> mvDepth;
  DBoW2::FeatureVector mFeatVec;
  cv::Mat mDescriptors, mDescriptorsRight;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  inline static float mfGridElementWidthInv = 0.f;
  inline static float mfGridElementHeightInv = 0.f;
  cv::Mat mTcw;
  int mnScaleLevels = 0;
  float mfScaleFactor = 0.f;
  float mfLogScaleFactor = 0.f;
  std::vector<float> mvScaleFactors;
  std::vector<float> mvInvScaleFactors;
  std::vector<float> mvLevelSigma2;
  std::vector<float> mvInvLevelSigma2;
  inline static float mnMinX = 0.f;
  inline static float mnMaxX = 0.f;
  inline static float mnMinY = 0.f;
  inline static float mnMaxY = 0.f;
};

}  // namespace ORB_SLAM2

#endif
