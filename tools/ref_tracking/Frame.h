/*
 * A stand-in for the reference's include/Frame.h, for tools/ref_tracking: the members the KeyFrame constructor copies (src/KeyFrame.cpp:35-61),
 * the ones a MapPoint constructor reads, and what src/Tracking.cpp names of a frame.  The driver fills mnId, N, mvpMapPoints, the pose (mRcw,
 * mtcw, mOw as real 3x3 / 3x1 float matrices), the camera, the bounds and the levels.  isInFrustum is the one member that runs (use_gpu_ = 0): the
 * driver defines it, logs the pointer and answers from K16.  Members the local-map path never reaches abort with their name.  <algorithm>,
 * <cmath>, <list> and the using-directive are here because the reference's sources rely on their headers for them.
 */
#ifndef FRAME_H
#define FRAME_H

#include <algorithm>
#include <cmath>
#include <list>
#include <map>
#include <set>
#include <vector>

#include <opencv2/opencv.hpp>

#include "ORBVocabulary.h"
#include "ORBextractor.h"
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

using namespace std;

namespace Jetson_SLAM {

class MapPoint;
class KeyFrame;

class Frame {
public:
    Frame() {}
    Frame(const cv::Mat &, const cv::Mat &, const double &, ORBExtractor *, ORBExtractor *, ORBVocabulary *, cv::Mat &, cv::Mat &, const float &,
          const float &, int) { cv::Mat::unused("Frame(stereo)"); }
    Frame(const cv::Mat &, const cv::Mat &, const double &, ORBExtractor *, ORBVocabulary *, cv::Mat &, cv::Mat &, const float &, const float &, int) {
        cv::Mat::unused("Frame(RGB-D)");
    }
    Frame(const cv::Mat &, const double &, ORBExtractor *, ORBVocabulary *, cv::Mat &, cv::Mat &, const float &, const float &, int) { cv::Mat::unused("Frame(mono)"); }
    void SetPose(cv::Mat) { cv::Mat::unused("Frame::SetPose"); }
    void UpdatePoseMatrices() { cv::Mat::unused("Frame::UpdatePoseMatrices"); }
    void ComputeBoW() { cv::Mat::unused("Frame::ComputeBoW"); }
    cv::Mat GetCameraCenter() { return mOw.clone(); }
    cv::Mat GetRotationInverse() { cv::Mat::unused("Frame::GetRotationInverse"); return cv::Mat(); }
    cv::Mat UnprojectStereo(const int &) { cv::Mat::unused("Frame::UnprojectStereo"); return cv::Mat(); }
    bool isInFrustum(MapPoint *pMP, float viewingCosLimit);      /* tools/ref_tracking/driver.cpp */
    static long unsigned int nNextId;
    static bool mbInitialComputations;
    long unsigned int mnId = 0;
    double mTimeStamp = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    float fx = 1, fy = 1, cx = 0, cy = 0, invfx = 1, invfy = 1, mbf = 0, mb = 0, mThDepth = 0;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    std::vector<bool> mvbOutlier;
    cv::Mat mDescriptors, mDescriptorsRight;
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    int mnScaleLevels = 1;
    float mfScaleFactor = 1, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    cv::Mat mK, mDistCoef, mTcw, mRcw, mtcw, mRwc, mOw;
    std::vector<MapPoint *> mvpMapPoints;
    ORBVocabulary *mpORBvocabulary = nullptr;
    ORBExtractor *mpORBextractorLeft = nullptr, *mpORBextractorRight = nullptr;
    KeyFrame *mpReferenceKF = nullptr;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
};

}  // namespace Jetson_SLAM

#endif
