/*
 * A stand-in for the reference's include/Frame.h, for tools/ref_culling: the members the KeyFrame constructor copies (src/KeyFrame.cpp:35-61) and
 * the ones a MapPoint constructor reads.  The driver fills the keypoints' octaves, mvuRight, mvDepth, mThDepth and mvpMapPoints.  <algorithm>,
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

#include <opencv2/core/core.hpp>

#include "ORBVocabulary.h"
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
    cv::Mat GetCameraCenter() { return cv::Mat(); }
    long unsigned int mnId = 0;
    double mTimeStamp = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    float fx = 1, fy = 1, cx = 0, cy = 0, invfx = 1, invfy = 1, mbf = 0, mb = 0, mThDepth = 0;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors;
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    int mnScaleLevels = 1;
    float mfScaleFactor = 1, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    cv::Mat mK, mTcw;
    std::vector<MapPoint *> mvpMapPoints;
    ORBVocabulary *mpORBvocabulary = nullptr;
    KeyFrame *mpReferenceKF = nullptr;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
};

}  // namespace Jetson_SLAM

#endif
