/*
 * A stand-in for the reference's include/Frame.h, for tools/ref_mappoint: the members of Frame that src/MapPoint.cpp and src/ORBmatcher.cpp touch
 * (see KeyFrame.h here); MapPoint is only forward-declared.
 */
#ifndef FRAME_H
#define FRAME_H

#include <vector>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#include "cuda/orb_matcher.hpp"

using namespace std;
using namespace orb_cuda;

namespace Jetson_SLAM {

class MapPoint;

class Frame {
public:
    Frame();

    cv::Mat GetCameraCenter();
    vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const;
    void GetFeaturesInArea(const float &x, const float &y, const float &invzc, const float &r, std::vector<int> &nbr_indices,
                           const int minLevel = -1, const int maxLevel = -1);

    long unsigned int mnId;
    float fx, fy, cx, cy, mbf, mb;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    float mfGridElementWidthInv, mfGridElementHeightInv;
    int mnGridCols, mnGridRows;
    cv::Mat mTcw;
    int mnScaleLevels;
    float mfLogScaleFactor;
    vector<float> mvScaleFactors;
    float mnMinX, mnMaxX, mnMinY, mnMaxY;
};

}  // namespace Jetson_SLAM

#endif
