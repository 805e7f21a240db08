/*
 * A stand-in for the reference's include/Frame.h: the members of Frame that src/ORBmatcher.cpp touches (see MapPoint.h here).  The grid
 * is cols x rows as the caller gives it (FRAME_GRID_COLS x FRAME_GRID_ROWS in the reference), the intrinsics and bounds are plain members
 * (static there).
 */
#ifndef FRAME_H
#define FRAME_H

#include "MapPoint.h"
#include "KeyFrame.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"
#include "cuda/orb_matcher.hpp"

using namespace std;
using namespace orb_cuda;

namespace Jetson_SLAM {

class Frame {
public:
    Frame();

    vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1, const int maxLevel = -1) const;
    void GetFeaturesInArea(const float &x, const float &y, const float &invzc, const float &r, std::vector<int> &nbr_indices,
                           const int minLevel = -1, const int maxLevel = -1);

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
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    cv::Mat mTcw;
    int mnScaleLevels;
    float mfLogScaleFactor;
    vector<float> mvScaleFactors;
    float mnMinX, mnMaxX, mnMinY, mnMaxY;
};

}  // namespace Jetson_SLAM

#endif
