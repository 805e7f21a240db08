/*
 * A stand-in for the reference's include/KeyFrame.h, for tools/ref_mappoint: the members of KeyFrame that src/MapPoint.cpp and src/ORBmatcher.cpp
 * touch, in the manner of oracle/ref_matcher/KeyFrame.h - but MapPoint is only forward-declared here, because the MapPoint this driver runs is the
 * reference's own include/MapPoint.h.  The member functions are defined by driver.cpp as far as the linked code calls them.
 */
#ifndef KEYFRAME_H
#define KEYFRAME_H

#include <cstddef>
#include <set>
#include <vector>

#include <opencv2/core/core.hpp>

#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"

namespace Jetson_SLAM {

class MapPoint;

class KeyFrame {
public:
    KeyFrame();

    cv::Mat GetRotation();
    cv::Mat GetTranslation();
    cv::Mat GetCameraCenter();

    std::vector<MapPoint *> GetMapPointMatches();
    std::set<MapPoint *> GetMapPoints();
    MapPoint *GetMapPoint(const size_t &idx);
    void AddMapPoint(MapPoint *pMP, const size_t &idx);
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP);
    void EraseMapPointMatch(const size_t &idx);
    bool isBad();

    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const;
    bool IsInImage(const float &x, const float &y) const;

    long unsigned int mnId, mnFrameId;
    int mnGridCols, mnGridRows;
    float mfGridElementWidthInv, mfGridElementHeightInv;
    float fx, fy, cx, cy, mbf;
    int N;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors;
    int mnScaleLevels;
    float mfLogScaleFactor;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    float mnMinX, mnMinY, mnMaxX, mnMaxY;

    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Ow;
    bool bad;                             /* what isBad() answers: set by the driver */
};

}  // namespace Jetson_SLAM

#endif
