/*
 * A stand-in for the reference's include/KeyFrame.h: the members of KeyFrame that src/ORBmatcher.cpp touches (see MapPoint.h here).
 * The image bounds are float here (const int in the reference): the comparisons convert an int to float first, so whole-number bounds
 * behave the same, and the project's keyframe description carries floats.
 */
#ifndef KEYFRAME_H
#define KEYFRAME_H

#include "MapPoint.h"
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"

namespace Jetson_SLAM {

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

    long unsigned int mnId;
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
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    cv::Mat Rcw, tcw, Ow;
};

}  // namespace Jetson_SLAM

#endif
