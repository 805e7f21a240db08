/*
 * A stand-in for the reference's include/ORBmatcher.h, for tools/ref_tracking: what src/Tracking.cpp and src/MapPoint.cpp name of the matcher.
 * SearchByProjection(Frame&, const vector<MapPoint*>&, th) is the one member that runs: the driver defines it, records th, the list and every
 * point's track fields, and matches nothing (the matcher itself is pinned by tests/golden/ref_matcher_search_local.npz).  The others abort.
 */
#ifndef ORBMATCHER_H
#define ORBMATCHER_H

#include <set>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class KeyFrame;
class MapPoint;
class Frame;

class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) {}
    static int DescriptorDistance(const cv::Mat &, const cv::Mat &) { cv::Mat::unused("DescriptorDistance"); return 0; }
    int SearchByProjection(Frame &F, const std::vector<MapPoint *> &vpMapPoints, const float th = 3);      /* tools/ref_tracking/driver.cpp */
    int SearchByProjection(Frame &, const Frame &, const float, const bool) { cv::Mat::unused("SearchByProjection(last frame)"); return 0; }
    int SearchByProjection(Frame &, KeyFrame *, const std::set<MapPoint *> &, const float, const int) { cv::Mat::unused("SearchByProjection(keyframe)"); return 0; }
    int SearchByBoW(KeyFrame *, Frame &, std::vector<MapPoint *> &) { cv::Mat::unused("SearchByBoW"); return 0; }
    int SearchForInitialization(Frame &, Frame &, std::vector<cv::Point2f> &, std::vector<int> &, int = 10) { cv::Mat::unused("SearchForInitialization"); return 0; }
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
};

}  // namespace Jetson_SLAM

#endif
