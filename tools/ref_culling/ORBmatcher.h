/*
 * A stand-in for the reference's include/ORBmatcher.h, for tools/ref_culling: what src/LocalMapping.cpp and src/MapPoint.cpp name of the matcher.
 * Culling never reaches any of it: the driver defines the members, and they abort.
 */
#ifndef ORBMATCHER_H
#define ORBMATCHER_H

#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class KeyFrame;
class MapPoint;

class ORBmatcher {
public:
    ORBmatcher(float nnratio = 0.6, bool checkOri = true);
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b);
    int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo);
    int Fuse(KeyFrame *pKF, const std::vector<MapPoint *> &vpMapPoints, const float th = 3.0);
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
};

}  // namespace Jetson_SLAM

#endif
