/*
 * A stand-in for the reference's include/MapPoint.h, for tools/ref_covis: what src/KeyFrame.cpp touches of a map point.  The driver fills
 * observations and bad itself; EraseObservation does nothing, because a world's `registered` bytes do not change when a keyframe is erased.
 */
#ifndef MAPPOINT_H
#define MAPPOINT_H

#include <cstddef>
#include <map>

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class KeyFrame;

class MapPoint {
public:
    bool isBad() { return bad; }
    std::map<KeyFrame *, size_t> GetObservations() { return observations; }
    int Observations() { return (int)observations.size(); }
    void EraseObservation(KeyFrame *) {}
    int GetIndexInKeyFrame(KeyFrame *pKF) { return observations.count(pKF) ? (int)observations[pKF] : -1; }
    cv::Mat GetWorldPos() { return cv::Mat(); }

    bool bad = false;
    std::map<KeyFrame *, size_t> observations;
};

}  // namespace Jetson_SLAM

#endif
