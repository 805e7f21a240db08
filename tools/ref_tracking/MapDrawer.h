/* A stand-in for the reference's include/MapDrawer.h (pangolin), for tools/ref_tracking: the one call of Tracking::Track; never reached. */
#ifndef MAPDRAWER_H
#define MAPDRAWER_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class MapDrawer {
public:
    void SetCurrentCameraPose(const cv::Mat &) { cv::Mat::unused("MapDrawer::SetCurrentCameraPose"); }
};

}  // namespace Jetson_SLAM

#endif
