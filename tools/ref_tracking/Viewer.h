/* A stand-in for the reference's include/Viewer.h (pangolin), for tools/ref_tracking: what Tracking::Reset names; never reached. */
#ifndef VIEWER_H
#define VIEWER_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class Viewer {
public:
    void RequestStop() { cv::Mat::unused("Viewer::RequestStop"); }
    bool isStopped() { cv::Mat::unused("Viewer::isStopped"); return true; }
    void Release() { cv::Mat::unused("Viewer::Release"); }
};

}  // namespace Jetson_SLAM

#endif
