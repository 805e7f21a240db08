/* A stand-in for the reference's include/LoopClosing.h, for tools/ref_tracking: the one call of Tracking::Reset; never reached. */
#ifndef LOOPCLOSING_H
#define LOOPCLOSING_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class LoopClosing {
public:
    void RequestReset() { cv::Mat::unused("LoopClosing::RequestReset"); }
};

}  // namespace Jetson_SLAM

#endif
