/* A stand-in for the reference's include/Initializer.h, for tools/ref_tracking: the monocular initialisation of Tracking; never reached. */
#ifndef INITIALIZER_H
#define INITIALIZER_H

#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"

namespace Jetson_SLAM {

class Initializer {
public:
    Initializer(const Frame &, float = 1.0, int = 200) { cv::Mat::unused("Initializer"); }
    bool Initialize(const Frame &, const std::vector<int> &, cv::Mat &, cv::Mat &, std::vector<cv::Point3f> &, std::vector<bool> &) {
        cv::Mat::unused("Initializer::Initialize");
        return false;
    }
};

}  // namespace Jetson_SLAM

#endif
