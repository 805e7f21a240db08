/* A stand-in for the reference's include/Converter.h, for tools/ref_culling: KeyFrame::ComputeBoW has to compile and is never called. */
#ifndef CONVERTER_H
#define CONVERTER_H

#include <vector>

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class Converter {
public:
    static std::vector<cv::Mat> toDescriptorVector(const cv::Mat &) { return std::vector<cv::Mat>(); }
};

}  // namespace Jetson_SLAM

#endif
