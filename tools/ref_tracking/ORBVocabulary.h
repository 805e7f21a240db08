/* A stand-in for the reference's include/ORBVocabulary.h, for tools/ref_culling: KeyFrame::ComputeBoW has to compile and is never called. */
#ifndef ORBVOCABULARY_H
#define ORBVOCABULARY_H

#include <vector>

#include <opencv2/core/core.hpp>

#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"

namespace Jetson_SLAM {

class ORBVocabulary {
public:
    void transform(const std::vector<cv::Mat> &, DBoW2::BowVector &, DBoW2::FeatureVector &, int) const {}
};

}  // namespace Jetson_SLAM

#endif
