/* A stand-in for the reference's include/Optimizer.h, for tools/ref_tracking: the calls of src/Tracking.cpp.  The driver stops after
 * SearchLocalPoints, before TrackLocalMap's PoseOptimization; never reached. */
#ifndef OPTIMIZER_H
#define OPTIMIZER_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class Frame;
class Map;

class Optimizer {
public:
    static int PoseOptimization(Frame *) { cv::Mat::unused("Optimizer::PoseOptimization"); return 0; }
    static void GlobalBundleAdjustemnt(Map *, int = 5, bool * = nullptr, const unsigned long = 0, const bool = true) { cv::Mat::unused("Optimizer::GlobalBundleAdjustemnt"); }
};

}  // namespace Jetson_SLAM

#endif
