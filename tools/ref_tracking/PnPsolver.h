/* A stand-in for the reference's include/PnPsolver.h, for tools/ref_tracking: Tracking::Relocalization's solver; never reached.  Like the
 * reference's, it includes MapPoint.h (the reference's own, with KeyFrame.h), which src/Tracking.cpp relies on.  It is NOT force-included: src/Tracking.cpp finds it on the
 * include path, after the force-included stand-ins that those two headers name. */
#ifndef PNPSOLVER_H
#define PNPSOLVER_H

#include <vector>

#include <opencv2/core/core.hpp>

#include "Frame.h"
#include "MapPoint.h"
#include "KeyFrame.h"

namespace Jetson_SLAM {

class MapPoint;

class PnPsolver {
public:
    PnPsolver(const Frame &, const std::vector<MapPoint *> &) { cv::Mat::unused("PnPsolver"); }
    void SetRansacParameters(double = 0.99, int = 8, int = 300, int = 4, float = 0.4, float = 5.991) { cv::Mat::unused("PnPsolver::SetRansacParameters"); }
    cv::Mat iterate(int, bool &, std::vector<bool> &, int &) { cv::Mat::unused("PnPsolver::iterate"); return cv::Mat(); }
};

}  // namespace Jetson_SLAM

#endif
