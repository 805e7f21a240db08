/* A stand-in for the reference's include/System.h, for tools/ref_tracking: the sensor kinds (SearchLocalPoints reads RGBD for th = 3) and Reset. */
#ifndef SYSTEM_H
#define SYSTEM_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class System {
public:
    enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 };
    void Reset() { cv::Mat::unused("System::Reset"); }
};

}  // namespace Jetson_SLAM

#endif
