/* A stand-in for the reference's include/FrameDrawer.h, for tools/ref_tracking: Tracking's constructor writes the tile size; Update is never reached. */
#ifndef FRAMEDRAWER_H
#define FRAMEDRAWER_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class Tracking;

class FrameDrawer {
public:
    void Update(Tracking *) { cv::Mat::unused("FrameDrawer::Update"); }
    int tile_h_ = 0, tile_w_ = 0;
};

}  // namespace Jetson_SLAM

#endif
