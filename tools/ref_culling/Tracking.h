/* A stand-in for the reference's include/Tracking.h, for tools/ref_culling: src/LocalMapping.cpp holds a pointer to it and calls nothing. */
#ifndef TRACKING_H
#define TRACKING_H

namespace Jetson_SLAM {

class Tracking {
};

}  // namespace Jetson_SLAM

#endif
