/* A stand-in for the reference's include/LoopClosing.h, for tools/ref_culling: the one call of src/LocalMapping.cpp; the driver's definition aborts. */
#ifndef LOOPCLOSING_H
#define LOOPCLOSING_H

namespace Jetson_SLAM {

class KeyFrame;

class LoopClosing {
public:
    void InsertKeyFrame(KeyFrame *pKF);
};

}  // namespace Jetson_SLAM

#endif
