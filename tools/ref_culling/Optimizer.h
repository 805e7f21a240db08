/* A stand-in for the reference's include/Optimizer.h, for tools/ref_culling: the one call of src/LocalMapping.cpp; the driver's definition aborts. */
#ifndef OPTIMIZER_H
#define OPTIMIZER_H

namespace Jetson_SLAM {

class KeyFrame;
class Map;

class Optimizer {
public:
    static void LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap);
};

}  // namespace Jetson_SLAM

#endif
