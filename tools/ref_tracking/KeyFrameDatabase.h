/* A stand-in for the reference's include/KeyFrameDatabase.h, for tools/ref_tracking: SetBadFlag's last line and Tracking's relocalisation query;
 * never reached. */
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <vector>

namespace Jetson_SLAM {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    void erase(KeyFrame *) {}
    void clear() {}
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *) { return std::vector<KeyFrame *>(); }
};

}  // namespace Jetson_SLAM

#endif
