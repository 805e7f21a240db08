/* A stand-in for the reference's include/KeyFrameDatabase.h, for tools/ref_culling: SetBadFlag's last line. */
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

namespace Jetson_SLAM {

class KeyFrame;

class KeyFrameDatabase {
public:
    void erase(KeyFrame *) {}
};

}  // namespace Jetson_SLAM

#endif
