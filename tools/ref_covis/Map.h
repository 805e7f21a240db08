/* A stand-in for the reference's include/Map.h, for tools/ref_covis: what src/KeyFrame.cpp touches of the map. */
#ifndef MAP_H
#define MAP_H

namespace Jetson_SLAM {

class KeyFrame;

class Map {
public:
    void EraseKeyFrame(KeyFrame *) {}
};

}  // namespace Jetson_SLAM

#endif
