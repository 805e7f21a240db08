/* A stand-in for the reference's include/Map.h, for tools/ref_culling: what the three sources touch of the map.  It records what was erased. */
#ifndef MAP_H
#define MAP_H

#include <mutex>
#include <set>

namespace Jetson_SLAM {

class KeyFrame;
class MapPoint;

class Map {
public:
    void AddKeyFrame(KeyFrame *) {}
    void AddMapPoint(MapPoint *) {}
    void EraseKeyFrame(KeyFrame *pKF) { erased_keyframes.insert(pKF); }
    void EraseMapPoint(MapPoint *pMP) { erased_points.insert(pMP); }
    long unsigned int KeyFramesInMap() { return 0; }
    std::mutex mMutexPointCreation, mMutexMapUpdate;
    std::set<KeyFrame *> erased_keyframes;
    std::set<MapPoint *> erased_points;
};

}  // namespace Jetson_SLAM

#endif
