/* A stand-in for the reference's include/Map.h, for tools/ref_tracking: what the three sources touch of the map.  UpdateLocalMap hands it the local
 * map points "for visualization" (Tracking.cpp:1811): it keeps the last list, which the driver never reads back. */
#ifndef MAP_H
#define MAP_H

#include <mutex>
#include <set>
#include <vector>

namespace Jetson_SLAM {

class KeyFrame;
class MapPoint;

class Map {
public:
    void AddKeyFrame(KeyFrame *) {}
    void AddMapPoint(MapPoint *) {}
    void EraseKeyFrame(KeyFrame *) {}
    void EraseMapPoint(MapPoint *) {}
    void SetReferenceMapPoints(const std::vector<MapPoint *> &v) { reference_points = v; }
    std::vector<MapPoint *> GetAllMapPoints() { return std::vector<MapPoint *>(); }
    long unsigned int KeyFramesInMap() { return 0; }
    long unsigned int MapPointsInMap() { return 0; }
    void clear() {}
    std::vector<KeyFrame *> mvpKeyFrameOrigins;
    std::mutex mMutexPointCreation, mMutexMapUpdate;
    std::vector<MapPoint *> reference_points;
};

}  // namespace Jetson_SLAM

#endif
