/*
 * A stand-in for the reference's include/Map.h, for tools/ref_mappoint: what src/MapPoint.cpp touches of the map.  <climits> and <algorithm> are
 * included here because MapPoint.cpp uses INT_MAX and sort without including them itself.
 */
#ifndef MAP_H
#define MAP_H

#include <algorithm>
#include <climits>
#include <mutex>

namespace Jetson_SLAM {

class MapPoint;

class Map {
public:
    void EraseMapPoint(MapPoint *) {}
    std::mutex mMutexPointCreation;
};

}  // namespace Jetson_SLAM

#endif
