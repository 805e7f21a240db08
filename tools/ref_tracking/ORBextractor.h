/* A stand-in for the reference's include/ORBextractor.h, for tools/ref_tracking: Tracking's constructor makes extractors and nothing runs them. */
#ifndef ORBEXTRACTOR_H
#define ORBEXTRACTOR_H

#include <string>

namespace Jetson_SLAM {

class ORBExtractor {
public:
    ORBExtractor(int, int, float, int, int, int, int, int, const std::string &, int, int, int, int, int, int) {}
};

}  // namespace Jetson_SLAM

#endif
