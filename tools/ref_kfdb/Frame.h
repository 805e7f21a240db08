/*
 * A stand-in for the reference's include/Frame.h, for tools/ref_kfdb: what KeyFrameDatabase::DetectRelocalizationCandidates reads of a Frame.
 * AUTHORING TOOLING ONLY.
 */
#ifndef FRAME_H
#define FRAME_H

#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

namespace Jetson_SLAM {

class Frame {
public:
    Frame() : mnId(0) {}
    DBoW2::BowVector mBowVec;
    long unsigned int mnId;
};

}  // namespace Jetson_SLAM

#endif
