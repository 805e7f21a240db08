/*
 * A stand-in for the reference's include/KeyFrame.h, for tools/ref_kfdb: the members of KeyFrame that src/KeyFrameDatabase.cpp touches.  The two
 * scores, which the reference's constructor leaves uninitialised, start at 0 (include/jsorb.h defines them so); the connected set and the
 * covisibility list are what the driver scripted.  AUTHORING TOOLING ONLY.
 */
#ifndef KEYFRAME_H
#define KEYFRAME_H

#include <set>
#include <vector>

#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

namespace Jetson_SLAM {

class KeyFrame {
public:
    KeyFrame() : mnId(0), mnLoopQuery(0), mnLoopWords(0), mLoopScore(0), mnRelocQuery(0), mnRelocWords(0), mRelocScore(0), slot(-1) {}

    std::set<KeyFrame *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)neighbours.size() < N) return neighbours;
        return std::vector<KeyFrame *>(neighbours.begin(), neighbours.begin() + N);
    }

    long unsigned int mnId;
    long unsigned int mnLoopQuery;
    int mnLoopWords;
    float mLoopScore;
    long unsigned int mnRelocQuery;
    int mnRelocWords;
    float mRelocScore;
    DBoW2::BowVector mBowVec;

    int slot;                                    /* the driver's: the slot it stands in */
    std::set<KeyFrame *> connected;
    std::vector<KeyFrame *> neighbours;
};

}  // namespace Jetson_SLAM

#endif
