/*
 * A stand-in for the reference's include/MapPoint.h: the members of MapPoint that src/ORBmatcher.cpp touches.  TEST INFRASTRUCTURE ONLY.
 * It defines the include guard of the header it stands in for, so that the reference's include/ORBmatcher.h (whose #include "MapPoint.h"
 * finds its own directory first) reads nothing more; the build rule passes the three stand-ins with -include.
 * The member functions (harness.cpp) are this project's restatements of src/MapPoint.cpp, cited there line by line.
 */
#ifndef MAPPOINT_H
#define MAPPOINT_H

#include <map>
#include <set>
#include <vector>
#include <mutex>
#include <chrono>
#include <iostream>
#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class KeyFrame;
class Frame;

class MapPoint {
public:
    MapPoint();

    cv::Mat GetWorldPos();
    cv::Mat GetNormal();
    cv::Mat GetDescriptor();
    void GetWorldPosExp(float &Px, float &Py, float &Pz);
    void GetDescriptorExp(unsigned char *output);

    int Observations();
    bool isBad();
    bool IsInKeyFrame(KeyFrame *pKF);
    int GetIndexInKeyFrame(KeyFrame *pKF);
    void AddObservation(KeyFrame *pKF, size_t idx);
    void Replace(MapPoint *pMP);
    void ComputeDistinctiveDescriptors();

    float GetMinDistanceInvariance();
    float GetMaxDistanceInvariance();
    int PredictScale(const float &currentDist, KeyFrame *pKF);
    int PredictScale(const float &currentDist, Frame *pF);

    long unsigned int mnId;

    /* Tracking::SearchLocalPoints' hand-over (Frame::isInFrustum writes them) */
    float mTrackProjX, mTrackProjY, mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;

    /* state, set by the harness */
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    std::map<KeyFrame *, size_t> mObservations;
    int nObs;
    bool mbBad;
    MapPoint *mpReplaced;
    float mfMinDistance, mfMaxDistance;
};

}  // namespace Jetson_SLAM

#endif
