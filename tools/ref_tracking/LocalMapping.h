/* A stand-in for the reference's include/LocalMapping.h, for tools/ref_tracking: what Tracking names of the local mapper; never reached. */
#ifndef LOCALMAPPING_H
#define LOCALMAPPING_H

#include <opencv2/core/core.hpp>

namespace Jetson_SLAM {

class KeyFrame;

class LocalMapping {
public:
    void InsertKeyFrame(KeyFrame *) { cv::Mat::unused("LocalMapping::InsertKeyFrame"); }
    bool isStopped() { cv::Mat::unused("LocalMapping::isStopped"); return false; }
    bool stopRequested() { cv::Mat::unused("LocalMapping::stopRequested"); return false; }
    bool AcceptKeyFrames() { cv::Mat::unused("LocalMapping::AcceptKeyFrames"); return false; }
    void InterruptBA() { cv::Mat::unused("LocalMapping::InterruptBA"); }
    int KeyframesInQueue() { cv::Mat::unused("LocalMapping::KeyframesInQueue"); return 0; }
    bool SetNotStop(bool) { cv::Mat::unused("LocalMapping::SetNotStop"); return false; }
    void RequestReset() { cv::Mat::unused("LocalMapping::RequestReset"); }
};

}  // namespace Jetson_SLAM

#endif
