/* <opencv2/opencv.hpp> for tools/ref_tracking: the core double and the colour conversion Tracking's Grab* members name and the driver never calls. */
#ifndef JSORB_REF_TRACKING_OPENCV_HPP
#define JSORB_REF_TRACKING_OPENCV_HPP

#include <opencv2/core/core.hpp>
#include <opencv2/imgproc/types_c.h>

namespace cv {
inline void cvtColor(const Mat &, Mat &, int) { Mat::unused("cvtColor"); }
}  // namespace cv

#endif
