/* A stand-in for <opencv2/features2d/features2d.hpp>: cv::KeyPoint lives in the core stand-in. */
#ifndef JSORB_REF_SHADOW_OPENCV_FEATURES2D_HPP
#define JSORB_REF_SHADOW_OPENCV_FEATURES2D_HPP
#include <opencv2/core/core.hpp>
#endif
