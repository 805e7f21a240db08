/*
 * <opencv2/core/core.hpp> for tools/ref_mappoint: the project's stand-in (oracle/ref_matcher/opencv2/core/core.hpp, included as it is) with the
 * two members the reference's src/MapPoint.cpp needs on top - cv::Mat::zeros and cv::Mat::copyTo.  The oracle's class is compiled under the name
 * MatBase and cv::Mat derives from it; the views and copies are repeated so that they give a cv::Mat again.  AUTHORING TOOLING ONLY.
 */
#ifndef JSORB_REF_MAPPOINT_OPENCV_CORE_HPP
#define JSORB_REF_MAPPOINT_OPENCV_CORE_HPP

#define Mat MatBase
#include "../../../../oracle/ref_matcher/opencv2/core/core.hpp"
#undef Mat

namespace cv {

class Mat : public MatBase {
public:
    Mat() {}
    Mat(int r, int c, int type) : MatBase(r, c, type) {}
    Mat(const MatBase &m) : MatBase(m) {}
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }          /* create() zero-fills */
    void copyTo(Mat &dst) const { dst = MatBase::clone(); }
    Mat clone() const { return MatBase::clone(); }
    Mat rowRange(int a, int b) const { return MatBase::rowRange(a, b); }
    Mat colRange(int a, int b) const { return MatBase::colRange(a, b); }
    Mat row(int i) const { return MatBase::row(i); }
    Mat col(int j) const { return MatBase::col(j); }
    Mat t() const { return MatBase::t(); }
};

}  // namespace cv

#endif
