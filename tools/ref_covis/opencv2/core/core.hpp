/*
 * <opencv2/core/core.hpp> for tools/ref_covis: a double of this project's own writing that lets the reference's src/KeyFrame.cpp compile.  The
 * driver runs only the covisibility functions, which touch no matrix, so every operation here type-checks and does nothing (SetPose and
 * SetBadFlag's mTcp run through them).  tools/ref_mappoint's double computes; this one does not have to.  AUTHORING TOOLING ONLY.
 */
#ifndef JSORB_REF_COVIS_OPENCV_CORE_HPP
#define JSORB_REF_COVIS_OPENCV_CORE_HPP

#include <cmath>
#include <vector>

#define CV_32F 5

namespace cv {

struct Point2f {
    float x = 0, y = 0;
};
struct KeyPoint {
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};

class Mat {
public:
    Mat() {}
    Mat(int, int, int) {}
    static Mat eye(int, int, int) { return Mat(); }
    static Mat zeros(int, int, int) { return Mat(); }
    Mat clone() const { return Mat(); }
    void copyTo(const Mat &) const {}
    Mat rowRange(int, int) const { return Mat(); }
    Mat colRange(int, int) const { return Mat(); }
    Mat row(int) const { return Mat(); }
    Mat col(int) const { return Mat(); }
    Mat t() const { return Mat(); }
    int type() const { return CV_32F; }
    bool empty() const { return true; }
    double dot(const Mat &) const { return 0.0; }
    template <class T> T &at(int, int)
    {
        static T cell;
        return cell = T();
    }
    int rows = 0, cols = 0;
};
inline Mat operator-(const Mat &) { return Mat(); }
inline Mat operator-(const Mat &, const Mat &) { return Mat(); }
inline Mat operator+(const Mat &, const Mat &) { return Mat(); }
inline Mat operator*(const Mat &, const Mat &) { return Mat(); }

template <class T> class Mat_ : public Mat {
public:
    Mat_(int r, int c) : Mat(r, c, CV_32F) {}
};
/* (Mat_<float>(r, c) << a, b, c): the values are dropped */
template <class T> struct MatCommaInitializer_ {
    MatCommaInitializer_ &operator,(T) { return *this; }
    operator Mat() const { return Mat(); }
};
template <class T> inline MatCommaInitializer_<T> operator<<(const Mat_<T> &, T) { return MatCommaInitializer_<T>(); }

}  // namespace cv

#endif
