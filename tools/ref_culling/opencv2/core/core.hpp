/*
 * <opencv2/core/core.hpp> for tools/ref_culling: a double of this project's own writing that lets the reference's src/LocalMapping.cpp,
 * src/KeyFrame.cpp and src/MapPoint.cpp compile.  The driver runs only KeyFrameCulling with SetBadFlag and EraseObservation, which touch no matrix
 * (SetBadFlag's mTcp runs through it), so every operation here type-checks and does nothing.  AUTHORING TOOLING ONLY.
 */
#ifndef JSORB_REF_CULLING_OPENCV_CORE_HPP
#define JSORB_REF_CULLING_OPENCV_CORE_HPP

#include <climits>
#include <cmath>
#include <cstring>
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
    Mat inv() const { return Mat(); }
    int type() const { return CV_32F; }
    bool empty() const { return true; }
    double dot(const Mat &) const { return 0.0; }
    template <class T> T &at(int, int = 0) const
    {
        static T cell;
        return cell = T();
    }
    template <class T> T *ptr(int = 0) const { return nullptr; }
    int rows = 0, cols = 0;
    unsigned char *data = nullptr;
};
inline Mat operator-(const Mat &) { return Mat(); }
inline Mat operator-(const Mat &, const Mat &) { return Mat(); }
inline Mat operator+(const Mat &, const Mat &) { return Mat(); }
inline Mat operator*(const Mat &, const Mat &) { return Mat(); }
inline Mat operator*(const Mat &, double) { return Mat(); }
inline Mat operator*(double, const Mat &) { return Mat(); }
inline Mat operator/(const Mat &, double) { return Mat(); }
inline double norm(const Mat &) { return 0.0; }
struct SVD {
    enum { MODIFY_A = 1, FULL_UV = 4 };
    static void compute(const Mat &, Mat &, Mat &, Mat &, int = 0) {}
};

template <class T> class Mat_ : public Mat {
public:
    Mat_(int r, int c) : Mat(r, c, CV_32F) {}
};
/* (Mat_<float>(r, c) << a, b, c): the values are dropped */
template <class T> struct MatCommaInitializer_ {
    template <class U> MatCommaInitializer_ &operator,(U) { return *this; }
    operator Mat() const { return Mat(); }
};
template <class T, class U> inline MatCommaInitializer_<T> operator<<(const Mat_<T> &, U) { return MatCommaInitializer_<T>(); }

}  // namespace cv

#endif
