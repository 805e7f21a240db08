/*
 * <opencv2/core/core.hpp> for tools/ref_newpoints: a double of this project's own writing that lets the reference's src/LocalMapping.cpp,
 * src/KeyFrame.cpp and src/MapPoint.cpp compile and RUN LocalMapping::CreateNewMapPoints, with real float storage.  The model is
 * tools/ref_tracking/opencv2/core/core.hpp, whose operations mean the same here: a float matrix product summed left to right, norm = sqrtf of the
 * float sum of squares, Mat / double and double * Mat through (float)s, views that share the owner's storage.  What the contract of
 * jsorb_create_new_map_points (include/jsorb.h) defines anew is here as it is written there: Mat::dot accumulates (double)a * (double)b left to
 * right and returns double; SVD::compute is eight sweeps of one-sided Jacobi in double over the column pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
 * vt.row(3) the column of V with the smallest squared norm (ties to the highest index) rounded to float; an assignment to a row view
 * (A.row(0) = ...) copies the elements.  inv() is a 3x3 cofactor inverse in float: only ComputeF12 uses it, and its result feeds the stubbed
 * matcher alone.  AUTHORING TOOLING ONLY.
 */
#ifndef JSORB_REF_NEWPOINTS_OPENCV_CORE_HPP
#define JSORB_REF_NEWPOINTS_OPENCV_CORE_HPP

#include <cassert>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

struct Point2f {
    float x, y;
    Point2f() : x(0), y(0) {}
    Point2f(float x_, float y_) : x(x_), y(y_) {}
};
struct Point3f {
    float x, y, z;
    Point3f() : x(0), y(0), z(0) {}
    Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};

class Mat {
public:
    int rows, cols;
    unsigned char *data;
    size_t step[2];                       /* bytes between rows, bytes per element */

    Mat() : rows(0), cols(0), data(nullptr), type_(CV_32F) { step[0] = step[1] = 0; }
    Mat(const Mat &) = default;
    Mat &operator=(const Mat &o) & { rows = o.rows; cols = o.cols; data = o.data; step[0] = o.step[0]; step[1] = o.step[1]; type_ = o.type_; store_ = o.store_; return *this; }
    /* a temporary is a view (A.row(0) = expr): the elements are copied into the owner's storage */
    Mat &operator=(const Mat &o) && { assert(rows == o.rows && cols == o.cols && type_ == o.type_); assign(o); return *this; }
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(const Point3f &p) { create(3, 1, CV_32F); at<float>(0) = p.x; at<float>(1) = p.y; at<float>(2) = p.z; }

    void create(int r, int c, int type) {
        rows = r, cols = c, type_ = type;
        step[1] = type == CV_32F ? sizeof(float) : 1;
        step[0] = step[1] * (size_t)c;
        store_ = std::make_shared<std::vector<unsigned char> >(step[0] * (size_t)r + 4, (unsigned char)0);
        data = store_->data();
    }
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
    static Mat eye(int r, int c, int type) {
        Mat m(r, c, type);
        for (int i = 0; i < r && i < c; i++) m.at<float>(i, i) = 1.0f;
        return m;
    }
    int type() const { return type_; }
    int channels() const { return 1; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }

    Mat clone() const {
        Mat m;
        if (empty()) return m;
        m.create(rows, cols, type_);
        m.assign(*this);
        return m;
    }
    /* into a destination of the same shape (a view, too): element by element; otherwise the destination becomes a new owner */
    void copyTo(Mat &dst) const {
        if (empty()) { dst = Mat(); return; }
        if (dst.data == nullptr || dst.rows != rows || dst.cols != cols || dst.type_ != type_) dst.create(rows, cols, type_);
        dst.assign(*this);
    }
    void copyTo(Mat &&dst) const { copyTo(dst); }
    void convertTo(Mat &dst, int, double = 1.0) const { unused("Mat::convertTo"); copyTo(dst); }
    void resize(size_t) { unused("Mat::resize"); }

    /* views */
    Mat rowRange(int a, int b) const { return view(a, b, 0, cols); }
    Mat colRange(int a, int b) const { return view(0, rows, a, b); }
    Mat row(int i) const { return view(i, i + 1, 0, cols); }
    Mat col(int j) const { return view(0, rows, j, j + 1); }

    template <typename T> T &at(int i, int j) { return *(T *)(data + i * step[0] + j * step[1]); }
    template <typename T> const T &at(int i, int j) const { return *(const T *)(data + i * step[0] + j * step[1]); }
    /* one index: the element of a vector (a single column or a single row) */
    template <typename T> T &at(int i) { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    template <typename T> const T &at(int i) const { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    template <typename T> T *ptr(int i = 0) { return (T *)(data + i * step[0]); }
    template <typename T> const T *ptr(int i = 0) const { return (const T *)(data + i * step[0]); }

    Mat t() const {
        Mat m(cols, rows, CV_32F);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++)
                m.at<float>(j, i) = at<float>(i, j);
        return m;
    }
    Mat inv() const {
        assert(rows == 3 && cols == 3);
        Mat m(3, 3, CV_32F);
        const auto a = [this](int i, int j) { return at<float>(i % 3, j % 3); };
        const float det = a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0)) + a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0));
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) m.at<float>(j, i) = (a(i + 1, j + 1) * a(i + 2, j + 2) - a(i + 1, j + 2) * a(i + 2, j + 1)) / det;
        return m;
    }

    double dot(const Mat &b) const {
        assert(rows * cols == b.rows * b.cols);
        double s = 0.0;
        bool first = true;
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++) {
                const double p = (double)at<float>(i, j) * (double)b.el(i * cols + j);
                s = first ? p : s + p;
                first = false;
            }
        return s;
    }
    float el(int k) const { return at<float>(k / cols, k % cols); }

    static void unused(const char *what) { std::fprintf(stderr, "ref_newpoints: %s was reached\n", what); std::abort(); }

private:
    int type_;
    std::shared_ptr<std::vector<unsigned char> > store_;

    void assign(const Mat &src) {
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++)
                std::memcpy(data + i * step[0] + j * step[1], src.data + i * src.step[0] + j * src.step[1], step[1]);
    }
    Mat view(int r0, int r1, int c0, int c1) const {
        Mat m;
        if (data == nullptr) return m;
        m.rows = r1 - r0, m.cols = c1 - c0, m.type_ = type_;
        m.step[0] = step[0], m.step[1] = step[1];
        m.data = data + r0 * step[0] + c0 * step[1];
        m.store_ = store_;
        return m;
    }
};

inline Mat operator*(const Mat &a, const Mat &b) {
    if (a.empty() || b.empty()) return Mat();
    assert(a.cols == b.rows);
    Mat m(a.rows, b.cols, CV_32F);
    for (int i = 0; i < a.rows; i++)
        for (int j = 0; j < b.cols; j++) {
            float s = a.at<float>(i, 0) * b.at<float>(0, j);
            for (int k = 1; k < a.cols; k++) {
                const float p = a.at<float>(i, k) * b.at<float>(k, j);
                s = s + p;
            }
            m.at<float>(i, j) = s;
        }
    return m;
}

template <typename F> inline Mat jsorb_ref_map2(const Mat &a, const Mat &b, F f) {
    if (a.empty() || b.empty()) return Mat();
    assert(a.rows == b.rows && a.cols == b.cols);
    Mat m(a.rows, a.cols, CV_32F);
    for (int i = 0; i < a.rows; i++)
        for (int j = 0; j < a.cols; j++)
            m.at<float>(i, j) = f(a.at<float>(i, j), b.at<float>(i, j));
    return m;
}
template <typename F> inline Mat jsorb_ref_map1(const Mat &a, F f) {
    if (a.empty()) return Mat();
    Mat m(a.rows, a.cols, CV_32F);
    for (int i = 0; i < a.rows; i++)
        for (int j = 0; j < a.cols; j++)
            m.at<float>(i, j) = f(a.at<float>(i, j));
    return m;
}

inline Mat operator+(const Mat &a, const Mat &b) { return jsorb_ref_map2(a, b, [](float x, float y) { return x + y; }); }
inline Mat operator-(const Mat &a, const Mat &b) { return jsorb_ref_map2(a, b, [](float x, float y) { return x - y; }); }
inline Mat operator-(const Mat &a) { return jsorb_ref_map1(a, [](float x) { return -x; }); }
inline Mat operator/(const Mat &a, double s) { const float f = (float)s; return jsorb_ref_map1(a, [f](float x) { return x / f; }); }
inline Mat operator*(double s, const Mat &a) { const float f = (float)s; return jsorb_ref_map1(a, [f](float x) { return f * x; }); }
inline Mat operator*(const Mat &a, double s) { return s * a; }

inline double norm(const Mat &a) {
    float s = 0.0f;
    bool first = true;
    for (int i = 0; i < a.rows; i++)
        for (int j = 0; j < a.cols; j++) {
            const float p = a.at<float>(i, j) * a.at<float>(i, j);
            s = first ? p : s + p;
            first = false;
        }
    return (double)sqrtf(s);
}

struct SVD {
    enum { MODIFY_A = 1, FULL_UV = 4 };
    static void compute(const Mat &Af, Mat &, Mat &, Mat &vt, int = 0) {
        assert(Af.rows == 4 && Af.cols == 4);
        double A[4][4], V[4][4];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) { A[i][j] = (double)Af.at<float>(i, j); V[i][j] = i == j ? 1.0 : 0.0; }
        for (int sweep = 0; sweep < 8; sweep++)
            for (int p = 0; p < 3; p++)
                for (int q = p + 1; q < 4; q++) {
                    double alpha = A[0][p] * A[0][p], beta = A[0][q] * A[0][q], gamma = A[0][p] * A[0][q];
                    for (int k = 1; k < 4; k++) { alpha = alpha + A[k][p] * A[k][p]; beta = beta + A[k][q] * A[k][q]; gamma = gamma + A[k][p] * A[k][q]; }
                    if (gamma == 0.0) continue;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                    for (int k = 0; k < 4; k++) { const double a = A[k][p], b = A[k][q]; A[k][p] = c * a - s * b; A[k][q] = s * a + c * b; }
                    for (int k = 0; k < 4; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
                }
        int best = 0;
        double least = 0.0;
        for (int j = 0; j < 4; j++) {
            double n = A[0][j] * A[0][j];
            for (int k = 1; k < 4; k++) n = n + A[k][j] * A[k][j];
            if (j == 0 || n <= least) { least = n; best = j; }
        }
        vt = Mat(4, 4, CV_32F);                  /* only row 3 is read (LocalMapping.cpp:337) */
        for (int k = 0; k < 4; k++) vt.at<float>(3, k) = (float)V[k][best];
    }
};

template <class T> class Mat_ : public Mat {
public:
    Mat_(int r, int c) : Mat(r, c, CV_32F) {}
};
/* (Mat_<float>(r, c) << a, b, c): the values in row-major order */
template <class T> struct MatCommaInitializer_ {
    Mat m;
    int k;
    template <class U> MatCommaInitializer_ &operator,(U v) {
        m.template at<T>(k / m.cols, k % m.cols) = (T)v;
        k++;
        return *this;
    }
    operator Mat() const { return m; }
};
template <class T, class U> inline MatCommaInitializer_<T> operator<<(const Mat_<T> &m, U v) {
    MatCommaInitializer_<T> c;
    c.m = m;
    c.k = 0;
    return (c, v);
}

/* the settings file of Tracking's constructor: every number reads as 0 and every string as empty */
struct FileNode {
    template <class T> operator T() const { return T(); }
};
template <class T> inline void operator>>(const FileNode &, T &v) { v = T(); }
struct FileStorage {
    enum { READ = 0 };
    FileStorage(const std::string &, int) {}
    FileNode operator[](const char *) const { return FileNode(); }
};

}  // namespace cv

#endif
