/*
 * A stand-in for <opencv2/core/core.hpp>: the part of cv::Mat, cv::KeyPoint and cv::Point2f that the reference's src/ORBmatcher.cpp and
 * include/ORBmatcher.h use, and nothing else.  TEST INFRASTRUCTURE ONLY (the build rule and its purpose: oracle/Makefile, target ref_matcher).
 *
 * Covered: CV_32F matrices up to 4x4 and CV_8U descriptor matrices, both as owners and as views (row, rowRange, colRange, col share the
 * owner's storage); t(), Mat*Mat, Mat+Mat, Mat-Mat, -Mat, Mat/scalar, scalar*Mat, dot, cv::norm, at<float>, ptr<T>, data / step[].
 * There is no MatExpr: every operator returns its result at once.
 *
 * ARITHMETIC.  Every operation is plain float: a product row is a[0]*b[0] + a[1]*b[1] + ... summed left to right, one rounding per
 * operation, nothing fused (the build rule passes -ffp-contract=off); a double scalar is converted to float once, before it is used;
 * cv::norm and dot sum their squares / products left to right in float and norm takes sqrtf of the sum.  NOTHING AVAILABLE TO THIS PROJECT
 * CAN CONFIRM THAT OpenCV 4.10 ROUNDS THIS WAY (its gemm and norm kernels are SIMD code with their own summation order and, for norm, a
 * double accumulator).  The fixtures made with this header are therefore built so that every such product and sum is exact in float under
 * any order, with or without fusing (tools/ref_matcher_goldens.py): what they pin does not depend on this choice.
 */
#ifndef JSORB_REF_SHADOW_OPENCV_CORE_HPP
#define JSORB_REF_SHADOW_OPENCV_CORE_HPP

#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

struct Point2f {
    float x, y;
    Point2f() : x(0), y(0) {}
    Point2f(float x_, float y_) : x(x_), y(y_) {}
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
    Mat(int r, int c, int type) { create(r, c, type); }

    void create(int r, int c, int type) {
        rows = r, cols = c, type_ = type;
        step[1] = type == CV_32F ? sizeof(float) : 1;
        step[0] = step[1] * (size_t)c;
        store_ = std::make_shared<std::vector<unsigned char> >(step[0] * (size_t)r + 4, (unsigned char)0);
        data = store_->data();
    }
    int type() const { return type_; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }

    Mat clone() const {
        Mat m(rows, cols, type_);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++)
                std::memcpy(m.data + i * m.step[0] + j * m.step[1], data + i * step[0] + j * step[1], step[1]);
        return m;
    }

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

    float dot(const Mat &b) const {
        assert(rows * cols == b.rows * b.cols);
        float s = 0.0f;
        bool first = true;
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++) {
                const float p = at<float>(i, j) * b.el(i * cols + j);
                s = first ? p : s + p;
                first = false;
            }
        return s;
    }

    float el(int k) const { return at<float>(k / cols, k % cols); }

private:
    int type_;
    std::shared_ptr<std::vector<unsigned char> > store_;

    Mat view(int r0, int r1, int c0, int c1) const {
        Mat m;
        m.rows = r1 - r0, m.cols = c1 - c0, m.type_ = type_;
        m.step[0] = step[0], m.step[1] = step[1];
        m.data = data + r0 * step[0] + c0 * step[1];
        m.store_ = store_;
        return m;
    }
};

inline Mat operator*(const Mat &a, const Mat &b) {
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
    assert(a.rows == b.rows && a.cols == b.cols);
    Mat m(a.rows, a.cols, CV_32F);
    for (int i = 0; i < a.rows; i++)
        for (int j = 0; j < a.cols; j++)
            m.at<float>(i, j) = f(a.at<float>(i, j), b.at<float>(i, j));
    return m;
}
template <typename F> inline Mat jsorb_ref_map1(const Mat &a, F f) {
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

}  // namespace cv

#endif
