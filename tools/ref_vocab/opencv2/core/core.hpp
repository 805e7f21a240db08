/*
 * <opencv2/core/core.hpp> for tools/ref_vocab: what DBoW2's TemplatedVocabulary.h, FORB.cpp, BowVector.cpp, FeatureVector.cpp and
 * ScoringObject.cpp need of OpenCV to compile unmodified.  cv::Mat is a reference-counted byte matrix with the few members FORB calls (copies
 * share the data, as OpenCV's do; release() leaves a matrix whose ptr() is null).  FileStorage / FileNode are tools/ref_kfdb's empty types, with
 * explicit conversions: TemplatedVocabulary::load casts a node to int, double and string.  AUTHORING TOOLING ONLY.
 */
#ifndef JSORB_REF_VOCAB_OPENCV_CORE_HPP
#define JSORB_REF_VOCAB_OPENCV_CORE_HPP

#include <float.h>
#include <math.h>                                /* ScoringObject.cpp calls ::sqrt and ::log, which OpenCV's header brings along */

#include <cstddef>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows, cols;
    Mat() : rows(0), cols(0) {}
    void create(int r, int c, int type)
    {
        rows = r; cols = c;
        data_ = std::make_shared<std::vector<unsigned char> >((size_t)r * c * (type == CV_32F ? 4 : 1));
    }
    static Mat zeros(int r, int c, int type) { Mat m; m.create(r, c, type); return m; }
    Mat clone() const
    {
        Mat m;
        m.rows = rows; m.cols = cols;
        if (data_) m.data_ = std::make_shared<std::vector<unsigned char> >(*data_);
        return m;
    }
    void release() { data_.reset(); rows = cols = 0; }
    bool empty() const { return !data_; }
    template <class T> T *ptr(int = 0) { return data_ ? reinterpret_cast<T *>(data_->data()) : (T *)0; }
    template <class T> const T *ptr(int = 0) const { return data_ ? reinterpret_cast<const T *>(data_->data()) : (const T *)0; }

private:
    std::shared_ptr<std::vector<unsigned char> > data_;
};

class FileNode {
public:
    enum { SEQ = 5 };
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    operator int() const { return 0; }
    operator double() const { return 0; }
    operator std::string() const { return std::string(); }
    int type() const { return 0; }
    size_t size() const { return 0; }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const std::string &, int) {}
    bool isOpened() const { return false; }
    void release() {}
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](const std::string &) const { return FileNode(); }
};

template <class T> FileStorage &operator<<(FileStorage &fs, const T &) { return fs; }

}  // namespace cv

#endif
