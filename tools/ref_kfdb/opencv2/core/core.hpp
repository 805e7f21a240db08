/*
 * <opencv2/core/core.hpp> for tools/ref_kfdb: DBoW2's ScoringObject.cpp includes TemplatedVocabulary.h, whose save / load templates name
 * cv::FileStorage and cv::FileNode.  Nothing of them is instantiated here; these empty types only let the header parse.  AUTHORING TOOLING ONLY.
 */
#ifndef JSORB_REF_KFDB_OPENCV_CORE_HPP
#define JSORB_REF_KFDB_OPENCV_CORE_HPP

#include <float.h>
#include <math.h>                                /* ScoringObject.cpp calls ::sqrt and ::log, which OpenCV's header brings along */

#include <cstddef>
#include <sstream>
#include <string>

namespace cv {

class FileNode {
public:
    enum { SEQ = 5 };
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    template <class T> operator T() const { return T(); }
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
