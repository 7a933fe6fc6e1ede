// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for <opencv2/core/core.hpp>, written for this project, as far as the reference's
// Thirdparty/DBoW2 (FORB.cpp, TemplatedVocabulary.h) names it: a reference-counted cv::Mat of
// CV_8U or CV_32F elements, and a cv::FileStorage / cv::FileNode pair that only throws (the
// YAML save / load are virtual, so they are instantiated, but the pin never calls them).
// create() zero-fills, OpenCV's does not: a descriptor DBoW2 leaves unwritten is 0 here.
#ifndef PLI_BOW_SHIM_CORE_HPP
#define PLI_BOW_SHIM_CORE_HPP
#include <cmath>
#include <cstddef>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

typedef unsigned char uchar;
#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
 public:
  int rows, cols;
  uchar* data;
  Mat() : rows(0), cols(0), data(NULL), m_type(CV_8U) {}
  Mat(int r, int c, int type) : rows(0), cols(0), data(NULL), m_type(CV_8U) { create(r, c, type); }
  void create(int r, int c, int type) {
    if (type != CV_8U && type != CV_32F) throw std::runtime_error("bow_shim cv::Mat: element type");
    if (data && r == rows && c == cols && type == m_type) return;
    rows = r; cols = c; m_type = type;
    m_buf = std::make_shared<std::vector<uchar> >((size_t)r * c * elemSize(), (uchar)0);
    data = m_buf->empty() ? NULL : m_buf->data();
  }
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
  size_t elemSize() const { return m_type == CV_32F ? 4 : 1; }
  int type() const { return m_type; }
  bool empty() const { return data == NULL; }
  template <class T> T* ptr(int row = 0) { return (T*)(data + (size_t)row * cols * elemSize()); }
  template <class T> const T* ptr(int row = 0) const { return (const T*)(data + (size_t)row * cols * elemSize()); }
  Mat clone() const {
    Mat m;
    if (data) { m.create(rows, cols, m_type); std::memcpy(m.data, data, m_buf->size()); }
    return m;
  }
  void release() { m_buf.reset(); data = NULL; rows = cols = 0; }

 private:
  int m_type;
  std::shared_ptr<std::vector<uchar> > m_buf;
};

class FileNode {
 public:
  FileNode operator[](const char*) const { fail(); return FileNode(); }
  FileNode operator[](const std::string&) const { fail(); return FileNode(); }
  FileNode operator[](int) const { fail(); return FileNode(); }
  size_t size() const { fail(); return 0; }
  operator int() const { fail(); return 0; }
  operator double() const { fail(); return 0; }
  operator std::string() const { fail(); return std::string(); }
  static void fail() { throw std::runtime_error("bow_shim: cv::FileStorage is not provided"); }
};

class FileStorage {
 public:
  enum { READ = 0, WRITE = 1 };
  FileStorage(const char*, int) { FileNode::fail(); }
  bool isOpened() const { return false; }
  FileNode operator[](const char*) const { FileNode::fail(); return FileNode(); }
  FileNode operator[](const std::string&) const { FileNode::fail(); return FileNode(); }
};
template <class T> FileStorage& operator<<(FileStorage& fs, const T&) { FileNode::fail(); return fs; }

}  // namespace cv
#endif
