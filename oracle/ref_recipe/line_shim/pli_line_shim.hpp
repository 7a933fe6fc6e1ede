// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for the OpenCV / Eigen / g2o headers that the reference's line front end pulls in
// (src/LineExtractor.cc, src/Config.cpp, Thirdparty/line_descriptor/src/LSDDetector_custom.cpp and
// binary_descriptor_custom.cpp, through their own LineExtractor.h, Auxiliar.h, Config.h, descriptor_custom.hpp
// and precomp_custom.hpp), so that those four translation units compile where they lie without OpenCV
// (oracle/Makefile, target ref_line).  Written for this project; it supplies cv::, Eigen and g2o names only and
// declares nothing of the reference: KeyLine, BinaryDescriptor, LSDDetectorC, Lineextractor and Config come from
// the reference's real headers.  The files beside this one only forward the include names to it.
//
// What works: a typed single-channel cv::Mat (any depth by element size; used as 8U, 8S, 16S, 32S, 32F) that
// shares its buffer between copies, Mat_<T> with the converting assignment and row indexing that
// EDLineDetector::InitEDLine_ uses, Ptr, the value types, and DECLARATIONS of four primitives that
// ref_line_main.cpp defines over the oracle's restatements: LineSegmentDetector::detect (createLineSegmentDetector),
// LineIterator (its Point2f constructor: the conversion to integer points is part of that restatement),
// GaussianBlur and Sobel.
//
// What prints its name and abort()s: every operation reached only by code that Lineextractor::operator() never
// runs: the EDLine detector's Mat arithmetic (abs, add, threshold, compare, setTo, Mat / scalar, Mat_ products, sums and
// transposes), resize, pyrDown (one octave: its loop never runs), cvtColor, the FileStorage / FileNode reads and
// writes of Config::loadFromFile and BinaryDescriptor::Params, and Scalar::all (a default argument of the drawing
// functions, which are declared by the reference's header and defined in a file this recipe does not compile).
//
// Header regime.  namespace cv carries the using-declarations of std::min, max, abs, swap, sqrt, exp, pow and log that
// opencv2/core/base.hpp has, so sqrt(float) inside namespace cv is the float overload as under OpenCV.  cos, sin,
// atan2 and round are NOT among them: unqualified, they resolve in the global namespace, where only <math.h>'s
// C++ wrapper puts the float overloads.  This file pulls in <cmath> only; with -DPLI_LINE_SHIM_MATH_H it also
// includes <math.h> (binary pli_ref_line_mathh).  The reference's own bitarray_custom.hpp includes <math.h> before
// either of its two line_descriptor sources is compiled, so on a libstdc++ whose <math.h> is that wrapper (GCC 6 and
// later) the two regimes cannot differ; tests/test_ref_pin_line.py asserts what the two binaries do.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#ifdef PLI_LINE_SHIM_MATH_H
#include <math.h>
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

typedef unsigned char uchar;
#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_8UC1 CV_8U
#define CV_8SC1 CV_8S
#define CV_16SC1 CV_16S
#define CV_32SC1 CV_32S
#define CV_32FC1 CV_32F
#define CV_64FC1 CV_64F
#define CV_EXPORTS
#define CV_OUT
#define CV_IN_OUT
#define CV_WRAP
#define CV_PI 3.1415926535897932384626433832795

#define PLI_SHIM_DEAD(name) do { std::fprintf(stderr, "pli_line_shim: %s is not implemented\n", name); std::abort(); } while (0)

namespace cv {
using std::min; using std::max; using std::abs; using std::swap; using std::sqrt; using std::exp; using std::pow; using std::log;

typedef std::string String;
template <class T> struct DataType;
template <> struct DataType<uchar> { enum { type = CV_8U }; };
template <> struct DataType<signed char> { enum { type = CV_8S }; };
template <> struct DataType<short> { enum { type = CV_16S }; };
template <> struct DataType<int> { enum { type = CV_32S }; };
template <> struct DataType<float> { enum { type = CV_32F }; };
template <> struct DataType<double> { enum { type = CV_64F }; };

template <class T> struct Point_ { T x, y; Point_() : x(0), y(0) {} Point_(T a, T b) : x(a), y(b) {} };
typedef Point_<int> Point2i; typedef Point2i Point; typedef Point_<float> Point2f;
struct Size { int width, height; Size() : width(0), height(0) {} Size(int w, int h) : width(w), height(h) {}
  bool operator==(const Size& o) const { return width == o.width && height == o.height; }
  bool operator!=(const Size& o) const { return !(*this == o); } };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {} };
struct DMatch { int queryIdx, trainIdx, imgIdx; float distance; DMatch() : queryIdx(-1), trainIdx(-1), imgIdx(-1), distance(FLT_MAX) {} };
template <class T, int N> struct Vec { T v[N]; Vec() { for (int i = 0; i < N; ++i) v[i] = T(); }
  T& operator[](int i) { return v[i]; } const T& operator[](int i) const { return v[i]; }
  T& operator()(int i) { return v[i]; } const T& operator()(int i) const { return v[i]; } };
typedef Vec<float, 4> Vec4f;
struct Scalar { double v[4]; static Scalar all(double) { PLI_SHIM_DEAD("Scalar::all"); } };
enum { NORM_HAMMING = 6, COLOR_BGR2GRAY = 6, THRESH_TOZERO = 3, CMP_LT = 3, BORDER_DEFAULT = 4, INTER_LINEAR = 1 };

template <class T> struct Ptr : std::shared_ptr<T> {
  Ptr() {}
  explicit Ptr(T* p) : std::shared_ptr<T>(p) {}
  template <class U> Ptr(const Ptr<U>& o) : std::shared_ptr<T>(o) {}
};
template <class T> inline Ptr<T> makePtr() { return Ptr<T>(new T()); }
struct Algorithm { virtual ~Algorithm() {} };

struct _OutputArray;
struct Mat {
  std::shared_ptr<std::vector<uchar>> buf; uchar* data; int rows, cols; size_t step; int type_;
  Mat() : data(nullptr), rows(0), cols(0), step(0), type_(0) {}
  Mat(int r, int c, int t) : Mat() { create(r, c, t); }
  Mat(Size s, int t) : Mat() { create(s.height, s.width, t); }
  static size_t elemSizeOf(int t) { static const size_t k[7] = {1, 1, 2, 2, 4, 4, 8}; if (t < 0 || t > 6) PLI_SHIM_DEAD("Mat of more than one channel"); return k[t]; }
  // zero-filled, unlike OpenCV's: nothing that runs reads a plane before it is written
  void create(int r, int c, int t) { if (data && r == rows && c == cols && t == type_) return;
    buf = std::make_shared<std::vector<uchar>>((size_t)r * c * elemSizeOf(t)); data = buf->data(); rows = r; cols = c; type_ = t; step = (size_t)c * elemSizeOf(t); }
  int type() const { return type_; }
  int depth() const { return type_; }
  int channels() const { return 1; }
  size_t elemSize() const { return elemSizeOf(type_); }
  Size size() const { return Size(cols, rows); }
  bool empty() const { return !data || !rows || !cols; }
  template <class T> T& at(int y, int x) { return *(T*)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
  template <class T> const T& at(int y, int x) const { return *(const T*)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
  uchar* ptr(int y = 0) { return data + (size_t)y * step; }
  const uchar* ptr(int y = 0) const { return data + (size_t)y * step; }
  template <class T> T* ptr(int y = 0) { return (T*)(data + (size_t)y * step); }
  template <class T> const T* ptr(int y = 0) const { return (const T*)(data + (size_t)y * step); }
  Mat clone() const { Mat m; if (data) { m.create(rows, cols, type_); std::memcpy(m.data, data, (size_t)rows * step); } return m; }
  void copyTo(Mat& m) const { if (!data) { m = Mat(); return; } m.create(rows, cols, type_); std::memcpy(m.data, data, (size_t)rows * step); }
  inline void copyTo(const _OutputArray& o) const;
  void release() { *this = Mat(); }
  Mat& setTo(double) { PLI_SHIM_DEAD("Mat::setTo"); }
};
struct _InputArray { Mat* m; _InputArray(const Mat& x) : m(const_cast<Mat*>(&x)) {} bool empty() const { return m->empty(); } Mat getMat() const { return *m; } };
struct _OutputArray : _InputArray { _OutputArray(Mat& x) : _InputArray(x) {} void create(int r, int c, int t) const { m->create(r, c, t); } };
typedef const _InputArray& InputArray; typedef const _OutputArray& OutputArray;
inline void Mat::copyTo(const _OutputArray& o) const { copyTo(*o.m); }

template <class T> struct Mat_ : Mat {
  Mat_() { type_ = DataType<T>::type; }
  Mat_(int r, int c) : Mat(r, c, DataType<T>::type) {}
  // cv::Mat_<T>::operator=(const Mat&): converts the elements where the types differ
  template <class U> Mat_& operator=(const Mat_<U>& o) {
    Mat::create(o.rows, o.cols, DataType<T>::type);
    for (int y = 0; y < rows; ++y) for (int x = 0; x < cols; ++x) (*this)[y][x] = (T)o[y][x];
    return *this;
  }
  T* operator[](int y) { return (T*)Mat::ptr(y); }
  const T* operator[](int y) const { return (const T*)Mat::ptr(y); }
  Mat_ t() const { PLI_SHIM_DEAD("Mat_::t"); }
};
template <class T> inline Mat_<T> operator*(const Mat_<T>&, const Mat_<T>&) { PLI_SHIM_DEAD("Mat_ * Mat_"); }
template <class T> inline Mat_<T> operator+(const Mat_<T>&, const Mat_<T>&) { PLI_SHIM_DEAD("Mat_ + Mat_"); }
inline Mat operator/(const Mat&, double) { PLI_SHIM_DEAD("Mat / scalar"); }
inline Mat abs(const Mat&) { PLI_SHIM_DEAD("abs(Mat)"); }
inline void add(const Mat&, const Mat&, Mat&) { PLI_SHIM_DEAD("add"); }
inline double threshold(const Mat&, Mat&, double, double, int) { PLI_SHIM_DEAD("threshold"); }
inline void compare(const Mat&, const Mat&, Mat&, int) { PLI_SHIM_DEAD("compare"); }
inline void resize(const Mat&, Mat&, Size, double = 0, double = 0, int = INTER_LINEAR) { PLI_SHIM_DEAD("resize"); }
inline void pyrDown(const Mat&, Mat&, const Size& = Size()) { PLI_SHIM_DEAD("pyrDown"); }
inline void cvtColor(const Mat&, Mat&, int) { PLI_SHIM_DEAD("cvtColor"); }

struct FileNode { enum { NONE = 0, INT = 1, REAL = 2, STR = 3 };
  int type() const { PLI_SHIM_DEAD("FileNode::type"); }
  FileNode operator[](const char*) const { PLI_SHIM_DEAD("FileNode::operator[]"); }
  operator int() const { PLI_SHIM_DEAD("FileNode to int"); }
  operator float() const { PLI_SHIM_DEAD("FileNode to float"); }
  operator double() const { PLI_SHIM_DEAD("FileNode to double"); }
  operator std::string() const { PLI_SHIM_DEAD("FileNode to string"); } };
struct FileStorage { enum { READ = 0, WRITE = 1 };
  FileStorage() {}
  FileStorage(const std::string&, int) { PLI_SHIM_DEAD("FileStorage"); }
  FileNode operator[](const std::string&) const { PLI_SHIM_DEAD("FileStorage::operator[]"); } };
template <class T> inline FileStorage& operator<<(FileStorage&, const T&) { PLI_SHIM_DEAD("FileStorage <<"); }

// defined by ref_line_main.cpp over the oracle's restatements
void GaussianBlur(const Mat& src, Mat& dst, Size ksize, double sigmaX, double sigmaY = 0, int border = BORDER_DEFAULT);
void Sobel(const Mat& src, Mat& dst, int ddepth, int dx, int dy, int ksize = 3, double scale = 1, double delta = 0, int border = BORDER_DEFAULT);
struct LineIterator { int count; LineIterator(const Mat& img, Point2f pt1, Point2f pt2); };
struct LineSegmentDetector : Algorithm { virtual void detect(const Mat& image, std::vector<Vec4f>& lines) = 0; };
Ptr<LineSegmentDetector> createLineSegmentDetector(int refine = 1, double scale = 0.8, double sigma_scale = 0.6, double quant = 2.0,
                                                   double ang_th = 22.5, double log_eps = 0, double density_th = 0.7, int n_bins = 1024);
}  // namespace cv

// Auxiliar.h declares (never defines, never calls here) functions over these names
namespace Eigen { template <class T, int R, int C> struct Matrix { T operator()(int) const { return T(); } };
typedef Matrix<double,3,3> Matrix3d; typedef Matrix<double,4,4> Matrix4d; typedef Matrix<double,3,1> Vector3d; typedef Matrix<double,2,1> Vector2d;
typedef Matrix<double,-1,-1> MatrixXd; typedef Matrix<double,-1,1> VectorXd; typedef Matrix<float,-1,1> VectorXf; }
