// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for the OpenCV / Eigen / g2o / line_descriptor headers that the reference's
// src/ORBextractor.cc pulls in through ORBextractor.h and Auxiliar.h, so that this one
// translation unit compiles where it lies without OpenCV (oracle/Makefile, target ref_orb).
// Written for this project: 8-bit single-channel cv::Mat with ROI views that share one
// buffer, the small value types, and declarations of the four OpenCV primitives that
// ref_orb_main.cpp defines over oracle/ocv_prims.hpp.  Nothing of the reference is
// declared here; the files beside this one only forward the include names to it.
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>
#include <iostream>
typedef unsigned char uchar;
#define CV_8U 0
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795
namespace cv {
inline int cvRound(double v) { return (int)std::nearbyint(v); }
float fastAtan2(float y, float x);
inline int cvFloor(double v) { int i = (int)v; return i - (i > v); }
inline int cvCeil(double v) { int i = (int)v; return i + (i < v); }
template <class T> struct Point_ { T x, y; Point_() : x(0), y(0) {} Point_(T a, T b) : x(a), y(b) {}
  template <class U> Point_(const Point_<U>& o) : x((T)o.x), y((T)o.y) {}
  Point_& operator*=(float s) { x = (T)(x * s); y = (T)(y * s); return *this; } };
typedef Point_<int> Point2i; typedef Point2i Point; typedef Point_<float> Point2f;
struct Size { int width, height; Size() : width(0), height(0) {} Size(int w, int h) : width(w), height(h) {} };
struct Rect { int x, y, width, height; Rect(int a, int b, int c, int d) : x(a), y(b), width(c), height(d) {} };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {} };
struct DMatch { int queryIdx, trainIdx, imgIdx; float distance; };
template <class T, int N> struct Vec { T v[N]; T operator()(int i) const { return v[i]; } };
typedef Vec<float, 4> Vec4f;
enum { BORDER_REFLECT_101 = 4, BORDER_ISOLATED = 16, INTER_LINEAR = 1 };
struct Mat {
  std::shared_ptr<std::vector<uchar>> buf; uchar* data; int rows, cols; size_t step;
  Mat() : data(nullptr), rows(0), cols(0), step(0) {}
  Mat(int r, int c, int) : Mat() { create(r, c, 0); }
  Mat(Size s, int) : Mat() { create(s.height, s.width, 0); }
  void create(int r, int c, int) { if (data && r == rows && c == cols) return;
    buf = std::make_shared<std::vector<uchar>>((size_t)r * c); data = buf->data(); rows = r; cols = c; step = (size_t)c; }
  static Mat zeros(int r, int c, int t) { Mat m(r, c, t); std::memset(m.data, 0, (size_t)r * c); return m; }
  int type() const { return 0; }
  size_t step1() const { return step; }
  bool empty() const { return !data || !rows || !cols; }
  template <class T> T& at(int y, int x) { return *(T*)(data + (ptrdiff_t)y * (ptrdiff_t)step + x); }
  template <class T> const T& at(int y, int x) const { return *(const T*)(data + (ptrdiff_t)y * (ptrdiff_t)step + x); }
  uchar* ptr(int y = 0) { return data + (size_t)y * step; }
  const uchar* ptr(int y = 0) const { return data + (size_t)y * step; }
  Mat operator()(const Rect& r) const { Mat m = *this; m.data = data + (size_t)r.y * step + r.x; m.rows = r.height; m.cols = r.width; return m; }
  Mat rowRange(int a, int b) const { return (*this)(Rect(0, a, cols, b - a)); }
  Mat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }
  Mat row(int y) const { return rowRange(y, y + 1); }
  Mat clone() const { Mat m(rows, cols, 0); for (int y = 0; y < rows; ++y) std::memcpy(m.ptr(y), ptr(y), cols); return m; }
  void copyTo(Mat m) const { m.create(rows, cols, 0); for (int y = 0; y < rows; ++y) std::memcpy(m.ptr(y), ptr(y), cols); }
  void release() { *this = Mat(); }
};
struct _InputArray { Mat* m; _InputArray(const Mat& x) : m(const_cast<Mat*>(&x)) {} bool empty() const { return m->empty(); } Mat getMat() const { return *m; } };
struct _OutputArray : _InputArray { _OutputArray(Mat& x) : _InputArray(x) {} void create(int r, int c, int t) const { m->create(r, c, t); } void release() const { m->release(); } };
typedef const _InputArray& InputArray; typedef const _OutputArray& OutputArray;
void FAST(const Mat& img, std::vector<KeyPoint>& kps, int threshold, bool nms);
void GaussianBlur(const Mat& src, Mat& dst, Size k, double sx, double sy, int border);
void resize(const Mat& src, Mat& dst, Size sz, double fx, double fy, int interp);
void copyMakeBorder(const Mat& src, Mat& dst, int t, int b, int l, int r, int border);
struct KeyPointsFilter { static void retainBest(std::vector<KeyPoint>& k, int n); };
namespace line_descriptor { struct KeyLine { float response, lineLength; }; }
}
namespace Eigen { template <class T, int R, int C> struct Matrix { T operator()(int) const { return T(); } };
typedef Matrix<double,3,3> Matrix3d; typedef Matrix<double,4,4> Matrix4d; typedef Matrix<double,3,1> Vector3d; typedef Matrix<double,2,1> Vector2d;
typedef Matrix<double,-1,-1> MatrixXd; typedef Matrix<double,-1,1> VectorXd; typedef Matrix<float,-1,1> VectorXf; }
