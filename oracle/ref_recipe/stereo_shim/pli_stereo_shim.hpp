// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for everything the reference's src/LineMatcher.cpp (a whole translation unit), src/gridStructure.cpp, src/LineIterator.cpp,
// src/Config.cpp and the stereo functions of src/Frame.cc reach through their headers, written for this project.  oracle/Makefile
// (ref_stereo) force-includes this file (-include) in front of those sources, which are compiled where they lie, unmodified.  It
// predefines the include guards of the reference's Frame.h, MapPoint.h, MapLine.h, KeyFrame.h, ORBmatcher.h and ORBextractor.h, so
// that those headers (and OpenCV, Eigen, g2o, Sophus, DBoW2, boost behind them) stay out; the reference's own LineMatcher.h,
// gridStructure.h, LineIterator.h and Config.h are read as they are.
//
// ROUTE FOR Frame.cc: its definitions are cut out at build time (oracle/ref_recipe/cut_definitions.py: by the text a definition
// begins with and by brace matching) into oracle/_ref/stereo_Frame_cut.cc, which holds nothing else and is compiled behind this
// file.  The functions cut: AssignFeaturesToGrid, PosInGrid, GetFeaturesInArea, ComputeStereoMatches, ComputeStereoMatches_Lines,
// lineSegmentOverlapStereo, filterLineSegmentDisparity, ComputeStereoFromRGBD; and from src/ORBmatcher.cc the definitions of
// ORBmatcher::TH_HIGH, TH_LOW and DescriptorDistance, which ComputeStereoMatches reads.
//
// WHAT IS OURS HERE, and therefore NOT pinned: every class body below.  In particular
//   * cv::Mat: rowRange / colRange (a view; a range outside the matrix throws cv::Exception, as OpenCV's assertion does), convertTo
//     (CV_8U -> CV_16S, into fresh storage when the type changes, so a view's parent is never written), Mat - scalar on CV_16S
//     (saturating), push_back of rows, copyTo, clone;
//   * cv::norm(a, b, NORM_L1) on CV_16S: the integer sum of |a - b|, returned as double;
//   * cv::BFMatcher::knnMatch with NORM_HAMMING: brute force, the k nearest train rows per query row, equal distances to the lower
//     train index, fewer than k train rows give shorter rows; DMatch::distance is the bit count as a float;
//   * Eigen's Vector2d / Vector3d: the comma initialiser assigns coefficient by coefficient as each value arrives (the right-hand
//     sides are ordinary function arguments, evaluated before that call), cross() in the textbook order
//     (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), head(2), operator/ by a scalar per coefficient, operator();
//   * the Frame class: the reference's member names and types, none of its constructors; mnMinX ... mfGridElementHeightInv are
//     plain members here (statics there).
// WHAT THE PIN THEREFORE COVERS: the control flow, comparisons, conversions, visiting orders and scalar arithmetic of the functions
// named above as the compiler reads them, over the reference's own GridStructure::get, getLineCoords, LineIterator and Config.
#ifndef PLI_STEREO_SHIM_HPP
#define PLI_STEREO_SHIM_HPP
#define FRAME_H
#define MAPPOINT_H
#define MAPLINE_H
#define KEYFRAME_H
#define ORBMATCHER_H
#define ORBEXTRACTOR_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <list>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#define PLI_STEREO_DEAD(name) do { std::fprintf(stderr, "stereo_shim: %s has no stand-in (not reached by the pin)\n", name); std::abort(); } while (0)

#define CV_8U 0
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

namespace cv {

struct Exception : public std::runtime_error {
  explicit Exception(const std::string& what) : std::runtime_error(what) {}
};

enum { NORM_L1 = 2, NORM_HAMMING = 6 };

struct Point2f {
  float x, y;
  Point2f() : x(0), y(0) {}
  Point2f(float x_, float y_) : x(x_), y(y_) {}
};
struct KeyPoint {
  Point2f pt;
  float size = 0, angle = -1, response = 0;
  int octave = 0, class_id = -1;
};

class Mat {
 public:
  int rows = 0, cols = 0, flags = CV_8U;
  size_t step = 0;
  unsigned char* data = nullptr;

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }
  static size_t elemSizeOf(int type) { return type == CV_8U ? 1 : type == CV_16S ? 2 : 4; }
  void create(int r, int c, int type) {
    rows = r; cols = c; flags = type;
    step = (size_t)c * elemSizeOf(type);
    store_ = std::make_shared<std::vector<unsigned char>>((size_t)r * step, (unsigned char)0);
    data = store_->data();
  }
  int type() const { return flags; }
  size_t elemSize() const { return elemSizeOf(flags); }
  size_t total() const { return (size_t)rows * (size_t)cols; }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }

  template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data + (size_t)r * step); }
  template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data + (size_t)r * step); }
  template <class T> T& at(int r, int c) { return *reinterpret_cast<T*>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
  template <class T> const T& at(int r, int c) const { return *reinterpret_cast<const T*>(data + (size_t)r * step + (size_t)c * sizeof(T)); }

  Mat sub(int r0, int r1, int c0, int c1) const {        // a view on the same storage
    if (!(0 <= r0 && r0 <= r1 && r1 <= rows && 0 <= c0 && c0 <= c1 && c1 <= cols))
      throw Exception("Mat: range outside the matrix");
    Mat m;
    m.rows = r1 - r0; m.cols = c1 - c0; m.flags = flags; m.step = step; m.store_ = store_;
    m.data = data + (size_t)r0 * step + (size_t)c0 * elemSize();
    return m;
  }
  Mat row(int r) const { return sub(r, r + 1, 0, cols); }
  Mat rowRange(int r0, int r1) const { return sub(r0, r1, 0, cols); }
  Mat colRange(int c0, int c1) const { return sub(0, rows, c0, c1); }
  Mat clone() const {
    Mat m;
    if (rows == 0 || cols == 0) return m;
    m.create(rows, cols, flags);
    for (int r = 0; r < rows; ++r) std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, (size_t)cols * elemSize());
    return m;
  }
  void copyTo(Mat& dst) const { dst = clone(); }
  // CV_8U -> CV_16S or the identity.  The result has storage of its own whenever the type changes (OpenCV: Mat::create on dst).
  void convertTo(Mat& dst, int type) const {
    if (type == flags) { Mat m = clone(); dst = m; return; }
    if (flags != CV_8U || type != CV_16S) PLI_STEREO_DEAD("Mat::convertTo other than CV_8U -> CV_16S");
    Mat m(rows, cols, CV_16S);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) m.at<short>(r, c) = (short)at<unsigned char>(r, c);
    dst = m;
  }
  void reserve(size_t) {}
  void push_back(const Mat& m) {                         // rows of m appended
    if (m.rows == 0) return;
    if (rows != 0 && (m.cols != cols || m.flags != flags)) throw Exception("Mat::push_back: size or type differs");
    Mat out(rows + m.rows, m.cols, m.flags);
    for (int r = 0; r < rows; ++r) std::memcpy(out.data + (size_t)r * out.step, data + (size_t)r * step, (size_t)cols * elemSize());
    for (int r = 0; r < m.rows; ++r)
      std::memcpy(out.data + (size_t)(rows + r) * out.step, m.data + (size_t)r * m.step, (size_t)m.cols * m.elemSize());
    *this = out;
  }

 private:
  std::shared_ptr<std::vector<unsigned char>> store_;
};

// Mat - scalar, CV_16S only (what `IL - IL.at<short>(w, w)` asks for): per element, saturated to short
inline Mat operator-(const Mat& a, double s) {
  if (a.type() != CV_16S) PLI_STEREO_DEAD("Mat - scalar other than CV_16S");
  Mat m(a.rows, a.cols, CV_16S);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) {
      const double v = std::nearbyint((double)a.at<short>(r, c) - s);
      m.at<short>(r, c) = (short)(v < -32768.0 ? -32768.0 : v > 32767.0 ? 32767.0 : v);
    }
  return m;
}

// norm(a, b, NORM_L1) of two CV_16S matrices of one size
inline double norm(const Mat& a, const Mat& b, int normType) {
  if (normType != NORM_L1 || a.type() != CV_16S || b.type() != CV_16S || a.rows != b.rows || a.cols != b.cols)
    PLI_STEREO_DEAD("cv::norm other than NORM_L1 of two CV_16S matrices of one size");
  long long s = 0;
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) s += std::abs((int)a.at<short>(r, c) - (int)b.at<short>(r, c));
  return (double)s;
}

struct DMatch {
  int queryIdx = -1, trainIdx = -1, imgIdx = -1;
  float distance = 3.402823466e+38f;
  DMatch() {}
  DMatch(int q, int t, float d) : queryIdx(q), trainIdx(t), imgIdx(0), distance(d) {}
};

template <class T> using Ptr = std::shared_ptr<T>;

class BFMatcher {
 public:
  BFMatcher(int normType = NORM_HAMMING, bool crossCheck = false) : norm_(normType), cross_(crossCheck) {}
  static Ptr<BFMatcher> create(int normType = NORM_HAMMING, bool crossCheck = false) { return std::make_shared<BFMatcher>(normType, crossCheck); }
  void knnMatch(const Mat& query, const Mat& train, std::vector<std::vector<DMatch>>& matches, int k) const {
    if (norm_ != NORM_HAMMING || cross_) PLI_STEREO_DEAD("BFMatcher other than NORM_HAMMING without cross check");
    if (query.rows && train.rows && (query.type() != CV_8U || train.type() != CV_8U || query.cols != train.cols))
      throw Exception("BFMatcher::knnMatch: descriptor type or length differs");
    matches.clear();
    if (train.rows == 0) return;                          // (OpenCV returns no rows at all for an empty train set)
    matches.resize((size_t)query.rows);
    std::vector<std::pair<int, int>> d((size_t)train.rows);
    for (int q = 0; q < query.rows; ++q) {
      for (int t = 0; t < train.rows; ++t) {
        int bits = 0;
        for (int c = 0; c < query.cols; ++c) bits += __builtin_popcount((unsigned)(query.at<unsigned char>(q, c) ^ train.at<unsigned char>(t, c)));
        d[(size_t)t] = std::make_pair(bits, t);
      }
      std::sort(d.begin(), d.end());                      // by distance, then by train index
      for (int j = 0; j < k && j < train.rows; ++j) matches[(size_t)q].push_back(DMatch(q, d[(size_t)j].second, (float)d[(size_t)j].first));
    }
  }

 private:
  int norm_;
  bool cross_;
};

// Config.cpp's loadFromFile: declared so that it compiles; the driver sets Config's fields itself
struct FileNode {
  enum { NONE = 0, INT = 1, REAL = 2, STR = 3 };
  int type() const { PLI_STEREO_DEAD("FileNode::type"); }
  operator int() const { PLI_STEREO_DEAD("FileNode to int"); }
  operator float() const { PLI_STEREO_DEAD("FileNode to float"); }
  operator double() const { PLI_STEREO_DEAD("FileNode to double"); }
  operator std::string() const { PLI_STEREO_DEAD("FileNode to string"); }
};
struct FileStorage {
  enum { READ = 0 };
  FileStorage(const std::string&, int) { PLI_STEREO_DEAD("FileStorage"); }
  FileNode operator[](const std::string&) const { PLI_STEREO_DEAD("FileStorage::operator[]"); }
  bool isOpened() const { PLI_STEREO_DEAD("FileStorage::isOpened"); }
  void release() { PLI_STEREO_DEAD("FileStorage::release"); }
};

namespace line_descriptor {
struct KeyLine {
  float angle = 0;
  int class_id = -1, octave = 0;
  Point2f pt;
  float response = 0, size = 0;
  float startPointX = 0, startPointY = 0, endPointX = 0, endPointY = 0;
  float sPointInOctaveX = 0, sPointInOctaveY = 0, ePointInOctaveX = 0, ePointInOctaveY = 0;
  float lineLength = 0;
  int numOfPixels = 0;
};
}  // namespace line_descriptor

}  // namespace cv

namespace Eigen {
template <class T, int N> struct CommaInit;
template <class T, int R, int C> struct Matrix {
  static_assert(C == 1, "column vectors only");
  T v[R] = {};
  Matrix() {}
  Matrix(T a, T b) { static_assert(R == 2, "two coefficients"); v[0] = a; v[1] = b; }
  Matrix(T a, T b, T c) { static_assert(R == 3, "three coefficients"); v[0] = a; v[1] = b; v[2] = c; }
  T& operator()(int i) { return v[i]; }
  const T& operator()(int i) const { return v[i]; }
  Matrix<T, 3, 1> cross(const Matrix<T, 3, 1>& o) const {
    static_assert(R == 3, "cross of 3-vectors");
    return Matrix<T, 3, 1>(v[1] * o.v[2] - v[2] * o.v[1], v[2] * o.v[0] - v[0] * o.v[2], v[0] * o.v[1] - v[1] * o.v[0]);
  }
  Matrix<T, 2, 1> head(int n) const {
    if (n != 2) PLI_STEREO_DEAD("head(n) other than head(2)");
    return Matrix<T, 2, 1>(v[0], v[1]);
  }
  Matrix operator/(T s) const { Matrix m; for (int i = 0; i < R; ++i) m.v[i] = v[i] / s; return m; }
  CommaInit<T, R> operator<<(T s);
  CommaInit<T, R> operator<<(const Matrix& o);
};
// the comma initialiser: each value is stored where it arrives
template <class T, int N> struct CommaInit {
  Matrix<T, N, 1>* m;
  int n;
  CommaInit& operator,(T s) {
    if (n >= N) PLI_STEREO_DEAD("comma initialiser with too many coefficients");
    m->v[n++] = s;
    return *this;
  }
};
template <class T, int R, int C> CommaInit<T, R> Matrix<T, R, C>::operator<<(T s) { v[0] = s; return CommaInit<T, R>{this, 1}; }
template <class T, int R, int C> CommaInit<T, R> Matrix<T, R, C>::operator<<(const Matrix& o) {
  for (int i = 0; i < R; ++i) v[i] = o.v[i];
  return CommaInit<T, R>{this, R};
}
typedef Matrix<double, 2, 1> Vector2d;
typedef Matrix<double, 3, 1> Vector3d;
}  // namespace Eigen

// the reference's Frame.h chain says all of these before LineMatcher.h's text begins
using namespace std;
using namespace cv;
using namespace line_descriptor;
using namespace Eigen;

// The three orderings Linematcher::FrameBFMatch / lineDescriptorMAD name (the reference keeps them in Auxiliar.h, behind OpenCV, g2o
// and Eigen).  Ours, so that LineMatcher.cpp compiles as a whole; no case drives Linematcher's member functions.
struct sort_descriptor_by_queryIdx {
  bool operator()(const std::vector<cv::DMatch>& l, const std::vector<cv::DMatch>& r) const { return l[0].queryIdx < r[0].queryIdx; }
};
struct compare_descriptor_by_NN_dist {
  bool operator()(const std::vector<cv::DMatch>& l, const std::vector<cv::DMatch>& r) const { return l[0].distance < r[0].distance; }
};
struct compare_descriptor_by_NN12_dist {
  bool operator()(const std::vector<cv::DMatch>& l, const std::vector<cv::DMatch>& r) const {
    return l[1].distance - l[0].distance > r[1].distance - r[0].distance;
  }
};

namespace ORB_SLAM3 {

class Frame;
class KeyFrame;
class MapPoint;

class MapLine {
 public:
  cv::Mat mLDescriptor;
  cv::Mat GetDescriptor() { return mLDescriptor.clone(); }
};

// the members ComputeStereoMatches reads of an extractor
class ORBextractor {
 public:
  std::vector<cv::Mat> mvImagePyramid;
};

// declared here, defined by the text cut from the reference's ORBmatcher.cc
class ORBmatcher {
 public:
  static const int TH_LOW;
  static const int TH_HIGH;
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b);
};

}  // namespace ORB_SLAM3

#include "LineMatcher.h"      // the reference's own (line_2d, matchGrid, normalize, dot), and gridStructure.h behind it
#include "Config.h"           // the reference's own

namespace ORB_SLAM3 {

// The reference's member names and types (Frame.h); the function bodies come from the text cut out of Frame.cc.
class Frame {
 public:
  Frame() {}
  // cut from Frame.cc
  void AssignFeaturesToGrid();
  bool PosInGrid(const cv::KeyPoint& kp, int& posX, int& posY);
  vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const int minLevel = -1, const int maxLevel = -1,
                                   const bool bRight = false) const;
  void ComputeStereoMatches();
  void ComputeStereoMatches_Lines(bool initial = false);
  double lineSegmentOverlapStereo(double spl_obs, double epl_obs, double spl_proj, double epl_proj);
  void filterLineSegmentDisparity(Vector2d spl, Vector2d epl, Vector2d spr, Vector2d epr, double& disp_s, double& disp_e);
  void ComputeStereoFromRGBD(const cv::Mat& imDepth);

  ORBextractor *mpORBextractorLeft = nullptr, *mpORBextractorRight = nullptr;
  float mbf = 0, mb = 0;
  int N = 0, N_l = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
  std::vector<cv::line_descriptor::KeyLine> mvKeys_Line, mvKeysRight_Line;
  std::vector<float> mvuRight, mvDepth;
  std::vector<pair<float, float>> mvDisparity_l;
  std::vector<Vector3d> mvle_l;
  cv::Mat mDescriptors, mDescriptorsRight;
  cv::Mat mDescriptors_Line, mDescriptorsRight_Line;
  float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
  std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
  vector<float> mvScaleFactors, mvInvScaleFactors;
  double inv_width = 0, inv_height = 0;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
  int Nleft = -1, Nright = -1;
  std::vector<std::size_t> mGridRight[FRAME_GRID_COLS][FRAME_GRID_ROWS];
};

}  // namespace ORB_SLAM3
#endif
