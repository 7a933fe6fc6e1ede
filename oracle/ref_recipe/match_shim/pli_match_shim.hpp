// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for everything the reference's src/ORBmatcher.cc (and src/CameraModels/Pinhole.cpp) reaches through its headers, written
// for this project.  oracle/Makefile force-includes this file (-include) in front of those sources, which are compiled where they
// lie, unmodified.  It predefines the include guards of the reference's MapPoint.h, KeyFrame.h, Frame.h, Pinhole.h,
// GeometricCamera.h and TwoViewReconstruction.h, so that those headers (and OpenCV, Eigen, g2o, Sophus, boost behind them) stay
// out, and declares classes of this project's own that carry only the members those two sources touch.  Member names and types are
// the reference's; every body is ours.
//
// ARITHMETIC CONVENTION of the cv::Mat here (the one DESIGN.md §2 / §9 and tests/test_fuse_search_cpu.py: gemm_row state):
//   * A * B + C is ONE gemm: the float elements multiplied and summed in double, alpha applied to the sum, the addend added in the
//     same double, one rounding to float per element.  Products are lazy (MatExpr), as OpenCV's are: -A.t() * b is the gemm with
//     alpha = -1, a chain A * B * C materialises (A * B) as float first, (A * b) + c folds c into the gemm.
//   * Mat / s and s * Mat are (float)(x * alpha) with alpha = 1.0 / s resp. s in double.
//   * Mat + Mat and Mat - Mat are float operations per element.
//   * inv() of a 3 x 3 CV_32F matrix is the closed form: determinant and cofactors in double, each element
//     (float)(cofactor * (1 / det)), all zeros for det == 0.
//   * Mat::dot and cv::norm sum in double and return double.
// WHAT THE PIN THEREFORE COVERS: ORBmatcher.cc's own control flow, gates, visiting orders and scalar arithmetic, over this
// project's statement of cv::Mat, Frame / KeyFrame::GetFeaturesInArea (restated from Frame.cc:774-843 / KeyFrame.cc:881-925 in the
// reference's loop order: columns, then rows, then the cell's list), IsInImage, the grid assignment and MapPoint::PredictScale.
// It does NOT cover OpenCV's own bits (gemm accumulation order, MatExpr folding, inv); those stay with tools/pin/run_pin.sh.
#ifndef PLI_MATCH_SHIM_HPP
#define PLI_MATCH_SHIM_HPP
#define MAPPOINT_H
#define KEYFRAME_H
#define FRAME_H
#define CAMERAMODELS_PINHOLE_H
#define CAMERAMODELS_GEOMETRICCAMERA_H
#define TwoViewReconstruction_H

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <set>
#include <vector>
#include "Thirdparty/DBoW2/DBoW2/FeatureVector.h"     // the reference's own

#define CV_8U 0
#define CV_32S 4
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
  float size = 0, angle = -1, response = 0;
  int octave = 0, class_id = -1;
};

class Mat;

// a lazy product / scale / transpose / inverse, evaluated when it becomes a Mat
struct MatExpr {
  enum Kind { SCALE, GEMM, INV, ADD };
  Kind kind = SCALE;
  std::shared_ptr<Mat> a, b, c;      // SCALE: alpha * op(a); GEMM: alpha * op(a) * op(b) + beta * c; INV: inv(a); ADD: a + beta * b
  bool ta = false, tb = false;
  double alpha = 1.0, beta = 1.0;
  MatExpr t() const;
  MatExpr inv() const;
  Mat eval() const;
};

class Mat {
 public:
  int rows = 0, cols = 0, flags = CV_8U;
  size_t step = 0;
  unsigned char* data = nullptr;

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }
  Mat(const MatExpr& e) { *this = e.eval(); }
  Mat& operator=(const MatExpr& e) { *this = e.eval(); return *this; }

  void create(int r, int c, int type) {
    rows = r; cols = c; flags = type;
    step = (size_t)c * elemSize();
    store_ = std::make_shared<std::vector<unsigned char>>((size_t)r * step, (unsigned char)0);
    data = store_->data();
  }
  int type() const { return flags; }
  size_t elemSize() const { return flags == CV_8U ? 1 : 4; }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }

  template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data + (size_t)r * step); }
  template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data + (size_t)r * step); }
  template <class T> T& at(int r, int c) { return *reinterpret_cast<T*>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
  template <class T> const T& at(int r, int c) const { return *reinterpret_cast<const T*>(data + (size_t)r * step + (size_t)c * sizeof(T)); }
  // one index: along the only dimension a vector has
  template <class T> T& at(int i) { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
  template <class T> const T& at(int i) const { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }

  Mat sub(int r0, int r1, int c0, int c1) const {        // a view on the same storage
    Mat m;
    m.rows = r1 - r0; m.cols = c1 - c0; m.flags = flags; m.step = step; m.store_ = store_;
    m.data = data + (size_t)r0 * step + (size_t)c0 * elemSize();
    return m;
  }
  Mat row(int r) const { return sub(r, r + 1, 0, cols); }
  Mat col(int c) const { return sub(0, rows, c, c + 1); }
  Mat rowRange(int r0, int r1) const { return sub(r0, r1, 0, cols); }
  Mat colRange(int c0, int c1) const { return sub(0, rows, c0, c1); }
  Mat clone() const {
    Mat m;
    if (empty()) return m;
    m.create(rows, cols, flags);
    for (int r = 0; r < rows; ++r) std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, (size_t)cols * elemSize());
    return m;
  }
  MatExpr t() const { MatExpr e; e.a = std::make_shared<Mat>(*this); e.ta = true; return e; }
  MatExpr inv() const { MatExpr e; e.kind = MatExpr::INV; e.a = std::make_shared<Mat>(*this); return e; }
  double dot(const Mat& m) const {
    double s = 0.0;
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) s += (double)at<float>(r, c) * (double)m.at<float>(r, c);
    return s;
  }

 private:
  std::shared_ptr<std::vector<unsigned char>> store_;
};

inline double norm(const Mat& m) { return std::sqrt(m.dot(m)); }

inline MatExpr MatExpr::t() const {
  if (kind == SCALE) { MatExpr e = *this; e.ta = !ta; return e; }
  return eval().t();
}
inline MatExpr MatExpr::inv() const { return eval().inv(); }

inline Mat MatExpr::eval() const {
  Mat out;
  if (kind == SCALE) {
    const int R = ta ? a->cols : a->rows, C = ta ? a->rows : a->cols;
    out.create(R, C, CV_32F);
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < C; ++j) {
        const float v = ta ? a->at<float>(j, i) : a->at<float>(i, j);
        out.at<float>(i, j) = alpha == 1.0 ? v : (float)((double)v * alpha);
      }
  } else if (kind == GEMM) {
    const int R = ta ? a->cols : a->rows, K = ta ? a->rows : a->cols, C = tb ? b->rows : b->cols;
    assert(K == (tb ? b->cols : b->rows));
    out.create(R, C, CV_32F);
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < C; ++j) {
        double d = 0.0;
        for (int k = 0; k < K; ++k)
          d += (double)(ta ? a->at<float>(k, i) : a->at<float>(i, k)) * (double)(tb ? b->at<float>(j, k) : b->at<float>(k, j));
        out.at<float>(i, j) = (float)(alpha * d + (c ? beta * (double)c->at<float>(i, j) : 0.0));
      }
  } else if (kind == INV) {
    assert(a->rows == 3 && a->cols == 3);
    double S[9];
    for (int i = 0; i < 9; ++i) S[i] = (double)a->at<float>(i / 3, i % 3);
    out.create(3, 3, CV_32F);
    const double det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (det != 0.0) {
      const double d = 1.0 / det;
      const double co[9] = {S[4] * S[8] - S[5] * S[7], S[2] * S[7] - S[1] * S[8], S[1] * S[5] - S[2] * S[4],
                            S[5] * S[6] - S[3] * S[8], S[0] * S[8] - S[2] * S[6], S[2] * S[3] - S[0] * S[5],
                            S[3] * S[7] - S[4] * S[6], S[1] * S[6] - S[0] * S[7], S[0] * S[4] - S[1] * S[3]};
      for (int i = 0; i < 9; ++i) out.at<float>(i / 3, i % 3) = (float)(co[i] * d);
    }
  } else {
    out.create(a->rows, a->cols, CV_32F);
    for (int i = 0; i < a->rows; ++i)
      for (int j = 0; j < a->cols; ++j)
        out.at<float>(i, j) = beta < 0 ? a->at<float>(i, j) - b->at<float>(i, j) : a->at<float>(i, j) + b->at<float>(i, j);
  }
  return out;
}

namespace shim_detail {
inline MatExpr leaf(const Mat& m) { MatExpr e; e.a = std::make_shared<Mat>(m); return e; }
inline MatExpr flat(const MatExpr& e) { return e.kind == MatExpr::SCALE ? e : leaf(e.eval()); }     // an operand a gemm can take
inline MatExpr mul(const MatExpr& x, const MatExpr& y) {
  const MatExpr l = flat(x), r = flat(y);
  MatExpr e;
  e.kind = MatExpr::GEMM; e.a = l.a; e.ta = l.ta; e.b = r.a; e.tb = r.ta; e.alpha = l.alpha * r.alpha;
  return e;
}
inline MatExpr add(const MatExpr& x, const MatExpr& y, double sign) {
  if (x.kind == MatExpr::GEMM && !x.c) {                          // A * B + C: the addend goes into the gemm
    MatExpr e = x;
    e.c = std::make_shared<Mat>(y.kind == MatExpr::SCALE && !y.ta && y.alpha == 1.0 ? *y.a : y.eval());
    e.beta = sign;
    return e;
  }
  if (sign > 0 && y.kind == MatExpr::GEMM && !y.c) return add(y, x, 1.0);
  MatExpr e;
  e.kind = MatExpr::ADD; e.a = std::make_shared<Mat>(x.eval()); e.b = std::make_shared<Mat>(y.eval()); e.beta = sign;
  return e;
}
inline MatExpr scale(const MatExpr& x, double s) {
  if (x.kind == MatExpr::SCALE || (x.kind == MatExpr::GEMM && !x.c)) { MatExpr e = x; e.alpha *= s; return e; }
  MatExpr e = leaf(x.eval());
  e.alpha = s;
  return e;
}
}  // namespace shim_detail

inline MatExpr operator*(const Mat& x, const Mat& y) { return shim_detail::mul(shim_detail::leaf(x), shim_detail::leaf(y)); }
inline MatExpr operator*(const MatExpr& x, const Mat& y) { return shim_detail::mul(x, shim_detail::leaf(y)); }
inline MatExpr operator*(const Mat& x, const MatExpr& y) { return shim_detail::mul(shim_detail::leaf(x), y); }
inline MatExpr operator*(const MatExpr& x, const MatExpr& y) { return shim_detail::mul(x, y); }
inline MatExpr operator*(double s, const Mat& x) { return shim_detail::scale(shim_detail::leaf(x), s); }
inline MatExpr operator*(double s, const MatExpr& x) { return shim_detail::scale(x, s); }
inline MatExpr operator*(const Mat& x, double s) { return shim_detail::scale(shim_detail::leaf(x), s); }
inline MatExpr operator*(const MatExpr& x, double s) { return shim_detail::scale(x, s); }
inline MatExpr operator/(const Mat& x, double s) { return shim_detail::scale(shim_detail::leaf(x), 1.0 / s); }
inline MatExpr operator/(const MatExpr& x, double s) { return shim_detail::scale(x, 1.0 / s); }
inline MatExpr operator-(const Mat& x) { return shim_detail::scale(shim_detail::leaf(x), -1.0); }
inline MatExpr operator-(const MatExpr& x) { return shim_detail::scale(x, -1.0); }
inline MatExpr operator+(const Mat& x, const Mat& y) { return shim_detail::add(shim_detail::leaf(x), shim_detail::leaf(y), 1.0); }
inline MatExpr operator+(const MatExpr& x, const Mat& y) { return shim_detail::add(x, shim_detail::leaf(y), 1.0); }
inline MatExpr operator+(const Mat& x, const MatExpr& y) { return shim_detail::add(shim_detail::leaf(x), y, 1.0); }
inline MatExpr operator+(const MatExpr& x, const MatExpr& y) { return shim_detail::add(x, y, 1.0); }
inline MatExpr operator-(const Mat& x, const Mat& y) { return shim_detail::add(shim_detail::leaf(x), shim_detail::leaf(y), -1.0); }
inline MatExpr operator-(const MatExpr& x, const Mat& y) { return shim_detail::add(x, shim_detail::leaf(y), -1.0); }
inline MatExpr operator-(const Mat& x, const MatExpr& y) { return shim_detail::add(shim_detail::leaf(x), y, -1.0); }

// Mat_<float>(r, c) << a, b, ...: the comma initialiser
template <class T> class Mat_ : public Mat {
 public:
  Mat_() {}
  Mat_(int r, int c) : Mat(r, c, CV_32F) { static_assert(sizeof(T) == 4, "float matrices only"); }
};
template <class T> struct MatCommaInitializer_ {
  Mat_<T> m;
  int n = 0;
  template <class V> MatCommaInitializer_& operator,(V v) { m.template at<T>(n / m.cols, n % m.cols) = (T)v; ++n; return *this; }
  operator Mat() const { return m; }
  operator Mat_<T>() const { return m; }
};
template <class T, class V> MatCommaInitializer_<T> operator<<(const Mat_<T>& m, V v) {
  MatCommaInitializer_<T> ci;
  ci.m = m;
  return (ci, v);
}

}  // namespace cv

// the few Eigen names Pinhole.cpp mentions
namespace Eigen {
template <class T, int R, int C> struct Matrix {
  T v[R * C] = {};
  T& operator[](int i) { return v[i]; }
  const T& operator[](int i) const { return v[i]; }
  T& operator()(int i, int j) { return v[i * C + j]; }
  const T& operator()(int i, int j) const { return v[i * C + j]; }
};
typedef Matrix<double, 2, 1> Vector2d;
typedef Matrix<double, 3, 1> Vector3d;
}  // namespace Eigen

using namespace std;      // the reference's ORBmatcher.h writes map<>, pair<> and vector<> unqualified (its header chain says this)

namespace ORB_SLAM3 {

class KeyFrame;
class Frame;
class MapPoint;

// Every call Fuse makes on the map is recorded here, in order, when the driver switches recording on.
struct ShimLog {
  enum Op { GET_DESCRIPTOR = 1, GET_MAP_POINT = 2, REPLACE = 3, ADD_OBSERVATION = 4, ADD_MAP_POINT = 5 };
  bool on = false;
  std::vector<int32_t> ops;                      // triples: op, first index, second index
  void put(int op, int a, int b) { if (on) { ops.push_back(op); ops.push_back(a); ops.push_back(b); } }
  static ShimLog& get() { static ShimLog l; return l; }
};

class TwoViewReconstruction {
 public:
  explicit TwoViewReconstruction(const cv::Mat&) {}
  bool Reconstruct(const std::vector<cv::KeyPoint>&, const std::vector<cv::KeyPoint>&, const std::vector<int>&, cv::Mat&, cv::Mat&,
                   std::vector<cv::Point3f>&, std::vector<bool>&) { return false; }
};

class GeometricCamera {
 public:
  GeometricCamera() {}
  GeometricCamera(const std::vector<float>& _vParameters) : mvParameters(_vParameters) {}
  virtual ~GeometricCamera() {}
  virtual cv::Point2f project(const cv::Point3f& p3D) = 0;
  virtual cv::Point2f project(const cv::Mat& m3D) = 0;
  virtual cv::Mat toK() = 0;
  virtual bool epipolarConstrain(GeometricCamera* otherCamera, const cv::KeyPoint& kp1, const cv::KeyPoint& kp2, const cv::Mat& R12,
                                 const cv::Mat& t12, const float sigmaLevel, const float unc) = 0;
  // (only the SearchForTriangulation overload that is out of scope calls this)
  virtual bool matchAndtriangulate(const cv::KeyPoint&, const cv::KeyPoint&, GeometricCamera*, cv::Mat&, cv::Mat&, const float, const float,
                                   cv::Mat&) { return false; }
  static long unsigned int nNextId;

 protected:
  std::vector<float> mvParameters;
  unsigned int mnId = 0, mnType = 0;
};

// exactly the members src/CameraModels/Pinhole.cpp defines (each needs its declaration to compile); the bodies come from that file
class Pinhole : public GeometricCamera {
 public:
  Pinhole(const std::vector<float> _vParameters) : GeometricCamera(_vParameters), tvr(nullptr) {}
  cv::Point2f project(const cv::Point3f& p3D);
  cv::Point2f project(const cv::Mat& m3D);
  Eigen::Vector2d project(const Eigen::Vector3d& v3D);
  cv::Mat projectMat(const cv::Point3f& p3D);
  float uncertainty2(const Eigen::Matrix<double, 2, 1>& p2D);
  cv::Point3f unproject(const cv::Point2f& p2D);
  cv::Mat unprojectMat(const cv::Point2f& p2D);
  cv::Mat projectJac(const cv::Point3f& p3D);
  Eigen::Matrix<double, 2, 3> projectJac(const Eigen::Vector3d& v3D);
  cv::Mat unprojectJac(const cv::Point2f& p2D);
  bool ReconstructWithTwoViews(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2,
                               const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                               std::vector<bool>& vbTriangulated);
  cv::Mat toK();
  bool epipolarConstrain(GeometricCamera* pCamera2, const cv::KeyPoint& kp1, const cv::KeyPoint& kp2, const cv::Mat& R12,
                         const cv::Mat& t12, const float sigmaLevel, const float unc);
  friend std::ostream& operator<<(std::ostream& os, const Pinhole& ph);
  friend std::istream& operator>>(std::istream& os, Pinhole& ph);

 private:
  cv::Mat SkewSymmetricMatrix(const cv::Mat& v);
  TwoViewReconstruction* tvr;
};

// What Frame and KeyFrame share here: the tables, the 64 x 48 grid (Frame::AssignFeaturesToGrid / PosInGrid, Frame.cc:845-855: the
// cell is round() of the float product, features in index order) and the window walk of GetFeaturesInArea.
class ShimTable {
 public:
  static const int GRID_COLS = 64, GRID_ROWS = 48;
  int index = 0;                                  // the driver's number of this object
  int N = 0;
  std::vector<cv::KeyPoint> mvKeys, mvKeysUn, mvKeysRight;
  std::vector<float> mvuRight;
  cv::Mat mDescriptors;
  DBoW2::FeatureVector mFeatVec;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
  float mfLogScaleFactor = 0;
  int mnScaleLevels = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
  float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
  GeometricCamera *mpCamera = nullptr, *mpCamera2 = nullptr;
  std::vector<int> mvLeftToRightMatch, mvRightToLeftMatch;
  cv::Mat mTcw, mTrl, mRcw, mtcw, mOw;
  std::vector<size_t> mGrid[GRID_COLS][GRID_ROWS];

  void AssignFeaturesToGrid() {
    mfGridElementWidthInv = static_cast<float>(GRID_COLS) / static_cast<float>(mnMaxX - mnMinX);
    mfGridElementHeightInv = static_cast<float>(GRID_ROWS) / static_cast<float>(mnMaxY - mnMinY);
    for (int i = 0; i < N; ++i) {
      const int px = (int)std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv);
      const int py = (int)std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
      if (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) continue;
      mGrid[px][py].push_back((size_t)i);
    }
  }
  bool IsInImage(const float& x, const float& y) const { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }

 protected:
  // levels: Frame's test (Frame.cc:809-831); KeyFrame's walk has none
  std::vector<size_t> area(float x, float y, float r, bool levels, int minLevel, int maxLevel) const {
    std::vector<size_t> vIndices;
    const int c0 = std::max(0, (int)std::floor((x - mnMinX - r) * mfGridElementWidthInv));
    if (c0 >= GRID_COLS) return vIndices;
    const int c1 = std::min(GRID_COLS - 1, (int)std::ceil((x - mnMinX + r) * mfGridElementWidthInv));
    if (c1 < 0) return vIndices;
    const int r0 = std::max(0, (int)std::floor((y - mnMinY - r) * mfGridElementHeightInv));
    if (r0 >= GRID_ROWS) return vIndices;
    const int r1 = std::min(GRID_ROWS - 1, (int)std::ceil((y - mnMinY + r) * mfGridElementHeightInv));
    if (r1 < 0) return vIndices;
    const bool check = levels && (minLevel > 0 || maxLevel >= 0);
    for (int ix = c0; ix <= c1; ++ix)
      for (int iy = r0; iy <= r1; ++iy)
        for (size_t j : mGrid[ix][iy]) {
          const cv::KeyPoint& kp = mvKeysUn[j];
          if (check) {
            if (kp.octave < minLevel) continue;
            if (maxLevel >= 0 && kp.octave > maxLevel) continue;
          }
          const float dx = kp.pt.x - x, dy = kp.pt.y - y;
          if (std::fabs(dx) < r && std::fabs(dy) < r) vIndices.push_back(j);
        }
    return vIndices;
  }
};

class Frame : public ShimTable {
 public:
  int Nleft = -1;
  std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const int minLevel = -1, const int maxLevel = -1,
                                        const bool bRight = false) const {
    assert(!bRight);
    return area(x, y, r, true, minLevel, maxLevel);
  }
};

class KeyFrame : public ShimTable {
 public:
  int NLeft = -1;
  std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const bool bRight = false) const {
    assert(!bRight);
    return area(x, y, r, false, -1, -1);
  }
  cv::Mat GetPose() { return mTcw.clone(); }
  cv::Mat GetRotation() { return mRcw.clone(); }
  cv::Mat GetTranslation() { return mtcw.clone(); }
  cv::Mat GetCameraCenter() { return mOw.clone(); }
  cv::Mat GetRightPose() { return cv::Mat(); }
  cv::Mat GetRightRotation() { return cv::Mat(); }
  cv::Mat GetRightTranslation() { return cv::Mat(); }
  cv::Mat GetRightCameraCenter() { return cv::Mat(); }
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  std::set<MapPoint*> GetMapPoints();
  MapPoint* GetMapPoint(const size_t& idx);
  void AddMapPoint(MapPoint* pMP, const size_t& idx);
};

class MapPoint {
 public:
  int index = 0;                                  // the driver's number of this object
  cv::Mat mWorldPos, mNormalVector, mDescriptor;
  bool mbBad = false;
  float mMinDistInv = 0, mMaxDistInv = 0, mfMaxDistance = 0;      // the invariance bounds are stored as the getters return them
  int nObs = 0;
  std::map<KeyFrame*, int> mObservations;

  bool mbTrackInView = false, mbTrackInViewR = false;
  float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackProjYR = 0, mTrackDepth = 0, mTrackDepthR = 0;
  int mnTrackScaleLevel = 0, mnTrackScaleLevelR = 0;
  float mTrackViewCos = 0, mTrackViewCosR = 0;

  cv::Mat GetWorldPos() { return mWorldPos.clone(); }
  cv::Mat GetNormal() { return mNormalVector.clone(); }
  cv::Mat GetDescriptor() { ShimLog::get().put(ShimLog::GET_DESCRIPTOR, index, 0); return mDescriptor.clone(); }
  bool isBad() { return mbBad; }
  float GetMinDistanceInvariance() { return mMinDistInv; }
  float GetMaxDistanceInvariance() { return mMaxDistInv; }
  int Observations() { return nObs; }
  bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
  int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? mObservations[pKF] : -1; }
  void AddObservation(KeyFrame* pKF, size_t idx) {
    ShimLog::get().put(ShimLog::ADD_OBSERVATION, index, (int)idx);
    if (!mObservations.count(pKF)) { mObservations[pKF] = (int)idx; ++nObs; }
  }
  void Replace(MapPoint* pMP) { ShimLog::get().put(ShimLog::REPLACE, index, pMP->index); }
  // MapPoint::PredictScale (MapPoint.cc:449-481) by this project's statement of it (tests/test_fuse_search_cpu.py: predict_scale):
  // the float ratio, its logarithm in double, divided by the float log of the scale factor
  template <class T> int PredictScale(const float& currentDist, T* pT) {
    const float ratio = mfMaxDistance / currentDist;
    if (!(ratio > 0.0f)) return 0;
    if (std::isinf(ratio)) return pT->mnScaleLevels - 1;
    const double n = std::ceil(std::log((double)ratio) / (double)pT->mfLogScaleFactor);
    return n < 0 ? 0 : n >= pT->mnScaleLevels ? pT->mnScaleLevels - 1 : (int)n;
  }
};

inline std::set<MapPoint*> KeyFrame::GetMapPoints() {
  std::set<MapPoint*> s;
  for (MapPoint* p : mvpMapPoints)
    if (p && !p->isBad()) s.insert(p);
  return s;
}
inline MapPoint* KeyFrame::GetMapPoint(const size_t& idx) {
  ShimLog::get().put(ShimLog::GET_MAP_POINT, index, (int)idx);
  return mvpMapPoints[idx];
}
inline void KeyFrame::AddMapPoint(MapPoint* pMP, const size_t& idx) {
  ShimLog::get().put(ShimLog::ADD_MAP_POINT, pMP->index, (int)idx);
  mvpMapPoints[idx] = pMP;
}

}  // namespace ORB_SLAM3
#endif
