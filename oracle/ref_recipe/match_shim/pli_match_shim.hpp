// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for everything the reference's src/ORBmatcher.cc (and src/CameraModels/Pinhole.cpp, src/CameraModels/KannalaBrandt8.cpp)
// reaches through its headers, written for this project.  oracle/Makefile force-includes this file (-include) in front of those
// sources, which are compiled where they lie, unmodified.  It predefines the include guards of the reference's MapPoint.h, KeyFrame.h,
// Frame.h, Pinhole.h, KannalaBrandt8.h, GeometricCamera.h and TwoViewReconstruction.h, so that those headers (and OpenCV, Eigen, g2o, Sophus, boost behind them) stay
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
//   * s * Mat - Mat (KannalaBrandt8::Triangulate) is (float)(x * s) and then a float subtraction per element.
//   * cv::SVD::compute (4 x 4 CV_32F), cv::hconcat, Mat::eye and the Mat / s of the two-camera functions (a float factor, see
//     shim_detail::divisionFactorInFloat) are THIS PROJECT'S STATEMENT of OpenCV too, the same as oracle/match_oracle.hpp's.
//   * An expression assigned to a matrix of its own size and type fills that storage (A.row(0) = ...), as OpenCV's does.
// WHAT THE PIN THEREFORE COVERS: ORBmatcher.cc's own control flow, gates, visiting orders and scalar arithmetic, over this
// project's statement of cv::Mat, Frame / KeyFrame::GetFeaturesInArea (restated from Frame.cc:774-843 / KeyFrame.cc:881-925 in the
// reference's loop order: columns, then rows, then the cell's list), IsInImage, the grid assignment and MapPoint::PredictScale.
// For KannalaBrandt8.cpp: its own float arithmetic, gates and the overloads its libm calls select.  Two-camera tables (NLeft != -1):
// KeyFrame's right-pose getters are restated from KeyFrame.cc:1290-1373, KeyFrame::GetFeaturesInArea(..., bRight) from
// KeyFrame.cc:881-925 and Frame::GetFeaturesInArea(..., bRight) from Frame.cc:774-843, both over the two grids of Frame.cc:468-481.
// Driven for two cameras: SearchForTriangulation, SearchByBoW, Fuse and both frame SearchByProjection forms (the frame-to-frame one
// with a one-camera last frame).
// It does NOT cover OpenCV's own bits (gemm accumulation order, MatExpr folding, inv, the SVD); those stay with tools/pin/run_pin.sh.
#ifndef PLI_MATCH_SHIM_HPP
#define PLI_MATCH_SHIM_HPP
#define MAPPOINT_H
#define KEYFRAME_H
#define FRAME_H
#define CAMERAMODELS_PINHOLE_H
#define CAMERAMODELS_KANNALABRANDT8_H
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
#define CV_PI 3.1415926535897932384626433832795

// STANDARD MATH HEADERS.  OpenCV 3.3.1's core.hpp reaches <cmath> (cvdef.h -> fast_math.hpp) and no <math.h>; this file
// includes <cmath> and no <math.h> either.  That decides which overload an unqualified cos(float) in the reference's
// KannalaBrandt8.cpp selects: with <cmath> alone the global namespace holds only the C functions, so cos(float) is cos(double).
// The `using namespace std;` below would add the float overloads, and the header chain of KannalaBrandt8.cpp has none, so
// oracle/Makefile compiles that one file with -DPLI_MATCH_SHIM_NO_USING_STD.

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

namespace shim_detail {
// Mat / s.  This project holds two statements of it: (float)(x * (1.0 / s)) in double (the convention above, which the Sim3 searches
// of ORBmatcher.cc are pinned over), and x * (float)(1.0 / s) + 0.f in float (oracle/match_oracle.hpp: kb8TriangulateMatches,
// after convertTo's float work type for CV_32F).  The driver switches the second on for the two-camera functions, whose only
// division is the one in KannalaBrandt8::Triangulate; the single-camera cases keep the first.
inline bool& divisionFactorInFloat() { static bool on = false; return on; }
}  // namespace shim_detail

// a lazy product / scale / transpose / inverse, evaluated when it becomes a Mat
struct MatExpr {
  enum Kind { SCALE, GEMM, INV, ADD };
  Kind kind = SCALE;
  std::shared_ptr<Mat> a, b, c;      // SCALE: alpha * op(a); GEMM: alpha * op(a) * op(b) + beta * c; INV: inv(a); ADD: a + beta * b
  bool ta = false, tb = false, division = false;
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
  // an expression assigned to a matrix of its own size and type is written into that storage (A.row(0) = ... fills A)
  Mat& operator=(const MatExpr& e);
  static MatExpr eye(int r, int c, int type);

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
  // into a matrix or a view of this one's size and type (Rcw.copyTo(Tcw.colRange(0, 3)))
  void copyTo(Mat m) const {
    assert(m.data && m.rows == rows && m.cols == cols && m.flags == flags);
    for (int r = 0; r < rows; ++r) std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, (size_t)cols * elemSize());
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

inline Mat& Mat::operator=(const MatExpr& e) {
  const Mat v = e.eval();
  if (data && rows == v.rows && cols == v.cols && flags == v.flags) {
    for (int r = 0; r < rows; ++r) std::memcpy(data + (size_t)r * step, v.data + (size_t)r * v.step, (size_t)cols * elemSize());
  } else {
    *this = v;
  }
  return *this;
}

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
        if (division && shim_detail::divisionFactorInFloat()) out.at<float>(i, j) = v * (float)alpha + 0.f;
        else out.at<float>(i, j) = alpha == 1.0 ? v : (float)((double)v * alpha);
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
inline MatExpr operator/(const Mat& x, double s) { MatExpr e = shim_detail::scale(shim_detail::leaf(x), 1.0 / s); e.division = true; return e; }
inline MatExpr operator/(const MatExpr& x, double s) { MatExpr e = shim_detail::scale(x, 1.0 / s); e.division = e.kind == MatExpr::SCALE; return e; }
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

inline MatExpr Mat::eye(int r, int c, int type) {
  assert(type == CV_32F);
  Mat m(r, c, type);
  for (int i = 0; i < std::min(r, c); ++i) m.at<float>(i, i) = 1.f;
  return shim_detail::leaf(m);
}

// cv::hconcat of two CV_32F matrices with equal rows
inline void hconcat(const Mat& a, const Mat& b, Mat& dst) {
  assert(a.rows == b.rows && a.type() == CV_32F && b.type() == CV_32F);
  Mat m(a.rows, a.cols + b.cols, CV_32F);
  for (int r = 0; r < a.rows; ++r) {
    for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = a.at<float>(r, c);
    for (int c = 0; c < b.cols; ++c) m.at<float>(r, a.cols + c) = b.at<float>(r, c);
  }
  dst = m;
}

inline std::ostream& operator<<(std::ostream& os, const Mat& m) {
  for (int r = 0; r < m.rows; ++r)
    for (int c = 0; c < m.cols; ++c) os << (c ? ", " : r ? "; " : "[") << m.at<float>(r, c);
  return os << "]";
}

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4 x 4 CV_32F matrix only: THIS PROJECT'S STATEMENT of OpenCV 3.3.1's
// one-sided Jacobi (lapack.cpp: JacobiSVDImpl_<float> on the transposed matrix; eps = 2 * FLT_EPSILON, at most 30 sweeps, the
// rotations in float, norms and dot products in double, hypot(p, beta) as sqrt(p * p + beta * beta) in double, rows sorted by
// singular value), the same statement as oracle/match_oracle.hpp: jacobiSvdLastVt4.  w and vt are filled; u is left empty (the
// only caller, KannalaBrandt8::Triangulate, reads vt alone).
struct SVD {
  enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };
  static void compute(const Mat& A, Mat& w, Mat& u, Mat& vt, int flags = 0) {
    if (A.rows != 4 || A.cols != 4 || A.type() != CV_32F || flags != (MODIFY_A | FULL_UV)) {
      std::cerr << "match_shim: cv::SVD::compute is stated for 4 x 4 CV_32F with MODIFY_A | FULL_UV only" << std::endl;
      std::abort();
    }
    const int n = 4;
    float At[4][4], Vt[4][4];
    double W[4];
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k) At[i][k] = A.at<float>(k, i);
    const float eps = 1.1920928955078125e-07f * 2;
    for (int i = 0; i < n; ++i) {
      double sd = 0;
      for (int k = 0; k < n; ++k) { const float t = At[i][k]; sd += (double)t * t; }
      W[i] = sd;
      for (int k = 0; k < n; ++k) Vt[i][k] = i == k ? 1.f : 0.f;
    }
    for (int iter = 0; iter < 30; ++iter) {
      bool changed = false;
      for (int i = 0; i < n - 1; ++i)
        for (int j = i + 1; j < n; ++j) {
          float *Ai = At[i], *Aj = At[j];
          double a = W[i], p = 0, b = W[j];
          for (int k = 0; k < n; ++k) p += (double)Ai[k] * Aj[k];
          if (std::fabs(p) <= (double)eps * std::sqrt(a * b)) continue;
          p *= 2;
          const double beta = a - b, gamma = std::sqrt(p * p + beta * beta);
          float c, s;
          if (beta < 0) {
            const double delta = (gamma - beta) * 0.5;
            s = (float)std::sqrt(delta / gamma);
            c = (float)(p / (gamma * s * 2));
          } else {
            c = (float)std::sqrt((gamma + beta) / (gamma * 2));
            s = (float)(p / (gamma * c * 2));
          }
          a = b = 0;
          for (int k = 0; k < n; ++k) {
            const float t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
            Ai[k] = t0; Aj[k] = t1;
            a += (double)t0 * t0; b += (double)t1 * t1;
          }
          W[i] = a; W[j] = b;
          changed = true;
          float *Vi = Vt[i], *Vj = Vt[j];
          for (int k = 0; k < n; ++k) {
            const float t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k];
            Vi[k] = t0; Vj[k] = t1;
          }
        }
      if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
      double sd = 0;
      for (int k = 0; k < n; ++k) { const float t = At[i][k]; sd += (double)t * t; }
      W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; ++i) {
      int j = i;
      for (int k = i + 1; k < n; ++k)
        if (W[j] < W[k]) j = k;
      if (i != j) {
        std::swap(W[i], W[j]);
        for (int k = 0; k < n; ++k) { std::swap(At[i][k], At[j][k]); std::swap(Vt[i][k], Vt[j][k]); }
      }
    }
    Mat wm(4, 1, CV_32F), vm(4, 4, CV_32F);
    for (int i = 0; i < n; ++i) {
      wm.at<float>(i, 0) = (float)W[i];
      for (int k = 0; k < n; ++k) vm.at<float>(i, k) = Vt[i][k];
    }
    w = wm; vt = vm; u = Mat();
  }
};

// declared for KannalaBrandt8::ReconstructWithTwoViews, which no case reaches
namespace fisheye {
inline void undistortPoints(const std::vector<Point2f>&, std::vector<Point2f>&, const Mat&, const Mat&, const Mat&, const Mat&) {
  std::cerr << "match_shim: cv::fisheye::undistortPoints has no stand-in" << std::endl;
  std::abort();
}
}  // namespace fisheye

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

#ifndef PLI_MATCH_SHIM_NO_USING_STD
using namespace std;      // the reference's ORBmatcher.h writes map<>, pair<> and vector<> unqualified (its header chain says this)
#endif

// HOOKS for a stand-in that includes this one (map_shim/pli_map_shim.hpp, which compiles definitions cut out of the reference's
// MapPoint.cc, MapLine.cc, Frame.cc, LocalMapping.cc and KeyFrame.cc next to ORBmatcher.cc): members added to the three classes, the value type of
// MapPoint::mObservations, and PLI_SHIM_MAPPOINT_OWN_SCALE, under which GetMinDistanceInvariance, GetMaxDistanceInvariance and
// PredictScale(dist, Frame*) are only declared, because the reference's own definitions are linked in.  All unset here: ref_match
// and its fixtures see the text they always saw.
#ifndef PLI_SHIM_OBSERVATION_T
#define PLI_SHIM_OBSERVATION_T int
#endif
#ifndef PLI_SHIM_MAPPOINT_EXTRA
#define PLI_SHIM_MAPPOINT_EXTRA
#endif
#ifndef PLI_SHIM_KEYFRAME_EXTRA
#define PLI_SHIM_KEYFRAME_EXTRA
#endif
#ifndef PLI_SHIM_FRAME_EXTRA
#define PLI_SHIM_FRAME_EXTRA
#endif

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
  virtual cv::Point3f unproject(const cv::Point2f& p2D) = 0;
  virtual cv::Mat unprojectMat(const cv::Point2f& p2D) = 0;
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

// exactly the members src/CameraModels/KannalaBrandt8.cpp defines, as include/CameraModels/KannalaBrandt8.h declares them (without
// the serialisation); the bodies come from that file.  precision is the header's 1e-6.
class KannalaBrandt8 final : public GeometricCamera {
 public:
  KannalaBrandt8(const std::vector<float> _vParameters) : GeometricCamera(_vParameters), mvLappingArea(2, 0), precision(1e-6), tvr(nullptr) {
    assert(mvParameters.size() == 8);
  }
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
  float TriangulateMatches(GeometricCamera* pCamera2, const cv::KeyPoint& kp1, const cv::KeyPoint& kp2, const cv::Mat& R12,
                           const cv::Mat& t12, const float sigmaLevel, const float unc, cv::Mat& p3D);
  std::vector<int> mvLappingArea;
  bool matchAndtriangulate(const cv::KeyPoint& kp1, const cv::KeyPoint& kp2, GeometricCamera* pOther, cv::Mat& Tcw1, cv::Mat& Tcw2,
                           const float sigmaLevel1, const float sigmaLevel2, cv::Mat& x3Dtriangulated);
  friend std::ostream& operator<<(std::ostream& os, const KannalaBrandt8& kb);
  friend std::istream& operator>>(std::istream& is, KannalaBrandt8& kb);

 private:
  const float precision;
  TwoViewReconstruction* tvr;
  void Triangulate(const cv::Point2f& p1, const cv::Point2f& p2, const cv::Mat& Tcw1, const cv::Mat& Tcw2, cv::Mat& x3D);
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
  cv::Mat mTcw, mTrl, mTlr, mRcw, mtcw, mOw;      // mTlr: 3 x 4, the right camera's pose in the left one (two-camera tables only)
  std::vector<size_t> mGrid[GRID_COLS][GRID_ROWS], mGridRight[GRID_COLS][GRID_ROWS];
  int nLeftRows = -1;                             // Nleft / NLeft of a two-camera table (mvKeys holds that many rows), -1 otherwise

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
  // Frame::AssignFeaturesToGrid for a two-camera frame (Frame.cc:468-481): row i < Nleft is mvKeys[i] and goes to mGrid as i, the
  // others are mvKeysRight[i - Nleft] and go to mGridRight under their camera-local index
  void AssignFeaturesToGridTwoCameras(int nleft) {
    nLeftRows = nleft;
    mfGridElementWidthInv = static_cast<float>(GRID_COLS) / static_cast<float>(mnMaxX - mnMinX);
    mfGridElementHeightInv = static_cast<float>(GRID_ROWS) / static_cast<float>(mnMaxY - mnMinY);
    for (int i = 0; i < N; ++i) {
      const cv::KeyPoint& kp = i < nleft ? mvKeys[(size_t)i] : mvKeysRight[(size_t)(i - nleft)];
      const int px = (int)std::round((kp.pt.x - mnMinX) * mfGridElementWidthInv);
      const int py = (int)std::round((kp.pt.y - mnMinY) * mfGridElementHeightInv);
      if (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) continue;
      if (i < nleft) mGrid[px][py].push_back((size_t)i);
      else mGridRight[px][py].push_back((size_t)(i - nleft));
    }
  }
  bool IsInImage(const float& x, const float& y) const { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }

 protected:
  // levels: Frame's test (Frame.cc:809-831); KeyFrame's walk has none
  // bRight (KeyFrame.cc:909-914): the cell lists of mGridRight, the keypoints of mvKeysRight, camera-local indices
  std::vector<size_t> area(float x, float y, float r, bool levels, int minLevel, int maxLevel, bool bRight = false) const {
    const std::vector<cv::KeyPoint>& keys = bRight ? mvKeysRight : nLeftRows >= 0 ? mvKeys : mvKeysUn;
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
        for (size_t j : (bRight ? mGridRight[ix][iy] : mGrid[ix][iy])) {
          const cv::KeyPoint& kp = keys[j];
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
                                        const bool bRight = false) const {      // Frame.cc:774-843
    return area(x, y, r, true, minLevel, maxLevel, bRight);
  }
  PLI_SHIM_FRAME_EXTRA
};

class KeyFrame : public ShimTable {
 public:
  int NLeft = -1;
  std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const bool bRight = false) const {   // KeyFrame.cc:881-925
    return area(x, y, r, false, -1, -1, bRight);
  }
  cv::Mat GetPose() { return mTcw.clone(); }
  cv::Mat GetRotation() { return mRcw.clone(); }
  cv::Mat GetTranslation() { return mtcw.clone(); }
  cv::Mat GetCameraCenter() { return mOw.clone(); }
  // KeyFrame.cc:1290-1373 restated over mRcw / mtcw / mOw (the reference reads the same blocks out of Tcw and Ow); empty without a
  // second camera, as before
  cv::Mat GetRightRotation() {                              // KeyFrame.cc:1354-1362
    if (mTlr.empty()) return cv::Mat();
    cv::Mat Rrl = mTlr.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat Rlw = mRcw.clone();
    cv::Mat Rrw = Rrl * Rlw;
    return Rrw.clone();
  }
  cv::Mat GetRightTranslation() {                           // KeyFrame.cc:1364-1373
    if (mTlr.empty()) return cv::Mat();
    cv::Mat Rrl = mTlr.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat tlw = mtcw.clone();
    cv::Mat trl = -Rrl * mTlr.rowRange(0, 3).col(3);
    cv::Mat trw = Rrl * tlw + trl;
    return trw.clone();
  }
  cv::Mat GetRightPose() {                                  // KeyFrame.cc:1290-1303
    if (mTlr.empty()) return cv::Mat();
    cv::Mat Trw;
    cv::hconcat(GetRightRotation(), GetRightTranslation(), Trw);
    return Trw.clone();
  }
  cv::Mat GetRightCameraCenter() {                          // KeyFrame.cc:1343-1352
    if (mTlr.empty()) return cv::Mat();
    cv::Mat Rwl = mRcw.t();
    cv::Mat tlr = mTlr.rowRange(0, 3).col(3);
    cv::Mat twl = mOw.clone();
    cv::Mat twr = Rwl * tlr + twl;
    return twr.clone();
  }
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  std::set<MapPoint*> GetMapPoints();
  MapPoint* GetMapPoint(const size_t& idx);
  void AddMapPoint(MapPoint* pMP, const size_t& idx);
  PLI_SHIM_KEYFRAME_EXTRA
};

class MapPoint {
 public:
  int index = 0;                                  // the driver's number of this object
  cv::Mat mWorldPos, mNormalVector, mDescriptor;
  bool mbBad = false;
  float mMinDistInv = 0, mMaxDistInv = 0, mfMaxDistance = 0;      // the invariance bounds are stored as the getters return them
  int nObs = 0;
  std::map<KeyFrame*, PLI_SHIM_OBSERVATION_T> mObservations;
  PLI_SHIM_MAPPOINT_EXTRA

  bool mbTrackInView = false, mbTrackInViewR = false;
  float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackProjYR = 0, mTrackDepth = 0, mTrackDepthR = 0;
  int mnTrackScaleLevel = 0, mnTrackScaleLevelR = 0;
  float mTrackViewCos = 0, mTrackViewCosR = 0;

  cv::Mat GetWorldPos() { return mWorldPos.clone(); }
  cv::Mat GetNormal() { return mNormalVector.clone(); }
  cv::Mat GetDescriptor() { ShimLog::get().put(ShimLog::GET_DESCRIPTOR, index, 0); return mDescriptor.clone(); }
  bool isBad() { return mbBad; }
#ifdef PLI_SHIM_MAPPOINT_OWN_SCALE
  float GetMinDistanceInvariance();
  float GetMaxDistanceInvariance();
  int PredictScale(const float& currentDist, Frame* pF);
#else
  float GetMinDistanceInvariance() { return mMinDistInv; }
  float GetMaxDistanceInvariance() { return mMaxDistInv; }
#endif
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
