// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-in for what the definitions oracle/Makefile (ref_map) cuts out of the reference's src/Frame.cc, src/MapPoint.cc,
// src/MapLine.cc, src/LocalMapping.cc and src/KeyFrame.cc reach through their headers, written for this project.  It includes the matcher's stand-in
// (match_shim/pli_match_shim.hpp: cv::Mat and its ARITHMETIC CONVENTION, stated once there, both camera models, Frame, KeyFrame,
// MapPoint) and adds, through that file's hooks, only what the cut definitions touch:
//   Frame     declarations of isInFrustum and isInFrustum_l (the bodies are the reference's) and of isInFrustumChecks (the driver's:
//             it aborts; only a two-camera frame reaches it)
//   KeyFrame  isBad() over a flag the driver sets, mDescriptors_l; for CreateNewMapPoints: GetBestCovisibilityKeyFrames (the case's
//             list), mPrevKF, mvDepth, invfx / invfy, mfScaleFactor, Twc and its mutex, GetMap, ComputeSceneMedianDepth (a value the
//             driver sets), a declaration of UnprojectStereo (the reference's)
//   LocalMapping, Atlas, Map, Tracking   the members CreateNewMapPoints reads; CheckNewKeyFrames() answers false
//   MapPoint  a constructor (position, reference keyframe, map), an empty UpdateNormalAndDepth (it is not on the device), the two
//             mutexes the reference locks, mfMinDistance, mObservations with the reference's value type (size_t), and
//             declarations of GetMinDistanceInvariance, GetMaxDistanceInvariance and PredictScale(dist, Frame*), whose bodies are
//             the reference's here (ORBmatcher.cc's PredictScale(dist, KeyFrame*) stays the matcher stand-in's restatement)
//   MapLine   the members isInFrustum_l and MapLine::ComputeDistinctiveDescriptors touch
//   Vector6d with head(3) / tail(3), Converter::toCvMat(Vector3d) (Converter.cc:90-97: one float conversion per element),
//   cv::norm(a, b, NORM_HAMMING) of two CV_8U rows (the number of differing bits)
// Keyframes of two KannalaBrandt8 cameras (the branch LocalMapping.cc:463-528) need nothing more: mpCamera2, NLeft, mvKeysRight, mTlr
// and the right-pose getters are the matcher stand-in's.
// WHAT THE PIN COVERS: the control flow, gates, orders and scalar arithmetic of the cut definitions and which libm overloads they
// select (log of a float under `using namespace std` is logf).  It does not cover OpenCV's own gemm, norm and dot (stated in the
// matcher's stand-in), nor anything the cut text only calls.
#ifndef PLI_MAP_SHIM_HPP
#define PLI_MAP_SHIM_HPP
#define MAPLINE_H
#define CONVERTER_H

#include <climits>
#include <list>
#include <mutex>

namespace ORB_SLAM3 { class MapLine; class Map; class KeyFrame; }

#define PLI_SHIM_OBSERVATION_T size_t
#define PLI_SHIM_MAPPOINT_OWN_SCALE
#define PLI_SHIM_MAPPOINT_EXTRA                                                                               \
  std::mutex mMutexFeatures, mMutexPos;                                                                       \
  float mfMinDistance = 0;                                                                                    \
  bool mbSeenInFrame = false;                                                                                 \
  KeyFrame* mpRefKF = nullptr;                                                                                \
  MapPoint() {}                                                                                               \
  MapPoint(const cv::Mat& Pos, KeyFrame* pRefKF, Map*) : mpRefKF(pRefKF) { mWorldPos = Pos.clone(); }         \
  void ComputeDistinctiveDescriptors();                                                                       \
  void UpdateNormalAndDepth() {} /* (not on the device) */
#define PLI_SHIM_KEYFRAME_EXTRA                                                                               \
  bool mbBad = false;                                                                                         \
  bool isBad() { return mbBad; }                                                                              \
  cv::Mat mDescriptors_l, Twc;                                                                                \
  std::mutex mMutexPose;                                                                                      \
  KeyFrame* mPrevKF = nullptr;                                                                                \
  Map* mpMap = nullptr;                                                                                       \
  std::vector<KeyFrame*> mvpNeighbours; /* what GetBestCovisibilityKeyFrames answers, in the case's order */  \
  std::vector<float> mvDepth;                                                                                 \
  float invfx = 0, invfy = 0, mfScaleFactor = 0, mSceneMedianDepth = 0;                                       \
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) { return mvpNeighbours; }                   \
  Map* GetMap() { return mpMap; }                                                                             \
  float ComputeSceneMedianDepth(const int) { return mSceneMedianDepth; }                                      \
  cv::Mat UnprojectStereo(int i); /* the reference's */
#define PLI_SHIM_FRAME_EXTRA                                    \
  bool isInFrustum(MapPoint* pMP, float viewingCosLimit);       \
  bool isInFrustum_l(MapLine* pML, float viewingCosLimit);      \
  bool isInFrustumChecks(MapPoint* pMP, float viewingCosLimit, bool bRight = false);
#include "../match_shim/pli_match_shim.hpp"

namespace cv {
enum { NORM_HAMMING = 6 };
inline double norm(const Mat& a, const Mat& b, int normType) {
  if (normType != NORM_HAMMING || a.type() != CV_8U || b.type() != CV_8U || a.rows != 1 || b.rows != 1 || a.cols != b.cols) {
    std::cerr << "map_shim: cv::norm(a, b, type) is stated for NORM_HAMMING of two CV_8U rows only" << std::endl;
    std::abort();
  }
  int bits = 0;
  for (int i = 0; i < a.cols; ++i) bits += __builtin_popcount((unsigned)(a.data[i] ^ b.data[i]));
  return (double)bits;
}
}  // namespace cv
using cv::NORM_HAMMING;      // (the reference's KeyFrame.h says `using namespace cv;`)

namespace Eigen {
// a 6-vector that gives its halves away: all MapLine::GetWorldPos's caller asks of it
template <> struct Matrix<double, 6, 1> {
  double v[6] = {};
  double& operator[](int i) { return v[i]; }
  const double& operator[](int i) const { return v[i]; }
  Matrix<double, 3, 1> head(int n) const { assert(n == 3); Matrix<double, 3, 1> m; for (int i = 0; i < 3; ++i) m[i] = v[i]; return m; }
  Matrix<double, 3, 1> tail(int n) const { assert(n == 3); Matrix<double, 3, 1> m; for (int i = 0; i < 3; ++i) m[i] = v[3 + i]; return m; }
};
}  // namespace Eigen
using namespace Eigen;       // (the reference's Frame.h and MapLine.h say this)
typedef Eigen::Matrix<double, 6, 1> Vector6d;

namespace ORB_SLAM3 {

class Converter {
 public:
  static cv::Mat toCvMat(const Eigen::Matrix<double, 3, 1>& m) {      // Converter.cc:90-97
    cv::Mat cvMat(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) cvMat.at<float>(i) = (float)m[i];
    return cvMat.clone();
  }
};

// what LocalMapping::CreateNewMapPoints reads of the map, the tracker and itself
class Map {
 public:
  bool mbIMU_BA1 = false, mbIMU_BA2 = false;
  bool GetIniertialBA1() { return mbIMU_BA1; }
  bool GetIniertialBA2() { return mbIMU_BA2; }
};
class Atlas {
 public:
  Map map;
  std::vector<MapPoint*> added;
  Map* GetCurrentMap() { return &map; }
  void AddMapPoint(MapPoint* pMP) { added.push_back(pMP); }
};
class Tracking {
 public:
  enum eTrackingState { SYSTEM_NOT_READY = -1, NO_IMAGES_YET = 0, NOT_INITIALIZED = 1, OK = 2, RECENTLY_LOST = 3, LOST = 4, OK_KLT = 5 };
  eTrackingState mState = OK;
};
class LocalMapping {
 public:
  bool mbMonocular = false, mbInertial = false, mbFarPoints = false;
  float mThFarPoints = 0;
  KeyFrame* mpCurrentKeyFrame = nullptr;
  Tracking* mpTracker = nullptr;
  Atlas* mpAtlas = nullptr;
  std::list<MapPoint*> mlpRecentAddedMapPoints;
  bool CheckNewKeyFrames() { return false; }
  void CreateNewMapPoints();                                       // the reference's, as the next two
  cv::Mat ComputeF12(KeyFrame*& pKF1, KeyFrame*& pKF2);
  cv::Mat SkewSymmetricMatrix(const cv::Mat& v);
};

class MapLine {
 public:
  int index = 0;                                  // the driver's number of this object
  Vector6d mWorldPos;
  cv::Mat mDescriptor;
  bool mbBad = false, mbSeenInFrame = false;
  std::map<KeyFrame*, size_t> mObservations;
  std::mutex mMutexFeatures, mMutexPos;
  bool mbTrackInView = false;
  float mTrackProjsX = 0, mTrackProjsY = 0, mTrackProjeX = 0, mTrackProjeY = 0;
  double mnTrackangle = 0;

  Vector6d GetWorldPos() { return mWorldPos; }
  bool isBad() { return mbBad; }
  void ComputeDistinctiveDescriptors();           // the reference's
};

}  // namespace ORB_SLAM3
#endif
