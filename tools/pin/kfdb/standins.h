// PIN — DEV-TIME TEST INFRASTRUCTURE ONLY (tools/gen_kfdb_ref.py).
// Force-included (-include) in front of the reference's own src/KeyFrameDatabase.cc, which is compiled where it lies, unmodified.
// Defines the include guards of the reference's KeyFrame.h, Frame.h and Map.h, so that those headers (and OpenCV, Eigen, g2o, Sophus
// behind them) stay out, and declares stand-in KeyFrame, Frame and Map classes of this project's own with just the members that
// KeyFrameDatabase.cc reads and writes.  Member names and types are the reference's; everything else is ours.
#ifndef PLI_PIN_KFDB_STANDINS_H
#define PLI_PIN_KFDB_STANDINS_H
#define KEYFRAME_H
#define FRAME_H
#define MAP_H

#include <algorithm>
#include <array>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <vector>
#include <opencv2/core/core.hpp>                 // oracle/ref_recipe/bow_shim: a cv::Mat that stores bytes
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"     // the reference's own

namespace cv {
struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; float size = 0; };
}  // namespace cv

using namespace std;      // the reference's KeyFrameDatabase.h writes vector<> and map<> unqualified (its KeyFrame.h chain says this)

namespace ORB_SLAM3 {

class Map {
 public:
  bool IsBad() { return mbBad; }
  bool mbBad = false;
  int index = 0;
};

class KeyFrame {
 public:
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n) {      // the first n of the ordered covisibility list
    const size_t m = std::min(mvpOrderedConnectedKeyFrames.size(), (size_t)std::max(n, 0));
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + m);
  }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(mConnected.begin(), mConnected.end()); }
  Map* GetMap() { return mpMap; }
  bool isBad() { return mbBad; }

  long unsigned int mnId = 0;
  int N = 0, N_l = 0;
  DBoW2::BowVector mBowVec, mBowVec_l;
  // the members' initial values are KeyFrame.cc's constructor's
  long unsigned int mnLoopQuery = 0, mnLoopQuery_l = 0;
  int mnLoopWords = 0, mnLoopWords_l = 0;
  float mLoopScore = 0, mLoopScore_l = 0, mLoopScore_pl = 0;
  long unsigned int mnRelocQuery = 0, mnRelocQuery_l = 0;
  int mnRelocWords = 0, mnRelocWords_l = 0;
  float mRelocScore = 0, mRelocScore_l = 0, mRelocScore_pl = 0;
  long unsigned int mnMergeQuery = 0;
  int mnMergeWords = 0;
  float mMergeScore = 0;
  long unsigned int mnPlaceRecognitionQuery = 0;
  int mnPlaceRecognitionWords = 0;
  float mPlaceRecognitionScore = 0;

  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  std::vector<KeyFrame*> mConnected;
  Map* mpMap = nullptr;
  bool mbBad = false;
};

class Frame {
 public:
  long unsigned int mnId = 0;
  int N = 0, N_l = 0;
  DBoW2::BowVector mBowVec, mBowVec_l;
};

}  // namespace ORB_SLAM3
#endif
