// SearchByBoW(KF, KF) harness (test infrastructure, -m gpu): drives ORB_SLAM3::PliORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12)
// (pli_slam_amd/adapters/orbslam_adapters.hpp) through stub KeyFrame / MapPoint types holding std::map FeatureVectors, as
// LoopClosing::DetectCommonRegionsFromBoW calls it (LoopClosing.cc:533): once per pair, then the batch form once for all pairs.
// A device context comes from one ORBextractor call on a small image, as in the tracker.  tests/test_cpp_bow_kf_search.py
// compares the dumped vpMatches12 (as feature indices of pKF2, -1 = NULL) with the Python restatement.
//
//   usage: bow_kf_search_harness <in> <out>
//   in:  i32 nkf | f32 nnratio | i32 checkOri | pKF1, then nkf keyframes, each:
//        i32 n | u8 desc[n*32] f32 angle[n] i32 node[n] u8 state[n] (0 = no map point, 1 = good, 2 = isBad())
//   out: per keyframe, single call: i32 nmatches, i32 match12[n1]; then the same for the batch call
#define PLI_ADAPTER_NO_KEYLINE_HEADER
#define PLI_ADAPTER_KEYLINE_TYPE cv::line_descriptor::KeyLine
#include <opencv2/core/core.hpp>
namespace cv { namespace line_descriptor {
struct KeyLine {
  float angle; int class_id; int octave; cv::Point2f pt; float response; float size;
  float startPointX, startPointY, endPointX, endPointY, sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
  float lineLength; int numOfPixels;
};
}}
#include "pli_slam_amd/adapters/orbslam_adapters.hpp"
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;     // DBoW2::FeatureVector
struct MapPoint {
  bool bad = false;
  int idx = -1;
  bool isBad() { return bad; }
};
struct Camera {};
struct KeyFrame {
  int N = 0, NLeft = -1;
  cv::Mat mDescriptors;
  std::vector<cv::KeyPoint> mvKeysUn;
  FeatureVector mFeatVec;
  Camera* mpCamera2 = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};
struct Frame {};                                                              // PliORBmatcher's FrameT: the (KF, KF) overloads do not read it

template <class T> static void rd(FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}

static void fill(int n, FILE* f, cv::Mat& desc, std::vector<cv::KeyPoint>& kps, FeatureVector& fv) {
  desc.create(n, 32, CV_8U);
  std::vector<uint8_t> d((size_t)n * 32);
  std::vector<float> a(n);
  std::vector<int32_t> node(n);
  rd(f, d.data(), d.size());
  rd(f, a.data(), a.size());
  rd(f, node.data(), node.size());
  kps.resize(n);
  for (int i = 0; i < n; ++i) {
    std::memcpy(desc.ptr<uint8_t>(i), &d[(size_t)i * 32], 32);
    kps[i].angle = a[i];
    if (node[i] >= 0) fv[(unsigned)node[i]].push_back((unsigned)i);     // FeatureVector::addFeature in feature order
  }
}

static void readKeyFrame(FILE* in, KeyFrame& kf, std::vector<std::unique_ptr<MapPoint>>& points) {
  rd(in, &kf.N, 1);
  fill(kf.N, in, kf.mDescriptors, kf.mvKeysUn, kf.mFeatVec);
  std::vector<uint8_t> state(kf.N);
  rd(in, state.data(), state.size());
  kf.mvpMapPoints.assign(kf.N, nullptr);
  for (int i = 0; i < kf.N; ++i)
    if (state[i]) {
      points.emplace_back(new MapPoint());
      points.back()->bad = state[i] == 2;
      points.back()->idx = i;
      kf.mvpMapPoints[i] = points.back().get();
    }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t nkf, checkOri;
  float nnratio;
  rd(in, &nkf, 1); rd(in, &nnratio, 1); rd(in, &checkOri, 1);
  std::vector<std::unique_ptr<MapPoint>> points;
  KeyFrame kf1;
  readKeyFrame(in, kf1, points);
  const int n1 = kf1.N;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  for (int k = 0; k < nkf; ++k) {
    kfs.emplace_back(new KeyFrame());
    readKeyFrame(in, *kfs.back(), points);
  }
  std::fclose(in);
  try {
    // the device context: one extractor call, as the tracker has made before it matches anything
    ORB_SLAM3::ORBextractor extractor(500, 1.2f, 8, 20, 7);
    cv::Mat img(240, 376, CV_8U), mask, desc;
    for (int y = 0; y < img.rows; ++y)
      for (int x = 0; x < img.cols; ++x) img.ptr<uint8_t>(y)[x] = (uint8_t)((x * 7 + y * 13) ^ (x * y));
    std::vector<cv::KeyPoint> kps;
    std::vector<int> lap = {0, 0};
    extractor(img, mask, kps, desc, lap);

    ORB_SLAM3::PliORBmatcher<Frame, MapPoint> matcher(nnratio, checkOri != 0);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    auto dump = [&](int n, const std::vector<MapPoint*>& m) {
      std::vector<int32_t> v(n1, -1);
      if ((int)m.size() != n1) { std::fprintf(stderr, "vpMatches12 has %d entries, pKF1->N = %d\n", (int)m.size(), n1); std::exit(3); }
      for (int i = 0; i < n1; ++i) v[i] = m[i] ? m[i]->idx : -1;
      const int32_t n32 = n;
      std::fwrite(&n32, 4, 1, out);
      std::fwrite(v.data(), 4, v.size(), out);
    };
    for (int k = 0; k < nkf; ++k) {
      std::vector<MapPoint*> vpMatches12;
      const int n = matcher.SearchByBoW(&kf1, kfs[k].get(), vpMatches12);
      dump(n, vpMatches12);
    }
    std::vector<KeyFrame*> vpKFs;
    for (auto& k : kfs) vpKFs.push_back(k.get());
    std::vector<std::vector<MapPoint*>> vv;
    std::vector<int> vn;
    matcher.SearchByBoW(&kf1, vpKFs, vv, vn);
    for (int k = 0; k < nkf; ++k) dump(vn[k], vv[k]);
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
