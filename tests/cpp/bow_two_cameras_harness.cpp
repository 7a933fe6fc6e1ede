// SearchByBoW harness for frames and keyframes of two cameras (test infrastructure, -m gpu): drives
// ORB_SLAM3::PliORBmatcherTwoCameras::SearchByBoW (pli_slam_amd/adapters/orbslam_two_cameras.hpp) through stub KeyFrame / Frame /
// MapPoint types holding std::map FeatureVectors, as Tracking.cc calls it: once per keyframe (TrackReferenceKeyFrame, :2648 /
// :2708) and once for all candidates (Relocalization's loop, :4205-4230).  A frame of two cameras keeps its angles in mvKeys /
// mvKeysRight, a keyframe of two cameras too (its mvKeysUn holds NLeft entries, as in the reference, with other angles, so that
// a read of the wrong table shows); a keyframe of one camera keeps them in mvKeysUn.  A device context comes from one
// ORBextractor call on a small image.  tests/test_cpp_bow_two_cameras.py compares the dumped vpMapPointMatches (as keyframe
// feature indices, -1 = NULL) with the Python restatements.
//
//   usage: bow_two_cameras_harness <in> <out>
//   in:  i32 nkf nf fNleft (-1: a frame of one camera) | f32 nnratio | i32 checkOri | frame: u8 desc[nf*32] f32 angle[nf] i32 node[nf] |
//        per keyframe: i32 n nleft (-1: a keyframe of one camera) | u8 desc[n*32] f32 angle[n] i32 node[n]
//        u8 state[n] (0 = no map point, 1 = good, 2 = isBad())
//   out: per keyframe, single call: i32 nmatches, i32 match[nf]; then the same for the batch call
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
#include "pli_slam_amd/adapters/orbslam_two_cameras.hpp"
#include <cmath>
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
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
  FeatureVector mFeatVec;
  Camera* mpCamera2 = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};
struct Frame {
  int N = 0, Nleft = -1, Nright = -1;
  cv::Mat mDescriptors;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
  FeatureVector mFeatVec;
};

// the angles of a two-camera table: rows < nleft in `left`, the others in `right`; unrectified: what mvKeysUn holds then
static void split(const std::vector<cv::KeyPoint>& all, int nleft, std::vector<cv::KeyPoint>& left, std::vector<cv::KeyPoint>& right,
                  std::vector<cv::KeyPoint>* unrectified) {
  left.assign(all.begin(), all.begin() + nleft);
  right.assign(all.begin() + nleft, all.end());
  if (unrectified) {
    *unrectified = left;
    for (cv::KeyPoint& k : *unrectified) k.angle = std::fmod(k.angle + 33.f, 360.f);
  }
}

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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t nkf, nf, fNleft, checkOri;
  float nnratio;
  rd(in, &nkf, 1); rd(in, &nf, 1); rd(in, &fNleft, 1); rd(in, &nnratio, 1); rd(in, &checkOri, 1);
  Frame F;
  F.N = nf;
  std::vector<cv::KeyPoint> all;
  fill(nf, in, F.mDescriptors, all, F.mFeatVec);
  if (fNleft >= 0) { F.Nleft = fNleft; F.Nright = nf - fNleft; split(all, fNleft, F.mvKeys, F.mvKeysRight, nullptr); }
  else F.mvKeys = all;
  static Camera camera2;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<std::unique_ptr<MapPoint>> points;
  for (int k = 0; k < nkf; ++k) {
    kfs.emplace_back(new KeyFrame());
    KeyFrame& kf = *kfs.back();
    int32_t h[2];
    rd(in, h, 2);
    kf.N = h[0];
    fill(kf.N, in, kf.mDescriptors, all, kf.mFeatVec);
    if (h[1] >= 0) { kf.NLeft = h[1]; kf.mpCamera2 = &camera2; split(all, h[1], kf.mvKeys, kf.mvKeysRight, &kf.mvKeysUn); }
    else {
      kf.mvKeysUn = all;
      kf.mvKeys = all;
      for (cv::KeyPoint& kp : kf.mvKeys) kp.angle = std::fmod(kp.angle + 33.f, 360.f);      // (not read for such a keyframe, :380)
    }
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

    ORB_SLAM3::PliORBmatcherTwoCameras<Frame, MapPoint> matcher(nnratio, checkOri != 0);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    auto dump = [&](int n, const std::vector<MapPoint*>& m) {
      std::vector<int32_t> v(nf, -1);
      if ((int)m.size() != nf) { std::fprintf(stderr, "vpMapPointMatches has %d entries, F.N = %d\n", (int)m.size(), nf); std::exit(3); }
      for (int i = 0; i < nf; ++i) v[i] = m[i] ? m[i]->idx : -1;
      const int32_t n32 = n;
      std::fwrite(&n32, 4, 1, out);
      std::fwrite(v.data(), 4, v.size(), out);
    };
    for (int k = 0; k < nkf; ++k) {
      std::vector<MapPoint*> vpMapPointMatches;
      const int n = matcher.SearchByBoW(kfs[k].get(), F, vpMapPointMatches);
      dump(n, vpMapPointMatches);
    }
    std::vector<KeyFrame*> vpKFs;
    for (auto& k : kfs) vpKFs.push_back(k.get());
    std::vector<std::vector<MapPoint*>> vv;
    std::vector<int> vn;
    matcher.SearchByBoW(vpKFs, F, vv, vn);
    for (int k = 0; k < nkf; ++k) dump(vn[k], vv[k]);
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
