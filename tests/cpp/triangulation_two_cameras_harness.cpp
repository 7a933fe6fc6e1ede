// SearchForTriangulation harness for keyframes of two cameras (test infrastructure, -m gpu): drives
// ORB_SLAM3::PliORBmatcherTwoCameras::SearchForTriangulation (pli_slam_amd/adapters/orbslam_two_cameras.hpp) through stub KeyFrame /
// MapPoint / camera types, as LocalMapping::CreateNewMapPoints calls it (LocalMapping.cc:387-423): once per neighbour with the
// reference's signature and once for all neighbours (the batch form).  The stub KeyFrame carries mvKeys / mvKeysRight, NLeft, mTlr
// and the right-pose getters written as KeyFrame.cc:1343-1373, so the adapter's four relative poses are computed from the same
// members the reference reads.  Keyframes without a second camera (twoCameras = 0) go the forwarded way, through
// PliORBmatcher::SearchForTriangulation.  A device context comes from one ORBextractor call on a small image, as in the tracker.
// tests/test_cpp_triangulation_two_cameras.py compares the dumped pair lists with the Python restatement.
//
//   usage: triangulation_two_cameras_harness <in> <out>
//   in:  i32 nkf onlyStereo coarse checkOri | f32 camLeft[8] camRight[8] | f32 Tlr[12] (3 x 4, row major) | keyframe, then nkf
//        neighbours, each: i32 n nleft twoCameras | f32 Rcw[9] tcw[3] | f32 x[n] y[n] | i32 octave[n] | f32 angle[n] |
//        u8 desc[n*32] | i32 node[n] | u8 hasMp[n]
//   out: per neighbour, single call: i32 nmatches, i32 match12[n1] (from vMatchedPairs); the same for the batch call; then
//        two cameras: i32 threwMixed threwCameras (1 = std::logic_error: a neighbour without mpCamera2, a neighbour with
//        other camera parameters); one camera: per neighbour f32 F12[9] ep[2] (pli_detail::triangulationGeometry)
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
#include <cstdio>
#include <map>
#include <memory>
#include <utility>
#include <vector>

typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;     // DBoW2::FeatureVector
struct MapPoint {
  bool isBad() { return true; }          // SearchForTriangulation asks GetMapPoint() only: a bad point blocks a feature too
};
struct Frame {};
struct Camera {                          // GeometricCamera: mvParameters behind getParameter()
  std::vector<float> mvParameters;
  float getParameter(const int i) { return mvParameters[i]; }
  size_t size() { return mvParameters.size(); }
  cv::Mat toK() {
    cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
    K.at<float>(0, 0) = mvParameters[0]; K.at<float>(1, 1) = mvParameters[1];
    K.at<float>(0, 2) = mvParameters[2]; K.at<float>(1, 2) = mvParameters[3];
    return K;
  }
};
struct KeyFrame {
  int N = 0, NLeft = -1;
  cv::Mat mDescriptors, Tcw, Ow, mTlr;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
  std::vector<float> mvuRight;
  FeatureVector mFeatVec;
  Camera* mpCamera = nullptr;
  Camera* mpCamera2 = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
  cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
  cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
  cv::Mat GetCameraCenter() { return Ow.clone(); }
  cv::Mat GetRightCameraCenter() {
    cv::Mat Rwl = Tcw.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat tlr = mTlr.rowRange(0, 3).col(3);
    cv::Mat twl = Ow.clone();
    cv::Mat twr = Rwl * tlr + twl;
    return twr.clone();
  }
  cv::Mat GetRightRotation() {
    cv::Mat Rrl = mTlr.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat Rlw = Tcw.rowRange(0, 3).colRange(0, 3).clone();
    cv::Mat Rrw = Rrl * Rlw;
    return Rrw.clone();
  }
  cv::Mat GetRightTranslation() {
    cv::Mat Rrl = mTlr.rowRange(0, 3).colRange(0, 3).t();
    cv::Mat tlw = Tcw.rowRange(0, 3).col(3).clone();
    cv::Mat trl = -Rrl * mTlr.rowRange(0, 3).col(3);
    cv::Mat trw = Rrl * tlw + trl;
    return trw.clone();
  }
  cv::Mat GetRightPose() {               // [Rrw | trw]
    cv::Mat Trw(3, 4, CV_32F);
    const cv::Mat R = GetRightRotation(), t = GetRightTranslation();
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Trw.at<float>(i, j) = R.at<float>(i, j);
      Trw.at<float>(i, 3) = t.at<float>(i);
    }
    return Trw;
  }
};

template <class T> static void rd(FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}

static MapPoint g_point;

static void fill(FILE* f, KeyFrame& kf, Camera* camL, Camera* camR, const cv::Mat& Tlr) {
  int32_t h[3];
  rd(f, h, 3);
  const int n = h[0], nleft = h[1];
  const bool two = h[2] != 0;
  kf.N = n;
  kf.NLeft = two ? nleft : -1;
  kf.mpCamera = camL;
  kf.mpCamera2 = two ? camR : nullptr;
  kf.mTlr = Tlr.clone();
  float R[9], t[3];
  rd(f, R, 9); rd(f, t, 3);
  kf.Tcw.create(3, 4, CV_32F);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) kf.Tcw.at<float>(i, j) = R[i * 3 + j];
    kf.Tcw.at<float>(i, 3) = t[i];
  }
  kf.Ow = -kf.Tcw.rowRange(0, 3).colRange(0, 3).t() * kf.Tcw.rowRange(0, 3).col(3);     // Ow = -Rwc * tcw (KeyFrame.cc SetPose)
  std::vector<float> x(n), y(n), a(n);
  std::vector<int32_t> oct(n), node(n);
  std::vector<uint8_t> d((size_t)n * 32), mp(n);
  rd(f, x.data(), n); rd(f, y.data(), n); rd(f, oct.data(), n); rd(f, a.data(), n); rd(f, d.data(), d.size());
  rd(f, node.data(), n); rd(f, mp.data(), n);
  kf.mDescriptors.create(n, 32, CV_8U);
  kf.mvuRight.assign(n, -1.f);
  kf.mvpMapPoints.assign(n, nullptr);
  for (int i = 0; i < n; ++i) {
    std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), &d[(size_t)i * 32], 32);
    const cv::KeyPoint k(x[i], y[i], 31.f, a[i], 0.f, oct[i]);
    if (!two) { kf.mvKeys.push_back(k); kf.mvKeysUn.push_back(k); }
    else if (i < nleft) kf.mvKeys.push_back(k);
    else kf.mvKeysRight.push_back(k);
    if (mp[i]) kf.mvpMapPoints[i] = &g_point;
    if (node[i] >= 0) kf.mFeatVec[(unsigned)node[i]].push_back((unsigned)i);     // FeatureVector::addFeature in feature order
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[4];
  rd(in, hdr, 4);
  const int nkf = hdr[0];
  const bool onlyStereo = hdr[1] != 0, coarse = hdr[2] != 0, checkOri = hdr[3] != 0;
  Camera camL, camR;
  camL.mvParameters.resize(8); camR.mvParameters.resize(8);
  rd(in, camL.mvParameters.data(), 8); rd(in, camR.mvParameters.data(), 8);
  cv::Mat Tlr(3, 4, CV_32F);
  rd(in, Tlr.ptr<float>(0), 12);
  KeyFrame kf1;
  fill(in, kf1, &camL, &camR, Tlr);
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  for (int k = 0; k < nkf; ++k) {
    kfs.emplace_back(new KeyFrame());
    fill(in, *kfs.back(), &camL, &camR, Tlr);
  }
  std::fclose(in);
  try {
    // the device context: one extractor call, as the tracker has made before the mapper matches anything
    ORB_SLAM3::ORBextractor extractor(500, 1.2f, 8, 20, 7);
    cv::Mat img(240, 376, CV_8U), mask, desc;
    for (int y = 0; y < img.rows; ++y)
      for (int x = 0; x < img.cols; ++x) img.ptr<uint8_t>(y)[x] = (uint8_t)((x * 7 + y * 13) ^ (x * y));
    std::vector<cv::KeyPoint> kps;
    std::vector<int> lap = {0, 0};
    extractor(img, mask, kps, desc, lap);

    ORB_SLAM3::PliORBmatcherTwoCameras<Frame, MapPoint> matcher(0.6f, checkOri);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int n1 = kf1.N;
    auto dump = [&](int n, const std::vector<std::pair<size_t, size_t>>& pairs) {
      std::vector<int32_t> v(n1, -1);
      if ((int)pairs.size() != n) { std::fprintf(stderr, "%d pairs, return value %d\n", (int)pairs.size(), n); std::exit(3); }
      for (size_t p = 0; p < pairs.size(); ++p) {
        if (p > 0 && pairs[p - 1].first >= pairs[p].first) { std::fprintf(stderr, "vMatchedPairs not in index order\n"); std::exit(3); }
        v[pairs[p].first] = (int32_t)pairs[p].second;
      }
      const int32_t n32 = n;
      std::fwrite(&n32, 4, 1, out);
      std::fwrite(v.data(), 4, v.size(), out);
    };
    for (int k = 0; k < nkf; ++k) {
      std::vector<std::pair<size_t, size_t>> vMatchedPairs(3);      // (cleared by the call, as in the reference)
      const int n = matcher.SearchForTriangulation(&kf1, kfs[k].get(), cv::Mat(), vMatchedPairs, onlyStereo, coarse);
      dump(n, vMatchedPairs);
    }
    std::vector<KeyFrame*> vpKF2;
    for (auto& k : kfs) vpKF2.push_back(k.get());
    std::vector<std::vector<std::pair<size_t, size_t>>> vv;
    std::vector<int> vn;
    matcher.SearchForTriangulation(&kf1, vpKF2, vv, vn, onlyStereo, coarse);
    for (int k = 0; k < nkf; ++k) dump(vn[k], vv[k]);
    if (kf1.mpCamera2) {
      // the two refusals: a neighbour without a second camera beside one with, and a neighbour with other camera parameters
      int32_t threw[2] = {0, 0};
      if (nkf > 0) {
        KeyFrame mono = *kfs[0];
        mono.mpCamera2 = nullptr;
        mono.NLeft = -1;
        std::vector<KeyFrame*> mixed = vpKF2;
        mixed.push_back(&mono);
        try { matcher.SearchForTriangulation(&kf1, mixed, vv, vn, onlyStereo, coarse); } catch (const std::logic_error&) { threw[0] = 1; }
        Camera other = camR;
        other.mvParameters[2] += 0.5f;
        KeyFrame moved = *kfs[0];
        moved.mpCamera2 = &other;
        std::vector<std::pair<size_t, size_t>> vMatchedPairs;
        try { matcher.SearchForTriangulation(&kf1, &moved, cv::Mat(), vMatchedPairs, onlyStereo, coarse); }
        catch (const std::logic_error&) { threw[1] = 1; }
      }
      std::fwrite(threw, 4, 2, out);
    } else {
      // the geometry the forwarded call used, from the same members
      for (int k = 0; k < nkf; ++k) {
        float R1[9], t1[3], R2[9], t2[3], cw[3], g[11];
        const cv::Mat Cw = kf1.GetCameraCenter();
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) { R1[i * 3 + j] = kf1.Tcw.at<float>(i, j); R2[i * 3 + j] = kfs[k]->Tcw.at<float>(i, j); }
          t1[i] = kf1.Tcw.at<float>(i, 3); t2[i] = kfs[k]->Tcw.at<float>(i, 3); cw[i] = Cw.at<float>(i);
        }
        ORB_SLAM3::pli_detail::triangulationGeometry(R1, t1, cw, camL.mvParameters.data(), R2, t2, camL.mvParameters.data(), g, g + 9);
        std::fwrite(g, 4, 11, out);
      }
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
