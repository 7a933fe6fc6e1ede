// Sim3 projection harness (test infrastructure, -m gpu): drives the three ORB_SLAM3::PliORBmatcher::SearchByProjection(KeyFrame,
// Scw, ...) forms (pli_slam_amd/adapters/orbslam_adapters.hpp) through stub KeyFrame / MapPoint types, as LoopClosing calls them
// (LoopClosing.cc:631, :656, :852): per keyframe the reference's two signatures on copies of the same state (vpMatched partly filled
// at entry, bad points in the list, vpMatchedKF written), then the batch form once over all keyframes.  A device context comes
// from one ORBextractor call on a small image.  tests/test_cpp_sim3_projection.py compares the dumps with the restatement.
//
//   usage: sim3_projection_harness <in> <out>
//   in:  i32 nkf npool nlist | f32 cam[9] th ratio | i32 list[nlist] (pool index) | i32 listKf[nlist] (a keyframe index) |
//        pool: pli_fuse_point[npool] | u8 desc[npool*32] |
//        per keyframe: i32 n | f32 Scw[16] | f32 x[n] y[n] | i32 octave[n] | u8 desc[n*32] | i32 matched[n] (pool index or -1)
//   out: per keyframe: i32 n4 | i32 vpMatched[n] (pool index or -1)        (the form without vpPointsKFs)
//                      i32 n6 | i32 vpMatched[n] | i32 vpMatchedKF[n] (keyframe index or -1)
//        then the batch form: per keyframe i32 nb | i32 vpMatched[n];  then f32 level_ratio[7] and f32 pose[15] per keyframe
//        (the tables the adapter built with this host's compiler)
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
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <set>
#include <vector>

struct Frame {};
struct Camera {};
struct MapPoint;
struct KeyFrame {
  int N = 0, NLeft = -1;
  Camera* mpCamera2 = nullptr;
  float fx, fy, cx, cy, mbf;
  int mnMinX, mnMaxX, mnMinY, mnMaxY, mnScaleLevels = 8;
  float mfLogScaleFactor = std::log(1.2f);
  cv::Mat mDescriptors, Scw;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<int32_t> matched;
};
struct MapPoint {
  pli_fuse_point P;
  cv::Mat pos, normal, desc;
  bool bad = false;
  bool isBad() { return bad; }
  cv::Mat GetWorldPos() { return pos.clone(); }
  cv::Mat GetNormal() { return normal.clone(); }
  float GetMinDistanceInvariance() { return P.min_dist_inv; }
  float GetMaxDistanceInvariance() { return P.max_dist_inv; }
  float GetMaxDistance() { return P.max_dist; }
  cv::Mat GetDescriptor() { return desc.clone(); }
};

template <class T> static void rd(FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}
static void wr(FILE* f, const std::vector<int32_t>& v) { if (!v.empty()) std::fwrite(v.data(), 4, v.size(), f); }

struct World {
  std::vector<std::unique_ptr<MapPoint>> pool;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<MapPoint*> list;
  std::vector<KeyFrame*> listKf;
  float th = 3.f, ratio = 1.f;
};

static void load(const char* path, World& w) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "no input\n"); std::exit(2); }
  int32_t hdr[3];
  rd(f, hdr, 3);
  const int nkf = hdr[0], npool = hdr[1], nlist = hdr[2];
  float cam[11];
  rd(f, cam, 11);
  w.th = cam[9]; w.ratio = cam[10];
  std::vector<int32_t> list(nlist), listKf(nlist);
  rd(f, list.data(), nlist); rd(f, listKf.data(), nlist);
  std::vector<pli_fuse_point> P(npool);
  std::vector<uint8_t> d((size_t)npool * 32);
  rd(f, P.data(), npool); rd(f, d.data(), d.size());
  for (int i = 0; i < npool; ++i) {
    w.pool.emplace_back(new MapPoint());
    MapPoint& m = *w.pool.back();
    m.P = P[i];
    m.bad = !P[i].valid;
    m.pos.create(3, 1, CV_32F); m.normal.create(3, 1, CV_32F); m.desc.create(1, 32, CV_8U);
    for (int j = 0; j < 3; ++j) { m.pos.at<float>(j) = P[i].pos[j]; m.normal.at<float>(j) = P[i].normal[j]; }
    std::memcpy(m.desc.ptr<uint8_t>(), &d[(size_t)i * 32], 32);
  }
  for (int k = 0; k < nkf; ++k) {
    w.kfs.emplace_back(new KeyFrame());
    KeyFrame& kf = *w.kfs.back();
    int32_t n;
    rd(f, &n, 1);
    kf.N = n;
    kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.mbf = cam[4];
    kf.mnMinX = (int)cam[5]; kf.mnMaxX = (int)cam[6]; kf.mnMinY = (int)cam[7]; kf.mnMaxY = (int)cam[8];
    kf.Scw.create(4, 4, CV_32F);
    rd(f, kf.Scw.ptr<float>(), 16);
    std::vector<float> x(n), y(n);
    std::vector<int32_t> oct(n);
    std::vector<uint8_t> kd((size_t)n * 32);
    kf.matched.resize(n);
    rd(f, x.data(), n); rd(f, y.data(), n); rd(f, oct.data(), n); rd(f, kd.data(), kd.size()); rd(f, kf.matched.data(), n);
    kf.mDescriptors.create(n, 32, CV_8U);
    kf.mvKeysUn.resize(n);
    kf.mvuRight.assign(n, -1.f);
    for (int i = 0; i < n; ++i) {
      std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), &kd[(size_t)i * 32], 32);
      kf.mvKeysUn[i] = cv::KeyPoint(x[i], y[i], 31.f, 0.f, 0.f, oct[i]);
    }
  }
  for (int i = 0; i < nlist; ++i) { w.list.push_back(w.pool[list[i]].get()); w.listKf.push_back(w.kfs[listKf[i]].get()); }
  std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  World w;
  load(argv[1], w);
  try {
    // the device context: one extractor call, as the tracker has made before loop closing matches anything
    ORB_SLAM3::ORBextractor extractor(500, 1.2f, 8, 20, 7);
    cv::Mat img(240, 376, CV_8U), mask, desc;
    for (int y = 0; y < img.rows; ++y)
      for (int x = 0; x < img.cols; ++x) img.ptr<uint8_t>(y)[x] = (uint8_t)((x * 7 + y * 13) ^ (x * y));
    std::vector<cv::KeyPoint> kps;
    std::vector<int> lap = {0, 0};
    extractor(img, mask, kps, desc, lap);

    ORB_SLAM3::PliORBmatcher<Frame, MapPoint> matcher(0.9f, true);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::map<MapPoint*, int32_t> id;
    for (size_t i = 0; i < w.pool.size(); ++i) id[w.pool[i].get()] = (int32_t)i;
    std::map<KeyFrame*, int32_t> kid;
    for (size_t i = 0; i < w.kfs.size(); ++i) kid[w.kfs[i].get()] = (int32_t)i;
    auto entry = [&](KeyFrame& kf) {
      std::vector<MapPoint*> m(kf.N, nullptr);
      for (int i = 0; i < kf.N; ++i) if (kf.matched[i] >= 0) m[i] = w.pool[kf.matched[i]].get();
      return m;
    };
    auto ids = [&](const std::vector<MapPoint*>& m) {
      std::vector<int32_t> v;
      for (MapPoint* p : m) v.push_back(p ? id[p] : -1);
      return v;
    };
    std::vector<KeyFrame*> all;
    std::vector<cv::Mat> vScw;
    std::vector<std::vector<MapPoint*>> vvpMatched;
    for (auto& kfp : w.kfs) {
      KeyFrame& kf = *kfp;
      std::vector<MapPoint*> m4 = entry(kf);
      const int32_t n4 = matcher.SearchByProjection(&kf, kf.Scw, w.list, m4, (int)w.th, w.ratio);
      std::fwrite(&n4, 4, 1, out); wr(out, ids(m4));
      std::vector<MapPoint*> m6 = entry(kf);
      std::vector<KeyFrame*> mkf(kf.N, nullptr);
      const int32_t n6 = matcher.SearchByProjection(&kf, kf.Scw, w.list, w.listKf, m6, mkf, (int)w.th, w.ratio);
      std::fwrite(&n6, 4, 1, out); wr(out, ids(m6));
      std::vector<int32_t> v;
      for (KeyFrame* p : mkf) v.push_back(p ? kid[p] : -1);
      wr(out, v);
      all.push_back(&kf); vScw.push_back(kf.Scw); vvpMatched.push_back(entry(kf));
    }
    std::vector<int> vn;
    matcher.SearchByProjection(all, vScw, w.list, vvpMatched, (int)w.th, w.ratio, vn);
    for (size_t k = 0; k < all.size(); ++k) {
      const int32_t nb = vn[k];
      std::fwrite(&nb, 4, 1, out); wr(out, ids(vvpMatched[k]));
    }
    if (!w.kfs.empty()) {
      const std::vector<float>& lr = matcher.fuseLevelRatio(w.kfs[0].get());
      std::fwrite(lr.data(), 4, lr.size(), out);
    }
    for (auto& kfp : w.kfs) {
      float pose[15];
      ORB_SLAM3::PliORBmatcher<Frame, MapPoint>::sim3Pose(kfp->Scw, pose);
      std::fwrite(pose, 4, 15, out);
    }
    // a keyframe of two cameras is refused
    if (!w.kfs.empty()) {
      KeyFrame& kf = *w.kfs[0];
      std::vector<MapPoint*> m = entry(kf);
      int refused = 0;
      kf.NLeft = 10;
      try { matcher.SearchByProjection(&kf, kf.Scw, w.list, m, 3, 1.5f); } catch (const std::logic_error&) { ++refused; }
      kf.NLeft = -1;
      Camera second;
      kf.mpCamera2 = &second;
      try { matcher.SearchByProjection(&kf, kf.Scw, w.list, m, 3, 1.5f); } catch (const std::logic_error&) { ++refused; }
      kf.mpCamera2 = nullptr;
      if (refused != 2 || ids(m) != ids(entry(kf))) { std::fprintf(stderr, "two-camera keyframes were not refused\n"); return 3; }
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
