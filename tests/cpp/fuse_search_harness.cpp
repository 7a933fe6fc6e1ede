// Fuse harness (test infrastructure, -m gpu): drives ORB_SLAM3::PliORBmatcher::Fuse (pli_slam_amd/adapters/orbslam_adapters.hpp)
// through stub KeyFrame / MapPoint types, as LocalMapping::SearchInNeighbors calls it (LocalMapping.cc:743-749): the reference's
// signature keyframe after keyframe, and the batch form once, on two copies of the same state.  The stub MapPoint::Replace moves
// the observations as MapPoint.cc:232-276 does and installs a different descriptor (from the input file) on the survivor, which
// stands for ComputeDistinctiveDescriptors().  A device context comes from one ORBextractor call on a small image.
// tests/test_cpp_fuse_search.py compares the dumps with a Python simulation over the restatement.
//
//   usage: fuse_search_harness <in> <out>
//   in:  i32 nkf npool nlist | f32 cam[9] th | i32 list[nlist] (pool index or -1) |
//        pool: pli_fuse_point[npool] | u8 desc[npool*32] | u8 altDesc[npool*32] | i32 obs0[npool] |
//        per keyframe: i32 n | f32 pose[15] | f32 x[n] y[n] | i32 octave[n] | u8 desc[n*32] | f32 uright[n] | i32 mp[n] (pool index or -1)
//   out: for the single calls, then for the batch call: i32 nFused[nkf] | per keyframe i32 mvpMapPoints[n] (pool index or -1) |
//        i32 bad[npool] | i32 number of repeated searches;  then f32 level_ratio[7] (the table the adapter built)
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
struct MapPoint;
struct KeyFrame {
  int N = 0, NLeft = -1;
  float fx, fy, cx, cy, mbf;
  int mnMinX, mnMaxX, mnMinY, mnMaxY, mnScaleLevels = 8;
  float mfLogScaleFactor = std::log(1.2f);
  cv::Mat mDescriptors, Rcw, tcw, Ow;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<MapPoint*> mvpMapPoints;
  MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
  void AddMapPoint(MapPoint* p, const size_t& idx) { mvpMapPoints[idx] = p; }
  void ReplaceMapPointMatch(const int& idx, MapPoint* p) { mvpMapPoints[idx] = p; }
  void EraseMapPointMatch(const int& idx) { mvpMapPoints[idx] = nullptr; }
  std::set<MapPoint*> GetMapPoints() {
    std::set<MapPoint*> s;
    for (MapPoint* p : mvpMapPoints) if (p) s.insert(p);
    return s;
  }
  cv::Mat GetRotation() { return Rcw.clone(); }
  cv::Mat GetTranslation() { return tcw.clone(); }
  cv::Mat GetCameraCenter() { return Ow.clone(); }
};
struct MapPoint {
  pli_fuse_point P;
  cv::Mat pos, normal, desc, altDesc;
  bool bad = false;
  int obs0 = 0;
  std::map<KeyFrame*, int> obs;
  bool isBad() { return bad; }
  bool IsInKeyFrame(KeyFrame* kf) { return obs.count(kf) != 0; }
  cv::Mat GetWorldPos() { return pos.clone(); }
  cv::Mat GetNormal() { return normal.clone(); }
  float GetMinDistanceInvariance() { return P.min_dist_inv; }
  float GetMaxDistanceInvariance() { return P.max_dist_inv; }
  float GetMaxDistance() { return P.max_dist; }
  cv::Mat GetDescriptor() { return desc.clone(); }
  int Observations() { return obs0 + (int)obs.size(); }
  void AddObservation(KeyFrame* kf, int idx) { if (!obs.count(kf)) obs[kf] = idx; }
  void Replace(MapPoint* pMP) {                        // MapPoint.cc:232-276
    if (pMP == this) return;
    std::map<KeyFrame*, int> o = obs;
    obs.clear();
    bad = true;
    for (auto& e : o) {
      if (!pMP->IsInKeyFrame(e.first)) { e.first->ReplaceMapPointMatch(e.second, pMP); pMP->AddObservation(e.first, e.second); }
      else e.first->EraseMapPointMatch(e.second);
    }
    pMP->obs0 += obs0;
    pMP->desc = pMP->altDesc.clone();                 // ComputeDistinctiveDescriptors(): another descriptor
  }
};

template <class T> static void rd(FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}

struct World {
  std::vector<std::unique_ptr<MapPoint>> pool;
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  std::vector<MapPoint*> list;
};

static void load(const char* path, World& w, float& th) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "no input\n"); std::exit(2); }
  int32_t hdr[3];
  rd(f, hdr, 3);
  const int nkf = hdr[0], npool = hdr[1], nlist = hdr[2];
  float cam[10];
  rd(f, cam, 10);
  th = cam[9];
  std::vector<int32_t> list(nlist), obs0(npool);
  rd(f, list.data(), nlist);
  std::vector<pli_fuse_point> P(npool);
  std::vector<uint8_t> d((size_t)npool * 32), a((size_t)npool * 32);
  rd(f, P.data(), npool); rd(f, d.data(), d.size()); rd(f, a.data(), a.size()); rd(f, obs0.data(), npool);
  for (int i = 0; i < npool; ++i) {
    w.pool.emplace_back(new MapPoint());
    MapPoint& m = *w.pool.back();
    m.P = P[i];
    m.bad = !P[i].valid;
    m.obs0 = obs0[i];
    m.pos.create(3, 1, CV_32F); m.normal.create(3, 1, CV_32F); m.desc.create(1, 32, CV_8U); m.altDesc.create(1, 32, CV_8U);
    for (int j = 0; j < 3; ++j) { m.pos.at<float>(j) = P[i].pos[j]; m.normal.at<float>(j) = P[i].normal[j]; }
    std::memcpy(m.desc.ptr<uint8_t>(), &d[(size_t)i * 32], 32);
    std::memcpy(m.altDesc.ptr<uint8_t>(), &a[(size_t)i * 32], 32);
  }
  for (int i = 0; i < nlist; ++i) w.list.push_back(list[i] < 0 ? nullptr : w.pool[list[i]].get());
  for (int k = 0; k < nkf; ++k) {
    w.kfs.emplace_back(new KeyFrame());
    KeyFrame& kf = *w.kfs.back();
    int32_t n;
    rd(f, &n, 1);
    kf.N = n;
    kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.mbf = cam[4];
    kf.mnMinX = (int)cam[5]; kf.mnMaxX = (int)cam[6]; kf.mnMinY = (int)cam[7]; kf.mnMaxY = (int)cam[8];
    float pose[15];
    rd(f, pose, 15);
    kf.Rcw.create(3, 3, CV_32F); kf.tcw.create(3, 1, CV_32F); kf.Ow.create(3, 1, CV_32F);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) kf.Rcw.at<float>(i, j) = pose[i * 3 + j];
      kf.tcw.at<float>(i) = pose[9 + i];
      kf.Ow.at<float>(i) = pose[12 + i];
    }
    std::vector<float> x(n), y(n), ur(n);
    std::vector<int32_t> oct(n), mp(n);
    std::vector<uint8_t> kd((size_t)n * 32);
    rd(f, x.data(), n); rd(f, y.data(), n); rd(f, oct.data(), n); rd(f, kd.data(), kd.size()); rd(f, ur.data(), n); rd(f, mp.data(), n);
    kf.mDescriptors.create(n, 32, CV_8U);
    kf.mvKeysUn.resize(n);
    kf.mvuRight = ur;
    kf.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; ++i) {
      std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), &kd[(size_t)i * 32], 32);
      kf.mvKeysUn[i] = cv::KeyPoint(x[i], y[i], 31.f, 0.f, 0.f, oct[i]);
      if (mp[i] >= 0) { kf.mvpMapPoints[i] = w.pool[mp[i]].get(); w.pool[mp[i]]->AddObservation(&kf, i); }
    }
  }
  std::fclose(f);
}

static void dump(FILE* out, World& w, const std::vector<int>& nFused, int nresearch) {
  std::map<MapPoint*, int32_t> id;
  for (size_t i = 0; i < w.pool.size(); ++i) id[w.pool[i].get()] = (int32_t)i;
  for (int n : nFused) { const int32_t v = n; std::fwrite(&v, 4, 1, out); }
  for (auto& kf : w.kfs)
    for (MapPoint* p : kf->mvpMapPoints) { const int32_t v = p ? id[p] : -1; std::fwrite(&v, 4, 1, out); }
  for (auto& p : w.pool) { const int32_t v = p->bad ? 1 : 0; std::fwrite(&v, 4, 1, out); }
  const int32_t r = nresearch;
  std::fwrite(&r, 4, 1, out);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  World a, b;
  float th = 3.f;
  load(argv[1], a, th);
  load(argv[1], b, th);
  try {
    // the device context: one extractor call, as the tracker has made before the mapper fuses anything
    ORB_SLAM3::ORBextractor extractor(500, 1.2f, 8, 20, 7);
    cv::Mat img(240, 376, CV_8U), mask, desc;
    for (int y = 0; y < img.rows; ++y)
      for (int x = 0; x < img.cols; ++x) img.ptr<uint8_t>(y)[x] = (uint8_t)((x * 7 + y * 13) ^ (x * y));
    std::vector<cv::KeyPoint> kps;
    std::vector<int> lap = {0, 0};
    extractor(img, mask, kps, desc, lap);

    ORB_SLAM3::PliORBmatcher<Frame, MapPoint> matcher(0.6f, true);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::vector<int> nFused;
    for (auto& kf : a.kfs) nFused.push_back(matcher.Fuse(kf.get(), a.list, th));
    dump(out, a, nFused, 0);
    std::vector<KeyFrame*> targets;
    for (auto& kf : b.kfs) targets.push_back(kf.get());
    int nresearch = 0;
    matcher.Fuse(targets, b.list, th, nFused, &nresearch);
    dump(out, b, nFused, nresearch);
    if (!b.kfs.empty()) {
      const std::vector<float>& lr = matcher.fuseLevelRatio(b.kfs[0].get());
      std::fwrite(lr.data(), 4, lr.size(), out);
      // the Sim3 overload with Scw = [Rcw | tcw] (scale 1) on a third copy: compiled and run, its count dumped last
      World c;
      load(argv[1], c, th);
      cv::Mat Scw = cv::Mat::eye(4, 4, CV_32F);
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Scw.at<float>(i, j) = c.kfs[0]->Rcw.at<float>(i, j);
        Scw.at<float>(i, 3) = c.kfs[0]->tcw.at<float>(i);
      }
      std::vector<MapPoint*> pts, repl;
      for (MapPoint* p : c.list) if (p) pts.push_back(p);
      repl.assign(pts.size(), nullptr);
      const int32_t n3 = matcher.Fuse(c.kfs[0].get(), Scw, pts, th, repl);
      std::fwrite(&n3, 4, 1, out);
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
