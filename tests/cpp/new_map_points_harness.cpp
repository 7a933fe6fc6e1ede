// CreateNewMapPoints harness (test infrastructure, -m gpu): drives ORB_SLAM3::PliCreateNewMapPoints
// (pli_slam_amd/adapters/orbslam_local_mapping.hpp) through stub KeyFrame / MapPoint / Atlas types that log every call of
// LocalMapping.cc:670-683.  A device context comes from one ORBextractor call on a small image, as in the tracker.
// tests/test_cpp_new_map_points.py compares the dumped log with the Python restatement of the reference's loop, run on the F12 /
// epipole that pli_detail::triangulationGeometry produced (dumped too), so the host arithmetic needs no tolerance.
//
//   usage: new_map_points_harness <in> <out>
//   in:  i32 nkf coarse farPoints stopBefore (-1: never) | f32 K[4] (fx fy cx cy) bf mb thFar scaleFactor | keyframe, then nkf
//        neighbours, each: i32 n | f32 pose[15] (Rcw, tcw, Ow) | f32 x[n] y[n] | i32 octave[n] | f32 angle[n] | u8 desc[n*32] |
//        i32 node[n] | u8 hasMp[n] | f32 uright[n] depth[n] key[2n]
//   out: i32 return value, nlog | nlog x (i32 what, a, b, c) | f32 x3D[3] per created point | per neighbour f32 F12[9] ep[2]
//        what: 0 new MapPoint (a = reference keyframe, b = serial of the point), 1 AddObservation (a = point, b = keyframe, c = idx),
//        2 AddMapPoint (a = keyframe, b = point, c = idx), 3 ComputeDistinctiveDescriptors (a = point), 4 UpdateNormalAndDepth,
//        5 Atlas::AddMapPoint, 6 the entry of mlpRecentAddedMapPoints (read at the end), 7 CheckNewKeyFrames asked
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
#include "pli_slam_amd/adapters/orbslam_local_mapping.hpp"
#include <cstdio>
#include <list>
#include <map>
#include <memory>
#include <vector>

typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;     // DBoW2::FeatureVector
static std::vector<int32_t> g_log;
static std::vector<float> g_pos;
static void logCall(int what, int a, int b, int c) { g_log.push_back(what); g_log.push_back(a); g_log.push_back(b); g_log.push_back(c); }

struct Map {};
struct KeyFrame;
struct MapPoint {
  int serial = -1;                       // -1: a map point the keyframe had at entry
  MapPoint() {}
  MapPoint(const cv::Mat& pos, KeyFrame* pRefKF, Map* pMap);
  void AddObservation(KeyFrame* pKF, int idx);
  void ComputeDistinctiveDescriptors() { logCall(3, serial, 0, 0); }
  void UpdateNormalAndDepth() { logCall(4, serial, 0, 0); }
};
struct Frame {};
struct Camera {
  float k[4];
  cv::Mat toK() {
    cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
    K.at<float>(0, 0) = k[0]; K.at<float>(1, 1) = k[1]; K.at<float>(0, 2) = k[2]; K.at<float>(1, 2) = k[3];
    return K;
  }
};
struct KeyFrame {
  int id = 0, N = 0, NLeft = -1;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0, mfScaleFactor = 0;
  cv::Mat mDescriptors, Rcw, tcw, Ow;
  std::vector<cv::KeyPoint> mvKeysUn, mvKeys;
  std::vector<float> mvuRight, mvDepth;
  FeatureVector mFeatVec;
  Camera* mpCamera = nullptr;
  Camera* mpCamera2 = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; logCall(2, id, pMP->serial, (int)idx); }
  cv::Mat GetRotation() { return Rcw.clone(); }
  cv::Mat GetTranslation() { return tcw.clone(); }
  cv::Mat GetCameraCenter() { return Ow.clone(); }                 // the stored value (KeyFrame::SetPose)
};
static int g_serial = 0;
MapPoint::MapPoint(const cv::Mat& pos, KeyFrame* pRefKF, Map*) : serial(g_serial++) {
  logCall(0, pRefKF->id, serial, 0);
  for (int r = 0; r < 3; ++r) g_pos.push_back(pos.at<float>(r));
}
void MapPoint::AddObservation(KeyFrame* pKF, int idx) { logCall(1, serial, pKF->id, idx); }
struct Atlas {
  Map map;
  Map* GetCurrentMap() { return &map; }
  void AddMapPoint(MapPoint* pMP) { logCall(5, pMP->serial, 0, 0); }
};

template <class T> static void rd(FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}

static MapPoint g_point;

static void fill(FILE* f, KeyFrame& kf, Camera* cam, const float* par) {
  int32_t n;
  rd(f, &n, 1);
  kf.N = n;
  kf.mpCamera = cam;
  kf.fx = cam->k[0]; kf.fy = cam->k[1]; kf.cx = cam->k[2]; kf.cy = cam->k[3];
  kf.mbf = par[0]; kf.mb = par[1]; kf.mfScaleFactor = par[3];
  float pose[15];
  rd(f, pose, 15);
  kf.Rcw.create(3, 3, CV_32F); kf.tcw.create(3, 1, CV_32F); kf.Ow.create(3, 1, CV_32F);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) kf.Rcw.at<float>(i, j) = pose[i * 3 + j];
    kf.tcw.at<float>(i) = pose[9 + i];
    kf.Ow.at<float>(i) = pose[12 + i];
  }
  std::vector<float> x(n), y(n), a(n), ur(n), z(n), key((size_t)n * 2);
  std::vector<int32_t> oct(n), node(n);
  std::vector<uint8_t> d((size_t)n * 32), mp(n);
  rd(f, x.data(), n); rd(f, y.data(), n); rd(f, oct.data(), n); rd(f, a.data(), n); rd(f, d.data(), d.size());
  rd(f, node.data(), n); rd(f, mp.data(), n); rd(f, ur.data(), n); rd(f, z.data(), n); rd(f, key.data(), key.size());
  kf.mDescriptors.create(n, 32, CV_8U);
  kf.mvKeysUn.resize(n);
  kf.mvKeys.resize(n);
  kf.mvuRight = ur;
  kf.mvDepth = z;
  kf.mvpMapPoints.assign(n, nullptr);
  for (int i = 0; i < n; ++i) {
    std::memcpy(kf.mDescriptors.ptr<uint8_t>(i), &d[(size_t)i * 32], 32);
    kf.mvKeysUn[i] = cv::KeyPoint(x[i], y[i], 31.f, a[i], 0.f, oct[i]);
    kf.mvKeys[i] = cv::KeyPoint(key[2 * i], key[2 * i + 1], 31.f, a[i], 0.f, oct[i]);
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
  const int nkf = hdr[0], stopBefore = hdr[3];
  const bool coarse = hdr[1] != 0, farPoints = hdr[2] != 0;
  Camera cam;
  rd(in, cam.k, 4);
  float par[4];                           // bf, mb, thFar, scaleFactor
  rd(in, par, 4);
  KeyFrame kf1;
  fill(in, kf1, &cam, par);
  std::vector<std::unique_ptr<KeyFrame>> kfs;
  for (int k = 0; k < nkf; ++k) {
    kfs.emplace_back(new KeyFrame());
    kfs.back()->id = k + 1;
    fill(in, *kfs.back(), &cam, par);
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

    std::vector<KeyFrame*> vpNeighKFs;
    for (auto& k : kfs) vpNeighKFs.push_back(k.get());
    Atlas atlas;
    std::list<MapPoint*> recent;
    int asked = 0;
    const int created = ORB_SLAM3::PliCreateNewMapPoints<MapPoint>(&kf1, vpNeighKFs, &atlas, recent, coarse, farPoints, par[2], [&]() {
      ++asked;                            // asked before neighbour `asked` is applied
      logCall(7, asked, 0, 0);
      return asked == stopBefore;
    });
    for (MapPoint* p : recent) logCall(6, p->serial, 0, 0);
    // a keyframe of two cameras is refused
    KeyFrame two = kf1;
    two.mpCamera2 = &cam;
    bool threw = false;
    try {
      ORB_SLAM3::PliCreateNewMapPoints<MapPoint>(&two, vpNeighKFs, &atlas, recent, coarse, farPoints, par[2], [] { return false; });
    } catch (const std::logic_error&) { threw = true; }
    if (!threw && nkf > 0) { std::fprintf(stderr, "a keyframe of two cameras was accepted\n"); return 3; }

    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const int32_t head[2] = {created, (int32_t)(g_log.size() / 4)};
    std::fwrite(head, 4, 2, out);
    std::fwrite(g_log.data(), 4, g_log.size(), out);
    std::fwrite(g_pos.data(), 4, g_pos.size(), out);
    for (int k = 0; k < nkf; ++k) {
      float R1[9], t1[3], R2[9], t2[3], cw[3], g[11];
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { R1[i * 3 + j] = kf1.Rcw.at<float>(i, j); R2[i * 3 + j] = kfs[k]->Rcw.at<float>(i, j); }
        t1[i] = kf1.tcw.at<float>(i); t2[i] = kfs[k]->tcw.at<float>(i); cw[i] = kf1.Ow.at<float>(i);
      }
      ORB_SLAM3::pli_detail::triangulationGeometry(R1, t1, cw, cam.k, R2, t2, cam.k, g, g + 9);
      std::fwrite(g, 4, 11, out);
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
