// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over the reference's own src/ORBmatcher.cc, src/CameraModels/Pinhole.cpp, src/CameraModels/KannalaBrandt8.cpp and
// Thirdparty/DBoW2/DBoW2/FeatureVector.cpp, which oracle/Makefile compiles from the reference tree (never copied) against
// match_shim/ (pli_match_shim.hpp: what that stand-in states and what the pin therefore covers).
//
//   pli_ref_match CASE RESULT
//   pli_ref_match --functions        prints the names "fn" may take, one per line (a caller asks this before it relies on a
//                                    function that a program built from an earlier recipe does not have)
//
// CASE and RESULT are files of named arrays (tests/helpers_match_ref.py writes and reads them): "PLIM", int32 count, then per
// array: int32 name length, the name, int32 type (0: uint8, 1: int32, 2: float32, 3: float64), int32 ndim, ndim x int64 extent,
// the elements.
//
// A case holds ONE call (SearchForInitialization: a chain of calls) of the function "fn" names:
//   fn        the function (below), as bytes
//   params    float64: nnratio, checkOrientation, then the function's own
//   mp_*      the MapPoints of the case, ONE array of objects, so that pointer order is index order (ORBmatcher.cc keeps sets of
//             pointers): pos[n,3], normal[n,3], desc[n,32], bad[n], min_dist_inv[n], max_dist_inv[n] (what the getters return),
//             max_dist[n], nobs[n], in_kf[tables, n] (IsInKeyFrame), track[n,8] (mbTrackInView, mTrackProjX, mTrackProjY,
//             mTrackProjXR, mTrackDepth, mnTrackScaleLevel, mTrackViewCos, unused)
//   t<k>_*    table k, held both as a Frame and as a KeyFrame (again one array each): x, y, octave, angle, desc[n,32], uright (-1
//             when absent), node (the FeatureVector node that lists the feature, -1: none), mp (index of its MapPoint, -1: NULL),
//             outlier, cam (fx fy cx cy bf minX maxX minY maxY mb), sf / sigma2 / inv_sigma2 [levels], logsf, and either Tcw[4,4]
//             or R[3,3], t[3], Ow[3]; a two-camera table has nleft[1] (rows [0, nleft) are mvKeys, the rest mvKeysRight), kb1[8], kb2[8]
//             (the KannalaBrandt8 parameters of mpCamera, mpCamera2) and Tlr[3,4] besides
//   list, matched, found, points_kf, Scw, prev: the function's arguments (indices of MapPoints / tables, -1: NULL)
// One function runs no reference code: "area" (kp, nleft, bounds, q -> idx, start; see areaOfStandIn below) answers with the stand-in's
// own grid assignment and GetFeaturesInArea, so that they can be held to what the reference's Frame.cc returned (pli_ref_stereo).
// RESULT records what the caller of the reference function can see: "ret", and per function the containers named below, pointers
// as indices.
#include "ORBmatcher.h"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace ORB_SLAM3;

namespace {

struct Arr {
  int32_t type = 0;
  std::vector<int64_t> shape;
  std::vector<unsigned char> data;
  size_t count() const { size_t n = 1; for (int64_t s : shape) n *= (size_t)s; return n; }
};
const size_t kElem[4] = {1, 4, 4, 8};
typedef std::map<std::string, Arr> Bag;

void die(const std::string& what) { std::fprintf(stderr, "pli_ref_match: %s\n", what.c_str()); std::exit(2); }

Bag readBag(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) die(std::string("cannot open ") + path);
  auto get = [&](void* p, size_t n) { if (n && std::fread(p, 1, n, f) != n) die("short case file"); };
  char magic[4];
  int32_t count = 0;
  get(magic, 4); get(&count, 4);
  if (std::memcmp(magic, "PLIM", 4) != 0 || count < 0 || count > 4096) die("not a case file");
  Bag bag;
  for (int i = 0; i < count; ++i) {
    int32_t len = 0, ndim = 0;
    get(&len, 4);
    if (len <= 0 || len > 256) die("bad name");
    std::string name((size_t)len, '\0');
    get(&name[0], (size_t)len);
    Arr a;
    get(&a.type, 4); get(&ndim, 4);
    if (a.type < 0 || a.type > 3 || ndim < 0 || ndim > 4) die("bad array header: " + name);
    a.shape.resize((size_t)ndim);
    get(a.shape.data(), (size_t)ndim * 8);
    for (int64_t s : a.shape) if (s < 0 || s > (1 << 24)) die("bad extent: " + name);
    if (a.count() > ((size_t)1 << 26)) die("array too large: " + name);
    a.data.resize(a.count() * kElem[a.type]);
    get(a.data.data(), a.data.size());
    bag[name] = a;
  }
  std::fclose(f);
  return bag;
}

void writeBag(const char* path, const Bag& bag) {
  FILE* f = std::fopen(path, "wb");
  if (!f) die(std::string("cannot write ") + path);
  auto put = [&](const void* p, size_t n) { if (n && std::fwrite(p, 1, n, f) != n) die("write failed"); };
  const int32_t count = (int32_t)bag.size();
  put("PLIM", 4); put(&count, 4);
  for (const auto& kv : bag) {
    const int32_t len = (int32_t)kv.first.size(), ndim = (int32_t)kv.second.shape.size();
    put(&len, 4); put(kv.first.data(), kv.first.size());
    put(&kv.second.type, 4); put(&ndim, 4);
    put(kv.second.shape.data(), (size_t)ndim * 8);
    put(kv.second.data.data(), kv.second.data.size());
  }
  if (std::fclose(f) != 0) die("write failed");
}

Arr ints(const std::vector<int32_t>& v, std::vector<int64_t> shape = {}) {
  Arr a;
  a.type = 1;
  a.shape = shape.empty() ? std::vector<int64_t>{(int64_t)v.size()} : shape;
  a.data.resize(v.size() * 4);
  if (!v.empty()) std::memcpy(a.data.data(), v.data(), v.size() * 4);
  return a;
}
Arr floats(const std::vector<float>& v, std::vector<int64_t> shape) {
  Arr a;
  a.type = 2;
  a.shape = shape;
  a.data.resize(v.size() * 4);
  if (!v.empty()) std::memcpy(a.data.data(), v.data(), v.size() * 4);
  return a;
}

struct Case {
  Bag bag;
  bool has(const std::string& n) const { return bag.count(n) != 0; }
  const Arr& arr(const std::string& n, int type, size_t count = (size_t)-1) const {
    auto it = bag.find(n);
    if (it == bag.end()) die("missing array " + n);
    if (it->second.type != type) die("wrong type: " + n);
    if (count != (size_t)-1 && it->second.count() != count) die("wrong size: " + n);
    return it->second;
  }
  const float* f32(const std::string& n, size_t count) const { return reinterpret_cast<const float*>(arr(n, 2, count).data.data()); }
  const int32_t* i32(const std::string& n, size_t count) const { return reinterpret_cast<const int32_t*>(arr(n, 1, count).data.data()); }
  const unsigned char* u8(const std::string& n, size_t count) const { return arr(n, 0, count).data.data(); }
  size_t len(const std::string& n) const { auto it = bag.find(n); if (it == bag.end()) die("missing array " + n); return it->second.shape.empty() ? 1 : (size_t)it->second.shape[0]; }
};

cv::Mat matOf(const float* p, int rows, int cols) {
  cv::Mat m(rows, cols, CV_32F);
  for (int i = 0; i < rows * cols; ++i) m.at<float>(i / cols, i % cols) = p[i];
  return m;
}

// the objects of a case; the vectors are sized once and never grow, so that the addresses order as the indices do
struct World {
  std::vector<MapPoint> mps;
  std::vector<Frame> frames;
  std::vector<KeyFrame> kfs;
  std::vector<GeometricCamera*> cams;
  ~World() { for (GeometricCamera* c : cams) delete c; }
  MapPoint* mp(int i) { if (i >= (int)mps.size()) die("map point index out of range"); return i < 0 ? nullptr : &mps[(size_t)i]; }
  int index(MapPoint* p) const { return p ? p->index : -1; }
};

void fillTable(const Case& c, const std::string& pre, ShimTable& T, World& W, int k) {
  const size_t n = c.len(pre + "x");
  T.index = k;
  T.N = (int)n;
  const float *x = c.f32(pre + "x", n), *y = c.f32(pre + "y", n), *angle = c.f32(pre + "angle", n);
  const int32_t* octave = c.i32(pre + "octave", n);
  T.mvKeysUn.resize(n);
  for (size_t i = 0; i < n; ++i) {
    cv::KeyPoint& kp = T.mvKeysUn[i];
    kp.pt.x = x[i]; kp.pt.y = y[i]; kp.octave = octave[i]; kp.angle = angle[i]; kp.size = 31.f;
  }
  T.mvKeys = T.mvKeysUn;
  const unsigned char* desc = c.u8(pre + "desc", n * 32);
  T.mDescriptors.create((int)n, 32, CV_8U);
  if (n) std::memcpy(T.mDescriptors.data, desc, n * 32);
  T.mvuRight.assign(n, -1.f);
  if (c.has(pre + "uright")) T.mvuRight.assign(c.f32(pre + "uright", n), c.f32(pre + "uright", n) + n);
  if (c.has(pre + "node")) {
    const int32_t* node = c.i32(pre + "node", n);
    for (size_t i = 0; i < n; ++i)
      if (node[i] >= 0) T.mFeatVec.addFeature((DBoW2::NodeId)node[i], (unsigned int)i);      // the reference's own FeatureVector.cpp
  }
  T.mvpMapPoints.assign(n, nullptr);
  if (c.has(pre + "mp")) {
    const int32_t* mp = c.i32(pre + "mp", n);
    for (size_t i = 0; i < n; ++i) T.mvpMapPoints[i] = W.mp(mp[i]);
  }
  T.mvbOutlier.assign(n, false);
  if (c.has(pre + "outlier")) {
    const unsigned char* o = c.u8(pre + "outlier", n);
    for (size_t i = 0; i < n; ++i) T.mvbOutlier[i] = o[i] != 0;
  }
  const float* cam = c.f32(pre + "cam", 10);
  T.fx = cam[0]; T.fy = cam[1]; T.cx = cam[2]; T.cy = cam[3]; T.mbf = cam[4];
  T.mnMinX = cam[5]; T.mnMaxX = cam[6]; T.mnMinY = cam[7]; T.mnMaxY = cam[8]; T.mb = cam[9];
  const size_t nl = c.len(pre + "sf");
  T.mnScaleLevels = (int)nl;
  T.mvScaleFactors.assign(c.f32(pre + "sf", nl), c.f32(pre + "sf", nl) + nl);
  T.mvLevelSigma2.assign(c.f32(pre + "sigma2", nl), c.f32(pre + "sigma2", nl) + nl);
  T.mvInvLevelSigma2.assign(c.f32(pre + "inv_sigma2", nl), c.f32(pre + "inv_sigma2", nl) + nl);
  T.mfLogScaleFactor = c.f32(pre + "logsf", 1)[0];
  if (c.has(pre + "Tcw")) {
    T.mTcw = matOf(c.f32(pre + "Tcw", 16), 4, 4);
    T.mRcw = T.mTcw.rowRange(0, 3).colRange(0, 3).clone();
    T.mtcw = T.mTcw.rowRange(0, 3).col(3).clone();
  }
  if (c.has(pre + "R")) {
    T.mRcw = matOf(c.f32(pre + "R", 9), 3, 3);
    T.mtcw = matOf(c.f32(pre + "t", 3), 3, 1);
    T.mOw = matOf(c.f32(pre + "Ow", 3), 3, 1);
  }
  if (c.has(pre + "nleft")) {
    // a two-camera table: rows [0, nleft) are mvKeys, the rest mvKeysRight (camera-local indices); both cameras KannalaBrandt8
    // (kb1, kb2: fx fy cx cy k0 k1 k2 k3); Tlr[3,4].  The two grids are filled when the table has image bounds.  mvuRight has
    // Nleft entries, all -1, as Frame.cc:1589 leaves it for such a rig: Fuse reads mvuRight[idx] with the camera-local idx of
    // EITHER camera (:1533), so a case with bRight must keep Nright <= Nleft (the reference reads past the vector otherwise).
    const int nleft = c.i32(pre + "nleft", 1)[0];
    if (nleft < 0 || nleft > (int)n) die("bad nleft");
    T.mvKeysRight.assign(T.mvKeys.begin() + nleft, T.mvKeys.end());
    T.mvKeys.resize((size_t)nleft);
    const float *k1 = c.f32(pre + "kb1", 8), *k2 = c.f32(pre + "kb2", 8);
    // pinhole[4] (fx fy cx cy): mpCamera is a Pinhole instead, for cases that need a projection which is exact in float
    if (c.has(pre + "pinhole")) W.cams.push_back(new Pinhole(std::vector<float>(c.f32(pre + "pinhole", 4), c.f32(pre + "pinhole", 4) + 4)));
    else W.cams.push_back(new KannalaBrandt8(std::vector<float>(k1, k1 + 8)));
    T.mpCamera = W.cams.back();
    W.cams.push_back(new KannalaBrandt8(std::vector<float>(k2, k2 + 8)));
    T.mpCamera2 = W.cams.back();
    T.mTlr = matOf(c.f32(pre + "Tlr", 12), 3, 4);
    if (c.has(pre + "Trl")) T.mTrl = matOf(c.f32(pre + "Trl", 12), 3, 4);
    T.mvuRight.assign((size_t)nleft, -1.f);
    T.mvLeftToRightMatch.assign((size_t)nleft, -1);                  // l2r[nleft] / r2l[n - nleft]: Frame::ComputeStereoFishEyeMatches' tables
    T.mvRightToLeftMatch.assign(n - (size_t)nleft, -1);
    if (c.has(pre + "l2r")) T.mvLeftToRightMatch.assign(c.i32(pre + "l2r", (size_t)nleft), c.i32(pre + "l2r", (size_t)nleft) + nleft);
    if (c.has(pre + "r2l")) T.mvRightToLeftMatch.assign(c.i32(pre + "r2l", n - (size_t)nleft), c.i32(pre + "r2l", n - (size_t)nleft) + (n - (size_t)nleft));
    if (T.mnMaxX > T.mnMinX && T.mnMaxY > T.mnMinY) T.AssignFeaturesToGridTwoCameras(nleft);
    return;
  }
  Pinhole* cam1 = new Pinhole(std::vector<float>{T.fx, T.fy, T.cx, T.cy});
  W.cams.push_back(cam1);
  T.mpCamera = cam1;
  T.AssignFeaturesToGrid();
}

void build(const Case& c, World& W) {
  const size_t nmp = c.has("mp_pos") ? c.len("mp_pos") : 0;
  int ntab = 0;
  while (c.has("t" + std::to_string(ntab) + "_x")) ++ntab;
  W.mps.resize(nmp);
  W.frames.resize((size_t)ntab);
  W.kfs.resize((size_t)ntab);
  if (nmp) {
    const float *pos = c.f32("mp_pos", nmp * 3), *normal = c.f32("mp_normal", nmp * 3);
    const unsigned char *desc = c.u8("mp_desc", nmp * 32), *bad = c.u8("mp_bad", nmp);
    const float *mn = c.f32("mp_min_dist_inv", nmp), *mx = c.f32("mp_max_dist_inv", nmp), *md = c.f32("mp_max_dist", nmp);
    const int32_t* nobs = c.i32("mp_nobs", nmp);
    const float* track = c.has("mp_track") ? c.f32("mp_track", nmp * 8) : nullptr;
    for (size_t i = 0; i < nmp; ++i) {
      MapPoint& P = W.mps[i];
      P.index = (int)i;
      P.mWorldPos = matOf(pos + 3 * i, 3, 1);
      P.mNormalVector = matOf(normal + 3 * i, 3, 1);
      P.mDescriptor.create(1, 32, CV_8U);
      std::memcpy(P.mDescriptor.data, desc + 32 * i, 32);
      P.mbBad = bad[i] != 0;
      P.mMinDistInv = mn[i]; P.mMaxDistInv = mx[i]; P.mfMaxDistance = md[i];
      P.nObs = nobs[i];
      if (track) {
        const float* t = track + 8 * i;
        P.mbTrackInView = t[0] != 0.f; P.mTrackProjX = t[1]; P.mTrackProjY = t[2]; P.mTrackProjXR = t[3]; P.mTrackDepth = t[4];
        P.mnTrackScaleLevel = (int)t[5]; P.mTrackViewCos = t[6];
      }
      if (c.has("mp_track_r")) {     // [n,6]: mbTrackInViewR, mTrackProjXR, mTrackProjYR, mnTrackScaleLevelR, mTrackViewCosR, mTrackDepthR
        const float* t = c.f32("mp_track_r", nmp * 6) + 6 * i;
        P.mbTrackInViewR = t[0] != 0.f; P.mTrackProjXR = t[1]; P.mTrackProjYR = t[2]; P.mnTrackScaleLevelR = (int)t[3];
        P.mTrackViewCosR = t[4]; P.mTrackDepthR = t[5];
      }
    }
  }
  for (int k = 0; k < ntab; ++k) {
    const std::string pre = "t" + std::to_string(k) + "_";
    fillTable(c, pre, W.frames[(size_t)k], W, k);
    fillTable(c, pre, W.kfs[(size_t)k], W, k);
    if (c.has(pre + "nleft")) W.frames[(size_t)k].Nleft = W.kfs[(size_t)k].NLeft = c.i32(pre + "nleft", 1)[0];
  }
  if (c.has("mp_in_kf")) {
    const unsigned char* in = c.u8("mp_in_kf", (size_t)ntab * nmp);
    for (int k = 0; k < ntab; ++k)
      for (size_t i = 0; i < nmp; ++i)
        if (in[(size_t)k * nmp + i]) W.mps[i].mObservations[&W.kfs[(size_t)k]] = 0;
  }
}

std::vector<MapPoint*> pointList(const Case& c, World& W, const std::string& name) {
  const size_t n = c.len(name);
  const int32_t* idx = c.i32(name, n);
  std::vector<MapPoint*> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = W.mp(idx[i]);
  return v;
}
std::vector<int32_t> indices(const World& W, const std::vector<MapPoint*>& v) {
  std::vector<int32_t> out(v.size());
  for (size_t i = 0; i < v.size(); ++i) out[i] = W.index(v[i]);
  return out;
}

// "area": no reference code at all -- the STAND-IN's own Frame::AssignFeaturesToGrid / GetFeaturesInArea (match_shim), on the case
// format of pli_ref_stereo's function of that name (kp [n,3]: x, y, octave; nleft [1]; bounds [4]; q [m,6]: x, y, r, minLevel,
// maxLevel, bRight -> idx, start).  tests/test_ref_pin_stereo.py holds its answers to what the reference's own Frame.cc returned.
void areaOfStandIn(const Case& c, Bag& out) {
  const Arr& ka = c.arr("kp", 2);
  if (ka.shape.size() != 2 || ka.shape[1] != 3) die("area: kp must be [n,3]");
  const size_t n = (size_t)ka.shape[0];
  const float* k = c.f32("kp", n * 3);
  const int nleft = c.i32("nleft", 1)[0];
  const float* b = c.f32("bounds", 4);
  Frame F;
  F.N = (int)n;
  std::vector<cv::KeyPoint> kp(n);
  for (size_t i = 0; i < n; ++i) { kp[i].pt.x = k[3 * i]; kp[i].pt.y = k[3 * i + 1]; kp[i].octave = (int)k[3 * i + 2]; }
  F.mnMinX = b[0]; F.mnMaxX = b[1]; F.mnMinY = b[2]; F.mnMaxY = b[3];
  if (nleft == -1) {
    F.mvKeysUn = kp; F.mvKeys = kp;
    F.AssignFeaturesToGrid();
  } else {
    if (nleft < 0 || (size_t)nleft > n) die("area: nleft outside the table");
    F.Nleft = nleft;
    F.mvKeys.assign(kp.begin(), kp.begin() + nleft);
    F.mvKeysRight.assign(kp.begin() + nleft, kp.end());
    F.AssignFeaturesToGridTwoCameras(nleft);
  }
  const Arr& qa = c.arr("q", 2);
  if (qa.shape.size() != 2 || qa.shape[1] != 6) die("area: q must be [m,6]");
  const size_t m = (size_t)qa.shape[0];
  const float* q = c.f32("q", m * 6);
  std::vector<int32_t> idx, start(1, 0);
  for (size_t i = 0; i < m; ++i) {
    const float* r = q + 6 * i;
    for (size_t j : F.GetFeaturesInArea(r[0], r[1], r[2], (int)r[3], (int)r[4], r[5] != 0.f)) idx.push_back((int32_t)j);
    start.push_back((int32_t)idx.size());
  }
  out["idx"] = ints(idx); out["start"] = ints(start);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--functions") {
    for (const char* f : {"fuse", "fuse_sim3", "sim3", "sim3_kfs", "reloc", "bow", "bow_kf", "init", "tri", "frame", "local", "kb8", "tri2",
                          "bow2", "fuse2", "local2", "frame2", "area"})
      std::printf("%s\n", f);
    return 0;
  }
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASE RESULT\n", argv[0]); return 2; }
  Case c;
  c.bag = readBag(argv[1]);
  const Arr& fnArr = c.arr("fn", 0);
  const std::string fn(fnArr.data.begin(), fnArr.data.end());
  if (fn == "area") {
    Bag res;
    areaOfStandIn(c, res);
    writeBag(argv[2], res);
    return 0;
  }
  const Arr& pa = c.arr("params", 3);
  const double* params = reinterpret_cast<const double*>(pa.data.data());
  const size_t np = pa.count();
  auto param = [&](size_t i) { if (i >= np) die("missing parameter"); return params[i]; };
  World W;
  build(c, W);
  ORBmatcher matcher((float)param(0), param(1) != 0.0);
  Bag out;
  int ret = 0;
  auto table = [&](size_t k) { if (k >= W.kfs.size()) die("missing table"); return k; };

  if (fn == "fuse2") {                             // Fuse(pKF, vpMapPoints, th, bRight): params[2] = th, params[3] = bRight
    KeyFrame* pKF = &W.kfs[table(0)];
    const bool bRight = param(3) != 0.0;
    if (!pKF->mpCamera2) die("fuse2 needs a two-camera table");
    if (bRight && pKF->mvKeysRight.size() > pKF->mvuRight.size()) die("fuse2 with bRight needs Nright <= Nleft (mvuRight has Nleft entries)");
    cv::shim_detail::divisionFactorInFloat() = true;
    const std::vector<MapPoint*> list = pointList(c, W, "list");
    ShimLog::get().on = true;
    ret = matcher.Fuse(pKF, list, (float)param(2), bRight);
    ShimLog::get().on = false;
    out["ops"] = ints(ShimLog::get().ops, {(int64_t)ShimLog::get().ops.size() / 3, 3});
    out["kf_mp"] = ints(indices(W, pKF->mvpMapPoints));
  } else if (fn == "fuse") {                       // Fuse(pKF, vpMapPoints, th): params[2] = th
    KeyFrame* pKF = &W.kfs[table(0)];
    const std::vector<MapPoint*> list = pointList(c, W, "list");
    ShimLog::get().on = true;
    ret = matcher.Fuse(pKF, list, (float)param(2));
    ShimLog::get().on = false;
    out["ops"] = ints(ShimLog::get().ops, {(int64_t)ShimLog::get().ops.size() / 3, 3});
    out["kf_mp"] = ints(indices(W, pKF->mvpMapPoints));
  } else if (fn == "fuse_sim3") {                  // Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): params[2] = th
    KeyFrame* pKF = &W.kfs[table(0)];
    const std::vector<MapPoint*> list = pointList(c, W, "list");
    std::vector<MapPoint*> replace(list.size(), nullptr);
    ShimLog::get().on = true;
    ret = matcher.Fuse(pKF, matOf(c.f32("Scw", 16), 4, 4), list, (float)param(2), replace);
    ShimLog::get().on = false;
    out["ops"] = ints(ShimLog::get().ops, {(int64_t)ShimLog::get().ops.size() / 3, 3});
    out["replace"] = ints(indices(W, replace));
    out["kf_mp"] = ints(indices(W, pKF->mvpMapPoints));
  } else if (fn == "sim3" || fn == "sim3_kfs") {   // SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratio)
    KeyFrame* pKF = &W.kfs[table(0)];
    const std::vector<MapPoint*> list = pointList(c, W, "list");
    std::vector<MapPoint*> matched = pointList(c, W, "matched");
    if (fn == "sim3") {
      ret = matcher.SearchByProjection(pKF, matOf(c.f32("Scw", 16), 4, 4), list, matched, (int)param(2), (float)param(3));
    } else {
      const int32_t* pk = c.i32("points_kf", list.size());
      std::vector<KeyFrame*> pointsKF(list.size()), matchedKF(matched.size(), nullptr);
      for (size_t i = 0; i < list.size(); ++i) pointsKF[i] = &W.kfs[table((size_t)pk[i])];
      ret = matcher.SearchByProjection(pKF, matOf(c.f32("Scw", 16), 4, 4), list, pointsKF, matched, matchedKF, (int)param(2), (float)param(3));
      std::vector<int32_t> mk(matchedKF.size());
      for (size_t i = 0; i < mk.size(); ++i) mk[i] = matchedKF[i] ? matchedKF[i]->index : -1;
      out["matched_kf"] = ints(mk);
    }
    out["matched"] = ints(indices(W, matched));
  } else if (fn == "reloc") {                      // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
    Frame& F = W.frames[table(0)];
    KeyFrame* pKF = &W.kfs[table(1)];
    const std::vector<MapPoint*> found = pointList(c, W, "found");
    const std::set<MapPoint*> sFound(found.begin(), found.end());
    ret = matcher.SearchByProjection(F, pKF, sFound, (float)param(2), (int)param(3));
    out["frame_mp"] = ints(indices(W, F.mvpMapPoints));
  } else if (fn == "bow" || fn == "bow2") {        // SearchByBoW(pKF, F, vpMapPointMatches); bow2: F.Nleft != -1 (a two-camera table)
    if (fn == "bow2" && (W.frames[table(1)].Nleft == -1 || !W.frames[table(1)].mpCamera2)) die("bow2 needs a two-camera frame");
    std::vector<MapPoint*> matches;
    ret = matcher.SearchByBoW(&W.kfs[table(0)], W.frames[table(1)], matches);
    out["matches"] = ints(indices(W, matches));
  } else if (fn == "bow_kf") {                     // SearchByBoW(pKF1, pKF2, vpMatches12)
    std::vector<MapPoint*> matches;
    ret = matcher.SearchByBoW(&W.kfs[table(0)], &W.kfs[table(1)], matches);
    out["matches"] = ints(indices(W, matches));
  } else if (fn == "init") {                       // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize), F2 = tables 1, 2, ...
    Frame& F1 = W.frames[table(0)];
    const size_t n1 = (size_t)F1.N;
    const float* prev = c.f32("prev", n1 * 2);
    std::vector<cv::Point2f> vbPrevMatched(n1);
    for (size_t i = 0; i < n1; ++i) vbPrevMatched[i] = cv::Point2f(prev[2 * i], prev[2 * i + 1]);
    std::vector<int32_t> rets, all12;
    std::vector<float> allPrev;
    for (size_t k = 1; k < W.frames.size(); ++k) {
      std::vector<int> vnMatches12;
      rets.push_back(matcher.SearchForInitialization(F1, W.frames[k], vbPrevMatched, vnMatches12, (int)param(2)));
      all12.insert(all12.end(), vnMatches12.begin(), vnMatches12.end());
      for (const cv::Point2f& p : vbPrevMatched) { allPrev.push_back(p.x); allPrev.push_back(p.y); }
    }
    ret = rets.empty() ? 0 : rets.back();
    out["rets"] = ints(rets);
    out["matches12"] = ints(all12, {(int64_t)rets.size(), (int64_t)n1});
    out["prev"] = floats(allPrev, {(int64_t)rets.size(), (int64_t)n1, 2});
  } else if (fn == "tri" || fn == "tri2") {        // SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse);
    // tri2: both tables carry nleft (mpCamera2 set on both keyframes)
    if (fn == "tri2") {
      if (!W.kfs[table(0)].mpCamera2 || !W.kfs[table(1)].mpCamera2) die("tri2 needs two-camera tables");
      cv::shim_detail::divisionFactorInFloat() = true;
    }
    std::vector<std::pair<size_t, size_t>> pairs;
    ret = matcher.SearchForTriangulation(&W.kfs[table(0)], &W.kfs[table(1)], cv::Mat(), pairs, param(2) != 0.0, param(3) != 0.0);
    std::vector<int32_t> flat;
    for (const auto& p : pairs) { flat.push_back((int32_t)p.first); flat.push_back((int32_t)p.second); }
    out["pairs"] = ints(flat, {(int64_t)pairs.size(), 2});
    if (fn == "tri2") {
      // not an output of the reference function: the right-pose getters of the stand-in (KeyFrame.cc:1354-1373 restated there) and
      // the four relative poses of ORBmatcher.cc:995-1003 formed HERE over the stand-in's cv::Mat, ll lr rl rr, R12 then t12, so
      // that the host arithmetic of the restatements and of the adapter can be held to the same bits
      KeyFrame *k1 = &W.kfs[table(0)], *k2 = &W.kfs[table(1)];
      std::vector<float> rel, right;
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
          const cv::Mat Ra = a ? k1->GetRightRotation() : k1->GetRotation(), ta = a ? k1->GetRightTranslation() : k1->GetTranslation();
          const cv::Mat Rb = b ? k2->GetRightRotation() : k2->GetRotation(), tb = b ? k2->GetRightTranslation() : k2->GetTranslation();
          const cv::Mat R12 = Ra * Rb.t(), t12 = Ra * (-Rb.t() * tb) + ta;
          for (int i = 0; i < 9; ++i) rel.push_back(R12.at<float>(i / 3, i % 3));
          for (int i = 0; i < 3; ++i) rel.push_back(t12.at<float>(i));
        }
      for (KeyFrame* k : {k1, k2}) {
        const cv::Mat R = k->GetRightRotation(), t = k->GetRightTranslation(), O = k->GetRightCameraCenter();
        for (int i = 0; i < 9; ++i) right.push_back(R.at<float>(i / 3, i % 3));
        for (int i = 0; i < 3; ++i) right.push_back(t.at<float>(i));
        for (int i = 0; i < 3; ++i) right.push_back(O.at<float>(i));
      }
      out["rel"] = floats(rel, {4, 12});
      out["right_poses"] = floats(right, {2, 15});
    }
  } else if (fn == "frame" || fn == "frame2") {    // SearchByProjection(CurrentFrame, LastFrame, th, bMono); frame2: CurrentFrame.Nleft != -1
    Frame& F = W.frames[table(0)];
    if (fn == "frame2" && (F.Nleft == -1 || F.mTrl.empty())) die("frame2 needs a two-camera current frame with Trl");
    ret = matcher.SearchByProjection(F, W.frames[table(1)], (float)param(2), param(3) != 0.0);
    out["frame_mp"] = ints(indices(W, F.mvpMapPoints));
  } else if (fn == "local" || fn == "local2") {    // SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints); local2: F.Nleft != -1
    Frame& F = W.frames[table(0)];
    if (fn == "local2" && (F.Nleft == -1 || !c.has("mp_track_r"))) die("local2 needs a two-camera frame and mp_track_r");
    ret = matcher.SearchByProjection(F, pointList(c, W, "list"), (float)param(2), param(3) != 0.0, (float)param(4));
    out["frame_mp"] = ints(indices(W, F.mvpMapPoints));
  } else if (fn == "kb8") {                        // no matcher: the compiled KannalaBrandt8 members on tables of points, pixels and pairs
    // cam1[8], cam2[8]: fx fy cx cy k0 k1 k2 k3; points[n,3], pixels[m,2]: project / unproject of BOTH cameras; kp1[k,2] (camera 1),
    // kp2[k,2] (camera 2), R12[9], t12[3], sigma[k], unc[k]: cam1.TriangulateMatches(&cam2, ...) -> tri_ret[k], tri_p3d[k,3]
    // (zeros where p3D stayed empty), and the two rays it starts from: tri_r1[k,3] = cam1.unproject(kp1), tri_r2[k,3] = cam2.unproject(kp2)
    cv::shim_detail::divisionFactorInFloat() = true;
    const float *c1 = c.f32("cam1", 8), *c2 = c.f32("cam2", 8);
    KannalaBrandt8 cam1(std::vector<float>(c1, c1 + 8)), cam2(std::vector<float>(c2, c2 + 8));
    KannalaBrandt8* cams[2] = {&cam1, &cam2};
    const size_t n = c.len("points"), m = c.len("pixels"), k = c.len("kp1");
    const float *pts = c.f32("points", n * 3), *pix = c.f32("pixels", m * 2);
    for (int e = 0; e < 2; ++e) {
      std::vector<float> proj(n * 2), unproj(m * 3);
      for (size_t i = 0; i < n; ++i) {
        const cv::Point2f uv = cams[e]->project(cv::Point3f(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
        proj[2 * i] = uv.x; proj[2 * i + 1] = uv.y;
      }
      for (size_t i = 0; i < m; ++i) {
        const cv::Point3f r = cams[e]->unproject(cv::Point2f(pix[2 * i], pix[2 * i + 1]));
        unproj[3 * i] = r.x; unproj[3 * i + 1] = r.y; unproj[3 * i + 2] = r.z;
      }
      out[e ? "proj2" : "proj1"] = floats(proj, {(int64_t)n, 2});
      out[e ? "unproj2" : "unproj1"] = floats(unproj, {(int64_t)m, 3});
    }
    const float *kp1 = c.f32("kp1", k * 2), *kp2 = c.f32("kp2", k * 2), *sigma = c.f32("sigma", k), *unc = c.f32("unc", k);
    const cv::Mat R12 = matOf(c.f32("R12", 9), 3, 3), t12 = matOf(c.f32("t12", 3), 3, 1);
    std::vector<float> triRet(k), triP(k * 3, 0.f), triR1(k * 3), triR2(k * 3);
    for (size_t i = 0; i < k; ++i) {
      cv::KeyPoint a, b;
      a.pt = cv::Point2f(kp1[2 * i], kp1[2 * i + 1]);
      b.pt = cv::Point2f(kp2[2 * i], kp2[2 * i + 1]);
      const cv::Point3f r1 = cam1.unproject(a.pt), r2 = cam2.unproject(b.pt);
      triR1[3 * i] = r1.x; triR1[3 * i + 1] = r1.y; triR1[3 * i + 2] = r1.z;
      triR2[3 * i] = r2.x; triR2[3 * i + 1] = r2.y; triR2[3 * i + 2] = r2.z;
      cv::Mat p3D;
      triRet[i] = cam1.TriangulateMatches(&cam2, a, b, R12, t12, sigma[i], unc[i], p3D);
      if (!p3D.empty())
        for (int j = 0; j < 3; ++j) triP[3 * i + (size_t)j] = p3D.at<float>(j);
    }
    out["tri_ret"] = floats(triRet, {(int64_t)k});
    out["tri_p3d"] = floats(triP, {(int64_t)k, 3});
    out["tri_r1"] = floats(triR1, {(int64_t)k, 3});
    out["tri_r2"] = floats(triR2, {(int64_t)k, 3});
  } else {
    die("unknown function " + fn);
  }
  out["ret"] = ints(std::vector<int32_t>{ret});
  writeBag(argv[2], out);
  return 0;
}
