// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over the reference's own src/ORBmatcher.cc, src/CameraModels/Pinhole.cpp and
// Thirdparty/DBoW2/DBoW2/FeatureVector.cpp, which oracle/Makefile compiles from the reference tree (never copied) against
// match_shim/ (pli_match_shim.hpp: what that stand-in states and what the pin therefore covers).
//
//   pli_ref_match CASE RESULT
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
//             or R[3,3], t[3], Ow[3]
//   list, matched, found, points_kf, Scw, prev: the function's arguments (indices of MapPoints / tables, -1: NULL)
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
  std::vector<Pinhole*> cams;
  ~World() { for (Pinhole* c : cams) delete c; }
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
    }
  }
  for (int k = 0; k < ntab; ++k) {
    const std::string pre = "t" + std::to_string(k) + "_";
    fillTable(c, pre, W.frames[(size_t)k], W, k);
    fillTable(c, pre, W.kfs[(size_t)k], W, k);
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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASE RESULT\n", argv[0]); return 2; }
  Case c;
  c.bag = readBag(argv[1]);
  const Arr& fnArr = c.arr("fn", 0);
  const std::string fn(fnArr.data.begin(), fnArr.data.end());
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

  if (fn == "fuse") {                              // Fuse(pKF, vpMapPoints, th): params[2] = th
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
  } else if (fn == "bow") {                        // SearchByBoW(pKF, F, vpMapPointMatches)
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
  } else if (fn == "tri") {                        // SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse)
    std::vector<std::pair<size_t, size_t>> pairs;
    ret = matcher.SearchForTriangulation(&W.kfs[table(0)], &W.kfs[table(1)], cv::Mat(), pairs, param(2) != 0.0, param(3) != 0.0);
    std::vector<int32_t> flat;
    for (const auto& p : pairs) { flat.push_back((int32_t)p.first); flat.push_back((int32_t)p.second); }
    out["pairs"] = ints(flat, {(int64_t)pairs.size(), 2});
  } else if (fn == "frame") {                      // SearchByProjection(CurrentFrame, LastFrame, th, bMono)
    Frame& F = W.frames[table(0)];
    ret = matcher.SearchByProjection(F, W.frames[table(1)], (float)param(2), param(3) != 0.0);
    out["frame_mp"] = ints(indices(W, F.mvpMapPoints));
  } else if (fn == "local") {                      // SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints)
    Frame& F = W.frames[table(0)];
    ret = matcher.SearchByProjection(F, pointList(c, W, "list"), (float)param(2), param(3) != 0.0, (float)param(4));
    out["frame_mp"] = ints(indices(W, F.mvpMapPoints));
  } else {
    die("unknown function " + fn);
  }
  out["ret"] = ints(std::vector<int32_t>{ret});
  writeBag(argv[2], out);
  return 0;
}
