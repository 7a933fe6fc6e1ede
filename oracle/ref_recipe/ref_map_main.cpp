// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over definitions of the reference's own src/Frame.cc (Frame::isInFrustum, isInFrustum_l),
// src/MapPoint.cc (MapPoint::ComputeDistinctiveDescriptors, PredictScale(dist, Frame*), Get{Min,Max}DistanceInvariance) and
// src/MapLine.cc (MapLine::ComputeDistinctiveDescriptors), src/LocalMapping.cc (CreateNewMapPoints, ComputeF12,
// SkewSymmetricMatrix) and src/KeyFrame.cc (UnprojectStereo), which oracle/Makefile (ref_map) cuts out of the reference tree at build
// time and compiles unmodified, next to the whole src/ORBmatcher.cc and src/CameraModels/*.cpp, against map_shim/pli_map_shim.hpp
// (what that stand-in states and what the pin therefore covers is written there).
//
//   pli_ref_map CASE RESULT
//   pli_ref_map --functions
//
// CASE and RESULT are the files of named arrays of pli_ref_match ("PLIM"; tests/helpers_match_ref.py writes and reads them).
// All map points, map lines and keyframes of a case are allocated from one array each, so that pointer order is index order
// (mObservations is keyed by pointer).  "fn" names the operation:
//
// frustum_points   params: nnratio, th, bFarPoints, thFarPoints.  mp_pos[n,3], mp_normal[n,3], mp_desc[n,32], mp_bad[n],
//                  mp_min_dist[n], mp_max_dist[n] (mfMinDistance, mfMaxDistance), mp_seen[n] (mnLastFrameSeen == the frame's id),
//                  mp_track[n,8] (the fields a point holds at entry: mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR,
//                  mTrackDepth, mnTrackScaleLevel, mTrackViewCos, unused).  The frame: f_cam[10] (fx fy cx cy bf minX maxX minY
//                  maxY mb), f_R[9], f_t[3], f_Ow[3], f_sf / f_sigma2 / f_inv_sigma2 [levels], f_logsf[1], f_x, f_y, f_octave,
//                  f_angle, f_desc[m,32], f_uright[m], f_occ[m] (0: NULL, 1: a map point with observations, 2: one without; their
//                  objects follow the list's in the array).
//                  The loop of Tracking.cc:3809-3827 is written out here (skip, isInFrustum(pMP, 0.5), count), then
//                  ORBmatcher(nnratio).SearchByProjection(F, list, th, bFarPoints, thFarPoints) runs whenever any point is in view.
//                  -> track[n,8] after the loop, n_to_match[1], frame_mp[m] (index of the object each row holds, -1: NULL), ret[1]
// frustum_lines    ml_sp[n,3], ml_ep[n,3] (float: the adapter's table; held as the reference's doubles), ml_bad[n], ml_seen[n], f_cam,
//                  f_R, f_t, f_Ow.  Tracking.cc:3862-3877.  mTrackProjeX / Y are zero before every call (the reference reads them
//                  uninitialised for mnTrackangle, which is not recorded).
//                  -> in_view[n], proj_s[n,2] (mTrackProjsX / Y), list[k] (the in-frustum list, in order), n_to_match[1]
// distinctive      params: lines (0: MapPoint and KeyFrame::mDescriptors, 1: MapLine and mDescriptors_l).  kf_desc[nkf,rows,32],
//                  kf_bad[nkf], ft_bad[nf], obs[k,3] (feature, keyframe, row).  ComputeDistinctiveDescriptors() of every feature.
//                  -> written[nf] (mDescriptor is not empty afterwards; it is empty at entry), desc[nf,32], row[nf]: the first
//                  position, in the order of vDescriptors (keyframes ascending, bad ones left out), whose descriptor mDescriptor equals
// new_map_points   params: mbMonocular, bCoarse (mbInertial with GetIniertialBA1() and not BA2), mbFarPoints, mThFarPoints.  cam[6] (fx fy
//                  cx cy bf mb), scale[1] (mfScaleFactor), sf / sigma2 [levels]; k0_* the current keyframe, k1_*, ... its neighbours in
//                  the order GetBestCovisibilityKeyFrames returns them: x, y, octave, angle (mvKeysUn), key[n,2] (mvKeys[i].pt),
//                  desc[n,32], node, has_mp, uright, depth (mvDepth), bf[1] (optional: this keyframe's mbf), pose[15] (Rcw, tcw, the stored Ow; Twc is Rcw.t() and that Ow).
//                  With kb1[8], kb2[8] and Tlr[3,4] every keyframe has two KannalaBrandt8 cameras (the branch :463-528): nleft[1] per keyframe,
//                  rows [0, nleft) are mvKeys, the rest mvKeysRight; key, uright and depth are not read (mvuRight is all -1).
//                  One whole LocalMapping::CreateNewMapPoints().
//                  -> created[m,3] (neighbour, idx1, idx2) and x3d[m,3] in mlpRecentAddedMapPoints order, desc[m,32] and desc_row[m]
//                  (0: mDescriptor is the current keyframe's row, 1: the neighbour's), pairs[p,3] (neighbour, idx1, idx2): vMatchedIndices
//                  as the loop saw it at every neighbour -- learnt without touching the cut text: the function is run on the
//                  neighbours before k in a world of its own, then the driver makes the search the loop would make next
#include "ORBmatcher.h"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace ORB_SLAM3;

// Frame::isInFrustum names it for a two-camera frame (Nleft != -1), which this driver never builds; it is not cut (it needs mRwc)
bool Frame::isInFrustumChecks(MapPoint*, float, bool) {
  std::fprintf(stderr, "pli_ref_map: isInFrustumChecks has no stand-in (one camera only)\n");
  std::abort();
}

namespace {

struct Arr {
  int32_t type = 0;
  std::vector<int64_t> shape;
  std::vector<unsigned char> data;
  size_t count() const { size_t n = 1; for (int64_t s : shape) n *= (size_t)s; return n; }
};
const size_t kElem[4] = {1, 4, 4, 8};
typedef std::map<std::string, Arr> Bag;

void die(const std::string& what) { std::fprintf(stderr, "pli_ref_map: %s\n", what.c_str()); std::exit(2); }

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

template <class T> Arr arrayOf(int32_t type, const std::vector<T>& v, std::vector<int64_t> shape = {}) {
  Arr a;
  a.type = type;
  a.shape = shape.empty() ? std::vector<int64_t>{(int64_t)v.size()} : shape;
  a.data.resize(v.size() * sizeof(T));
  if (!v.empty()) std::memcpy(a.data.data(), v.data(), v.size() * sizeof(T));
  return a;
}
Arr bytes(const std::vector<unsigned char>& v, std::vector<int64_t> shape = {}) { return arrayOf(0, v, shape); }
Arr ints(const std::vector<int32_t>& v, std::vector<int64_t> shape = {}) { return arrayOf(1, v, shape); }
Arr floats(const std::vector<float>& v, std::vector<int64_t> shape = {}) { return arrayOf(2, v, shape); }

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

// the frame of a frustum case: pose, camera, pyramid and, where the case has them, keypoints
void fillFrame(const Case& c, Frame& F, std::vector<GeometricCamera*>& cams) {
  const float* cam = c.f32("f_cam", 10);
  F.fx = cam[0]; F.fy = cam[1]; F.cx = cam[2]; F.cy = cam[3]; F.mbf = cam[4];
  F.mnMinX = cam[5]; F.mnMaxX = cam[6]; F.mnMinY = cam[7]; F.mnMaxY = cam[8]; F.mb = cam[9];
  F.mRcw = matOf(c.f32("f_R", 9), 3, 3);
  F.mtcw = matOf(c.f32("f_t", 3), 3, 1);
  F.mOw = matOf(c.f32("f_Ow", 3), 3, 1);
  cams.push_back(new Pinhole(std::vector<float>{F.fx, F.fy, F.cx, F.cy}));
  F.mpCamera = cams.back();
  F.Nleft = -1;
  if (!c.has("f_sf")) return;
  const size_t nl = c.len("f_sf");
  F.mnScaleLevels = (int)nl;
  F.mvScaleFactors.assign(c.f32("f_sf", nl), c.f32("f_sf", nl) + nl);
  F.mvLevelSigma2.assign(c.f32("f_sigma2", nl), c.f32("f_sigma2", nl) + nl);
  F.mvInvLevelSigma2.assign(c.f32("f_inv_sigma2", nl), c.f32("f_inv_sigma2", nl) + nl);
  F.mfLogScaleFactor = c.f32("f_logsf", 1)[0];
  const size_t n = c.len("f_x");
  F.N = (int)n;
  const float *x = c.f32("f_x", n), *y = c.f32("f_y", n), *angle = c.f32("f_angle", n), *ur = c.f32("f_uright", n);
  const int32_t* octave = c.i32("f_octave", n);
  F.mvKeysUn.resize(n);
  for (size_t i = 0; i < n; ++i) {
    cv::KeyPoint& kp = F.mvKeysUn[i];
    kp.pt.x = x[i]; kp.pt.y = y[i]; kp.octave = octave[i]; kp.angle = angle[i]; kp.size = 31.f;
  }
  F.mvKeys = F.mvKeysUn;
  F.mDescriptors.create((int)n, 32, CV_8U);
  if (n) std::memcpy(F.mDescriptors.data, c.u8("f_desc", n * 32), n * 32);
  F.mvuRight.assign(ur, ur + n);
  F.mvpMapPoints.assign(n, nullptr);
  F.mvbOutlier.assign(n, false);
  F.AssignFeaturesToGrid();
}

void frustumPoints(const Case& c, const double* params, Bag& out) {
  const size_t nq = c.len("mp_pos"), ncur = c.len("f_x");
  const unsigned char* occ = c.u8("f_occ", ncur);
  size_t nocc = 0;
  for (size_t i = 0; i < ncur; ++i) nocc += occ[i] != 0;
  std::vector<MapPoint> mps(nq + nocc);                                  // one array: pointer order is index order
  std::vector<GeometricCamera*> cams;
  Frame F;
  fillFrame(c, F, cams);
  const float *pos = c.f32("mp_pos", nq * 3), *normal = c.f32("mp_normal", nq * 3), *mn = c.f32("mp_min_dist", nq), *mx = c.f32("mp_max_dist", nq);
  const float* track = c.f32("mp_track", nq * 8);
  const unsigned char *desc = c.u8("mp_desc", nq * 32), *bad = c.u8("mp_bad", nq), *seen = c.u8("mp_seen", nq);
  for (size_t i = 0; i < mps.size(); ++i) mps[i].index = (int)i;
  std::vector<MapPoint*> list(nq);
  for (size_t i = 0; i < nq; ++i) {
    MapPoint& P = mps[i];
    P.mWorldPos = matOf(pos + 3 * i, 3, 1);
    P.mNormalVector = matOf(normal + 3 * i, 3, 1);
    P.mDescriptor.create(1, 32, CV_8U);
    std::memcpy(P.mDescriptor.data, desc + 32 * i, 32);
    P.mbBad = bad[i] != 0;
    P.mfMinDistance = mn[i]; P.mfMaxDistance = mx[i];
    P.mbSeenInFrame = seen[i] != 0;
    P.nObs = 1;
    const float* t = track + 8 * i;
    P.mbTrackInView = t[0] != 0.f; P.mTrackProjX = t[1]; P.mTrackProjY = t[2]; P.mTrackProjXR = t[3]; P.mTrackDepth = t[4];
    P.mnTrackScaleLevel = (int)t[5]; P.mTrackViewCos = t[6];
    list[i] = &P;
  }
  size_t at = nq;
  for (size_t i = 0; i < ncur; ++i)
    if (occ[i]) { mps[at].nObs = occ[i] == 1 ? 3 : 0; F.mvpMapPoints[i] = &mps[at++]; }

  int nToMatch = 0;                                                      // Tracking.cc:3806-3827
  for (std::vector<MapPoint*>::iterator vit = list.begin(), vend = list.end(); vit != vend; vit++) {
    MapPoint* pMP = *vit;
    if (pMP->mbSeenInFrame) continue;                                   // mnLastFrameSeen == mCurrentFrame.mnId
    if (pMP->isBad()) continue;
    if (F.isInFrustum(pMP, 0.5)) nToMatch++;
  }
  std::vector<float> after(nq * 8, 0.f);
  for (size_t i = 0; i < nq; ++i) {
    const MapPoint& P = mps[i];
    const float v[8] = {P.mbTrackInView ? 1.f : 0.f, P.mTrackProjX, P.mTrackProjY, P.mTrackProjXR, P.mTrackDepth, (float)P.mnTrackScaleLevel,
                        P.mTrackViewCos, 0.f};
    std::memcpy(&after[8 * i], v, sizeof v);
  }
  int ret = 0;
  if (nToMatch > 0) {                                                    // :3829-3855 (th is the case's)
    ORBmatcher matcher((float)params[0]);
    ret = matcher.SearchByProjection(F, list, (float)params[1], params[2] != 0.0, (float)params[3]);
  }
  std::vector<int32_t> rows(ncur);
  for (size_t i = 0; i < ncur; ++i) rows[i] = F.mvpMapPoints[i] ? F.mvpMapPoints[i]->index : -1;
  out["track"] = floats(after, {(int64_t)nq, 8});
  out["n_to_match"] = ints({nToMatch});
  out["frame_mp"] = ints(rows);
  out["ret"] = ints({ret});
  for (GeometricCamera* g : cams) delete g;
}

void frustumLines(const Case& c, Bag& out) {
  const size_t nl = c.len("ml_sp");
  std::vector<MapLine> mls(nl);
  std::vector<GeometricCamera*> cams;
  Frame F;
  fillFrame(c, F, cams);
  const float *sp = c.f32("ml_sp", nl * 3), *ep = c.f32("ml_ep", nl * 3);
  const unsigned char *bad = c.u8("ml_bad", nl), *seen = c.u8("ml_seen", nl);
  std::vector<MapLine*> lines(nl);
  for (size_t i = 0; i < nl; ++i) {
    MapLine& L = mls[i];
    L.index = (int)i;
    for (int k = 0; k < 3; ++k) { L.mWorldPos[k] = (double)sp[3 * i + k]; L.mWorldPos[3 + k] = (double)ep[3 * i + k]; }
    L.mbBad = bad[i] != 0;
    L.mbSeenInFrame = seen[i] != 0;
    lines[i] = &L;
  }
  int nToMatch = 0;                                                      // Tracking.cc:3858-3877
  std::vector<MapLine*> inFrustum;
  inFrustum.reserve(lines.size());
  for (std::vector<MapLine*>::iterator vit = lines.begin(), vend = lines.end(); vit != vend; vit++) {
    MapLine* pML = *vit;
    if (pML->mbSeenInFrame) continue;
    if (pML->isBad()) continue;
    pML->mTrackProjeX = 0.f; pML->mTrackProjeY = 0.f;
    if (F.isInFrustum_l(pML, 0.5)) { nToMatch++; inFrustum.push_back(pML); }
  }
  std::vector<int32_t> inView(nl), lst;
  std::vector<float> proj(nl * 2);
  for (size_t i = 0; i < nl; ++i) { inView[i] = mls[i].mbTrackInView; proj[2 * i] = mls[i].mTrackProjsX; proj[2 * i + 1] = mls[i].mTrackProjsY; }
  for (MapLine* p : inFrustum) lst.push_back(p->index);
  out["in_view"] = ints(inView);
  out["proj_s"] = floats(proj, {(int64_t)nl, 2});
  out["list"] = ints(lst);
  out["n_to_match"] = ints({nToMatch});
  for (GeometricCamera* g : cams) delete g;
}

template <class Feature> void distinctive(const Case& c, bool lines, Bag& out) {
  const Arr& kd = c.arr("kf_desc", 0);
  if (kd.shape.size() != 3 || kd.shape[2] != 32) die("distinctive: kf_desc must be [nkf,rows,32]");
  const size_t nkf = (size_t)kd.shape[0], rows = (size_t)kd.shape[1], nf = c.len("ft_bad"), nobs = c.len("obs");
  const unsigned char *kfBad = c.u8("kf_bad", nkf), *ftBad = c.u8("ft_bad", nf);
  const int32_t* obs = c.i32("obs", nobs * 3);
  std::vector<KeyFrame> kfs(nkf);
  std::vector<Feature> fts(nf);
  for (size_t k = 0; k < nkf; ++k) {
    kfs[k].index = (int)k;
    kfs[k].mbBad = kfBad[k] != 0;
    cv::Mat& D = lines ? kfs[k].mDescriptors_l : kfs[k].mDescriptors;
    D.create((int)rows, 32, CV_8U);
    if (rows) std::memcpy(D.data, kd.data.data() + k * rows * 32, rows * 32);
  }
  for (size_t i = 0; i < nf; ++i) { fts[i].index = (int)i; fts[i].mbBad = ftBad[i] != 0; fts[i].mDescriptor = cv::Mat(); }
  for (size_t o = 0; o < nobs; ++o) {
    const int32_t f = obs[3 * o], k = obs[3 * o + 1], r = obs[3 * o + 2];
    if (f < 0 || (size_t)f >= nf || k < 0 || (size_t)k >= nkf || r < 0 || (size_t)r >= rows) die("distinctive: observation out of range");
    fts[(size_t)f].mObservations[&kfs[(size_t)k]] = (size_t)r;
  }
  std::vector<unsigned char> written(nf, 0), desc(nf * 32, 0);
  std::vector<int32_t> row(nf, -1);
  for (size_t i = 0; i < nf; ++i) {
    fts[i].ComputeDistinctiveDescriptors();
    const cv::Mat& d = fts[i].mDescriptor;
    if (d.empty()) continue;
    if (d.rows != 1 || d.cols != 32 || d.type() != CV_8U) die("distinctive: mDescriptor is not a 1 x 32 CV_8U row");
    written[i] = 1;
    std::memcpy(&desc[32 * i], d.data, 32);
    int pos = 0;
    for (const auto& kv : fts[i].mObservations) {
      if (kv.first->mbBad) continue;
      const cv::Mat& D = lines ? kv.first->mDescriptors_l : kv.first->mDescriptors;
      if (std::memcmp(D.ptr<unsigned char>((int)kv.second), d.data, 32) == 0) { row[i] = pos; break; }
      ++pos;
    }
  }
  out["written"] = bytes(written);
  out["desc"] = bytes(desc, {(int64_t)nf, 32});
  out["row"] = ints(row);
}

// ---- new_map_points: a current keyframe (k0_*) and its neighbours (k1_*, ...), all KeyFrames from one array (the current one first,
// so that it has the lowest address), the map points the tables hold at entry from another
struct MapWorld {
  std::vector<KeyFrame> kfs;
  std::vector<MapPoint> held;
  std::vector<GeometricCamera*> cams;
  Atlas atlas;
  Tracking tracker;
  LocalMapping mapper;
  ~MapWorld() {
    for (MapPoint* p : atlas.added) delete p;
    for (GeometricCamera* g : cams) delete g;
  }
};

void buildMapWorld(const Case& c, const double* params, MapWorld& W, size_t nkf, size_t limit) {
  const float* cam = c.f32("cam", 6);                                     // fx fy cx cy bf mb
  const size_t nl = c.len("sf");
  W.kfs = std::vector<KeyFrame>(1 + nkf);
  size_t nheld = 0;
  for (size_t k = 0; k <= nkf; ++k) {
    const std::string pre = "k" + std::to_string(k) + "_";
    const unsigned char* has = c.u8(pre + "has_mp", c.len(pre + "x"));
    for (size_t i = 0; i < c.len(pre + "x"); ++i) nheld += has[i] != 0;
  }
  W.held = std::vector<MapPoint>(nheld);
  size_t at = 0;
  for (size_t k = 0; k <= nkf; ++k) {
    const std::string pre = "k" + std::to_string(k) + "_";
    KeyFrame& K = W.kfs[k];
    const size_t n = c.len(pre + "x");
    K.index = (int)k;
    K.N = (int)n;
    const bool twoCameras = c.has("kb1");                                  // both cameras KannalaBrandt8, NLeft rows of mvKeys, then mvKeysRight
    const float *x = c.f32(pre + "x", n), *y = c.f32(pre + "y", n), *angle = c.f32(pre + "angle", n);
    const float* key = twoCameras ? nullptr : c.f32(pre + "key", n * 2);
    const int32_t *octave = c.i32(pre + "octave", n), *node = c.i32(pre + "node", n);
    const unsigned char* has = c.u8(pre + "has_mp", n);
    K.mvKeysUn.resize(n);
    for (size_t i = 0; i < n; ++i) {
      cv::KeyPoint& kp = K.mvKeysUn[i];
      kp.pt.x = x[i]; kp.pt.y = y[i]; kp.octave = octave[i]; kp.angle = angle[i]; kp.size = 31.f;
    }
    K.mvKeys = K.mvKeysUn;
    if (key)
      for (size_t i = 0; i < n; ++i) { K.mvKeys[i].pt.x = key[2 * i]; K.mvKeys[i].pt.y = key[2 * i + 1]; }
    K.mDescriptors.create((int)n, 32, CV_8U);
    if (n) std::memcpy(K.mDescriptors.data, c.u8(pre + "desc", n * 32), n * 32);
    for (size_t i = 0; i < n; ++i)
      if (node[i] >= 0) K.mFeatVec.addFeature((DBoW2::NodeId)node[i], (unsigned int)i);
    K.mvpMapPoints.assign(n, nullptr);
    for (size_t i = 0; i < n; ++i)
      if (has[i]) { W.held[at].index = (int)at; K.mvpMapPoints[i] = &W.held[at++]; }
    if (twoCameras) {
      // Frame.cc:1589 gives such a keyframe NLeft entries of mvuRight, and :449 / :458 read mvuRight[idx] for the rows of either camera
      // (bStereo is false whatever they hold, :450): N entries here, so that the read the reference leaves undefined stays inside
      K.mvuRight.assign(n, -1.f);
      K.mvDepth.assign(n, -1.f);
    } else {
      K.mvuRight.assign(c.f32(pre + "uright", n), c.f32(pre + "uright", n) + n);
      K.mvDepth.assign(c.f32(pre + "depth", n), c.f32(pre + "depth", n) + n);
    }
    K.mvbOutlier.assign(n, false);
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4]; K.mb = cam[5];
    if (c.has(pre + "bf")) K.mbf = c.f32(pre + "bf", 1)[0];                 // a keyframe with an mbf of its own
    K.invfx = 1.0f / K.fx; K.invfy = 1.0f / K.fy;                           // Frame.cc:194-195
    K.mnMinX = 0; K.mnMaxX = 752; K.mnMinY = 0; K.mnMaxY = 480;
    K.mnScaleLevels = (int)nl;
    K.mvScaleFactors.assign(c.f32("sf", nl), c.f32("sf", nl) + nl);
    K.mvLevelSigma2.assign(c.f32("sigma2", nl), c.f32("sigma2", nl) + nl);
    K.mvInvLevelSigma2.resize(nl);
    for (size_t l = 0; l < nl; ++l) K.mvInvLevelSigma2[l] = 1.0f / K.mvLevelSigma2[l];
    K.mfScaleFactor = c.f32("scale", 1)[0];
    K.mfLogScaleFactor = std::log(K.mfScaleFactor);
    const float* pose = c.f32(pre + "pose", 15);
    K.mRcw = matOf(pose, 3, 3);
    K.mtcw = matOf(pose + 9, 3, 1);
    K.mOw = matOf(pose + 12, 3, 1);
    K.mTcw = cv::Mat::eye(4, 4, CV_32F);
    K.mRcw.copyTo(K.mTcw.rowRange(0, 3).colRange(0, 3));
    K.mtcw.copyTo(K.mTcw.rowRange(0, 3).col(3));
    K.Twc = cv::Mat::eye(4, 4, CV_32F);                                   // KeyFrame.cc:159-164: Rcw.t() and the stored Ow
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) K.Twc.at<float>(i, j) = pose[3 * j + i];
      K.Twc.at<float>(i, 3) = pose[12 + i];
    }
    K.mpMap = &W.atlas.map;
    K.mSceneMedianDepth = 2.0f;                                           // (monocular: the baseline test passes)
    if (twoCameras) {
      const int nleft = c.i32(pre + "nleft", 1)[0];
      if (nleft < 0 || nleft > (int)n) die("bad nleft");
      K.NLeft = nleft;
      K.mvKeysRight.assign(K.mvKeys.begin() + nleft, K.mvKeys.end());
      K.mvKeys.resize((size_t)nleft);
      const float *k1 = c.f32("kb1", 8), *k2 = c.f32("kb2", 8);
      W.cams.push_back(new KannalaBrandt8(std::vector<float>(k1, k1 + 8)));
      K.mpCamera = W.cams.back();
      W.cams.push_back(new KannalaBrandt8(std::vector<float>(k2, k2 + 8)));
      K.mpCamera2 = W.cams.back();
      K.mTlr = matOf(c.f32("Tlr", 12), 3, 4);                             // the right-pose getters are the matcher stand-in's
    } else {
      W.cams.push_back(new Pinhole(std::vector<float>{K.fx, K.fy, K.cx, K.cy}));
      K.mpCamera = W.cams.back();
      K.AssignFeaturesToGrid();
    }
  }
  for (size_t k = 1; k <= limit; ++k) W.kfs[0].mvpNeighbours.push_back(&W.kfs[k]);
  W.mapper.mbMonocular = params[0] != 0.0;
  W.mapper.mbInertial = params[1] != 0.0;                                 // with BA1 and not BA2: bCoarse (:420-422)
  W.atlas.map.mbIMU_BA1 = true;
  W.mapper.mbFarPoints = params[2] != 0.0;
  W.mapper.mThFarPoints = (float)params[3];
  W.mapper.mpCurrentKeyFrame = &W.kfs[0];
  W.mapper.mpTracker = &W.tracker;
  W.mapper.mpAtlas = &W.atlas;
}

void newMapPoints(const Case& c, const double* params, Bag& out) {
  cv::shim_detail::divisionFactorInFloat() = true;                        // x3D.rowRange(0, 3) / x3D.at<float>(3), :569
  size_t nkf = 0;
  while (c.has("k" + std::to_string(nkf + 1) + "_x")) ++nkf;
  // what the loop sees at neighbour k: the whole function on the neighbours before it, then the search it would make
  std::vector<int32_t> pairs;
  for (size_t k = 1; k <= nkf; ++k) {
    MapWorld W;
    buildMapWorld(c, params, W, nkf, k - 1);
    W.mapper.CreateNewMapPoints();
    KeyFrame *p1 = &W.kfs[0], *p2 = &W.kfs[k];
    std::vector<std::pair<size_t, size_t>> v;
    ORBmatcher matcher(0.6f, false);
    matcher.SearchForTriangulation(p1, p2, W.mapper.ComputeF12(p1, p2), v, false, params[1] != 0.0);
    for (const auto& p : v) { pairs.push_back((int32_t)(k - 1)); pairs.push_back((int32_t)p.first); pairs.push_back((int32_t)p.second); }
  }
  MapWorld W;
  buildMapWorld(c, params, W, nkf, nkf);
  W.mapper.CreateNewMapPoints();
  std::vector<int32_t> created, descRow;
  std::vector<float> x3d;
  std::vector<unsigned char> desc;
  for (MapPoint* p : W.mapper.mlpRecentAddedMapPoints) {
    if (p->mObservations.size() != 2 || p->mObservations.begin()->first != &W.kfs[0]) die("new_map_points: a new point without its two observations");
    auto second = p->mObservations.begin();
    ++second;
    created.push_back(second->first->index - 1);
    created.push_back((int32_t)p->mObservations.begin()->second);
    created.push_back((int32_t)second->second);
    for (int i = 0; i < 3; ++i) x3d.push_back(p->mWorldPos.at<float>(i));
    if (p->mDescriptor.empty() || p->mDescriptor.cols != 32) die("new_map_points: a new point without a descriptor");
    desc.insert(desc.end(), p->mDescriptor.data, p->mDescriptor.data + 32);
    int row = -1, pos = 0;
    for (const auto& kv : p->mObservations) {
      if (row < 0 && std::memcmp(kv.first->mDescriptors.ptr<unsigned char>((int)kv.second), p->mDescriptor.data, 32) == 0) row = pos;
      ++pos;
    }
    descRow.push_back(row);
  }
  if (W.atlas.added.size() != W.mapper.mlpRecentAddedMapPoints.size()) die("new_map_points: AddMapPoint and the recent list disagree");
  const int64_t m = (int64_t)descRow.size();
  out["pairs"] = ints(pairs, {(int64_t)pairs.size() / 3, 3});
  out["created"] = ints(created, {m, 3});
  out["x3d"] = floats(x3d, {m, 3});
  out["desc"] = bytes(desc, {m, 32});
  out["desc_row"] = ints(descRow);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--functions") {
    for (const char* f : {"frustum_points", "frustum_lines", "distinctive", "new_map_points"}) std::printf("%s\n", f);
    return 0;
  }
  if (argc != 3) { std::fprintf(stderr, "usage: %s CASE RESULT\n", argv[0]); return 2; }
  Case c;
  c.bag = readBag(argv[1]);
  const Arr& fnArr = c.arr("fn", 0);
  const std::string fn(fnArr.data.begin(), fnArr.data.end());
  const Arr& pa = c.arr("params", 3);
  const double* params = reinterpret_cast<const double*>(pa.data.data());
  Bag out;
  if (fn == "frustum_points") {
    if (pa.count() != 4) die("frustum_points takes four parameters");
    frustumPoints(c, params, out);
  } else if (fn == "frustum_lines") {
    frustumLines(c, out);
  } else if (fn == "distinctive") {
    if (pa.count() != 1) die("distinctive takes one parameter");
    if (params[0] != 0.0) distinctive<MapLine>(c, true, out);
    else distinctive<MapPoint>(c, false, out);
  } else if (fn == "new_map_points") {
    if (pa.count() != 4) die("new_map_points takes four parameters");
    newMapPoints(c, params, out);
  } else {
    die("unknown function " + fn);
  }
  writeBag(argv[2], out);
  return 0;
}
