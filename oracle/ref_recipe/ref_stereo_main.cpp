// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over the reference's own src/LineMatcher.cpp, src/gridStructure.cpp, src/LineIterator.cpp, src/Config.cpp and
// the stereo functions of src/Frame.cc (cut out at build time, see stereo_shim/pli_stereo_shim.hpp), which oracle/Makefile compiles
// from the reference tree (never copied) against stereo_shim/.
//
//   pli_ref_stereo CASE RESULT
//   pli_ref_stereo --functions       prints the names "fn" may take, one per line
//
// CASE and RESULT are files of named arrays in the format of pli_ref_match (tests/helpers_match_ref.py: write_bag / read_bag).
// A case holds ONE call of the function "fn" names (bytes):
//   points   kpL / kpR [n,3] float32 (x, y, octave), descL / descR [n,32], sf / inv_sf [levels], rig [2] (mb, mbf),
//            pyrL<l> / pyrR<l> [h,w] uint8 per level            -> uright [n], depth [n]
//   lines    klL / klR [n,4] float32 (start x, y, end x, y), ldL / ldR [n,32], inv [2] float64 (inv_width, inv_height),
//            cfg [8] float64 (matchingSWs, bestLRMatches, lineSimTh, minRatio12L, minDisp, lineHorizTh, stereoOverlapTh,
//            lsMinDispRatio)                                       -> disp [n,2], le [n,3] float64, m12 [n] (a separate matchGrid call)
//   overlap  table [n,4] float64, cfg as above                     -> out [n] float64
//   filter   table [n,8] float64 (spl, epl, spr, epr), cfg         -> out [n,2] float64
//   nnr      d1, d2 [n,32], params [1] float64 (nnr)               -> ret [1], m12 [n]
//   match    d1, d2, params [2] float64 (nnr, bestLRMatches)       -> ret [1], m12 [n]
//   dist     a, b [n,32]                                           -> out [n]
//   area     kp [n,3] (one camera: the undistorted keypoints; two cameras: rows [0, nleft) left, the rest right), nleft [1],
//            bounds [4] float32 (minX, maxX, minY, maxY), q [m,6] float32 (x, y, r, minLevel, maxLevel, bRight)
//                                                                  -> idx (all lists, one after the other), start [m+1]
//   rgbd     kp [n,3], kpun [n,3], depth_image [h,w] float32, rig  -> uright [n], depth [n]
// A reference call that throws ends the program with status 3: a failed generation, never a result.
#include <cstdio>
#include <cstdlib>
#include <map>
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

void die(const std::string& what) { std::fprintf(stderr, "pli_ref_stereo: %s\n", what.c_str()); std::exit(2); }

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

template <class T> Arr arrayOf(int type, const std::vector<T>& v, std::vector<int64_t> shape = {}) {
  Arr a;
  a.type = type;
  a.shape = shape.empty() ? std::vector<int64_t>{(int64_t)v.size()} : shape;
  a.data.resize(v.size() * sizeof(T));
  if (!v.empty()) std::memcpy(a.data.data(), v.data(), a.data.size());
  return a;
}
Arr ints(const std::vector<int32_t>& v, std::vector<int64_t> s = {}) { return arrayOf(1, v, s); }
Arr floats(const std::vector<float>& v, std::vector<int64_t> s = {}) { return arrayOf(2, v, s); }
Arr doubles(const std::vector<double>& v, std::vector<int64_t> s = {}) { return arrayOf(3, v, s); }

struct Case {
  Bag bag;
  const Arr& arr(const std::string& n, int type) const {
    auto it = bag.find(n);
    if (it == bag.end()) die("missing array " + n);
    if (it->second.type != type) die("wrong type: " + n);
    return it->second;
  }
  const Arr& arr(const std::string& n, int type, size_t count) const {
    const Arr& a = arr(n, type);
    if (a.count() != count) die("wrong size: " + n);
    return a;
  }
  // the rows of a 2-D array with `cols` columns
  size_t rows(const std::string& n, int type, size_t cols) const {
    const Arr& a = arr(n, type);
    if (a.shape.size() != 2 || (size_t)a.shape[1] != cols) die("wrong shape: " + n);
    return (size_t)a.shape[0];
  }
  const float* f32(const std::string& n) const { return reinterpret_cast<const float*>(arr(n, 2).data.data()); }
  const double* f64(const std::string& n) const { return reinterpret_cast<const double*>(arr(n, 3).data.data()); }
  const unsigned char* u8(const std::string& n) const { return arr(n, 0).data.data(); }
};

std::vector<cv::KeyPoint> keypointsOf(const Case& c, const std::string& n) {
  const size_t rows = c.rows(n, 2, 3);
  const float* p = c.f32(n);
  std::vector<cv::KeyPoint> v(rows);
  for (size_t i = 0; i < rows; ++i) { v[i].pt.x = p[3 * i]; v[i].pt.y = p[3 * i + 1]; v[i].octave = (int)p[3 * i + 2]; }
  return v;
}
std::vector<cv::line_descriptor::KeyLine> keylinesOf(const Case& c, const std::string& n) {
  const size_t rows = c.rows(n, 2, 4);
  const float* p = c.f32(n);
  std::vector<cv::line_descriptor::KeyLine> v(rows);
  for (size_t i = 0; i < rows; ++i) {
    v[i].startPointX = p[4 * i]; v[i].startPointY = p[4 * i + 1]; v[i].endPointX = p[4 * i + 2]; v[i].endPointY = p[4 * i + 3];
  }
  return v;
}
cv::Mat bytesOf(const Case& c, const std::string& n) {
  const Arr& a = c.arr(n, 0);
  if (a.shape.size() != 2) die("wrong shape: " + n);
  cv::Mat m;
  if (a.shape[0] == 0) { m.cols = (int)a.shape[1]; return m; }      // (no rows: an empty header, as OpenCV's Mat(0, 32, CV_8U))
  m.create((int)a.shape[0], (int)a.shape[1], CV_8U);
  std::memcpy(m.data, a.data.data(), a.data.size());
  return m;
}
std::vector<float> floatsOf(const Case& c, const std::string& n) {
  const Arr& a = c.arr(n, 2);
  const float* p = c.f32(n);
  return std::vector<float>(p, p + a.count());
}
void configOf(const Case& c) {
  const double* p = reinterpret_cast<const double*>(c.arr("cfg", 3, 8).data.data());
  Config::matchingSWs() = (int)p[0];
  Config::bestLRMatches() = p[1] != 0.0;
  Config::lrInParallel() = false;
  Config::lineSimTh() = p[2];
  Config::minRatio12L() = p[3];
  Config::minDisp() = p[4];
  Config::lineHorizTh() = p[5];
  Config::stereoOverlapTh() = p[6];
  Config::lsMinDispRatio() = p[7];
}

void fnPoints(const Case& c, Bag& out) {
  Frame F;
  ORBextractor eL, eR;
  F.mvKeys = keypointsOf(c, "kpL"); F.mvKeysRight = keypointsOf(c, "kpR");
  F.N = (int)F.mvKeys.size();
  F.mDescriptors = bytesOf(c, "descL"); F.mDescriptorsRight = bytesOf(c, "descR");
  F.mvScaleFactors = floatsOf(c, "sf"); F.mvInvScaleFactors = floatsOf(c, "inv_sf");
  const float* rig = reinterpret_cast<const float*>(c.arr("rig", 2, 2).data.data());
  F.mb = rig[0]; F.mbf = rig[1];
  for (size_t l = 0; l < F.mvScaleFactors.size(); ++l) {
    eL.mvImagePyramid.push_back(bytesOf(c, "pyrL" + std::to_string(l)));
    eR.mvImagePyramid.push_back(bytesOf(c, "pyrR" + std::to_string(l)));
  }
  F.mpORBextractorLeft = &eL; F.mpORBextractorRight = &eR;
  F.ComputeStereoMatches();
  out["uright"] = floats(F.mvuRight); out["depth"] = floats(F.mvDepth);
}

void fnLines(const Case& c, Bag& out) {
  configOf(c);
  Frame F;
  F.mvKeys_Line = keylinesOf(c, "klL"); F.mvKeysRight_Line = keylinesOf(c, "klR");
  F.N_l = (int)F.mvKeys_Line.size();
  F.mDescriptors_Line = bytesOf(c, "ldL"); F.mDescriptorsRight_Line = bytesOf(c, "ldR");
  const double* inv = reinterpret_cast<const double*>(c.arr("inv", 3, 2).data.data());
  F.inv_width = inv[0]; F.inv_height = inv[1];
  F.ComputeStereoMatches_Lines();
  const size_t n = F.mvKeys_Line.size();
  if (F.mvDisparity_l.size() != n || F.mvle_l.size() != n) die("lines: the result vectors changed their size");
  std::vector<float> disp(2 * n);
  std::vector<double> le(3 * n);
  for (size_t i = 0; i < n; ++i) {
    disp[2 * i] = F.mvDisparity_l[i].first; disp[2 * i + 1] = F.mvDisparity_l[i].second;
    for (int k = 0; k < 3; ++k) le[3 * i + (size_t)k] = F.mvle_l[i](k);
  }
  out["disp"] = floats(disp, {(int64_t)n, 2}); out["le"] = doubles(le, {(int64_t)n, 3});
  // a matchGrid call of its own on the same inputs: the arguments as ComputeStereoMatches_Lines states them, the grid filled
  // through the reference's own getLineCoords and GridStructure
  std::vector<int32_t> m12(n, -1);
  if (n && !F.mvKeysRight_Line.empty()) {
    std::vector<line_2d> coords;
    for (const cv::line_descriptor::KeyLine& kl : F.mvKeys_Line)
      coords.push_back(std::make_pair(std::make_pair(kl.startPointX * F.inv_width, kl.startPointY * F.inv_height),
                                      std::make_pair(kl.endPointX * F.inv_width, kl.endPointY * F.inv_height)));
    std::list<std::pair<int, int>> cells;
    GridStructure grid(FRAME_GRID_ROWS, FRAME_GRID_COLS);
    std::vector<std::pair<double, double>> directions(F.mvKeysRight_Line.size());
    for (unsigned int idx = 0; idx < F.mvKeysRight_Line.size(); ++idx) {
      const cv::line_descriptor::KeyLine& kl = F.mvKeysRight_Line[idx];
      directions[idx] = std::make_pair((kl.endPointX - kl.startPointX) * F.inv_width, (kl.endPointY - kl.startPointY) * F.inv_height);
      normalize(directions[idx]);
      getLineCoords(kl.startPointX * F.inv_width, kl.startPointY * F.inv_height, kl.endPointX * F.inv_width, kl.endPointY * F.inv_height, cells);
      for (const std::pair<int, int>& p : cells) grid.at(p.first, p.second).push_back((int)idx);
    }
    GridWindow w;
    w.width = std::make_pair(Config::matchingSWs(), 0);
    w.height = std::make_pair(0, 0);
    std::vector<int> m;
    matchGrid(coords, F.mDescriptors_Line, grid, F.mDescriptorsRight_Line, directions, w, m);
    if (m.size() != n) die("lines: matchGrid changed the size of matches_12");
    for (size_t i = 0; i < n; ++i) m12[i] = m[i];
  }
  out["m12"] = ints(m12);
}

void fnOverlap(const Case& c, Bag& out) {
  configOf(c);
  const size_t n = c.rows("table", 3, 4);
  const double* t = c.f64("table");
  Frame F;
  std::vector<double> o(n);
  for (size_t i = 0; i < n; ++i) o[i] = F.lineSegmentOverlapStereo(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
  out["out"] = doubles(o);
}

void fnFilter(const Case& c, Bag& out) {
  configOf(c);
  const size_t n = c.rows("table", 3, 8);
  const double* t = c.f64("table");
  Frame F;
  std::vector<double> o(2 * n);
  for (size_t i = 0; i < n; ++i) {
    const double* r = t + 8 * i;
    F.filterLineSegmentDisparity(Vector2d(r[0], r[1]), Vector2d(r[2], r[3]), Vector2d(r[4], r[5]), Vector2d(r[6], r[7]), o[2 * i], o[2 * i + 1]);
  }
  out["out"] = doubles(o, {(int64_t)n, 2});
}

void fnMatch(const Case& c, Bag& out, bool nnrOnly) {
  const cv::Mat d1 = bytesOf(c, "d1"), d2 = bytesOf(c, "d2");
  const double* p = c.f64("params");
  if (!nnrOnly) { Config::bestLRMatches() = p[1] != 0.0; Config::lrInParallel() = false; }
  std::vector<int> m;
  const int ret = nnrOnly ? matchNNR(d1, d2, (float)p[0], m) : match(d1, d2, (float)p[0], m);
  out["ret"] = ints({ret});
  out["m12"] = ints(std::vector<int32_t>(m.begin(), m.end()));
}

void fnDist(const Case& c, Bag& out) {
  const cv::Mat a = bytesOf(c, "a"), b = bytesOf(c, "b");
  if (a.rows != b.rows || (a.rows && (a.cols != 32 || b.cols != 32))) die("dist: two tables of equal length with 32 columns");
  std::vector<int32_t> o((size_t)a.rows);
  for (int i = 0; i < a.rows; ++i) o[(size_t)i] = ORB_SLAM3::distance(a.row(i), b.row(i));
  out["out"] = ints(o);
}

void fnArea(const Case& c, Bag& out) {
  Frame F;
  const std::vector<cv::KeyPoint> kp = keypointsOf(c, "kp");
  const int nleft = reinterpret_cast<const int32_t*>(c.arr("nleft", 1, 1).data.data())[0];
  const float* b = reinterpret_cast<const float*>(c.arr("bounds", 2, 4).data.data());
  F.N = (int)kp.size();
  F.Nleft = nleft;
  if (nleft == -1) {
    F.mvKeysUn = kp; F.mvKeys = kp;
  } else {
    if (nleft < 0 || nleft > F.N) die("area: nleft outside the table");
    F.mvKeys.assign(kp.begin(), kp.begin() + nleft);
    F.mvKeysRight.assign(kp.begin() + nleft, kp.end());
    F.Nright = F.N - nleft;
  }
  F.mnMinX = b[0]; F.mnMaxX = b[1]; F.mnMinY = b[2]; F.mnMaxY = b[3];
  F.mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(F.mnMaxX - F.mnMinX);      // Frame.cc:180-181
  F.mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(F.mnMaxY - F.mnMinY);
  F.AssignFeaturesToGrid();
  const size_t m = c.rows("q", 2, 6);
  const float* q = c.f32("q");
  std::vector<int32_t> idx, start(1, 0);
  for (size_t i = 0; i < m; ++i) {
    const float* r = q + 6 * i;
    const bool bRight = r[5] != 0.f;
    if (bRight && nleft == -1) die("area: bRight on a one-camera frame");
    const std::vector<size_t> v = F.GetFeaturesInArea(r[0], r[1], r[2], (int)r[3], (int)r[4], bRight);
    for (size_t j : v) idx.push_back((int32_t)j);
    start.push_back((int32_t)idx.size());
  }
  out["idx"] = ints(idx); out["start"] = ints(start);
}

void fnRgbd(const Case& c, Bag& out) {
  Frame F;
  F.mvKeys = keypointsOf(c, "kp"); F.mvKeysUn = keypointsOf(c, "kpun");
  F.N = (int)F.mvKeys.size();
  if (F.mvKeysUn.size() != F.mvKeys.size()) die("rgbd: kp and kpun differ in length");
  const float* rig = reinterpret_cast<const float*>(c.arr("rig", 2, 2).data.data());
  F.mb = rig[0]; F.mbf = rig[1];
  const Arr& a = c.arr("depth_image", 2);
  if (a.shape.size() != 2) die("wrong shape: depth_image");
  cv::Mat im((int)a.shape[0], (int)a.shape[1], CV_32F);
  std::memcpy(im.data, a.data.data(), a.data.size());
  F.ComputeStereoFromRGBD(im);
  out["uright"] = floats(F.mvuRight); out["depth"] = floats(F.mvDepth);
}

const char* kFunctions[] = {"points", "lines", "overlap", "filter", "nnr", "match", "dist", "area", "rgbd"};

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--functions") {
    for (const char* f : kFunctions) std::printf("%s\n", f);
    return 0;
  }
  if (argc != 3) die("usage: pli_ref_stereo CASE RESULT | --functions");
  Case c;
  c.bag = readBag(argv[1]);
  const Arr& fa = c.arr("fn", 0);
  const std::string fn(fa.data.begin(), fa.data.end());
  Bag out;
  try {
    if (fn == "points") fnPoints(c, out);
    else if (fn == "lines") fnLines(c, out);
    else if (fn == "overlap") fnOverlap(c, out);
    else if (fn == "filter") fnFilter(c, out);
    else if (fn == "nnr") fnMatch(c, out, true);
    else if (fn == "match") fnMatch(c, out, false);
    else if (fn == "dist") fnDist(c, out);
    else if (fn == "area") fnArea(c, out);
    else if (fn == "rgbd") fnRgbd(c, out);
    else die("unknown function " + fn);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pli_ref_stereo: %s: the reference call threw: %s\n", fn.c_str(), e.what());
    return 3;
  }
  writeBag(argv[2], out);
  return 0;
}
