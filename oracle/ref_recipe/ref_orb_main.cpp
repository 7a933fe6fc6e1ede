// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over the reference's own src/ORBextractor.cc, which oracle/Makefile
// compiles from the reference tree (never copied) against cv_shim/.  The four OpenCV
// primitives that translation unit leaves undefined are defined here over
// oracle/ocv_prims.hpp; cv::FAST goes by the definition, ONE threshold per call, and is
// deliberately not the oracle's merged two-threshold fastCell.
//
//   pli_ref_orb REQUEST RESPONSE            (-DPLI_REF_BUMP: monotone operator new)
//   pli_ref_orb_sysheap REQUEST RESPONSE    (the C library's heap)
//
// REQUEST : int32 W, H, nfeatures; float32 scaleFactor; int32 nlevels, iniThFAST, minThFAST,
//           lap0, lap1; W*H image bytes.
// RESPONSE: int32 monoIndex, n; n x {float32 x, y, size, angle, response; int32 octave};
//           n x 32 descriptor bytes; int32 nlevels; per level int32 w, h and w*h bytes of
//           the mvImagePyramid[level] ROI.
//
// A program of its own because it replaces operator new: DistributeOctTree sorts
// pair<int, ExtractorNode*>, so equal node sizes are ordered by heap address, and only a
// heap that hands out growing addresses makes the run reproducible.  Never load this
// into another process.
#include "pli_cv_shim.hpp"
#include "ORBextractor.h"
#include "../ocv_prims.hpp"
#include <cstdio>
#include <cstdlib>
#include <new>

#ifdef PLI_REF_BUMP
// 16-byte aligned, never reuses, delete is a no-op
static char* g_arena = nullptr;
static size_t g_off = 0;
static const size_t kArenaBytes = (size_t)2 << 30;
void* operator new(size_t n) {
  if (!g_arena) {
    g_arena = (char*)std::malloc(kArenaBytes);
    if (!g_arena) std::abort();
  }
  n = (n + 15) & ~(size_t)15;
  if (g_off + n > kArenaBytes) std::abort();
  void* p = g_arena + g_off;
  g_off += n;
  return p;
}
void* operator new[](size_t n) { return operator new(n); }
void operator delete(void*) noexcept {}
void operator delete[](void*) noexcept {}
void operator delete(void*, size_t) noexcept {}
void operator delete[](void*, size_t) noexcept {}
#endif

namespace cv {

float fastAtan2(float y, float x) { return orc::fastAtan2(y, x); }

static orc::Img8 toImg(const Mat& m) {
  orc::Img8 o(m.cols, m.rows);
  for (int y = 0; y < m.rows; ++y) std::memcpy(o.row(y), m.ptr(y), m.cols);
  return o;
}
// keeps dst's buffer (an ROI included) when the size already matches
static void fromImg(const orc::Img8& s, Mat& d) {
  d.create(s.h, s.w, CV_8UC1);
  for (int y = 0; y < s.h; ++y) std::memcpy(d.ptr(y), s.row(y), s.w);
}

// cv::FAST(img, keys, th, true), FAST-9/16: interior 3..dim-4 of the sub-image, corner iff arc value > th, score = arc - 1,
// kept iff strictly greater than its 8 neighbours (non-corners at this threshold and pixels outside the interior count 0)
void FAST(const Mat& img, std::vector<KeyPoint>& kps, int th, bool) {
  kps.clear();
  const int w = img.cols, h = img.rows;
  if (w < 7 || h < 7) return;
  const int iw = w - 6, ih = h - 6;
  std::vector<int> sc((size_t)iw * ih);
  for (int y = 0; y < ih; ++y)
    for (int x = 0; x < iw; ++x) {
      const int arc = orc::fastArcValue(img.ptr(y + 3) + x + 3, (int)img.step);
      sc[(size_t)y * iw + x] = arc > th ? arc - 1 : 0;
    }
  auto S = [&](int y, int x) { return (x < 0 || y < 0 || x >= iw || y >= ih) ? 0 : sc[(size_t)y * iw + x]; };
  for (int y = 0; y < ih; ++y)
    for (int x = 0; x < iw; ++x) {
      const int s = S(y, x);
      if (!s) continue;
      if (s > S(y - 1, x - 1) && s > S(y - 1, x) && s > S(y - 1, x + 1) && s > S(y, x - 1) && s > S(y, x + 1) &&
          s > S(y + 1, x - 1) && s > S(y + 1, x) && s > S(y + 1, x + 1)) {
        KeyPoint k;
        k.pt = Point2f((float)(x + 3), (float)(y + 3));
        k.size = 7.f;
        k.response = (float)s;
        kps.push_back(k);
      }
    }
}

void GaussianBlur(const Mat& src, Mat& dst, Size k, double sx, double, int) {
  orc::Img8 s = toImg(src), d;
  orc::gaussianBlur8u(s, d, k.width, sx);
  fromImg(d, dst);
}

void resize(const Mat& src, Mat& dst, Size sz, double, double, int) {
  orc::Img8 s = toImg(src), d;
  orc::resizeLinear8u(s, d, sz.width, sz.height, 1.0 / ((double)sz.width / src.cols), 1.0 / ((double)sz.height / src.rows));
  fromImg(d, dst);
}

// src may be an ROI of dst: it is copied out first
void copyMakeBorder(const Mat& src, Mat& dst, int t, int b, int l, int r, int) {
  orc::Img8 s = toImg(src);
  dst.create(src.rows + t + b, src.cols + l + r, CV_8UC1);
  for (int y = 0; y < dst.rows; ++y)
    for (int x = 0; x < dst.cols; ++x)
      dst.at<uchar>(y, x) = s.at(orc::reflect101(y - t, s.h), orc::reflect101(x - l, s.w));
}

// named by the dead ComputeKeyPointsOld only
void KeyPointsFilter::retainBest(std::vector<KeyPoint>&, int) { std::abort(); }

}  // namespace cv

static bool readAll(FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }
static void put(FILE* f, const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, f) != n) { std::perror("write"); std::exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s REQUEST RESPONSE\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t W, H, nf, nlevels, iniTh, minTh, lap[2];
  float sf;
  if (!readAll(in, &W, 4) || !readAll(in, &H, 4) || !readAll(in, &nf, 4) || !readAll(in, &sf, 4) || !readAll(in, &nlevels, 4) ||
      !readAll(in, &iniTh, 4) || !readAll(in, &minTh, 4) || !readAll(in, lap, 8) || W <= 0 || H <= 0 || W > 8192 || H > 8192 ||
      nlevels <= 0 || nlevels > 64) {
    std::fprintf(stderr, "bad request header\n");
    return 2;
  }
  cv::Mat image(H, W, CV_8UC1);
  if (!readAll(in, image.data, (size_t)W * H)) { std::fprintf(stderr, "short image\n"); return 2; }
  std::fclose(in);

  ORB_SLAM3::ORBextractor ex(nf, sf, nlevels, iniTh, minTh);
  std::vector<cv::KeyPoint> kps;
  cv::Mat desc;
  std::vector<int> vLappingArea = {lap[0], lap[1]};
  const int32_t mono = ex(image, cv::Mat(), kps, desc, vLappingArea);

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const int32_t n = (int32_t)kps.size();
  put(out, &mono, 4);
  put(out, &n, 4);
  for (const cv::KeyPoint& k : kps) {
    const float f[5] = {k.pt.x, k.pt.y, k.size, k.angle, k.response};
    const int32_t o = k.octave;
    put(out, f, sizeof f);
    put(out, &o, 4);
  }
  for (int i = 0; i < n; ++i) put(out, desc.ptr(i), 32);
  put(out, &nlevels, 4);
  for (int l = 0; l < nlevels; ++l) {
    const cv::Mat& m = ex.mvImagePyramid[l];
    const int32_t wh[2] = {m.cols, m.rows};
    put(out, wh, 8);
    for (int y = 0; y < m.rows; ++y) put(out, m.ptr(y), m.cols);
  }
  std::fclose(out);
  return 0;
}
