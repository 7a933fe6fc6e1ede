// Host test of pli_slam_amd/adapters/frame_single.hpp (tests/test_cpp_single_frame.py; a stand-alone program, linked against
// tests/cpp/mock_pli_single_frame.cpp): PliSingleCameraFrame fills a stub Frame — the members of the reference's Frame that its two
// single-camera constructors write (src/Frame.cc:231-331, :334-448) — and every member is compared with what the C entry point
// returned for the same image on a second context.  Checked: every member of the list in the adapter's header; mvKeysUn[i]'s
// other fields against mvKeys[i]; mvKeysUn_Line with and without k1; the order of mGrid's cells; the image bounds on the first
// Frame only; the early return on a Frame without keypoints; the monocular lapping area; bad arguments.
// Prints one "ok <case>" line per case and returns 0, or prints what differs and returns 1.
#include <opencv2/core/core.hpp>
namespace cv { namespace line_descriptor {
struct KeyLine {      // field names as Thirdparty/line_descriptor/include/line_descriptor/descriptor_custom.hpp:105-144
  float angle; int class_id; int octave; cv::Point2f pt; float response; float size;
  float startPointX, startPointY, endPointX, endPointY, sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
  float lineLength; int numOfPixels;
};
}}
#include "pli_slam_amd/adapters/frame_single.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using cv::line_descriptor::KeyLine;

struct Frame {                         // the members the adapter writes, with the reference's names and types (include/Frame.h)
  std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  cv::Mat mDescriptors, mDescriptors_Line;
  std::vector<KeyLine> mvKeys_Line, mvKeysUn_Line;
  std::vector<float> mvuRight, mvDepth;
  int monoLeft = -1;
  float mbf = 40.f;
  std::vector<std::size_t> mGrid[64][48];
  static bool mbInitialComputations;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
};
bool Frame::mbInitialComputations = true;
float Frame::mnMinX = 0, Frame::mnMaxX = 0, Frame::mnMinY = 0, Frame::mnMaxY = 0;

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_fail; } } while (0)

static const int W = 160, H = 120;

static cv::Mat image(int seed) {
  cv::Mat m(H, W, CV_8UC1);
  for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) m.at<unsigned char>(y, x) = (unsigned char)((x * 7 + y * 13 + seed * 31 + (x * y) % 11) & 255);
  return m;
}
static cv::Mat depthImage() {          // a plane with a band of zeros and a band of negative values
  cv::Mat d(H, W, CV_32F);
  for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) d.at<float>(y, x) = y >= 30 && y < 45 ? 0.f : y >= 70 && y < 85 ? -1.5f : 1.f + 0.01f * x + 0.02f * y;
  return d;
}

struct Direct {                        // what the C entry point returns for the same input, on a context of its own
  std::vector<uint8_t> rec; std::vector<float> kpUn, klUn; std::vector<int32_t> cell; int32_t nMono = 0; int N = 0, M = 0;
};
static Direct direct(pli::Frontend& fe, const cv::Mat& img, const cv::Mat* depth, int x0, int x1) {
  const pli_table_layout& Y = fe.layout();
  Direct D;
  D.rec.resize((size_t)Y.record_bytes); D.kpUn.resize((size_t)Y.kp_cap * 2); D.klUn.resize((size_t)Y.kl_cap * 4); D.cell.resize(Y.kp_cap);
  pli::check(pli_frame_extract_single(fe.handle(), img.data, img.cols, img.rows, (int64_t)img.step, x0, x1,
                                      depth ? reinterpret_cast<const float*>(depth->data) : nullptr, depth ? (int64_t)(depth->step / 4) : 0,
                                      D.rec.data(), D.kpUn.data(), D.klUn.data(), D.cell.data(), &D.nMono));
  const int32_t* counts = reinterpret_cast<const int32_t*>(D.rec.data() + Y.off_counts);
  D.N = counts[0]; D.M = counts[2];
  return D;
}

static void checkExtractors(const char* what, const Frame& F, const Direct& D, const pli_table_layout& Y) {
  const pli_keypoint* kp = reinterpret_cast<const pli_keypoint*>(D.rec.data() + Y.off_kp[0]);
  const pli_keyline* kl = reinterpret_cast<const pli_keyline*>(D.rec.data() + Y.off_kl[0]);
  EXPECT((int)F.mvKeys.size() == D.N && (int)F.mvKeys_Line.size() == D.M, "%s: %zu keypoints, %zu key lines", what, F.mvKeys.size(), F.mvKeys_Line.size());
  EXPECT(F.monoLeft == D.nMono, "%s: monoLeft %d, the call returned %d", what, F.monoLeft, D.nMono);
  for (int i = 0; i < D.N && i < (int)F.mvKeys.size(); ++i) {
    const cv::KeyPoint& k = F.mvKeys[i];
    EXPECT(k.pt.x == kp[i].x && k.pt.y == kp[i].y && k.size == kp[i].size && k.angle == kp[i].angle && k.response == kp[i].response &&
           k.octave == kp[i].octave && k.class_id == -1, "%s: mvKeys[%d]", what, i);
  }
  if (D.N) {
    EXPECT(F.mDescriptors.rows == D.N && F.mDescriptors.cols == 32 && F.mDescriptors.type() == CV_8UC1, "%s: mDescriptors %d x %d", what, F.mDescriptors.rows, F.mDescriptors.cols);
    for (int i = 0; i < D.N && i < F.mDescriptors.rows; ++i)
      EXPECT(std::memcmp(F.mDescriptors.ptr(i), D.rec.data() + Y.off_desc[0] + (size_t)i * 32, 32) == 0, "%s: mDescriptors row %d", what, i);
  } else {
    EXPECT(F.mDescriptors.empty(), "%s: mDescriptors of a Frame without keypoints", what);
  }
  for (int i = 0; i < D.M && i < (int)F.mvKeys_Line.size(); ++i) {
    const KeyLine& k = F.mvKeys_Line[i];
    const pli_keyline& s = kl[i];
    EXPECT(k.angle == s.angle && k.class_id == s.class_id && k.octave == s.octave && k.pt.x == s.pt_x && k.pt.y == s.pt_y && k.response == s.response &&
           k.size == s.size && k.startPointX == s.startPointX && k.startPointY == s.startPointY && k.endPointX == s.endPointX && k.endPointY == s.endPointY &&
           k.sPointInOctaveX == s.sPointInOctaveX && k.sPointInOctaveY == s.sPointInOctaveY && k.ePointInOctaveX == s.ePointInOctaveX &&
           k.ePointInOctaveY == s.ePointInOctaveY && k.lineLength == s.lineLength && k.numOfPixels == s.numOfPixels, "%s: mvKeys_Line[%d]", what, i);
  }
  EXPECT(F.mDescriptors_Line.rows == D.M && F.mDescriptors_Line.cols == 32, "%s: mDescriptors_Line %d x %d", what, F.mDescriptors_Line.rows, F.mDescriptors_Line.cols);
  for (int i = 0; i < D.M && i < F.mDescriptors_Line.rows; ++i)
    EXPECT(std::memcmp(F.mDescriptors_Line.ptr(i), D.rec.data() + Y.off_ldesc[0] + (size_t)i * 32, 32) == 0, "%s: mDescriptors_Line row %d", what, i);
}

static void checkBehind(const char* what, const Frame& F, const Direct& D, const pli_table_layout& Y, bool distorted) {
  EXPECT((int)F.mvKeysUn.size() == D.N && (int)F.mvKeysUn_Line.size() == D.M, "%s: %zu / %zu undistorted", what, F.mvKeysUn.size(), F.mvKeysUn_Line.size());
  int movedPts = 0;
  for (int i = 0; i < D.N && i < (int)F.mvKeysUn.size(); ++i) {
    const cv::KeyPoint &u = F.mvKeysUn[i], &k = F.mvKeys[i];
    EXPECT(u.pt.x == D.kpUn[2 * i] && u.pt.y == D.kpUn[2 * i + 1], "%s: mvKeysUn[%d].pt", what, i);
    EXPECT(u.size == k.size && u.angle == k.angle && u.response == k.response && u.octave == k.octave && u.class_id == k.class_id,
           "%s: mvKeysUn[%d]'s other fields are mvKeys[%d]'s", what, i, i);
    movedPts += u.pt.x != k.pt.x;
  }
  EXPECT(distorted ? movedPts > 0 : movedPts == 0, "%s: %d keypoints moved", what, movedPts);
  for (int i = 0; i < D.M && i < (int)F.mvKeysUn_Line.size(); ++i) {
    const KeyLine &u = F.mvKeysUn_Line[i], &k = F.mvKeys_Line[i];
    EXPECT(u.startPointX == D.klUn[4 * i] && u.startPointY == D.klUn[4 * i + 1] && u.endPointX == D.klUn[4 * i + 2] && u.endPointY == D.klUn[4 * i + 3],
           "%s: mvKeysUn_Line[%d]", what, i);
    if (distorted)      // Frame.cc:937-944: fresh key lines, the four coordinates alone are set
      EXPECT(u.lineLength == 0.f && u.numOfPixels == 0 && u.class_id == 0 && u.response == 0.f, "%s: mvKeysUn_Line[%d] carries more than its end points", what, i);
    else                // :911: a copy
      EXPECT(u.lineLength == k.lineLength && u.numOfPixels == k.numOfPixels && u.class_id == k.class_id && u.response == k.response, "%s: mvKeysUn_Line[%d] is no copy", what, i);
  }
  const float* ur = reinterpret_cast<const float*>(D.rec.data() + Y.off_uright);
  const float* dp = reinterpret_cast<const float*>(D.rec.data() + Y.off_depth);
  EXPECT((int)F.mvuRight.size() == D.N && (int)F.mvDepth.size() == D.N, "%s: mvuRight %zu, mvDepth %zu rows", what, F.mvuRight.size(), F.mvDepth.size());
  for (int i = 0; i < D.N && i < (int)F.mvuRight.size(); ++i) EXPECT(F.mvuRight[i] == ur[i] && F.mvDepth[i] == dp[i], "%s: mvuRight / mvDepth [%d]", what, i);
  // mGrid: cell by cell the rows i with that cell, ascending (push_back order)
  size_t inGrid = 0, fullest = 0;
  int outside = 0;
  for (int i = 0; i < D.N; ++i) outside += D.cell[i] < 0;
  for (int cx = 0; cx < 64; ++cx)
    for (int cy = 0; cy < 48; ++cy) {
      std::vector<std::size_t> want;
      for (int i = 0; i < D.N; ++i) if (D.cell[i] == cx * 48 + cy) want.push_back((std::size_t)i);
      EXPECT(F.mGrid[cx][cy] == want, "%s: mGrid[%d][%d] holds %zu rows, %zu expected, or in another order", what, cx, cy, F.mGrid[cx][cy].size(), want.size());
      inGrid += F.mGrid[cx][cy].size();
      fullest = std::max(fullest, want.size());
    }
  EXPECT(inGrid + (size_t)outside == (size_t)D.N && outside > 0 && fullest >= 2, "%s: %zu rows in the grid, %d outside, fullest cell %zu", what, inGrid, outside, fullest);
}

int main() {
  pli_frontend_config cfg;
  pli_config_default(&cfg, W, H);
  pli::Frontend fe(cfg), fe2(cfg);
  const pli_table_layout Y = fe.layout();
  cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
  K.at<float>(0, 0) = 130.f; K.at<float>(1, 1) = 129.f; K.at<float>(0, 2) = 80.f; K.at<float>(1, 2) = 60.f;
  cv::Mat dist5(5, 1, CV_32F), dist4(4, 1, CV_32F), distGated(4, 1, CV_32F);
  const float coef[5] = {0.26f, -0.95f, -0.005f, 0.0026f, 1.16f};
  for (int i = 0; i < 5; ++i) dist5.at<float>(i) = coef[i];
  for (int i = 0; i < 4; ++i) { dist4.at<float>(i) = coef[i]; distGated.at<float>(i) = i ? coef[i] : 0.f; }
  const cv::Mat depth = depthImage();

  {   // RGB-D, the first Frame: everything, the bounds included
    ORB_SLAM3::PliSingleCameraFrame<Frame> body(fe, K, dist5);
    Frame::mbInitialComputations = true;
    Frame::mnMinX = Frame::mnMaxX = Frame::mnMinY = Frame::mnMaxY = 777.f;
    Frame F;
    const cv::Mat img = image(1);
    const bool more = body.extract(F, img, &depth, 0, 0);
    fe2.setStereoCamera(F.mbf, K.at<float>(0, 0));
    float b2[4];
    pli_pinhole_distortion cam = {130.f, 129.f, 80.f, 60.f, coef[0], coef[1], coef[2], coef[3], coef[4]};
    pli::check(pli_set_pinhole_distortion(fe2.handle(), &cam, b2));
    const Direct D = direct(fe2, img, &depth, 0, 0);
    EXPECT(more && D.N > 100 && D.M > 10, "rgbd: %d keypoints, %d key lines", D.N, D.M);
    checkExtractors("rgbd", F, D, Y);
    checkBehind("rgbd", F, D, Y, true);
    int withDepth = 0;
    for (float d : F.mvDepth) withDepth += d > 0;
    EXPECT(withDepth > 0 && withDepth < D.N, "rgbd: %d of %d keypoints have a depth", withDepth, D.N);
    EXPECT(Frame::mnMinX == b2[0] && Frame::mnMaxX == b2[1] && Frame::mnMinY == b2[2] && Frame::mnMaxY == b2[3] && b2[0] != 777.f,
           "rgbd: bounds %g %g %g %g", Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY);
    EXPECT(body.bounds()[0] == b2[0] && body.bounds()[3] == b2[3], "rgbd: bounds()");
    EXPECT(Frame::mbInitialComputations, "rgbd: the flag is the constructor's to clear (Frame.cc:307)");
    if (!g_fail) std::printf("ok rgbd first frame\n");

    // the second Frame: the bounds are not written again
    Frame::mbInitialComputations = false;
    Frame::mnMinX = Frame::mnMaxX = Frame::mnMinY = Frame::mnMaxY = 555.f;
    Frame G;
    const cv::Mat img2 = image(2);
    EXPECT(body.extract(G, img2, &depth, 0, 0), "second frame");
    const Direct D2 = direct(fe2, img2, &depth, 0, 0);
    checkExtractors("second", G, D2, Y);
    checkBehind("second", G, D2, Y, true);
    EXPECT(Frame::mnMinX == 555.f && Frame::mnMaxX == 555.f && Frame::mnMinY == 555.f && Frame::mnMaxY == 555.f, "second: the bounds were written again");
    if (!g_fail) std::printf("ok second frame keeps the bounds\n");

    // a Frame without keypoints: the constructor returns behind the extractors (Frame.cc:270-271); nothing else is touched
    Frame::mbInitialComputations = true;
    Frame E;
    E.mvKeysUn.assign(3, cv::KeyPoint(1.f, 2.f, 3.f));
    E.mvKeysUn_Line.resize(2);
    E.mvuRight.assign(4, 9.f);
    E.mvDepth.assign(4, 8.f);
    cv::Mat flat(H, W, CV_8UC1);
    std::memset(flat.data, 90, (size_t)W * H);
    EXPECT(!body.extract(E, flat, &depth, 0, 0), "empty: extract() must return false");
    const Direct D3 = direct(fe2, flat, &depth, 0, 0);
    EXPECT(D3.N == 0 && D3.M > 0, "empty: %d keypoints, %d key lines", D3.N, D3.M);
    checkExtractors("empty", E, D3, Y);
    EXPECT(E.mvKeysUn.size() == 3 && E.mvKeysUn_Line.size() == 2 && E.mvuRight.size() == 4 && E.mvuRight[0] == 9.f && E.mvDepth.size() == 4 && E.mvDepth[0] == 8.f,
           "empty: members behind the early return were written");
    size_t inGrid = 0;
    for (int cx = 0; cx < 64; ++cx) for (int cy = 0; cy < 48; ++cy) inGrid += E.mGrid[cx][cy].size();
    EXPECT(inGrid == 0 && Frame::mnMinX == 555.f, "empty: grid rows %zu, mnMinX %g", inGrid, Frame::mnMinX);
    if (!g_fail) std::printf("ok empty frame returns early\n");
  }
  {   // monocular, 4 coefficients, the lapping area of Frame.cc:360
    ORB_SLAM3::PliSingleCameraFrame<Frame> body(fe, K, dist4);
    Frame::mbInitialComputations = true;
    Frame F;
    const cv::Mat img = image(3);
    EXPECT(body.extract(F, img, nullptr, 0, 1000), "mono");
    pli_pinhole_distortion cam = {130.f, 129.f, 80.f, 60.f, coef[0], coef[1], coef[2], coef[3], 0.f};
    pli::check(pli_set_pinhole_distortion(fe2.handle(), &cam, nullptr));
    const Direct D = direct(fe2, img, nullptr, 0, 1000);
    checkExtractors("mono", F, D, Y);
    checkBehind("mono", F, D, Y, true);
    EXPECT(F.monoLeft == 0, "mono: every keypoint lies in [0, 1000], monoLeft %d", F.monoLeft);
    bool allMinus = true;
    for (size_t i = 0; i < F.mvuRight.size(); ++i) allMinus = allMinus && F.mvuRight[i] == -1.f && F.mvDepth[i] == -1.f;
    EXPECT(allMinus && F.mvuRight.size() == F.mvKeys.size(), "mono: mvuRight / mvDepth must be -1 (Frame.cc:384-385)");
    if (!g_fail) std::printf("ok monocular frame\n");
  }
  {   // k1 == 0 with the other coefficients set: copies (Frame.cc:874-878, :909-913) and the image's own bounds
    ORB_SLAM3::PliSingleCameraFrame<Frame> body(fe, K, distGated);
    Frame::mbInitialComputations = true;
    Frame F;
    const cv::Mat img = image(4);
    EXPECT(body.extract(F, img, &depth, 0, 0), "gated");
    pli_pinhole_distortion cam = {130.f, 129.f, 80.f, 60.f, 0.f, coef[1], coef[2], coef[3], 0.f};
    pli::check(pli_set_pinhole_distortion(fe2.handle(), &cam, nullptr));
    const Direct D = direct(fe2, img, &depth, 0, 0);
    checkExtractors("gated", F, D, Y);
    checkBehind("gated", F, D, Y, false);
    EXPECT(Frame::mnMinX == 0.f && Frame::mnMaxX == (float)W && Frame::mnMinY == 0.f && Frame::mnMaxY == (float)H, "gated: bounds %g %g %g %g",
           Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY);
    if (!g_fail) std::printf("ok k1 == 0 copies\n");
  }
  {   // arguments the adapter refuses
    int thrown = 0;
    try { ORB_SLAM3::PliSingleCameraFrame<Frame> bad(fe, cv::Mat(3, 4, CV_32F), dist4); } catch (const std::invalid_argument&) { ++thrown; }
    try { ORB_SLAM3::PliSingleCameraFrame<Frame> bad(fe, K, cv::Mat(3, 1, CV_32F)); } catch (const std::invalid_argument&) { ++thrown; }
    ORB_SLAM3::PliSingleCameraFrame<Frame> body(fe, K, dist4);
    Frame F;
    try { body.extract(F, cv::Mat(H, W, CV_32F), nullptr, 0, 0); } catch (const std::invalid_argument&) { ++thrown; }
    const cv::Mat small(H / 2, W, CV_32F);
    try { body.extract(F, image(5), &small, 0, 0); } catch (const std::invalid_argument&) { ++thrown; }
    EXPECT(thrown == 4, "%d of 4 bad arguments were refused", thrown);
    if (!g_fail) std::printf("ok bad arguments\n");
  }
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("all ok\n");
  return 0;
}
