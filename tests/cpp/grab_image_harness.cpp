// Host test of pli_slam_amd/adapters/tracking_grab.hpp and of PliSingleCameraFrame::extractRaw (tests/test_cpp_grab_image.py; a
// stand-alone program, linked against tests/cpp/mock_pli.cpp).  TEST-ONLY: beside that mock this file brings stand-ins of its own for
// pli_set_image_format and pli_set_depth_format, which record their calls, and for pli_set_pinhole_distortion and
// pli_frame_extract_single, which records its arguments and returns a Frame without keypoints.  Checked: the image format PliGrabImage
// picks for 1, 3 and 4 channels with and without mbRGB (Tracking.cc:889-914); 2 channels and a 16-bit image throw; the setters are
// called only when a setting changes; the gate of :979 on four depth maps; depth types other than CV_32F / CV_16U throw; extractRaw
// hands pointers and strides on untouched.  The cv::Mat reading runs on a Mat-like struct of this file (the stub core.hpp knows
// neither colour nor 16-bit types).
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
#include "pli_slam_amd/adapters/tracking_grab.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using cv::line_descriptor::KeyLine;
using ORB_SLAM3::PliGrabImage;

// ---- the stand-ins -------------------------------------------------------------------------------------------------------------
struct FormatCall { int fmt; };
struct DepthCall { int type; float scale; };
static std::vector<FormatCall> g_formatCalls;
static std::vector<DepthCall> g_depthCalls;
struct SingleCall {
  const uint8_t* img = nullptr; int w = 0, h = 0; int64_t stride = 0; int lap0 = 0, lap1 = 0; const float* depth = nullptr; int64_t depthStride = 0;
  int calls = 0;
};
static SingleCall g_single;

extern "C" {
pli_status pli_set_image_format(pli_ctx* c, pli_image_format fmt) {
  if (!c || (int)fmt < 0 || (int)fmt > (int)PLI_IMAGE_BGRA8) return PLI_ERR_INVALID;
  g_formatCalls.push_back({(int)fmt});
  return PLI_OK;
}
pli_status pli_set_depth_format(pli_ctx* c, pli_depth_type type, float scale) {
  if (!c || ((int)type != PLI_DEPTH_F32 && (int)type != PLI_DEPTH_U16)) return PLI_ERR_INVALID;
  g_depthCalls.push_back({(int)type, scale});
  return PLI_OK;
}
pli_status pli_set_pinhole_distortion(pli_ctx* c, const pli_pinhole_distortion*, float bounds[4]) {
  if (!c) return PLI_ERR_INVALID;
  if (bounds) { bounds[0] = bounds[2] = 0.f; bounds[1] = 160.f; bounds[3] = 120.f; }
  return PLI_OK;
}
pli_status pli_frame_extract_single(pli_ctx* c, const uint8_t* img, int32_t w, int32_t h, int64_t stride, int32_t lap0, int32_t lap1,
                                    const float* depth, int64_t depthStride, void* record, float* kpUn, float* klUn, int32_t* cell,
                                    int32_t* nMono) {
  if (!c || !record || !kpUn || !klUn || !cell || !nMono) return PLI_ERR_INVALID;
  pli_table_layout Y;
  pli_ctx_layout(c, &Y);
  std::memset(record, 0, (size_t)Y.record_bytes);      // counts 0: a Frame without keypoints or key lines
  *nMono = 0;
  g_single.img = img; g_single.w = w; g_single.h = h; g_single.stride = stride; g_single.lap0 = lap0; g_single.lap1 = lap1;
  g_single.depth = depth; g_single.depthStride = depthStride; ++g_single.calls;
  return PLI_OK;
}
}

// ---- a Mat-like struct: the members PliGrabImage's templates read --------------------------------------------------------------
struct TestMat {
  unsigned char* data = nullptr;
  int cols = 0, rows = 0;
  size_t step = 0;                       // bytes per row
  int nch = 1, dep = PliGrabImage::kDepth8U;
  std::vector<unsigned char> buf;
  TestMat(int r, int c, int channels, int depthCode, size_t padBytes = 0, size_t baseOffset = 0) : cols(c), rows(r), nch(channels), dep(depthCode) {
    const size_t elem = depthCode == PliGrabImage::kDepth32F ? 4 : depthCode == PliGrabImage::kDepth16U ? 2 : 1;
    step = (size_t)c * channels * elem + padBytes;
    buf.assign(baseOffset + (size_t)r * step, 7);
    data = buf.data() + baseOffset;
  }
  int channels() const { return nch; }
  int depth() const { return dep; }
};

struct Frame {                         // the members PliSingleCameraFrame writes, with the reference's names and types (include/Frame.h)
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

template <class Fn>
static bool throwsInvalid(Fn fn) {
  try { fn(); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main() {
  pli_frontend_config cfg;
  pli_config_default(&cfg, W, H);
  cfg.orb_nfeatures = 300; cfg.lsd_nfeatures = 50;
  pli::Frontend fe(cfg);

  {  // Tracking.cc:889-914
    const struct { int ch; bool rgb; pli_image_format want; } T[] = {
        {1, true, PLI_IMAGE_GRAY8}, {1, false, PLI_IMAGE_GRAY8}, {3, true, PLI_IMAGE_RGB8}, {3, false, PLI_IMAGE_BGR8},
        {4, true, PLI_IMAGE_RGBA8}, {4, false, PLI_IMAGE_BGRA8}};
    for (const auto& t : T) {
      EXPECT(PliGrabImage::formatOf(t.ch, t.rgb) == t.want, "%d channels, mbRGB %d", t.ch, (int)t.rgb);
      g_formatCalls.clear();
      PliGrabImage grab(fe, t.rgb);
      TestMat im(H, W, t.ch, PliGrabImage::kDepth8U);
      const pli::ImageView v = grab.image(im);
      EXPECT(grab.format() == t.want && v.channels == t.ch && v.data == im.data && v.cols == W && v.rows == H && v.step == (int64_t)im.step,
             "%d channels, mbRGB %d: format %d", t.ch, (int)t.rgb, (int)grab.format());
      // a fresh context reads gray: one call for a colour format, none for gray
      EXPECT(g_formatCalls.size() == (t.ch == 1 ? 0u : 1u) && (t.ch == 1 || g_formatCalls[0].fmt == (int)t.want), "%d channels: %zu setter calls", t.ch, g_formatCalls.size());
    }
    std::printf("ok format for 1, 3 and 4 channels\n");
  }

  {
    PliGrabImage grab(fe, true);
    g_formatCalls.clear();
    TestMat two(H, W, 2, PliGrabImage::kDepth8U), wide(H, W, 3, PliGrabImage::kDepth16U), zero(H, W, 0, PliGrabImage::kDepth8U);
    EXPECT(throwsInvalid([&] { grab.image(two); }), "2 channels");
    EXPECT(throwsInvalid([&] { grab.image(zero); }), "0 channels");
    EXPECT(throwsInvalid([&] { grab.image(wide); }), "a 16-bit image");
    EXPECT(throwsInvalid([&] { PliGrabImage::formatOf(5, false); }), "5 channels");
    EXPECT(g_formatCalls.empty(), "a refused image reached the setter");
    std::printf("ok 2 channels throw\n");
  }

  {
    PliGrabImage grab(fe, false, 1.0f / 5000.0f);
    g_formatCalls.clear(); g_depthCalls.clear();
    TestMat bgr(H, W, 3, PliGrabImage::kDepth8U), bgra(H, W, 4, PliGrabImage::kDepth8U), gray(H, W, 1, PliGrabImage::kDepth8U);
    TestMat d16(H, W, 1, PliGrabImage::kDepth16U), d32(H, W, 1, PliGrabImage::kDepth32F);
    grab.image(bgr); grab.image(bgr); grab.image(bgr);
    EXPECT(g_formatCalls.size() == 1 && g_formatCalls[0].fmt == PLI_IMAGE_BGR8, "three BGR frames: %zu calls", g_formatCalls.size());
    EXPECT(grab.imageRight(bgr).data == bgr.data && g_formatCalls.size() == 1, "the right image calls no setter");
    EXPECT(throwsInvalid([&] { grab.imageRight(gray); }), "a gray right image beside a BGR left one");
    grab.image(bgra);
    EXPECT(g_formatCalls.size() == 2 && g_formatCalls[1].fmt == PLI_IMAGE_BGRA8, "then BGRA: %zu calls", g_formatCalls.size());
    grab.image(gray); grab.image(gray);
    EXPECT(g_formatCalls.size() == 3 && g_formatCalls[2].fmt == PLI_IMAGE_GRAY8, "then gray twice: %zu calls", g_formatCalls.size());
    grab.depth(d16); grab.depth(d16);
    EXPECT(g_depthCalls.size() == 1 && g_depthCalls[0].type == PLI_DEPTH_U16 && g_depthCalls[0].scale == 1.0f / 5000.0f, "two uint16 maps: %zu calls", g_depthCalls.size());
    grab.depth(d32);
    EXPECT(g_depthCalls.size() == 2 && g_depthCalls[1].type == PLI_DEPTH_F32 && g_depthCalls[1].scale == 1.0f / 5000.0f, "then a float map: %zu calls", g_depthCalls.size());
    grab.depth(d32);
    EXPECT(g_depthCalls.size() == 2, "the same float map again: %zu calls", g_depthCalls.size());
    std::printf("ok setters called only on change\n");
  }

  {  // Tracking.cc:979
    const float nearOne = 1.0f + 5e-6f;
    const struct { int dep; float factor; pli_depth_type type; float scale; size_t calls; const char* what; } T[] = {
        {PliGrabImage::kDepth32F, 1.0f, PLI_DEPTH_F32, 1.0f, 0, "F32 factor 1"},
        {PliGrabImage::kDepth32F, nearOne, PLI_DEPTH_F32, 1.0f, 0, "F32 factor 1 + 5e-6"},
        {PliGrabImage::kDepth32F, 0.5f, PLI_DEPTH_F32, 0.5f, 1, "F32 factor 0.5"},
        {PliGrabImage::kDepth16U, 1.0f, PLI_DEPTH_U16, 1.0f, 1, "U16 factor 1"}};
    EXPECT(nearOne != 1.0f && std::fabs(nearOne - 1.0f) <= 1e-5, "1 + 5e-6 is a float of its own inside the gate");
    for (const auto& t : T) {
      pli_depth_type type = PLI_DEPTH_U16;
      float scale = -1.f;
      PliGrabImage::depthFormatOf(t.dep, t.factor, &type, &scale);
      EXPECT(type == t.type && scale == t.scale, "%s: type %d, scale %.9g", t.what, (int)type, scale);
      g_depthCalls.clear();
      PliGrabImage grab(fe, true, t.factor);
      TestMat d(H, W, 1, t.dep, 6);
      const pli::DepthView v = grab.depth(d);
      EXPECT(v.type == t.type && v.data == d.data && v.step == (int64_t)d.step && v.cols == W && v.rows == H, "%s: the view", t.what);
      EXPECT(grab.depthType() == t.type && grab.depthScale() == t.scale, "%s: the setting kept", t.what);
      EXPECT(g_depthCalls.size() == t.calls && (t.calls == 0 || (g_depthCalls[0].type == (int)t.type && g_depthCalls[0].scale == t.scale)),
             "%s: %zu setter calls", t.what, g_depthCalls.size());
    }
    PliGrabImage grab(fe, true, 1.0f);
    TestMat d8(H, W, 1, PliGrabImage::kDepth8U), d2(H, W, 2, PliGrabImage::kDepth16U);
    EXPECT(throwsInvalid([&] { grab.depth(d8); }), "a CV_8U depth map");
    EXPECT(throwsInvalid([&] { grab.depth(d2); }), "a two-channel depth map");
    pli_depth_type type; float scale;
    EXPECT(throwsInvalid([&] { PliGrabImage::depthFormatOf(6 /* CV_64F */, 1.0f, &type, &scale); }), "a CV_64F depth map");
    std::printf("ok depth gate of Tracking.cc:979\n");
  }

  {
    cv::Mat K = cv::Mat::eye(3, 3, CV_32F), dist(4, 1, CV_32F);
    K.at<float>(0, 0) = 535.4f; K.at<float>(1, 1) = 539.2f; K.at<float>(0, 2) = 320.1f; K.at<float>(1, 2) = 247.6f;
    ORB_SLAM3::PliSingleCameraFrame<Frame> single(fe, K, dist);
    PliGrabImage grab(fe, true, 1.0f / 5000.0f);
    // a colour image with padded rows whose first byte lies one byte into its buffer, a uint16 map with padded rows
    TestMat rgb(H, W, 3, PliGrabImage::kDepth8U, 5, 1), d16(H, W, 1, PliGrabImage::kDepth16U, 6), d32(H, W, 1, PliGrabImage::kDepth32F, 8);
    Frame F;
    const pli::ImageView iv = grab.image(rgb);
    const pli::DepthView dv = grab.depth(d16);
    g_single = SingleCall();
    EXPECT(!single.extractRaw(F, iv, &dv, 0, 0), "a Frame without keypoints returns false");
    EXPECT(g_single.calls == 1 && g_single.img == rgb.data && g_single.w == W && g_single.h == H && g_single.stride == (int64_t)(W * 3 + 5),
           "image: stride %lld", (long long)g_single.stride);
    EXPECT((const void*)g_single.depth == (const void*)d16.data && g_single.depthStride == (int64_t)(W * 2 + 6) / 2 && g_single.lap0 == 0 && g_single.lap1 == 0,
           "uint16 depth: stride %lld elements", (long long)g_single.depthStride);
    const pli::DepthView fv = grab.depth(d32);
    g_single = SingleCall();
    single.extractRaw(F, iv, &fv, 0, 1000);
    EXPECT((const void*)g_single.depth == (const void*)d32.data && g_single.depthStride == (int64_t)(W * 4 + 8) / 4 && g_single.lap0 == 0 && g_single.lap1 == 1000,
           "float depth: stride %lld elements", (long long)g_single.depthStride);
    g_single = SingleCall();
    single.extractRaw(F, iv, nullptr, 0, 1000);
    EXPECT(g_single.calls == 1 && g_single.depth == nullptr && g_single.depthStride == 0 && g_single.img == rgb.data, "monocular: no depth map");
    // extract() still takes the gray / CV_32F Mats of the reference's constructors and goes the same way
    cv::Mat gray(H, W, CV_8UC1), depth(H, W, CV_32F);
    g_single = SingleCall();
    single.extract(F, gray, &depth, 0, 0);
    EXPECT(g_single.calls == 1 && g_single.img == gray.data && g_single.stride == (int64_t)gray.step && (const void*)g_single.depth == (const void*)depth.data &&
           g_single.depthStride == (int64_t)W, "extract(): stride %lld, depth stride %lld", (long long)g_single.stride, (long long)g_single.depthStride);
    std::printf("ok extractRaw forwards pointers and strides\n");
  }

  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("all ok\n");
  return 0;
}
