// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over the reference's own line front end: src/LineExtractor.cc, src/Config.cpp,
// Thirdparty/line_descriptor/src/LSDDetector_custom.cpp and binary_descriptor_custom.cpp, which oracle/Makefile
// compiles from the reference tree (never copied) against line_shim/ and the reference's real headers.  The four
// OpenCV primitives those translation units leave undefined are defined here over the oracle's restatements:
// LineSegmentDetector::detect over orc::lsdDetect, LineIterator over lineIteratorCount, GaussianBlur over
// gaussianBlur8u, Sobel over sobel3x3_16s.  Everything between them is the reference's compiled code: the clamps,
// the float/double length, the min_length gate, every KeyLine field, std::sort by response, the cut, the
// re-numbering, computeImpl's ScaleLines bookkeeping, computeSobel, computeLBD, binaryConversion and the weights.
//
//   pli_ref_line REQUEST RESPONSE          (line_shim includes <cmath> only)
//   pli_ref_line_mathh REQUEST RESPONSE    (-DPLI_LINE_SHIM_MATH_H: line_shim also includes <math.h>)
//
// REQUEST : int32 mode (0: run the detector, 1: the detector returns the segment list below), W, H, lsd_nfeatures,
//           lsd_refine, lsd_n_bins, lsd_flags (1: CV_64F input, 2: float trig in the grower), nseg;
//           float64 min_line_length, lsd_scale, lsd_sigma_scale, lsd_quant, lsd_ang_th, lsd_log_eps, lsd_density_th;
//           W*H image bytes; nseg x 4 float32.
// RESPONSE: int32 nseg, nseg x 4 float32 (what the detector stand-in returned, before the clamps);
//           int32 n, n x KeyLine (17 fields, 68 bytes, the struct's own order);
//           int32 rows, rows x 32 descriptor bytes (rows = 0 where descriptors_line was left untouched);
//           int32 rowsF, rowsF x 72 float32 (a second compute(..., returnFloatDescr = true) on the same key lines);
//           int32 planes (0 or 1), then W*H int16 dx and W*H int16 dy of that second call's computeSobel.
#include "pli_line_shim.hpp"
#include "LineExtractor.h"
#include "../ocv_prims.hpp"
#include "../line_oracle.hpp"

static bool g_segment_mode = false;
static std::vector<float> g_request_segments, g_returned_segments;
static int g_lsd_flags = 1;

namespace cv {

static orc::Img8 toImg(const Mat& m) {
  if (m.type() != CV_8UC1) PLI_SHIM_DEAD("a primitive on a Mat that is not CV_8UC1");
  orc::Img8 o(m.cols, m.rows);
  for (int y = 0; y < m.rows; ++y) std::memcpy(o.row(y), m.ptr(y), m.cols);
  return o;
}

// src may be dst: it is copied out first
void GaussianBlur(const Mat& src, Mat& dst, Size k, double sx, double sy, int border) {
  if (k.width != k.height || sy != 0 || border != BORDER_DEFAULT) PLI_SHIM_DEAD("GaussianBlur with these arguments");
  orc::Img8 s = toImg(src), d;
  orc::gaussianBlur8u(s, d, k.width, sx);
  dst.create(d.h, d.w, CV_8UC1);
  for (int y = 0; y < d.h; ++y) std::memcpy(dst.ptr(y), d.row(y), d.w);
}

void Sobel(const Mat& src, Mat& dst, int ddepth, int dx, int dy, int ksize, double scale, double delta, int border) {
  if (ddepth != CV_16SC1 || dx + dy != 1 || ksize != 3 || scale != 1 || delta != 0 || border != BORDER_DEFAULT)
    PLI_SHIM_DEAD("Sobel with these arguments");
  std::vector<int16_t> gx, gy;
  orc::sobel3x3_16s(toImg(src), gx, gy);
  dst.create(src.rows, src.cols, CV_16SC1);
  const std::vector<int16_t>& g = dx ? gx : gy;
  for (int y = 0; y < src.rows; ++y) std::memcpy(dst.ptr(y), g.data() + (size_t)y * src.cols, (size_t)src.cols * 2);
}

LineIterator::LineIterator(const Mat&, Point2f a, Point2f b) : count(orc::lineIteratorCount(a.x, a.y, b.x, b.y)) {}

struct LsdStandIn : LineSegmentDetector {
  orc::LsdParams P;
  void detect(const Mat& image, std::vector<Vec4f>& lines) override {
    std::vector<float> segs;
    if (g_segment_mode) {
      segs = g_request_segments;
    } else {
      orc::LsdDebug D;
      orc::lsdDetect(toImg(image), P, D);
      segs = D.segments;
    }
    g_returned_segments = segs;
    lines.clear();
    for (size_t k = 0; k + 3 < segs.size(); k += 4) {
      Vec4f v;
      for (int i = 0; i < 4; ++i) v[i] = segs[k + i];
      lines.push_back(v);
    }
  }
};

Ptr<LineSegmentDetector> createLineSegmentDetector(int refine, double scale, double sigma_scale, double quant, double ang_th,
                                                   double log_eps, double density_th, int n_bins) {
  LsdStandIn* d = new LsdStandIn();
  d->P.refine = refine; d->P.scale = scale; d->P.sigma_scale = sigma_scale; d->P.quant = quant; d->P.ang_th = ang_th;
  d->P.log_eps = log_eps; d->P.density_th = density_th; d->P.n_bins = n_bins;
  d->P.input_f64 = (g_lsd_flags & 1) != 0;
  d->P.trig_f32 = (g_lsd_flags & 2) != 0;
  if (refine != 0) PLI_SHIM_DEAD("LineSegmentDetector with refine != LSD_REFINE_NONE");
  return Ptr<LineSegmentDetector>(d);
}

}  // namespace cv

static bool readAll(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
static void put(FILE* f, const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, f) != n) { std::perror("write"); std::exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s REQUEST RESPONSE\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t hdr[8];
  double par[7];
  if (!readAll(in, hdr, sizeof hdr) || !readAll(in, par, sizeof par)) { std::fprintf(stderr, "short request header\n"); return 2; }
  const int32_t mode = hdr[0], W = hdr[1], H = hdr[2], nfeatures = hdr[3], refine = hdr[4], n_bins = hdr[5], nseg = hdr[7];
  g_lsd_flags = hdr[6];
  // computeLBD holds the image sizes and a line's pixel count in shorts
  if (mode < 0 || mode > 1 || W <= 0 || H <= 0 || W > 32767 || H > 32767 || nseg < 0 || nseg > (1 << 20)) {
    std::fprintf(stderr, "bad request header\n");
    return 2;
  }
  cv::Mat image(H, W, CV_8UC1);
  g_request_segments.resize((size_t)nseg * 4);
  if (!readAll(in, image.data, (size_t)W * H) || !readAll(in, g_request_segments.data(), (size_t)nseg * 16)) {
    std::fprintf(stderr, "short request\n");
    return 2;
  }
  std::fclose(in);
  g_segment_mode = mode == 1;

  // as Tracking.cc constructs it
  ORB_SLAM3::Lineextractor ex(nfeatures, par[0], refine, par[1], par[2], par[3], par[4], par[5], par[6], n_bins, false);
  std::vector<cv::line_descriptor::KeyLine> kls;
  cv::Mat desc;
  ex(image, cv::Mat(), kls, desc);

  cv::Ptr<cv::line_descriptor::BinaryDescriptor> lbd = cv::line_descriptor::BinaryDescriptor::createBinaryDescriptor();
  cv::Mat fdesc;
  std::vector<cv::line_descriptor::KeyLine> kls2 = kls;
  lbd->compute(image, kls2, fdesc, true);

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const int32_t nret = (int32_t)(g_returned_segments.size() / 4);
  put(out, &nret, 4);
  put(out, g_returned_segments.data(), (size_t)nret * 16);
  const int32_t n = (int32_t)kls.size();
  put(out, &n, 4);
  for (const cv::line_descriptor::KeyLine& k : kls) {
    put(out, &k.angle, 4);
    const int32_t ci[2] = {k.class_id, k.octave};
    put(out, ci, 8);
    const float f[13] = {k.pt.x, k.pt.y, k.response, k.size, k.startPointX, k.startPointY, k.endPointX, k.endPointY,
                         k.sPointInOctaveX, k.sPointInOctaveY, k.ePointInOctaveX, k.ePointInOctaveY, k.lineLength};
    put(out, f, sizeof f);
    const int32_t np = k.numOfPixels;
    put(out, &np, 4);
  }
  const int32_t rows = desc.empty() ? 0 : desc.rows;
  if (rows && (desc.type() != CV_8UC1 || desc.cols != 32 || rows != n)) { std::fprintf(stderr, "unexpected descriptor matrix\n"); return 3; }
  put(out, &rows, 4);
  for (int i = 0; i < rows; ++i) put(out, desc.ptr(i), 32);
  const int32_t rowsF = fdesc.empty() ? 0 : fdesc.rows;
  if (rowsF && (fdesc.type() != CV_32FC1 || fdesc.cols != 72 || rowsF != n)) { std::fprintf(stderr, "unexpected float descriptor matrix\n"); return 3; }
  put(out, &rowsF, 4);
  for (int i = 0; i < rowsF; ++i) put(out, fdesc.ptr(i), 72 * 4);
  const int32_t planes = lbd->dxImg_vector.empty() ? 0 : 1;
  put(out, &planes, 4);
  if (planes) {
    const cv::Mat& dx = lbd->dxImg_vector[0];
    const cv::Mat& dy = lbd->dyImg_vector[0];
    if (dx.rows != H || dx.cols != W || dy.rows != H || dy.cols != W || dx.type() != CV_16SC1 || dy.type() != CV_16SC1) {
      std::fprintf(stderr, "unexpected gradient planes\n");
      return 3;
    }
    for (int y = 0; y < H; ++y) put(out, dx.ptr(y), (size_t)W * 2);
    for (int y = 0; y < H; ++y) put(out, dy.ptr(y), (size_t)W * 2);
  }
  if (std::fclose(out) != 0) { std::perror("close"); return 2; }
  return 0;
}
