// Host side of libpli_frontend.so: context, geometry tables, stage scheduling
// on one HIP stream, and the extern "C" entry points of include/pli_frontend.h
// that create a context, extract, match the context's own record or measure
// (the line chain, runLines and its stages: line_chain.hip; the stateless matcher entry points: match_capi.hip; what they share:
// capi_host.hpp).
// There is no CPU fallback: without a gfx950 device every compute entry point
// fails with PLI_ERR_NO_DEVICE.
#include "capi_host.hpp"
#include <cmath>
#include <cfloat>
#include <algorithm>
#include <memory>
#include <limits>

thread_local std::string g_err;

namespace {

inline int cvRoundf(float v) { return (int)std::nearbyintf(v); }
inline int cvRoundd(double v) { return (int)std::nearbyint(v); }
inline int cvFloorf(float v) { int i = (int)v; return i - (i > v); }

// tiles of 32 for contexts of up to 32 frames of 752x480 (four times the waves where 64-pixel tiles leave the chip under-occupied: a
// single stereo pair takes 4.6 instead of 7.3 ms with the round-1 code; now, frames/s with 32 vs 64: 16 frames 2228 vs 2066,
// 32 frames 2930 vs 2777; from 64 frames on the extra border conflicts cost more: 3343 vs 3445, 128 frames 3568 vs 3782)
// — in tile waves: 32 frames of 752x480 are 64 x 135 = 8640 waves of 64-pixel tiles, about what the chip holds at once (7168)
constexpr int TX_SMALL_TILE_WAVES = 12000;

}  // namespace

PliRoctx g_roctx;

namespace {

// The CV_64F front of the LSD (lsd_f64.hip).  Gaussian kernel in double (cv::getGaussianKernel(n, sigma, CV_64F)); radius 0 / kernel
// {1} converts u8 -> double (lsd_scale 1).  Returns the radius, -1 above 3.
int lsdGauss64(double lsdScale, double sigmaScale, double k[7]) {
  const double sigma = (lsdScale < 1) ? (sigmaScale / lsdScale) : sigmaScale;
  const unsigned h = lsdScale != 1 ? (unsigned)std::ceil(sigma * std::sqrt(2 * 3.0 * std::log(10.0))) : 0u;
  if (h > 3) return -1;
  for (int i = 0; i < 7; ++i) k[i] = 0;
  const int n = 1 + 2 * (int)h;
  if (h == 0) k[0] = 1.0;
  else {
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; k[i] = std::exp(scale2X * x * x); sum += k[i]; }
    sum = 1. / sum;
    for (int i = 0; i < n; ++i) k[i] *= sum;
  }
  return (int)h;
}

// cv::resize coefficient tables for CV_64F (imgwarp.cpp): float weights (1 - f, f), x clamped at the borders, y not.
// xofs[dw] | alpha[2*dw] (float bits) | yofs[dh] | beta[2*dh] (float bits); sc = 1 / lsd_scale.
std::vector<int> buildResizeTab64(int sw, int sh, int dw, int dh, double sc) {
  std::vector<int> t((size_t)3 * dw + 3 * dh);
  auto fbits = [](float f) { int b; std::memcpy(&b, &f, 4); return b; };
  for (int d = 0; d < dw; ++d) {
    float f = (float)((d + 0.5) * sc - 0.5);
    int sidx = cvFloorf(f);
    f -= sidx;
    if (sidx < 0) { f = 0; sidx = 0; }
    if (sidx >= sw - 1) { f = 0; sidx = sw - 1; }
    t[d] = sidx; t[dw + 2 * d] = fbits(1.f - f); t[dw + 2 * d + 1] = fbits(f);
  }
  for (int d = 0; d < dh; ++d) {
    float f = (float)((d + 0.5) * sc - 0.5);
    int sidx = cvFloorf(f);
    f -= sidx;
    t[3 * dw + d] = sidx; t[3 * dw + dh + 2 * d] = fbits(1.f - f); t[3 * dw + dh + 2 * d + 1] = fbits(f);
  }
  return t;
}

// both fused fronts give the source window of a strip of 64 (+ 1) scaled columns 64 columns: of LDS (k_lsd_front64), of lanes (k_lsd_front64s)
bool frontStripsFit(const std::vector<int>& t, int sw, int dw) {
  for (int x0 = 0; x0 < dw; x0 += 64) {
    const int x1 = std::min(x0 + 64, dw - 1);
    if (std::min(t[x1] + 1, sw - 1) - t[x0] + 1 > 64) return false;
  }
  return true;
}

// the fused front (k_lsd_front64) stages the source window of a 64 x 16 tile of the scaled image in LDS: 64 x 20 at most
bool frontTiledFits(const std::vector<int>& t, int sw, int sh, int dw, int dh, int radius) {
  bool fits = radius <= 3 && frontStripsFit(t, sw, dw);
  for (int y0 = 0; y0 < dh && fits; y0 += 16) {
    const int y1 = std::min(y0 + 16, dh - 1);
    const int a = std::min(std::max(t[3 * dw + y0], 0), sh - 1), b = std::min(std::max(t[3 * dw + y1] + 1, 0), sh - 1);
    fits = b - a + 1 <= 20;
  }
  return fits;
}

// the streaming front (k_lsd_front64s): radius 3 with one reflection at the borders, the source window of every strip within the
// wave's 64 lanes, and source rows and columns that advance by 0 or 1 per scaled one
bool frontStreamFits(const std::vector<int>& t, int sw, int sh, int dw, int dh, int radius) {
  if (radius != 3 || sw <= 6 || sh <= 6 || dw < 1 || dh < 1 || !frontStripsFit(t, sw, dw)) return false;
  for (int d = 1; d < dw; ++d) if (t[d] - t[d - 1] < 0 || t[d] - t[d - 1] > 1) return false;
  for (int d = 1; d < dh; ++d) if (t[3 * dw + d] - t[3 * dw + d - 1] < 0 || t[3 * dw + d] - t[3 * dw + d - 1] > 1) return false;
  return true;
}

// the form for a geometry (t: buildResizeTab64); dev switch PLI_LSD_NOFUSE: the three kernels
LsdFront frontForm(const std::vector<int>& t, int sw, int sh, int dw, int dh, int radius) {
  if (!frontTiledFits(t, sw, sh, dw, dh, radius) || DEVENV("PLI_LSD_NOFUSE")) return LsdFront::Unfused;
  return frontStreamFits(t, sw, sh, dw, dh, radius) ? LsdFront::Stream : LsdFront::Tiled;
}

// cv::resize coefficient tables (see oracle/ocv_prims.hpp for the derivation):
// xofs[dw] | alpha[2*dw] | yofs[dh] | beta[2*dh], all int32.
std::vector<int> buildResizeTab(int sw, int sh, int dw, int dh, double scale_x, double scale_y) {
  std::vector<int> t((size_t)3 * dw + 3 * dh);
  for (int d = 0; d < dw; ++d) {
    float f = (float)((d + 0.5) * scale_x - 0.5);
    int s = cvFloorf(f);
    f -= s;
    if (s < 0) { f = 0; s = 0; }
    if (s >= sw - 1) { f = 0; s = sw - 1; }
    t[d] = s;
    t[dw + 2 * d] = (short)cvRoundf((1.f - f) * 2048.f);
    t[dw + 2 * d + 1] = (short)cvRoundf(f * 2048.f);
  }
  for (int d = 0; d < dh; ++d) {
    float f = (float)((d + 0.5) * scale_y - 0.5);
    int s = cvFloorf(f);
    f -= s;
    t[3 * dw + d] = s;
    t[3 * dw + dh + 2 * d] = (short)cvRoundf((1.f - f) * 2048.f);
    t[3 * dw + dh + 2 * d + 1] = (short)cvRoundf(f * 2048.f);
  }
  return t;
}

void gaussKernelFixed8(int n, double sigma, int* k) {
  std::vector<float> cf(n);
  double scale2X = -0.5 / (sigma * sigma), sum = 0;
  for (int i = 0; i < n; ++i) {
    double x = i - (n - 1) * 0.5;
    cf[i] = (float)std::exp(scale2X * x * x);
    sum += cf[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) {
    cf[i] = (float)(cf[i] * sum);
    k[i] = cvRoundd((double)cf[i] * 256.0);
  }
}

pli_status validate(const pli_frontend_config& c) {
  if (c.width < 64 || c.height < 64 || c.width > 4095 || c.height > 4095) { g_err = "width/height must be in [64,4095]"; return PLI_ERR_INVALID; }
  if (c.max_frames < 1) { g_err = "max_frames < 1"; return PLI_ERR_INVALID; }
  if (c.orb_nlevels < 1 || c.orb_nlevels > MAX_LEVELS) { g_err = "orb_nlevels out of range"; return PLI_ERR_INVALID; }
  if (c.orb_nfeatures < 1 || !(c.orb_scale_factor > 1.f)) { g_err = "orb_nfeatures/scale_factor invalid"; return PLI_ERR_INVALID; }
  if (c.orb_min_th_fast < 1 || c.orb_ini_th_fast < c.orb_min_th_fast || c.orb_ini_th_fast > 254) { g_err = "FAST thresholds invalid"; return PLI_ERR_INVALID; }
  if (c.lsd_refine != 0) { g_err = "only lsd_refine = 0 (LSD_REFINE_NONE) is on the reference path"; return PLI_ERR_INVALID; }
  if (c.lsd_n_bins < 1 || c.lsd_n_bins > 1024) { g_err = "lsd_n_bins must be in [1,1024]"; return PLI_ERR_INVALID; }
  if (c.max_lines < 1 || c.max_lines > (1 << 20)) { g_err = "max_lines must be in [1,2^20]"; return PLI_ERR_INVALID; }
  if (c.parity_flags < 0 || c.parity_flags > 31) { g_err = "parity_flags: unknown bits"; return PLI_ERR_INVALID; }
  if (c.lsd_mode < 0 || c.lsd_mode > 3) { g_err = "lsd_mode must be 0, 1, 2 or 3"; return PLI_ERR_INVALID; }
  if (c.lsd_nfeatures < 0 || c.lsd_nfeatures > c.max_lines) { g_err = "lsd_nfeatures must be in [0,max_lines]"; return PLI_ERR_INVALID; }
  if (!(c.lsd_scale > 0) || !(c.lsd_ang_th > 0 && c.lsd_ang_th < 180)) { g_err = "lsd_scale/ang_th invalid"; return PLI_ERR_INVALID; }
  return PLI_OK;
}

pli_status buildGeometry(pli_ctx* c) {
  const pli_frontend_config& cfg = c->cfg;
  DevParams& P = c->hp;
  std::memset(&P, 0, sizeof(P));
  P.W = cfg.width; P.H = cfg.height;
  P.nlevels = cfg.orb_nlevels;
  P.iniTh = cfg.orb_ini_th_fast; P.minTh = cfg.orb_min_th_fast;
  const int L = P.nlevels;
  // scale tables and per-level quotas, ORBextractor.cc:413-444
  std::vector<float> sc(L), inv(L);
  sc[0] = 1.0f;
  for (int i = 1; i < L; i++) sc[i] = sc[i - 1] * cfg.orb_scale_factor;
  for (int i = 0; i < L; i++) inv[i] = 1.0f / sc[i];
  std::vector<int> quota(L);
  {
    float factor = 1.0f / cfg.orb_scale_factor;
    float nDesired = cfg.orb_nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
      quota[l] = cvRoundf(nDesired);
      sum += quota[l];
      nDesired *= factor;
    }
    quota[L - 1] = std::max(cfg.orb_nfeatures - sum, 0);
  }
  int64_t off = 0;
  int cellBase = 0, kpBase = 0, candBase = 0;
  for (int l = 0; l < L; ++l) {
    LevelGeom& G = P.lv[l];
    G.scale = sc[l]; G.invScale = inv[l];
    G.w = cvRoundf((float)P.W * inv[l]);
    G.h = cvRoundf((float)P.H * inv[l]);
    G.pitch = (int)alignUp(G.w, 64);
    G.offset = off;
    off += (int64_t)G.pitch * G.h;
    off = alignUp(off, 256);
    G.minBX = 19 - 3; G.minBY = 19 - 3;
    G.maxBX = G.w - 19 + 3; G.maxBY = G.h - 19 + 3;
    const float width = (float)(G.maxBX - G.minBX), height = (float)(G.maxBY - G.minBY);
    G.nCols = width > 0 ? (int)(width / 30.f) : 0;
    G.nRows = height > 0 ? (int)(height / 30.f) : 0;
    if (G.nCols <= 0 || G.nRows <= 0) { G.nCols = 0; G.nRows = 0; G.wCell = 0; G.hCell = 0; }
    else {
      G.wCell = (int)std::ceil(width / G.nCols);
      G.hCell = (int)std::ceil(height / G.nRows);
    }
    G.cellBase = cellBase;
    cellBase += G.nCols * G.nRows;
    G.nfeatures = quota[l];
    if (G.nfeatures + 8 > 1000) { g_err = "per-level feature quota above 992 is not supported by k_octree"; return PLI_ERR_INVALID; }
    G.nIni = (G.maxBY - G.minBY) > 0 ? (int)std::round(static_cast<float>(G.maxBX - G.minBX) / (G.maxBY - G.minBY)) : 0;
    if (G.nCols == 0) G.nIni = 0;
    G.hX = G.nIni > 0 ? static_cast<float>(G.maxBX - G.minBX) / G.nIni : 1.f;
    G.kpBase = kpBase;
    G.kpCap = std::max(G.nfeatures + 4, 4 * G.nIni + 4);
    kpBase += G.kpCap;
    const int perCell = std::min(CELL_CAP, ((G.wCell + 1) / 2) * ((G.hCell + 1) / 2));
    G.candBase = candBase;
    G.candCap = G.nCols * G.nRows * perCell;
    candBase += (int)alignUp(G.candCap, 4);
  }
  P.pyrBlock = alignUp(off, 256);
  P.cellsPerImage = cellBase;
  P.kpSlotsPerImage = kpBase;
  P.candPerImage = candBase;
  P.kpCap = pli_kp_capacity(&cfg);
  P.klCap = pli_kl_capacity(&cfg);
  // umax, ORBextractor.cc:451-467
  {
    const int HP = 15;
    int umax[HP + 2] = {0};
    int v, v0, vmax = cvFloorf(HP * std::sqrt(2.f) / 2 + 1);
    int vmin = (int)std::ceil(HP * std::sqrt(2.f) / 2);
    const double hp2 = HP * HP;
    for (v = 0; v <= vmax; ++v) umax[v] = cvRoundd(std::sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
      while (umax[v0] == umax[v0 + 1]) ++v0;
      umax[v] = v0;
      ++v0;
    }
    for (int i = 0; i < 16; ++i) P.umax[i] = umax[i];
  }
  // LSD (OpenCV lsd.cpp flsd)
  P.lsdScale = cfg.lsd_scale;
  P.LWt = cfg.lsd_scale != 1 ? cvRoundd(P.W * cfg.lsd_scale) : P.W;
  P.LH = cfg.lsd_scale != 1 ? cvRoundd(P.H * cfg.lsd_scale) : P.H;
  // LW is the ROW PITCH, in pixels, of every per-pixel plane of the detector (records, norms, owner pairs, region tables' pixel
  // indices): the true width LWt rounded up to 16 pixels, so that a row of 8-byte records starts on a 128-byte line and a row of 4-byte
  // words on a 64-byte sector (902 -> 912 at 752 x 480 x 1.2: k_tx_sort's id stores and the row-wise passes touch whole sectors).  The
  // pad columns are undefined pixels — as the image's last column already is — written by the front pass; nothing after it knows the
  // true width.  Pixel indices (seed order within a bin, region ids in key mode) keep their order: (y, x) lexicographic either way.
  P.LW = (int)alignUp(P.LWt, 16);
  if (DEVENV("PLI_LSD_NOPAD")) P.LW = P.LWt;                 // dev switch (A/B)
  P.lpitch = (int)alignUp(P.LWt, 64);
  P.prec = 3.14159265358979323846 * cfg.lsd_ang_th / 180;
  {
    // Vector form of isAligned (lsd.cpp region_grow): the angle between the region's (sumdx, sumdy) and a pixel's
    // (cos, sin) is within prec  <=>  dot > 0 and dot^2 >= cos^2(prec) |sum|^2.  The sequential grower uses it with a
    // margin on both sides (fastAtan2 is within 0.01 deg of atan2) and decides only the pixels inside the margin with
    // the reference's own expression.
    double margin = 0.05 * 3.14159265358979323846 / 180;
    // (test switch PLI_ALIGN_MARGIN_DEG: a wide margin sends many more candidates through the exact expression — and, on the hot records,
    // through the exact sums; the results must not change)
    if (const char* e = DEVENV("PLI_ALIGN_MARGIN_DEG")) margin = std::max(0.05, std::min(20.0, atof(e))) * 3.14159265358979323846 / 180;
    P.hotBand2 = 0.0;
    if (const char* e = DEVENV("PLI_TX_HOT_BAND2")) P.hotBand2 = std::max(0.0, atof(e));              // test switch: 10 = the exact sums at every event
    P.rectApproxBand = 2e-3;
    if (const char* e = DEVENV("PLI_RECT_APPROX_BAND")) P.rectApproxBand = std::max(2e-3, atof(e));     // test switch: 10 = every region
    P.alignFilter = (P.prec + margin < 1.5) && (P.prec - margin > 0.01);
    const double cl = std::cos(P.prec + margin), ch = std::cos(P.prec - margin);
    // (without the filter: every candidate is a "maybe", none is "sure")
    P.alignLo = P.alignFilter ? (float)(cl * cl * (1 - 1e-5)) : -INFINITY;
    P.alignHi = P.alignFilter ? (float)(ch * ch * (1 + 1e-5)) : INFINITY;
    P.alignPad = 0;                                       // dev switches of the speculative grower
    if (const char* e = DEVENV("PLI_LSD_SPEC")) P.alignPad = atoi(e) == 3 ? 1 : atoi(e) == 4 ? 3 : 0;
    if (const char* e = DEVENV("PLI_LSD_SPEC_CAP")) P.alignPad |= std::max(0, std::min(8, atoi(e))) << 4;
  }
  {
    const double rho = cfg.lsd_quant / std::sin(P.prec);
    int g = 0;
    while (std::sqrt(g / 4.0) <= rho) ++g;     // defined  <=>  sqrt(g2/4) > rho
    P.g2Thresh = g - 1;
  }
  P.nBins = cfg.lsd_n_bins;
  P.parityFlags = cfg.parity_flags; P.parityPad = 0;
  P.rho = cfg.lsd_quant / std::sin(P.prec);
  {
    const double p = cfg.lsd_ang_th / 180;
    const double LOG_NT = 5 * (std::log10(double(P.LWt)) + std::log10(double(P.LH))) / 2 + std::log10(11.0);
    P.minRegSize = (int)size_t(-LOG_NT / std::log10(p));
  }
  P.maxLines = cfg.max_lines;
  P.lsdNFeatures = cfg.lsd_nfeatures;
  P.minLength = cfg.min_line_length * (std::min(P.W, P.H));
  P.segBoxCut = lsd_seg_box_cut(P.lsdScale, P.minLength, P.W, P.H);     // (a plain context; pli_debug_enable switches the cut off)
  P.segBoxPad = 0;
  P.bf = cfg.bf;
  P.maxD = cfg.stereo_maxd_inf ? std::numeric_limits<float>::infinity() : cfg.bf / (cfg.bf / cfg.fx);
  P.sWs = cfg.matching_s_ws; P.bestLR = cfg.best_lr_matches;
  P.lineSimTh = cfg.line_sim_th; P.overlapTh = cfg.stereo_overlap_th; P.ratio12L = cfg.min_ratio_12_l;
  P.minDispRatio = cfg.ls_min_disp_ratio; P.minDisp = cfg.min_disp; P.horizTh = cfg.line_horiz_th;
  return PLI_OK;
}

void buildLayout(pli_ctx* c) {
  pli_table_layout& L = c->lay;
  const int kc = c->hp.kpCap, lc = c->hp.klCap;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t r = o; o = alignUp(o + bytes, 16); return r; };
  L.kp_cap = kc; L.kl_cap = lc;
  L.off_counts = take(8 * 4);
  L.off_kp[0] = take((int64_t)kc * sizeof(pli_keypoint));
  L.off_kp[1] = take((int64_t)kc * sizeof(pli_keypoint));
  L.off_desc[0] = take((int64_t)kc * 32);
  L.off_desc[1] = take((int64_t)kc * 32);
  L.off_uright = take((int64_t)kc * 4);
  L.off_depth = take((int64_t)kc * 4);
  L.off_kl[0] = take((int64_t)lc * sizeof(pli_keyline));
  L.off_kl[1] = take((int64_t)lc * sizeof(pli_keyline));
  L.off_ldesc[0] = take((int64_t)lc * 32);
  L.off_ldesc[1] = take((int64_t)lc * 32);
  L.off_disp = take((int64_t)lc * 8);
  L.off_le = take((int64_t)lc * 24);
  L.record_bytes = alignUp(o, 256);
}

pli_status allocAll(pli_ctx* c) {
  const DevParams& P = c->hp;
  const int NI = c->NI;
  pli_status st;
#define A(ptr, n) if ((st = c->dalloc(&(ptr), (size_t)(n))) != PLI_OK) return st
  A(c->dP, 1);
  HIPCHK(hipMemcpy(c->dP, &c->hp, sizeof(DevParams), hipMemcpyHostToDevice));
  A(c->pyr, (size_t)P.pyrBlock * NI);
  for (int l = 1; l < P.nlevels; ++l) {
    const LevelGeom &S = P.lv[l - 1], &D = P.lv[l];
    std::vector<int> t = buildResizeTab(S.w, S.h, D.w, D.h, 1. / ((double)D.w / S.w), 1. / ((double)D.h / S.h));
    A(c->resizeTab[l], t.size());
    HIPCHK(hipMemcpy(c->resizeTab[l], t.data(), t.size() * 4, hipMemcpyHostToDevice));
  }
  A(c->cellCand, (size_t)NI * P.cellsPerImage * CELL_CAP);
  A(c->cellCount, (size_t)NI * P.cellsPerImage);
  A(c->candAll, (size_t)NI * P.candPerImage);
  A(c->nodeOf, (size_t)NI * P.candPerImage);
  A(c->candCount, (size_t)NI * P.nlevels);
  A(c->kpSel, (size_t)NI * P.kpSlotsPerImage);
  A(c->kpSelCount, (size_t)NI * P.nlevels);
  // blur jobs
  {
    BlurJob J;
    std::memset(&J, 0, sizeof(J));
    J.nplanes = P.nlevels;
    J.radius = ORB_BLUR_R;
    gaussKernelFixed8(2 * ORB_BLUR_R + 1, 2.0, J.k);
    {
      // k_describe keeps the horizontal sums of its window in 16 bits and takes them with v_dot4
      int ksum = 0, kmax = 0;
      for (int i = 0; i < 2 * ORB_BLUR_R + 1; ++i) { ksum += J.k[i]; kmax = std::max(kmax, J.k[i]); }
      if (ksum * 255 > 65535 || kmax > 255) { g_err = "ORB blur coefficients do not fit k_describe's 16-bit sums"; return PLI_ERR_INVALID; }
    }
    int tb = 0;
    for (int l = 0; l < P.nlevels; ++l) {
      BlurPlane& p = J.pl[l];
      p.w = P.lv[l].w; p.h = P.lv[l].h; p.pitchIn = p.pitchOut = P.lv[l].pitch;
      p.offIn = p.offOut = P.lv[l].offset;
      p.tilesX = (p.w + 63) / 64;
      p.tileBase = tb;
      tb += p.tilesX * ((p.h + 31) / 32);
    }
    c->orbTiles = tb;
    A(c->jobOrb, 1);
    HIPCHK(hipMemcpy(c->jobOrb, &J, sizeof(J), hipMemcpyHostToDevice));
    // LSD pre-filter: level 0 -> tmp8, kernel size from sigma (lsd.cpp)
    c->tmpPitch = (int)alignUp(P.W, 64);
    c->tmp8Stride = alignUp((int64_t)c->tmpPitch * P.H, 256);
    std::memset(&J, 0, sizeof(J));
    J.nplanes = 1;
    const double sigma = (c->cfg.lsd_scale < 1) ? (c->cfg.lsd_sigma_scale / c->cfg.lsd_scale) : c->cfg.lsd_sigma_scale;
    const unsigned h = (unsigned)std::ceil(sigma * std::sqrt(2 * 3.0 * std::log(10.0)));
    if (h > 3) { g_err = "LSD pre-filter radius > 3 not supported"; return PLI_ERR_INVALID; }
    J.radius = (int)h;
    gaussKernelFixed8(1 + 2 * (int)h, sigma, J.k);
    J.pl[0].w = P.W; J.pl[0].h = P.H; J.pl[0].pitchIn = P.lv[0].pitch; J.pl[0].pitchOut = c->tmpPitch;
    J.pl[0].offIn = P.lv[0].offset; J.pl[0].offOut = 0;
    J.pl[0].tilesX = (P.W + 63) / 64; J.pl[0].tileBase = 0;
    c->l0Tiles = J.pl[0].tilesX * ((P.H + 31) / 32);
    A(c->jobLsd, 1);
    HIPCHK(hipMemcpy(c->jobLsd, &J, sizeof(J), hipMemcpyHostToDevice));
    // LBD: 5x5 sigma 1 (binary_descriptor_custom.cpp:358)
    J.radius = LBD_BLUR_R;
    std::memset(J.k, 0, sizeof(J.k));
    gaussKernelFixed8(2 * LBD_BLUR_R + 1, 1.0, J.k);
    A(c->jobLbd, 1);
    HIPCHK(hipMemcpy(c->jobLbd, &J, sizeof(J), hipMemcpyHostToDevice));
  }
  A(c->tmp8, (size_t)c->tmp8Stride * NI);
  c->lsdStride = alignUp((int64_t)P.lpitch * P.LH, 256);
  A(c->lsdScaled, (size_t)c->lsdStride * NI);
  if (c->cfg.lsd_scale != 1) {
    std::vector<int> t = buildResizeTab(P.W, P.H, P.LWt, P.LH, 1. / c->cfg.lsd_scale, 1. / c->cfg.lsd_scale);
    A(c->lsdTab, t.size());
    HIPCHK(hipMemcpy(c->lsdTab, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  }
  const size_t npix = (size_t)P.LW * P.LH;
  A(c->rec, npix * NI);
  c->lsdF64 = (c->cfg.parity_flags & PLI_PARITY_LSD_F64) != 0;
  if (c->lsdF64) {
    A(c->mg, npix * NI);
    A(c->maxMg, NI);
    double k[7];
    const int h = lsdGauss64(c->cfg.lsd_scale, c->cfg.lsd_sigma_scale, k);
    if (h < 0) { g_err = "LSD pre-filter radius > 3 not supported"; return PLI_ERR_INVALID; }
    c->lsdRadius = h;
    A(c->kern64, 7);
    HIPCHK(hipMemcpy(c->kern64, k, sizeof(k), hipMemcpyHostToDevice));
    if (c->cfg.lsd_scale != 1) {
      A(c->tmp64, (size_t)P.W * P.H * NI);
      const std::vector<int> t = buildResizeTab64(P.W, P.H, P.LWt, P.LH, 1. / c->cfg.lsd_scale);
      A(c->lsdTab64, t.size());
      HIPCHK(hipMemcpy(c->lsdTab64, t.data(), t.size() * 4, hipMemcpyHostToDevice));
      c->lsdFront = frontForm(t, P.W, P.H, P.LWt, P.LH, h);
    }
  } else {
    A(c->g2, npix * NI);
  }
  c->lsdMode = c->cfg.lsd_mode;
  if (const char* e = getenv("PLI_LSD_MODE")) {
    const int m = atoi(e);
    if (m < 0 || m > 3) { g_err = "PLI_LSD_MODE must be 0, 1, 2 or 3"; return PLI_ERR_INVALID; }
    c->lsdMode = m;
  }
#ifndef PLI_DEV
  if (c->lsdMode == 1) { g_err = "lsd_mode 1 (the lane relaxation, round 1's schedule) is kept for cross-checks in the development build only (libpli_frontend_dev.so)"; return PLI_ERR_INVALID; }
#endif
  if (c->lsdMode != 2) {     // buffers of the relaxations (in auto mode only batches below RX_AUTO_IMAGES use them)
    // (auto mode: a context sized for the sequential regime keeps the relaxations' buffers — 20-30 MB per image — for 2047 images,
    // as in round 2, and batches above that take the sequential grower: 2048 frames stay at ~160 GB of HBM instead of 289)
    const size_t NR = c->lsdMode == 0 ? ((int)NI >= RX_AUTO_IMAGES ? std::min<size_t>(NI, 2047) : NI) : NI;
    c->rxImages = (int)NR;
    const bool lane = c->lsdMode == 1, tiles = c->lsdMode == 0 || c->lsdMode == 3;
    A(c->own, npix * NR);
    if (tiles && c->lsdF64) { A(c->hot, npix * NR); A(c->cold, npix * NR); }
    if (lane) {               // lane / lane-group growers of lsd_relax.hip
      A(c->smallSeeds, npix * NR);
      c->bigCap = (int)(npix / RX_HAND + 64);               // a region listed as large had >= RX_HAND pixels of its own
      A(c->bigSeeds, (size_t)c->bigCap * NR);
      c->handCap = (int)(npix / RX_HAND + 64);
      A(c->hand, (size_t)c->handCap * NR);
      A(c->rgClean, npix * NR);
    }
    c->rectCap = 2 * ((int)(npix / std::max(P.minRegSize, 1)) + 64);
    A(c->rects, (size_t)c->rectCap * NR);
    A(c->lastSize, npix * NR);                            // region tables, indexed by seed rank
    A(c->rgBox, npix * NR);
    A(c->rgSeg, npix * NR);
    A(c->rankOf, npix * NR);
    c->tilesW = (P.LW + 7) / 8; c->tilesH = (P.LH + 7) / 8;
    A(c->tileMin, (size_t)c->tilesW * c->tilesH * NR);
    A(c->tileAct, (size_t)c->tilesW * c->tilesH * NR);
    A(c->tileTouch, (size_t)c->tilesW * c->tilesH * NR);
    A(c->rgDirty, npix * NR);
    A(c->rgLost, npix * NR);
    // (round stamps above a per-call base, pli_ctx::lineStampNext: cleared here, once, and not per call)
    HIPCHK(hipMemset(c->rgDirty, 0, sizeof(int) * npix * NR));
    HIPCHK(hipMemset(c->rgLost, 0, sizeof(int) * npix * NR));
    HIPCHK(hipDeviceSynchronize());
    if (const char* e = DEVENV("PLI_TX_STAMP0")) c->lineStampNext = std::max(0, atoi(e));     // test switch: a start next to the overflow
    c->rxChunks = (int)((npix + 2047) / 2048);
    A(c->rxChunkCnt, (size_t)c->rxChunks * NR);
    // pixel lists for region2rect (<= npix per round) + queue overflow blocks; the lane growers also park hand-overs here
    // Words of arena per scaled pixel.  A round needs one word per pixel for the finished regions' lists — and, in the tile relaxation,
    // queue overflow blocks for every region of more than TX_GQ pixels that is being grown, by EVERY tile it has seeds in at the
    // same time in round 1: long parallel structures (blinds, corrugated walls; the "stripes" image of the tests) multiply that
    // by the tiles a region crosses.  3 words per pixel sent all 512 stripes images to the sequential grower (455 ms per batch
    // instead of 50); they need < 16 (8 is not enough: round 3's last commit budgeted 8 GiB, which gave the 256-frame context 8 words,
    // and the stripes batch took the fallback again, 507 ms — found by tools/rounds_sweep.py in round 4).  A context gets 16 words per
    // pixel as long as its arenas stay below 18 GiB (256 frames of 752 x 480: 17.0 GB of the 288 GB HBM); larger contexts share that
    // budget (512 frames: 8 words; a 2047-image context of the auto mode: ~10 words, 19 GB).  The budget is also clamped to a
    // quarter of what the device has FREE when the context is created (several large contexts in one process, a part with less HBM),
    // and an allocation that still fails is retried with half the words down to 3 before the context gives up.
    size_t arenaFactor = lane ? 8 : 16;
    if (!lane) {
      size_t budget = (size_t)18 << 30, freeB = 0, totalB = 0;
      if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB > 0) budget = std::min(budget, freeB / 4);
      arenaFactor = std::max<size_t>(3, std::min<size_t>(16, budget / (npix * 4 * NR)));
    }
    if (const char* e = DEVENV("PLI_RX_ARENA")) arenaFactor = (size_t)std::max(1, atoi(e));     // dev: words of arena per scaled pixel
    const size_t arenaAsked = arenaFactor;
    for (;;) {
      c->arenaCap = (int)std::min<size_t>(arenaFactor * npix + 65536, (size_t)1 << 30);
      const pli_status as = c->dalloc(&c->arena, (size_t)c->arenaCap * NR);
      if (as == PLI_OK) break;
      if (lane || arenaFactor <= 3) return as;
      (void)hipGetLastError();                              // (the failed allocation's error state)
      arenaFactor = std::max<size_t>(3, arenaFactor / 2);
    }
    c->arenaFactor = (int)arenaFactor;
    // (results stay exact below 16 words per pixel, but hostile batches — long parallel structures — then take the ~500 ms fallback: say so once)
    if (!lane && arenaFactor < 16 && arenaAsked >= arenaFactor && !DEVENV("PLI_RX_ARENA")) {
      static std::atomic<bool> warned{false};
      if (!warned.exchange(true))
        std::fprintf(stderr, "pli_frontend: the LSD relaxation's arena of this context holds %d words per scaled pixel (16 wanted: %zu images, "
                             "free device memory); results are unchanged, batches of long parallel structures may take the slow fallback "
                             "(pli_lsd_arena_words)\n", (int)arenaFactor, NR);
    }
    if (tiles) {
      // (the measure is the number of 64-pixel tile waves the context can put on the chip, not the number of images)
      c->txTs = (int64_t)NI * ((P.LW + 63) / 64) * ((P.LH + 63) / 64) <= TX_SMALL_TILE_WAVES ? 32 : 64;
      if (const char* e = DEVENV("PLI_TX_TS")) c->txTs = atoi(e) == 16 ? 16 : atoi(e) == 32 ? 32 : atoi(e) == 128 ? 128 : 64;
      c->txNtx = (P.LW + c->txTs - 1) / c->txTs; c->txNty = (P.LH + c->txTs - 1) / c->txTs;
      A(c->txList, (size_t)c->txNtx * c->txNty * c->txTs * c->txTs * NR);
      A(c->txTileCnt, (size_t)c->txNtx * c->txNty * NR);
      A(c->txDirtyList, (size_t)c->txNtx * c->txNty * c->txTs * c->txTs * NR);
      A(c->txDirtyCnt, (size_t)c->txNtx * c->txNty * NR);
      A(c->tailBar, 64);
      A(c->txCellList, (size_t)c->tilesW * c->tilesH * NR);
      A(c->txCellCnt, (size_t)2 * TX_CELL_ROUNDS * NR);
      A(c->txPerm, (size_t)c->txNtx * c->txNty * NR);
      // key mode (lsd_tile.hip, k_tx_sort): ids of (bits of nBins - 1) + pixbits bits must stay below LSD_ID_INF = 2^31 - 1: with 1024 bins
      // up to 2^21 scaled pixels (1280 x 720 scales to 1536 x 864 = 1.33 M; 3840 x 2160 to 11.9 M pixels = 24 bits: ranks).
      // PLI_TX_KEYS=0: ranks.  (debug contexts keep the ordered list for PLI_DBG_LSD_ORDER: checked at run time)
      c->txPixBits = 1;
      while (((size_t)1 << c->txPixBits) < npix) ++c->txPixBits;
      int binBits = 1;
      while ((1 << binBits) < P.nBins) ++binBits;
      // (the largest id is (nBins - 1) << pixbits | npix - 1: strictly below 2^31 - 1 unless every bit is used AND the image fills 2^pixbits)
      c->txKeys = c->lsdF64 && P.nBins <= 1024 && (binBits + c->txPixBits < 31 || (binBits + c->txPixBits == 31 && npix < ((size_t)1 << c->txPixBits))) &&
                  !(DEVENV("PLI_TX_KEYS") && atoi(DEVENV("PLI_TX_KEYS")) == 0);
      if (c->txKeys) {
        A(c->txCand, (size_t)TX_EMIT_CAP * NR);
        A(c->txCandCnt, NR);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tx_emit_sorted), hipFuncAttributeMaxDynamicSharedMemorySize, TX_EMIT_CAP * 4));
      }
    }
  }
  A(c->jrCtl, NI);
  c->jrHost.resize(NI);

  A(c->maxG2, NI);
  c->nChunks = (int)((npix + LSD_CHUNK - 1) / LSD_CHUNK);
  A(c->chunkHist, (size_t)NI * c->nChunks * P.nBins);
  A(c->chunkBase, (size_t)NI * c->nChunks * P.nBins);
  if (c->nChunks > 256 && !DEVENV("PLI_LSD_SCAN1")) {     // (dev switch: the one-block scan)
    c->scanChunksPerGroup = 64;
    c->scanGroups = (c->nChunks + c->scanChunksPerGroup - 1) / c->scanChunksPerGroup;
    A(c->scanGroupOff, (size_t)NI * c->scanGroups * P.nBins);
  }
  A(c->nDefined, NI);
  A(c->order, npix * NI);
  A(c->regScratch, npix * NI);
  c->maxSeg = (int)(npix / std::max(P.minRegSize, 1)) + 64;   // a region needs minRegSize pixels: no image can yield more segments
  A(c->seg, (size_t)NI * c->maxSeg * 4);
  A(c->rectItems, (size_t)NI * c->maxSeg);
  if (c->lsdF64) A(c->rectW, npix * NI);
  A(c->nSeg, NI);
  A(c->tmpKL, (size_t)NI * P.maxLines);
  A(c->dxy, (size_t)P.W * P.H * NI);
  {
    // BinaryDescriptor ctor weights, binary_descriptor_custom.cpp:217-259 (integer divisions kept)
    LbdCoef C;
    const int widthOfBand = 7, NUM_OF_BANDS = 9;
    double u = (widthOfBand * 3 - 1) / 2;
    double sigma = (widthOfBand * 2 + 1) / 2;
    double invsigma2 = -1 / (2 * sigma * sigma);
    for (int i = 0; i < widthOfBand * 3; i++) { double dis = i - u; C.L[i] = (float)std::exp(dis * dis * invsigma2); }
    u = (NUM_OF_BANDS * widthOfBand - 1) / 2;
    sigma = u;
    invsigma2 = -1 / (2 * sigma * sigma);
    for (int i = 0; i < NUM_OF_BANDS * widthOfBand; i++) { double dis = i - u; C.G[i] = (float)std::exp(dis * dis * invsigma2); }
    A(c->lbdCoef, 1);
    HIPCHK(hipMemcpy(c->lbdCoef, &C, sizeof(C), hipMemcpyHostToDevice));
  }
  const int NF = c->cfg.max_frames;
  A(c->sad, (size_t)NF * P.kpCap);
  A(c->bestIdx, (size_t)NF * P.kpCap);
  A(c->lmask, (size_t)NF * P.klCap * GRID_ROWS);
  A(c->ldir, (size_t)NF * P.klCap * 2);
  A(c->dmat, (size_t)NF * P.klCap * P.klCap);
  A(c->m12, (size_t)NF * P.klCap);
  A(c->m21, (size_t)NF * P.klCap);
  A(c->inStage[0], (size_t)P.W * P.H);
  A(c->inStage[1], (size_t)P.W * P.H);
  A(c->ownTable, (size_t)c->lay.record_bytes * NF);
  HIPCHK(hipMemset(c->ownTable, 0, (size_t)c->lay.record_bytes * NF));
  c->hostRec.resize((size_t)c->lay.record_bytes);
#undef A
  return PLI_OK;
}

// ---- stage scheduling -------------------------------------------------------
pli_status runIngest(pli_ctx* c, const uint8_t* dl, const uint8_t* dr, int64_t stride, int64_t frameStride, int img0, int nimg) {
  TraceRange range__("pli:ingest");
  const DevParams& P = c->hp;
  if (c->imgFormat != PLI_IMAGE_GRAY8) {       // (pli_set_image_format: stride and frameStride are bytes of the colour images)
    const bool rgb = c->imgFormat == PLI_IMAGE_RGB8 || c->imgFormat == PLI_IMAGE_RGBA8;
    const int c0 = rgb ? 4899 : 1868, c2 = rgb ? 1868 : 4899;       // the coefficients of bytes 0 and 2: R2Y and B2Y, or swapped
    dim3 g((P.W + 1023) / 1024, P.H, nimg);
    if (c->imgChannels == 3)
      LAUNCH(c, "k_ingest", k_ingest_colour<3>, g, dim3(256), 0, dl, dr, stride, frameStride, c->pyr, P.pyrBlock, P.W, P.H, P.lv[0].pitch,
             (const float2*)c->rectMap[0], (const float2*)c->rectMap[1], img0, c0, c2);
    else
      LAUNCH(c, "k_ingest", k_ingest_colour<4>, g, dim3(256), 0, dl, dr, stride, frameStride, c->pyr, P.pyrBlock, P.W, P.H, P.lv[0].pitch,
             (const float2*)c->rectMap[0], (const float2*)c->rectMap[1], img0, c0, c2);
    return PLI_OK;
  }
  const bool aligned16 = !c->rectMap[0] && !c->rectMap[1] && (P.W % 16) == 0 && (stride % 16) == 0 && (frameStride % 16) == 0 &&
                         (reinterpret_cast<uintptr_t>(dl) % 16) == 0 && (reinterpret_cast<uintptr_t>(dr) % 16) == 0 && (P.lv[0].pitch % 16) == 0 &&
                         (P.pyrBlock % 16) == 0;
  if (aligned16) {
    const int n16 = (P.W / 16) * P.H;
    LAUNCH(c, "k_ingest", k_ingest_copy16, dim3(std::max(1, std::min((n16 + 255) / 256, 64)), nimg), dim3(256), 0, dl, dr, stride, frameStride,
           c->pyr, P.pyrBlock, P.W / 16, P.H, P.lv[0].pitch, img0);
    return PLI_OK;
  }
  dim3 g((P.W + 1023) / 1024, P.H, nimg);
  LAUNCH(c, "k_ingest", k_ingest, g, dim3(256), 0, dl, dr, stride, frameStride, c->pyr, P.pyrBlock, P.W, P.H, P.lv[0].pitch,
         (const float2*)c->rectMap[0], (const float2*)c->rectMap[1], img0);
  return PLI_OK;
}

pli_status runOrb(pli_ctx* c, int img0, int nimg, uint8_t* table) {
  TraceRange range__("pli:orb chain");
  const DevParams& P = c->hp;
  const pli_table_layout& Y = c->lay;
  for (int l = 1; l < P.nlevels; ++l) {
    const LevelGeom &S = P.lv[l - 1], &D = P.lv[l];
    dim3 g((D.w + 255) / 256, (D.h + 15) / 16, nimg);
    LAUNCH(c, "k_resize_level", k_resize_level, g, dim3(256), 0, c->pyr + S.offset, P.pyrBlock, S.w, S.h, S.pitch,
           c->pyr + D.offset, P.pyrBlock, D.w, D.h, D.pitch, c->resizeTab[l], img0);
  }
  if (P.cellsPerImage > 0)
    LAUNCH(c, "k_fast_cells", k_fast_cells, dim3(P.cellsPerImage, nimg), dim3(256), 0, c->dP, c->pyr, c->cellCand, c->cellCount, img0);
  {
    // node capacity of the octree instance: the list ends at quota..quota+3 nodes (first pass: 4 per root)
    int need = 0;
    for (int l = 0; l < P.nlevels; ++l) need = std::max(need, std::max(P.lv[l].nfeatures + 8, 4 * P.lv[l].nIni + 8));
    // workgroups of 1024 threads while the (level, image) workgroups do not fill the chip (4K: 32 images x 8 levels; a single pair:
    // 16 workgroups): the passes over a level's keys are the long pole, 4x the threads on them
    const bool wide = P.nlevels * nimg <= 1024;
    const dim3 og(P.nlevels, nimg), ob(wide ? 1024 : 256);
#define OCTREE_LAUNCH(K) LAUNCH(c, "k_octree", K, og, ob, 0, c->dP, c->cellCand, c->cellCount, c->candAll, c->nodeOf, c->candCount, c->kpSel, c->kpSelCount, img0)
    if (need <= 320) { if (wide) OCTREE_LAUNCH(k_octree_320_w); else OCTREE_LAUNCH(k_octree_320); }
    else if (need <= 512) { if (wide) OCTREE_LAUNCH(k_octree_512_w); else OCTREE_LAUNCH(k_octree_512); }
    else { if (wide) OCTREE_LAUNCH(k_octree_w); else OCTREE_LAUNCH(k_octree); }
#undef OCTREE_LAUNCH
  }
  // the blurred pyramid is a debug item only (PLI_DBG_BLUR_LEVEL): k_describe blurs the window of each keypoint itself
  if (c->debug && c->blur)
    LAUNCH(c, "k_blur_orb", k_blur, dim3(c->orbTiles, nimg), dim3(256), 0, c->jobOrb, c->pyr, P.pyrBlock, c->blur, P.pyrBlock, img0);
  LAUNCH(c, "k_kp_counts", k_kp_counts, dim3((nimg + 63) / 64), dim3(64), 0, c->dP, c->kpSelCount, table, Y.record_bytes,
         Y.off_counts, nimg, img0);
  LAUNCH(c, "k_describe", k_describe, dim3(P.kpSlotsPerImage, nimg), dim3(64), 0, c->dP, c->pyr, c->jobOrb, c->kpSel,
         c->kpSelCount, table, Y.record_bytes, Y.off_counts, Y.off_kp[0], Y.off_kp[1], Y.off_desc[0], Y.off_desc[1], img0);
  return PLI_OK;
}

pli_status runStereoPoints(pli_ctx* c, int nframes, uint8_t* table) {
  TraceRange range__("pli:stereo points");
  const DevParams& P = c->hp;
  const pli_table_layout& Y = c->lay;
  LAUNCH(c, "k_stereo_points", k_stereo_points, dim3(P.kpCap, nframes), dim3(64), 0, c->dP, c->pyr, table, Y.record_bytes,
         Y.off_counts, Y.off_kp[0], Y.off_kp[1], Y.off_desc[0], Y.off_desc[1], Y.off_uright, Y.off_depth, c->sad,
         c->debug ? c->bestIdx : (int*)nullptr);
  LAUNCH(c, "k_stereo_median", k_stereo_median, dim3(nframes), dim3(256), (size_t)P.kpCap * 4, c->dP, table, Y.record_bytes,
         Y.off_counts, Y.off_uright, Y.off_depth, c->sad);
  return PLI_OK;
}

pli_status runStereoLines(pli_ctx* c, int nframes, uint8_t* table) {
  TraceRange range__("pli:stereo lines");
  const pli_table_layout& Y = c->lay;
  // (many lines per frame: the pair distances by several workgroups per frame, see the kernel)
  const int cap = c->hp.klCap;
  const int slices = cap >= 192 ? std::max(1, std::min(64, (cap * cap) / 8192)) : 1;
  for (int phase = slices > 1 ? 1 : 0; phase <= (slices > 1 ? 3 : 0); ++phase)
    LAUNCH(c, "k_stereo_lines", k_stereo_lines, dim3(nframes, phase == 2 ? slices : 1), dim3(256), 0, c->dP, table, Y.record_bytes,
           Y.off_counts, Y.off_kl[0], Y.off_kl[1], Y.off_ldesc[0], Y.off_ldesc[1], Y.off_disp, Y.off_le, c->lmask, c->ldir, c->dmat,
           c->m12, c->m21, phase);
  return PLI_OK;
}

// The ORB chain runs beside the line chain (fork after the ingest, join before whatever reads both chains' tables) except under the
// sequential grower above 2560 images.  Measured, 752x480, frames/s without -> with: tile relaxation 32 frames 2688 -> 2847,
// 128 frames 3711 -> 3947, 256 frames 4054 -> 4245, 512 frames 4268 -> 4379, 768 frames 4303 -> 4420; sequential grower
// 1024 frames 4213 -> 4544, 1280 frames 4830 -> 5266; from 1536 frames on the grower's blocks fill the CUs' LDS, the ORB
// kernels wait for it and stretch the grower: 5170 -> 4287, 2048 frames 6067 -> 4942.
bool chainsRunBeside(const pli_ctx* c, int nimg) {
  static const int sideMax = DEVENV("PLI_SIDE_MAX") ? atoi(DEVENV("PLI_SIDE_MAX")) : INT_MAX;    // (dev: images below which the tile relaxation has the ORB chain beside it)
  return (sequentialGrower(c, nimg) ? nimg <= 2560 : nimg < sideMax) && !c->syncDebug;
}

// Both chains of images img0 .. img0 + nimg - 1 (ingested already) into `table`, the ORB chain on the side stream, and the join: on
// return the context's stream has waited for the side stream.  pointFrames > 0: the stereo point matcher of that many frames behind
// the ORB chain.  One function for pli_batch_run and pli_frame_extract_single; the caller has asked chainsRunBeside.
pli_status runChainsBeside(pli_ctx* c, int img0, int nimg, uint8_t* T, int pointFrames) {
  pli_status st;
  const bool seqGrower = sequentialGrower(c, nimg);
  if (!c->aux) {
    // (the line chain is the longer one: the ORB chain beside it takes what the line kernels leave free)
    int prLow = 0, prHigh = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prLow, &prHigh));
    HIPCHK(hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, prLow));
    HIPCHK(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evLbdPre, hipEventDisableTiming));
  }
  hipStream_t main = c->stream;
  c->lbdPreOnSide = c->lsdF64;
  // the side chain: forks from the line chain where it is enqueued.  Under the tile relaxation that is right after the
  // launch of round 1 (relaxTile, line_chain.hip, calls it): round 1 keeps the chip to itself, and the later rounds, which leave most of it
  // idle, host the ORB kernels; otherwise before the line chain starts.
  auto sideChain = [c, img0, nimg, pointFrames, T, main]() -> pli_status {
    HIPCHK(hipEventRecord(c->evFork, main));
    HIPCHK(hipStreamWaitEvent(c->aux, c->evFork, 0));
    {
      StreamScope onSide(c, c->aux);
      pli_status s2 = runOrb(c, img0, nimg, T);
      if (s2 != PLI_OK) return s2;
      // (the stereo point matcher needs the ORB tables only: it stays on the side stream, off the line chain's path)
      if (pointFrames > 0 && (s2 = runStereoPoints(c, pointFrames, T)) != PLI_OK) return s2;
      if (c->lbdPreOnSide) {
        if ((s2 = runLbdPre(c, img0, nimg)) != PLI_OK) return s2;
        HIPCHK(hipEventRecord(c->evLbdPre, c->aux));
      }
    }
    HIPCHK(hipEventRecord(c->evJoin, c->aux));
    return PLI_OK;
  };
  // (measured: +1.3 % at 32 frames, +1.4 % on the 4K configuration (16 frames), +1 % on a single pair; neutral at 64 and 128
  // frames, -0.5 % at 256, -3 % on the 720p configuration with its 2000 keypoints: up to 64 images it is)
  // Round 5, with round 1 a tenth shorter when it has the chip to itself: 256 frames of 752 x 480 +1.9 % (47.4 -> 46.6 ms), 128 frames +2 %,
  // 512 frames +0.3 %, 1024 frames -0.4 %; 64 frames of 1280 x 720 (2000 keypoints: a longer ORB chain) still -1.3 %.  So: up to 64
  // images always, up to 1024 images of EuRoC-sized frames (< 0.5 M pixels).  Behind a LATER round (PLI_SIDE_FORK_ROUND = 3 / 4 / 5 / 7)
  // it is 47.4 / 47.5 / 47.9 / 48.4 ms on the synthetic stream; which round it forks behind: relaxTile (sideForkRound).
  const int sideDeferMax = DEVENV("PLI_SIDE_DEFER_MAX") ? atoi(DEVENV("PLI_SIDE_DEFER_MAX")) : -1;   // (dev: images up to which the ORB chain starts behind round 1)
  const bool deferSide = sideDeferMax >= 0 ? nimg <= sideDeferMax : (nimg <= 64 || (nimg <= 1024 && (int64_t)c->hp.W * c->hp.H < 500000));
  if (!seqGrower && c->lsdMode != 1 && deferSide) c->sideChain = sideChain;
  else if ((st = sideChain()) != PLI_OK) { c->lbdPreOnSide = false; return st; }
  st = runLines(c, img0, nimg, T);
  if (st == PLI_OK && c->sideChain) { auto f = std::move(c->sideChain); c->sideChain = nullptr; st = f(); }   // (not taken by runLines)
  c->sideChain = nullptr;
  c->lbdPreOnSide = false;
  if (st != PLI_OK) return st;
  HIPCHK(hipStreamWaitEvent(main, c->evJoin, 0));
  return PLI_OK;
}

// The counts block of a record (include/pli_frontend.h: pli_table_layout.off_counts), as the kernels write it.
struct RecordCounts {
  int32_t kp[2], kl[2];                   // keypoints / keylines of eye 0, 1
  int32_t stereoPoints, stereoLines;
  uint8_t linesCut[2], kpCut[2];          // truncation flags per eye: segments beyond max_lines, keypoints beyond kp_cap
  int32_t reserved;
};
static_assert(sizeof(RecordCounts) == 32 && offsetof(RecordCounts, linesCut) == 24, "the int32[8] at off_counts");

// ... of the context's own record, once the stream has finished
pli_status readCounts(pli_ctx* c, RecordCounts& rc) {
  HIPCHK(hipMemcpyAsync(&rc, c->ownTable + c->lay.off_counts, sizeof(rc), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

// n rows (of `per` elements) of a column of the context's own record to the host; nothing for a null pointer or n <= 0
template <typename T>
hipError_t copyColumn(pli_ctx* c, T* dst, int64_t off, int n, int per = 1) {
  return dst && n > 0 ? hipMemcpy(dst, c->ownTable + off, (size_t)n * per * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// bytes of one image row as the entry points read it: the context's width times the bytes per pixel of pli_set_image_format
inline int64_t rowBytes(const pli_ctx* c) { return (int64_t)c->cfg.width * c->imgChannels; }
// bytes of one element of a depth image (pli_set_depth_format)
inline size_t depthElemBytes(const pli_ctx* c) { return c->depthFmt.u16 ? sizeof(uint16_t) : sizeof(float); }

pli_status checkImage(pli_ctx* c, const uint8_t* img, int w, int h, int64_t stride) {
  if (!img || w <= 0 || h <= 0) { g_err = "empty image"; return PLI_ERR_EMPTY_IMAGE; }
  if (w != c->cfg.width || h != c->cfg.height) { g_err = "image size differs from the context's"; return PLI_ERR_INVALID; }
  if (stride < rowBytes(c)) { g_err = "stride < width x bytes per pixel"; return PLI_ERR_INVALID; }
  return PLI_OK;
}

pli_status stageImage(pli_ctx* c, int eye, const uint8_t* img, int w, int h, int64_t stride) {
  const size_t row = (size_t)rowBytes(c);
  HIPCHK(hipMemcpy2DAsync(c->inStage[eye], row, img, stride, row, h, hipMemcpyHostToDevice, c->stream));
  return runIngest(c, c->inStage[0], c->inStage[1], (int64_t)row, 0, eye, 1);
}

}  // namespace

extern "C" {

const char* pli_version(void) { return "pli-frontend-mi355x 0.1 (gfx950)"; }
const char* pli_last_error(void) { return g_err.c_str(); }

void pli_config_default(pli_frontend_config* c, int32_t width, int32_t height) {
  std::memset(c, 0, sizeof(*c));
  c->width = width; c->height = height; c->max_frames = 1;
  c->orb_nfeatures = 1200; c->orb_scale_factor = 1.2f; c->orb_nlevels = 8;
  c->orb_ini_th_fast = 20; c->orb_min_th_fast = 7;
  c->lsd_nfeatures = 500; c->lsd_refine = 0; c->lsd_n_bins = 1024;
  c->max_lines = std::max(4096, width * height / 64);   // the reference keeps every segment above the length cut
  c->min_line_length = 0.025; c->lsd_scale = 1.2; c->lsd_sigma_scale = 0.6; c->lsd_quant = 2.0;
  c->lsd_ang_th = 22.5; c->lsd_log_eps = 1.0; c->lsd_density_th = 0.6;
  c->bf = 47.90639384423901f; c->fx = 435.2046959714599f; c->stereo_maxd_inf = 0;
  c->matching_s_ws = 10; c->best_lr_matches = 1;
  c->line_sim_th = 0.75; c->stereo_overlap_th = 0.75; c->min_ratio_12_l = 0.9;
  c->ls_min_disp_ratio = 0.7; c->min_disp = 1.0; c->line_horiz_th = 0.1;
  c->lsd_mode = 0;
  c->parity_flags = PLI_PARITY_TRIG_F32_ORB | PLI_PARITY_LSD_F64;
}

int32_t pli_kp_capacity(const pli_frontend_config* c) {
  // DistributeOctTree returns up to quota+3 keypoints per level (ORBextractor.cc:713-733) — or, when the quota is tiny,
  // the 4 children of each of its nIni = round(width/height) root nodes (:540-589, first expansion)
  int64_t extra = 0;
  float sc = 1.0f;
  for (int l = 0; l < c->orb_nlevels; ++l) {
    const float inv = 1.0f / sc;
    const int w = cvRoundf((float)c->width * inv), h = cvRoundf((float)c->height * inv);
    const int bw = w - 32, bh = h - 32;                     // maxBorder - minBorder, EDGE_THRESHOLD - 3 = 16 each side
    const int nIni = (bw > 0 && bh > 0) ? (int)std::round((float)bw / (float)bh) : 0;
    extra += std::max(4, 4 * nIni);
    sc *= c->orb_scale_factor;
  }
  return (int32_t)alignUp((int64_t)c->orb_nfeatures + extra + 8, 64);
}
int32_t pli_kl_capacity(const pli_frontend_config* c) { return c->lsd_nfeatures != 0 ? c->lsd_nfeatures : c->max_lines; }
int32_t pli_lsd_segment_box_cut(const pli_frontend_config* c) {
  return lsd_seg_box_cut(c->lsd_scale, c->min_line_length * std::min(c->width, c->height), c->width, c->height);
}

pli_status pli_ctx_create(const pli_frontend_config* cfg, int32_t device, pli_ctx** out) {
  if (!cfg || !out) { g_err = "null argument"; return PLI_ERR_INVALID; }
  *out = nullptr;
  pli_status st = validate(*cfg);
  if (st != PLI_OK) return st;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    g_err = "no HIP device: this library has no CPU path";
    return PLI_ERR_NO_DEVICE;
  }
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
    g_err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return PLI_ERR_NO_DEVICE;
  }
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<pli_ctx> c(new pli_ctx());
  c->cfg = *cfg;
  c->device = device;
  c->NI = 2 * cfg->max_frames;
  c->pinhole.maxX = (float)cfg->width; c->pinhole.maxY = (float)cfg->height;     // no camera yet: the grid spans the image (pli_set_pinhole_distortion)
  st = buildGeometry(c.get());
  if (st != PLI_OK) return st;
  buildLayout(c.get());
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  st = allocAll(c.get());
  if (st != PLI_OK) { pli_ctx_destroy(c.release()); return st; }
  *out = c.release();
  return PLI_OK;
}

void pli_ctx_destroy(pli_ctx* c) {
  if (!c) return;
  { CtxGuard wait__(c); }       // a call still running on another thread finishes first (destroying under it is the caller's bug)
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (void* p : c->allocs) hipFree(p);
  if (c->scratch) hipFree(c->scratch);
  for (hipEvent_t e : c->evPool) hipEventDestroy(e);
  if (c->ownStream && c->stream) hipStreamDestroy(c->stream);
  if (c->aux2) { hipStreamSynchronize(c->aux2); hipStreamDestroy(c->aux2); }
  if (c->evRectFork) { hipEventDestroy(c->evRectFork); hipEventDestroy(c->evRectDone); }
  if (c->aux) { hipStreamSynchronize(c->aux); hipStreamDestroy(c->aux); hipEventDestroy(c->evFork); hipEventDestroy(c->evJoin); hipEventDestroy(c->evLbdPre); }
  for (int e = 0; e < 2; ++e) if (c->rectMap[e]) hipFree(c->rectMap[e]);
  for (int s = 0; s < 2; ++s) {
    if (c->hs[s].busy) hipEventSynchronize(c->hs[s].d2h);
    if (c->hs[s].dimg) hipFree(c->hs[s].dimg);
    if (c->hs[s].dtab) hipFree(c->hs[s].dtab);
    if (c->hs[s].h2d) { hipEventDestroy(c->hs[s].h2d); hipEventDestroy(c->hs[s].kern); hipEventDestroy(c->hs[s].d2h); }
  }
  if (c->sH2D) { hipStreamDestroy(c->sH2D); hipStreamDestroy(c->sD2H); }
  if (c->rxSeen) { hipHostFree(c->rxSeen); hipEventDestroy(c->evRxSeen); }
  for (int e = 0; e < 2; ++e) if (c->pyrHost[e]) hipHostFree(c->pyrHost[e]);
  if (c->recPinned) hipHostFree(c->recPinned);
  delete c;
}

pli_status pli_ctx_layout(const pli_ctx* c, pli_table_layout* out) {
  CtxGuard guard__(c);
  if (!c || !out) return PLI_ERR_INVALID;
  *out = c->lay;
  return PLI_OK;
}

pli_status pli_ctx_set_stream(pli_ctx* c, void* s) {
  CtxGuard guard__(c);
  if (!c) return PLI_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (s) {
    if (c->ownStream) hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)s;
    c->ownStream = false;
  } else if (!c->ownStream) {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->ownStream = true;
  }
  return PLI_OK;
}

pli_status pli_set_rectify_maps(pli_ctx* c, int32_t eye, const float* mapx, const float* mapy) {
  CtxGuard guard__(c);
  if (!c || eye < 0 || eye > 1 || ((mapx == nullptr) != (mapy == nullptr))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!mapx) {
    if (c->rectMap[eye]) { hipFree(c->rectMap[eye]); c->rectMap[eye] = nullptr; }
    return PLI_OK;
  }
  const size_t n = (size_t)c->cfg.width * c->cfg.height;
  if (!c->rectMap[eye]) HIPCHK(hipMalloc(&c->rectMap[eye], n * sizeof(float2)));
  std::vector<float2> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = make_float2(mapx[i], mapy[i]);
  HIPCHK(hipMemcpy(c->rectMap[eye], h.data(), n * sizeof(float2), hipMemcpyHostToDevice));
  return PLI_OK;
}

pli_status pli_set_image_format(pli_ctx* c, pli_image_format fmt) {
  CtxGuard guard__(c);
  if (!c) { g_err = "null argument"; return PLI_ERR_INVALID; }
  int ch = 0;
  switch ((int)fmt) {
    case PLI_IMAGE_GRAY8: ch = 1; break;
    case PLI_IMAGE_RGB8: case PLI_IMAGE_BGR8: ch = 3; break;
    case PLI_IMAGE_RGBA8: case PLI_IMAGE_BGRA8: ch = 4; break;
    default: g_err = "unknown image format"; return PLI_ERR_INVALID;
  }
  if (c->hsWaited < c->hsSubmitted) { g_err = "a submitted batch is in flight: pli_batch_wait first"; return PLI_ERR_INVALID; }
  if ((int)fmt == c->imgFormat) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));           // kernels and copies in flight read the staging of the old format
  if (ch != c->imgChannels) {
    // the per-call staging: W * H pixels per eye; the slots of pli_batch_submit_host are sized again by the next submit
    // (both new buffers first: a failed allocation leaves the context as it was)
    uint8_t* fresh[2] = {nullptr, nullptr};
    for (int e = 0; e < 2; ++e)
      if (hipMalloc((void**)&fresh[e], (size_t)c->cfg.width * c->cfg.height * ch) != hipSuccess) {
        if (fresh[0]) hipFree(fresh[0]);
        g_err = "out of device memory for the image staging";
        return PLI_ERR_HIP;
      }
    for (int e = 0; e < 2; ++e) {
      std::replace(c->allocs.begin(), c->allocs.end(), (void*)c->inStage[e], (void*)fresh[e]);
      hipFree(c->inStage[e]);
      c->inStage[e] = fresh[e];
    }
    for (int s = 0; s < 2; ++s) {
      if (c->hs[s].dimg) hipFree(c->hs[s].dimg);
      c->hs[s].dimg = nullptr; c->hs[s].imgBytes = 0;
    }
  }
  c->imgFormat = (int)fmt;
  c->imgChannels = ch;
  return PLI_OK;
}

pli_status pli_set_depth_format(pli_ctx* c, pli_depth_type type, float scale) {
  CtxGuard guard__(c);
  if (!c) { g_err = "null argument"; return PLI_ERR_INVALID; }
  if ((int)type != PLI_DEPTH_F32 && (int)type != PLI_DEPTH_U16) { g_err = "unknown depth type"; return PLI_ERR_INVALID; }
  if (!std::isfinite(scale)) { g_err = "the depth scale is not finite"; return PLI_ERR_INVALID; }
  c->depthFmt = DepthFormat{(int)type == PLI_DEPTH_U16 ? 1 : 0, scale};      // (passed by value with each launch: nothing in flight reads it)
  return PLI_OK;
}

pli_status pli_ctx_sync(pli_ctx* c) {
  CtxGuard guard__(c);
  if (!c) return PLI_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_batch_run(pli_ctx* c, int32_t nframes, const uint8_t* dl, const uint8_t* dr, int64_t stride,
                         int64_t frameStride, uint32_t stages, void* table) {
  CtxGuard guard__(c);
  TraceRange range__("pli_batch_run");
  if (!c || !dl || !dr || !table) { g_err = "null argument"; return PLI_ERR_INVALID; }
  if (nframes < 1 || nframes > c->cfg.max_frames) { g_err = "nframes exceeds the context's max_frames"; return PLI_ERR_INVALID; }
  if (stride < rowBytes(c)) { g_err = "stride < width x bytes per pixel"; return PLI_ERR_INVALID; }
  if (((uintptr_t)table & 15) != 0) { g_err = "the table must be 16-byte aligned"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  uint8_t* T = (uint8_t*)table;
  pli_status st;
  const int nimg = 2 * nframes;
  // a batch overwrites the pyramids and tables of images 0/1: whatever the per-call entry points cached about the last Frame
  // on this context is gone (pli_frame_extract, which calls this, sets its own state afterwards)
  c->frameFresh = c->pointsFresh = false;
  for (int e = 0; e < 2; ++e) { c->orbDone[e] = c->lineDone[e] = false; c->pyrHostValid[e] = false; }
  if ((st = runIngest(c, dl, dr, stride, frameStride, 0, nimg)) != PLI_OK) return st;
  bool stereoPointsDone = false;
  if ((stages & PLI_RUN_ORB) && (stages & PLI_RUN_LINES) && chainsRunBeside(c, nimg)) {
    stereoPointsDone = (stages & PLI_RUN_STEREO_POINTS) != 0;
    if ((st = runChainsBeside(c, 0, nimg, T, stereoPointsDone ? nframes : 0)) != PLI_OK) return st;
  } else {
    if (stages & PLI_RUN_ORB) if ((st = runOrb(c, 0, nimg, T)) != PLI_OK) return st;
    if (stages & PLI_RUN_LINES) if ((st = runLines(c, 0, nimg, T)) != PLI_OK) return st;
  }
  if (stages & PLI_RUN_STEREO_LINES) if ((st = runStereoLines(c, nframes, T)) != PLI_OK) return st;
  if ((stages & PLI_RUN_STEREO_POINTS) && !stereoPointsDone) if ((st = runStereoPoints(c, nframes, T)) != PLI_OK) return st;
  return PLI_OK;
}

pli_status pli_batch_run_host(pli_ctx* c, int32_t nframes, const uint8_t* left, const uint8_t* right, int64_t stride,
                              int64_t frameStride, uint32_t stages, void* table) {
  CtxGuard guard__(c);
  TraceRange range__("pli_batch_run_host");
  if (!c || !left || !right || !table) { g_err = "null argument"; return PLI_ERR_INVALID; }
  if (nframes < 1 || nframes > c->cfg.max_frames) { g_err = "nframes exceeds the context's max_frames"; return PLI_ERR_INVALID; }
  if (stride < rowBytes(c)) { g_err = "stride < width x bytes per pixel"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const int W = (int)rowBytes(c), H = c->cfg.height;      // (W: bytes of a staged row)
  const size_t imgBytes = (size_t)W * H;
  ScratchPlan plan;
  auto dl = plan.add<uint8_t>(2 * imgBytes * nframes);                  // the left images, then the right ones
  auto dt = plan.add<uint8_t>((size_t)c->lay.record_bytes * nframes);   // (a block of its own: the table needs its natural alignment)
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  uint8_t* dr = dl + imgBytes * nframes;
  for (int f = 0; f < nframes; ++f) {
    HIPCHK(hipMemcpy2DAsync(dl + imgBytes * f, W, left + (int64_t)f * frameStride, stride, W, H, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpy2DAsync(dr + imgBytes * f, W, right + (int64_t)f * frameStride, stride, W, H, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemsetAsync(dt, 0, (size_t)c->lay.record_bytes * nframes, c->stream));
  st = pli_batch_run(c, nframes, dl, dr, W, (int64_t)imgBytes, stages, dt);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemcpyAsync(table, dt, (size_t)c->lay.record_bytes * nframes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_frame_extract(pli_ctx* c, const uint8_t* left, const uint8_t* right, int32_t w, int32_t h, int64_t strideLeft,
                             int64_t strideRight, void* record) {
  CtxGuard guard__(c);
  TraceRange range__("pli_frame_extract");
  if (!c || !record) { g_err = "null argument"; return PLI_ERR_INVALID; }
  pli_status st = checkImage(c, left, w, h, strideLeft);
  if (st != PLI_OK) return st;
  if ((st = checkImage(c, right, w, h, strideRight)) != PLI_OK) return st;
  HIPCHK(hipSetDevice(c->device));
  const int W = (int)rowBytes(c), H = c->cfg.height;      // (W: bytes of a staged row)
  HIPCHK(hipMemcpy2DAsync(c->inStage[0], W, left, strideLeft, W, H, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpy2DAsync(c->inStage[1], W, right, strideRight, W, H, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->ownTable, 0, (size_t)c->lay.record_bytes, c->stream));
  c->frameFresh = false;
  if ((st = pli_batch_run(c, 1, c->inStage[0], c->inStage[1], W, 0, PLI_RUN_ALL, c->ownTable)) != PLI_OK) return st;
  if (!c->recPinned) HIPCHK(hipHostMalloc((void**)&c->recPinned, (size_t)c->lay.record_bytes, hipHostMallocDefault));
  HIPCHK(hipMemcpyAsync(c->recPinned, c->ownTable, (size_t)c->lay.record_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(c->hostRec.data(), c->recPinned, (size_t)c->lay.record_bytes);
  std::memcpy(record, c->recPinned, (size_t)c->lay.record_bytes);
  RecordCounts rc;
  std::memcpy(&rc, c->hostRec.data() + c->lay.off_counts, sizeof(rc));
  for (int e = 0; e < 2; ++e) {
    c->orbDone[e] = c->lineDone[e] = true;
    c->orbCount[e] = c->monoCount[e] = rc.kp[e];
    c->lineCount[e] = rc.kl[e];
    c->pyrHostValid[e] = false;
  }
  if (rc.linesCut[0] || rc.linesCut[1]) { g_err = "more segments pass the length cut than max_lines holds: raise pli_frontend_config.max_lines"; return PLI_ERR_CAPACITY; }
  if (rc.kpCut[0] || rc.kpCut[1]) { g_err = "more keypoints than kp_cap holds"; return PLI_ERR_CAPACITY; }
  c->frameFresh = true;
  c->pointsFresh = true;
  return PLI_OK;
}

pli_status pli_host_alloc(size_t bytes, void** out) {
  if (!out) { g_err = "null argument"; return PLI_ERR_INVALID; }
  *out = nullptr;
  HIPCHK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return PLI_OK;
}
void pli_host_free(void* p) { if (p) (void)hipHostFree(p); }

static pli_status waitSlot(pli_ctx* c, int s) {
  pli_ctx::HostSlot& S = c->hs[s];
  if (S.busy) { HIPCHK(hipEventSynchronize(S.d2h)); S.busy = false; ++c->hsWaited; }
  return PLI_OK;
}

pli_status pli_batch_wait(pli_ctx* c, int32_t all) {
  CtxGuard guard__(c);
  if (!c) return PLI_ERR_INVALID;
  HIPCHK(hipSetDevice(c->device));
  pli_status st;
  while (c->hsWaited < c->hsSubmitted) {
    if ((st = waitSlot(c, (int)(c->hsWaited & 1))) != PLI_OK) return st;
    if (!all) break;
  }
  return PLI_OK;
}

pli_status pli_batch_submit_host(pli_ctx* c, int32_t nframes, const uint8_t* left, const uint8_t* right, int64_t stride,
                                 int64_t frameStride, uint32_t stages, void* table) {
  CtxGuard guard__(c);
  TraceRange range__("pli_batch_submit_host");
  if (!c || !left || !right || !table) { g_err = "null argument"; return PLI_ERR_INVALID; }
  if (nframes < 1 || nframes > c->cfg.max_frames) { g_err = "nframes exceeds the context's max_frames"; return PLI_ERR_INVALID; }
  if (stride < rowBytes(c)) { g_err = "stride < width x bytes per pixel"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const int W = (int)rowBytes(c), H = c->cfg.height;      // (W: bytes of a staged row)
  const size_t imgBytes = (size_t)W * H, tabBytes = (size_t)c->lay.record_bytes * nframes;
  if (!c->sH2D) {
    HIPCHK(hipStreamCreateWithFlags(&c->sH2D, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->sD2H, hipStreamNonBlocking));
  }
  const int s = (int)(c->hsSubmitted & 1);
  pli_ctx::HostSlot& S = c->hs[s];
  pli_status st = waitSlot(c, s);                     // the slot's previous batch (two submits ago) must have left
  if (st != PLI_OK) return st;
  if (!S.h2d) {
    HIPCHK(hipEventCreateWithFlags(&S.h2d, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&S.kern, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&S.d2h, hipEventDisableTiming));
  }
  const size_t needImg = alignUp(2 * imgBytes * (size_t)c->cfg.max_frames, 256), needTab = (size_t)c->lay.record_bytes * c->cfg.max_frames;
  if (S.imgBytes < needImg) { if (S.dimg) hipFree(S.dimg); S.dimg = nullptr; HIPCHK(hipMalloc(&S.dimg, needImg)); S.imgBytes = needImg; }
  if (S.tabBytes < needTab) { if (S.dtab) hipFree(S.dtab); S.dtab = nullptr; HIPCHK(hipMalloc(&S.dtab, needTab)); S.tabBytes = needTab; }
  uint8_t* dl = S.dimg;
  uint8_t* dr = S.dimg + imgBytes * nframes;
  if (stride == W && frameStride == (int64_t)imgBytes) {
    HIPCHK(hipMemcpyAsync(dl, left, imgBytes * nframes, hipMemcpyHostToDevice, c->sH2D));
    HIPCHK(hipMemcpyAsync(dr, right, imgBytes * nframes, hipMemcpyHostToDevice, c->sH2D));
  } else {
    for (int f = 0; f < nframes; ++f) {
      HIPCHK(hipMemcpy2DAsync(dl + imgBytes * f, W, left + (int64_t)f * frameStride, stride, W, H, hipMemcpyHostToDevice, c->sH2D));
      HIPCHK(hipMemcpy2DAsync(dr + imgBytes * f, W, right + (int64_t)f * frameStride, stride, W, H, hipMemcpyHostToDevice, c->sH2D));
    }
  }
  HIPCHK(hipEventRecord(S.h2d, c->sH2D));
  HIPCHK(hipStreamWaitEvent(c->stream, S.h2d, 0));
  HIPCHK(hipMemsetAsync(S.dtab, 0, tabBytes, c->stream));
  st = pli_batch_run(c, nframes, dl, dr, W, (int64_t)imgBytes, stages, S.dtab);
  if (st != PLI_OK) return st;
  HIPCHK(hipEventRecord(S.kern, c->stream));
  HIPCHK(hipStreamWaitEvent(c->sD2H, S.kern, 0));
  HIPCHK(hipMemcpyAsync(table, S.dtab, tabBytes, hipMemcpyDeviceToHost, c->sD2H));
  HIPCHK(hipEventRecord(S.d2h, c->sD2H));
  S.busy = true;
  ++c->hsSubmitted;
  return PLI_OK;
}

pli_status pli_orb_extract(pli_ctx* c, int32_t eye, const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                           pli_keypoint* kp, int32_t cap, uint8_t* desc, int32_t* n) {
  CtxGuard guard__(c);
  TraceRange range__("pli_orb_extract");
  if (!c || eye < 0 || eye > 1 || !n) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  *n = 0;
  pli_status st = checkImage(c, img, w, h, stride);
  if (st != PLI_OK) return st;
  HIPCHK(hipSetDevice(c->device));
  if ((st = stageImage(c, eye, img, w, h, stride)) != PLI_OK) return st;
  if ((st = runOrb(c, eye, 1, c->ownTable)) != PLI_OK) return st;
  const pli_table_layout& Y = c->lay;
  RecordCounts rc;
  if ((st = readCounts(c, rc)) != PLI_OK) return st;
  const int N = rc.kp[eye];
  c->orbDone[eye] = true;
  c->frameFresh = false;
  c->pyrHostValid[eye] = false;
  c->orbCount[eye] = N;
  c->monoCount[eye] = N;
  *n = N;
  if (rc.kpCut[eye]) { g_err = "more keypoints than kp_cap holds"; return PLI_ERR_CAPACITY; }
  if (N > cap) { g_err = "keypoint buffer too small"; return PLI_ERR_CAPACITY; }
  HIPCHK(copyColumn(c, kp, Y.off_kp[eye], N));
  HIPCHK(copyColumn(c, desc, Y.off_desc[eye], N, 32));
  return PLI_OK;
}

pli_status pli_orb_pyramid_level(pli_ctx* c, int32_t eye, int32_t level, uint8_t* dst, int64_t dstBytes, int32_t* w, int32_t* h) {
  CtxGuard guard__(c);
  if (!c || eye < 0 || eye > 1 || level < 0 || level >= c->hp.nlevels) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!c->orbDone[eye]) { g_err = "pli_orb_extract has not run for this eye"; return PLI_ERR_STATE; }
  const LevelGeom& G = c->hp.lv[level];
  if (w) *w = G.w;
  if (h) *h = G.h;
  if (!dst) return PLI_OK;
  if (dstBytes < (int64_t)G.w * G.h) { g_err = "buffer too small"; return PLI_ERR_CAPACITY; }
  // One device-to-host copy of the eye's whole pyramid block into pinned memory per extraction (1.3 MB at 752x480), then the levels
  // are de-pitched on the host: eight pitched hipMemcpy2D calls into pageable memory cost 0.8 ms EACH (13 ms per extractor call of
  // the adapters, which fill the public member mvImagePyramid).
  if (!c->pyrHost[eye]) HIPCHK(hipHostMalloc((void**)&c->pyrHost[eye], (size_t)c->hp.pyrBlock, hipHostMallocDefault));
  if (!c->pyrHostValid[eye]) {
    HIPCHK(hipMemcpyAsync(c->pyrHost[eye], c->pyr + (int64_t)eye * c->hp.pyrBlock, (size_t)c->hp.pyrBlock, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->pyrHostValid[eye] = true;
  }
  const uint8_t* src = c->pyrHost[eye] + G.offset;
  for (int y = 0; y < G.h; ++y) std::memcpy(dst + (size_t)y * G.w, src + (size_t)y * G.pitch, (size_t)G.w);
  return PLI_OK;
}

pli_status pli_line_extract(pli_ctx* c, int32_t eye, const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                            pli_keyline* kl, int32_t cap, uint8_t* desc, int32_t* n) {
  CtxGuard guard__(c);
  TraceRange range__("pli_line_extract");
  if (!c || eye < 0 || eye > 1 || !n) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  *n = 0;
  pli_status st = checkImage(c, img, w, h, stride);
  if (st != PLI_OK) return st;
  HIPCHK(hipSetDevice(c->device));
  if ((st = stageImage(c, eye, img, w, h, stride)) != PLI_OK) return st;
  if ((st = runLines(c, eye, 1, c->ownTable)) != PLI_OK) return st;
  const pli_table_layout& Y = c->lay;
  RecordCounts rc;
  if ((st = readCounts(c, rc)) != PLI_OK) return st;
  const int N = rc.kl[eye];
  c->lineDone[eye] = true;
  c->frameFresh = false;
  c->lineCount[eye] = N;
  *n = N;
  if (rc.linesCut[eye]) {
    g_err = "more segments pass the length cut than max_lines holds: raise pli_frontend_config.max_lines";
    return PLI_ERR_CAPACITY;
  }
  if (N > cap) { g_err = "keyline buffer too small"; return PLI_ERR_CAPACITY; }
  HIPCHK(copyColumn(c, kl, Y.off_kl[eye], N));
  HIPCHK(copyColumn(c, desc, Y.off_ldesc[eye], N, 32));
  return PLI_OK;
}

pli_status pli_selftest_hot_trig(pli_ctx* c, double* max_abs_err) {
  CtxGuard guard__(c);
  if (!c || !max_abs_err) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  pli_status st = ensureScratch(c, 256);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemsetAsync(c->scratch, 0, 8, c->stream));
  LAUNCH(c, "k_tx_hot_trig_err", k_tx_hot_trig_err, dim3(4096), dim3(256), 0, (unsigned long long*)c->scratch);
  unsigned long long bits = 0;
  HIPCHK(hipMemcpyAsync(&bits, c->scratch, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(max_abs_err, &bits, 8);
  return PLI_OK;
}

// The three forms of the CV_64F front pass (lsd_f64.hip) on the caller's images, compared on the device.  The geometry is the call's
// own (any size from 1 x 1, any scale above 1), not the context's: the context lends its device, stream, rho and flags.
// flags bit 0: the owner words carry the norm (LAZY ids); bit 1: the forms write the 16-byte records and the owner plane — what the
// schedules off the hot records take from the front pass — instead of the hot and cold planes
pli_status pli_selftest_front_stream(pli_ctx* c, const uint8_t* imgs, int32_t n, int32_t w, int32_t h, double scale, int32_t flags,
                                     int32_t out[10]) {
  CtxGuard guard__(c);
  if (!c || !imgs || !out || n < 1 || n > 64 || w < 1 || h < 1 || w > 4095 || h > 4095 || !(scale > 1) || !(scale <= 4)) {
    g_err = "bad argument";
    return PLI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(c->device));
  const DevParams& P = c->hp;
  const int dw = cvRoundd(w * scale), dh = cvRoundd(h * scale), dp = (int)alignUp(dw, 16);
  double k[7];
  const int radius = lsdGauss64(scale, c->cfg.lsd_sigma_scale, k);
  if (radius < 0) { g_err = "LSD pre-filter radius > 3 not supported"; return PLI_ERR_INVALID; }
  const std::vector<int> t = buildResizeTab64(w, h, dw, dh, 1. / scale);
  const bool tiled = frontTiledFits(t, w, h, dw, dh, radius);
  const bool stream = tiled && frontStreamFits(t, w, h, dw, dh, radius);
  if (!tiled) { g_err = "the fused front pass does not apply to this size"; return PLI_ERR_INVALID; }
  const size_t npix = (size_t)dp * dh, srcPix = (size_t)w * h;
  ScratchPlan plan;
  auto dSrc = plan.add<uint8_t>(srcPix * n);
  auto dTab = plan.add<int>(t.size());
  auto dKern = plan.add<double>(7);
  auto dBlur = plan.add<double>(srcPix * n);
  auto dScaled = plan.add<double>((size_t)dw * dh * n);
  auto dCount = plan.add<unsigned>(8);
  // per form (in the order of LsdFront): the 16-byte records and the owner plane, or the hot and cold planes; mg, maxMg
  const bool records = (flags & 2) != 0;
  struct FormOut { ScratchBlock<float4> rec; ScratchBlock<int2> own, hot; ScratchBlock<float2> cold; ScratchBlock<double> mg; ScratchBlock<unsigned long long> max; };
  std::vector<FormOut> F;
  for (int f = 0; f < 3; ++f)
    F.push_back({plan.addIf<float4>(records, npix * n), plan.addIf<int2>(records, npix * n), plan.addIf<int2>(!records, npix * n),
                 plan.addIf<float2>(!records, npix * n), plan.add<double>(npix * n), plan.add<unsigned long long>(n)});
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  // (0xA5 everywhere first: a word that a form does not write differs from the other forms' only if they wrote it)
  HIPCHK(hipMemsetAsync(plan.base(), 0xA5, plan.bytes(), c->stream));
  HIPCHK(hipMemcpyAsync(dSrc, imgs, srcPix * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dTab, t.data(), t.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dKern, k, sizeof(k), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(dCount, 0, 8 * sizeof(unsigned), c->stream));
  const FrontSrc S{dSrc, (int64_t)srcPix, w, h, w};
  const FrontGeom G{dKern, radius, dTab, dw, dh, dp, LSD_FRONT_CHUNK, P.rho, (c->cfg.parity_flags & PLI_PARITY_TRIG_F32_LSD) ? 1 : 0};
  const FrontUnfused U{dBlur, (int64_t)srcPix, dScaled, (int64_t)dw * dh, nullptr};
  for (int f = 0; f < (stream ? 3 : 2); ++f)
    if ((st = launchFront64(c, LsdFront(f), S, G, LsdFrontPlanes{F[f].rec, F[f].mg, F[f].own, F[f].hot, F[f].cold, flags & 1}, F[f].max, 0, n, U)) != PLI_OK)
      return st;
  // out[0..3]: the streaming form against the tiled one; out[4..7]: against the three kernels (where the streaming form does not
  // apply, the tiled form — what the host then runs — stands in its place in out[4..7], and out[0..3] are 0)
  const int mine = stream ? 2 : 1;
  auto diff = [&](const void* a, const void* b, size_t bytes, int slot) -> pli_status {
    const int64_t words = (int64_t)(bytes / 4);
    LAUNCH(c, "k_count_diff_words", k_count_diff_words, dim3((unsigned)std::min<int64_t>((words + 255) / 256, 4096)), dim3(256), 0,
           (const uint32_t*)a, (const uint32_t*)b, words, (unsigned*)dCount + slot);
    return PLI_OK;
  };
  for (int ref = 0; ref < 2; ++ref) {
    const int other = ref == 0 ? 1 : 0, base = ref == 0 ? 0 : 4;
    if (ref == 0 && !stream) continue;
    const FormOut &A = F[mine], &B = F[other];
    if (records) {
      if ((st = diff(A.rec, B.rec, npix * n * sizeof(float4), base + 0)) != PLI_OK) return st;
      if ((st = diff(A.own, B.own, npix * n * sizeof(int2), base + 1)) != PLI_OK) return st;
    } else {
      if ((st = diff(A.hot, B.hot, npix * n * sizeof(int2), base + 0)) != PLI_OK) return st;
      if ((st = diff(A.cold, B.cold, npix * n * sizeof(float2), base + 1)) != PLI_OK) return st;
    }
    if ((st = diff(A.mg, B.mg, npix * n * sizeof(double), base + 2)) != PLI_OK) return st;
    if ((st = diff(A.max, B.max, (size_t)n * sizeof(unsigned long long), base + 3)) != PLI_OK) return st;
  }
  unsigned counts[8];
  HIPCHK(hipMemcpyAsync(counts, dCount, sizeof(counts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < 8; ++i) out[i] = (int32_t)std::min<unsigned>(counts[i], INT32_MAX);
  out[8] = LSD_FRONT_CHUNK;
  out[9] = stream ? 1 : 0;
  return PLI_OK;
}

// One form of the CV_64F front pass (lsd_f64.hip) on the caller's images, its planes copied out: what tests compare with the oracle.
// Arguments and geometry as pli_selftest_front_stream; form: 0 the three kernels, 1 the tiled pass, 2 the streaming pass — the one
// asked for or PLI_ERR_INVALID, never another in its place.  flags bit 0 / bit 1 as there: bit 1 clear, plane_a = the hot records
// (int2), plane_b = the cold plane (float2); bit 1 set, plane_a = the 16-byte records, plane_b = the owner plane (int2).
pli_status pli_selftest_front_planes(pli_ctx* c, const uint8_t* imgs, int32_t n, int32_t w, int32_t h, double scale, int32_t form,
                                     int32_t flags, int64_t pixels, void* plane_a, void* plane_b, double* norm, uint64_t* max_bits,
                                     double* scaled) {
  CtxGuard guard__(c);
  if (!c || !imgs || !plane_a || !plane_b || !norm || !max_bits || n < 1 || n > 64 || w < 1 || h < 1 || w > 4095 || h > 4095 ||
      !(scale > 1) || !(scale <= 4) || form < 0 || form > 2 || (flags & ~3) || (form == 0 && !scaled)) {
    g_err = "bad argument";
    return PLI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(c->device));
  const int dw = cvRoundd(w * scale), dh = cvRoundd(h * scale), dp = (int)alignUp(dw, 16);
  const size_t npix = (size_t)dp * dh, srcPix = (size_t)w * h;
  if (pixels != (int64_t)(npix * n)) { g_err = "the planes hold n * alignUp(dw, 16) * dh pixels"; return PLI_ERR_INVALID; }
  double k[7];
  const int radius = lsdGauss64(scale, c->cfg.lsd_sigma_scale, k);
  if (radius < 0) { g_err = "LSD pre-filter radius > 3 not supported"; return PLI_ERR_INVALID; }
  const std::vector<int> t = buildResizeTab64(w, h, dw, dh, 1. / scale);
  const bool tiled = frontTiledFits(t, w, h, dw, dh, radius);
  if ((form >= 1 && !tiled) || (form == 2 && !frontStreamFits(t, w, h, dw, dh, radius))) {
    g_err = "this form of the front pass does not apply to this size";
    return PLI_ERR_INVALID;
  }
  const bool records = (flags & 2) != 0, unfused = form == 0;
  ScratchPlan plan;
  auto dSrc = plan.add<uint8_t>(srcPix * n);
  auto dTab = plan.add<int>(t.size());
  auto dKern = plan.add<double>(7);
  auto dBlur = plan.addIf<double>(unfused, srcPix * n);
  auto dScaled = plan.addIf<double>(unfused, (size_t)dw * dh * n);
  auto dRec = plan.addIf<float4>(records, npix * n);
  auto dOwn = plan.addIf<int2>(records, npix * n);
  auto dHot = plan.addIf<int2>(!records, npix * n);
  auto dCold = plan.addIf<float2>(!records, npix * n);
  auto dMg = plan.add<double>(npix * n);
  auto dMax = plan.add<unsigned long long>(n);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  // (0xA5 everywhere first: a word that the form does not write shows)
  HIPCHK(hipMemsetAsync(plan.base(), 0xA5, plan.bytes(), c->stream));
  HIPCHK(hipMemcpyAsync(dSrc, imgs, srcPix * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dTab, t.data(), t.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dKern, k, sizeof(k), hipMemcpyHostToDevice, c->stream));
  const FrontSrc S{dSrc, (int64_t)srcPix, w, h, w};
  const FrontGeom G{dKern, radius, dTab, dw, dh, dp, LSD_FRONT_CHUNK, c->hp.rho,
                    (c->cfg.parity_flags & PLI_PARITY_TRIG_F32_LSD) ? 1 : 0};
  const FrontUnfused U{dBlur, (int64_t)srcPix, dScaled, (int64_t)dw * dh, nullptr};
  if ((st = launchFront64(c, LsdFront(form), S, G, LsdFrontPlanes{dRec, dMg, dOwn, dHot, dCold, flags & 1}, dMax, 0, n, U)) != PLI_OK) return st;
  if (records) {
    HIPCHK(hipMemcpyAsync(plane_a, dRec, npix * n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(plane_b, dOwn, npix * n * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
  } else {
    HIPCHK(hipMemcpyAsync(plane_a, dHot, npix * n * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(plane_b, dCold, npix * n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(norm, dMg, npix * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(max_bits, dMax, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  if (unfused) HIPCHK(hipMemcpyAsync(scaled, dScaled, (size_t)dw * dh * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_lsd_round_stats(pli_ctx* c, int32_t out[4]) {
  CtxGuard guard__(c);
  if (!c || !out) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->rxSeenImages > 0 && hipEventQuery(c->evRxSeen) == hipSuccess) out[1] = foldRoundStats(c);   // (as the next call would)
  else out[1] = c->rxLastRounds;
  out[0] = c->rxPlanned;
  out[2] = (int32_t)std::min<int64_t>(c->rxSlowImages, INT32_MAX);
  out[3] = c->rxLastRounds;
  return PLI_OK;
}

pli_status pli_lsd_arena_words(pli_ctx* c, int32_t* words_per_pixel) {
  CtxGuard guard__(c);
  if (!c || !words_per_pixel) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  *words_per_pixel = c->arenaFactor;
  return PLI_OK;
}

pli_status pli_set_stereo_camera(pli_ctx* c, float bf, float fx) {
  CtxGuard guard__(c);
  if (!c || !(bf > 0) || !(fx > 0)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (bf == c->cfg.bf && fx == c->cfg.fx) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));           // kernels in flight read the old parameter block
  if (c->aux) HIPCHK(hipStreamSynchronize(c->aux));
  c->cfg.bf = bf; c->cfg.fx = fx;
  c->pointsFresh = false;                            // a fused Frame's cached mvuRight / mvDepth belong to the old rig (Frame.cc:1005-1008,
                                                     // 1131: maxD and bf / disparity); the line matcher does not read the rig
  c->hp.bf = bf;
  c->hp.maxD = c->cfg.stereo_maxd_inf ? std::numeric_limits<float>::infinity() : bf / (bf / fx);
  HIPCHK(hipMemcpy(c->dP, &c->hp, sizeof(DevParams), hipMemcpyHostToDevice));
  return PLI_OK;
}

pli_status pli_last_counts(pli_ctx* c, int32_t counts[4]) {
  CtxGuard guard__(c);
  if (!c || !counts) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  for (int e = 0; e < 2; ++e) {
    counts[e] = c->orbDone[e] ? c->orbCount[e] : -1;
    counts[2 + e] = c->lineDone[e] ? c->lineCount[e] : -1;
  }
  return PLI_OK;
}

pli_status pli_stereo_match_points(pli_ctx* c, float* uright, float* depth, int32_t cap) {
  CtxGuard guard__(c);
  TraceRange range__("pli_stereo_match_points");
  if (!c) return PLI_ERR_INVALID;
  if (!c->orbDone[0] || !c->orbDone[1]) { g_err = "pli_orb_extract must run for both eyes first"; return PLI_ERR_STATE; }
  if (c->frameFresh && c->pointsFresh) {                // (pli_frame_extract has matched already, with this rig)
    const pli_table_layout& Yf = c->lay;
    const int Nf = c->orbCount[0];
    if (Nf > cap) { g_err = "output buffer too small"; return PLI_ERR_CAPACITY; }
    if (uright) std::memcpy(uright, c->hostRec.data() + Yf.off_uright, (size_t)Nf * 4);
    if (depth) std::memcpy(depth, c->hostRec.data() + Yf.off_depth, (size_t)Nf * 4);
    return PLI_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  pli_status st = runStereoPoints(c, 1, c->ownTable);
  if (st != PLI_OK) return st;
  const pli_table_layout& Y = c->lay;
  RecordCounts rc;
  if ((st = readCounts(c, rc)) != PLI_OK) return st;
  const int N = rc.kp[0];
  if (c->frameFresh) {                                  // the Frame's cached record follows the rig it was re-matched with
    HIPCHK(copyColumn(c, reinterpret_cast<float*>(c->hostRec.data() + Y.off_uright), Y.off_uright, N));
    HIPCHK(copyColumn(c, reinterpret_cast<float*>(c->hostRec.data() + Y.off_depth), Y.off_depth, N));
  }
  c->pointsFresh = c->frameFresh;
  if (N > cap) { g_err = "output buffer too small"; return PLI_ERR_CAPACITY; }
  HIPCHK(copyColumn(c, uright, Y.off_uright, N));
  HIPCHK(copyColumn(c, depth, Y.off_depth, N));
  return PLI_OK;
}

pli_status pli_stereo_from_depth(pli_ctx* c, const float* depth, int64_t strideFloats, float* uright, float* depthOut, int32_t cap) {
  CtxGuard guard__(c);
  if (!c || !depth || strideFloats < c->cfg.width) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!c->orbDone[0]) { g_err = "pli_orb_extract must run for the left eye first"; return PLI_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  const int W = c->cfg.width, H = c->cfg.height;
  const size_t el = depthElemBytes(c);        // (pli_set_depth_format: `depth` holds floats or uint16_t, the stride counts elements)
  pli_status st = ensureScratch(c, (size_t)W * H * el);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemcpy2DAsync(c->scratch, (size_t)W * el, depth, (size_t)strideFloats * el, (size_t)W * el, H, hipMemcpyHostToDevice, c->stream));
  const pli_table_layout& Y = c->lay;
  LAUNCH(c, "k_stereo_from_depth", k_stereo_from_depth, dim3((c->hp.kpCap + 255) / 256), dim3(256), 0, c->dP, (const void*)c->scratch,
         c->depthFmt, (int64_t)W, W, H, c->ownTable, Y.off_counts, Y.off_kp[0], Y.off_uright, Y.off_depth);
  RecordCounts rc;
  if ((st = readCounts(c, rc)) != PLI_OK) return st;
  const int N = rc.kp[0];
  if (N > cap) { g_err = "output buffer too small"; return PLI_ERR_CAPACITY; }
  HIPCHK(copyColumn(c, uright, Y.off_uright, N));
  HIPCHK(copyColumn(c, depthOut, Y.off_depth, N));
  return PLI_OK;
}

// ORBextractor::operator() with a lapping area (ORBextractor.cc:1135-1144): pli_orb_extract, then the device table of that eye
// is put into the reference's mono-first / lapping-from-the-back order (k_lapping_order), which is the order
// pli_stereo_fisheye expects; *n_mono = the reference's return value (monoIndex).
pli_status pli_orb_extract_lapping(pli_ctx* c, int32_t eye, const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                                   int32_t lap0, int32_t lap1, pli_keypoint* kp, int32_t cap, uint8_t* desc, int32_t* n,
                                   int32_t* n_mono) {
  CtxGuard guard__(c);
  if (!n_mono) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  *n_mono = 0;
  pli_status st = pli_orb_extract(c, eye, img, w, h, stride, nullptr, INT_MAX, nullptr, n);
  if (st != PLI_OK) return st;
  const int N = *n;
  if (N > cap) { g_err = "keypoint buffer too small"; return PLI_ERR_CAPACITY; }
  if (N == 0) return PLI_OK;
  const pli_table_layout& Y = c->lay;
  ScratchPlan plan;
  auto sk = plan.add<pli_keypoint>(N);
  auto sd = plan.add<uint8_t>((size_t)N * 32);
  auto dmono = plan.add<int>(1);
  if ((st = commitScratch(c, plan)) != PLI_OK) return st;
  pli_keypoint* tk = (pli_keypoint*)(c->ownTable + Y.off_kp[eye]);
  uint8_t* td = c->ownTable + Y.off_desc[eye];
  HIPCHK(hipMemcpyAsync(sk, tk, (size_t)N * sizeof(pli_keypoint), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sd, td, (size_t)N * 32, hipMemcpyDeviceToDevice, c->stream));
  LAUNCH(c, "k_lapping_order", k_lapping_order, dim3(1), dim3(1024), 0, (const pli_keypoint*)sk, (const uint8_t*)sd, N, (float)lap0,
         (float)lap1, tk, td, dmono);
  if (kp) HIPCHK(hipMemcpyAsync(kp, tk, (size_t)N * sizeof(pli_keypoint), hipMemcpyDeviceToHost, c->stream));
  if (desc) HIPCHK(hipMemcpyAsync(desc, td, (size_t)N * 32, hipMemcpyDeviceToHost, c->stream));
  if ((st = fetchCount(c, dmono, n_mono)) != PLI_OK) return st;
  c->monoCount[eye] = *n_mono;
  return PLI_OK;
}

// ---- single-camera Frames of a distorted pinhole camera (frame_kernels.hip) ----
// the state without a camera: nothing is undistorted and the grid spans the image (Frame.cc:967-973)
static void clearPinhole(pli_ctx* c) {
  c->pinhole = PinholeUndist{};
  c->pinhole.maxX = (float)c->cfg.width;
  c->pinhole.maxY = (float)c->cfg.height;
}

// Frame::ComputeImageBounds (Frame.cc:947-974) and the camera of the two calls below
pli_status pli_set_pinhole_distortion(pli_ctx* c, const pli_pinhole_distortion* cam, float bounds[4]) {
  CtxGuard guard__(c);
  if (!c) { g_err = "null argument"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  clearPinhole(c);
  if (cam && cam->k1 != 0.0f) {                    // (:949 `mDistCoef.at<float>(0)!=0.0`)
    PinholeUndist U = c->pinhole;
    U.cam = *cam;
    U.on = 1;
    const float W = (float)c->cfg.width, H = (float)c->cfg.height;
    const float2 corners[4] = {{0.f, 0.f}, {W, 0.f}, {0.f, H}, {W, H}};       // (:952-955)
    float2 m[4];
    ScratchPlan plan;
    auto din = plan.in(corners, 4);
    auto dout = plan.add<float2>(4);
    pli_status st = commitScratch(c, plan);
    if (st != PLI_OK) return st;
    LAUNCH(c, "k_undistort_points", k_undistort_points, dim3(1), dim3(64), 0, U, (const float2*)din, 4, (float2*)dout, (int*)nullptr);
    HIPCHK(download(c, m, dout));
    HIPCHK(hipStreamSynchronize(c->stream));
    U.minX = std::min(m[0].x, m[2].x);             // (:962-965)
    U.maxX = std::max(m[1].x, m[3].x);
    U.minY = std::min(m[0].y, m[1].y);
    U.maxY = std::max(m[2].y, m[3].y);
    c->pinhole = U;
  } else if (cam) {
    c->pinhole.cam = *cam;                         // (kept for the record; with k1 == 0 nothing reads it)
  }
  if (bounds) { bounds[0] = c->pinhole.minX; bounds[1] = c->pinhole.maxX; bounds[2] = c->pinhole.minY; bounds[3] = c->pinhole.maxY; }
  return PLI_OK;
}

// cv::undistortPoints of Frame::UndistortKeyPoints / UndistortKeyLines (Frame.cc:891, :931-932) and Frame::PosInGrid (:845-855) on
// caller tables
pli_status pli_undistort_points(pli_ctx* c, const float* xy, int32_t n, float* xyUn, int32_t* cell) {
  CtxGuard guard__(c);
  if (!c || n < 0 || (n > 0 && (!xy || !xyUn))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (n == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto din = plan.in(reinterpret_cast<const float2*>(xy), (size_t)n);
  auto dout = plan.add<float2>((size_t)n);
  auto dcell = plan.addIf<int>(cell != nullptr, (size_t)n);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  LAUNCH(c, "k_undistort_points", k_undistort_points, dim3((n + 255) / 256), dim3(256), 0, c->pinhole, (const float2*)din, (int)n,
         (float2*)dout, (int*)dcell);
  HIPCHK(download(c, reinterpret_cast<float2*>(xyUn), dout));
  HIPCHK(download(c, (int*)cell, dcell));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

// The monocular (Frame.cc:334-448) and RGB-D (:231-331) constructors' front-end in one submission: see include/pli_frontend.h.
pli_status pli_frame_extract_single(pli_ctx* c, const uint8_t* img, int32_t w, int32_t h, int64_t stride, int32_t lap0, int32_t lap1,
                                    const float* depth, int64_t depthStrideFloats, void* record, float* kpUn, float* klUn,
                                    int32_t* cell, int32_t* n_mono) {
  CtxGuard guard__(c);
  TraceRange range__("pli_frame_extract_single");
  if (!c || !record || !kpUn || !klUn || !cell || !n_mono) { g_err = "null argument"; return PLI_ERR_INVALID; }
  *n_mono = 0;
  pli_status st = checkImage(c, img, w, h, stride);
  if (st != PLI_OK) return st;
  if (depth && depthStrideFloats < w) { g_err = "depth stride < width"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const int W = c->cfg.width, H = c->cfg.height;
  const pli_table_layout& Y = c->lay;
  const DevParams& P = c->hp;
  // what the call stages and what it reads back: the depth image; the snapshot of the eye's table that the lapping reorder reads; the
  // caller's three columns and the mono count, contiguous behind each other so that one copy brings them to the pinned buffer
  const size_t kpUnBytes = (size_t)P.kpCap * sizeof(float2), klUnBytes = (size_t)P.klCap * sizeof(float4), cellBytes = (size_t)P.kpCap * 4;
  const size_t offKl = alignUp(kpUnBytes, 16), offCell = offKl + klUnBytes, offMono = offCell + cellBytes, outBytes = offMono + 4;
  ScratchPlan plan;
  const size_t el = depthElemBytes(c);        // (pli_set_depth_format: `depth` holds floats or uint16_t, the stride counts elements)
  auto ddepth = plan.addIf<uint8_t>(depth != nullptr, (size_t)W * H * el);
  auto sk = plan.add<pli_keypoint>((size_t)P.kpCap);
  auto sd = plan.add<uint8_t>((size_t)P.kpCap * 32);
  auto dout = plan.add<uint8_t>(outBytes);
  if ((st = commitScratch(c, plan)) != PLI_OK) return st;
  const size_t recBytes = (size_t)Y.record_bytes, pinnedNeed = alignUp((int64_t)recBytes, 16) + outBytes;
  if (!c->recPinned || c->recPinnedBytes < pinnedNeed) {
    if (c->recPinned) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipHostFree(c->recPinned)); c->recPinned = nullptr; }
    HIPCHK(hipHostMalloc((void**)&c->recPinned, pinnedNeed, hipHostMallocDefault));
    c->recPinnedBytes = pinnedNeed;
  }
  // the record starts from zeros, as pli_frame_extract's does: what it returns does not depend on an earlier Frame, and what the
  // per-call entry points cached about eye 1 ends here (a single-camera Frame has no right eye)
  c->frameFresh = c->pointsFresh = false;
  for (int e = 0; e < 2; ++e) { c->orbDone[e] = c->lineDone[e] = false; c->pyrHostValid[e] = false; }
  HIPCHK(hipMemsetAsync(c->ownTable, 0, recBytes, c->stream));
  const size_t row = (size_t)rowBytes(c);
  HIPCHK(hipMemcpy2DAsync(c->inStage[0], row, img, stride, row, H, hipMemcpyHostToDevice, c->stream));
  if (depth)
    HIPCHK(hipMemcpy2DAsync(ddepth, (size_t)W * el, depth, (size_t)depthStrideFloats * el, (size_t)W * el, H, hipMemcpyHostToDevice, c->stream));
  if ((st = runIngest(c, c->inStage[0], c->inStage[1], (int64_t)row, 0, 0, 1)) != PLI_OK) return st;
  if (chainsRunBeside(c, 1)) {
    if ((st = runChainsBeside(c, 0, 1, c->ownTable, 0)) != PLI_OK) return st;
  } else {
    if ((st = runOrb(c, 0, 1, c->ownTable)) != PLI_OK) return st;
    if ((st = runLines(c, 0, 1, c->ownTable)) != PLI_OK) return st;
  }
  // the lapping reorder (ORBextractor.cc:1135-1144) with the count read on the device; {0, 0} and every other area still go through
  // it, as pli_orb_extract_lapping does: the order and the mono count are the kernel's
  pli_keypoint* tk = (pli_keypoint*)(c->ownTable + Y.off_kp[0]);
  uint8_t* td = c->ownTable + Y.off_desc[0];
  int* dmono = reinterpret_cast<int*>((uint8_t*)dout + offMono);
  HIPCHK(hipMemcpyAsync(sk, tk, (size_t)P.kpCap * sizeof(pli_keypoint), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sd, td, (size_t)P.kpCap * 32, hipMemcpyDeviceToDevice, c->stream));
  LAUNCH(c, "k_lapping_order", k_lapping_order_counted, dim3(1), dim3(1024), 0, (const pli_keypoint*)sk, (const uint8_t*)sd,
         reinterpret_cast<const int*>(c->ownTable + Y.off_counts), P.kpCap, (float)lap0, (float)lap1, tk, td, dmono);
  LAUNCH(c, "k_frame_single_tail", k_frame_single_tail, dim3((P.kpCap + P.klCap + 255) / 256), dim3(256), 0, c->dP, c->pinhole,
         (const void*)(uint8_t*)ddepth, c->depthFmt, (int64_t)W, c->ownTable, Y.off_counts, Y.off_kp[0], Y.off_kl[0], Y.off_uright, Y.off_depth,
         reinterpret_cast<float2*>((uint8_t*)dout), reinterpret_cast<int*>((uint8_t*)dout + offCell),
         reinterpret_cast<float4*>((uint8_t*)dout + offKl));
  uint8_t* pinOut = c->recPinned + alignUp((int64_t)recBytes, 16);
  HIPCHK(hipMemcpyAsync(c->recPinned, c->ownTable, recBytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(pinOut, (uint8_t*)dout, outBytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(record, c->recPinned, recBytes);
  std::memcpy(kpUn, pinOut, kpUnBytes);
  std::memcpy(klUn, pinOut + offKl, klUnBytes);
  std::memcpy(cell, pinOut + offCell, cellBytes);
  std::memcpy(n_mono, pinOut + offMono, 4);
  RecordCounts rc;
  std::memcpy(&rc, c->recPinned + Y.off_counts, sizeof(rc));
  c->orbDone[0] = c->lineDone[0] = true;
  c->orbCount[0] = rc.kp[0];
  c->lineCount[0] = rc.kl[0];
  c->monoCount[0] = *n_mono;
  if (rc.kpCut[0]) { g_err = "more keypoints than kp_cap holds"; return PLI_ERR_CAPACITY; }
  if (rc.linesCut[0]) { g_err = "more segments pass the length cut than max_lines holds: raise pli_frontend_config.max_lines"; return PLI_ERR_CAPACITY; }
  return PLI_OK;
}

// Frame::ComputeStereoFishEyeMatches (Frame.cc:1577-1618): tables on the device (kL/dL/kR/dR: the context's record) or, with
// `hostTables`, the caller's, which are staged in blocks of the same plan; results to host buffers.
static pli_status fisheyeCore(pli_ctx* c, bool hostTables, const pli_keypoint* kL, const uint8_t* dL, int NL, int monoL,
                              const pli_keypoint* kR, const uint8_t* dR, int NR, int monoR, const pli_kb8_camera* cam1,
                              const pli_kb8_camera* cam2, const float* Rlr, const float* tlr, int32_t* l2r, int32_t* r2l, float* depth,
                              float* p3d, int32_t* nmatches) {
  monoL = std::min(std::max(monoL, 0), NL);
  monoR = std::min(std::max(monoR, 0), NR);
  const int nq = NL - monoL, nt = NR - monoR;
  if (hostTables) {
    // k_fisheye_triangulate indexes mvLevelSigma2 by the octave of both keypoints and projects with their coordinates: the
    // caller's rows are checked here, before anything is allocated or launched (the oracle's orc_fisheye_tables_valid is the same list)
    for (int e = 0; e < 2; ++e) {
      const pli_keypoint* k = e ? kR : kL;
      const int n = e ? NR : NL;
      for (int i = 0; i < n; ++i)
        if (!std::isfinite(k[i].x) || !std::isfinite(k[i].y) || k[i].octave < 0 || k[i].octave >= c->hp.nlevels) {
          g_err = "pli_stereo_fisheye_tables: a keypoint's octave is outside 0 .. nlevels-1 or its coordinates are not finite";
          return PLI_ERR_INVALID;
        }
    }
  }
  float hRt[12], hsig[MAX_LEVELS];
  for (int i = 0; i < 9; ++i) hRt[i] = Rlr[i];
  for (int i = 0; i < 3; ++i) hRt[9 + i] = tlr[i];
  for (int l = 0; l < c->hp.nlevels; ++l) hsig[l] = c->hp.lv[l].scale * c->hp.lv[l].scale;      // mvLevelSigma2, ORBextractor.cc:424
  const int sL = hostTables ? NL : 0, sR = hostTables ? NR : 0;      // rows staged from the caller's tables
  ScratchPlan plan;
  auto kidx = plan.add<int>((size_t)nq * 2);             // k_knn2: two ints per query, the indices ...
  auto kdst = plan.add<int>((size_t)nq * 2);             // ... and the distances
  auto dl2r = plan.add<int>(NL);
  auto ddepth = plan.add<float>(NL);
  auto dr2l = plan.add<int>(NR);
  auto dp3 = plan.add<float>((size_t)NL * 3);
  auto dRt = plan.in(hRt, 12);
  auto dsig = plan.in(hsig, c->hp.nlevels);
  auto dcnt = plan.add<int>(1);
  auto skL = plan.in(kL, sL);
  auto sdL = plan.in(dL, (size_t)sL * 32);
  auto skR = plan.in(kR, sR);
  auto sdR = plan.in(dR, (size_t)sR * 32);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  if (hostTables) { kL = skL; dL = sdL; kR = skR; dR = sdR; }
  HIPCHK(hipMemsetAsync(dl2r, 0xFF, (size_t)std::max(NL, 1) * 4, c->stream));
  HIPCHK(hipMemsetAsync(dr2l, 0xFF, (size_t)std::max(NR, 1) * 4, c->stream));
  HIPCHK(hipMemsetAsync(dp3, 0, (size_t)std::max(NL, 1) * 12, c->stream));
  HIPCHK(hipMemsetAsync(dcnt, 0, 4, c->stream));
  LAUNCH(c, "k_fill_f32", k_fill_f32, dim3((std::max(NL, 1) + 255) / 256), dim3(256), 0, ddepth, std::max(NL, 1), -1.0f);
  if (nq > 0) {
    LAUNCH(c, "k_knn2", k_knn2, dim3(nq), dim3(64), 0, dL + (size_t)monoL * 32, nq, dR + (size_t)monoR * 32, nt, kidx, kdst);
    Kb8 c1, c2;
    memcpy(&c1, cam1, sizeof(c1));
    memcpy(&c2, cam2, sizeof(c2));
    LAUNCH(c, "k_fisheye_triangulate", k_fisheye_triangulate, dim3((nq + 63) / 64), dim3(64), 0, kL, kR, (const int*)kidx,
           (const int*)kdst, nq, nt, monoL, monoR, c1, c2, (const float*)dRt, (const float*)dsig, dl2r, dr2l, ddepth, dp3, dcnt);
  }
  HIPCHK(download(c, l2r, dl2r));
  HIPCHK(download(c, r2l, dr2l));
  HIPCHK(download(c, depth, ddepth));
  HIPCHK(download(c, p3d, dp3));
  return fetchCount(c, dcnt, nmatches);
}

// ... on the device tables of the last pli_orb_extract_lapping of both eyes
pli_status pli_stereo_fisheye(pli_ctx* c, const pli_kb8_camera* cam1, const pli_kb8_camera* cam2, const float* Rlr, const float* tlr,
                              int32_t* l2r, int32_t capL, int32_t* r2l, int32_t capR, float* depth, float* p3d, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || !cam1 || !cam2 || !Rlr || !tlr) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nmatches) *nmatches = 0;
  if (!c->orbDone[0] || !c->orbDone[1]) { g_err = "pli_orb_extract_lapping must run for both eyes first"; return PLI_ERR_STATE; }
  HIPCHK(hipSetDevice(c->device));
  const pli_table_layout& Y = c->lay;
  RecordCounts rc;
  pli_status st = readCounts(c, rc);
  if (st != PLI_OK) return st;
  const int NL = rc.kp[0], NR = rc.kp[1];
  if (NL > capL || NR > capR) { g_err = "output buffer too small"; return PLI_ERR_CAPACITY; }
  return fisheyeCore(c, false, (const pli_keypoint*)(c->ownTable + Y.off_kp[0]), c->ownTable + Y.off_desc[0], NL, c->monoCount[0],
                     (const pli_keypoint*)(c->ownTable + Y.off_kp[1]), c->ownTable + Y.off_desc[1], NR, c->monoCount[1], cam1, cam2,
                     Rlr, tlr, l2r, r2l, depth, p3d, nmatches);
}

// ... on caller tables (the Frame members mvKeys / mDescriptors / mvKeysRight / mDescriptorsRight, monoLeft / monoRight)
pli_status pli_stereo_fisheye_tables(pli_ctx* c, const pli_keypoint* kpL, const uint8_t* descL, int32_t nleft, int32_t monoLeft,
                                     const pli_keypoint* kpR, const uint8_t* descR, int32_t nright, int32_t monoRight,
                                     const pli_kb8_camera* cam1, const pli_kb8_camera* cam2, const float* Rlr, const float* tlr,
                                     int32_t* l2r, int32_t* r2l, float* depth, float* p3d, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || !cam1 || !cam2 || !Rlr || !tlr || nleft < 0 || nright < 0 || (nleft > 0 && (!kpL || !descL)) ||
      (nright > 0 && (!kpR || !descR))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nmatches) *nmatches = 0;
  HIPCHK(hipSetDevice(c->device));
  return fisheyeCore(c, true, kpL, descL, nleft, monoLeft, kpR, descR, nright, monoRight, cam1, cam2, Rlr, tlr, l2r, r2l, depth, p3d,
                     nmatches);
}

pli_status pli_stereo_match_lines(pli_ctx* c, float* disp, double* le, int32_t cap) {
  CtxGuard guard__(c);
  TraceRange range__("pli_stereo_match_lines");
  if (!c) return PLI_ERR_INVALID;
  if (!c->lineDone[0] || !c->lineDone[1]) { g_err = "pli_line_extract must run for both eyes first"; return PLI_ERR_STATE; }
  if (c->frameFresh) {                                  // (pli_frame_extract has matched already)
    const pli_table_layout& Yf = c->lay;
    const int Nf = c->lineCount[0];
    if (Nf > cap) { g_err = "output buffer too small"; return PLI_ERR_CAPACITY; }
    if (disp) std::memcpy(disp, c->hostRec.data() + Yf.off_disp, (size_t)Nf * 8);
    if (le) std::memcpy(le, c->hostRec.data() + Yf.off_le, (size_t)Nf * 24);
    return PLI_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  pli_status st = runStereoLines(c, 1, c->ownTable);
  if (st != PLI_OK) return st;
  const pli_table_layout& Y = c->lay;
  RecordCounts rc;
  if ((st = readCounts(c, rc)) != PLI_OK) return st;
  const int N = rc.kl[0];
  if (N > cap) { g_err = "output buffer too small"; return PLI_ERR_CAPACITY; }
  HIPCHK(copyColumn(c, disp, Y.off_disp, N, 2));
  HIPCHK(copyColumn(c, le, Y.off_le, N, 3));
  return PLI_OK;
}

// ---- frame-to-frame track matching of a batch (match_kernels.hip: k_track_*) ------------------------
static void trackLayout(const pli_ctx* c, pli_track_layout& L) {
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t r = o; o = alignUp(o + bytes, 16); return r; };
  L.kp_cap = c->hp.kpCap; L.kl_cap = c->hp.klCap;
  L.off_counts = take(16);
  L.off_best = take((int64_t)L.kp_cap * 4);
  L.off_lines = take((int64_t)L.kl_cap * 4);
  L.record_bytes = alignUp(o, 256);
}

pli_status pli_track_layout_get(const pli_ctx* c, pli_track_layout* out) {
  CtxGuard guard__(c);
  if (!c || !out) return PLI_ERR_INVALID;
  trackLayout(c, *out);
  return PLI_OK;
}

pli_status pli_batch_track(pli_ctx* c, int32_t nframes, const void* table, const float* poses, const pli_track_params* tpar,
                           void* track) {
  CtxGuard guard__(c);
  TraceRange range__("pli_batch_track");
  if (!c || !table || !poses || !tpar || !track) { g_err = "null argument"; return PLI_ERR_INVALID; }
  if (nframes < 1 || nframes > c->cfg.max_frames) { g_err = "nframes exceeds the context's max_frames"; return PLI_ERR_INVALID; }
  if (!(tpar->max_x > tpar->min_x) || !(tpar->max_y > tpar->min_y) || !(tpar->fx > 0) || !(tpar->fy > 0)) { g_err = "bad track parameters"; return PLI_ERR_INVALID; }
  if (nframes < 2) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  const DevParams& P = c->hp;
  if ((size_t)P.kpCap * 4 > 160 * 1024 - 1024) { g_err = "too many keypoints for the LDS owner table of the batch track matcher"; return PLI_ERR_INVALID; }
  pli_track_layout TL;
  trackLayout(c, TL);
  TrackParams tp;
  tp.fx = tpar->fx; tp.fy = tpar->fy; tp.cx = tpar->cx; tp.cy = tpar->cy; tp.bf = tpar->bf; tp.th = tpar->th;
  tp.minX = tpar->min_x; tp.maxX = tpar->max_x; tp.minY = tpar->min_y; tp.maxY = tpar->max_y;
  tp.mono = tpar->mono; tp.checkOri = tpar->check_orientation; tp.nnrLines = tpar->nnr_lines;
  tp.kpCap = P.kpCap; tp.klCap = P.klCap;
  const pli_table_layout& Y = c->lay;
  tp.recordBytes = Y.record_bytes; tp.offCounts = Y.off_counts; tp.offKp0 = Y.off_kp[0]; tp.offDesc0 = Y.off_desc[0];
  tp.offUr = Y.off_uright; tp.offDepth = Y.off_depth; tp.offLd0 = Y.off_ldesc[0];
  tp.trackBytes = TL.record_bytes; tp.toffCounts = TL.off_counts; tp.toffBest = TL.off_best; tp.toffLines = TL.off_lines;
  const size_t NF = (size_t)nframes;
  ScratchPlan plan;
  auto dq = plan.add<pli_proj_query>(NF * P.kpCap);
  auto dkeys = plan.add<unsigned long long>(NF * P.kpCap * PROJ_K);
  auto dcc = plan.add<int>(NF * P.kpCap);
  auto dl = plan.add<int>(NF * std::max(P.klCap, 1));
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const uint8_t* T = (const uint8_t*)table;
  LAUNCH(c, "k_track_queries", k_track_queries, dim3((P.kpCap + 255) / 256, nframes - 1), dim3(256), 0, c->dP, T, poses, tp, dq);
  LAUNCH(c, "k_track_candidates", k_track_candidates, dim3(P.kpCap, nframes - 1), dim3(64), 0, T, tp, dq, dkeys, dcc);
  LAUNCH(c, "k_track_assign", k_track_assign, dim3(nframes - 1), dim3(64), (size_t)P.kpCap * 4, T, tp, dq, dkeys, dcc, (uint8_t*)track);
  LAUNCH(c, "k_track_lines", k_track_lines, dim3(nframes - 1), dim3(256), 0, T, tp, c->cfg.best_lr_matches != 0 ? 1 : 0, dl, (uint8_t*)track);
  return PLI_OK;
}

// ---- measurement -----------------------------------------------------------
int64_t pli_trace_ranges(void) { return (int64_t)g_roctx.pushed.load(std::memory_order_relaxed); }

pli_status pli_prof_enable(pli_ctx* c, int32_t on) {
  CtxGuard guard__(c);
  if (!c) return PLI_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->prof = on != 0;
  return PLI_OK;
}
pli_status pli_prof_reset(pli_ctx* c) {
  CtxGuard guard__(c);
  if (!c) return PLI_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->profLog.clear();
  c->evNext = 0;
  return PLI_OK;
}
pli_status pli_prof_report(pli_ctx* c, char* buf, int64_t bytes) {
  CtxGuard guard__(c);
  if (!c || !buf || bytes <= 0) return PLI_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(c->stream));
  std::map<std::string, std::pair<int, double>> acc;
  std::vector<std::string> orderNames;
  for (const ProfEntry& e : c->profLog) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) continue;
    auto it = acc.find(e.name);
    if (it == acc.end()) { acc[e.name] = std::make_pair(1, (double)ms); orderNames.push_back(e.name); }
    else { it->second.first++; it->second.second += ms; }
  }
  std::string s;
  char line[256];
  for (const std::string& nme : orderNames) {
    std::snprintf(line, sizeof(line), "%s %d %.6f\n", nme.c_str(), acc[nme].first, acc[nme].second);
    s += line;
  }
  if ((int64_t)s.size() + 1 > bytes) { g_err = "report buffer too small"; return PLI_ERR_CAPACITY; }
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return PLI_OK;
}

pli_status pli_debug_enable(pli_ctx* c, int32_t on) {
  CtxGuard guard__(c);
  if (!c) return PLI_ERR_INVALID;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (on && !c->angDbg) {
    pli_status st;
    if ((st = c->dalloc(&c->blur, (size_t)c->hp.pyrBlock * c->NI)) != PLI_OK) return st;
    if ((st = c->dalloc(&c->angDbg, (size_t)c->hp.LW * c->hp.LH * c->NI)) != PLI_OK) return st;
    if ((st = c->dalloc(&c->lbdFloat, (size_t)c->NI * c->hp.klCap * 72)) != PLI_OK) return st;
    if (c->lsdF64 && (st = c->dalloc(&c->scaled64Dbg, (size_t)c->hp.LW * c->hp.LH * c->NI)) != PLI_OK) return st;
  }
  c->debug = on != 0;
  // (a debug context lists every detected segment — PLI_DBG_LSD_SEGMENTS is compared with the reference's detector there —: no short-segment cut)
  c->hp.segBoxCut = c->debug ? -1 : lsd_seg_box_cut(c->hp.lsdScale, c->hp.minLength, c->hp.W, c->hp.H);
  HIPCHK(hipMemcpy(c->dP, &c->hp, sizeof(DevParams), hipMemcpyHostToDevice));
  return PLI_OK;
}

pli_status pli_debug_fetch(pli_ctx* c, int32_t image, int32_t what, int32_t arg, void* dst, int64_t dstBytes, int64_t* outBytes) {
  CtxGuard guard__(c);
  if (!c || image < 0 || image >= c->NI || !outBytes) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const DevParams& P = c->hp;
  auto need = [&](int64_t n) -> bool { *outBytes = n; return dst && dstBytes >= n; };
  switch (what) {
    case PLI_DBG_PYRAMID_LEVEL:
    case PLI_DBG_BLUR_LEVEL: {
      if (arg < 0 || arg >= P.nlevels) return PLI_ERR_INVALID;
      const LevelGeom& G = P.lv[arg];
      if (what == PLI_DBG_BLUR_LEVEL && !c->blur) { g_err = "pli_debug_enable was not on during the run"; return PLI_ERR_STATE; }
      if (!need((int64_t)G.w * G.h)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      const uint8_t* base = (what == PLI_DBG_PYRAMID_LEVEL ? c->pyr : c->blur) + (int64_t)image * P.pyrBlock + G.offset;
      HIPCHK(hipMemcpy2D(dst, G.w, base, G.pitch, G.w, G.h, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_FAST_CANDIDATES:
    case PLI_DBG_LEVEL_KEYPOINTS: {
      if (arg < 0 || arg >= P.nlevels) return PLI_ERR_INVALID;
      const LevelGeom& G = P.lv[arg];
      int n = 0;
      const int* cntp = (what == PLI_DBG_FAST_CANDIDATES ? c->candCount : c->kpSelCount) + image * P.nlevels + arg;
      HIPCHK(hipMemcpy(&n, cntp, 4, hipMemcpyDeviceToHost));
      if (!need(4 + (int64_t)n * 12)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      std::vector<uint32_t> raw(std::max(n, 1));
      const uint32_t* src = what == PLI_DBG_FAST_CANDIDATES ? c->candAll + (int64_t)image * P.candPerImage + G.candBase
                                                            : c->kpSel + (int64_t)image * P.kpSlotsPerImage + G.kpBase;
      if (n) HIPCHK(hipMemcpy(raw.data(), src, (size_t)n * 4, hipMemcpyDeviceToHost));
      int* o = (int*)dst;
      o[0] = n;
      for (int i = 0; i < n; ++i) { o[1 + 3 * i] = (raw[i] >> 8) & 0xFFF; o[2 + 3 * i] = raw[i] >> 20; o[3 + 3 * i] = raw[i] & 0xFF; }
      return PLI_OK;
    }
    case PLI_DBG_LSD_SCALED: {
      if (c->lsdF64) {     // CV_64F pipeline: doubles (the debug copy: the plane itself is the growers' arena)
        if (!need((int64_t)P.LWt * P.LH * 8)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
        if (!c->scaled64Dbg) { g_err = "pli_debug_enable was not on during the run"; return PLI_ERR_STATE; }
        const double* src64 = c->scaled64Dbg;     // (rows of the true width, images pitch x height apart: lineFront, line_chain.hip)
        HIPCHK(hipMemcpy(dst, src64 + (int64_t)image * P.LW * P.LH, (size_t)P.LWt * P.LH * 8, hipMemcpyDeviceToHost));
        return PLI_OK;
      }
      if (!need((int64_t)P.LWt * P.LH)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      if (c->cfg.lsd_scale != 1)
        HIPCHK(hipMemcpy2D(dst, P.LWt, c->lsdScaled + (int64_t)image * c->lsdStride, P.lpitch, P.LWt, P.LH, hipMemcpyDeviceToHost));
      else
        HIPCHK(hipMemcpy2D(dst, P.W, c->pyr + (int64_t)image * P.pyrBlock, P.lv[0].pitch, P.W, P.H, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_LSD_ANGLE: {
      if (!c->angDbg) { g_err = "pli_debug_enable was not on during the run"; return PLI_ERR_STATE; }
      const int64_t n = (int64_t)P.LWt * P.LH * 4;   // (the debug plane has rows of the true width)
      if (!need(n)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      HIPCHK(hipMemcpy(dst, c->angDbg + (int64_t)image * P.LWt * P.LH, n, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_LSD_SEGMENTS: {
      int n = 0;
      HIPCHK(hipMemcpy(&n, c->nSeg + image, 4, hipMemcpyDeviceToHost));
      if (!need(4 + (int64_t)n * 16)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      *(int*)dst = n;
      if (n) HIPCHK(hipMemcpy((char*)dst + 4, c->seg + (int64_t)image * c->maxSeg * 4, (size_t)n * 16, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_LSD_ORDER: {
      int n = 0;
      HIPCHK(hipMemcpy(&n, c->nDefined + image, 4, hipMemcpyDeviceToHost));
      if (!need(4 + (int64_t)n * 4)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      *(int*)dst = n;
      if (n) HIPCHK(hipMemcpy((char*)dst + 4, c->order + (int64_t)image * P.LW * P.LH, (size_t)n * 4, hipMemcpyDeviceToHost));
      if (P.LW != P.LWt) {     // device pixel indices are y * pitch + x: the caller gets y * width + x
        int* o = (int*)dst + 1;
        for (int i = 0; i < n; ++i) o[i] = (o[i] / P.LW) * P.LWt + o[i] % P.LW;
      }
      return PLI_OK;
    }
    case PLI_DBG_LBD_DXDY: {
      const int64_t n = (int64_t)P.W * P.H * 2;
      if (!need(2 * n)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      // device layout: interleaved (dx, dy) pairs; the caller gets the dx plane followed by the dy plane
      std::vector<short> tmp((size_t)P.W * P.H * 2);
      HIPCHK(hipMemcpy(tmp.data(), c->dxy + (int64_t)image * P.W * P.H, 2 * n, hipMemcpyDeviceToHost));
      short* o = (short*)dst;
      for (int64_t i = 0; i < (int64_t)P.W * P.H; ++i) { o[i] = tmp[2 * i]; o[(int64_t)P.W * P.H + i] = tmp[2 * i + 1]; }
      return PLI_OK;
    }
    case PLI_DBG_LBD_FLOAT: {
      if (!c->lbdFloat) { g_err = "pli_debug_enable was not on during the run"; return PLI_ERR_STATE; }
      const int64_t n = (int64_t)P.klCap * 72 * 4;
      if (!need(n)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      HIPCHK(hipMemcpy(dst, c->lbdFloat + (int64_t)image * P.klCap * 72, n, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_LSD_OWNER: {
      const int64_t np = (int64_t)P.LW * P.LH;
      if (!need(4 + (int64_t)P.LWt * P.LH * 4)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      RxCtl ctl;
      HIPCHK(hipMemcpy(&ctl, c->jrCtl + image, sizeof(ctl), hipMemcpyDeviceToHost));
      std::vector<int2> own(np);
      HIPCHK(hipMemcpy(own.data(), c->own + image * np, np * 8, hipMemcpyDeviceToHost));
      int* o = (int*)dst;
      o[0] = ctl.rounds;
      const int comp = (ctl.rounds - 1) & 1;          // owner_{t-1} of the round that detected the fixed point
      for (int y = 0; y < P.LH; ++y)
        for (int x = 0; x < P.LWt; ++x) { const int2 w = own[(int64_t)y * P.LW + x]; o[1 + (int64_t)y * P.LWt + x] = comp ? w.y : w.x; }
      return PLI_OK;
    }
    case 15: {   // debug: raw owner pairs
      const int64_t np = (int64_t)P.LW * P.LH;
      if (!need(np * 8)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      HIPCHK(hipMemcpy(dst, c->own + image * np, np * 8, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case 14: {   // debug: captured queue of PLI_DBG_RANK (dev aid)
      if (!need(4096 * 4)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      HIPCHK(hipMemcpy(dst, c->regScratch, 4096 * 4, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_LSD_SIZES: {
      const int64_t np = (int64_t)P.LW * P.LH;
      if (!need(np * 4)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      HIPCHK(hipMemcpy(dst, c->lastSize + image * np, np * 4, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    case PLI_DBG_STEREO_SAD: {
      const int frame = image >> 1;
      const int64_t n = (int64_t)P.kpCap * 4;
      if (!need(2 * n)) return dst ? PLI_ERR_CAPACITY : PLI_OK;
      HIPCHK(hipMemcpy(dst, c->sad + (int64_t)frame * P.kpCap, n, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy((char*)dst + n, c->bestIdx + (int64_t)frame * P.kpCap, n, hipMemcpyDeviceToHost));
      return PLI_OK;
    }
    default:
      g_err = "unknown debug item";
      return PLI_ERR_INVALID;
  }
}

}  // extern "C"

#ifdef PLI_DEV
// development build: the reach k_describe's window is sized for (kernels.hpp, ORB_REACH), for the test that recomputes it from the pattern
extern "C" int32_t pli_dev_orb_window_reach(void) { return ORB_REACH; }
#endif
