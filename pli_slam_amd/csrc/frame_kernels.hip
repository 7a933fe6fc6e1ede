// The undistortion family of the single-camera Frame constructors (Frame.cc:231-331 RGB-D, :334-448 monocular) for a pinhole camera
// with distortion coefficients: UndistortKeyPoints (:872-905), UndistortKeyLines (:907-945), ComputeImageBounds (:947-974),
// ComputeStereoFromRGBD (:1309-1330) and PosInGrid (:845-855) as AssignFeaturesToGrid (:451-482) calls it on mvKeysUn.
//
// undistort_point is the ONLY statement of the arithmetic: OpenCV 3.3.1's cvUndistortPoints (imgproc/src/undistort.cpp) for CV_32FC2
// points with no R, P = K and no tilt — five fixed-point steps without a convergence test, all in double, K and the coefficients
// converted from float, one rounding to float at the end.  Every expression is kept whole and in the source's association, the terms
// of the absent coefficients k[5..11] = 0 included: a non-finite intermediate then propagates as it does there (0 * inf is NaN, not 0).
// The library is built with -ffp-contract=off and the double division is the correctly rounded one.  (Later OpenCV versions leave the
// loop on an epsilon: a different function.)  Parity with a real OpenCV is unpinned; tests/helpers_undistort.py restates
// the same text in float64 numpy and the GPU tests compare byte for byte.
//
// The kernels are element-wise and small: one thread per point, nothing shared, no tuning.
#include "kernels.hpp"

namespace pli {

namespace {

__device__ __forceinline__ float2 undistort_point(const PinholeUndist& C, float px, float py) {
  if (!C.on) return make_float2(px, py);          // the reference's gate (Frame.cc:874, :909, :949): k1 == 0 -> a copy
  const double fx = C.cam.fx, fy = C.cam.fy, cx = C.cam.cx, cy = C.cam.cy;
  const double k[12] = {C.cam.k1, C.cam.k2, C.cam.p1, C.cam.p2, C.cam.k3, 0., 0., 0., 0., 0., 0., 0.};
  const double ifx = 1. / fx, ify = 1. / fy;
  // RR = K . I (cvMatMul in double: the products with the identity's ones and zeros are exact)
  const double RR[3][3] = {{fx, 0., cx}, {0., fy, cy}, {0., 0., 1.}};
  double x = px, y = py;
  x = (x - cx) * ifx;
  y = (y - cy) * ify;
  const double x0 = x, y0 = y;
  for (int j = 0; j < 5; ++j) {
    const double r2 = x * x + y * y;
    const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
    const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
    const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  const double xx = RR[0][0] * x + RR[0][1] * y + RR[0][2];
  const double yy = RR[1][0] * x + RR[1][1] * y + RR[1][2];
  const double ww = 1. / (RR[2][0] * x + RR[2][1] * y + RR[2][2]);
  return make_float2((float)(xx * ww), (float)(yy * ww));
}

// Frame::PosInGrid (Frame.cc:845-855) against the bounds of C: posX * FRAME_GRID_ROWS + posY, or -1 where it returns false.  round()
// is on a float argument; the range test is made on the rounded float, before the conversion to int: the reference's answer
// wherever that conversion is defined, and false where it is not (a NaN or a value no int holds).
__device__ __forceinline__ int grid_cell(const PinholeUndist& C, float2 p) {
  const float winv = __fdiv_rn(64.f, __fsub_rn(C.maxX, C.minX));      // mfGridElementWidthInv (:297, :402)
  const float hinv = __fdiv_rn(48.f, __fsub_rn(C.maxY, C.minY));
  const float fxp = roundf(__fmul_rn(__fsub_rn(p.x, C.minX), winv));
  const float fyp = roundf(__fmul_rn(__fsub_rn(p.y, C.minY), hinv));
  if (!(fxp >= 0.f && fxp < 64.f && fyp >= 0.f && fyp < 48.f)) return -1;
  return (int)fxp * 48 + (int)fyp;
}

}  // namespace

// pli_undistort_points: n caller points; cell may be null.  (pli_set_pinhole_distortion sends the four image corners through it.)
__global__ void k_undistort_points(PinholeUndist C, const float2* __restrict__ xy, int n, float2* __restrict__ xyUn, int* __restrict__ cell) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float2 p = xy[i];
  const float2 u = undistort_point(C, p.x, p.y);
  xyUn[i] = u;
  if (cell) cell[i] = grid_cell(C, u);
}

// The tail of pli_frame_extract_single, one launch behind the joined chains: thread t < kpCap owns keypoint row t of eye 0, thread
// kpCap + j keyline row j; the counts come from the record, as k_stereo_from_depth reads them.
//   keypoint i < N:  kpUn[i] = the undistorted position, cell[i] = its grid cell; with a depth image ComputeStereoFromRGBD — d at
//                    (int)v, (int)u of the DISTORTED keypoint, mvuRight = kpU.x - bf / d in float (k_stereo_from_depth's in-image guard
//                    kept: the reference's read outside the image is undefined) —, without one mvuRight = mvDepth = -1 (:384-385);
//                    the image is the caller's raw one, d = depth_value (kernels.hpp) of the element read
//   keyline j < M:   klUn[j] = (startPoint, endPoint) of mvKeys_Line[j], each undistorted
// Rows from the count on: kpUn / klUn 0, cell / mvuRight / mvDepth -1, so the caller's buffers and those two columns do not depend on
// an earlier call.
__global__ void k_frame_single_tail(const DevParams* __restrict__ Pp, PinholeUndist C, const void* __restrict__ depthImg, DepthFormat fmt, int64_t pitch,
                                    uint8_t* __restrict__ table, int64_t offCounts, int64_t offKp0, int64_t offKl0, int64_t offUr,
                                    int64_t offDepth, float2* __restrict__ kpUn, int* __restrict__ cell, float4* __restrict__ klUn) {
  const DevParams& P = *Pp;
  const int* counts = reinterpret_cast<const int*>(table + offCounts);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < P.kpCap) {
    const int N = min(counts[0], P.kpCap);
    float2 u = make_float2(0.f, 0.f);
    int cl = -1;
    float ur = -1.f, dp = -1.f;
    if (t < N) {
      const pli_keypoint kp = reinterpret_cast<const pli_keypoint*>(table + offKp0)[t];
      u = undistort_point(C, kp.x, kp.y);
      cl = grid_cell(C, u);
      if (depthImg) {
        const int iu = (int)kp.x, iv = (int)kp.y;
        if (iu >= 0 && iv >= 0 && iu < P.W && iv < P.H) {
          const float d = depth_value(depthImg, fmt, (int64_t)iv * pitch + iu);
          if (d > 0) { dp = d; ur = __fsub_rn(u.x, __fdiv_rn(P.bf, d)); }
        }
      }
    }
    kpUn[t] = u;
    cell[t] = cl;
    reinterpret_cast<float*>(table + offUr)[t] = ur;
    reinterpret_cast<float*>(table + offDepth)[t] = dp;
    return;
  }
  const int j = t - P.kpCap;
  if (j >= P.klCap) return;
  const int M = min(counts[2], P.klCap);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j < M) {
    const pli_keyline& kl = reinterpret_cast<const pli_keyline*>(table + offKl0)[j];
    const float2 s = undistort_point(C, kl.startPointX, kl.startPointY);
    const float2 e = undistort_point(C, kl.endPointX, kl.endPointY);
    o = make_float4(s.x, s.y, e.x, e.y);
  }
  klUn[j] = o;
}

}  // namespace pli
