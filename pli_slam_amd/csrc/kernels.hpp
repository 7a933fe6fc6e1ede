// Kernel prototypes (definitions in orb_kernels.hip, line_kernels.hip, match_kernels.hip, kfdb_kernels.hip, mapfeat_kernels.hip, frame_kernels.hip).
// Started from tools/gen_kernel_protos.py; kept by hand since (the octree instances come from a macro the script does not see; the
// script writes a templated kernel's prototype as the ones below are written).
#pragma once
#include "common.hpp"

namespace pli {

struct BlurPlane {
  int w, h, pitchIn, pitchOut;
  int64_t offIn, offOut;
  int tilesX, tileBase;
};
struct BlurJob {
  int nplanes;
  BlurPlane pl[MAX_LEVELS];
  int k[7];
  int radius;
};
struct LbdCoef { float L[21]; float G[63]; };

// The depth image of ComputeStereoFromRGBD as the caller holds it (pli_set_depth_format), by value to its two kernels: the
// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) of Tracking.cc:979-980 is made at the keypoint, on the one element read.
struct DepthFormat {
  int u16;        // elements are uint16_t (PLI_DEPTH_U16), otherwise float
  float scale;
};
// element i of the image as ComputeStereoFromRGBD sees it: cvtScale16u32f with shift 0 is (float)raw * scale in float, one rounding
// (every uint16 is exact in float); a float element times 1.0f keeps its bits without the multiplication (a signalling NaN too)
__device__ __forceinline__ float depth_value(const void* __restrict__ img, DepthFormat f, int64_t i) {
  if (f.u16) return __fmul_rn((float)static_cast<const uint16_t*>(img)[i], f.scale);
  const float d = static_cast<const float*>(img)[i];
  return f.scale == 1.0f ? d : __fmul_rn(d, f.scale);
}

// k_describe blurs the window of its keypoint itself (orb_kernels.hip).  The window follows from the test pattern: a tap (x, y) is
// rotated by the keypoint angle and each coordinate rounded, so no coordinate leaves [-n, n] for the smallest n with
// n + 0.5 > |(x, y)| * (1 + 1e-4) (the factor covers the float cos/sin and the roundings of the products).
constexpr signed char ORB_PATTERN_HOST[1024] = {
#include "../../include/pli_orb_pattern.inc"
};
constexpr int orbPatternReach() {
  int best = 0;
  for (int i = 0; i < 512; ++i) {
    const long long x = ORB_PATTERN_HOST[2 * i], y = ORB_PATTERN_HOST[2 * i + 1], r2 = x * x + y * y;
    int n = 0;
    while ((long long)(2 * n + 1) * (2 * n + 1) * 10000 <= 4 * r2 * 10002) ++n;       // (2n + 1)^2 > 4 r^2 (1 + 1e-4)^2
    best = n > best ? n : best;
  }
  return best;
}
constexpr int ORB_REACH = orbPatternReach();     // 18 for the published pattern
constexpr int ORB_BLUR_R = 3;                    // GaussianBlur 7x7 (jobOrb)
constexpr int ORB_HALF_PATCH = 15;               // IC_Angle's disc
constexpr int LBD_BLUR_R = 2;                    // GaussianBlur 5x5 (jobLbd); k_sobel's tile has a halo of LBD_BLUR_R + 1
// projection searches (match_kernels.hip: k_proj_*, k_track_*): candidate keys kept per query, the stride of the hosts' key buffers;
// a query with more is rescanned in phase 2
constexpr int PROJ_K = 64;
__global__ void k_ingest_copy16(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right, int64_t stride, int64_t frameStride, uint8_t* __restrict__ pyr, int64_t pyrBlock, int W16, int H, int pitch, int img0);
__global__ void k_ingest(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right, int64_t stride, int64_t frameStride, uint8_t* __restrict__ pyr, int64_t pyrBlock, int W, int H, int pitch, const float2* __restrict__ mapL, const float2* __restrict__ mapR, int img0);
template <int CH> __global__ void k_ingest_colour(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right, int64_t stride, int64_t frameStride, uint8_t* __restrict__ pyr, int64_t pyrBlock, int W, int H, int pitch, const float2* __restrict__ mapL, const float2* __restrict__ mapR, int img0, int c0, int c2);
__global__ void k_resize_level(const uint8_t* __restrict__ srcBase, int64_t srcImgStride, int sw, int sh, int spitch, uint8_t* __restrict__ dstBase, int64_t dstImgStride, int dw, int dh, int dpitch, const int* __restrict__ tab, int img0);
__global__ void k_fast_cells(const DevParams* __restrict__ Pp, const uint8_t* __restrict__ pyr, uint32_t* __restrict__ cellCand, int* __restrict__ cellCount, int img0);
__global__ void k_octree(const DevParams* __restrict__ Pp, const uint32_t* __restrict__ cellCand, const int* __restrict__ cellCount, uint32_t* __restrict__ candAll, unsigned short* __restrict__ nodeOfAll, int* __restrict__ candCount, uint32_t* __restrict__ kpSel, int* __restrict__ kpSelCount, int img0);
__global__ void k_octree_512(const DevParams* __restrict__ Pp, const uint32_t* __restrict__ cellCand, const int* __restrict__ cellCount, uint32_t* __restrict__ candAll, unsigned short* __restrict__ nodeOfAll, int* __restrict__ candCount, uint32_t* __restrict__ kpSel, int* __restrict__ kpSelCount, int img0);
__global__ void k_octree_320(const DevParams* __restrict__ Pp, const uint32_t* __restrict__ cellCand, const int* __restrict__ cellCount, uint32_t* __restrict__ candAll, unsigned short* __restrict__ nodeOfAll, int* __restrict__ candCount, uint32_t* __restrict__ kpSel, int* __restrict__ kpSelCount, int img0);
__global__ void k_octree_w(const DevParams* __restrict__ Pp, const uint32_t* __restrict__ cellCand, const int* __restrict__ cellCount, uint32_t* __restrict__ candAll, unsigned short* __restrict__ nodeOfAll, int* __restrict__ candCount, uint32_t* __restrict__ kpSel, int* __restrict__ kpSelCount, int img0);
__global__ void k_octree_512_w(const DevParams* __restrict__ Pp, const uint32_t* __restrict__ cellCand, const int* __restrict__ cellCount, uint32_t* __restrict__ candAll, unsigned short* __restrict__ nodeOfAll, int* __restrict__ candCount, uint32_t* __restrict__ kpSel, int* __restrict__ kpSelCount, int img0);
__global__ void k_octree_320_w(const DevParams* __restrict__ Pp, const uint32_t* __restrict__ cellCand, const int* __restrict__ cellCount, uint32_t* __restrict__ candAll, unsigned short* __restrict__ nodeOfAll, int* __restrict__ candCount, uint32_t* __restrict__ kpSel, int* __restrict__ kpSelCount, int img0);
__global__ void k_blur(const BlurJob* __restrict__ Jp, const uint8_t* __restrict__ in, int64_t inImgStride, uint8_t* __restrict__ out, int64_t outImgStride, int img0);
__global__ void k_describe(const DevParams* __restrict__ Pp, const uint8_t* __restrict__ pyr, const BlurJob* __restrict__ Jp, const uint32_t* __restrict__ kpSel, const int* __restrict__ kpSelCount, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int64_t offKp0, int64_t offKp1, int64_t offDesc0, int64_t offDesc1, int img0);
__global__ void k_kp_counts(const DevParams* __restrict__ Pp, const int* __restrict__ kpSelCount, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int nimg, int img0);
__global__ void k_lsd_grad(const uint8_t* __restrict__ scaled, int64_t imgStride, int W, int H, int WP, int pitch, int g2Thresh, float4* __restrict__ rec, int* __restrict__ g2o, int2* __restrict__ own, int* __restrict__ maxG2, float* __restrict__ angDbg, int img0, int trigF32);
__global__ void k_lsd_hist(const int* __restrict__ g2a, int npix, int g2Thresh, int nBins, const int* __restrict__ maxG2, unsigned short* __restrict__ chunkHist, int nChunks, int img0, const double* __restrict__ mgAll, const unsigned long long* __restrict__ maxMg, double rho, const RxCtl* __restrict__ onlyUnsettled);
__global__ void k_lsd_scan(const unsigned short* __restrict__ chunkHist, int nChunks, int nBins, int* __restrict__ chunkBase, int* __restrict__ nDefined, int img0, const RxCtl* __restrict__ onlyUnsettled);
__global__ void k_lsd_scatter(const int* __restrict__ g2a, int npix, int g2Thresh, int nBins, const int* __restrict__ maxG2, const int* __restrict__ chunkBase, int nChunks, int* __restrict__ order, int img0, int nimg, const double* __restrict__ mgAll, const unsigned long long* __restrict__ maxMg, double rho, int* __restrict__ rankAll, const int* __restrict__ groupOff, int chunksPerGroup, int nGroups, const RxCtl* __restrict__ onlyUnsettled);
__global__ void k_lsd_scan_part(const unsigned short* __restrict__ chunkHist, int nChunks, int nBins, int chunksPerGroup, int* __restrict__ chunkBase, int* __restrict__ groupOff, int img0, const RxCtl* __restrict__ onlyUnsettled);
__global__ void k_lsd_scan_groups(int nGroups, int nBins, int* __restrict__ groupOff, int* __restrict__ nDefined, int img0, const RxCtl* __restrict__ onlyUnsettled);
__global__ void k_lsd_grow_unsettled(const DevParams* __restrict__ Pp, float4* __restrict__ recAll, const double* __restrict__ mgAll, const int* __restrict__ orderAll, const int* __restrict__ nDefined, uint2* __restrict__ regOverflow, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, int nimg, RxCtl* __restrict__ ctl);
__global__ void k_lsd_grow(const DevParams* __restrict__ Pp, float4* __restrict__ recAll, const double* __restrict__ mgAll, const int* __restrict__ orderAll, const int* __restrict__ nDefined, uint2* __restrict__ regOverflow, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, int nimg);
__global__ void k_lsd_grow2(const DevParams* __restrict__ Pp, float4* __restrict__ recAll, const double* __restrict__ mgAll, const int* __restrict__ orderAll, const int* __restrict__ nDefined, uint2* __restrict__ regOverflow, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, int nimg);
__global__ void k_lsd_grow_spec(const DevParams* __restrict__ Pp, float4* __restrict__ recAll, const double* __restrict__ mgAll, const int* __restrict__ orderAll, const int* __restrict__ nDefined, uint2* __restrict__ regOverflow, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, int nimg, LsdRectItem* __restrict__ rectAll, double* __restrict__ rectWAll);
__global__ void k_lsd_grow2_spec(const DevParams* __restrict__ Pp, float4* __restrict__ recAll, const double* __restrict__ mgAll, const int* __restrict__ orderAll, const int* __restrict__ nDefined, uint2* __restrict__ regOverflow, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, int nimg, LsdRectItem* __restrict__ rectAll, double* __restrict__ rectWAll);
__global__ void k_lsd_rect(const DevParams* __restrict__ Pp, const LsdRectItem* __restrict__ rectAll, const uint2* __restrict__ arenaAll, const double* __restrict__ mgAll, const double* __restrict__ rectWAll, const int* __restrict__ nSeg, float* __restrict__ segAll, int maxSeg, int img0);
__global__ void k_keylines(const DevParams* __restrict__ Pp, const float* __restrict__ seg, const int* __restrict__ nSeg, int maxSeg, pli_keyline* __restrict__ tmpKL, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int64_t offKl0, int64_t offKl1, int img0);
__global__ void k_sobel(const BlurJob* __restrict__ Jp, const uint8_t* __restrict__ in, int64_t inImgStride, short2* __restrict__ dxy, int img0);
__global__ void k_lbd(const DevParams* __restrict__ Pp, const LbdCoef* __restrict__ coef, const short2* __restrict__ dxya, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int64_t offKl0, int64_t offKl1, int64_t offLd0, int64_t offLd1, float* __restrict__ dbgFloat, int img0);
__global__ void k_lsd_blur64(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int W, int H, int pitch, const double* __restrict__ kern, int radius, double* __restrict__ out, int64_t outImgStride, int img0);
__global__ void k_lsd_resize64(const double* __restrict__ src, int sw, int sh, double* __restrict__ dst, int dw, int dh, int64_t dstImgStride, const int* __restrict__ tab, int img0);
__global__ void k_lsd_grad64(const double* __restrict__ scaled, int W, int H, int WP, int64_t scaledImgStride, double rho, LsdFrontPlanes P, unsigned long long* __restrict__ maxMg, float* __restrict__ angDbg, int img0, int trigF32);
__global__ void k_lsd_front64(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int sw, int sh, int pitch, const double* __restrict__ kern, int radius, const int* __restrict__ tab, int dw, int dh, int dp, double rho, LsdFrontPlanes P, unsigned long long* __restrict__ maxMg, int img0, int trigF32);
constexpr int LSD_FRONT_STREAM_WAVES = 4;      // strips of 64 scaled columns per 256-thread workgroup of k_lsd_front64s
__global__ void k_lsd_front64s(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int sw, int sh, int pitch, const double* __restrict__ kern, const int* __restrict__ tab, int dw, int dh, int dp, double rho, LsdFrontPlanes P, unsigned long long* __restrict__ maxMg, int img0, int trigF32, int chunk);
__global__ void k_count_diff_words(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int64_t n, unsigned* __restrict__ count);
__global__ void k_rx_guess(const float4* __restrict__ recAll, const int* __restrict__ rankAll, int2* __restrict__ ownAll, int W, int H, float precDeg, int img0);
__global__ void k_rx_diff(RxCtl* __restrict__ ctl, const int2* __restrict__ ownAll, int* __restrict__ tileMinAll, int* __restrict__ tileActAll, int W, int H, int TW, int TH, int t, int img0, const int* __restrict__ tileTouchAll);
__global__ void k_rx_classify(RxCtl* __restrict__ ctl, const int2* __restrict__ ownAll, const int* __restrict__ rankAll, const int2* __restrict__ rgBoxAll, uint8_t* __restrict__ rgCleanAll, const int* __restrict__ tileMinAll, int W, int H, int TW, int TH, int t, int img0);
__global__ void k_rx_seed(RxCtl* __restrict__ ctl, int2* __restrict__ ownAll, const int* __restrict__ rankAll, const float4* __restrict__ recAll, const int* __restrict__ rgSizeAll, const uint8_t* __restrict__ rgCleanAll, RxSeed* __restrict__ smallAll, RxSeed* __restrict__ bigAll, int bigCap, int W, int H, int bigThresh, int t, int img0);
__global__ void k_rx_mark(RxCtl* __restrict__ ctl, const int2* __restrict__ ownAll, const int* __restrict__ rankAll, const int2* __restrict__ rgBoxAll, int* __restrict__ rgDirtyAll, const int* __restrict__ tileMinAll, int* __restrict__ tileActAll, int W, int H, int TW, int TH, int t, int img0, int seedRule, const int* __restrict__ rgLostAll, TxDirtyLists DL);
__global__ void k_rx_seed_sparse(RxCtl* __restrict__ ctl, int2* __restrict__ ownAll, const int* __restrict__ rankAll, const float4* __restrict__ recAll, const int* __restrict__ rgSizeAll, const int* __restrict__ rgDirtyAll, const int* __restrict__ tileActAll, RxSeed* __restrict__ smallAll, RxSeed* __restrict__ bigAll, int bigCap, int W, int H, int TW, int TH, int bigThresh, int t, int img0);
__global__ void k_rx_grow(const DevParams* __restrict__ Pp, RxCtl* __restrict__ ctl, const float4* __restrict__ recAll, int2* __restrict__ ownAll, const RxSeed* __restrict__ smallAll, int* __restrict__ rgSizeAll, int2* __restrict__ rgBoxAll, RxHand* __restrict__ handAll, int handCap, int* __restrict__ arenaAll, int arenaCap, RxRect* __restrict__ rectAll, int rectCap, int img0, int t);
__global__ void k_rx_grow_big(const DevParams* __restrict__ Pp, RxCtl* __restrict__ ctl, const float4* __restrict__ recAll, int2* __restrict__ ownAll, const RxSeed* __restrict__ bigAll, int bigCap, const RxHand* __restrict__ handAll, int handCap, int* __restrict__ rgSizeAll, int2* __restrict__ rgBoxAll, int* __restrict__ arenaAll, int arenaCap, RxRect* __restrict__ rectAll, int rectCap, int img0, int t);
__global__ void k_rx_grow_wave(const DevParams* __restrict__ Pp, RxCtl* __restrict__ ctl, const float4* __restrict__ recAll, int2* __restrict__ ownAll, const RxSeed* __restrict__ bigAll, int bigCap, const RxHand* __restrict__ handAll, int handCap, int* __restrict__ rgSizeAll, int2* __restrict__ rgBoxAll, int* __restrict__ arenaAll, int arenaCap, RxRect* __restrict__ rectAll, int rectCap, int img0, int t);
__global__ void k_rx_rect(const DevParams* __restrict__ Pp, RxCtl* __restrict__ ctl, const float4* __restrict__ recAll, const int* __restrict__ arenaAll, int arenaCap, const RxRect* __restrict__ rectAll, int rectCap, float4* __restrict__ rgSegAll, int img0, const double* __restrict__ mgAll, int rmask, const int2* __restrict__ hotAll, const float2* __restrict__ coldAll);
__global__ void k_rx_count(const RxCtl* __restrict__ ctl, const int* __restrict__ orderAll, const int* __restrict__ nDefined, const int2* __restrict__ ownAll, const int* __restrict__ rgSizeAll, int* __restrict__ chunkCntAll, int nChunks, int64_t npix, int minReg, int img0, const int2* __restrict__ rgBoxAll, int boxCut);
__global__ void k_rx_emit(const RxCtl* __restrict__ ctl, const int* __restrict__ orderAll, const int* __restrict__ nDefined, const int2* __restrict__ ownAll, const int* __restrict__ rgSizeAll, const float4* __restrict__ rgSegAll, const int* __restrict__ chunkCntAll, int nChunks, int64_t npix, int minReg, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, const int2* __restrict__ rgBoxAll, int boxCut);
__global__ void k_tx_sort(const int* __restrict__ rankAll, const int* __restrict__ orderAll, int2* __restrict__ ownAll, int2* __restrict__ listAll, int* __restrict__ tileCntAll, int W, int H, int ts, int ntx, int nty, int img0, TxKeys keys);
__global__ void k_tx_sort128(const int* __restrict__ rankAll, const int* __restrict__ orderAll, int2* __restrict__ ownAll, int2* __restrict__ listAll, int* __restrict__ tileCntAll, int W, int H, int ts, int ntx, int nty, int img0, TxKeys keys);
__global__ void k_tx_mark(TxRound A, int t, const int* __restrict__ tileMinAll);
__global__ void k_tx_round2(TxRound A, int t, const float4* __restrict__ recPack, int keepRect);
__global__ void k_tx_reset_rect(RxCtl* __restrict__ ctl, int nimg, int img0);
__global__ void k_tx_diffmark(TxRound A, int t);
__global__ void k_tx_diff2(TxRound A, int t, int* __restrict__ tileMinAll);
__global__ void k_tx_prep(TxRound A, int t, int full);
__global__ void k_tx_grow(TxRound A, int t);
__global__ void k_tx_grow_p1(TxRound A, int t, TxKeys keys);
__global__ void k_tx_grow_p2(TxRound A, int t, TxKeys keys);
__global__ void k_tx_grow_h1(const DevParams* __restrict__ Pp, RxCtl* __restrict__ ctl, const float4* __restrict__ recAll, int2* __restrict__ ownAll, const int2* __restrict__ listAll, const int* __restrict__ tileCntAll, int ts, int ntx, int nty, int* __restrict__ rgSizeAll, int2* __restrict__ rgBoxAll, const int* __restrict__ rgDirtyAll, const int* __restrict__ tileActAll, int TW, int TH, int* __restrict__ arenaAll, int arenaCap, RxRect* __restrict__ rectAll, int rectCap, int img0, int t, const int* __restrict__ rankAll, int* __restrict__ rgLostAll, int* __restrict__ tileTouchAll, TxDirtyLists DL, TxKeys keys);
__global__ void k_tx_grow_h2(TxRound A, int t, TxKeys keys);
__global__ void k_tx_grow_spec(TxRound A, int t);
__global__ void k_tx_grow_sparse(TxRound A, int t);
__global__ void k_tx_grow_sparse_h(TxRound A, int t);
__global__ void k_stereo_points(const DevParams* __restrict__ Pp, const uint8_t* __restrict__ pyr, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int64_t offKp0, int64_t offKp1, int64_t offDesc0, int64_t offDesc1, int64_t offUr, int64_t offDepth, int* __restrict__ sadOut, int* __restrict__ bestIdxOut);
__global__ void k_stereo_median(const DevParams* __restrict__ Pp, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int64_t offUr, int64_t offDepth, const int* __restrict__ sadIn);
__global__ void k_stereo_lines(const DevParams* __restrict__ Pp, uint8_t* __restrict__ table, int64_t recordBytes, int64_t offCounts, int64_t offKl0, int64_t offKl1, int64_t offLd0, int64_t offLd1, int64_t offDisp, int64_t offLe, unsigned long long* __restrict__ maskAll, double* __restrict__ dirAll, short* __restrict__ dmatAll, int* __restrict__ m12All, int* __restrict__ m21All, int phase);
__global__ void k_distance(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int n, int* __restrict__ out);
__global__ void k_knn2(const uint8_t* __restrict__ q, int nq, const uint8_t* __restrict__ t, int nt, int* __restrict__ idx, int* __restrict__ dist);
__global__ void k_ratio(const int* __restrict__ idx, const int* __restrict__ dist, int n, int nTrain, float nnr, int* __restrict__ m);
__global__ void k_mutual(int* __restrict__ m12, const int* __restrict__ m21, int n1, int* __restrict__ nmatches);
__global__ void k_stereo_from_depth(const DevParams* __restrict__ Pp, const void* __restrict__ depthImg, DepthFormat fmt, int64_t pitch, int W, int H, uint8_t* __restrict__ table, int64_t offCounts, int64_t offKp0, int64_t offUr, int64_t offDepth);
__global__ void k_proj_candidates(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq, const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const float* __restrict__ uright, int ncur, float minX, float maxX, float minY, float maxY, int checkBounds, int distLimit, unsigned long long* __restrict__ candKeys, int* __restrict__ candCount);
__global__ void k_proj_assign(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq, const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const float* __restrict__ uright, const uint8_t* __restrict__ occupied, int ncur, float minX, float maxX, float minY, float maxY, int mode, int checkOri, float nnratio, const unsigned long long* __restrict__ candKeys, const int* __restrict__ candCount, int* __restrict__ bestIdx2, int* __restrict__ nmatchesOut, int* __restrict__ rawIdx2);
__global__ void k_proj_assign_scan(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq, const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc, const float* __restrict__ uright, const uint8_t* __restrict__ occupied, int ncur, float minX, float maxX, float minY, float maxY, int mode, int checkOri, float nnratio, int* __restrict__ owner /* ncur */, int* __restrict__ bestIdx2, int* __restrict__ nmatchesOut, int* __restrict__ rawIdx2);
__global__ void k_track_queries(const DevParams* __restrict__ Pp, const uint8_t* __restrict__ table, const float* __restrict__ poses, TrackParams tp, pli_proj_query* __restrict__ qAll);
__global__ void k_track_candidates(const uint8_t* __restrict__ table, TrackParams tp, const pli_proj_query* __restrict__ qAll, unsigned long long* __restrict__ candKeysAll, int* __restrict__ candCountAll);
__global__ void k_track_assign(const uint8_t* __restrict__ table, TrackParams tp, const pli_proj_query* __restrict__ qAll, const unsigned long long* __restrict__ candKeysAll, const int* __restrict__ candCountAll, uint8_t* __restrict__ track);
__global__ void k_track_lines(const uint8_t* __restrict__ table, TrackParams tp, int bestLR, int* __restrict__ scratch, uint8_t* __restrict__ track);
__global__ void k_bow_descend(const uint8_t* __restrict__ feat, int n, const int* __restrict__ childOff, const int* __restrict__ childList, const uint8_t* __restrict__ nodeDesc, const int* __restrict__ nodeWord, const double* __restrict__ nodeWeight, int nidLevel, int* __restrict__ wordId, double* __restrict__ weight, int* __restrict__ nodeId);
__global__ void k_node_sort(const int* __restrict__ kfOff, int nkOne, const int* __restrict__ kfNode, const uint8_t* __restrict__ kfFlag, int flagWanted, const uint8_t* __restrict__ kfStereo, int onlyStereo, int keyCap, uint32_t* __restrict__ sNode, uint16_t* __restrict__ sIdx, int* __restrict__ nListed, int* __restrict__ stat);
__global__ void k_search_by_bow(const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc, const float* __restrict__ kfAngle, const int* __restrict__ kfNode, const uint8_t* __restrict__ kfValid, const uint8_t* __restrict__ fDesc, const float* __restrict__ fAngle, const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, int nf, int keyCap, float nnratio, int checkOri, int* __restrict__ matches, int* __restrict__ nmatchesOut);
__global__ void k_search_by_bow_two_cameras(const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc, const float* __restrict__ kfAngle, const int* __restrict__ kfNode, const uint8_t* __restrict__ kfValid, const uint8_t* __restrict__ fDesc, const float* __restrict__ fAngle, const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, int nf, int fNleft, int keyCap, float nnratio, int checkOri, int* __restrict__ matches, int* __restrict__ nmatchesOut);
__global__ void k_tri_match(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1, const int* __restrict__ node1, const uint8_t* __restrict__ hasMp1, const uint8_t* __restrict__ stereo1, int n1, const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc, const uint8_t* __restrict__ kfStereo, const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, const float* __restrict__ F12, const float* __restrict__ ep, const float* __restrict__ scaleFactor, const float* __restrict__ sigma2, int onlyStereo, int coarse, int checkOri, int* __restrict__ matches12, int* __restrict__ stat);
__global__ void k_tri_finish(const pli_keypoint* __restrict__ kp1, int n1, const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp, int* __restrict__ matches12, int* __restrict__ stat);
__global__ void k_kb8_rays(const pli_keypoint* __restrict__ kp1, int n1, int n1Left, const pli_keypoint* __restrict__ kfKp, const int* __restrict__ kfOff, const int* __restrict__ kfNleft, int nkf, Kb8 camL, Kb8 camR, float2* __restrict__ ray1, float2* __restrict__ kfRay);
__global__ void k_tri_match_kb8(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1, const int* __restrict__ node1, const uint8_t* __restrict__ hasMp1, const float2* __restrict__ ray1, int n1, int n1Left, const int* __restrict__ kfOff, const int* __restrict__ kfNleft, const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc, const float2* __restrict__ kfRay, const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, const float* __restrict__ rel, Kb8 camL, Kb8 camR, const float* __restrict__ sigma2, int coarse, int checkOri, int* __restrict__ matches12, int* __restrict__ stat);
// the per-feature tables of pli_create_new_map_points beyond the search's: mvuRight, mvDepth, mvKeys[i].pt, the 15-float poses
struct NewPtTables {
  const pli_keypoint* kp1; const float* ur1; const float* depth1; const float2* key1; const float* pose1; int n1;
  const int* kfOff; const pli_keypoint* kfKp; const float* kfUr; const float* kfDepth; const float2* kfKey; const float* kfPose;
  const float* scaleFactor; const float* sigma2;
};
__global__ void k_newpt_list(const int* __restrict__ matches12, int npairs, int* __restrict__ list, int* __restrict__ nListed, int* __restrict__ status, float* __restrict__ x3d);
__global__ void k_newpt_geometry(NewPtTables D, pli_fuse_camera cam, float mb, int farPoints, float thFar, float ratioFactor, const int* __restrict__ matches12, const int* __restrict__ list, const int* __restrict__ nListed, int* __restrict__ status, float* __restrict__ x3d);
// the tables of pli_create_new_map_points_two_cameras: mvKeys then mvKeysRight per keyframe, the rays of k_kb8_rays, 2 x 15 floats of
// pose per keyframe (left, then right)
struct NewPtKb8Tables {
  const pli_keypoint* kp1; const float2* ray1; const float* pose1; int n1, n1Left;
  const int* kfOff; const int* kfNleft; const pli_keypoint* kfKp; const float2* kfRay; const float* kfPose;
  const float* scaleFactor; const float* sigma2;
};
__global__ void k_newpt_geometry_kb8(NewPtKb8Tables D, Kb8 camL, Kb8 camR, int farPoints, float thFar, float ratioFactor, const int* __restrict__ matches12, const int* __restrict__ list, const int* __restrict__ nListed, int* __restrict__ status, float* __restrict__ x3d);
__global__ void k_newpt_pick(int n1, int nkf, int* __restrict__ matches12, int* __restrict__ status, int* __restrict__ nmatches, int* __restrict__ nnew);
__global__ void k_search_by_bow_kf(const uint8_t* __restrict__ desc1, const float* __restrict__ angle1, const int* __restrict__ node1, const uint8_t* __restrict__ valid1, int n1, const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc, const float* __restrict__ kfAngle, const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, int keyCap, float nnratio, int checkOri, int* __restrict__ matches12, int* __restrict__ nmatchesOut);
struct FuseSurvivor { int kf, mp; float u, v, ur, radius; int level, pad; };     // a (keyframe, point) pair that reaches the window search
__global__ void k_fuse_grid(const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp, pli_fuse_camera cam, int* __restrict__ cellStart, uint16_t* __restrict__ sIdx);
__global__ void k_fuse_project(const pli_fuse_point* __restrict__ mp, int nmp, int nkf, const float* __restrict__ kfPose, const uint8_t* __restrict__ skip, pli_fuse_camera cam, float th, const float* __restrict__ levelRatio, int nlevels, const float* __restrict__ scaleFactor, FuseSurvivor* __restrict__ surv, int* __restrict__ nSurv, int* __restrict__ bestIdx, int* __restrict__ bestDist);
template <int G, bool kViews> __global__ void k_fuse_match(const FuseSurvivor* __restrict__ surv, const int* __restrict__ nSurv, int nmp, const uint8_t* __restrict__ mpDesc, const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc, const float* __restrict__ kfUright, const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, const float* __restrict__ invSigma2, int reprojGate, int* __restrict__ bestIdx, int* __restrict__ bestDist);
__global__ void k_sim3_project(const pli_fuse_point* __restrict__ mp, int nmp, int npair, const float* __restrict__ kfPose, const uint8_t* __restrict__ skip, pli_fuse_camera cam, float th, const float* __restrict__ levelRatio, int nlevels, const float* __restrict__ scaleFactor, int form, FuseSurvivor* __restrict__ surv, int* __restrict__ candCount, int* __restrict__ bestIdx);
template <int kUp> __global__ void k_window_candidates(const FuseSurvivor* __restrict__ surv, int64_t nslot, const uint8_t* __restrict__ mpDesc, const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc, const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, int distLimit, int width, unsigned long long* __restrict__ candKeys, int* __restrict__ candCount);
__global__ void k_sim3_assign(const FuseSurvivor* __restrict__ surv, int nmp, const uint8_t* __restrict__ mpDesc, const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc, const uint8_t* __restrict__ occupied, const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, int distLimit, int width, const unsigned long long* __restrict__ candKeys, const int* __restrict__ candCount, int* __restrict__ rowPoint, int* __restrict__ bestIdx, int* __restrict__ nmatchesOut);
__global__ void k_reloc_project(const pli_fuse_point* __restrict__ mp, const int* __restrict__ mpOff, int ncand, const float* __restrict__ pose, pli_fuse_camera cam, float th, const float* __restrict__ levelRatio, int nlevels, const float* __restrict__ scaleFactor, FuseSurvivor* __restrict__ surv, int* __restrict__ candCount, int* __restrict__ bestIdx);
__global__ void k_reloc_assign(const FuseSurvivor* __restrict__ surv, const int* __restrict__ mpOff, const uint8_t* __restrict__ mpDesc, const float* __restrict__ mpAngle, const int* __restrict__ fOff, const pli_keypoint* __restrict__ fKp, const uint8_t* __restrict__ fDesc, int nf, const uint8_t* __restrict__ occupied, const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, int distLimit, int width, int checkOri, const unsigned long long* __restrict__ candKeys, const int* __restrict__ candCount, int* __restrict__ rowPoint, int* __restrict__ bestIdx, int* __restrict__ nmatchesOut);
__global__ void k_init_candidates(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1, int n1, const float* __restrict__ prevMatched, const pli_keypoint* __restrict__ kp2, const uint8_t* __restrict__ desc2, const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, float radius, int distLimit, int width, unsigned long long* __restrict__ candKeys, int* __restrict__ candCount);
__global__ void k_init_assign(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1, int n1, const float* __restrict__ prevMatched, const pli_keypoint* __restrict__ kp2, const uint8_t* __restrict__ desc2, int n2, const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, float radius, int distLimit, int width, float nnratio, int checkOri, const unsigned long long* __restrict__ candKeys, const int* __restrict__ candCount, int* __restrict__ matches12, int* __restrict__ raw12, int* __restrict__ nmatchesOut);
__global__ void k_fisheye_triangulate(const pli_keypoint* __restrict__ kpL, const pli_keypoint* __restrict__ kpR, const int* __restrict__ knnIdx, const int* __restrict__ knnDist, int nl, int nr, int monoL, int monoR, Kb8 c1, Kb8 c2, const float* __restrict__ R12t12, const float* __restrict__ sigma2, int* __restrict__ l2r, int* __restrict__ r2l, float* __restrict__ depth, float* __restrict__ p3d, int* __restrict__ nmatches);
__global__ void k_fuse_project_views(const pli_fuse_point* __restrict__ mp, int nmp, int nkf, const float* __restrict__ kfPose, const uint8_t* __restrict__ skip, Kb8 camL, Kb8 camR, pli_fuse_camera bounds, int sides, float th, const float* __restrict__ levelRatio, int nlevels, const float* __restrict__ scaleFactor, FuseSurvivor* __restrict__ surv, int* __restrict__ nSurv, int* __restrict__ bestIdx, int* __restrict__ bestDist);
__global__ void k_fill_f32(float* __restrict__ dst, int n, float v);
__global__ void k_local_project(const pli_fuse_point* __restrict__ mp, int nq, const float* __restrict__ T, pli_fuse_camera cam, float viewCosLimit, float th, int farPoints, float thFar, const float* __restrict__ levelRatio, int nlevels, const float* __restrict__ scaleFactor, pli_local_view* __restrict__ view, pli_proj_query* __restrict__ q, int* __restrict__ nInView);
__global__ void k_local_lines_project(const float* __restrict__ sp, const uint8_t* __restrict__ valid, const uint8_t* __restrict__ desc, int nl, const float* __restrict__ T, pli_fuse_camera cam, int* __restrict__ inViewOut, float* __restrict__ projS, int* __restrict__ inFrustum, uint8_t* __restrict__ gathered, int* __restrict__ count);
__global__ void k_proj_assign_fisheye(const pli_proj_query* __restrict__ qL, const pli_proj_query* __restrict__ qR, const uint8_t* __restrict__ qdesc, int nq, const pli_keypoint* __restrict__ kpL, const uint8_t* __restrict__ descL, const uint8_t* __restrict__ occL, const int* __restrict__ l2r, int nL, const pli_keypoint* __restrict__ kpR, const uint8_t* __restrict__ descR, const uint8_t* __restrict__ occR, const int* __restrict__ r2l, int nR, const float* __restrict__ noUright, float minX, float maxX, float minY, float maxY, float nnratio, const unsigned long long* __restrict__ keysL, const int* __restrict__ cntL, const unsigned long long* __restrict__ keysR, const int* __restrict__ cntR, int* __restrict__ mpL, int* __restrict__ mpR, int* __restrict__ nmatchesOut);
__global__ void k_proj2_candidates(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq, const pli_keypoint* __restrict__ kpL, const uint8_t* __restrict__ descL, int nL, const pli_keypoint* __restrict__ kpR, const uint8_t* __restrict__ descR, int nR, const float* __restrict__ noUright, float minX, float maxX, float minY, float maxY, unsigned long long* __restrict__ candKeys, int* __restrict__ candCount, int* __restrict__ leftOpen);
__global__ void k_proj2_assign(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq, const pli_keypoint* __restrict__ kpL, const uint8_t* __restrict__ descL, const uint8_t* __restrict__ occL, int nL, const pli_keypoint* __restrict__ kpR, const uint8_t* __restrict__ descR, const uint8_t* __restrict__ occR, int nR, const float* __restrict__ noUright, float minX, float maxX, float minY, float maxY, int checkOri, const unsigned long long* __restrict__ candKeys, const int* __restrict__ candCount, const int* __restrict__ leftOpen, int* __restrict__ rawIdx2, int* __restrict__ hist, int* __restrict__ accepts);
__global__ void k_proj2_finish(const pli_proj_query* __restrict__ q, int nq, const pli_keypoint* __restrict__ kpL, const pli_keypoint* __restrict__ kpR, int checkOri, const int* __restrict__ rawIdx2, const int* __restrict__ hist, const int* __restrict__ accepts, int* __restrict__ bestIdx2, int* __restrict__ nmatchesOut);
__global__ void k_lapping_order(const pli_keypoint* __restrict__ srcKp, const uint8_t* __restrict__ srcDesc, int n, float lap0, float lap1, pli_keypoint* __restrict__ dstKp, uint8_t* __restrict__ dstDesc, int* __restrict__ monoCount);
__global__ void k_lapping_order_counted(const pli_keypoint* __restrict__ srcKp, const uint8_t* __restrict__ srcDesc, const int* __restrict__ count, int cap, float lap0, float lap1, pli_keypoint* __restrict__ dstKp, uint8_t* __restrict__ dstDesc, int* __restrict__ monoCount);
// single-camera Frames of a distorted pinhole camera (frame_kernels.hip): the context's camera and its image bounds, by value
struct PinholeUndist {
  pli_pinhole_distortion cam;
  int on;                             // a camera is set and its k1 != 0 (the reference's gate); 0: every "undistorted" output is a copy
  float minX, maxX, minY, maxY;       // mnMinX .. mnMaxY (ComputeImageBounds)
};
__global__ void k_undistort_points(PinholeUndist C, const float2* __restrict__ xy, int n, float2* __restrict__ xyUn, int* __restrict__ cell);
__global__ void k_frame_single_tail(const DevParams* __restrict__ Pp, PinholeUndist C, const void* __restrict__ depthImg, DepthFormat fmt, int64_t pitch, uint8_t* __restrict__ table, int64_t offCounts, int64_t offKp0, int64_t offKl0, int64_t offUr, int64_t offDepth, float2* __restrict__ kpUn, int* __restrict__ cell, float4* __restrict__ klUn);

__global__ void k_tx_tail(TxTailArgs T);
__global__ void k_tx_rec_from_hot(const RxCtl* __restrict__ ctl, const int2* __restrict__ hotAll, const float2* __restrict__ coldAll, float4* __restrict__ recAll, int64_t npix, int img0);
__global__ void k_tx_hot_trig_err(unsigned long long* __restrict__ maxErrBits);
__global__ void k_tx_cells(RxCtl* __restrict__ ctl, const int* __restrict__ stampAll, int* __restrict__ tileTouchAll, int ncell, int nimg, int img0, int t, int mode, int* __restrict__ list, int* __restrict__ cnt);
__global__ void k_tx_diffmark_cells(TxRound A, int t, const int* __restrict__ list, const int* __restrict__ cnt);
__global__ void k_tx_prep_cells(TxRound A, int t, const int* __restrict__ list, const int* __restrict__ cnt);
__global__ void k_zero_ranges(ZeroRanges Z);
__global__ void k_tx_collect(RxCtl* __restrict__ ctl, const int* __restrict__ idPlaneAll, const int2* __restrict__ ownAll, const int* __restrict__ rgSizeAll, int64_t npix, int minReg, int* __restrict__ candAll, int* __restrict__ candCnt, int img0, int emitCap, const int2* __restrict__ rgBoxAll, int boxCut);
__global__ void k_tx_emit_sorted(const RxCtl* __restrict__ ctl, const int* __restrict__ candAll, const int* __restrict__ candCnt, const float4* __restrict__ rgSegAll, int64_t npix, int rmask, float* __restrict__ segAll, int* __restrict__ nSeg, int maxSeg, int img0, int emitCap);
__global__ void k_tx_order(const int* __restrict__ tileCntAll, int ntile, int nimg, int img0, int* __restrict__ perm);
// keyframe database (kfdb_kernels.hip): a slot's run of the word / value arena, and what a query answers per slot
struct KfdbSlot { long long off; int count, pad; };
struct KfdbAnswer { int common, first; double score; };
constexpr int KFDB_QUERY_BLOCK = 256;                                     // 4 waves, one slot each at a time
constexpr int KFDB_QUERY_MAX_BLOCKS = PLI_KFDB_QUERY_MAX_WAVES / (KFDB_QUERY_BLOCK / 64);
__global__ void k_kfdb_query(const uint32_t* __restrict__ qWord, const double* __restrict__ qValue, int nq, const KfdbSlot* __restrict__ slots, int nslots, const uint32_t* __restrict__ word, const double* __restrict__ value, KfdbAnswer* __restrict__ out);
// distinctive descriptors of map points and lines (mapfeat_kernels.hip): `list` holds the group ids of one size class
constexpr int DISTINCTIVE_BLOCK = 256;                                    // k_distinctive_wave: 4 waves, one group each at a time
constexpr int DISTINCTIVE_WAVE_ROWS = 64;                                 // the small class: groups of up to one wave's lanes
static_assert(PLI_DISTINCTIVE_MAX_OBS * 32 <= 65536 && PLI_DISTINCTIVE_MAX_OBS <= 4096, "a group fits the LDS of a workgroup, a row index the key's low 12 bits");
constexpr int DISTINCTIVE_MAX_BLOCKS = 512;                               // per launch (two per compute unit); the lists are strided over the grid
__global__ void k_distinctive_wave(const uint8_t* __restrict__ desc, const int* __restrict__ off, const int* __restrict__ list, int nlist, int* __restrict__ best, int* __restrict__ bestMedian, int* __restrict__ rowMedian);
struct DistinctiveChunk { int group, firstRow; };                        // rows firstRow .. firstRow + DISTINCTIVE_BLOCK of a large group
__global__ void k_distinctive_block(const uint8_t* __restrict__ desc, const int* __restrict__ off, const DistinctiveChunk* __restrict__ chunks, int nchunks, int* __restrict__ rowMedian);
__global__ void k_distinctive_pick(const int* __restrict__ off, const int* __restrict__ list, int nlist, const int* __restrict__ rowMedian, int* __restrict__ best, int* __restrict__ bestMedian);
}  // namespace pli
