// Matching kernels for gfx950 (wave64): 256-bit Hamming by XOR + popcount on
// 4 x u64, wave-wide argmin by 64-bit key reduction.
//
//   k_stereo_points + k_stereo_median   Frame::ComputeStereoMatches        (Frame.cc:976-1154)
//   k_stereo_lines                      Frame::ComputeStereoMatches_Lines  (Frame.cc:1156-1307)
//                                       + matchGrid(lines) (LineMatcher.cpp:317-396)
//                                       + GridStructure/LineIterator (gridStructure.cpp, LineIterator.cpp)
//   k_distance                          ORBmatcher::DescriptorDistance     (ORBmatcher.cc:2495-2511)
//   k_knn2, k_ratio, k_mutual           matchNNR / match                   (LineMatcher.cpp:139-229)
//   k_proj_candidates + k_proj_assign   ORBmatcher::SearchByProjection(F,F)(ORBmatcher.cc:2179-2323) and
//   (k_proj_assign_scan: large frames)  ORBmatcher::SearchByProjection(F,MPs)(ORBmatcher.cc:44-143)
//   k_proj_assign_fisheye               the same (F,MPs) for a frame of two fisheye cameras (ORBmatcher.cc:44-214)
//   k_track_queries/candidates/assign/lines   frame-to-frame track matching of a batch (pli_batch_track)
//   k_node_sort + k_search_by_bow       ORBmatcher::SearchByBoW(KF,F)        (ORBmatcher.cc:269-470)
//   k_node_sort, k_tri_match, k_tri_finish  ORBmatcher::SearchForTriangulation (ORBmatcher.cc:965-1206)
//   k_kb8_rays, k_node_sort, k_tri_match_kb8, k_tri_finish  the same for keyframes of two KannalaBrandt8 cameras (mpCamera2)
//   k_node_sort, k_tri_match, k_newpt_list, k_newpt_geometry, k_newpt_pick  LocalMapping::CreateNewMapPoints (LocalMapping.cc:423-684)
//   k_kb8_rays, k_node_sort, k_tri_match_kb8, k_newpt_list, k_newpt_geometry_kb8, k_newpt_pick  the same for keyframes of two KannalaBrandt8 cameras
//   k_node_sort + k_search_by_bow_kf    ORBmatcher::SearchByBoW(KF,KF)       (ORBmatcher.cc:823-963)
//   k_fuse_grid, k_fuse_project, k_fuse_match  the search of ORBmatcher::Fuse (ORBmatcher.cc:1399-1609, :1611-1733)
//   k_fuse_grid, k_fuse_project_views, k_fuse_match<8, true>  the same search for keyframes of two KannalaBrandt8 cameras, both values of bRight
//   k_node_sort + k_search_by_bow_two_cameras  ORBmatcher::SearchByBoW(KF,F) for a frame of two cameras (ORBmatcher.cc:342-369, :373-433)
//   k_fuse_grid, k_sim3_project, k_window_candidates<0>, k_sim3_assign  ORBmatcher::SearchByProjection(KF, Scw, ...) (ORBmatcher.cc:473-704)
//   k_fuse_grid, k_reloc_project, k_window_candidates<1>, k_reloc_assign  ORBmatcher::SearchByProjection(Frame, KF, sAlreadyFound, ...) (ORBmatcher.cc:2325-2447)
//   k_fuse_grid, k_init_candidates, k_init_assign  ORBmatcher::SearchForInitialization (ORBmatcher.cc:706-821)
#include "kernels.hpp"
#include "device_prims.hpp"
#include <climits>

namespace pli {

__device__ __forceinline__ void load_desc(const uint8_t* p, uint64_t d[4]) {
  const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
  d[0] = q[0]; d[1] = q[1]; d[2] = q[2]; d[3] = q[3];
}

// ---------------------------------------------------------------------------
// Rotation consistency (mbCheckOrientation), shared by the projection, BoW and triangulation searches: a match votes for the
// bin of the angle between its two keypoints; matches outside the three fullest bins are dropped.
// ---------------------------------------------------------------------------
constexpr int HISTO_LENGTH = 30;

// the raw bin of the reference expression (ORBmatcher.cc:2286-2291; :391-396 in SearchByBoW): 0..12 for angles in [0, 360); other floats may
// give any int, and each search family states below what it does with a bin outside 0..HISTO_LENGTH-1
__device__ __forceinline__ int rot_bin(float a, float b) {
  float rot = __fsub_rn(a, b);
  if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
  int bin = (int)roundf(__fmul_rn(rot, 1.0f / HISTO_LENGTH));
  if (bin == HISTO_LENGTH) bin = 0;
  return bin;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2449-2490) on a histogram of HISTO_LENGTH counts: the three fullest bins, the
// second and third only if they hold at least 10 % of the first (-1: none)
__device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
  for (int i = 0; i < HISTO_LENGTH; i++) {
    const int s = hist[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
    else if (s > max3) { max3 = s; i3 = i; }
  }
  if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
  else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) i3 = -1;
  ind1 = i1; ind2 = i2; ind3 = i3;
}

// ---------------------------------------------------------------------------
// Stereo points: one wave per left keypoint.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_stereo_points(const DevParams* __restrict__ Pp, const uint8_t* __restrict__ pyr,
                                                      uint8_t* __restrict__ table, int64_t recordBytes,
                                                      int64_t offCounts, int64_t offKp0, int64_t offKp1,
                                                      int64_t offDesc0, int64_t offDesc1, int64_t offUr,
                                                      int64_t offDepth, int* __restrict__ sadOut,
                                                      int* __restrict__ bestIdxOut) {
  const DevParams& P = *Pp;
  const int frame = blockIdx.y, iL = blockIdx.x, lane = threadIdx.x;
  uint8_t* rec = table + (int64_t)frame * recordBytes;
  const int* counts = reinterpret_cast<const int*>(rec + offCounts);
  const int N = counts[0], Nr = counts[1];
  if (iL >= N) return;
  const pli_keypoint* kpsL = reinterpret_cast<const pli_keypoint*>(rec + offKp0);
  const pli_keypoint* kpsR = reinterpret_cast<const pli_keypoint*>(rec + offKp1);
  const uint8_t* descL = rec + offDesc0;
  const uint8_t* descR = rec + offDesc1;
  float* uright = reinterpret_cast<float*>(rec + offUr);
  float* depth = reinterpret_cast<float*>(rec + offDepth);
  const pli_keypoint kpL = kpsL[iL];
  const int levelL = kpL.octave;
  const float vL = kpL.y, uL = kpL.x;
  const int rowL = (int)vL;
  const float maxD = P.maxD, minD = 0.f;
  const float minU = __fsub_rn(uL, maxD), maxU = __fsub_rn(uL, minD);
  uint64_t dL[4];
  load_desc(descL + (int64_t)iL * 32, dL);
  unsigned long long bestKey = ~0ull;
  // (row band half-height per level through LDS: the scan below then has no load that waits for another)
  __shared__ float s_r[MAX_LEVELS];
  if (lane < MAX_LEVELS) s_r[lane] = lane < P.nlevels ? __fmul_rn(2.0f, P.lv[lane].scale) : 0.f;
  __syncthreads();
  if (!(maxU < 0)) {
#pragma unroll 4
    for (int iR = lane; iR < Nr; iR += 64) {
      const pli_keypoint kpR = kpsR[iR];
      const float r = s_r[kpR.octave];
      const int maxr = (int)ceilf(__fadd_rn(kpR.y, r));
      const int minr = (int)floorf(__fsub_rn(kpR.y, r));
      if (rowL < minr || rowL > maxr) continue;
      if (kpR.octave < levelL - 1 || kpR.octave > levelL + 1) continue;
      const float uR = kpR.x;
      if (uR >= minU && uR <= maxU) {
        uint64_t dR[4];
        load_desc(descR + (int64_t)iR * 32, dR);
        const int dist = hamming256(dL, dR);
        if (dist < 100) {     // ORBmatcher::TH_HIGH, strict
          unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)iR;
          bestKey = key < bestKey ? key : bestKey;
        }
      }
    }
  }
  bestKey = wave_min_u64(bestKey);
  float outU = -1.f, outD = -1.f;
  int outSad = -1, outIdx = -1;
  const int thOrbDist = (100 + 50) / 2;
  if (bestKey != ~0ull && (int)(bestKey >> 32) < thOrbDist) {
    const int bestIdxR = (int)(bestKey & 0xFFFFFFFFu);
    outIdx = bestIdxR;
    const float uR0 = kpsR[bestIdxR].x;
    const LevelGeom& G = P.lv[levelL];
    const float scaleFactor = G.invScale;
    const float scaleduL = roundf(__fmul_rn(kpL.x, scaleFactor));
    const float scaledvL = roundf(__fmul_rn(kpL.y, scaleFactor));
    const float scaleduR0 = roundf(__fmul_rn(uR0, scaleFactor));
    const int w = 5, L = 5;
    const int cy = (int)scaledvL, cxl = (int)scaleduL, cxr = (int)scaleduR0;
    bool ok = !(cy - w < 0 || cy + w + 1 > G.h || cxl - w < 0 || cxl + w + 1 > G.w);
    const float iniu = __fadd_rn(scaleduR0, (float)(L - w));
    const float endu = __fadd_rn(scaleduR0, (float)(L + w + 1));
    if (iniu < 0 || endu >= (float)G.w) ok = false;
    if (cxr - L - w < 0) ok = false;
    if (ok) {
      const uint8_t* imL = pyr + (int64_t)(frame * 2) * P.pyrBlock + G.offset;
      const uint8_t* imR = pyr + (int64_t)(frame * 2 + 1) * P.pyrBlock + G.offset;
      const int cL = imL[(int64_t)cy * G.pitch + cxl];
      // each lane owns up to two pixels of the 11x11 window
      int aL[2], px[2], py[2];
      bool act[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        int i = lane + 64 * k;
        act[k] = i < 121;
        int dy = act[k] ? i / 11 - w : 0, dx = act[k] ? i % 11 - w : 0;
        px[k] = dx; py[k] = dy;
        aL[k] = act[k] ? (int)imL[(int64_t)(cy + dy) * G.pitch + cxl + dx] - cL : 0;
      }
      float vDists[11];
      int bestDist = INT_MAX, bestincR = 0;
#pragma unroll
      for (int incR = -L; incR <= L; ++incR) {
        const int cR = imR[(int64_t)cy * G.pitch + cxr + incR];
        int s = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (act[k]) {
            int b = (int)imR[(int64_t)(cy + py[k]) * G.pitch + cxr + incR + px[k]] - cR;
            s += abs(aL[k] - b);
          }
        s = wave_sum_i32(s);
        const float dist = (float)s;
        if (dist < (float)bestDist) { bestDist = (int)dist; bestincR = incR; }
        vDists[L + incR] = dist;
      }
      if (!(bestincR == -L || bestincR == L)) {
        float dist1 = 0, dist2 = 0, dist3 = 0;
#pragma unroll
        for (int k = 1; k < 10; ++k)
          if (k == L + bestincR) { dist1 = vDists[k - 1]; dist2 = vDists[k]; dist3 = vDists[k + 1]; }
        const float deltaR = __fdiv_rn(__fsub_rn(dist1, dist3),
                                       __fmul_rn(2.0f, __fsub_rn(__fadd_rn(dist1, dist3), __fmul_rn(2.0f, dist2))));
        if (!(deltaR < -1 || deltaR > 1)) {
          float bestuR = __fmul_rn(G.scale, __fadd_rn(__fadd_rn(scaleduR0, (float)bestincR), deltaR));
          float disparity = __fsub_rn(uL, bestuR);
          if (disparity >= minD && disparity < maxD) {
            if (disparity <= 0) {
              disparity = 0.01f;
              bestuR = (float)((double)uL - 0.01);
            }
            outD = __fdiv_rn(P.bf, disparity);
            outU = bestuR;
            outSad = bestDist;
          }
        }
      }
    }
  }
  if (lane == 0) {
    uright[iL] = outU;
    depth[iL] = outD;
    sadOut[(int64_t)frame * P.kpCap + iL] = outSad;
    if (bestIdxOut) bestIdxOut[(int64_t)frame * P.kpCap + iL] = outIdx;
  }
}

// median-based outlier cut (Frame.cc:1140-1153), one workgroup per frame
__global__ __launch_bounds__(256) void k_stereo_median(const DevParams* __restrict__ Pp, uint8_t* __restrict__ table,
                                                       int64_t recordBytes, int64_t offCounts, int64_t offUr,
                                                       int64_t offDepth, const int* __restrict__ sadIn) {
  extern __shared__ int s_sad[];
  __shared__ int s_m, s_median, s_left;
  const DevParams& P = *Pp;
  const int frame = blockIdx.x, tid = threadIdx.x;
  uint8_t* rec = table + (int64_t)frame * recordBytes;
  int* counts = reinterpret_cast<int*>(rec + offCounts);
  const int N = counts[0];
  float* uright = reinterpret_cast<float*>(rec + offUr);
  float* depth = reinterpret_cast<float*>(rec + offDepth);
  const int* sad = sadIn + (int64_t)frame * P.kpCap;
  if (tid == 0) { s_m = 0; s_median = -1; s_left = 0; }
  __syncthreads();
  int loc = 0;
  for (int i = tid; i < N; i += 256) {
    int v = sad[i];
    s_sad[i] = v;
    loc += v >= 0;
  }
  if (loc) atomicAdd(&s_m, loc);
  __syncthreads();
  const int M = s_m;
  if (M == 0) {
    if (tid == 0) counts[4] = 0;
    return;
  }
  // the median = the (M / 2)-th smallest valid distance (Frame.cc:1143-1146 sorts and takes element size / 2): radix select, four
  // passes of 8 bits from the top — a 256-bin LDS histogram of the values that match the bits chosen so far, and one wave that finds
  // the bin holding the k-th.  (The earlier form counted, for every value, the smaller ones with one dependent LDS read per
  // comparison: 93 us for the 1200 keypoints of a single pair.)
  __shared__ int s_hist[256];
  __shared__ unsigned s_pref, s_mask;
  __shared__ int s_k;
  if (tid == 0) { s_pref = 0u; s_mask = 0u; s_k = M / 2; }
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;
    __syncthreads();
    const unsigned pref = s_pref, mask = s_mask;
    for (int i = tid; i < N; i += 256) {
      const int v = s_sad[i];
      if (v >= 0 && ((unsigned)v & mask) == pref) atomicAdd(&s_hist[((unsigned)v >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid < 64) {
      const int h0 = s_hist[4 * tid], h1 = s_hist[4 * tid + 1], h2 = s_hist[4 * tid + 2], h3 = s_hist[4 * tid + 3];
      const int sum = h0 + h1 + h2 + h3;
      int inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t2 = __shfl_up(inc, o, 64);
        if (tid >= o) inc += t2;
      }
      const int k = s_k, before = inc - sum;
      if (before <= k && k < inc) {                 // exactly one lane: the k-th lies in its four bins
        int b = 0, c = before;
        if (k >= c + h0) { c += h0; b = 1; if (k >= c + h1) { c += h1; b = 2; if (k >= c + h2) { c += h2; b = 3; } } }
        s_pref = pref | ((unsigned)(4 * tid + b) << shift);
        s_mask = mask | (255u << shift);
        s_k = k - c;
      }
    }
    __syncthreads();
  }
  if (tid == 0) s_median = (int)s_pref;
  __syncthreads();
  const float median = (float)s_median;
  const float thDist = __fmul_rn(__fmul_rn(1.5f, 1.4f), median);
  loc = 0;
  for (int i = tid; i < N; i += 256) {
    const int v = s_sad[i];
    if (v < 0) continue;
    if (!((float)v < thDist)) {
      uright[i] = -1.f;
      depth[i] = -1.f;
    } else ++loc;
  }
  if (loc) atomicAdd(&s_left, loc);
  __syncthreads();
  if (tid == 0) counts[4] = s_left;
}

// ---------------------------------------------------------------------------
// Stereo lines: one workgroup per frame.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void normalize2(double& a, double& b) {
  const double m = sqrt(a * a + b * b);
  a /= m;
  b /= m;
}

__device__ double line_overlap_stereo(double spl_obs, double epl_obs, double spl_proj, double epl_proj, double horizTh) {
  double overlap = 1.f;
  if (fabs(epl_obs - spl_obs) > horizTh) {
    double sln = fmin(spl_obs, epl_obs);
    double eln = fmax(spl_obs, epl_obs);
    double spn = fmin(spl_proj, epl_proj);
    double epn = fmax(spl_proj, epl_proj);
    double length = eln - spn;
    if ((epn < sln) || (spn > eln)) overlap = 0.f;
    else {
      if ((epn > eln) && (spn < sln)) overlap = eln - sln;
      else overlap = fmin(eln, epn) - fmax(sln, spn);
    }
    if (length > 0.01f) overlap = overlap / length;
    else overlap = 0.f;
    if (overlap > 1.f) overlap = 1.f;
  }
  return overlap;
}

__global__ __launch_bounds__(256) void k_stereo_lines(const DevParams* __restrict__ Pp, uint8_t* __restrict__ table,
                                                      int64_t recordBytes, int64_t offCounts, int64_t offKl0,
                                                      int64_t offKl1, int64_t offLd0, int64_t offLd1, int64_t offDisp,
                                                      int64_t offLe, unsigned long long* __restrict__ maskAll,
                                                      double* __restrict__ dirAll, short* __restrict__ dmatAll,
                                                      int* __restrict__ m12All, int* __restrict__ m21All, int phase) {
  // phase 0: the whole matcher, one workgroup per frame.  With many lines (4K: 500 x 500 pairs per frame) the pair distances are
  // the bulk and one workgroup per frame leaves the chip idle: the host then launches phase 1 (tables of the right lines),
  // phase 2 (the pair distances, gridDim.y workgroups per frame) and phase 3 (the selection) — the phases already talk through
  // global memory.
  const DevParams& P = *Pp;
  const int frame = blockIdx.x, tid = threadIdx.x;
  uint8_t* rec = table + (int64_t)frame * recordBytes;
  int* counts = reinterpret_cast<int*>(rec + offCounts);
  const int n1 = counts[2], n2 = counts[3];
  const pli_keyline* KL = reinterpret_cast<const pli_keyline*>(rec + offKl0);
  const pli_keyline* KR = reinterpret_cast<const pli_keyline*>(rec + offKl1);
  const uint8_t* descL = rec + offLd0;
  const uint8_t* descR = rec + offLd1;
  float* disp = reinterpret_cast<float*>(rec + offDisp);
  double* le = reinterpret_cast<double*>(rec + offLe);
  const int cap = P.klCap;
  unsigned long long* mask = maskAll + (int64_t)frame * cap * GRID_ROWS;
  double* dir = dirAll + (int64_t)frame * cap * 2;
  short* dmat = dmatAll + (int64_t)frame * cap * cap;
  int* m12 = m12All + (int64_t)frame * cap;
  int* m21 = m21All + (int64_t)frame * cap;
  if (phase <= 1)
  for (int i = tid; i < n1; i += 256) {
    disp[2 * i] = -1.f; disp[2 * i + 1] = -1.f;
    le[3 * i] = 0.0; le[3 * i + 1] = 0.0; le[3 * i + 2] = 0.0;
    m12[i] = -1;
  }
  if (n1 == 0 || n2 == 0) {
    if (tid == 0 && phase != 2) counts[5] = 0;
    return;
  }
  const double inv_width = (double)GRID_COLS / (double)P.W;
  const double inv_height = (double)GRID_ROWS / (double)P.H;
  // right lines: direction + Bresenham cell masks (getLineCoords / LineIterator)
  if (phase <= 1)
  for (int i2 = tid; i2 < n2; i2 += 256) {
    const pli_keyline kl = KR[i2];
    double vx = (double)__fsub_rn(kl.endPointX, kl.startPointX) * inv_width;
    double vy = (double)__fsub_rn(kl.endPointY, kl.startPointY) * inv_height;
    normalize2(vx, vy);
    dir[2 * i2] = vx; dir[2 * i2 + 1] = vy;
    unsigned long long* mk = mask + (int64_t)i2 * GRID_ROWS;
    for (int r = 0; r < GRID_ROWS; ++r) mk[r] = 0ull;
    double x1 = (double)kl.startPointX * inv_width, y1 = (double)kl.startPointY * inv_height;
    double x2 = (double)kl.endPointX * inv_width, y2 = (double)kl.endPointY * inv_height;
    const bool steep = fabs(y2 - y1) > fabs(x2 - x1);
    if (steep) { double t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t; }
    if (x1 > x2) { double t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
    const double dx = x2 - x1, dy = fabs(y2 - y1);
    double error = dx / 2.0;
    const int ystep = (y1 < y2) ? 1 : -1;
    int x = (int)x1, y = (int)y1;
    const int maxX = (int)x2;
    while (x <= maxX) {
      const int cx = steep ? y : x, cy = steep ? x : y;
      if (cx >= 0 && cx < GRID_COLS && cy >= 0 && cy < GRID_ROWS) mk[cy] |= 1ull << cx;
      error -= dy;
      if (error < 0) { y += ystep; error += dx; }
      x++;
    }
  }
  if (phase == 1) return;
  __threadfence_block();
  __syncthreads();
  // pair distances for candidate pairs passing the direction gate, else -1
  const int ws = P.sWs;
  if (phase == 0 || phase == 2)
  for (int pidx = tid + 256 * (int)blockIdx.y; pidx < n1 * n2; pidx += 256 * (int)gridDim.y) {
    const int i1 = pidx / n2, i2 = pidx - i1 * n2;
    const pli_keyline kl = KL[i1];
    const int sx = (int)((double)kl.startPointX * inv_width), sy = (int)((double)kl.startPointY * inv_height);
    const int ex = (int)((double)kl.endPointX * inv_width), ey = (int)((double)kl.endPointY * inv_height);
    const unsigned long long* mk = mask + (int64_t)i2 * GRID_ROWS;
    bool cand = false;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int qx = e ? ex : sx, qy = e ? ey : sy;
      const int min_x = max(0, qx - ws), max_x = min(GRID_COLS, qx + 0 + 1);
      if (qy >= 0 && qy < GRID_ROWS && max_x > min_x) {
        const unsigned long long hi = max_x >= 64 ? ~0ull : ((1ull << max_x) - 1ull);
        const unsigned long long wm = hi & ~((1ull << min_x) - 1ull);
        cand = cand || ((mk[qy] & wm) != 0ull);
      }
    }
    short d = -1;
    if (cand) {
      double vx = (double)(ex - sx), vy = (double)(ey - sy);
      normalize2(vx, vy);
      const double dt = vx * dir[2 * i2] + vy * dir[2 * i2 + 1];
      if (!(fabs(dt) < P.lineSimTh)) {
        uint64_t a[4], b[4];
        load_desc(descL + (int64_t)i1 * 32, a);
        load_desc(descR + (int64_t)i2 * 32, b);
        d = (short)hamming256(a, b);
      }
    }
    dmat[(int64_t)i1 * cap + i2] = d;
  }
  if (phase == 2) return;
  __threadfence_block();
  __syncthreads();
  // bestLRMatches: a pair only counts if it lowers the running minimum of its column
  if (P.bestLR) {
    for (int i2 = tid; i2 < n2; i2 += 256) {
      int run = INT_MAX, who = -1;
      for (int i1 = 0; i1 < n1; ++i1) {
        const int d = dmat[(int64_t)i1 * cap + i2];
        if (d < 0) continue;
        if (d < run) { run = d; who = i1; }
        else dmat[(int64_t)i1 * cap + i2] = -1;
      }
      m21[i2] = who;
    }
    __threadfence_block();
    __syncthreads();
  }
  for (int i1 = tid; i1 < n1; i1 += 256) {
    int best_d = INT_MAX, best_d2 = INT_MAX, best_idx = -1;
    for (int i2 = 0; i2 < n2; ++i2) {
      const int d = dmat[(int64_t)i1 * cap + i2];
      if (d < 0) continue;
      if (d < best_d) { best_d2 = best_d; best_d = d; best_idx = i2; }
      else if (d < best_d2) best_d2 = d;
    }
    int m = -1;
    if ((double)best_d < (double)best_d2 * P.ratio12L) m = best_idx;
    if (P.bestLR && m >= 0 && m21[m] != i1) m = -1;
    m12[i1] = m;
  }
  __threadfence_block();
  __syncthreads();
  int loc = 0;
  for (int i1 = tid; i1 < n1; i1 += 256) {
    const int i2 = m12[i1];
    if (i2 < 0) continue;
    const pli_keyline a = KL[i1], b = KR[i2];
    const double spl0 = a.startPointX, spl1 = a.startPointY, epl0 = a.endPointX, epl1 = a.endPointY;
    double l0 = spl1 * 1.0 - 1.0 * epl1, l1 = 1.0 * epl0 - spl0 * 1.0, l2 = spl0 * epl1 - spl1 * epl0;
    const double nrm = sqrt(l0 * l0 + l1 * l1);
    l0 = l0 / nrm; l1 = l1 / nrm; l2 = l2 / nrm;
    double spr0 = b.startPointX, spr1 = b.startPointY, epr0 = b.endPointX, epr1 = b.endPointY;
    const double overlap = line_overlap_stereo(spl1, epl1, spr1, epr1, P.horizTh);
    const double nsx = (spr0 * (spl1 - epr1) + epr0 * (spr1 - spl1)) / (spr1 - epr1);
    spr0 = nsx; spr1 = spl1;
    const double nex = (spr0 * (epl1 - epr1) + epr0 * (spr1 - epl1)) / (spr1 - epr1);
    epr0 = nex; epr1 = epl1;
    double disp_s = spl0 - spr0, disp_e = epl0 - epr0;
    if (fmin(disp_s, disp_e) / fmax(disp_s, disp_e) < P.minDispRatio) { disp_s = -1.0; disp_e = -1.0; }
    if (disp_s >= P.minDisp && disp_e >= P.minDisp && fabs(spl1 - epl1) > P.horizTh && fabs(spr1 - epr1) > P.horizTh &&
        overlap > P.overlapTh) {
      disp[2 * i1] = (float)disp_s;
      disp[2 * i1 + 1] = (float)disp_e;
      le[3 * i1] = l0; le[3 * i1 + 1] = l1; le[3 * i1 + 2] = l2;
      ++loc;
    }
  }
  __shared__ int s_cnt;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  if (loc) atomicAdd(&s_cnt, loc);
  __syncthreads();
  if (tid == 0) counts[5] = s_cnt;
}

// ---------------------------------------------------------------------------
// Stateless matchers on caller tables
// ---------------------------------------------------------------------------
__global__ void k_distance(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int n, int* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t x[4], y[4];
  load_desc(a + (int64_t)i * 32, x);
  load_desc(b + (int64_t)i * 32, y);
  out[i] = hamming256(x, y);
}

// knnMatch(k=2): one wave per query; ties -> lower train index
__global__ __launch_bounds__(64) void k_knn2(const uint8_t* __restrict__ q, int nq, const uint8_t* __restrict__ t, int nt,
                                             int* __restrict__ idx, int* __restrict__ dist) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= nq) return;
  uint64_t dq[4];
  load_desc(q + (int64_t)i * 32, dq);
  WaveTop2 top;
  for (int j = lane; j < nt; j += 64) {
    uint64_t dt[4];
    load_desc(t + (int64_t)j * 32, dt);
    top.push(((unsigned long long)hamming256(dq, dt) << 32) | (unsigned)j);
  }
  const unsigned long long m1 = top.min1(), m2 = top.min2(m1);
  if (lane == 0) {
    idx[2 * i] = m1 == ~0ull ? -1 : (int)(m1 & 0xFFFFFFFFu);
    dist[2 * i] = m1 == ~0ull ? INT_MAX : (int)(m1 >> 32);
    idx[2 * i + 1] = m2 == ~0ull ? -1 : (int)(m2 & 0xFFFFFFFFu);
    dist[2 * i + 1] = m2 == ~0ull ? INT_MAX : (int)(m2 >> 32);
  }
}

// matchNNR ratio test on knn2 output
__global__ void k_ratio(const int* __restrict__ idx, const int* __restrict__ dist, int n, int nTrain, float nnr,
                        int* __restrict__ m) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int r = -1;
  if (nTrain >= 2 && (float)dist[2 * i] < __fmul_rn((float)dist[2 * i + 1], nnr)) r = idx[2 * i];
  m[i] = r;
}

__global__ void k_mutual(int* __restrict__ m12, const int* __restrict__ m21, int n1, int* __restrict__ nmatches) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int ok = 0;
  if (i < n1) {
    int i2 = m12[i];
    if (i2 >= 0 && m21 && m21[i2] != i) { m12[i] = -1; i2 = -1; }
    ok = i2 >= 0;
  }
  unsigned long long b = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(nmatches, __popcll(b));
}

// ---------------------------------------------------------------------------
// Frame::ComputeStereoFromRGBD (Frame.cc:1309-1331): depth of every left keypoint from a registered float
// depth image, mvuRight = x - bf / d.  (cv::Mat::at<float>(v, u) with float arguments truncates them.)
// The image is the caller's raw one (float or uint16, pitch in elements): depth_value (kernels.hpp) converts the element read.
// ---------------------------------------------------------------------------
__global__ void k_stereo_from_depth(const DevParams* __restrict__ Pp, const void* __restrict__ depthImg, DepthFormat fmt, int64_t pitch,
                                    int W, int H, uint8_t* __restrict__ table, int64_t offCounts, int64_t offKp0,
                                    int64_t offUr, int64_t offDepth) {
  const DevParams& P = *Pp;
  const int N = reinterpret_cast<const int*>(table + offCounts)[0];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const pli_keypoint kp = reinterpret_cast<const pli_keypoint*>(table + offKp0)[i];
  const int u = (int)kp.x, v = (int)kp.y;
  float ur = -1.f, dp = -1.f;
  if (u >= 0 && v >= 0 && u < W && v < H) {
    const float d = depth_value(depthImg, fmt, (int64_t)v * pitch + u);
    if (d > 0) { dp = d; ur = __fsub_rn(kp.x, __fdiv_rn(P.bf, d)); }
  }
  reinterpret_cast<float*>(table + offUr)[i] = ur;
  reinterpret_cast<float*>(table + offDepth)[i] = dp;
}

// ---------------------------------------------------------------------------
// The two projection searches: SearchByProjection(CurrentFrame, LastFrame) (ORBmatcher.cc:2179-2323) and
// SearchByProjection(Frame, MapPoints) (:44-143, rectified stereo branch).
// Which keypoints a query may take (grid window, pyramid levels, radius, uRight gate) and their Hamming distances do
// not depend on the other queries; only "already taken" does.  Phase 1 (one wave per query, all queries in parallel)
// lists the candidates of every query as (distance, visiting order, index) keys; phase 2 (one wave, queries in
// order, because a keypoint taken by an earlier query is not available to later ones) takes the smallest key whose
// keypoint is still free — the reference's running minimum in visiting order — with the owner table in LDS and the
// next query's keys already in flight.  A frame whose keypoints do not fit the LDS owner table runs phase 2 alone,
// with the owner table in global memory and one scan of the frame per query (proj_assign_dev).
// ---------------------------------------------------------------------------

__device__ __forceinline__ bool proj_window(const pli_proj_query& Q, float minX, float maxX, float minY, float maxY,
                                            float gwInv, float ghInv, bool checkBounds, int& c0, int& c1, int& r0, int& r1) {
  if (!Q.valid) return false;
  const float u = Q.u, v = Q.v, radius = Q.radius;
  if (checkBounds && (u < minX || u > maxX || v < minY || v > maxY)) return false;
  c0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, minX), radius), gwInv)));
  if (c0 >= GRID_COLS) return false;
  c1 = min(GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, minX), radius), gwInv)));
  if (c1 < 0) return false;
  r0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, minY), radius), ghInv)));
  if (r0 >= GRID_ROWS) return false;
  r1 = min(GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, minY), radius), ghInv)));
  return r1 >= 0;
}

// key of keypoint i2 for query Q (~0: not a candidate); everything except "already taken"
__device__ __forceinline__ unsigned long long proj_key(const pli_proj_query& Q, const uint64_t dq[4], int i2,
                                                       const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc,
                                                       const float* __restrict__ uright, float minX, float minY, float gwInv,
                                                       float ghInv, int c0, int c1, int r0, int r1) {
  const pli_keypoint k = kp[i2];
  const int px = (int)roundf(__fmul_rn(__fsub_rn(k.x, minX), gwInv));
  const int py = (int)roundf(__fmul_rn(__fsub_rn(k.y, minY), ghInv));
  if (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) return ~0ull;   // PosInGrid
  if (px < c0 || px > c1 || py < r0 || py > r1) return ~0ull;
  if ((Q.min_level > 0) || (Q.max_level >= 0)) {
    if (k.octave < Q.min_level) return ~0ull;
    if (Q.max_level >= 0 && k.octave > Q.max_level) return ~0ull;
  }
  if (!(fabsf(__fsub_rn(k.x, Q.u)) < Q.radius && fabsf(__fsub_rn(k.y, Q.v)) < Q.radius)) return ~0ull;
  const float ur2 = uright[i2];
  if (ur2 > 0 && fabsf(__fsub_rn(Q.ur, ur2)) > Q.radius) return ~0ull;
  uint64_t d2[4];
  load_desc(desc + (int64_t)i2 * 32, d2);
  const int dist = hamming256(dq, d2);
  return ((unsigned long long)dist << 40) | ((unsigned long long)px << 34) | ((unsigned long long)py << 28) | (unsigned long long)i2;
}

__device__ __forceinline__ void proj_candidates_dev(int i, int lane, const pli_proj_query* __restrict__ q,
                                                    const uint8_t* __restrict__ qdesc, int nq,
                                                    const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc,
                                                    const float* __restrict__ uright, int ncur, float minX, float maxX,
                                                    float minY, float maxY, int checkBounds, int distLimit,
                                                    unsigned long long* __restrict__ candKeys, int* __restrict__ candCount,
                                                    int* __restrict__ windowOpen = nullptr /* nq, or null */) {
  if (i >= nq) return;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(maxX, minX));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(maxY, minY));
  const pli_proj_query Q = q[i];
  int c0, c1, r0, r1;
  int count = 0;
  bool open = false;                                    // GetFeaturesInArea returns something: before "taken" and before any distance
  if (proj_window(Q, minX, maxX, minY, maxY, gwInv, ghInv, checkBounds != 0, c0, c1, r0, r1)) {
    uint64_t dq[4];
    load_desc(qdesc + (int64_t)i * 32, dq);
    for (int b = 0; b < ncur; b += 64) {
      const int i2 = b + lane;
      unsigned long long key = ~0ull;
      if (i2 < ncur) key = proj_key(Q, dq, i2, kp, desc, uright, minX, minY, gwInv, ghInv, c0, c1, r0, r1);
      const bool keep = key != ~0ull && (int)(key >> 40) <= distLimit;
      if (windowOpen) open = open || __builtin_amdgcn_ballot_w64(key != ~0ull) != 0ull;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
      const int pos = count + __popcll(bal & ((1ull << lane) - 1ull));
      if (keep && pos < PROJ_K) candKeys[(int64_t)i * PROJ_K + pos] = key;
      count += __popcll(bal);
    }
  }
  if (lane == 0) candCount[i] = count <= PROJ_K ? count : -1;
  if (windowOpen && lane == 0) windowOpen[i] = open ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_proj_candidates(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc,
                                                        int nq, const pli_keypoint* __restrict__ kp,
                                                        const uint8_t* __restrict__ desc, const float* __restrict__ uright,
                                                        int ncur, float minX, float maxX, float minY, float maxY,
                                                        int checkBounds, int distLimit, unsigned long long* __restrict__ candKeys,
                                                        int* __restrict__ candCount) {
  proj_candidates_dev(blockIdx.x, threadIdx.x, q, qdesc, nq, kp, desc, uright, ncur, minX, maxX, minY, maxY, checkBounds, distLimit,
                      candKeys, candCount);
}

// The projection searches keep a match out of the rotation histogram, and reject it in the filter, when its bin lies outside
// 0..HISTO_LENGTH-1 (angles outside [0, 360)): -1
__device__ __forceinline__ int proj_rot_bin(float qAngle, float kpAngle) {
  const int bin = rot_bin(qAngle, kpAngle);
  return (bin >= 0 && bin < HISTO_LENGTH) ? bin : -1;
}

// The ordered phase of both searches, one wave.  mode 0: SearchByProjection(CurrentFrame, LastFrame) (ORBmatcher.cc:2179-2323);
// mode 1: (Frame, MapPoints) (:44-143).
// owner: ncur ints: -1 free, else the query that took the keypoint (INT_MAX: occupied before).  kOwnerInLds says where the caller
// keeps them; the only difference is the fence that orders a query's owner store before the next query's owner loads.
// candCount null: no candidate lists, every query scans the frame.
// kCamera (mode 0) 1 / 2: the walk of the left / right camera of a two-camera frame (k_proj2_assign below).  The right walk leaves
// out the queries whose skipUnless[i] is 0 and has no image gate (ORBmatcher.cc:2086); the rotation filter waits for the other
// camera, so either walk leaves its histogram in histOut[HISTO_LENGTH], the matches before the filter in bestIdx2 and their
// number in *nmatchesOut.
template <bool kOwnerInLds, int kCamera = 0>
__device__ __forceinline__ void proj_assign_dev(int lane, int* owner, const pli_proj_query* __restrict__ q,
                                                const uint8_t* __restrict__ qdesc, int nq,
                                                const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc,
                                                const float* __restrict__ uright, const uint8_t* __restrict__ occupied,
                                                int ncur, float minX, float maxX, float minY, float maxY, int mode,
                                                int checkOri, float nnratio, const unsigned long long* __restrict__ candKeys,
                                                const int* __restrict__ candCount, int* __restrict__ bestIdx2,
                                                int* __restrict__ nmatchesOut, int* __restrict__ rawIdx2 /* mode 0, or null */,
                                                const int* __restrict__ skipUnless = nullptr, int* __restrict__ histOut = nullptr) {
  __shared__ int hist[HISTO_LENGTH];
  __shared__ int keep[HISTO_LENGTH];
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(maxX, minX));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(maxY, minY));
  for (int i = lane; i < ncur; i += 64) owner[i] = (occupied && occupied[i]) ? INT_MAX : -1;
  for (int i = lane; i < nq; i += 64) bestIdx2[i] = -1;
  if (lane < HISTO_LENGTH) hist[lane] = 0;
  __syncthreads();
  int nmatches = 0;
  int cntNext = !candCount ? -1 : nq > 0 ? candCount[0] : 0;
  unsigned long long keyNext = (nq > 0 && lane < cntNext) ? candKeys[lane] : ~0ull;
  for (int i = 0; i < nq; ++i) {
    const int cnt = cntNext;
    unsigned long long key = keyNext;
    if (candCount && i + 1 < nq) {                      // the next query's keys travel while this one is decided
      cntNext = candCount[i + 1];
      keyNext = lane < cntNext ? candKeys[(int64_t)(i + 1) * PROJ_K + lane] : ~0ull;
    }
    if (kCamera == 2 && !skipUnless[i]) continue;                   // (nothing was stored: no fence needed)
    WaveTop2 top;
    if (cnt >= 0) {
      if (key != ~0ull && owner[(int)(key & 0xFFFFFFFull)] >= 0) key = ~0ull;
      top.push(key);
    } else {                                            // no list, or more than PROJ_K candidates: scan the frame for this query
      const pli_proj_query Q = q[i];
      int c0, c1, r0, r1;
      if (proj_window(Q, minX, maxX, minY, maxY, gwInv, ghInv, mode == 0 && kCamera != 2, c0, c1, r0, r1)) {
        uint64_t dq[4];
        load_desc(qdesc + (int64_t)i * 32, dq);
        for (int i2 = lane; i2 < ncur; i2 += 64) {
          const unsigned long long kk = proj_key(Q, dq, i2, kp, desc, uright, minX, minY, gwInv, ghInv, c0, c1, r0, r1);
          // not a candidate (~0), or all 256 bits differ: never below the reference's initial bestDist = bestDist2 = 256
          if ((int)(kk >> 40) >= 256 || owner[i2] >= 0) continue;
          top.push(kk);
        }
      }
    }
    const unsigned long long m1 = top.min1();
    if (m1 != ~0ull && (int)(m1 >> 40) <= 100) {
      const int b1 = (int)(m1 & 0xFFFFFFFull);
      bool accept = true;
      if (mode == 1) {
        const unsigned long long m2 = top.min2(m1);
        const int bestDist = (int)(m1 >> 40), bestLevel = kp[b1].octave;
        int bestDist2 = 256, bestLevel2 = -1;
        if (m2 != ~0ull) { bestDist2 = (int)(m2 >> 40); bestLevel2 = kp[(int)(m2 & 0xFFFFFFFull)].octave; }
        accept = !(bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2));
      }
      if (accept) {
        // (every lane stores the same value.  Mode 0: a query whose map point has no observations — bit 1 of `valid` — does not take
        // its keypoint away from the queries behind it, ORBmatcher.cc:2259-2261)
        if (mode == 1 || !(q[i].valid & 2)) owner[b1] = i;
        bestIdx2[i] = b1;
        if (mode == 0 && checkOri && lane == 0) {
          const int bin = proj_rot_bin(q[i].angle, kp[b1].angle);
          if (bin >= 0) hist[bin]++;
        }
        ++nmatches;
      }
    }
    if (kOwnerInLds) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // single wave: LDS is executed in order
    } else {
      __threadfence_block();                                   // global memory: the store is visible before the next query's loads
      __syncthreads();
    }
  }
  __syncthreads();
  if (kCamera != 0) {
    if (lane < HISTO_LENGTH) histOut[lane] = hist[lane];
  } else if (mode == 0) {
    if (checkOri) {
      if (lane == 0) {
        int ind1, ind2, ind3;
        three_maxima(hist, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; ++i) keep[i] = (i == ind1 || i == ind2 || i == ind3);
      }
      __syncthreads();
    }
    // the rotation filter, per accepted query (:2303-2320: every entry of a rejected bin takes one off nmatches)
    int removed = 0;
    for (int i = lane; i < nq; i += 64) {
      const int b = bestIdx2[i];
      if (rawIdx2) rawIdx2[i] = b;
      if (b < 0 || !checkOri) continue;
      const int bin = proj_rot_bin(q[i].angle, kp[b].angle);
      if (bin < 0 || !keep[bin]) { bestIdx2[i] = -1; ++removed; }
    }
    removed = wave_sum_i32(removed);
    nmatches -= removed;
  }
  if (lane == 0) *nmatchesOut = nmatches;
}

// frames of up to PROJ_LDS_KEYPOINTS keypoints, after k_proj_candidates; LDS: ncur ints
__global__ __launch_bounds__(64) void k_proj_assign(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq,
                                                    const pli_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc,
                                                    const float* __restrict__ uright, const uint8_t* __restrict__ occupied,
                                                    int ncur, float minX, float maxX, float minY, float maxY, int mode,
                                                    int checkOri, float nnratio, const unsigned long long* __restrict__ candKeys,
                                                    const int* __restrict__ candCount, int* __restrict__ bestIdx2,
                                                    int* __restrict__ nmatchesOut, int* __restrict__ rawIdx2) {
  extern __shared__ int owner[];
  proj_assign_dev<true>(threadIdx.x, owner, q, qdesc, nq, kp, desc, uright, occupied, ncur, minX, maxX, minY, maxY, mode, checkOri,
                        nnratio, candKeys, candCount, bestIdx2, nmatchesOut, rawIdx2);
}

// larger frames: no candidate lists, the owner table in global memory
__global__ __launch_bounds__(64) void k_proj_assign_scan(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc,
                                                         int nq, const pli_keypoint* __restrict__ kp,
                                                         const uint8_t* __restrict__ desc, const float* __restrict__ uright,
                                                         const uint8_t* __restrict__ occupied, int ncur, float minX, float maxX,
                                                         float minY, float maxY, int mode, int checkOri, float nnratio,
                                                         int* __restrict__ owner /* ncur */, int* __restrict__ bestIdx2,
                                                         int* __restrict__ nmatchesOut, int* __restrict__ rawIdx2) {
  proj_assign_dev<false>(threadIdx.x, owner, q, qdesc, nq, kp, desc, uright, occupied, ncur, minX, maxX, minY, maxY, mode, checkOri,
                         nnratio, nullptr, nullptr, bestIdx2, nmatchesOut, rawIdx2);
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for a current frame of two cameras (ORBmatcher.cc:1961-2177
// with CurrentFrame.Nleft != -1).  The left search reads and writes only the left half of CurrentFrame.mvpMapPoints and the right
// search only the right half, so the two ordered walks never see each other's writes.  What couples them is (a) the left
// `continue`s of :2004-2007 and :2024, which leave the right camera unsearched too and depend on the geometry alone — the
// windowOpen flag of the left candidates — and (b) the one rotation histogram.  So: candidates of every (query, camera) in
// parallel, the two walks side by side (one wave each, owner table in LDS), then one wave that adds the histograms and filters.
//   q: [2][nq] (left, then right with valid and angle of the left), keys [2][nq][PROJ_K], cnt / best / raw [2][nq],
//   hist [2][HISTO_LENGTH], accepts [2]; noUright: max(nL, nR) floats of -1 (this branch has no mvuRight gate, :2040)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_proj2_candidates(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq,
                                                         const pli_keypoint* __restrict__ kpL, const uint8_t* __restrict__ descL, int nL,
                                                         const pli_keypoint* __restrict__ kpR, const uint8_t* __restrict__ descR, int nR,
                                                         const float* __restrict__ noUright, float minX, float maxX, float minY,
                                                         float maxY, unsigned long long* __restrict__ candKeys,
                                                         int* __restrict__ candCount, int* __restrict__ leftOpen) {
  const int cam = blockIdx.y;
  // (the image gate :2004-2007 is the left projection's; the right projection has none, :2086)
  proj_candidates_dev(blockIdx.x, threadIdx.x, q + (int64_t)cam * nq, qdesc, nq, cam ? kpR : kpL, cam ? descR : descL, noUright,
                      cam ? nR : nL, minX, maxX, minY, maxY, cam ? 0 : 1, 100, candKeys + (int64_t)cam * nq * PROJ_K,
                      candCount + (int64_t)cam * nq, cam ? nullptr : leftOpen);
}

// grid 2: block = camera; LDS: max(nL, nR) ints
__global__ __launch_bounds__(64) void k_proj2_assign(const pli_proj_query* __restrict__ q, const uint8_t* __restrict__ qdesc, int nq,
                                                     const pli_keypoint* __restrict__ kpL, const uint8_t* __restrict__ descL,
                                                     const uint8_t* __restrict__ occL, int nL, const pli_keypoint* __restrict__ kpR,
                                                     const uint8_t* __restrict__ descR, const uint8_t* __restrict__ occR, int nR,
                                                     const float* __restrict__ noUright, float minX, float maxX, float minY, float maxY,
                                                     int checkOri, const unsigned long long* __restrict__ candKeys,
                                                     const int* __restrict__ candCount, const int* __restrict__ leftOpen,
                                                     int* __restrict__ rawIdx2, int* __restrict__ hist, int* __restrict__ accepts) {
  extern __shared__ int owner[];
  const int cam = blockIdx.x;
  if (cam == 0)
    proj_assign_dev<true, 1>(threadIdx.x, owner, q, qdesc, nq, kpL, descL, noUright, occL, nL, minX, maxX, minY, maxY, 0, checkOri, 0.0f,
                             candKeys, candCount, rawIdx2, accepts, nullptr, nullptr, hist);
  else
    proj_assign_dev<true, 2>(threadIdx.x, owner, q + nq, qdesc, nq, kpR, descR, noUright, occR, nR, minX, maxX, minY, maxY, 0, checkOri,
                             0.0f, candKeys + (int64_t)nq * PROJ_K, candCount + nq, rawIdx2 + nq, accepts + 1, nullptr, leftOpen,
                             hist + HISTO_LENGTH);
}

// one wave: ComputeThreeMaxima on the joint histogram, then the filter :2163-2173 over both cameras' matches
__global__ __launch_bounds__(64) void k_proj2_finish(const pli_proj_query* __restrict__ q, int nq, const pli_keypoint* __restrict__ kpL,
                                                     const pli_keypoint* __restrict__ kpR, int checkOri,
                                                     const int* __restrict__ rawIdx2, const int* __restrict__ hist,
                                                     const int* __restrict__ accepts, int* __restrict__ bestIdx2,
                                                     int* __restrict__ nmatchesOut) {
  __shared__ int joint[HISTO_LENGTH];
  __shared__ int keep[HISTO_LENGTH];
  const int lane = threadIdx.x;
  if (lane < HISTO_LENGTH) joint[lane] = hist[lane] + hist[HISTO_LENGTH + lane];
  __syncthreads();
  if (checkOri && lane == 0) {
    int ind1, ind2, ind3;
    three_maxima(joint, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; ++i) keep[i] = (i == ind1 || i == ind2 || i == ind3);
  }
  __syncthreads();
  int removed = 0;
  for (int cam = 0; cam < 2; ++cam) {
    const pli_keypoint* kp = cam ? kpR : kpL;
    for (int i = lane; i < nq; i += 64) {
      int b = rawIdx2[(int64_t)cam * nq + i];
      if (b >= 0 && checkOri) {
        const int bin = proj_rot_bin(q[i].angle, kp[b].angle);
        if (bin < 0 || !keep[bin]) { b = -1; ++removed; }
      }
      bestIdx2[(int64_t)cam * nq + i] = b;
    }
  }
  removed = wave_sum_i32(removed);
  if (lane == 0) *nmatchesOut = accepts[0] + accepts[1] - removed;
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th) for a frame of two fisheye cameras (ORBmatcher.cc:44-214 with
// F.Nleft != -1).  The candidates of every (map point, camera)
// come from k_proj_candidates, all in parallel; this wave walks the map points in order — left camera, then right unless
// the left ratio test sent the map point away — with the two halves of F.mvpMapPoints as owner tables in LDS (-1 free,
// INT_MAX taken before the call, else the map point that wrote the slot last), and writes a match to the stereo partner
// of the keypoint as the reference does (mvLeftToRightMatch / mvRightToLeftMatch; the partner's slot is overwritten, taken
// or not).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_proj_assign_fisheye(
    const pli_proj_query* __restrict__ qL, const pli_proj_query* __restrict__ qR, const uint8_t* __restrict__ qdesc, int nq,
    const pli_keypoint* __restrict__ kpL, const uint8_t* __restrict__ descL, const uint8_t* __restrict__ occL,
    const int* __restrict__ l2r, int nL, const pli_keypoint* __restrict__ kpR, const uint8_t* __restrict__ descR,
    const uint8_t* __restrict__ occR, const int* __restrict__ r2l, int nR, const float* __restrict__ noUright, float minX,
    float maxX, float minY, float maxY, float nnratio, const unsigned long long* __restrict__ keysL,
    const int* __restrict__ cntL, const unsigned long long* __restrict__ keysR, const int* __restrict__ cntR,
    int* __restrict__ mpL, int* __restrict__ mpR, int* __restrict__ nmatchesOut) {
  extern __shared__ int owner[];                         // [nL] left slots, [nR] right slots
  int* ownL = owner;
  int* ownR = owner + nL;
  const int lane = threadIdx.x;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(maxX, minX));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(maxY, minY));
  for (int i = lane; i < nL; i += 64) ownL[i] = (occL && occL[i]) ? INT_MAX : -1;
  for (int i = lane; i < nR; i += 64) ownR[i] = (occR && occR[i]) ? INT_MAX : -1;
  __syncthreads();
  int nmatches = 0;
  // best and second best of one camera among the free keypoints; returns 0 nothing within TH_HIGH, 1 accepted (b1), 2 the
  // ratio test failed (ORBmatcher.cc:124-126 / :197-199)
  auto search = [&](int i, const pli_proj_query* q, const pli_keypoint* kp, const uint8_t* desc, int ncur, const int* own,
                    const unsigned long long* keys, const int* cnts, int& b1) -> int {
    const int cnt = cnts[i];
    WaveTop2 top;
    if (cnt >= 0) {
      unsigned long long key = lane < cnt ? keys[(int64_t)i * PROJ_K + lane] : ~0ull;
      if (key != ~0ull && own[(int)(key & 0xFFFFFFFull)] >= 0) key = ~0ull;
      top.push(key);
    } else {                                             // more than PROJ_K candidates: scan the camera for this query
      const pli_proj_query Q = q[i];
      int c0, c1, r0, r1;
      if (proj_window(Q, minX, maxX, minY, maxY, gwInv, ghInv, false, c0, c1, r0, r1)) {
        uint64_t dq[4];
        load_desc(qdesc + (int64_t)i * 32, dq);
        for (int i2 = lane; i2 < ncur; i2 += 64) {
          if (own[i2] >= 0) continue;
          top.push(proj_key(Q, dq, i2, kp, desc, noUright, minX, minY, gwInv, ghInv, c0, c1, r0, r1));
        }
      }
    }
    const unsigned long long m1 = top.min1();
    if (m1 == ~0ull || (int)(m1 >> 40) > 100) return 0;
    b1 = (int)(m1 & 0xFFFFFFFull);
    const unsigned long long m2 = top.min2(m1);
    const int bestDist = (int)(m1 >> 40), bestLevel = kp[b1].octave;
    int bestDist2 = 256, bestLevel2 = -1;
    if (m2 != ~0ull) { bestDist2 = (int)(m2 >> 40); bestLevel2 = kp[(int)(m2 & 0xFFFFFFFull)].octave; }
    return (bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(nnratio, (float)bestDist2)) ? 2 : 1;
  };
  for (int i = 0; i < nq; ++i) {
    int b1 = -1;
    bool leave = false;
    if (qL[i].valid) {
      const int r = search(i, qL, kpL, descL, nL, ownL, keysL, cntL, b1);
      if (r == 2) leave = true;
      if (r == 1) {
        ownL[b1] = i;                                     // every lane stores the same value
        const int p = l2r[b1];
        if (p != -1) { ownR[p] = i; ++nmatches; }
        ++nmatches;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // single wave: LDS is executed in order
    }
    if (!leave && qR[i].valid) {
      const int r = search(i, qR, kpR, descR, nR, ownR, keysR, cntR, b1);
      if (r == 1) {
        const int p = r2l[b1];
        if (p != -1) { ownL[p] = i; ++nmatches; }
        ownR[b1] = i;
        ++nmatches;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
  }
  __syncthreads();
  for (int i = lane; i < nL; i += 64) { const int o = ownL[i]; mpL[i] = (o >= 0 && o != INT_MAX) ? o : -1; }
  for (int i = lane; i < nR; i += 64) { const int o = ownR[i]; mpR[i] = (o >= 0 && o != INT_MAX) ? o : -1; }
  if (lane == 0) *nmatchesOut = nmatches;
}

// ---------------------------------------------------------------------------
// Frame-to-frame track matching of a whole batch on the device tables (pli_batch_track): frame i against frame i-1.
//   k_track_queries     the projection part of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono, match12)
//                       (ORBmatcher.cc:2190-2244: fx*xc*invzc + cx; the overload without match12 has Pinhole::project)
//                       with LastFrame's stereo points standing for its map points
//                       (Frame::UnprojectStereo, Frame.cc:1334-1350, as Tracking::UpdateLastFrame creates them)
//   k_track_candidates / k_track_assign   the two-phase search above, one launch for all frame pairs
//   k_track_lines       match(last.mDescriptors_Line, cur.mDescriptors_Line, nnr, matches_12) (LineMatcher.cpp:201-229)
// cv::Mat arithmetic (CV_32F): a product A*B (+ C) is OpenCV's gemm, restated here as double accumulation of the float
// products, then ONE rounding to float ("OpenCV-3.3.1-compatible by intent", like the other OpenCV primitives).
// ---------------------------------------------------------------------------

__device__ __forceinline__ float cvmat_dot3(const float* a, int sa, const float* b, double alpha, double c) {
  const double d = (double)a[0] * (double)b[0] + (double)a[sa] * (double)b[1] + (double)a[2 * sa] * (double)b[2];
  return (float)(alpha * d + c);
}

__global__ __launch_bounds__(256) void k_track_queries(const DevParams* __restrict__ Pp, const uint8_t* __restrict__ table,
                                                       const float* __restrict__ poses, TrackParams tp,
                                                       pli_proj_query* __restrict__ qAll) {
  const DevParams& P = *Pp;
  const int frame = blockIdx.y + 1, j = blockIdx.x * 256 + threadIdx.x;     // frame >= 1 is matched against frame - 1
  const uint8_t* last = table + (int64_t)(frame - 1) * tp.recordBytes;
  const int nq = reinterpret_cast<const int*>(last + tp.offCounts)[0];
  if (j >= nq) return;
  const float* Tc = poses + (int64_t)frame * 12;        // mTcw of the current frame, row major 3x4
  const float* Tl = poses + (int64_t)(frame - 1) * 12;  // mTcw of the last frame
  const float tcw[3] = {Tc[3], Tc[7], Tc[11]}, tlw[3] = {Tl[3], Tl[7], Tl[11]};
  // twc = -Rcw.t()*tcw; tlc = Rlw*twc+tlw (ORBmatcher.cc:2193-2200)
  float twc[3], tlc[3];
  for (int r = 0; r < 3; ++r) twc[r] = cvmat_dot3(Tc + r, 4, tcw, -1.0, 0.0);
  for (int r = 0; r < 3; ++r) tlc[r] = cvmat_dot3(Tl + 4 * r, 1, twc, 1.0, (double)tlw[r]);
  const float mb = __fdiv_rn(tp.bf, tp.fx);             // Frame.cc:197
  const bool bForward = tlc[2] > mb && !tp.mono, bBackward = -tlc[2] > mb && !tp.mono;
  const pli_keypoint k = reinterpret_cast<const pli_keypoint*>(last + tp.offKp0)[j];
  const float z = reinterpret_cast<const float*>(last + tp.offDepth)[j];
  pli_proj_query Q;
  Q.u = 0.f; Q.v = 0.f; Q.radius = 0.f; Q.ur = 0.f; Q.min_level = 0; Q.max_level = -1; Q.angle = k.angle; Q.valid = 0;
  if (z > 0) {
    // LastFrame.UnprojectStereo(j): x3Dc = ((u-cx)*z*invfx, (v-cy)*z*invfy, z); x3Dw = mRwc*x3Dc+mOw with mRwc = Rlw.t(), mOw = -Rlw.t()*tlw
    const float invfx = __fdiv_rn(1.0f, tp.fx), invfy = __fdiv_rn(1.0f, tp.fy);
    const float xl[3] = {__fmul_rn(__fmul_rn(__fsub_rn(k.x, tp.cx), z), invfx), __fmul_rn(__fmul_rn(__fsub_rn(k.y, tp.cy), z), invfy), z};
    float Ow[3], xw[3], xc[3];
    for (int r = 0; r < 3; ++r) Ow[r] = cvmat_dot3(Tl + r, 4, tlw, -1.0, 0.0);
    for (int r = 0; r < 3; ++r) xw[r] = cvmat_dot3(Tl + r, 4, xl, 1.0, (double)Ow[r]);
    // x3Dc = Rcw*x3Dw+tcw (ORBmatcher.cc:2212)
    for (int r = 0; r < 3; ++r) xc[r] = cvmat_dot3(Tc + 4 * r, 1, xw, 1.0, (double)tcw[r]);
    const float invzc = (float)(1.0 / (double)xc[2]);
    if (!(invzc < 0)) {
      Q.u = __fadd_rn(__fmul_rn(__fmul_rn(tp.fx, xc[0]), invzc), tp.cx);
      Q.v = __fadd_rn(__fmul_rn(__fmul_rn(tp.fy, xc[1]), invzc), tp.cy);
      Q.radius = __fmul_rn(tp.th, P.lv[k.octave].scale);
      Q.ur = __fsub_rn(Q.u, __fmul_rn(tp.bf, invzc));
      if (bForward) { Q.min_level = k.octave; Q.max_level = -1; }
      else if (bBackward) { Q.min_level = 0; Q.max_level = k.octave; }
      else { Q.min_level = k.octave - 1; Q.max_level = k.octave + 1; }
      Q.valid = 1;
    }
  }
  qAll[(int64_t)frame * tp.kpCap + j] = Q;
}

__global__ __launch_bounds__(64) void k_track_candidates(const uint8_t* __restrict__ table, TrackParams tp,
                                                         const pli_proj_query* __restrict__ qAll,
                                                         unsigned long long* __restrict__ candKeysAll, int* __restrict__ candCountAll) {
  const int frame = blockIdx.y + 1;
  const uint8_t* last = table + (int64_t)(frame - 1) * tp.recordBytes;
  const uint8_t* cur = table + (int64_t)frame * tp.recordBytes;
  const int nq = reinterpret_cast<const int*>(last + tp.offCounts)[0], ncur = reinterpret_cast<const int*>(cur + tp.offCounts)[0];
  proj_candidates_dev(blockIdx.x, threadIdx.x, qAll + (int64_t)frame * tp.kpCap, last + tp.offDesc0, nq,
                      reinterpret_cast<const pli_keypoint*>(cur + tp.offKp0), cur + tp.offDesc0,
                      reinterpret_cast<const float*>(cur + tp.offUr), ncur, tp.minX, tp.maxX, tp.minY, tp.maxY, 1, 100,
                      candKeysAll + (int64_t)frame * tp.kpCap * PROJ_K, candCountAll + (int64_t)frame * tp.kpCap);
}

__global__ __launch_bounds__(64) void k_track_assign(const uint8_t* __restrict__ table, TrackParams tp,
                                                     const pli_proj_query* __restrict__ qAll,
                                                     const unsigned long long* __restrict__ candKeysAll,
                                                     const int* __restrict__ candCountAll, uint8_t* __restrict__ track) {
  extern __shared__ int owner[];
  const int frame = blockIdx.x + 1;
  const uint8_t* last = table + (int64_t)(frame - 1) * tp.recordBytes;
  const uint8_t* cur = table + (int64_t)frame * tp.recordBytes;
  uint8_t* out = track + (int64_t)frame * tp.trackBytes;
  const int nq = reinterpret_cast<const int*>(last + tp.offCounts)[0], ncur = reinterpret_cast<const int*>(cur + tp.offCounts)[0];
  int* counts = reinterpret_cast<int*>(out + tp.toffCounts);
  if (threadIdx.x == 0) counts[0] = nq;
  proj_assign_dev<true>(threadIdx.x, owner, qAll + (int64_t)frame * tp.kpCap, last + tp.offDesc0, nq,
                  reinterpret_cast<const pli_keypoint*>(cur + tp.offKp0), cur + tp.offDesc0,
                  reinterpret_cast<const float*>(cur + tp.offUr), nullptr, ncur, tp.minX, tp.maxX, tp.minY, tp.maxY, 0, tp.checkOri, 0.f,
                  candKeysAll + (int64_t)frame * tp.kpCap * PROJ_K, candCountAll + (int64_t)frame * tp.kpCap,
                  reinterpret_cast<int*>(out + tp.toffBest), counts + 1, nullptr);
}

// one workgroup per frame pair: knn2 both ways, ratio tests, mutual check (descriptor tables of <= klCap lines)
__global__ __launch_bounds__(256) void k_track_lines(const uint8_t* __restrict__ table, TrackParams tp, int bestLR,
                                                     int* __restrict__ scratch, uint8_t* __restrict__ track) {
  __shared__ int s_cnt;
  const int frame = blockIdx.x + 1, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint8_t* last = table + (int64_t)(frame - 1) * tp.recordBytes;
  const uint8_t* cur = table + (int64_t)frame * tp.recordBytes;
  uint8_t* out = track + (int64_t)frame * tp.trackBytes;
  const int n1 = reinterpret_cast<const int*>(last + tp.offCounts)[2], n2 = reinterpret_cast<const int*>(cur + tp.offCounts)[2];
  const uint8_t* d1 = last + tp.offLd0;
  const uint8_t* d2 = cur + tp.offLd0;
  int* m12 = reinterpret_cast<int*>(out + tp.toffLines);
  int* m21 = scratch + (int64_t)frame * tp.klCap;
  if (tid == 0) s_cnt = 0;
  for (int dir = 0; dir < (bestLR ? 2 : 1); ++dir) {
    const uint8_t* q = dir ? d2 : d1;
    const uint8_t* t = dir ? d1 : d2;
    const int nq = dir ? n2 : n1, nt = dir ? n1 : n2;
    int* m = dir ? m21 : m12;
    for (int i = wv; i < nq; i += 4) {
      uint64_t dq[4];
      load_desc(q + (int64_t)i * 32, dq);
      WaveTop2 top;
      for (int j = lane; j < nt; j += 64) {
        uint64_t dt[4];
        load_desc(t + (int64_t)j * 32, dt);
        top.push(((unsigned long long)hamming256(dq, dt) << 32) | (unsigned)j);
      }
      const unsigned long long m1 = top.min1(), m2 = top.min2(m1);
      if (lane == 0) {
        int r = -1;
        if (nt >= 2 && (float)(int)(m1 >> 32) < __fmul_rn((float)(int)(m2 >> 32), tp.nnrLines)) r = (int)(m1 & 0xFFFFFFFFu);
        m[i] = r;
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  int ok = 0;
  for (int i = tid; i < n1; i += 256) {
    int i2 = m12[i];
    if (i2 >= 0 && bestLR && n2 > 0 && m21[i2] != i) { m12[i] = -1; i2 = -1; }
    ok += i2 >= 0;
  }
  if (ok) atomicAdd(&s_cnt, ok);
  __syncthreads();
  if (tid == 0) {
    int* counts = reinterpret_cast<int*>(out + tp.toffCounts);
    counts[2] = n1;
    counts[3] = s_cnt;
  }
}

// ---------------------------------------------------------------------------
// DBoW2 vocabulary descent (TemplatedVocabulary.h:1230-1272): one wave per feature; at every level the lanes take
// one child each (k <= 64), a 64-bit (distance, position) key wave-min picks the nearest child, the first on ties.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bow_descend(const uint8_t* __restrict__ feat, int n, const int* __restrict__ childOff,
                                                    const int* __restrict__ childList, const uint8_t* __restrict__ nodeDesc,
                                                    const int* __restrict__ nodeWord, const double* __restrict__ nodeWeight,
                                                    int nidLevel, int* __restrict__ wordId, double* __restrict__ weight,
                                                    int* __restrict__ nodeId) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  uint64_t f[4];
  load_desc(feat + (int64_t)i * 32, f);
  int cur = 0, level = 0, nid = 0;
  for (;;) {
    const int c0 = childOff[cur], c1 = childOff[cur + 1];
    if (c0 == c1) break;                                   // Node::isLeaf(): no children
    ++level;
    unsigned long long best = ~0ull;
    for (int c = c0 + lane; c < c1; c += 64) {
      uint64_t d[4];
      load_desc(nodeDesc + (int64_t)childList[c] * 32, d);
      const unsigned long long key = ((unsigned long long)hamming256(f, d) << 32) | (unsigned)(c - c0);
      best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    cur = childList[c0 + (int)(best & 0xFFFFFFFFull)];
    if (level == nidLevel) nid = cur;
  }
  if (lane == 0) {
    wordId[i] = nodeWord[cur];
    weight[i] = nodeWeight[cur];
    nodeId[i] = nid;
  }
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:269-470, F.Nleft == -1 branch) for a batch of
// keyframes against one frame (Tracking::Relocalization's loop, Tracking.cc:4205-4230).
//
// Why the reference's sequential walk may run in parallel: a feature is listed in ONE node of its FeatureVector (DBoW2's
// addFeature runs once per feature), and only keyframe features of that same node are compared with it.  The walk's only state
// besides its outputs is "frame feature already matched in this call" (vpMapPointMatches[realIdxF] set), and a frame feature can
// only be matched by a keyframe feature of its own node, so that state never crosses a node: the common nodes are independent of
// each other, the keyframes are independent of each other, and only the keyframe features inside one node must be taken in list
// order (ascending index).  The rotation histogram and nmatches are sums over the matches: their order does not matter.
//
//   k_node_sort        (below, shared by the three node searches) one workgroup: the frame's features sorted by node id; the
//                      order inside a node does not matter, the candidate key below carries the index; unlisted ones (-1) last.
//   k_search_by_bow    one workgroup per keyframe: its valid features whose node the frame lists become (first position of the
//                      node in the sorted frame list, index) keys, sorted in LDS: runs of one common node in ascending index.
//                      The waves take 64-key chunks in turn and walk every run that starts in their chunk, keyframe feature after
//                      keyframe feature; the lanes hold the node's frame candidates (looping over more than 64).  The reference's
//                      running best / second best (strict <: ties keep the first listed, the lowest index) are the two smallest
//                      (distance, frame index) keys.  Which keyframe feature took a frame feature lives in LDS; the 30-bin
//                      rotation histogram takes LDS atomics, and thread 0 runs three_maxima before all
//                      threads write the row with the filter applied.
// ---------------------------------------------------------------------------
constexpr int BOW_TH_LOW = 50;
constexpr int TRI_STAT = 32;                                     // SearchForTriangulation, ints per neighbour: 30 bins, [30] the match counter

__device__ __forceinline__ int pow2_ceil(int m) {
  int n = 1;
  while (n < m) n <<= 1;
  return n;
}

// ascending bitonic sort of n (a power of two) keys in LDS by the whole block; the payload (may be NULL) moves with its key
__device__ void lds_bitonic_sort(uint32_t* key, uint16_t* val, int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const uint32_t a = key[i], b = key[l];
          if ((a > b) == ((i & k) == 0)) {
            key[i] = b; key[l] = a;
            if (val) { const uint16_t t = val[i]; val[i] = val[l]; val[l] = t; }
          }
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int bow_lower_bound(const uint32_t* a, int lo, int hi, uint32_t v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// SearchByBoW and SearchForTriangulation clamp a bin outside 0..HISTO_LENGTH-1 (the caller checks the angles; this only keeps
// the histogram index in range)
__device__ __forceinline__ int bow_rot_bin(float kfAngle, float fAngle) {
  return min(max(rot_bin(kfAngle, fAngle), 0), HISTO_LENGTH - 1);
}

// The candidate side of SearchByBoW(KF, F), SearchByBoW(KF, KF) and SearchForTriangulation: one workgroup per table (grid =
// tables), its features that may be taken sorted by node id (LDS bitonic sort of (node, index) pairs), the others last
// (0xFFFFFFFF); nListed = how many may be taken, 0 when none.  Table t is rows kfOff[t] .. kfOff[t + 1]; kfOff == NULL: one table,
// rows 0 .. nkOne (the frame of SearchByBoW(KF, F)).  A feature may be taken when it is listed in a node (node >= 0), (kfFlag != 0)
// == (flagWanted != 0) and, with onlyStereo, kfStereo is set; kfFlag == NULL: every listed feature.  SearchForTriangulation passes
// "has a map point" and 0, SearchByBoW(KF, KF) "map point set and not bad" and 1; stat (NULL: none) is SearchForTriangulation's
// histogram and counter, cleared here.  keyCap = a power of two >= every table's feature count (<= 8192); LDS: keyCap * 6 bytes.
__global__ __launch_bounds__(1024) void k_node_sort(const int* __restrict__ kfOff, int nkOne, const int* __restrict__ kfNode,
                                                    const uint8_t* __restrict__ kfFlag, int flagWanted,
                                                    const uint8_t* __restrict__ kfStereo, int onlyStereo, int keyCap,
                                                    uint32_t* __restrict__ sNode, uint16_t* __restrict__ sIdx,
                                                    int* __restrict__ nListed, int* __restrict__ stat) {
  extern __shared__ __align__(16) uint32_t nodeSortLds[];
  const int kf = blockIdx.x, base = kfOff ? kfOff[kf] : 0, nk = kfOff ? kfOff[kf + 1] - base : nkOne;
  const int n = min(pow2_ceil(max(nk, 1)), keyCap);
  uint32_t* key = nodeSortLds;
  uint16_t* val = reinterpret_cast<uint16_t*>(key + keyCap);
  if (stat)
    for (int i = threadIdx.x; i < TRI_STAT; i += blockDim.x) stat[kf * TRI_STAT + i] = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    uint32_t k = 0xFFFFFFFFu;
    if (i < nk) {
      const int node = kfNode[base + i];
      if (node >= 0 && (!kfFlag || (kfFlag[base + i] != 0) == (flagWanted != 0)) && (!onlyStereo || kfStereo[base + i])) k = (uint32_t)node;
    }
    key[i] = k;
    val[i] = (uint16_t)i;
  }
  if (threadIdx.x == 0) nListed[kf] = 0;
  __syncthreads();
  lds_bitonic_sort(key, val, n);
  for (int i = threadIdx.x; i < nk; i += blockDim.x) {
    sNode[base + i] = key[i];
    sIdx[base + i] = val[i];
    if (key[i] != 0xFFFFFFFFu && (i + 1 == nk || key[i + 1] == 0xFFFFFFFFu)) nListed[kf] = i + 1;
  }
}

// The ordered walk of both SearchByBoW kernels, by the whole block: key[0..m) (LDS, sorted) holds (first position of a common node in
// the candidate side's sorted list << 16 | walking feature), so a run of equal upper halves is one node's walking features in
// ascending index.  The waves take 64-key chunks in turn and walk every run that starts in their chunk, feature after feature; the
// lanes hold the node's candidates sIdx[lo..hi) (looping over more than 64).  The reference's running best / second best (strict <:
// ties keep the first listed, the lowest index) are the two smallest (distance, candidate index) keys.  owner[candidate] (LDS,
// -1 = free) takes the walking feature of an accepted match (bestDist1 <= maxDist and the ratio test); hist takes its rotation
// bin.  wDesc / wAngle and cDesc / cAngle are the walking and the candidate side's tables.  Returns this wave's accepted matches.
// kTwoCameras (SearchByBoW(KF, F) with F.Nleft != -1, ORBmatcher.cc:342-369, :373-433): the candidates < cNleft (the left camera's)
// and the others keep a top-2 each; only if bestDist1 <= maxDist, the left match is taken on its ratio test and - whether or not it
// was - the right one when bestDist1R <= maxDist, without a ratio test (`|| true`, :405).
template <bool kTwoCameras>
__device__ __forceinline__ int bow_walk(const uint32_t* key, int m, const uint8_t* __restrict__ wDesc, const float* __restrict__ wAngle,
                                        const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx, int nListed,
                                        const uint8_t* __restrict__ cDesc, const float* __restrict__ cAngle, short* owner, int* hist,
                                        int maxDist, float nnratio, int checkOri, int cNleft = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  int nm = 0;
  for (int c0 = wave * 64; c0 < m; c0 += nwaves * 64) {
    const int p = c0 + lane;
    unsigned long long starts = __builtin_amdgcn_ballot_w64(p < m && (p == 0 || (key[p] >> 16) != (key[p - 1] >> 16)));
    while (starts) {
      const int s = c0 + __builtin_ctzll(starts);
      starts &= starts - 1;
      const uint32_t lo = key[s] >> 16;
      const int hi = bow_lower_bound(sNode, (int)lo + 1, nListed, sNode[lo] + 1u);   // (node ids are < 2^31: no wrap)
      for (int q = s; q < m && (key[q] >> 16) == lo; ++q) {
        const int j = (int)(key[q] & 0xFFFFu);
        uint64_t dk[4];
        load_desc(wDesc + (int64_t)j * 32, dk);
        WaveTop2 top, topR;
        for (int t = (int)lo + lane; t < hi; t += 64) {
          const int fi = sIdx[t];
          if (owner[fi] >= 0) continue;                           // matched earlier in this call (:318-319, :345, :884)
          uint64_t df[4];
          load_desc(cDesc + (int64_t)fi * 32, df);
          const unsigned long long k = ((unsigned long long)hamming256(dk, df) << 32) | (unsigned)fi;
          if (kTwoCameras && fi >= cNleft) topR.push(k);          // :361-368
          else top.push(k);
        }
        const unsigned long long m1 = top.min1(), m2 = top.min2(m1);
        if (m1 == ~0ull) continue;                                // (two cameras: bestDist1 == 256 > TH_LOW takes nothing, :373)
        const int bestDist1 = (int)(m1 >> 32), bestDist2 = m2 != ~0ull ? (int)(m2 >> 32) : 256;
        auto take = [&](int fi) {
          owner[fi] = (short)j;                                   // every lane stores the same value
          ++nm;
          if (checkOri && lane == 0) atomicAdd(&hist[bow_rot_bin(wAngle[j], cAngle[fi])], 1);
        };
        if (bestDist1 <= maxDist) {
          bool taken = false;
          if ((float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) { take((int)(m1 & 0xFFFFFFFFull)); taken = true; }
          if (kTwoCameras) {
            const unsigned long long r1 = topR.min1();
            if (r1 != ~0ull && (int)(r1 >> 32) <= maxDist) { take((int)(r1 & 0xFFFFFFFFull)); taken = true; }      // :403-431
          }
          if (taken) __threadfence_block();
        }
      }
    }
  }
  return nm;
}

// The key collection of both SearchByBoW kernels, by the whole block: the walking side's features that take part (valid, and
// listed in a node that the candidate side's sorted list sNode[0..nListed) holds too) become (first position of the node in that
// list << 16 | index) keys, sorted in LDS and padded to a power of two for it.  *count (LDS, 0 at entry) counts them.  Returns m.
__device__ __forceinline__ int bow_collect_keys(const int* __restrict__ wNode, const uint8_t* __restrict__ wValid, int nw,
                                                const uint32_t* __restrict__ sNode, int nListed, uint32_t* key, int* count) {
  const int tid = threadIdx.x;
  for (int j = tid; j < nw; j += blockDim.x) {
    const int node = wNode[j];
    if (!wValid[j] || node < 0) continue;                         // (a feature in no node is never visited)
    const int lo = bow_lower_bound(sNode, 0, nListed, (uint32_t)node);
    if (lo < nListed && sNode[lo] == (uint32_t)node) key[atomicAdd(count, 1)] = ((uint32_t)lo << 16) | (uint32_t)j;
  }
  __syncthreads();
  const int m = *count, n2 = pow2_ceil(m);
  for (int i = m + tid; i < n2; i += blockDim.x) key[i] = 0xFFFFFFFFu;
  __syncthreads();
  lds_bitonic_sort(key, nullptr, n2);
  return m;
}

// The rotation filter's decision, by ONE thread: keep[0..2] = the bins ComputeThreeMaxima keeps (-1: none; all -1 without
// checkOri, where nothing is filtered); returns total less the matches of the dropped bins.
__device__ __forceinline__ int bow_keep_bins(const int* hist, int total, int checkOri, int* keep) {
  int ind1 = -1, ind2 = -1, ind3 = -1;
  if (checkOri) {
    three_maxima(hist, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; ++i)
      if (i != ind1 && i != ind2 && i != ind3) total -= hist[i];
  }
  keep[0] = ind1; keep[1] = ind2; keep[2] = ind3;
  return total;
}

// The body of k_search_by_bow and k_search_by_bow_two_cameras, by the whole block (one keyframe).
template <bool kTwoCameras>
__device__ __forceinline__ void search_by_bow_body(const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc,
                                                   const float* __restrict__ kfAngle, const int* __restrict__ kfNode,
                                                   const uint8_t* __restrict__ kfValid, const uint8_t* __restrict__ fDesc,
                                                   const float* __restrict__ fAngle, const uint32_t* __restrict__ sNode,
                                                   const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, int nf,
                                                   int fNleft, int keyCap, float nnratio, int checkOri, int* __restrict__ matches,
                                                   int* __restrict__ nmatchesOut) {
  extern __shared__ __align__(16) int bowLds[];
  int* hist = bowLds;                                             // 30 bins (32 ints)
  int* misc = bowLds + 32;                                        // [0] keys, [1] matches, [2..4] the bins ComputeThreeMaxima keeps
  uint32_t* key = reinterpret_cast<uint32_t*>(bowLds + 48);
  short* owner = reinterpret_cast<short*>(key + keyCap);          // per frame feature: the keyframe feature that took it, -1 free
  const int tid = threadIdx.x, lane = tid & 63;
  const int kf = blockIdx.x, base = kfOff[kf], nk = kfOff[kf + 1] - base;
  const int nfl = *nListed;
  for (int i = tid; i < 48; i += blockDim.x) bowLds[i] = 0;
  for (int i = tid; i < nf; i += blockDim.x) owner[i] = -1;
  __syncthreads();
  // the keyframe features that take part: map point set and not bad, listed in a node the frame lists too
  const int m = bow_collect_keys(kfNode + base, kfValid + base, nk, sNode, nfl, key, &misc[0]);
  const int nm = bow_walk<kTwoCameras>(key, m, kfDesc + (int64_t)base * 32, kfAngle + base, sNode, sIdx, nfl, fDesc, fAngle, owner, hist,
                                       BOW_TH_LOW, nnratio, checkOri, fNleft);
  if (lane == 0 && nm) atomicAdd(&misc[1], nm);
  __syncthreads();
  if (tid == 0) nmatchesOut[kf] = bow_keep_bins(hist, misc[1], checkOri, misc + 2);
  __syncthreads();
  const int ind1 = misc[2], ind2 = misc[3], ind3 = misc[4];
  int* row = matches + (int64_t)kf * nf;
  for (int i = tid; i < nf; i += blockDim.x) {
    int j = owner[i];
    if (j >= 0 && checkOri) {
      const int b = bow_rot_bin(kfAngle[base + j], fAngle[i]);
      if (b != ind1 && b != ind2 && b != ind3) j = -1;
    }
    row[i] = j;
  }
}

// grid = keyframes; LDS: 48 ints + keyCap keys (a power of two >= every keyframe's feature count) + nf shorts
__global__ __launch_bounds__(512) void k_search_by_bow(const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc,
                                                       const float* __restrict__ kfAngle, const int* __restrict__ kfNode,
                                                       const uint8_t* __restrict__ kfValid, const uint8_t* __restrict__ fDesc,
                                                       const float* __restrict__ fAngle, const uint32_t* __restrict__ sNode,
                                                       const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed, int nf,
                                                       int keyCap, float nnratio, int checkOri, int* __restrict__ matches,
                                                       int* __restrict__ nmatchesOut) {
  search_by_bow_body<false>(kfOff, kfDesc, kfAngle, kfNode, kfValid, fDesc, fAngle, sNode, sIdx, nListed, nf, 0, keyCap, nnratio,
                            checkOri, matches, nmatchesOut);
}

// SearchByBoW(pKF, F, vpMapPointMatches) for a frame with two cameras (F.Nleft != -1, ORBmatcher.cc:342-369, :373-433): the frame's
// rows < fNleft are the left camera's.  The independence argument above holds unchanged: the left and the right top-2 of a keyframe
// feature run over the still-unmatched frame features of ITS node, both matches it may take lie in that node, and "already matched"
// is the only state, so all state stays inside one node; inside a node the keyframe features go in list order, as before.  A
// frame feature is taken at most once (owner), by the left or by the right acceptance, so the filter and the counts are those of
// k_search_by_bow.  Same grid and LDS.
__global__ __launch_bounds__(512) void k_search_by_bow_two_cameras(const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc,
                                                                   const float* __restrict__ kfAngle, const int* __restrict__ kfNode,
                                                                   const uint8_t* __restrict__ kfValid, const uint8_t* __restrict__ fDesc,
                                                                   const float* __restrict__ fAngle, const uint32_t* __restrict__ sNode,
                                                                   const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed,
                                                                   int nf, int fNleft, int keyCap, float nnratio, int checkOri,
                                                                   int* __restrict__ matches, int* __restrict__ nmatchesOut) {
  search_by_bow_body<true>(kfOff, kfDesc, kfAngle, kfNode, kfValid, fDesc, fAngle, sNode, sIdx, nListed, nf, fNleft, keyCap, nnratio,
                           checkOri, matches, nmatchesOut);
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:965-1206, the branch
// without second cameras: NLeft == -1, mvKeysUn) for one keyframe against a batch of neighbours (LocalMapping::CreateNewMapPoints'
// loop, LocalMapping.cc:343-423).
//
// Why every feature of pKF1 may go alone: vbMatched2 (:1011) is read at :1067 and never set, so nothing a feature of pKF1 does is
// seen by another.  For one idx1 the loop of :1060-1137 keeps a candidate when dist <= TH_LOW, dist <= bestDist and the gates pass,
// and no gate reads bestDist: the result is, among the candidates of idx1's node that pass every gate, the smallest distance and,
// of equal distances, the LAST listed (a node lists its features in ascending index: the largest idx2).  That is the minimum of
// the key (distance << 32) | (0xffffffff - idx2); the order in which the candidates are visited does not matter.
//
//   k_node_sort    (above) one workgroup per neighbour: its features that may be taken (listed in a node, no map point, stereo
//                  when bOnlyStereo) sorted by node id, the others last; also clears the neighbour's histogram and counter.
//   k_tri_match    grid (slices of pKF1, neighbours), one wave per idx1, tri_match_body: a binary search finds the node's run in
//                  the neighbour's sorted list, the lanes stride over it (Hamming distance, TH_LOW, then TriPinholeGate: the
//                  epipole gate :1089-1097, the epipolar gate Pinhole.cpp:130-143 on the host's F12), a wave minimum of the key
//                  picks the winner; lane 0 writes vMatches12[idx1] and adds to the neighbour's 30-bin rotation histogram and
//                  counter (global atomics).
//   k_tri_finish   (mbCheckOrientation only) one workgroup per neighbour: three_maxima on the histogram, then
//                  the row is filtered (a match's bin is recomputed from the two angles) and the return value corrected.
// ---------------------------------------------------------------------------
constexpr int TRI_PER_WAVE = 4;

// What k_tri_match and k_tri_match_kb8 share: one wave per idx1 of pKF1 against neighbour blockIdx.y (rows base ..), the node's
// run in the neighbour's sorted list, the lanes striding over it, Hamming distance and TH_LOW first (:1080), the wave minimum of the
// key, and lane 0's epilogue (vMatches12[idx1], the neighbour's counter and rotation histogram).  The gate is the kernel's own:
//   gate.admits(idx1)      whether idx1 is searched at all (:1036-1045),
//   gate.begin(idx1, k1)   what depends on idx1 only,
//   gate.keeps(idx2)       whether the candidate idx2 of the neighbour, already within TH_LOW, stays.
template <class Gate>
__device__ __forceinline__ void tri_match_body(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1,
                                               const int* __restrict__ node1, int n1, int base,
                                               const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc,
                                               const uint32_t* __restrict__ sNode, const uint16_t* __restrict__ sIdx,
                                               const int* __restrict__ nListed, int checkOri, int* __restrict__ matches12,
                                               int* __restrict__ stat, Gate& gate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int kf = blockIdx.y, nl = nListed[kf];
  const uint32_t* sn = sNode + base;
  const uint16_t* si = sIdx + base;
  const int first = (blockIdx.x * nwaves + wave) * TRI_PER_WAVE;
  for (int idx1 = first; idx1 < min(first + TRI_PER_WAVE, n1); ++idx1) {
    int best = -1;
    const int node = node1[idx1];
    if (node >= 0 && gate.admits(idx1)) {                          // (a feature in no node is never visited)
      const int lo = bow_lower_bound(sn, 0, nl, (uint32_t)node);
      if (lo < nl && sn[lo] == (uint32_t)node) {
        const int hi = bow_lower_bound(sn, lo + 1, nl, (uint32_t)node + 1u);
        gate.begin(idx1, kp1[idx1]);
        uint64_t d1[4];
        load_desc(desc1 + (int64_t)idx1 * 32, d1);
        unsigned long long k = ~0ull;
        for (int t = lo + lane; t < hi; t += 64) {
          const int idx2 = si[t];
          uint64_t d2[4];
          load_desc(kfDesc + (int64_t)(base + idx2) * 32, d2);
          const int dist = hamming256(d1, d2);
          if (dist > BOW_TH_LOW) continue;                         // :1080 (dist > bestDist: the key's minimum)
          if (!gate.keeps(idx2)) continue;
          const unsigned long long kk = ((unsigned long long)dist << 32) | (0xFFFFFFFFu - (unsigned)idx2);
          k = kk < k ? kk : k;
        }
        k = wave_min_u64(k);
        if (k != ~0ull) best = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
      }
    }
    if (lane == 0) {
      matches12[(int64_t)kf * n1 + idx1] = best;
      if (best >= 0) {
        atomicAdd(&stat[kf * TRI_STAT + 30], 1);
        if (checkOri) atomicAdd(&stat[kf * TRI_STAT + bow_rot_bin(kp1[idx1].angle, kfKp[base + best].angle)], 1);
      }
    }
  }
}

// the pinhole gates: bOnlyStereo (:1043-1045), the epipole gate :1089-1097, the epipolar gate Pinhole.cpp:130-143 on the host's F12
struct TriPinholeGate {
  const uint8_t *__restrict__ hasMp1, *__restrict__ stereo1, *__restrict__ kfStereo;
  const pli_keypoint* __restrict__ kfKp;
  const float *__restrict__ F, *__restrict__ scaleFactor, *__restrict__ sigma2;
  float epx, epy;
  int base, onlyStereo, coarse;
  bool st1;                                                        // of idx1 (admits, begin):
  float a, b, c, den;
  __device__ __forceinline__ bool admits(int idx1) {
    st1 = stereo1[idx1] != 0;
    return !hasMp1[idx1] && (!onlyStereo || st1);                  // :1036-1045
  }
  __device__ __forceinline__ void begin(int, const pli_keypoint& k1) {
    // the epipolar line in the second image, l = x1' F12 = [a b c] (Pinhole.cpp:130-132)
    a = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, F[0]), __fmul_rn(k1.y, F[3])), F[6]);
    b = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, F[1]), __fmul_rn(k1.y, F[4])), F[7]);
    c = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, F[2]), __fmul_rn(k1.y, F[5])), F[8]);
    den = __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b));
  }
  __device__ __forceinline__ bool keeps(int idx2) const {
    const pli_keypoint k2 = kfKp[base + idx2];
    if (!st1 && !kfStereo[base + idx2]) {                          // :1089-1097
      const float ex = __fsub_rn(epx, k2.x), ey = __fsub_rn(epy, k2.y);
      if (__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) < __fmul_rn(100.0f, scaleFactor[k2.octave])) return false;
    }
    if (!coarse) {                                                 // Pinhole.cpp:134-143
      const float num = __fadd_rn(__fadd_rn(__fmul_rn(a, k2.x), __fmul_rn(b, k2.y)), c);
      if (den == 0.0f) return false;
      const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
      if (!((double)dsqr < 3.84 * (double)sigma2[k2.octave])) return false;
    }
    return true;
  }
};

// grid = (ceil(n1 / (waves per block * TRI_PER_WAVE)), neighbours)
__global__ __launch_bounds__(256) void k_tri_match(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1,
                                                   const int* __restrict__ node1, const uint8_t* __restrict__ hasMp1,
                                                   const uint8_t* __restrict__ stereo1, int n1, const int* __restrict__ kfOff,
                                                   const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc,
                                                   const uint8_t* __restrict__ kfStereo, const uint32_t* __restrict__ sNode,
                                                   const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed,
                                                   const float* __restrict__ F12, const float* __restrict__ ep,
                                                   const float* __restrict__ scaleFactor, const float* __restrict__ sigma2,
                                                   int onlyStereo, int coarse, int checkOri, int* __restrict__ matches12,
                                                   int* __restrict__ stat) {
  const int kf = blockIdx.y, base = kfOff[kf];
  TriPinholeGate gate{hasMp1, stereo1, kfStereo, kfKp, F12 + kf * 9, scaleFactor, sigma2, ep[kf * 2], ep[kf * 2 + 1], base, onlyStereo,
                      coarse};
  tri_match_body(kp1, desc1, node1, n1, base, kfKp, kfDesc, sNode, sIdx, nListed, checkOri, matches12, stat, gate);
}

// grid = neighbours (mbCheckOrientation only)
__global__ __launch_bounds__(256) void k_tri_finish(const pli_keypoint* __restrict__ kp1, int n1, const int* __restrict__ kfOff,
                                                    const pli_keypoint* __restrict__ kfKp, int* __restrict__ matches12,
                                                    int* __restrict__ stat) {
  __shared__ int keep[3];
  const int kf = blockIdx.x, base = kfOff[kf];
  int* hist = stat + kf * TRI_STAT;
  if (threadIdx.x == 0) hist[30] = bow_keep_bins(hist, hist[30], 1, keep);
  __syncthreads();
  const int ind1 = keep[0], ind2 = keep[1], ind3 = keep[2];
  int* row = matches12 + (int64_t)kf * n1;
  for (int i = threadIdx.x; i < n1; i += blockDim.x) {
    const int j = row[i];
    if (j < 0) continue;
    const int b = bow_rot_bin(kp1[i].angle, kfKp[base + j].angle);
    if (b != ind1 && b != ind2 && b != ind3) row[i] = -1;
  }
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (ORBmatcher.cc:823-963, NLeft == -1 on both sides) for one
// keyframe pKF1 against a batch of keyframes pKF2[k] (LoopClosing::DetectCommonRegionsFromBoW's loop, LoopClosing.cc:528-540).
//
// Against SearchByBoW(KF, Frame) the sides swap: pKF1 is walked in list order and pKF2's features are the ones taken away
// (vbMatched2), both sides carry the map-point gate, the distance test is strict (bestDist1 < TH_LOW) and the result is indexed by
// pKF1's feature.
//
// Why the reference's sequential walk may run in parallel: a feature is listed in ONE node of its FeatureVector, and
// vbMatched2[idx2] is only read and written while the node that lists idx2 is walked, that is by pKF1's features of that node.  So
// the common nodes are independent of each other, the pairs (pKF1, pKF2[k]) are independent of each other (vbMatched2 is per call),
// and only pKF1's features inside one node must be taken in list order (ascending index).  The rotation histogram and nmatches are
// sums over the matches; vbMatched2 is not given back by the rotation filter and is not read after it.
//
//   k_node_sort         (above) one workgroup per pKF2[k]: its valid features sorted by node id (the candidate list differs per pair).
//   k_search_by_bow_kf  one workgroup per pair: pKF1's valid features whose node k lists (with a valid feature: a node without one
//                       has no candidate) become (first position of the node in k's sorted list, idx1) keys, 13 bits each, sorted
//                       in LDS; bow_walk takes the runs.  owner[idx2] (LDS) is vbMatched2 with the idx1 that took it; thread 0
//                       runs three_maxima; the owner table is inverted in LDS with the filter applied and written as the row.
// Two launches per call, whatever nkf.
// ---------------------------------------------------------------------------
// grid = pairs; keyCap = a power of two >= n1, ownerCap >= every pKF2's feature count; LDS: 48 ints + keyCap keys + ownerCap shorts
__global__ __launch_bounds__(512) void k_search_by_bow_kf(const uint8_t* __restrict__ desc1, const float* __restrict__ angle1,
                                                          const int* __restrict__ node1, const uint8_t* __restrict__ valid1, int n1,
                                                          const int* __restrict__ kfOff, const uint8_t* __restrict__ kfDesc,
                                                          const float* __restrict__ kfAngle, const uint32_t* __restrict__ sNode,
                                                          const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed,
                                                          int keyCap, float nnratio, int checkOri, int* __restrict__ matches12,
                                                          int* __restrict__ nmatchesOut) {
  extern __shared__ __align__(16) int bowKfLds[];
  int* hist = bowKfLds;                                           // 30 bins (32 ints)
  int* misc = bowKfLds + 32;                                      // [0] keys, [1] matches, [2..4] the bins ComputeThreeMaxima keeps
  uint32_t* key = reinterpret_cast<uint32_t*>(bowKfLds + 48);
  short* owner = reinterpret_cast<short*>(key + keyCap);          // per feature of pKF2: the feature of pKF1 that took it, -1 free
  const int tid = threadIdx.x, lane = tid & 63;
  const int kf = blockIdx.x, base = kfOff[kf], nk = kfOff[kf + 1] - base, nl = nListed[kf];
  const uint32_t* sn = sNode + base;
  const uint16_t* si = sIdx + base;
  int* row = matches12 + (int64_t)kf * n1;
  for (int i = tid; i < 48; i += blockDim.x) bowKfLds[i] = 0;
  for (int i = tid; i < nk; i += blockDim.x) owner[i] = -1;
  __syncthreads();
  const int m = bow_collect_keys(node1, valid1, n1, sn, nl, key, &misc[0]);   // :862-866
  const int nm = bow_walk<false>(key, m, desc1, angle1, sn, si, nl, kfDesc + (int64_t)base * 32, kfAngle + base, owner, hist, BOW_TH_LOW - 1,
                          nnratio, checkOri);                     // bestDist1 < TH_LOW :906
  if (lane == 0 && nm) atomicAdd(&misc[1], nm);
  __syncthreads();
  if (tid == 0) nmatchesOut[kf] = bow_keep_bins(hist, misc[1], checkOri, misc + 2);
  int* inv = reinterpret_cast<int*>(key);                         // the keys are done: vpMatches12 as indices, n1 <= keyCap
  for (int i = tid; i < n1; i += blockDim.x) inv[i] = -1;
  __syncthreads();
  const int ind1 = misc[2], ind2 = misc[3], ind3 = misc[4];
  for (int i2 = tid; i2 < nk; i2 += blockDim.x) {
    const int i = owner[i2];
    if (i < 0) continue;
    if (checkOri) {
      const int b = bow_rot_bin(angle1[i], kfAngle[base + i2]);
      if (b != ind1 && b != ind2 && b != ind3) continue;
    }
    inv[i] = i2;
  }
  __syncthreads();
  for (int i = tid; i < n1; i += blockDim.x) row[i] = inv[i];
}

// ---------------------------------------------------------------------------
// The search half of ORBmatcher::Fuse (ORBmatcher.cc:1399-1609, the branch bRight == false, NLeft == -1, keypoints = mvKeysUn;
// and the Sim3 overload :1611-1733, which has no chi-square gate) for nmp map points against a batch of keyframes
// (LocalMapping::SearchInNeighbors, LocalMapping.cc:743-749 and :776; LoopClosing::SearchAndFuse).
//
// No map point's bestIdx reads another's, so every (keyframe, point) pair goes alone.  Its result is the strict minimum of the
// Hamming distance in the visiting order of KeyFrame::GetFeaturesInArea (KeyFrame.cc:881-925: cell columns, then cell rows, then
// the cell's list in ascending index): the minimum of the key (distance, column, row, index), proj_key's order.  What follows the
// search (Replace / AddObservation / AddMapPoint, isBad(), IsInKeyFrame) is sequential and stays on the host.
//
//   k_fuse_grid     one workgroup per keyframe: a counting sort of its features by grid cell (Frame::PosInGrid), the cells in the
//                   order column * 48 + row, so that the rows r0..r1 of one column are ONE run of the index list.
//   k_fuse_project  one thread per (keyframe, point): Rcw * p + tcw as cv::Mat arithmetic (cvmat_dot3), the depth, image, distance
//                   and viewing-angle gates, PredictScale as comparisons against the host's level_ratio table (no device
//                   logarithm), the radius.  Survivors go to a compact list (ballot + popcount, one atomic per wave); every pair
//                   gets -1 / 256 here.
//   k_fuse_match    FUSE_LANES lanes per survivor (a 3 px window holds a handful of keypoints: a whole wave per query would idle
//                   most lanes), a fixed grid striding over the list: cell_window_walk (the lanes stride over each column's run,
//                   apply the window and the level gate [level - 1, level]) with the chi-square gate :1533-1557 as its row gate,
//                   and the group minimum of the key by cross-lane shuffles.  TH_LOW decides the result.
// Three launches per call, whatever nkf and nmp.
// ---------------------------------------------------------------------------
constexpr int FUSE_CELLS = GRID_COLS * GRID_ROWS;
constexpr int FUSE_TH_LOW = 50;                                  // ORBmatcher::TH_LOW

__device__ __forceinline__ int fuse_cell(const pli_keypoint& k, float minX, float minY, float gwInv, float ghInv, int& px, int& py) {
  px = (int)roundf(__fmul_rn(__fsub_rn(k.x, minX), gwInv));
  py = (int)roundf(__fmul_rn(__fsub_rn(k.y, minY), ghInv));
  if (px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS) return -1;                  // PosInGrid
  return px * GRID_ROWS + py;
}

// The cells that GetFeaturesInArea visits for the window (u, v, radius) (KeyFrame.cc:889-903, Frame.cc:781-806): columns c0..c1,
// rows r0..r1, clamped to the grid.  Shared by every walk over the cell runs.
struct CellWindow {
  int c0, c1, r0, r1;
  __device__ __forceinline__ CellWindow(float u, float v, float radius, const pli_fuse_camera& cam, float gwInv, float ghInv)
      : c0(max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, cam.min_x), radius), gwInv)))),
        c1(min(GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, cam.min_x), radius), gwInv)))),
        r0(max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, cam.min_y), radius), ghInv)))),
        r1(min(GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, cam.min_y), radius), ghInv)))) {}
  __device__ __forceinline__ bool empty() const { return !(c0 < GRID_COLS && c1 >= 0 && r0 < GRID_ROWS && r1 >= 0 && r0 <= r1); }
};

// The key of row i2 (keypoint k) at Hamming distance dist: (distance, cell column, cell row, index), the visiting order of
// GetFeaturesInArea among equal distances.  key_row / key_dist take it apart again.
__device__ __forceinline__ unsigned long long cell_key(int dist, const pli_keypoint& k, const pli_fuse_camera& cam, float gwInv,
                                                       float ghInv, int i2) {
  int px, py;
  fuse_cell(k, cam.min_x, cam.min_y, gwInv, ghInv, px, py);
  return ((unsigned long long)dist << 40) | ((unsigned long long)px << 34) | ((unsigned long long)py << 28) | (unsigned long long)i2;
}
__device__ __forceinline__ int key_row(unsigned long long key) { return (int)(key & 0xFFFFFFFull); }
__device__ __forceinline__ int key_dist(unsigned long long key) { return (int)(key >> 40); }

// grid = keyframes, 256 threads; cellStart: nkf x (FUSE_CELLS + 1), sIdx: one uint16 per feature (the listed ones first)
__global__ __launch_bounds__(256) void k_fuse_grid(const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp,
                                                   pli_fuse_camera cam, int* __restrict__ cellStart,
                                                   uint16_t* __restrict__ sIdx) {
  __shared__ int cnt[FUSE_CELLS];
  __shared__ int part[256];
  const int kf = blockIdx.x, base = kfOff[kf], nk = kfOff[kf + 1] - base, t = threadIdx.x;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  for (int i = t; i < FUSE_CELLS; i += 256) cnt[i] = 0;
  __syncthreads();
  for (int i = t; i < nk; i += 256) {
    int px, py;
    const int cell = fuse_cell(kfKp[base + i], cam.min_x, cam.min_y, gwInv, ghInv, px, py);
    if (cell >= 0) atomicAdd(&cnt[cell], 1);
  }
  __syncthreads();
  // exclusive scan of the 3072 counts: 12 cells per thread, then the 256 partial sums
  constexpr int PER = FUSE_CELLS / 256;
  int s = 0;
  for (int j = 0; j < PER; ++j) s += cnt[t * PER + j];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  int* cs = cellStart + (int64_t)kf * (FUSE_CELLS + 1);
  for (int j = 0; j < PER; ++j) {
    const int c = cnt[t * PER + j];
    cs[t * PER + j] = run;
    cnt[t * PER + j] = run;                                      // from here on: the cell's write cursor
    run += c;
  }
  if (t == 255) cs[FUSE_CELLS] = run;
  __syncthreads();
  for (int i = t; i < nk; i += 256) {
    int px, py;
    const int cell = fuse_cell(kfKp[base + i], cam.min_x, cam.min_y, gwInv, ghInv, px, py);
    if (cell >= 0) sIdx[base + atomicAdd(&cnt[cell], 1)] = (uint16_t)i;      // (the order inside a cell is free: the key decides)
  }
}

static_assert(sizeof(FuseSurvivor) == 32, "FuseSurvivor layout");

// What the projection gates of Fuse / Sim3 and of relocalisation (:2360-2374) share once the point is inside the image:
// PO, the distance-range gate, (kNormalGate: Fuse and Sim3 only) the viewing-normal gate, PredictScale and the radius.
template <bool kNormalGate>
__device__ __forceinline__ bool project_point_tail(const pli_fuse_point& P, const float* __restrict__ T, float th,
                                                   const float* __restrict__ levelRatio, int nlevels,
                                                   const float* __restrict__ scaleFactor, FuseSurvivor& S) {
  const float po[3] = {__fsub_rn(P.pos[0], T[12]), __fsub_rn(P.pos[1], T[13]), __fsub_rn(P.pos[2], T[14])};
  // cv::norm(PO) (NORM_L2 of CV_32F: the squares summed in double) and PO.dot(Pn) (double)
  const double n2 = (double)po[0] * (double)po[0] + (double)po[1] * (double)po[1] + (double)po[2] * (double)po[2];
  const float dist3D = (float)sqrt(n2);
  if (dist3D < P.min_dist_inv || dist3D > P.max_dist_inv) return false;                    // reloc: :2368
  if (kNormalGate) {
    const double dot = (double)po[0] * (double)P.normal[0] + (double)po[1] * (double)P.normal[1] + (double)po[2] * (double)P.normal[2];
    if (dot < 0.5 * (double)dist3D) return false;
  }
  const float ratio = __fdiv_rn(P.max_dist, dist3D);             // MapPoint::PredictScale, MapPoint.cc:449-464 / :466-482
  int level = 0;
  for (int n = 0; n < nlevels - 1; ++n) level += ratio > levelRatio[n] ? 1 : 0;
  S.level = level;
  S.radius = __fmul_rn(th, scaleFactor[level]);                  // reloc: :2374
  return true;
}

// One (keyframe, point) pair up to the window search: the gates :1432-1500 (Sim3 searches: :501-543) in the reference's order.  true: S
// holds the projection, the level and the radius (S.ur only for kForm 0).  kForm 0: Pinhole::project (Pinhole.cpp:30-33, fx*x/z + cx),
// what Fuse and ORBmatcher.cc:519 call; kForm 1: ORBmatcher.cc:631-636 (invz = 1/z; x*invz; fx*x + cx), which rounds differently.
template <int kForm>
__device__ __forceinline__ bool fuse_project_point(const pli_fuse_point& P, const float* __restrict__ T /* Rcw row major, tcw, Ow */,
                                                   const pli_fuse_camera& cam, float th, const float* __restrict__ levelRatio,
                                                   int nlevels, const float* __restrict__ scaleFactor, FuseSurvivor& S) {
  float pc[3];
  for (int r = 0; r < 3; ++r) pc[r] = cvmat_dot3(T + 3 * r, 1, P.pos, 1.0, (double)T[9 + r]);      // Rcw*p3Dw + tcw
  const float x = pc[0], y = pc[1], z = pc[2];
  if (z < 0.0f) return false;                                    // :1448
  const float invz = __fdiv_rn(1.0f, z);
  if (kForm == 0) {
    S.u = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fx, x), z), cam.cx);             // Pinhole::project, Pinhole.cpp:30-33
    S.v = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fy, y), z), cam.cy);
  } else {
    S.u = __fadd_rn(__fmul_rn(cam.fx, __fmul_rn(x, invz)), cam.cx);          // ORBmatcher.cc:631-636
    S.v = __fadd_rn(__fmul_rn(cam.fy, __fmul_rn(y, invz)), cam.cy);
  }
  if (!(S.u >= cam.min_x && S.u < cam.max_x && S.v >= cam.min_y && S.v < cam.max_y)) return false;      // KeyFrame::IsInImage
  S.ur = __fsub_rn(S.u, __fmul_rn(cam.bf, invz));
  return project_point_tail<true>(P, T, th, levelRatio, nlevels, scaleFactor, S);
}

// the compact survivor list: ballot + popcount, one atomic per wave (every lane of the wave calls it)
__device__ __forceinline__ void compact_survivor(bool keep, const FuseSurvivor& S, FuseSurvivor* __restrict__ surv,
                                                 int* __restrict__ nSurv) {
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
  if (bal) {
    const int lane = threadIdx.x & 63;
    int first = 0;
    if (lane == 0) first = atomicAdd(nSurv, __popcll(bal));
    first = __shfl(first, 0, 64);
    if (keep) surv[first + __popcll(bal & ((1ull << lane) - 1ull))] = S;
  }
}

// grid = ceil(nkf * nmp / 256)
__global__ __launch_bounds__(256) void k_fuse_project(const pli_fuse_point* __restrict__ mp, int nmp, int nkf,
                                                      const float* __restrict__ kfPose, const uint8_t* __restrict__ skip,
                                                      pli_fuse_camera cam, float th, const float* __restrict__ levelRatio,
                                                      int nlevels, const float* __restrict__ scaleFactor,
                                                      FuseSurvivor* __restrict__ surv, int* __restrict__ nSurv,
                                                      int* __restrict__ bestIdx, int* __restrict__ bestDist) {
  const int64_t pair = (int64_t)blockIdx.x * 256 + threadIdx.x, npairs = (int64_t)nkf * nmp;
  bool keep = false;
  FuseSurvivor S;
  if (pair < npairs) {
    const int kf = (int)(pair / nmp), i = (int)(pair - (int64_t)kf * nmp);
    S.kf = kf; S.mp = i; S.pad = 0;
    bestIdx[pair] = -1;
    if (bestDist) bestDist[pair] = 256;
    const pli_fuse_point P = mp[i];
    if (P.valid && !(skip && skip[pair]))                        // !pMP, isBad(), IsInKeyFrame(pKF) / spAlreadyFound
      keep = fuse_project_point<0>(P, kfPose + (int64_t)kf * 15, cam, th, levelRatio, nlevels, scaleFactor, S);
  }
  compact_survivor(keep, S, surv, nSurv);
}

// ---------------------------------------------------------------------------
// The front of Tracking::SearchLocalPointsAndLines (Tracking.cc:3809-3883) for a frame of one camera (Nleft == -1).
//   k_local_project        one thread per local map point: Frame::isInFrustum (Frame.cc:585-647) in the reference's order and with
//                          its roundings, the view record the tracker keeps, and the point's query of
//                          ORBmatcher::SearchByProjection(F, vpMapPoints) as ORBmatcher.cc:53-73 builds it, left on the device for
//                          k_proj_candidates / k_proj_assign.  NOT fuse_project_point: the image gate is closed at mnMaxX / mnMaxY
//                          and lets a NaN through, the viewing angle is a float cosine against the caller's limit, and the record
//                          keeps the projection of a point that a later gate refuses.
//   k_local_lines_project  ONE workgroup: Frame::isInFrustum_l (Frame.cc:661-701) per local map line, then the in-view lines
//                          compacted in list order (the order is the result: matches_12 is indexed by the position in
//                          mvpLocalMapLines_InFrustum) with their descriptors gathered for k_knn2.
// ---------------------------------------------------------------------------
static_assert(sizeof(pli_local_view) == 32, "pli_local_view layout");

// grid = ceil(nq / 256); T: Rcw row major, tcw, Ow
__global__ __launch_bounds__(256) void k_local_project(const pli_fuse_point* __restrict__ mp, int nq, const float* __restrict__ T,
                                                       pli_fuse_camera cam, float viewCosLimit, float th, int farPoints,
                                                       float thFar, const float* __restrict__ levelRatio, int nlevels,
                                                       const float* __restrict__ scaleFactor, pli_local_view* __restrict__ view,
                                                       pli_proj_query* __restrict__ q, int* __restrict__ nInView) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool inView = false;
  if (i < nq) {
    pli_local_view V = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0};
    const pli_fuse_point P = mp[i];
    // A point skipped at Tracking.cc:3813 that still carries mbTrackInView from an earlier frame (PLI_LOCAL_STORED_VIEW): isInFrustum
    // does not run, ORBmatcher.cc:53-73 searches it with the fields it holds.  The row carries them; the record stays zero.
    const bool stored = P.valid == PLI_LOCAL_STORED_VIEW;
    if (stored) {
      V.proj_x = P.pos[0]; V.proj_y = P.pos[1]; V.proj_xr = P.pos[2];
      V.depth = P.normal[0]; V.view_cos = P.normal[1]; V.level = (int)P.normal[2];
    } else if (P.valid) {                                          // Tracking.cc:3813-3816
      V.proj_x = -1.0f; V.proj_y = -1.0f;                          // Frame.cc:589-590
      float pc[3];
      for (int r = 0; r < 3; ++r) pc[r] = cvmat_dot3(T + 3 * r, 1, P.pos, 1.0, (double)T[9 + r]);      // mRcw*P + mtcw
      const float pcDist = (float)sqrt((double)pc[0] * (double)pc[0] + (double)pc[1] * (double)pc[1] + (double)pc[2] * (double)pc[2]);
      const float z = pc[2];
      const float invz = __fdiv_rn(1.0f, z);
      if (!(z < 0.0f)) {                                           // :602
        const float u = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fx, pc[0]), z), cam.cx);       // Pinhole::project, Pinhole.cpp:30-33
        const float v = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fy, pc[1]), z), cam.cy);
        if (!(u < cam.min_x || u > cam.max_x) && !(v < cam.min_y || v > cam.max_y)) {    // :607-610, as written: a NaN stays
          V.proj_x = u; V.proj_y = v;                              // :612-613
          const float po[3] = {__fsub_rn(P.pos[0], T[12]), __fsub_rn(P.pos[1], T[13]), __fsub_rn(P.pos[2], T[14])};
          const float dist = (float)sqrt((double)po[0] * (double)po[0] + (double)po[1] * (double)po[1] + (double)po[2] * (double)po[2]);
          if (!(dist < P.min_dist_inv || dist > P.max_dist_inv)) { // :621
            const double dot = (double)po[0] * (double)P.normal[0] + (double)po[1] * (double)P.normal[1] + (double)po[2] * (double)P.normal[2];
            const float viewCos = (float)(dot / (double)dist);     // :627
            if (!(viewCos < viewCosLimit)) {                       // :629
              const float ratio = __fdiv_rn(P.max_dist, dist);     // MapPoint::PredictScale, MapPoint.cc:449-464
              int level = 0;
              for (int n = 0; n < nlevels - 1; ++n) level += ratio > levelRatio[n] ? 1 : 0;
              inView = true;
              V.in_view = 1; V.level = level; V.depth = pcDist; V.view_cos = viewCos;
              V.proj_xr = __fsub_rn(u, __fmul_rn(cam.bf, invz));   // :638
            }
          }
        }
      }
    }
    pli_proj_query Q = {0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0.0f, 0};
    if ((inView || stored) && !(farPoints && V.depth > thFar)) {   // ORBmatcher.cc:53-57
      float r = (double)V.view_cos > 0.998 ? 2.5f : 4.0f;          // RadiusByViewingCos :216-222
      if (th != 1.0f) r = __fmul_rn(r, th);                        // :69-70
      Q.u = V.proj_x; Q.v = V.proj_y; Q.ur = V.proj_xr;
      Q.radius = __fmul_rn(r, scaleFactor[min(max(V.level, 0), nlevels - 1)]);   // :73 (a stored level: the host checked it)
      Q.min_level = V.level - 1; Q.max_level = V.level;
      // a NaN projection takes no keypoint (every |x - u| < r is false): the query is closed here, so that no window is derived from it
      Q.valid = (Q.u != Q.u || Q.v != Q.v) ? 0 : 1;
    }
    q[i] = Q;
    if (stored) V = pli_local_view{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0};
    view[i] = V;
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(inView);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(nInView, __popcll(bal));
}

// grid = 1, 1024 threads; sp: nl x 3 floats, gathered: room for nl rows of 32 bytes, count[0] = the lines in view
__global__ __launch_bounds__(1024) void k_local_lines_project(const float* __restrict__ sp, const uint8_t* __restrict__ valid,
                                                              const uint8_t* __restrict__ desc, int nl,
                                                              const float* __restrict__ T, pli_fuse_camera cam,
                                                              int* __restrict__ inViewOut, float* __restrict__ projS,
                                                              int* __restrict__ inFrustum, uint8_t* __restrict__ gathered,
                                                              int* __restrict__ count) {
  __shared__ int waveCnt[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int base = 0;                                                    // in-view lines before this chunk (the same in every thread)
  for (int first = 0; first < nl; first += 1024) {
    const int i = first + t;
    bool in = false;
    float u = 0.0f, v = 0.0f;
    if (i < nl && valid[i]) {                                      // Tracking.cc:3865-3868
      float pc[3];
      for (int r = 0; r < 3; ++r) pc[r] = cvmat_dot3(T + 3 * r, 1, sp + 3 * (int64_t)i, 1.0, (double)T[9 + r]);   // mRcw*sp + mtcw
      if (!(pc[2] < 0.0f)) {                                       // Frame.cc:679
        const float invz = __fdiv_rn(1.0f, pc[2]);
        const float pu = __fadd_rn(__fmul_rn(__fmul_rn(cam.fx, pc[0]), invz), cam.cx);   // :684-685, left to right
        const float pv = __fadd_rn(__fmul_rn(__fmul_rn(cam.fy, pc[1]), invz), cam.cy);
        if (!(pu < cam.min_x || pu > cam.max_x) && !(pv < cam.min_y || pv > cam.max_y)) { in = true; u = pu; v = pv; }
      }
    }
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(in);
    if (lane == 0) waveCnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, chunk = 0;
    for (int w = 0; w < 16; ++w) { const int c = waveCnt[w]; before += w < wave ? c : 0; chunk += c; }
    if (i < nl) {
      inViewOut[i] = in ? 1 : 0;
      projS[2 * (int64_t)i] = u; projS[2 * (int64_t)i + 1] = v;
      if (in) {
        const int k = base + before + __popcll(bal & ((1ull << lane) - 1ull));
        inFrustum[k] = i;
        const uint4* s = reinterpret_cast<const uint4*>(desc + (int64_t)i * 32);
        uint4* d = reinterpret_cast<uint4*>(gathered + (int64_t)k * 32);
        d[0] = s[0]; d[1] = s[1];
      }
    }
    base += chunk;
    __syncthreads();                                               // waveCnt is read before the next chunk rewrites it
  }
  if (t == 0) count[0] = base;
}

// the minimum of a key over the G lanes of a group (G a power of two <= 64; all lanes of the wave take part)
template <int G>
__device__ __forceinline__ unsigned long long group_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// The window of survivor S in its keyframe's cell runs (KeyFrame::GetFeaturesInArea, KeyFrame.cc:881-925), `stride` lanes of which
// this is lane `sub`: emit(key) for every row inside the window whose octave lies in [level - 1, level + kUp] (kUp 0: :1524 / :563;
// kUp 1: Frame::GetFeaturesInArea(..., level - 1, level + 1) of ORBmatcher.cc:2376, the same cells in the same order), that
// rowGate(keypoint, row in the flat table) keeps (asked before the descriptor is loaded) and whose distance is <= distLimit (256,
// the largest Hamming distance: no limit).  The one walk of Fuse, the Sim3 search and relocalisation.
struct NoRowGate {
  __device__ __forceinline__ bool operator()(const pli_keypoint&, int) const { return true; }
};
template <int kUp, class RowGate, class Emit>
__device__ __forceinline__ void cell_window_walk(const FuseSurvivor& S, int sub, int stride, const uint8_t* __restrict__ mpDesc,
                                                 const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp,
                                                 const uint8_t* __restrict__ kfDesc, const int* __restrict__ cellStart,
                                                 const uint16_t* __restrict__ sIdx, const pli_fuse_camera& cam, float gwInv, float ghInv,
                                                 int distLimit, RowGate rowGate, Emit emit) {
  const float u = S.u, v = S.v, radius = S.radius;
  const CellWindow w(u, v, radius, cam, gwInv, ghInv);
  if (w.empty()) return;
  const int base = kfOff[S.kf];
  const int* cs = cellStart + (int64_t)S.kf * (FUSE_CELLS + 1);
  uint64_t dq[4];
  load_desc(mpDesc + (int64_t)S.mp * 32, dq);
  for (int cx = w.c0; cx <= w.c1; ++cx) {
    const int lo = cs[cx * GRID_ROWS + w.r0], hi = cs[cx * GRID_ROWS + w.r1 + 1];
    for (int t = lo + sub; t < hi; t += stride) {
      const int i2 = sIdx[base + t];
      const pli_keypoint k = kfKp[base + i2];
      if (!(fabsf(__fsub_rn(k.x, u)) < radius && fabsf(__fsub_rn(k.y, v)) < radius)) continue;        // KeyFrame.cc:918
      if (k.octave < S.level - 1 || k.octave > S.level + kUp) continue;                                // :1524 / :563 / :2376
      if (!rowGate(k, base + i2)) continue;
      uint64_t d2[4];
      load_desc(kfDesc + (int64_t)(base + i2) * 32, d2);
      const int dist = hamming256(dq, d2);
      if (dist > distLimit) continue;
      emit(cell_key(dist, k, cam, gwInv, ghInv, i2));
    }
  }
}

// a fixed grid of 256-thread blocks; G lanes per survivor.  kViews: the tables are the camera views of two-camera keyframes
// (k_fuse_project_views below): kfUright is not read - the gate is the monocular one, 5.99 - and the winner of a right view
// gets its keyframe's NLeft added (:1559).
template <int G, bool kViews>
__global__ __launch_bounds__(256) void k_fuse_match(const FuseSurvivor* __restrict__ surv, const int* __restrict__ nSurv, int nmp,
                                                    const uint8_t* __restrict__ mpDesc, const int* __restrict__ kfOff,
                                                    const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc,
                                                    const float* __restrict__ kfUright, const int* __restrict__ cellStart,
                                                    const uint16_t* __restrict__ sIdx, pli_fuse_camera cam,
                                                    const float* __restrict__ invSigma2, int reprojGate,
                                                    int* __restrict__ bestIdx, int* __restrict__ bestDist) {
  const int ns = *nSurv, sub = threadIdx.x & (G - 1);
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  constexpr int PER_BLOCK = 256 / G;
  // (the loop bound is the same for every lane of a wave: the shuffles below are executed by whole waves)
  for (int64_t b0 = (int64_t)blockIdx.x * PER_BLOCK; b0 < ns; b0 += (int64_t)gridDim.x * PER_BLOCK) {
    const int64_t s = b0 + threadIdx.x / G;
    unsigned long long key = ~0ull;
    FuseSurvivor S;
    S.kf = 0; S.mp = 0;
    if (s < ns) {
      S = surv[s];
      cell_window_walk<0>(S, sub, G, mpDesc, kfOff, kfKp, kfDesc, cellStart, sIdx, cam, gwInv, ghInv, 256,
                          [&](const pli_keypoint& k, int row) {  // the chi-square gate :1533-1557
                            if (!reprojGate) return true;
                            const float ex = __fsub_rn(S.u, k.x), ey = __fsub_rn(S.v, k.y);
                            const float kr = kViews ? -1.f : kfUright[row];
                            float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                            double lim = 5.99;
                            if (kr >= 0) {
                              const float er = __fsub_rn(S.ur, kr);
                              e2 = __fadd_rn(e2, __fmul_rn(er, er));
                              lim = 7.8;
                            }
                            return !((double)__fmul_rn(e2, invSigma2[k.octave]) > lim);
                          },
                          [&](unsigned long long kk) { key = kk < key ? kk : key; });
    }
    key = group_min_u64<G>(key);
    if (s < ns && sub == 0 && key != ~0ull) {
      const int dist = key_dist(key);
      const int64_t pair = (int64_t)S.kf * nmp + S.mp;
      if (bestDist) bestDist[pair] = dist;
      // (a right view 2k + 1 starts NLeft rows after its left view 2k)
      const int nleft = kViews && (S.kf & 1) ? kfOff[S.kf] - kfOff[S.kf - 1] : 0;
      if (dist <= FUSE_TH_LOW) bestIdx[pair] = key_row(key) + nleft;
    }
  }
}
template __global__ void k_fuse_match<8, false>(const FuseSurvivor*, const int*, int, const uint8_t*, const int*, const pli_keypoint*, const uint8_t*, const float*, const int*, const uint16_t*, pli_fuse_camera, const float*, int, int*, int*);
template __global__ void k_fuse_match<16, false>(const FuseSurvivor*, const int*, int, const uint8_t*, const int*, const pli_keypoint*, const uint8_t*, const float*, const int*, const uint16_t*, pli_fuse_camera, const float*, int, int*, int*);
template __global__ void k_fuse_match<64, false>(const FuseSurvivor*, const int*, int, const uint8_t*, const int*, const pli_keypoint*, const uint8_t*, const float*, const int*, const uint16_t*, pli_fuse_camera, const float*, int, int*, int*);
template __global__ void k_fuse_match<8, true>(const FuseSurvivor*, const int*, int, const uint8_t*, const int*, const pli_keypoint*, const uint8_t*, const float*, const int*, const uint16_t*, pli_fuse_camera, const float*, int, int*, int*);

// ---------------------------------------------------------------------------
// Loop closing's ORBmatcher::SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
// (ORBmatcher.cc:473-586 and :588-704) for one list of nmp map points against npair (keyframe, Scw) pairs.
//
// Unlike Fuse this search is sequential across the map points of a pair: vpMatched[bestIdx] = pMP (:579 / :696) takes the keypoint
// away from every later point (:558 / :675).  What a point may take apart from that (gates, window, levels, distances) does not
// depend on the other points, so:
//
//   k_fuse_grid        (unchanged) the cell sort of every pair's keyframe.
//   k_sim3_project     one thread per (pair, point), fuse_project_point<form>: the survivor record goes to the DENSE slot
//                      pair * nmp + point (level -1: the point left at a gate), so a pair's survivors stay in point order; the
//                      slot's candidate count and best_idx are reset here.
//   k_sim3_candidates  (k_window_candidates<0>) SIM3_LANES lanes per slot, a fixed grid striding over the slots:
//                      cell_window_walk, the window walk of k_fuse_match; every key
//                      (distance, cell column, cell row, index) that passes the window and the level gate with a distance within
//                      the limit goes to the slot's list of `width` keys (their order in the list is free: the minimum decides).
//                      The count keeps counting past the width: count > width marks the query as overflowed.
//   k_sim3_assign      one wave per pair, the owner table (-1 free, INT_MAX occupied at entry, else the point) in LDS: the wave
//                      reads 64 counts at a time, walks the slots with candidates in point order (the next one's keys already in
//                      flight), drops owned keys, takes the wave minimum = the reference's strict minimum in visiting order among
//                      the free rows, stores the owner.  An overflowed query walks its window again through the cell runs.
// The limit: bestDist <= TH_LOW * ratioHamming (:577) is a float comparison of an integer below 256, so it equals
// dist <= floor(50.0f * ratio) (the host computes it); a key above the limit can never be accepted, whichever rows are owned.
// Four launches per call, whatever npair and nmp.
// ---------------------------------------------------------------------------
constexpr int SIM3_LANES = 8;

// The dense slot of one point: the survivor record (level -1: the point left at a gate, or is not `live`), the slot's candidate
// count and best_idx reset.  project(S) runs the gates of a live point and fills S.
template <class Project>
__device__ __forceinline__ void dense_slot_store(int64_t slot, int kf, int mp, bool live, Project project,
                                                 FuseSurvivor* __restrict__ surv, int* __restrict__ candCount,
                                                 int* __restrict__ bestIdx) {
  FuseSurvivor S;
  S.kf = kf; S.mp = mp; S.u = 0.f; S.v = 0.f; S.ur = 0.f; S.radius = 0.f; S.level = -1; S.pad = 0;
  if (live && !project(S)) S.level = -1;
  surv[slot] = S;
  candCount[slot] = 0;
  if (bestIdx) bestIdx[slot] = -1;
}

// the table that owns `row` of a flat batch: the last t < n with off[t] <= row
__device__ __forceinline__ int owning_table(const int* __restrict__ off, int n, int row) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

// grid = ceil(npair * nmp / 256)
__global__ __launch_bounds__(256) void k_sim3_project(const pli_fuse_point* __restrict__ mp, int nmp, int npair,
                                                      const float* __restrict__ kfPose, const uint8_t* __restrict__ skip,
                                                      pli_fuse_camera cam, float th, const float* __restrict__ levelRatio,
                                                      int nlevels, const float* __restrict__ scaleFactor, int form,
                                                      FuseSurvivor* __restrict__ surv, int* __restrict__ candCount,
                                                      int* __restrict__ bestIdx) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= (int64_t)npair * nmp) return;
  const int kf = (int)(slot / nmp), i = (int)(slot - (int64_t)kf * nmp);
  const pli_fuse_point P = mp[i];
  const float* T = kfPose + (int64_t)kf * 15;
  dense_slot_store(slot, kf, i, P.valid && !(skip && skip[slot]),                         // isBad(), spAlreadyFound.count(pMP) :501
                   [&](FuseSurvivor& S) {
                     return form ? fuse_project_point<1>(P, T, cam, th, levelRatio, nlevels, scaleFactor, S)
                                 : fuse_project_point<0>(P, T, cam, th, levelRatio, nlevels, scaleFactor, S);
                   },
                   surv, candCount, bestIdx);
}

// The candidate lists of the Sim3 search (kUp 0, launched as "k_sim3_candidates") and of relocalisation (kUp 1,
// "k_reloc_candidates": the searched table is the frame, kfOff = {0, nf}, and distLimit is ORBdist :2403).  A fixed grid of
// 256-thread blocks; SIM3_LANES lanes per slot.  candCount: zeroed by k_sim3_project / k_reloc_project
template <int kUp>
__global__ __launch_bounds__(256) void k_window_candidates(const FuseSurvivor* __restrict__ surv, int64_t nslot,
                                                           const uint8_t* __restrict__ mpDesc, const int* __restrict__ kfOff,
                                                           const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc,
                                                           const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx,
                                                           pli_fuse_camera cam, int distLimit, int width,
                                                           unsigned long long* __restrict__ candKeys, int* __restrict__ candCount) {
  constexpr int PER_BLOCK = 256 / SIM3_LANES;
  const int sub = threadIdx.x & (SIM3_LANES - 1);
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  for (int64_t s = (int64_t)blockIdx.x * PER_BLOCK + threadIdx.x / SIM3_LANES; s < nslot; s += (int64_t)gridDim.x * PER_BLOCK) {
    const FuseSurvivor S = surv[s];
    if (S.level < 0) continue;
    unsigned long long* keys = candKeys + s * width;
    int* count = candCount + s;
    cell_window_walk<kUp>(S, sub, SIM3_LANES, mpDesc, kfOff, kfKp, kfDesc, cellStart, sIdx, cam, gwInv, ghInv, distLimit, NoRowGate(),
                          [=](unsigned long long key) {
                            const int pos = atomicAdd(count, 1);
                            if (pos < width) keys[pos] = key;
                          });
  }
}
template __global__ void k_window_candidates<0>(const FuseSurvivor*, int64_t, const uint8_t*, const int*, const pli_keypoint*, const uint8_t*, const int*, const uint16_t*, pli_fuse_camera, int, int, unsigned long long*, int*);
template __global__ void k_window_candidates<1>(const FuseSurvivor*, int64_t, const uint8_t*, const int*, const pli_keypoint*, const uint8_t*, const int*, const uint16_t*, pli_fuse_camera, int, int, unsigned long long*, int*);

// The cursor of one wave over the n slots of a list that have candidates, in order: 64 counts per load, one bit per slot with
// candidates, and the next slot's keys (keys: n x width) already in flight.  A caller takes i / cnt / key for itself and calls
// advance() BEFORE it decides that slot, so that the next slot's keys travel meanwhile.  i == n: none is left.
struct OrderedCursor {
  const int* __restrict__ cnts;
  const unsigned long long* __restrict__ keys;
  int n, width, lane;
  int chunk = -64, cntLane = 0;
  unsigned long long todo = 0;
  int i = -1, cnt = 0;
  unsigned long long key = ~0ull;                                // lane's key of slot i (~0ull: none, or the list overflowed)
  __device__ __forceinline__ OrderedCursor(const int* cnts, const unsigned long long* keys, int n, int width, int lane)
      : cnts(cnts), keys(keys), n(n), width(width), lane(lane) { advance(); }
  __device__ __forceinline__ void advance() {
    while (todo == 0) {
      chunk += 64;
      if (chunk >= n) { i = n; return; }
      cntLane = chunk + lane < n ? cnts[chunk + lane] : 0;
      todo = __builtin_amdgcn_ballot_w64(cntLane != 0);
    }
    const int bit = __builtin_ctzll(todo);
    todo &= todo - 1;
    i = chunk + bit;
    cnt = __shfl(cntLane, bit, 64);
    key = (cnt <= width && lane < cnt) ? keys[(int64_t)i * width + lane] : ~0ull;
  }
};

// The ordered walk of one wave over the slots slot0 .. slot0 + nmp (one pair's, or one candidate's, points in list order) against
// the owner table in LDS (-1 free, INT_MAX occupied at entry, else the point).  Returns the number of rows taken.  kUp as
// cell_window_walk.
template <int kUp>
__device__ __forceinline__ int sim3_ordered_walk(int* owner, int lane, const FuseSurvivor* __restrict__ surv, int64_t slot0, int nmp,
                                                 const uint8_t* __restrict__ mpDesc, const int* __restrict__ kfOff,
                                                 const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc,
                                                 const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx,
                                                 const pli_fuse_camera& cam, float gwInv, float ghInv, int distLimit, int width,
                                                 const unsigned long long* __restrict__ candKeys,
                                                 const int* __restrict__ candCount, int* __restrict__ bestIdx) {
  OrderedCursor cur(candCount + slot0, candKeys + slot0 * width, nmp, width, lane);
  int nmatches = 0;
  while (cur.i < nmp) {
    const int i = cur.i, cnt = cur.cnt;
    unsigned long long key = cur.key;
    cur.advance();                                               // the next query's keys travel while this one is decided
    if (cnt <= width) {
      if (key != ~0ull && owner[key_row(key)] != -1) key = ~0ull;                          // :558
    } else {                                                     // more candidates than the list holds: the window again
      key = ~0ull;
      cell_window_walk<kUp>(surv[slot0 + i], lane, 64, mpDesc, kfOff, kfKp, kfDesc, cellStart, sIdx, cam, gwInv, ghInv, distLimit,
                            NoRowGate(), [&](unsigned long long kk) {
                              if (owner[key_row(kk)] == -1 && kk < key) key = kk;
                            });
    }
    const unsigned long long m = wave_min_u64(key);
    if (m != ~0ull) {                                            // :577 (the limit is already applied)
      const int b = key_row(m);
      owner[b] = i;                                              // :579 (every lane stores the same value)
      if (lane == 0 && bestIdx) bestIdx[slot0 + i] = b;
      ++nmatches;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // single wave: LDS is executed in order
  }
  return nmatches;
}

// grid = pairs, one wave; LDS: the pair's rows as ints (the owner table)
__global__ __launch_bounds__(64) void k_sim3_assign(const FuseSurvivor* __restrict__ surv, int nmp, const uint8_t* __restrict__ mpDesc,
                                                    const int* __restrict__ kfOff, const pli_keypoint* __restrict__ kfKp,
                                                    const uint8_t* __restrict__ kfDesc, const uint8_t* __restrict__ occupied,
                                                    const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx,
                                                    pli_fuse_camera cam, int distLimit, int width,
                                                    const unsigned long long* __restrict__ candKeys,
                                                    const int* __restrict__ candCount, int* __restrict__ rowPoint,
                                                    int* __restrict__ bestIdx, int* __restrict__ nmatchesOut) {
  extern __shared__ int owner[];
  const int pair = blockIdx.x, lane = threadIdx.x, base = kfOff[pair], nk = kfOff[pair + 1] - base;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  for (int r = lane; r < nk; r += 64) owner[r] = (occupied && occupied[base + r]) ? INT_MAX : -1;      // vpMatched[idx] at entry
  __syncthreads();
  const int nmatches = sim3_ordered_walk<0>(owner, lane, surv, (int64_t)pair * nmp, nmp, mpDesc, kfOff, kfKp, kfDesc, cellStart, sIdx,
                                            cam, gwInv, ghInv, distLimit, width, candKeys, candCount, bestIdx);
  __syncthreads();
  for (int r = lane; r < nk; r += 64) {
    const int o = owner[r];
    rowPoint[base + r] = (o >= 0 && o != INT_MAX) ? o : -1;
  }
  if (lane == 0) nmatchesOut[pair] = nmatches;
}

// ---------------------------------------------------------------------------
// Relocalisation's ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2325-2447;
// Tracking.cc:4290, :4304) of ONE frame table against ncand candidates, each with its own point list (rows mpOff[c] .. mpOff[c + 1]
// of mp / mpDesc / mpAngle), its own pose (the frame's Tcw after that candidate's PnP) and its own occupied rows.
//
// The roles are those of the Sim3 search turned round: the searched table is the frame (one "keyframe" for k_fuse_grid, kfOff =
// {0, nf}), the lists belong to the candidates.  The search is ordered in the same way: mvpMapPoints[bestIdx2] = pMP (:2405) closes
// the row to every later point (:2389).
//
//   k_fuse_grid         (unchanged) the cell sort of the frame's table, once for all candidates.
//   k_reloc_project     one thread per point, the DENSE slot = the point's row in the ragged list; reloc_project_point: the gates of
//                       :2351-2374, which are NOT those of fuse_project_point (no z < 0 gate, the image gate closed on both sides,
//                       no viewing-normal gate).
//   k_reloc_candidates  k_window_candidates<1>: octaves in [level - 1, level + 1] (:2376), keys within ORBdist (:2403).
//   k_reloc_assign      one wave per candidate: the owner table of nf ints in LDS, sim3_ordered_walk<1>, then (mbCheckOrientation,
//                       :2408-2444) the 30-bin histogram over the rows taken, ComputeThreeMaxima, the filter and the corrected
//                       count.  A row that the filter gives back was closed during the whole walk, as in the reference.
// Four launches per call, whatever ncand and the lists.
// ---------------------------------------------------------------------------

// One point up to the window search, :2351-2374 in the reference's order.  true: S holds the projection, the level and the radius.
__device__ __forceinline__ bool reloc_project_point(const pli_fuse_point& P, const float* __restrict__ T /* Rcw row major, tcw, Ow */,
                                                    const pli_fuse_camera& cam, float th, const float* __restrict__ levelRatio,
                                                    int nlevels, const float* __restrict__ scaleFactor, FuseSurvivor& S) {
  float pc[3];
  for (int r = 0; r < 3; ++r) pc[r] = cvmat_dot3(T + 3 * r, 1, P.pos, 1.0, (double)T[9 + r]);      // Rcw*x3Dw + tcw :2351
  const float x = pc[0], y = pc[1], z = pc[2];                   // no z < 0 gate: a point behind the camera is searched too
  S.u = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fx, x), z), cam.cx);   // Pinhole::project, Pinhole.cpp:30-33
  S.v = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fy, y), z), cam.cy);
  // :2355-2358, closed on both sides; written so that a NaN leaves (the reference would convert it to int: undefined)
  if (!(S.u >= cam.min_x && S.u <= cam.max_x && S.v >= cam.min_y && S.v <= cam.max_y)) return false;
  return project_point_tail<false>(P, T, th, levelRatio, nlevels, scaleFactor, S);         // :2360-2374; no viewing-normal gate
}

// grid = ceil(npts / 256), npts = mpOff[ncand]
__global__ __launch_bounds__(256) void k_reloc_project(const pli_fuse_point* __restrict__ mp, const int* __restrict__ mpOff, int ncand,
                                                       const float* __restrict__ pose, pli_fuse_camera cam, float th,
                                                       const float* __restrict__ levelRatio, int nlevels,
                                                       const float* __restrict__ scaleFactor, FuseSurvivor* __restrict__ surv,
                                                       int* __restrict__ candCount, int* __restrict__ bestIdx) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= mpOff[ncand]) return;
  const float* T = pose + (int64_t)owning_table(mpOff, ncand, slot) * 15;                  // the pose of the point's candidate
  const pli_fuse_point P = mp[slot];
  dense_slot_store(slot, 0, slot, P.valid != 0,                  // kf 0: the frame's table; pMP, !isBad(), !sAlreadyFound :2345-2347
                   [&](FuseSurvivor& S) { return reloc_project_point(P, T, cam, th, levelRatio, nlevels, scaleFactor, S); }, surv,
                   candCount, bestIdx);
}

// grid = candidates, one wave; LDS: nf ints (the owner table) and 48 ints (the histogram and ComputeThreeMaxima's bins)
__global__ __launch_bounds__(64) void k_reloc_assign(const FuseSurvivor* __restrict__ surv, const int* __restrict__ mpOff,
                                                     const uint8_t* __restrict__ mpDesc, const float* __restrict__ mpAngle,
                                                     const int* __restrict__ fOff, const pli_keypoint* __restrict__ fKp,
                                                     const uint8_t* __restrict__ fDesc, int nf, const uint8_t* __restrict__ occupied,
                                                     const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx,
                                                     pli_fuse_camera cam, int distLimit, int width, int checkOri,
                                                     const unsigned long long* __restrict__ candKeys,
                                                     const int* __restrict__ candCount, int* __restrict__ rowPoint,
                                                     int* __restrict__ bestIdx, int* __restrict__ nmatchesOut) {
  extern __shared__ int relocLds[];
  int* hist = relocLds;                                          // 30 bins (32 ints)
  int* keep = relocLds + 32;                                     // the bins ComputeThreeMaxima keeps
  int* owner = relocLds + 48;
  const int cand = blockIdx.x, lane = threadIdx.x;
  const int slot0 = mpOff[cand], nmp = mpOff[cand + 1] - slot0;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  const uint8_t* occ = occupied ? occupied + (int64_t)cand * nf : nullptr;
  if (lane < 48) relocLds[lane] = 0;
  for (int r = lane; r < nf; r += 64) owner[r] = (occ && occ[r]) ? INT_MAX : -1;           // mvpMapPoints[i2] at entry :2389
  __syncthreads();
  const int taken = sim3_ordered_walk<1>(owner, lane, surv, (int64_t)slot0, nmp, mpDesc, fOff, fKp, fDesc, cellStart, sIdx, cam, gwInv,
                                         ghInv, distLimit, width, candKeys, candCount, bestIdx);
  __syncthreads();
  if (checkOri) {                                                // :2408-2418, over the rows taken (the order of the votes is free)
    for (int r = lane; r < nf; r += 64) {
      const int o = owner[r];
      if (o >= 0 && o != INT_MAX) atomicAdd(&hist[bow_rot_bin(mpAngle[slot0 + o], fKp[r].angle)], 1);
    }
    __syncthreads();
  }
  if (lane == 0) nmatchesOut[cand] = bow_keep_bins(hist, taken, checkOri, keep);           // :2425-2444
  __syncthreads();
  const int ind1 = keep[0], ind2 = keep[1], ind3 = keep[2];
  int* row = rowPoint + (int64_t)cand * nf;
  for (int r = lane; r < nf; r += 64) {
    int o = owner[r];
    if (o < 0 || o == INT_MAX) o = -1;
    else if (checkOri) {
      const int b = bow_rot_bin(mpAngle[slot0 + o], fKp[r].angle);
      if (b != ind1 && b != ind2 && b != ind3) o = -1;           // :2439
    }
    row[r] = o;
  }
}

// ---------------------------------------------------------------------------
// Monocular initialisation's ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
// (ORBmatcher.cc:706-821; Tracking.cc:2109-2110) of one F1 table against one F2 table.
//
// The walk over i1 is ordered, but a row of F2 is not closed once taken: its state is (vMatchedDistance, vnMatches21), a candidate is
// left out for i1 when vMatchedDistance[i2] <= dist (:745), and a later i1 with a strictly smaller distance takes the row again and
// evicts the earlier owner (:764-768).  The windows and the Hamming distances do not depend on that state, so:
//
//   k_fuse_grid        (unchanged) the cell sort of F2's table (one "keyframe", {0, n2}).
//   k_init_candidates  one wave per i1 with octave 0 (:723), a fixed grid striding over i1: the window of
//                      Frame::GetFeaturesInArea(x, y, r, 0, 0) (Frame.cc:774-843) around vbPrevMatched[i1] in the cell runs, 64 rows
//                      per step; the keys (distance, cell column, cell row, index) within the limit go to the list of i1 (`width`
//                      keys, in visiting order, placed by ballot and popcount: no atomics, nothing to clear) and are counted; the
//                      count keeps counting past the width, count > width marks the list as overflowed.
//   k_init_assign      ONE wave, the per-row state (distance << 16 | owner, all ones: INT_MAX / -1) and vnMatches12 (shorts) in LDS:
//                      walks the i1 that have candidates in order (the next one's keys in flight), drops the left-out keys, takes
//                      the two smallest keys of the wave = bestDist / bestIdx2 (the first strict minimum in visiting order) and
//                      bestDist2, applies :760-762 in float, evicts, stores.  An overflowed list walks its window again.  The
//                      histogram counts every acceptance, also those evicted later (:774-784: nothing leaves rotHist), and
//                      ComputeThreeMaxima sees those sizes; the filter clears only the entries that still hold a match (:805).
// The limit of the lists is the host's (pli_search_for_initialization, where the argument is written down).
// Three launches per call, whatever n1 and n2.
// ---------------------------------------------------------------------------
constexpr unsigned INIT_NO_OWNER = 0xFFFFu;

// The window of (x, y, r) in F2's cell runs by a whole wave in uniform steps: every lane calls visit(key) the same number of
// times, key = ~0ull where the lane has no row, the row is outside the window (strict, Frame.cc:836), not at octave 0 or its
// distance is above distLimit.
template <class Visit>
__device__ __forceinline__ void init_window(float x, float y, float r, const uint64_t dq[4], int lane,
                                            const pli_keypoint* __restrict__ kp2, const uint8_t* __restrict__ desc2,
                                            const int* __restrict__ cellStart, const uint16_t* __restrict__ sIdx,
                                            const pli_fuse_camera& cam, float gwInv, float ghInv, int distLimit, Visit visit) {
  const CellWindow w(x, y, r, cam, gwInv, ghInv);
  if (w.empty()) return;
  for (int cx = w.c0; cx <= w.c1; ++cx) {
    const int lo = cellStart[cx * GRID_ROWS + w.r0], hi = cellStart[cx * GRID_ROWS + w.r1 + 1];
    for (int t0 = lo; t0 < hi; t0 += 64) {
      unsigned long long key = ~0ull;
      if (t0 + lane < hi) {
        const int i2 = sIdx[t0 + lane];
        const pli_keypoint k = kp2[i2];
        if (k.octave == 0 && fabsf(__fsub_rn(k.x, x)) < r && fabsf(__fsub_rn(k.y, y)) < r) {           // Frame.cc:826-837
          uint64_t d2[4];
          load_desc(desc2 + (int64_t)i2 * 32, d2);
          const int dist = hamming256(dq, d2);
          if (dist <= distLimit) key = cell_key(dist, k, cam, gwInv, ghInv, i2);
        }
      }
      visit(key);
    }
  }
}

// a fixed grid of 256-thread blocks, one wave per i1.  candKeys: n1 x width, candCount: n1 (every entry is written)
__global__ __launch_bounds__(256) void k_init_candidates(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1, int n1,
                                                         const float* __restrict__ prevMatched, const pli_keypoint* __restrict__ kp2,
                                                         const uint8_t* __restrict__ desc2, const int* __restrict__ cellStart,
                                                         const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, float radius,
                                                         int distLimit, int width, unsigned long long* __restrict__ candKeys,
                                                         int* __restrict__ candCount) {
  const int lane = threadIdx.x & 63, wavesPerBlock = 256 / 64;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  for (int i1 = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); i1 < n1; i1 += gridDim.x * wavesPerBlock) {
    int count = 0;
    if (kp1[i1].octave == 0) {                                   // :723 (the octaves are checked: none is negative)
      uint64_t dq[4];
      load_desc(desc1 + (int64_t)i1 * 32, dq);
      unsigned long long* keys = candKeys + (int64_t)i1 * width;
      init_window(prevMatched[2 * i1], prevMatched[2 * i1 + 1], radius, dq, lane, kp2, desc2, cellStart, sIdx, cam, gwInv, ghInv,
                  distLimit, [&](unsigned long long key) {
                    const unsigned long long pass = __builtin_amdgcn_ballot_w64(key != ~0ull);
                    const int pos = count + __popcll(pass & ((1ull << lane) - 1ull));
                    if (key != ~0ull && pos < width) keys[pos] = key;
                    count += __popcll(pass);
                  });
    }
    if (lane == 0) candCount[i1] = count;
  }
}

// grid = 1, one wave; LDS: 48 ints (the histogram and ComputeThreeMaxima's bins), n2 words (the row state), n1 shorts (vnMatches12)
__global__ __launch_bounds__(64) void k_init_assign(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1, int n1,
                                                    const float* __restrict__ prevMatched, const pli_keypoint* __restrict__ kp2,
                                                    const uint8_t* __restrict__ desc2, int n2, const int* __restrict__ cellStart,
                                                    const uint16_t* __restrict__ sIdx, pli_fuse_camera cam, float radius,
                                                    int distLimit, int width, float nnratio, int checkOri,
                                                    const unsigned long long* __restrict__ candKeys,
                                                    const int* __restrict__ candCount, int* __restrict__ matches12,
                                                    int* __restrict__ raw12, int* __restrict__ nmatchesOut) {
  extern __shared__ int initLds[];
  int* hist = initLds;                                           // 30 bins (32 ints)
  int* keep = initLds + 32;                                      // the bins ComputeThreeMaxima keeps
  unsigned* state = reinterpret_cast<unsigned*>(initLds + 48);   // vMatchedDistance[i2] << 16 | vnMatches21[i2]
  short* m12 = reinterpret_cast<short*>(state + n2);             // vnMatches12 (n2 <= 8192)
  const int lane = threadIdx.x;
  const float gwInv = __fdiv_rn((float)GRID_COLS, __fsub_rn(cam.max_x, cam.min_x));
  const float ghInv = __fdiv_rn((float)GRID_ROWS, __fsub_rn(cam.max_y, cam.min_y));
  if (lane < 48) initLds[lane] = 0;
  for (int r = lane; r < n2; r += 64) state[r] = ~0u;            // INT_MAX, -1 :716-717
  for (int i = lane; i < n1; i += 64) m12[i] = -1;               // :709
  __syncthreads();
  OrderedCursor cur(candCount, candKeys, n1, width, lane);       // the i1 that have candidates, in order
  while (cur.i < n1) {
    const int i1 = cur.i, cnt = cur.cnt;
    const unsigned long long key = cur.key;
    cur.advance();                                               // the next i1's keys travel while this one is decided
    WaveTop2 top;
    if (cnt <= width) {
      if (key != ~0ull && (state[key_row(key)] >> 16) > (unsigned)key_dist(key)) top.push(key);                 // :745
    } else {                                                     // more candidates than the list holds: the window again
      uint64_t dq[4];
      load_desc(desc1 + (int64_t)i1 * 32, dq);
      init_window(prevMatched[2 * i1], prevMatched[2 * i1 + 1], radius, dq, lane, kp2, desc2, cellStart, sIdx, cam, gwInv, ghInv,
                  distLimit, [&](unsigned long long kk) {
                    if (kk != ~0ull && (state[key_row(kk)] >> 16) > (unsigned)key_dist(kk)) top.push(kk);
                  });
    }
    const unsigned long long k1 = top.min1();
    if (k1 != ~0ull) {
      const unsigned long long k2 = top.min2(k1);
      const int bestDist = key_dist(k1), bestDist2 = k2 != ~0ull ? key_dist(k2) : INT_MAX;
      if (bestDist <= FUSE_TH_LOW && (float)bestDist < __fmul_rn((float)bestDist2, nnratio)) {         // :760-762
        const int b = key_row(k1);
        const unsigned old = state[b] & 0xFFFFu;                 // (every lane reads and stores the same values)
        if (old != INIT_NO_OWNER) m12[old] = -1;                 // :764-768
        m12[i1] = (short)b;
        state[b] = ((unsigned)bestDist << 16) | (unsigned)i1;    // :770-771
        if (checkOri && lane == 0) ++hist[bow_rot_bin(kp1[i1].angle, kp2[b].angle)];       // :774-784, never taken back
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // single wave: LDS is executed in order
  }
  __syncthreads();
  if (lane == 0) bow_keep_bins(hist, 0, checkOri, keep);         // :796 (the count comes from the entries that are left)
  __syncthreads();
  const int ind1 = keep[0], ind2 = keep[1], ind3 = keep[2];
  int left = 0;
  for (int i1 = lane; i1 < n1; i1 += 64) {
    int m = m12[i1];
    if (raw12) raw12[i1] = m;
    if (m >= 0 && checkOri) {
      const int bin = bow_rot_bin(kp1[i1].angle, kp2[m].angle);
      if (bin != ind1 && bin != ind2 && bin != ind3) m = -1;     // :798-811, only where a match is still held (:805)
    }
    matches12[i1] = m;
    left += m >= 0 ? 1 : 0;
  }
  left = wave_sum_i32(left);                                     // nmatches: ++ :772, -- :767 and :808 = the entries left
  if (lane == 0) nmatchesOut[0] = left;
}

// ---------------------------------------------------------------------------
// SURVEY §8(f) row 4, fisheye stereo.
// Frame::ComputeStereoFishEyeMatches (Frame.cc:1577-1618): after knnMatch(k = 2) of the lapping-area descriptors (k_knn2),
// Lowe's ratio 0.7 and KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:334-402) per surviving pair:
// unproject both keypoints (Newton on the distortion polynomial, :103-130), parallax test, linear triangulation (:422-435),
// positive depths, reprojection errors against 5.991 * sigma^2 (project, :28-42).
// One thread per left lapping-area keypoint; cv::Mat arithmetic as OpenCV 3.3.1 evaluates it: gemm = double accumulation and
// one rounding, Mat::dot / norm in double, cv::SVD::compute = the one-sided float Jacobi of lapack.cpp (4x4, <= 30 sweeps,
// hypot as sqrt(p*p + beta*beta)), libm calls on floats in double and rounded.  Same statement as the checker's
// (match_oracle.hpp kb8TriangulateMatches), operation for operation.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void kb8_unproject(const Kb8& c, float u, float v, float r[3]) {
  const float pwx = (u - c.cx) / c.fx, pwy = (v - c.cy) / c.fy;
  float scale = 1.f;
  float theta_d = sqrtf(pwx * pwx + pwy * pwy);
  theta_d = fminf(fmaxf((float)(-3.1415926535897932384626433832795 / 2.0), theta_d), (float)(3.1415926535897932384626433832795 / 2.0));
  if ((double)theta_d > 1e-8) {
    float theta = theta_d;
    for (int j = 0; j < 10; j++) {
      const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
      const float k0t2 = c.k0 * theta2, k1t4 = c.k1 * theta4, k2t6 = c.k2 * theta6, k3t8 = c.k3 * theta8;
      const float fix = (theta * (1 + k0t2 + k1t4 + k2t6 + k3t8) - theta_d) / (1 + 3 * k0t2 + 5 * k1t4 + 7 * k2t6 + 9 * k3t8);
      theta = theta - fix;
      if (fabsf(fix) < 1e-6f) break;                  // KannalaBrandt8::precision
    }
    scale = (float)tan((double)theta) / theta_d;
  }
  r[0] = pwx * scale; r[1] = pwy * scale; r[2] = 1.f;
}

__device__ __forceinline__ void kb8_project(const Kb8& c, const float p[3], float& u, float& v) {
  const float x2y2 = p[0] * p[0] + p[1] * p[1];
  const float theta = (float)atan2((double)sqrtf(x2y2), (double)p[2]);
  const float psi = (float)atan2((double)p[1], (double)p[0]);
  const float t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
  const float r = theta + c.k0 * t3 + c.k1 * t5 + c.k2 * t7 + c.k3 * t9;
  u = (float)((double)(c.fx * r) * cos((double)psi) + (double)c.cx);
  v = (float)((double)(c.fy * r) * sin((double)psi) + (double)c.cy);
}

// last row of vt of cv::SVD::compute(A) for a 4x4 CV_32F matrix; At = A transposed
__device__ __forceinline__ void jacobi_svd_last_vt4(float At[4][4], float out[4]) {
  double W[4];
  float Vt[4][4];
  const float eps = 2.384185791015625e-07f;             // FLT_EPSILON * 2
  for (int i = 0; i < 4; i++) {
    double sd = 0;
    for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * t; }
    W[i] = sd;
    for (int k = 0; k < 4; k++) Vt[i][k] = 0;
    Vt[i][i] = 1;
  }
  for (int iter = 0; iter < 30; iter++) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = i + 1; j < 4; j++) {
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < 4; k++) p += (double)At[i][k] * At[j][k];
        if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = sqrt(p * p + beta * beta);
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)sqrt(delta / gamma);
          c = (float)(p / (gamma * s * 2));
        } else {
          c = (float)sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * c * 2));
        }
        a = b = 0;
        for (int k = 0; k < 4; k++) {
          const float t0 = c * At[i][k] + s * At[j][k];
          const float t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0; At[j][k] = t1;
          a += (double)t0 * t0; b += (double)t1 * t1;
        }
        W[i] = a; W[j] = b;
        changed = true;
        for (int k = 0; k < 4; k++) {
          const float t0 = c * Vt[i][k] + s * Vt[j][k];
          const float t1 = -s * Vt[i][k] + c * Vt[j][k];
          Vt[i][k] = t0; Vt[j][k] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < 4; i++) {
    double sd = 0;
    for (int k = 0; k < 4; k++) { const float t = At[i][k]; sd += (double)t * t; }
    W[i] = sqrt(sd);
  }
  // the descending selection sort of lapack.cpp only matters for where the smallest singular value ends up: row 3 takes
  // part in a swap at step i iff it holds the maximum of W[i..3] (the first maximum wins: W[j] < W[k] is strict)
  int idx[4] = {0, 1, 2, 3};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int j = i;
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      const double tw = W[i]; W[i] = W[j]; W[j] = tw;
      const int ti = idx[i]; idx[i] = idx[j]; idx[j] = ti;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (idx[3] == r)
      for (int k = 0; k < 4; k++) out[k] = Vt[r][k];
}

// KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:338-402) from the two unprojected rays on: the parallax test, the linear
// triangulation, both depths and both reprojection gates, the same operations in the same order for every caller.  (x1, y1) and
// (x2, y2) are the keypoints' coordinates, sigmaLevel / unc their mvLevelSigma2.  Returns z1 and x3 = x3D, or -1 as the reference
// does (x3 is then not meaningful); the caller applies its own floor on the depth (Frame.cc:1609, KannalaBrandt8.cpp:237).
__device__ __forceinline__ float kb8_triangulate_rays(const Kb8& c1, const Kb8& c2, const float r1[3], const float r2[3], float x1,
                                                      float y1, float x2, float y2, const float* __restrict__ R12,
                                                      const float* __restrict__ t12, float sigmaLevel, float unc, float x3[3]) {
  float r21[3];
  for (int a = 0; a < 3; ++a) r21[a] = cvmat_dot3(R12 + 3 * a, 1, r2, 1.0, 0.0);
  const double dot = (double)r1[0] * r21[0] + (double)r1[1] * r21[1] + (double)r1[2] * r21[2];
  const double n1 = sqrt((double)r1[0] * r1[0] + (double)r1[1] * r1[1] + (double)r1[2] * r1[2]);
  const double n2 = sqrt((double)r21[0] * r21[0] + (double)r21[1] * r21[1] + (double)r21[2] * r21[2]);
  const float cosPar = (float)(dot / (n1 * n2));
  if ((double)cosPar > 0.9998) return -1.f;
  // Tcw1 = [I | 0], Tcw2 = [R21 | t21] with R21 = R12^T, t21 = -R21 t12
  float R21[9], t21[3];
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) R21[3 * a + b] = R12[3 * b + a];
  for (int a = 0; a < 3; ++a) t21[a] = cvmat_dot3(R21 + 3 * a, 1, t12, -1.0, 0.0);
  const float T1[3][4] = {{1.f, 0.f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.f, 1.f, 0.f}};
  float T2[3][4];
  for (int a = 0; a < 3; ++a) { T2[a][0] = R21[3 * a]; T2[a][1] = R21[3 * a + 1]; T2[a][2] = R21[3 * a + 2]; T2[a][3] = t21[a]; }
  float At[4][4];
  for (int b = 0; b < 4; ++b) {
    At[b][0] = r1[0] * T1[2][b] - T1[0][b];
    At[b][1] = r1[1] * T1[2][b] - T1[1][b];
    At[b][2] = r2[0] * T2[2][b] - T2[0][b];
    At[b][3] = r2[1] * T2[2][b] - T2[1][b];
  }
  float vh[4];
  jacobi_svd_last_vt4(At, vh);
  const float inv = (float)(1.0 / (double)vh[3]);
  x3[0] = vh[0] * inv + 0.f; x3[1] = vh[1] * inv + 0.f; x3[2] = vh[2] * inv + 0.f;
  const float z1 = x3[2];
  if (!(z1 > 0)) return -1.f;                           // z1 <= 0 (or NaN: the callers' `depth > 0.0001f` fails for it in the reference)
  const float z2 = (float)(((double)R21[6] * x3[0] + (double)R21[7] * x3[1] + (double)R21[8] * x3[2]) + (double)t21[2]);
  if (z2 <= 0) return -1.f;
  float u1, v1;
  kb8_project(c1, x3, u1, v1);
  const float ex1 = u1 - x1, ey1 = v1 - y1;
  if ((double)(ex1 * ex1 + ey1 * ey1) > 5.991 * (double)sigmaLevel) return -1.f;
  float x32[3];
  for (int a = 0; a < 3; ++a) x32[a] = cvmat_dot3(R21 + 3 * a, 1, x3, 1.0, (double)t21[a]);
  float u2, v2;
  kb8_project(c2, x32, u2, v2);
  const float ex2 = u2 - x2, ey2 = v2 - y2;
  if ((double)(ex2 * ex2 + ey2 * ey2) > 5.991 * (double)unc) return -1.f;
  return z1;
}

__global__ __launch_bounds__(64) void k_fisheye_triangulate(const pli_keypoint* __restrict__ kpL, const pli_keypoint* __restrict__ kpR,
                                                            const int* __restrict__ knnIdx, const int* __restrict__ knnDist, int nl, int nr,
                                                            int monoL, int monoR, Kb8 c1, Kb8 c2, const float* __restrict__ R12t12,
                                                            const float* __restrict__ sigma2, int* __restrict__ l2r, int* __restrict__ r2l,
                                                            float* __restrict__ depth, float* __restrict__ p3d, int* __restrict__ nmatches) {
  const int i = blockIdx.x * 64 + threadIdx.x;          // index into the lapping-area (stereo) part of the left table
  if (i >= nl || nr < 2) return;                        // (*it).size() >= 2
  const int d0 = knnDist[2 * i], d1 = knnDist[2 * i + 1], j = knnIdx[2 * i];
  if (!((double)(float)d0 < (double)(float)d1 * 0.7)) return;
  const pli_keypoint k1 = kpL[monoL + i], k2 = kpR[monoR + j];
  float r1[3], r2[3], x3[3];
  kb8_unproject(c1, k1.x, k1.y, r1);
  kb8_unproject(c2, k2.x, k2.y, r2);
  const float z1 = kb8_triangulate_rays(c1, c2, r1, r2, k1.x, k1.y, k2.x, k2.y, R12t12, R12t12 + 9, sigma2[k1.octave], sigma2[k2.octave],
                                        x3);
  if (!(z1 > 0.0001f)) return;
  l2r[monoL + i] = monoR + j;
  atomicMax(&r2l[monoR + j], monoL + i);        // the reference's loop overwrites: the LAST left keypoint that takes a right one stays
  depth[monoL + i] = z1;
  p3d[3 * (monoL + i)] = x3[0]; p3d[3 * (monoL + i) + 1] = x3[1]; p3d[3 * (monoL + i) + 2] = x3[2];
  atomicAdd(nmatches, 1);
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchForTriangulation (ORBmatcher.cc:965-1206), the branch pKF1->mpCamera2 && pKF2->mpCamera2 (a rig of two
// KannalaBrandt8 cameras, NLeft != -1): a keyframe's N = NLeft + NRight features are the left camera's first, their keypoints
// mvKeys / mvKeysRight (:1048-1053, :1083-1087), and the gate of a candidate pair is KannalaBrandt8::epipolarConstrain
// (KannalaBrandt8.cpp:235-238) = TriangulateMatches(...) > 0.0001f with the relative pose and the two cameras that
// (bRight1, bRight2) pick (:1099-1129).  bStereo1 / bStereo2 are false (:1041, :1070) and the epipole gate is skipped (:1089).
// What k_tri_match's header says about vbMatched2 and the key holds unchanged.
//
//   k_kb8_rays          one thread per feature of pKF1 and of every neighbour: its ray, KannalaBrandt8::unproject with the camera
//                       of its side.  The ray depends on the keypoint and its own camera only, so the Newton steps and the tan
//                       leave the candidate loop; the stored floats are the ones TriangulateMatches would compute again.
//   k_node_sort         (above) as for k_tri_match, without the stereo flag.
//   k_tri_match_kb8     tri_match_body with TriKb8Gate, a kernel of its own because the gate needs five times k_tri_match's
//                       registers: Hamming distance and TH_LOW first (:1080), then, in the lane that holds the survivor, the gate.
//   k_tri_finish        (above) unchanged.
// ---------------------------------------------------------------------------
// grid = ceil((n1 + total) / 256): item i < n1 is feature i of pKF1, the others the neighbours' rows in table order
__global__ __launch_bounds__(256) void k_kb8_rays(const pli_keypoint* __restrict__ kp1, int n1, int n1Left,
                                                  const pli_keypoint* __restrict__ kfKp, const int* __restrict__ kfOff,
                                                  const int* __restrict__ kfNleft, int nkf, Kb8 camL, Kb8 camR,
                                                  float2* __restrict__ ray1, float2* __restrict__ kfRay) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = kfOff[nkf];
  if (i >= n1 + total) return;
  pli_keypoint k;
  bool right;
  if (i < n1) {
    k = kp1[i];
    right = i >= n1Left;
  } else {
    const int row = i - n1;
    const int nb = owning_table(kfOff, nkf, row);        // the neighbour that owns the row
    k = kfKp[row];
    right = row - kfOff[nb] >= kfNleft[nb];
  }
  float r[3];
  if (right) kb8_unproject(camR, k.x, k.y, r);
  else kb8_unproject(camL, k.x, k.y, r);
  if (i < n1) ray1[i] = make_float2(r[0], r[1]);
  else kfRay[i - n1] = make_float2(r[0], r[1]);
}

// the two-camera gate: KannalaBrandt8::epipolarConstrain with the relative pose and the cameras that (bRight1, bRight2) pick
// (:1099-1132); no stereo features and no epipole gate (:1041, :1070, :1089)
struct TriKb8Gate {
  const uint8_t* __restrict__ hasMp1;
  const pli_keypoint* __restrict__ kfKp;
  const float2 *__restrict__ ray1, *__restrict__ kfRay;
  const float *__restrict__ rel, *__restrict__ sigma2;             // rel: the neighbour's ll, lr, rl, rr
  const Kb8 &camL, &camR;
  int n1Left, nleft2, base, coarse;
  pli_keypoint k1;                                                 // of idx1 (begin):
  bool right1;
  float r1[3], s1;
  __device__ __forceinline__ bool admits(int idx1) const { return !hasMp1[idx1]; }         // :1036-1039
  __device__ __forceinline__ void begin(int idx1, const pli_keypoint& k) {
    k1 = k;
    right1 = idx1 >= n1Left;                                       // :1052
    const float2 q1 = ray1[idx1];
    r1[0] = q1.x; r1[1] = q1.y; r1[2] = 1.f;
    s1 = sigma2[k1.octave];
  }
  __device__ __forceinline__ bool keeps(int idx2) const {
    if (coarse) return true;                                       // :1099-1132
    const pli_keypoint k2 = kfKp[base + idx2];
    const bool right2 = idx2 >= nleft2;                            // :1086
    const float2 q2 = kfRay[base + idx2];
    const float r2[3] = {q2.x, q2.y, 1.f};
    const float* Rt = rel + ((right1 ? 2 : 0) + (right2 ? 1 : 0)) * 12;
    float x3[3];
    const float z1 = kb8_triangulate_rays(right1 ? camR : camL, right2 ? camR : camL, r1, r2, k1.x, k1.y, k2.x, k2.y, Rt, Rt + 9, s1,
                                          sigma2[k2.octave], x3);
    return z1 > 0.0001f;                                           // KannalaBrandt8.cpp:237
  }
};

// grid = (ceil(n1 / (waves per block * TRI_PER_WAVE)), neighbours); rel: per neighbour ll, lr, rl, rr, each R12 row major then t12
__global__ __launch_bounds__(256) void k_tri_match_kb8(const pli_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1,
                                                       const int* __restrict__ node1, const uint8_t* __restrict__ hasMp1,
                                                       const float2* __restrict__ ray1, int n1, int n1Left,
                                                       const int* __restrict__ kfOff, const int* __restrict__ kfNleft,
                                                       const pli_keypoint* __restrict__ kfKp, const uint8_t* __restrict__ kfDesc,
                                                       const float2* __restrict__ kfRay, const uint32_t* __restrict__ sNode,
                                                       const uint16_t* __restrict__ sIdx, const int* __restrict__ nListed,
                                                       const float* __restrict__ rel, Kb8 camL, Kb8 camR,
                                                       const float* __restrict__ sigma2, int coarse, int checkOri,
                                                       int* __restrict__ matches12, int* __restrict__ stat) {
  const int kf = blockIdx.y, base = kfOff[kf];
  TriKb8Gate gate{hasMp1, kfKp, ray1, kfRay, rel + (int64_t)kf * 48, sigma2, camL, camR, n1Left, kfNleft[kf], base, coarse};
  tri_match_body(kp1, desc1, node1, n1, base, kfKp, kfDesc, sNode, sIdx, nListed, checkOri, matches12, stat, gate);
}

// ---------------------------------------------------------------------------
// The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (ORBmatcher.cc:1399-1609) for keyframes with two
// KannalaBrandt8 cameras (NLeft != -1), both values of bRight of a batch of keyframes in one call (LocalMapping.cc:747-748,
// :776-777).  A keyframe's camera is a VIEW: view 2k is keyframe k's left rows (mvKeys, the grid mGrid), view 2k + 1 its right
// rows (mvKeysRight, mGridRight with camera-local indices, Frame.cc:468-481).  The offset list {off_k, off_k + NLeft_k, ...,
// off_nkf} of 2 nkf + 1 entries makes every view a "keyframe" of k_fuse_grid and cell_window_walk, which run unchanged.
//
//   k_fuse_grid            (unchanged) the cell sort of every view.
//   k_fuse_project_views   one thread per (view, point): Rcw * p + tcw with the view's pose (GetRotation() / GetRightRotation()
//                          ..., KeyFrame.cc:1343-1373: host arithmetic), z < 0 (:1459), KannalaBrandt8::project with the view's
//                          camera (kb8_project, :1470), IsInImage, then project_point_tail<true> with the view's Ow.  A view whose
//                          side is not asked for keeps -1 / 256.  Survivors are compacted as in k_fuse_project.
//   k_fuse_match<8, true>  the window walk with the 5.99 gate alone (every mvuRight of such a keyframe is -1, Frame.cc:1589) and
//                          the right view's winner + NLeft (:1559).
// Three launches per call, whatever nkf and nmp.
// ---------------------------------------------------------------------------
// grid = ceil(2 * nkf * nmp / 256); kfPose: nkf x 2 x 15, skip: nkf x 2 x nmp or null; sides: bit 0 = left, bit 1 = right
__global__ __launch_bounds__(256) void k_fuse_project_views(const pli_fuse_point* __restrict__ mp, int nmp, int nkf,
                                                            const float* __restrict__ kfPose, const uint8_t* __restrict__ skip,
                                                            Kb8 camL, Kb8 camR, pli_fuse_camera bounds, int sides, float th,
                                                            const float* __restrict__ levelRatio, int nlevels,
                                                            const float* __restrict__ scaleFactor, FuseSurvivor* __restrict__ surv,
                                                            int* __restrict__ nSurv, int* __restrict__ bestIdx,
                                                            int* __restrict__ bestDist) {
  const int64_t pair = (int64_t)blockIdx.x * 256 + threadIdx.x, npairs = (int64_t)2 * nkf * nmp;
  bool keep = false;
  FuseSurvivor S;
  if (pair < npairs) {
    const int view = (int)(pair / nmp), i = (int)(pair - (int64_t)view * nmp);
    S.kf = view; S.mp = i; S.pad = 0; S.ur = 0.f;
    bestIdx[pair] = -1;
    if (bestDist) bestDist[pair] = 256;
    const pli_fuse_point P = mp[i];
    if (((sides >> (view & 1)) & 1) && P.valid && !(skip && skip[pair])) {     // !pMP, isBad(), IsInKeyFrame(pKF) :1435-1452
      const float* T = kfPose + (int64_t)view * 15;
      float pc[3];
      for (int r = 0; r < 3; ++r) pc[r] = cvmat_dot3(T + 3 * r, 1, P.pos, 1.0, (double)T[9 + r]);  // Rcw*p3Dw + tcw :1456
      if (!(pc[2] < 0.0f)) {                                                   // :1459
        kb8_project((view & 1) ? camR : camL, pc, S.u, S.v);                   // pCamera->project :1470
        if (S.u >= bounds.min_x && S.u < bounds.max_x && S.v >= bounds.min_y && S.v < bounds.max_y)  // KeyFrame::IsInImage :1473
          keep = project_point_tail<true>(P, T, th, levelRatio, nlevels, scaleFactor, S);
      }
    }
  }
  compact_survivor(keep, S, surv, nSurv);
}

// ---------------------------------------------------------------------------
// LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:425-684), keyframes of one pinhole camera (NLeft == -1, no
// mpCamera2), for one keyframe against nkf neighbours (pli_create_new_map_points).  The search is k_node_sort + k_tri_match on the
// map-point state at entry; what the sequential loop adds is, per feature of pKF1, "the first neighbour in which it is matched and
// passes every gate keeps it, every later neighbour does not see it" (ORBmatcher.cc:1033-1039 after AddMapPoint at :675).
//
//   k_newpt_list        one thread per (neighbour, feature): the matched pairs of all neighbours into one list (ballot and popcount
//                       prefix per wave, one atomic per wave; the list's order is free, results are written at (k, i)); the
//                       unmatched ones get their status here.
//   k_newpt_geometry    one lane per listed pair: :530-667 operation for operation, cv::Mat arithmetic as k_tri_match_kb8 and
//                       k_fuse_project state it (a gemm row: double accumulation, one rounding; Mat::dot and cv::norm: sequential
//                       double; s*row - row: the rounded product, then a float subtraction; Mat / s: a multiplication by
//                       (float)(1/s); 1.0/z: the double reciprocal rounded once; the comparisons against 5.991*sigma2, 7.8*sigma2
//                       and 0.9998 in double; a libm call on a float: in double, rounded; the rest float in the written order).
//   k_newpt_pick        one thread per feature of pKF1: walks the neighbours in order, the first status 0 keeps the feature, every
//                       later matched entry becomes -1 / PLI_NEWPT_TAKEN_EARLIER; counts nmatches and nnew per neighbour.
//
// Kept as the reference has them: `else if(bStereo2)` at :544 (the second keyframe's stereo parallax only when the first side is
// not stereo), mpCurrentKeyFrame->mbf in the SECOND keyframe's stereo gate (:641), fx1..cy1 for the first and fx2..cy2 for the
// second keyframe (one pli_fuse_camera serves both here: the call shares its camera), mvKeys (not mvKeysUn) in UnprojectStereo.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_newpt_list(const int* __restrict__ matches12, int npairs, int* __restrict__ list,
                                                    int* __restrict__ nListed, int* __restrict__ status, float* __restrict__ x3d) {
  const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool matched = p < npairs && matches12[p] >= 0;
  if (p < npairs) {
    status[p] = PLI_NEWPT_NOT_MATCHED;                    // (a listed pair: k_newpt_geometry overwrites it)
    x3d[3 * (int64_t)p] = 0.f; x3d[3 * (int64_t)p + 1] = 0.f; x3d[3 * (int64_t)p + 2] = 0.f;
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(matched);
  if (bal == 0) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(nListed, __popcll(bal));
  base = __shfl(base, 0);
  if (matched) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = p;
}

struct NewPtSide {                                       // one keyframe's side of a pair
  float x, y; int octave;                                // mvKeysUn[idx]
  float ur, depth, keyX, keyY;                           // mvuRight[idx], mvDepth[idx], mvKeys[idx].pt
  const float* T;                                        // Rcw row major, tcw, Ow
};

// KeyFrame::UnprojectStereo (KeyFrame.cc:932-948) for z > 0: Twc.rowRange(0,3).colRange(0,3)*x3Dc + Twc.rowRange(0,3).col(3)
__device__ __forceinline__ void newpt_unproject_stereo(const NewPtSide& S, const pli_fuse_camera& cam, float invfx, float invfy,
                                                       float x3[3]) {
  const float xc[3] = {__fmul_rn(__fmul_rn(__fsub_rn(S.keyX, cam.cx), S.depth), invfx),
                       __fmul_rn(__fmul_rn(__fsub_rn(S.keyY, cam.cy), S.depth), invfy), S.depth};
  for (int r = 0; r < 3; ++r) x3[r] = cvmat_dot3(S.T + r, 3, xc, 1.0, (double)S.T[12 + r]);
}

// the reprojection gate of one keyframe (:597-623, :625-648): 0 = passed, 1 = the monocular bound, 2 = the stereo bound.
// mbf is mpCurrentKeyFrame's for both keyframes (:616, :641).
__device__ __forceinline__ int newpt_reproject(const NewPtSide& S, bool stereo, const pli_fuse_camera& cam, float mbf,
                                               const float x3[3], float z, float sigma2) {
  const float* T = S.T;
  const float x = (float)(((double)T[0] * x3[0] + (double)T[1] * x3[1] + (double)T[2] * x3[2]) + (double)T[9]);
  const float y = (float)(((double)T[3] * x3[0] + (double)T[4] * x3[1] + (double)T[5] * x3[2]) + (double)T[10]);
  const float invz = (float)(1.0 / (double)z);
  if (!stereo) {
    const float u = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fx, x), z), cam.cx);          // Pinhole::project, Pinhole.cpp:30-33
    const float v = __fadd_rn(__fdiv_rn(__fmul_rn(cam.fy, y), z), cam.cy);
    const float ex = __fsub_rn(u, S.x), ey = __fsub_rn(v, S.y);
    return (double)__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) > 5.991 * (double)sigma2 ? 1 : 0;
  }
  const float u = __fadd_rn(__fmul_rn(__fmul_rn(cam.fx, x), invz), cam.cx);
  const float ur = __fsub_rn(u, __fmul_rn(mbf, invz));
  const float v = __fadd_rn(__fmul_rn(__fmul_rn(cam.fy, y), invz), cam.cy);
  const float ex = __fsub_rn(u, S.x), ey = __fsub_rn(v, S.y), er = __fsub_rn(ur, S.ur);
  return (double)__fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(er, er)) > 7.8 * (double)sigma2 ? 2 : 0;
}

// cv::norm(x3D - Ow) as a float
__device__ __forceinline__ float newpt_dist(const float x3[3], const float* Ow) {
  double s = 0;
  for (int r = 0; r < 3; ++r) { const float d = __fsub_rn(x3[r], Ow[r]); s += (double)d * d; }
  return (float)sqrt(s);
}

// :534-667 from the point where xn1, xn2 and the two poses (Rcw row major, tcw, Ow) are known, for the pinhole kernel and the
// two-camera one: the ray cosine, the linear triangulation (A, cv::SVD::compute, w == 0, the division), z1 / z2, the distances, the
// far gate and the scale consistency.  What differs between the two is the caller's Rule:
//   parallax(cosRays, x3)    NEWPT_TRIANGULATE where the condition of :550 holds, NEWPT_HAVE_X3 where it wrote x3 itself
//                            (UnprojectStereo), else the status of the exit it took;
//   reproject(second, x3, z) the chi-square gate of the first / second keyframe (:597-623, :625-648): 0 or the status of the exit.
// Returns the status code; x3 is meaningful where it returns PLI_NEWPT_CREATED.
enum { NEWPT_TRIANGULATE = -1, NEWPT_HAVE_X3 = -2 };
template <class Rule>
__device__ __forceinline__ int newpt_from_rays(const float xn1[3], const float xn2[3], const float* T1, const float* T2, int octave1,
                                               int octave2, int farPoints, float thFar, float ratioFactor,
                                               const float* __restrict__ scaleFactor, const Rule& rule, float x3[3]) {
  // ray = Rwc*xn with Rwc = Rcw.t()
  float ray1[3], ray2[3];
  for (int r = 0; r < 3; ++r) { ray1[r] = cvmat_dot3(T1 + r, 3, xn1, 1.0, 0.0); ray2[r] = cvmat_dot3(T2 + r, 3, xn2, 1.0, 0.0); }
  const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
  const double n1 = sqrt((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1] + (double)ray1[2] * ray1[2]);
  const double n2 = sqrt((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1] + (double)ray2[2] * ray2[2]);
  const float cosRays = (float)(dot / (n1 * n2));
  const int how = rule.parallax(cosRays, x3);
  if (how == NEWPT_TRIANGULATE) {
    float At[4][4];                                       // A transposed; Tcw = [Rcw | tcw]
    for (int b = 0; b < 4; ++b) {
      const float t1r0 = b < 3 ? T1[b] : T1[9], t1r1 = b < 3 ? T1[3 + b] : T1[10], t1r2 = b < 3 ? T1[6 + b] : T1[11];
      const float t2r0 = b < 3 ? T2[b] : T2[9], t2r1 = b < 3 ? T2[3 + b] : T2[10], t2r2 = b < 3 ? T2[6 + b] : T2[11];
      At[b][0] = __fsub_rn(__fmul_rn(xn1[0], t1r2), t1r0);
      At[b][1] = __fsub_rn(__fmul_rn(xn1[1], t1r2), t1r1);
      At[b][2] = __fsub_rn(__fmul_rn(xn2[0], t2r2), t2r0);
      At[b][3] = __fsub_rn(__fmul_rn(xn2[1], t2r2), t2r1);
    }
    float vh[4];
    jacobi_svd_last_vt4(At, vh);
    if (vh[3] == 0) return PLI_NEWPT_W_ZERO;
    const float inv = (float)(1.0 / (double)vh[3]);
    for (int r = 0; r < 3; ++r) x3[r] = __fadd_rn(__fmul_rn(vh[r], inv), 0.f);
  } else if (how != NEWPT_HAVE_X3) {
    return how;
  }
  const float z1 = (float)(((double)T1[6] * x3[0] + (double)T1[7] * x3[1] + (double)T1[8] * x3[2]) + (double)T1[11]);
  if (z1 <= 0) return PLI_NEWPT_Z1;
  const float z2 = (float)(((double)T2[6] * x3[0] + (double)T2[7] * x3[1] + (double)T2[8] * x3[2]) + (double)T2[11]);
  if (z2 <= 0) return PLI_NEWPT_Z2;
  int g = rule.reproject(false, x3, z1);
  if (g) return g;
  g = rule.reproject(true, x3, z2);
  if (g) return g;
  const float dist1 = newpt_dist(x3, T1 + 12), dist2 = newpt_dist(x3, T2 + 12);
  if (dist1 == 0 || dist2 == 0) return PLI_NEWPT_DIST_ZERO;
  if (farPoints && (dist1 >= thFar || dist2 >= thFar)) return PLI_NEWPT_FAR;
  const float ratioDist = __fdiv_rn(dist2, dist1);
  const float ratioOctave = __fdiv_rn(scaleFactor[octave1], scaleFactor[octave2]);
  if (__fmul_rn(ratioDist, ratioFactor) < ratioOctave) return PLI_NEWPT_RATIO_LOW;
  if (ratioDist > __fmul_rn(ratioOctave, ratioFactor)) return PLI_NEWPT_RATIO_HIGH;
  return PLI_NEWPT_CREATED;
}

// keyframes of one pinhole camera: the stereo parallax of :543-547 and the branches :550, :576-583; the gates of newpt_reproject
struct NewPtPinholeRule {
  const NewPtSide& S1; const NewPtSide& S2; const pli_fuse_camera& cam; float mb; const float* __restrict__ sigma2;
  __device__ __forceinline__ int parallax(float cosRays, float x3[3]) const {
    const bool stereo1 = S1.ur >= 0, stereo2 = S2.ur >= 0;
    float cosStereo = __fadd_rn(cosRays, 1.f);
    float cosStereo1 = cosStereo, cosStereo2 = cosStereo;
    if (stereo1) cosStereo1 = (float)cos((double)__fmul_rn(2.f, (float)atan2((double)__fdiv_rn(mb, 2.f), (double)S1.depth)));
    else if (stereo2) cosStereo2 = (float)cos((double)__fmul_rn(2.f, (float)atan2((double)__fdiv_rn(mb, 2.f), (double)S2.depth)));
    cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;                   // min(cosParallaxStereo1, cosParallaxStereo2)
    const float invfx = __fdiv_rn(1.0f, cam.fx), invfy = __fdiv_rn(1.0f, cam.fy);     // Frame.cc: invfx = 1.0f/fx
    if (cosRays < cosStereo && cosRays > 0 && (stereo1 || stereo2 || (double)cosRays < 0.9998)) return NEWPT_TRIANGULATE;
    if (stereo1 && cosStereo1 < cosStereo2) {
      if (!(S1.depth > 0)) return PLI_NEWPT_EMPTY_UNPROJECT;
      newpt_unproject_stereo(S1, cam, invfx, invfy, x3);
      return NEWPT_HAVE_X3;
    }
    if (stereo2 && cosStereo2 < cosStereo1) {
      if (!(S2.depth > 0)) return PLI_NEWPT_EMPTY_UNPROJECT;
      newpt_unproject_stereo(S2, cam, invfx, invfy, x3);
      return NEWPT_HAVE_X3;
    }
    return PLI_NEWPT_LOW_PARALLAX;
  }
  __device__ __forceinline__ int reproject(bool second, const float x3[3], float z) const {
    const NewPtSide& S = second ? S2 : S1;
    const int g = newpt_reproject(S, S.ur >= 0, cam, cam.bf, x3, z, sigma2[S.octave]);
    if (!g) return 0;
    return second ? (g == 1 ? PLI_NEWPT_REPROJ2_MONO : PLI_NEWPT_REPROJ2_STEREO) : (g == 1 ? PLI_NEWPT_REPROJ1_MONO : PLI_NEWPT_REPROJ1_STEREO);
  }
};

// :530-667 for one matched pair of pinhole keyframes
__device__ __forceinline__ int newpt_pair(const NewPtSide& S1, const NewPtSide& S2, const pli_fuse_camera& cam, float mb,
                                          int farPoints, float thFar, float ratioFactor, const float* __restrict__ scaleFactor,
                                          const float* __restrict__ sigma2, float x3[3]) {
  // xn = pCamera->unprojectMat(kp.pt) (Pinhole.cpp:59-62)
  const float xn1[3] = {__fdiv_rn(__fsub_rn(S1.x, cam.cx), cam.fx), __fdiv_rn(__fsub_rn(S1.y, cam.cy), cam.fy), 1.f};
  const float xn2[3] = {__fdiv_rn(__fsub_rn(S2.x, cam.cx), cam.fx), __fdiv_rn(__fsub_rn(S2.y, cam.cy), cam.fy), 1.f};
  const NewPtPinholeRule rule = {S1, S2, cam, mb, sigma2};
  return newpt_from_rays(xn1, xn2, S1.T, S2.T, S1.octave, S2.octave, farPoints, thFar, ratioFactor, scaleFactor, rule, x3);
}

// grid-stride over the list (its length is the device's); 64 threads: the Jacobi's registers
__global__ __launch_bounds__(64) void k_newpt_geometry(NewPtTables D, pli_fuse_camera cam, float mb, int farPoints, float thFar,
                                                       float ratioFactor, const int* __restrict__ matches12,
                                                       const int* __restrict__ list, const int* __restrict__ nListed,
                                                       int* __restrict__ status, float* __restrict__ x3d) {
  const int n = *nListed;
  for (int e = blockIdx.x * 64 + threadIdx.x; e < n; e += gridDim.x * 64) {
    const int p = list[e], k = p / D.n1, i = p - k * D.n1;
    const int j = D.kfOff[k] + matches12[p];
    const pli_keypoint a = D.kp1[i], b = D.kfKp[j];
    const float2 ka = D.key1[i], kb = D.kfKey[j];
    const NewPtSide S1 = {a.x, a.y, a.octave, D.ur1[i], D.depth1[i], ka.x, ka.y, D.pose1};
    const NewPtSide S2 = {b.x, b.y, b.octave, D.kfUr[j], D.kfDepth[j], kb.x, kb.y, D.kfPose + 15 * (int64_t)k};
    float x3[3] = {0.f, 0.f, 0.f};
    const int st = newpt_pair(S1, S2, cam, mb, farPoints, thFar, ratioFactor, D.scaleFactor, D.sigma2, x3);
    status[p] = st;
    if (st == PLI_NEWPT_CREATED) { x3d[3 * (int64_t)p] = x3[0]; x3d[3 * (int64_t)p + 1] = x3[1]; x3d[3 * (int64_t)p + 2] = x3[2]; }
  }
}

// The same for keyframes of two KannalaBrandt8 cameras (pli_create_new_map_points_two_cameras, LocalMapping.cc:463-528): no stereo
// feature (bStereo1 / bStereo2 are false when mpCamera2 is set, :450, :459), so :550 is 0 < cosParallaxRays < 0.9998 and everything
// else "no stereo and very low parallax"; both gates are KannalaBrandt8::project against 5.991 * sigmaSquare (:605-610, :632-636).
struct NewPtKb8Rule {
  float x1, y1, x2, y2; int octave1, octave2;             // kp1.pt / kp2.pt: mvKeys or mvKeysRight, never mvKeysUn
  const Kb8& c1; const Kb8& c2;                           // pCamera1 / pCamera2 of the pair
  const float* T1; const float* T2; const float* __restrict__ sigma2;
  __device__ __forceinline__ int parallax(float cosRays, float*) const {
    // cosParallaxStereo = cosParallaxRays + 1 is above cosParallaxRays wherever cosParallaxRays > 0
    return cosRays > 0 && (double)cosRays < 0.9998 ? (int)NEWPT_TRIANGULATE : (int)PLI_NEWPT_LOW_PARALLAX;
  }
  __device__ __forceinline__ int reproject(bool second, const float x3[3], float z) const {
    const float* T = second ? T2 : T1;
    float pc[3];
    pc[0] = (float)(((double)T[0] * x3[0] + (double)T[1] * x3[1] + (double)T[2] * x3[2]) + (double)T[9]);
    pc[1] = (float)(((double)T[3] * x3[0] + (double)T[4] * x3[1] + (double)T[5] * x3[2]) + (double)T[10]);
    pc[2] = z;
    float u, v;
    kb8_project(second ? c2 : c1, pc, u, v);
    const float ex = __fsub_rn(u, second ? x2 : x1), ey = __fsub_rn(v, second ? y2 : y1);
    if ((double)__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) > 5.991 * (double)sigma2[second ? octave2 : octave1])
      return second ? PLI_NEWPT_REPROJ2_MONO : PLI_NEWPT_REPROJ1_MONO;
    return 0;
  }
};

// one lane per listed pair, as k_newpt_geometry.  (bRight1, bRight2) = (i >= n1Left, matches12 >= kfNleft[k]) pick the 15-float
// pose (left, then right, per keyframe) and the camera of each side; xn = unprojectMat(kp.pt) is the ray k_kb8_rays stored, z = 1.
__global__ __launch_bounds__(64) void k_newpt_geometry_kb8(NewPtKb8Tables D, Kb8 camL, Kb8 camR, int farPoints, float thFar,
                                                           float ratioFactor, const int* __restrict__ matches12,
                                                           const int* __restrict__ list, const int* __restrict__ nListed,
                                                           int* __restrict__ status, float* __restrict__ x3d) {
  const int n = *nListed;
  for (int e = blockIdx.x * 64 + threadIdx.x; e < n; e += gridDim.x * 64) {
    const int p = list[e], k = p / D.n1, i = p - k * D.n1;
    const int m = matches12[p], j = D.kfOff[k] + m;
    const bool right1 = i >= D.n1Left, right2 = m >= D.kfNleft[k];
    const pli_keypoint a = D.kp1[i], b = D.kfKp[j];
    const float2 ra = D.ray1[i], rb = D.kfRay[j];
    const float xn1[3] = {ra.x, ra.y, 1.f}, xn2[3] = {rb.x, rb.y, 1.f};
    const float* T1 = D.pose1 + (right1 ? 15 : 0);
    const float* T2 = D.kfPose + 30 * (int64_t)k + (right2 ? 15 : 0);
    const NewPtKb8Rule rule = {a.x, a.y, b.x, b.y, a.octave, b.octave, right1 ? camR : camL, right2 ? camR : camL, T1, T2, D.sigma2};
    float x3[3] = {0.f, 0.f, 0.f};
    const int st = newpt_from_rays(xn1, xn2, T1, T2, a.octave, b.octave, farPoints, thFar, ratioFactor, D.scaleFactor, rule, x3);
    status[p] = st;
    if (st == PLI_NEWPT_CREATED) { x3d[3 * (int64_t)p] = x3[0]; x3d[3 * (int64_t)p + 1] = x3[1]; x3d[3 * (int64_t)p + 2] = x3[2]; }
  }
}

// counts: nmatches[nkf] then nnew[nkf], zeroed by the caller
__global__ __launch_bounds__(256) void k_newpt_pick(int n1, int nkf, int* __restrict__ matches12, int* __restrict__ status,
                                                    int* __restrict__ nmatches, int* __restrict__ nnew) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  bool taken = false;
  for (int k = 0; k < nkf; ++k) {                         // (uniform over the wave: the ballots see every lane)
    bool matched = false, created = false;
    if (i < n1) {
      const int64_t p = (int64_t)k * n1 + i;
      matched = matches12[p] >= 0;
      if (matched && taken) { matches12[p] = -1; status[p] = PLI_NEWPT_TAKEN_EARLIER; matched = false; }
      else if (matched && status[p] == PLI_NEWPT_CREATED) { created = true; taken = true; }
    }
    const unsigned long long bm = __builtin_amdgcn_ballot_w64(matched), bc = __builtin_amdgcn_ballot_w64(created);
    if (lane == 0 && bm) atomicAdd(nmatches + k, __popcll(bm));
    if (lane == 0 && bc) atomicAdd(nnew + k, __popcll(bc));
  }
}

__global__ void k_fill_f32(float* __restrict__ dst, int n, float v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = v;
}

// ---------------------------------------------------------------------------
// The keypoint order ORBextractor::operator() leaves when a lapping area is given (ORBextractor.cc:1135-1144): keypoints
// with lap0 <= x <= lap1 (level-0 coordinates) fill the table from the back in visiting order, the others from the front.
// One workgroup per image: ordered counts by block scans over chunks of 1024 keypoints; src = snapshot of the table.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void lapping_order(const pli_keypoint* __restrict__ srcKp, const uint8_t* __restrict__ srcDesc,
                                              int n, float lap0, float lap1, pli_keypoint* __restrict__ dstKp,
                                              uint8_t* __restrict__ dstDesc, int* __restrict__ monoCount) {
  __shared__ int waveCnt[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + tid;
    pli_keypoint k;
    bool mono = false;
    if (i < n) { k = srcKp[i]; mono = !(k.x >= lap0 && k.x <= lap1); }
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(mono);
    if (lane == 0) waveCnt[wv] = __popcll(bal);
    __syncthreads();
    int before = base;
    for (int w = 0; w < wv; ++w) before += waveCnt[w];
    before += __popcll(bal & ((1ull << lane) - 1ull));       // mono keypoints before i
    if (i < n) {
      const int dst = mono ? before : n - 1 - (i - before);
      dstKp[dst] = k;
      const uint4* s4 = reinterpret_cast<const uint4*>(srcDesc + (int64_t)i * 32);
      uint4* d4 = reinterpret_cast<uint4*>(dstDesc + (int64_t)dst * 32);
      d4[0] = s4[0]; d4[1] = s4[1];
    }
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += waveCnt[w]; base += t; }
    __syncthreads();
  }
  if (tid == 0) *monoCount = base;
}

__global__ __launch_bounds__(1024) void k_lapping_order(const pli_keypoint* __restrict__ srcKp, const uint8_t* __restrict__ srcDesc,
                                                        int n, float lap0, float lap1, pli_keypoint* __restrict__ dstKp,
                                                        uint8_t* __restrict__ dstDesc, int* __restrict__ monoCount) {
  lapping_order(srcKp, srcDesc, n, lap0, lap1, dstKp, dstDesc, monoCount);
}

// ... with the keypoint count read on the device (pli_frame_extract_single: no host look between the extraction and the reorder):
// *count, at most cap, rows of the snapshot.
__global__ __launch_bounds__(1024) void k_lapping_order_counted(const pli_keypoint* __restrict__ srcKp, const uint8_t* __restrict__ srcDesc,
                                                                const int* __restrict__ count, int cap, float lap0, float lap1,
                                                                pli_keypoint* __restrict__ dstKp, uint8_t* __restrict__ dstDesc,
                                                                int* __restrict__ monoCount) {
  lapping_order(srcKp, srcDesc, min(*count, cap), lap0, lap1, dstKp, dstDesc, monoCount);
}

}  // namespace pli
