// The front of OpenCV 3.x's LineSegmentDetector on the CV_64FC1 copy of the image (PLI_PARITY_LSD_F64, the default: the
// reference pins OpenCV 3.3.1, whose lsd.cpp starts with `img.convertTo(image, CV_64FC1)`):
//   k_lsd_blur64    GaussianBlur(image, gaussian_img, ksize, sigma) on doubles — sepFilter2D with the filter engine's
//                   generic double filters: RowFilter (left to right), SymmColumnFilter (centre, then the +-k pairs)
//   k_lsd_resize64  resize(gaussian_img, scaled_image, Size(), SCALE, SCALE): INTER_LINEAR on doubles, float coefficients
//   k_lsd_grad64    ll_angle: 2x2 gradient in double, modgrad (double plane), level-line angle, max gradient
//   k_lsd_front64s  the three in one pass, a wave per strip of 64 scaled columns (the default where lsd_scale > 1)
//   k_lsd_front64   the three in one pass per 64 x 16 tile (where the streaming form does not apply)
// (OpenCV-3.3.1-compatible by intent: see DESIGN.md "Oracle" for what is known about each primitive.)
// The three forms write the same words because they call the same rules ("the shared rules" below): a form only decides where
// a rule's operands come from — global memory, LDS bytes or doubles, registers.
#include "kernels.hpp"
#include "device_prims.hpp"

namespace pli {

constexpr float F64_NOTDEF = -1024.f;
constexpr double F64_DEG2RAD = 3.14159265358979323846 / 180;

// ---------------------------------------------------------------------------
// the shared rules
// ---------------------------------------------------------------------------
// RowFilter: n taps t(0) .. t(n - 1), summed left to right
template <class Tap>
__device__ __forceinline__ double blur_row_sum(const double (&k)[7], int n, Tap t) {
  double s = k[0] * t(0);
  for (int j = 1; j < n; ++j) s += k[j] * t(j);
  return s;
}
// SymmColumnFilter of radius r: the centre t(0), then the pairs t(j) + t(-j)
template <class Tap>
__device__ __forceinline__ double blur_col_sum(const double (&k)[7], int r, Tap t) {
  double s = k[r] * t(0);
  for (int j = 1; j <= r; ++j) s += k[r + j] * (t(j) + t(-j));
  return s;
}

// tab: xofs[dw] | alpha[2*dw] (float bits) | yofs[dh] | beta[2*dh] (float bits).  A tap of the resize: the two source columns (rows)
// of a scaled one and their float weights, widened
struct ResizeTap {
  int s0, s1;
  double w0, w1;
  __device__ __forceinline__ double mix(double a, double b) const { return a * w0 + b * w1; }      // a = src[s0], b = src[s1]
};
__device__ __forceinline__ ResizeTap resize_tap(int s0, int s1, const int* __restrict__ tab, int w) {
  return {s0, s1, (double)__int_as_float(tab[w]), (double)__int_as_float(tab[w + 1])};
}
__device__ __forceinline__ ResizeTap resize_col_tap(const int* __restrict__ tab, int dw, int sw, int dx) {
  const int sx = tab[dx];                                  // (clamped by the host)
  return resize_tap(sx, min(sx + 1, sw - 1), tab, dw + 2 * dx);
}
__device__ __forceinline__ int resize_row_ofs(const int* __restrict__ tab, int dw, int dy) { return tab[3 * dw + dy]; }      // (not clamped by the host)
__device__ __forceinline__ ResizeTap resize_row_tap(const int* __restrict__ tab, int dw, int dh, int sh, int dy, int sy /* resize_row_ofs(dy) */) {
  return resize_tap(min(max(sy, 0), sh - 1), min(max(sy + 1, 0), sh - 1), tab, 3 * dw + dh + 2 * dy);
}
__device__ __forceinline__ ResizeTap resize_row_tap(const int* __restrict__ tab, int dw, int dh, int sh, int dy) {
  return resize_row_tap(tab, dw, dh, sh, dy, resize_row_ofs(tab, dw, dy));
}

// ll_angle of the pixel whose 2x2 neighbourhood of the scaled image is A B / C D; as constructed: a pixel without a level-line angle
// (the last row and column, the pad columns; norm <= rho keeps the norm).  m: bits of the largest norm above rho so far
// (non-negative doubles order like their bits)
struct LsdPixel { double norm = 0.0; float ang = F64_NOTDEF, cs = 0.f, sn = 0.f; };
__device__ __forceinline__ LsdPixel ll_angle_pixel(double A, double B, double C, double D, double rho, bool trigF32, unsigned long long& m) {
  LsdPixel px;
  const double DA = D - A;
  const double BC = B - C;
  const double gx = DA + BC, gy = DA - BC;
  px.norm = sqrt((gx * gx + gy * gy) / 4);
  if (!(px.norm <= rho)) {
    m = max(m, (unsigned long long)__double_as_longlong(px.norm));
    px.ang = fast_atan2_deg((float)gx, (float)(-gy));
    sincos_of_float((float)((double)px.ang * F64_DEG2RAD), trigF32, &px.sn, &px.cs);
  }
  return px;
}

// pixel o of the planes (common.hpp LsdFrontPlanes)
__device__ __forceinline__ void lsd_store_pixel(const LsdFrontPlanes& P, int64_t o, const LsdPixel& px) {
  if (P.rec) P.rec[o] = make_float4(px.ang, px.cs, px.sn, (P.packW && !P.hot) ? tx_unclaimed_norm_word(px.norm) : 0.f);
  if (P.hot) P.hot[o] = make_int2(__float_as_int(px.ang), P.packW ? __float_as_int(tx_unclaimed_norm_word(px.norm)) : 0);
  if (P.cold) P.cold[o] = make_float2(px.ang == F64_NOTDEF ? F64_NOTDEF : px.cs, px.sn);      // (cos = NOTDEF: no level-line angle)
  P.mg[o] = px.norm;
  if (P.own) P.own[o] = make_int2(0x7FFFFFFF, 0x7FFFFFFF);
}

// the largest norm of a 256-thread workgroup into the image's maximum
__device__ __forceinline__ void lsd_block_max(unsigned long long m, unsigned long long* __restrict__ imgMax) {
  __shared__ unsigned long long wmax[4];
  m = wave_max_u64(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m) atomicMax(imgMax, m);
  }
}

// ---------------------------------------------------------------------------
// the three kernels
// ---------------------------------------------------------------------------
// one 64 x 16 output tile per workgroup; u8 tile with halo and the row-filtered doubles staged in LDS
__global__ __launch_bounds__(256) void k_lsd_blur64(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int W, int H, int pitch,
                                                    const double* __restrict__ kern, int radius, double* __restrict__ out,
                                                    int64_t outImgStride, int img0) {
  __shared__ uint8_t tile[22][72];
  __shared__ double rows[22][64];
  const int img = blockIdx.z + img0, tid = threadIdx.x;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 16;
  const uint8_t* src = pyr + (int64_t)img * pyrBlock;
  const int r = radius, n = 2 * r + 1;
  const int tw = 64 + 2 * r, th = 16 + 2 * r;
  for (int i = tid; i < tw * th; i += 256) {
    const int ty = i / tw, tx = i - ty * tw;
    const int sx = reflect101(min(x0 + tx - r, W + r), W), sy = reflect101(min(y0 + ty - r, H + r), H);
    tile[ty][tx] = src[(int64_t)sy * pitch + sx];
  }
  __syncthreads();
  double k[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) k[i] = i < n ? kern[i] : 0.0;
  for (int i = tid; i < 64 * th; i += 256) {
    const int ty = i >> 6, tx = i & 63;
    rows[ty][tx] = blur_row_sum(k, n, [&](int j) { return (double)tile[ty][tx + j]; });
  }
  __syncthreads();
  for (int i = tid; i < 64 * 16; i += 256) {
    const int ty = i >> 6, tx = i & 63;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) continue;
    out[(int64_t)img * outImgStride + (int64_t)y * W + x] = blur_col_sum(k, r, [&](int j) { return rows[ty + r + j][tx]; });
  }
}

__global__ __launch_bounds__(256) void k_lsd_resize64(const double* __restrict__ src, int sw, int sh, double* __restrict__ dst,
                                                      int dw, int dh, int64_t dstImgStride, const int* __restrict__ tab, int img0) {
  const int img = blockIdx.z + img0, dy = blockIdx.y, dx = blockIdx.x * 256 + threadIdx.x;
  if (dx >= dw) return;
  const ResizeTap cx = resize_col_tap(tab, dw, sw, dx), ry = resize_row_tap(tab, dw, dh, sh, dy);
  const double* S0 = src + (int64_t)img * sw * sh + (int64_t)ry.s0 * sw;
  const double* S1 = src + (int64_t)img * sw * sh + (int64_t)ry.s1 * sw;
  dst[(int64_t)img * dstImgStride + (int64_t)dy * dw + dx] = ry.mix(cx.mix(S0[cx.s0], S0[cx.s1]), cx.mix(S1[cx.s0], S1[cx.s1]));
}

// (W: the true width, the scaled plane's row length; WP >= W: the row pitch of the planes written — the pad columns are undefined pixels)
__global__ __launch_bounds__(256) void k_lsd_grad64(const double* __restrict__ scaled, int W, int H, int WP, int64_t scaledImgStride, double rho,
                                                    LsdFrontPlanes P, unsigned long long* __restrict__ maxMg, float* __restrict__ angDbg,
                                                    int img0, int trigF32 /* PLI_PARITY_TRIG_F32_LSD */) {
  const int img = blockIdx.z + img0;
  const int x = blockIdx.x * 256 + threadIdx.x;
  unsigned long long m = 0ull;
  if (x < WP) {
    const int yEnd = min((int)(blockIdx.y + 1) * 16, H);
    const double* S = scaled + (int64_t)img * scaledImgStride;
    for (int y = blockIdx.y * 16; y < yEnd; ++y) {
      LsdPixel px;
      if (x < W - 1 && y < H - 1) {
        const double* r0 = S + (int64_t)y * W;
        const double* r1 = r0 + W;
        px = ll_angle_pixel(r0[x], r0[x + 1], r1[x], r1[x + 1], rho, trigF32 != 0, m);
      }
      lsd_store_pixel(P, (int64_t)img * WP * H + (int64_t)y * WP + x, px);
      if (angDbg && x < W) angDbg[(int64_t)img * W * H + (int64_t)y * W + x] = px.ang;      // (the debug plane: rows of the true width)
    }
  }
  lsd_block_max(m, &maxMg[img]);
}

// ---------------------------------------------------------------------------
// k_lsd_front64: the three kernels above in one pass per 64 x 16 tile of the SCALED image (lsd_scale != 1): the u8 source
// window of the tile (plus the blur radius) is staged in LDS, blurred there (rows, then columns), resized from LDS into a
// 65 x 17 tile of the scaled image, and the gradient / level-line angle of the 64 x 16 pixels is written.  Neither the blurred
// nor the scaled double plane goes to HBM: per scaled pixel the pass writes 24 B (record + norm) and reads ~0.8 B, where the
// three kernels moved 8·(2·P0/P' + 2) + 24 = 51 B.  The host uses it when the source window of every tile fits FS_W x FS_H
// (any scale >= 1; otherwise the separate kernels run) and debugging is off (PLI_DBG_LSD_SCALED wants the plane).
// ---------------------------------------------------------------------------
constexpr int FT_W = 64, FT_H = 16;        // scaled pixels per tile
constexpr int FS_W = 64, FS_H = 20;        // blurred source window (columns, rows) a tile may need
constexpr int FR = 3;                      // largest blur radius

// (R > 0: the blur radius at compile time — the taps unrolled with the kernel in registers; R = 0: any radius up to FR, the taps
// looped.  OpenCV's default sigma_scale 0.6 gives radius 3 for every scale >= 1.)
template <int R>
__device__ __forceinline__ void lsd_front64_tile(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int sw, int sh, int pitch,
                                                 const double* __restrict__ kern, int radius, const int* __restrict__ tab,
                                                 int dw, int dh, int dp, double rho, const LsdFrontPlanes& P,
                                                 unsigned long long* __restrict__ maxMg, int img0, int trigF32,
                                                 uint8_t (*tile)[FS_W + 2 * FR + 2], double (*rows)[FS_W], double (*blur)[FS_W]) {
  static_assert((FT_H + 1) * (FT_W + 1) <= (FS_H + 2 * FR) * FS_W, "the scaled tile reuses the row buffer");
  double (*scl)[FT_W + 1] = reinterpret_cast<double (*)[FT_W + 1]>(&rows[0][0]);
  const int img = blockIdx.z + img0, tid = threadIdx.x;
  const int x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_H;
  const uint8_t* src = pyr + (int64_t)img * pyrBlock;
  const int r = R > 0 ? R : radius, n = 2 * r + 1;
  // scaled pixels of this tile (with the +1 halo of the 2x2 gradient), and the source window they read
  const int x1 = min(x0 + FT_W, dw - 1), y1 = min(y0 + FT_H, dh - 1);          // last scaled column / row needed
  const int sx0 = tab[x0], sx1 = resize_col_tap(tab, dw, sw, x1).s1;
  const int sy0 = resize_row_tap(tab, dw, dh, sh, y0).s0, sy1 = resize_row_tap(tab, dw, dh, sh, y1).s1;
  const int cw = sx1 - sx0 + 1, ch = sy1 - sy0 + 1;                             // <= FS_W, FS_H (checked by the host)
  const int tw = cw + 2 * r, th = ch + 2 * r;
  // (thread = (column lx, row group ly): no division by the window width anywhere)
  const int lx = tid & 63, ly = tid >> 6;
  if (R > 0 && sw > 2 * R && sh > 2 * R) {
    // the window leaves the image by at most R < sw, sh pixels: ONE reflection, no loop — and a fixed trip count, so that the (up to
    // 14) byte loads of a thread are in flight together
    static_assert((FS_H + 2 * FR + 3) / 4 == 7 && FS_W + 2 * FR <= 128, "rows / columns a thread stages");
    const int c0 = reflect_once(sx0 + lx - R, sw), c1 = reflect_once(sx0 + lx + 64 - R, sw);
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int ty = ly + 4 * i;
      if (ty < th) {
        const uint8_t* row = src + (int64_t)reflect_once(sy0 + ty - R, sh) * pitch;
        if (lx < tw) tile[ty][lx] = row[c0];
        if (lx + 64 < tw) tile[ty][lx + 64] = row[c1];
      }
    }
  } else {
    for (int ty = ly; ty < th; ty += 4) {
      const int sy = reflect101(sy0 + ty - r, sh);
      for (int tx = lx; tx < tw; tx += 64) tile[ty][tx] = src[(int64_t)sy * pitch + reflect101(sx0 + tx - r, sw)];
    }
  }
  __syncthreads();
  double k[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) k[i] = i < n ? kern[i] : 0.0;
  if (lx < cw)
    for (int ty = ly; ty < th; ty += 4) rows[ty][lx] = blur_row_sum(k, n, [&](int j) { return (double)tile[ty][lx + j]; });
  __syncthreads();
  if (lx < cw)
    for (int ty = ly; ty < ch; ty += 4) blur[ty][lx] = blur_col_sum(k, r, [&](int j) { return rows[ty + r + j][lx]; });
  __syncthreads();
  const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;
  // thread = (column lx, rows ly, ly + 4, ..); the 65th column (the +1 halo of the 2x2 gradient) is spread over the first ny threads,
  // one row each, instead of a second pass of the whole workgroup for one lane's worth of pixels
  auto resizeCol = [&](int tx, int tyFirst, int tyStep) {
    const ResizeTap cx = resize_col_tap(tab, dw, sw, x0 + tx);
    const int c0 = cx.s0 - sx0, c1 = cx.s1 - sx0;         // (in the window)
    for (int ty = tyFirst; ty < ny; ty += tyStep) {
      const ResizeTap ry = resize_row_tap(tab, dw, dh, sh, y0 + ty);
      const double* B0 = blur[ry.s0 - sy0];
      const double* B1 = blur[ry.s1 - sy0];
      scl[ty][tx] = ry.mix(cx.mix(B0[c0], B0[c1]), cx.mix(B1[c0], B1[c1]));
    }
  };
  if (lx < nx) resizeCol(lx, ly, 4);
  if (nx > FT_W && tid < ny) resizeCol(FT_W, tid, FT_H + 1);
  __syncthreads();
  unsigned long long m = 0ull;
  for (int i = tid; i < FT_W * FT_H; i += 256) {
    const int ty = i >> 6, tx = i & 63;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= dp || y >= dh) continue;                      // (columns dw .. dp - 1: the pad of the planes' row pitch, undefined pixels)
    LsdPixel px;
    if (x < dw - 1 && y < dh - 1) px = ll_angle_pixel(scl[ty][tx], scl[ty][tx + 1], scl[ty + 1][tx], scl[ty + 1][tx + 1], rho, trigF32 != 0, m);
    lsd_store_pixel(P, (int64_t)img * dp * dh + (int64_t)y * dp + x, px);
  }
  lsd_block_max(m, &maxMg[img]);
}

__global__ __launch_bounds__(256) void k_lsd_front64(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int sw, int sh, int pitch,
                                                     const double* __restrict__ kern, int radius, const int* __restrict__ tab,
                                                     int dw, int dh, int dp /* row pitch of the planes written, >= dw */, double rho,
                                                     LsdFrontPlanes P, unsigned long long* __restrict__ maxMg, int img0,
                                                     int trigF32 /* as k_lsd_grad64 */) {
  __shared__ uint8_t tile[FS_H + 2 * FR][FS_W + 2 * FR + 2];
  __shared__ double rows[FS_H + 2 * FR][FS_W];               // row-filtered window; afterwards the scaled tile (scl)
  __shared__ double blur[FS_H][FS_W];
  if (radius == FR) lsd_front64_tile<FR>(pyr, pyrBlock, sw, sh, pitch, kern, radius, tab, dw, dh, dp, rho, P, maxMg, img0, trigF32, tile, rows, blur);
  else lsd_front64_tile<0>(pyr, pyrBlock, sw, sh, pitch, kern, radius, tab, dw, dh, dp, rho, P, maxMg, img0, trigF32, tile, rows, blur);
}

// ---------------------------------------------------------------------------
// k_lsd_front64s: the streaming form of k_lsd_front64.  ONE WAVE owns a strip of 64 columns of the scaled image and walks down
// `chunk` of its rows; there is no workgroup barrier and no tile.  Lane l owns source column sx0 + l of the strip's source window
// (cw <= 64 columns, checked by the host) and scaled column x0 + l.
//   per source row    one byte per lane (+ 6 halo bytes) staged in 72 bytes of LDS, the 7-tap row blur of the lane's column, and a
//                     7-deep window of row-blurred doubles in registers: the column blur of the row three back.  The vertical halo
//                     is paid once per chunk (6 rows warm the window up), not once per 16 scaled rows.
//   per blurred row   one 64-double row of LDS, from which every lane takes the horizontal half of the resize for its scaled column
//                     (row[s0] * w0 + row[s1] * w1, computed once per source row — a scaled row reads two of them), and for the
//                     strip's 65th column (the same value in every lane).
//   per scaled row    the vertical half with the row's tap from one uniform load, the right neighbour from the next lane (lane
//                     63: the 65th column), the row above from registers: gradient, norm, angle, {cos, sin}, the stores.
// Needs radius 3, sw > 6, sh > 6 (one reflection) and source rows that advance by 0 or 1 per scaled row (scale >= 1): the host
// checks (pli_capi.hip frontStreamFits).
// ---------------------------------------------------------------------------
constexpr int FW_WAVES = LSD_FRONT_STREAM_WAVES;      // strips (waves) per workgroup: neighbours in x, the same rows

__global__ __launch_bounds__(64 * FW_WAVES) void k_lsd_front64s(const uint8_t* __restrict__ pyr, int64_t pyrBlock, int sw, int sh, int pitch,
                                                                const double* __restrict__ kern, const int* __restrict__ tab,
                                                                int dw, int dh, int dp, double rho, LsdFrontPlanes P,
                                                                unsigned long long* __restrict__ maxMg, int img0, int trigF32,
                                                                int chunk /* scaled rows per wave */) {
  __shared__ uint32_t stage[FW_WAVES][18];                 // a source row's bytes: window columns -3 .. cw + 2
  __shared__ double blurRow[FW_WAVES][64];                 // the newest blurred row
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int x0 = (blockIdx.x * FW_WAVES + wv) * 64, y0 = blockIdx.y * chunk;
  if (x0 >= dw || y0 >= dh) return;                        // (no barrier anywhere: a wave without a strip just leaves)
  const int img = blockIdx.z + img0;
  const uint8_t* src = pyr + (int64_t)img * pyrBlock;
  // scaled rows y0 .. yl and columns x0 .. x1 (with the +1 halo of the 2x2 gradient), and the source window they read
  const int x1 = min(x0 + 64, dw - 1), yl = min(y0 + chunk, dh - 1);
  // the lane's scaled column (pad columns: the last one, never used) and the strip's 65th
  const ResizeTap cx = resize_col_tap(tab, dw, sw, min(x0 + lane, dw - 1)), ce = resize_col_tap(tab, dw, sw, x1);
  const int sx0 = tab[x0];
  const int cw = ce.s1 - sx0 + 1, tw = cw + 6;             // cw <= 64 (checked by the host)
  const int sxl = cx.s0 - sx0, sxn = cx.s1 - sx0, sxe = ce.s0 - sx0, sxen = ce.s1 - sx0;      // (in the window)
  const int bFirst = resize_row_tap(tab, dw, dh, sh, y0).s0, bLast = resize_row_tap(tab, dw, dh, sh, yl).s1;
  double k[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) k[i] = kern[i];
  // the window leaves the image by at most 3 < sw, sh pixels: one reflection
  const bool ld0 = lane < tw, ld1 = lane + 64 < tw;
  const int c0 = ld0 ? reflect_once(sx0 + lane - 3, sw) : 0, c1 = ld1 ? reflect_once(sx0 + lane + 64 - 3, sw) : 0;
  uint8_t* const stageB = reinterpret_cast<uint8_t*>(stage[wv]);
  const uint32_t* const stageW = stage[wv];
  double* const brow = blurRow[wv];
  const int vLast = bLast + 3;                             // source rows enter as "virtual" rows bFirst - 3 .. bLast + 3, reflected
  uint8_t n0, n1;                                          // the next row's bytes, loaded one row ahead
  {
    const uint8_t* row = src + (int64_t)reflect_once(bFirst - 3, sh) * pitch;
    n0 = row[c0]; n1 = row[c1];
  }
  double w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0;      // row-blurred rows v - 6 .. v
  double hp = 0, hpe = 0;                                  // the resize's horizontal half of the blurred row before: own column, 65th
  double p = 0, pR = 0;                                    // the scaled row before: own column, right neighbour
  int dy = y0, sy = resize_row_ofs(tab, dw, y0);           // the next scaled row and its source row offset, loaded a row ahead
  unsigned long long m = 0ull;
  const int x = x0 + lane;
  const int64_t obase = (int64_t)img * dp * dh + x;
  for (int v = bFirst - 3; v <= vLast; ++v) {
    stageB[lane] = n0;
    if (lane < 8) stageB[64 + lane] = n1;
    wave_lds_sync();
    if (v < vLast) {
      const uint8_t* row = src + (int64_t)reflect_once(v + 1, sh) * pitch;
      n0 = row[c0]; n1 = row[c1];
    }
    const uint32_t q0 = stageW[lane >> 2], q1 = stageW[(lane >> 2) + 1], q2 = stageW[(lane >> 2) + 2];
    wave_lds_sync();
    // bytes lane .. lane + 3 and lane + 4 .. lane + 6 of the row, out of the three words that hold them
    const uint32_t ta = (uint32_t)((((unsigned long long)q1 << 32) | q0) >> (8 * (lane & 3)));
    const uint32_t tb = (uint32_t)((((unsigned long long)q2 << 32) | q1) >> (8 * (lane & 3)));
    w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6;
    w6 = blur_row_sum(k, 7, [&](int j) { return (double)(uint8_t)(j < 4 ? ta >> (8 * j) : tb >> (8 * (j - 4))); });
    if (v < bFirst + 3) continue;                          // (the window is warming up)
    const int b = v - 3;                                   // the blurred row this source row completes
    const double win[7] = {w0, w1, w2, w3, w4, w5, w6};   // (an array kept across the rows compiled to 10 more instructions than the names)
    brow[lane] = blur_col_sum(k, 3, [&](int j) { return win[3 + j]; });
    wave_lds_sync();
    const double hc = cx.mix(brow[sxl], brow[sxn]);
    const double hce = ce.mix(brow[sxe], brow[sxen]);
    wave_lds_sync();
    // the scaled rows whose lower source row is b (their upper one is b - 1, or b at the image's border)
    while (dy <= yl) {
      const ResizeTap ry = resize_row_tap(tab, dw, dh, sh, dy, sy);
      if (ry.s1 != b) break;
      const bool same = ry.s0 == b;
      const double c = ry.mix(same ? hc : hp, hc);
      const double ce65 = ry.mix(same ? hce : hpe, hce);
      double cR = __shfl_down(c, 1, 64);
      if (lane == 63) cR = ce65;
      if (dy > y0 && x < dp) {                             // pixel (x, dy - 1): its 2x2 neighbourhood is p pR / c cR
        LsdPixel px;
        if (x < dw - 1) px = ll_angle_pixel(p, pR, c, cR, rho, trigF32 != 0, m);
        lsd_store_pixel(P, obase + (int64_t)(dy - 1) * dp, px);
      }
      p = c; pR = cR;
      if (++dy <= yl) sy = resize_row_ofs(tab, dw, dy);
    }
    hp = hc; hpe = hce;
  }
  if (y0 + chunk >= dh && x < dp) lsd_store_pixel(P, obase + (int64_t)(dh - 1) * dp, LsdPixel{});      // the image's last row: undefined pixels
  m = wave_max_u64(m);
  if (lane == 0 && m) atomicMax(&maxMg[img], m);
}

// (self-test, pli_selftest_front_stream) the number of 4-byte words in which two planes differ
__global__ __launch_bounds__(256) void k_count_diff_words(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int64_t n,
                                                          unsigned* __restrict__ count) {
  unsigned d = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d += a[i] != b[i];
  if (d) atomicAdd(count, d);
}

}  // namespace pli
