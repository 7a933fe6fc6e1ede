// The host passes at the head of Tracking::GrabImageRGBD (Tracking.cc:964-980) as plain C++ loops, for tools/colour_ingest_timing.py:
// what a caller of the gray / CV_32F entry points runs per frame before the call.  Built with g++ -O2 by that script; not part of
// the library.
//   pli_host_rgb_to_gray   cvtColor(im, im, CV_RGB2GRAY), OpenCV 3.3.1's C++ path: (R*4899 + G*9617 + B*1868 + 8192) >> 14
//   pli_host_depth_to_f32  imDepth.convertTo(imDepth, CV_32F, scale) of a CV_16U map: (float)raw * scale
#include <cstdint>

extern "C" {

void pli_host_rgb_to_gray(const uint8_t* src, int64_t stride, int w, int h, int channels, uint8_t* dst) {
  for (int y = 0; y < h; ++y) {
    const uint8_t* s = src + (int64_t)y * stride;
    uint8_t* d = dst + (int64_t)y * w;
    for (int x = 0; x < w; ++x, s += channels) d[x] = (uint8_t)((s[0] * 4899 + s[1] * 9617 + s[2] * 1868 + 8192) >> 14);
  }
}

void pli_host_depth_to_f32(const uint16_t* src, int w, int h, float scale, float* dst) {
  const int64_t n = (int64_t)w * h;
  for (int64_t i = 0; i < n; ++i) dst[i] = (float)src[i] * scale;
}

}
