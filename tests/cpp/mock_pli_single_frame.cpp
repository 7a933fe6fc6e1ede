// TEST-ONLY: tests/cpp/mock_pli.cpp (the stand-in for libpli_frontend.so on machines without a GPU, included here as it is, so
// this file is linked INSTEAD of it) plus pli_set_pinhole_distortion and pli_frame_extract_single with made-up deterministic
// results, for the host test of adapters/frame_single.hpp (tests/test_cpp_single_frame.py).  What it makes up: a constant image has
// no keypoints; the "undistorted" position of (x, y) is (1.01 x + 0.5, 0.99 y - 0.25) with a camera whose k1 != 0 and (x, y) without;
// the bounds are {-3, W + 5, -2, H + 4}; a keypoint's cell is a hash of its row, -1 for every seventh.  The lapping reorder and the
// depth association follow the real entry point, so that monoLeft, mvuRight and mvDepth mean something.  Nothing here is product code.
#include "mock_pli.cpp"

static pli_pinhole_distortion g_cam;
static bool g_camOn = false;

static void mockUndistort(float x, float y, float* ox, float* oy) {
  if (g_camOn) { *ox = 1.01f * x + 0.5f; *oy = 0.99f * y - 0.25f; } else { *ox = x; *oy = y; }
}

extern "C" {
pli_status pli_set_pinhole_distortion(pli_ctx* c, const pli_pinhole_distortion* cam, float bounds[4]) {
  if (!c) return PLI_ERR_INVALID;
  Lock l(c);
  g_camOn = cam && cam->k1 != 0.0f;
  if (cam) g_cam = *cam;
  if (bounds) {
    bounds[0] = g_camOn ? -3.f : 0.f; bounds[1] = (float)c->cfg.width + (g_camOn ? 5.f : 0.f);
    bounds[2] = g_camOn ? -2.f : 0.f; bounds[3] = (float)c->cfg.height + (g_camOn ? 4.f : 0.f);
  }
  return PLI_OK;
}

pli_status pli_frame_extract_single(pli_ctx* c, const uint8_t* img, int32_t w, int32_t h, int64_t stride, int32_t lap0, int32_t lap1,
                                    const float* depth, int64_t depthStride, void* record, float* kpUn, float* klUn, int32_t* cell,
                                    int32_t* nMono) {
  if (!c || !record || !kpUn || !klUn || !cell || !nMono) return PLI_ERR_INVALID;
  Lock l(c);
  if (!img || w <= 0 || h <= 0) return PLI_ERR_EMPTY_IMAGE;
  const pli_table_layout& Y = c->lay;
  uint8_t* rec = (uint8_t*)record;
  std::memset(rec, 0, (size_t)Y.record_bytes);
  int32_t* counts = (int32_t*)(rec + Y.off_counts);
  pli_keypoint* kp = (pli_keypoint*)(rec + Y.off_kp[0]);
  uint8_t* desc = rec + Y.off_desc[0];
  bool constant = true;
  for (int y = 0; y < h && constant; ++y) for (int x = 0; x < w; ++x) if (img[y * stride + x] != img[0]) { constant = false; break; }
  if (constant) {
    counts[0] = 0; c->nkp[0] = 0;
  } else {
    std::vector<pli_keypoint> k0(Y.kp_cap);
    std::vector<uint8_t> d0((size_t)Y.kp_cap * 32);
    pli_status s = pli_orb_extract(c, 0, img, w, h, stride, k0.data(), Y.kp_cap, d0.data(), &counts[0]);
    if (s != PLI_OK) return s;
    // ORBextractor.cc:1135-1144: lap0 <= x <= lap1 fills from the back in visiting order, the others from the front
    const int N = counts[0];
    int mono = 0, back = N - 1;
    for (int i = 0; i < N; ++i) {
      const bool lapping = k0[i].x >= (float)lap0 && k0[i].x <= (float)lap1;
      const int dst = lapping ? back-- : mono++;
      kp[dst] = k0[i];
      std::memcpy(desc + (size_t)dst * 32, d0.data() + (size_t)i * 32, 32);
    }
    *nMono = mono;
  }
  if (constant) *nMono = 0;
  pli_status s = pli_line_extract(c, 0, img, w, h, stride, (pli_keyline*)(rec + Y.off_kl[0]), Y.kl_cap, rec + Y.off_ldesc[0], &counts[2]);
  if (s != PLI_OK) return s;
  const int N = counts[0], M = counts[2];
  float* ur = (float*)(rec + Y.off_uright);
  float* dp = (float*)(rec + Y.off_depth);
  for (int i = 0; i < Y.kp_cap; ++i) {
    kpUn[2 * i] = kpUn[2 * i + 1] = 0.f; cell[i] = -1; ur[i] = dp[i] = -1.f;
    if (i >= N) continue;
    mockUndistort(kp[i].x, kp[i].y, &kpUn[2 * i], &kpUn[2 * i + 1]);
    cell[i] = i % 7 == 3 ? -1 : (int)(mix(c->seed[0], (uint32_t)i) % 40u) * 48 + (int)(mix(c->seed[0], (uint32_t)i + 7777u) % 30u);
    if (depth) {
      const int u = (int)kp[i].x, v = (int)kp[i].y;
      if (u >= 0 && v >= 0 && u < w && v < h) {
        const float d = depth[(int64_t)v * depthStride + u];
        if (d > 0) { dp[i] = d; ur[i] = kpUn[2 * i] - c->cfg.bf / d; }
      }
    }
  }
  const pli_keyline* kl = (const pli_keyline*)(rec + Y.off_kl[0]);
  for (int j = 0; j < Y.kl_cap; ++j) {
    for (int k = 0; k < 4; ++k) klUn[4 * j + k] = 0.f;
    if (j >= M) continue;
    mockUndistort(kl[j].startPointX, kl[j].startPointY, &klUn[4 * j], &klUn[4 * j + 1]);
    mockUndistort(kl[j].endPointX, kl[j].endPointY, &klUn[4 * j + 2], &klUn[4 * j + 3]);
  }
  return PLI_OK;
}
}
