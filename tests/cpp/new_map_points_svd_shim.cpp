// Test infrastructure: the oracle's statement of cv::SVD::compute on a 4x4 CV_32F matrix (oracle/match_oracle.hpp
// jacobiSvdLastVt4), reachable from Python through ctypes, so that tests/helpers_new_map_points.py does not state the Jacobi a
// second time.  A: 16 floats, row major; out: the last row of vt.
#include "oracle/match_oracle.hpp"

extern "C" void pli_test_svd_last_vt4(const float* A, float* out) {
  float At[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) At[c][r] = A[4 * r + c];
  orc::jacobiSvdLastVt4(At, out);
}
