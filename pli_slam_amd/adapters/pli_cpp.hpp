// Header-only C++ host layer over the C ABI (include/pli_frontend.h).
// No OpenCV types here, so it builds anywhere the library does; the shims with
// the reference's exact signatures (cv::Mat / cv::KeyPoint / KeyLine) are in
// orbslam_adapters.hpp and forward to these classes.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/pli_frontend.h"

namespace pli {

struct Error : std::runtime_error {
  pli_status status;
  Error(pli_status s, const std::string& what) : std::runtime_error(what), status(s) {}
};

inline void check(pli_status s) {
  if (s != PLI_OK) throw Error(s, pli_last_error());
}

// ORBmatcher::DescriptorDistance (ORBmatcher.cc:2495-2511) / LineMatcher distance() (LineMatcher.cpp:231-247) for ONE pair of
// 32-byte descriptors, on the host: the reference's bit-twiddling popcount over 8 x 32 bits gives the same number.
inline int descriptorDistance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 4; ++i) {
    uint64_t x, y;
    std::memcpy(&x, a + 8 * i, 8);
    std::memcpy(&y, b + 8 * i, 8);
    d += __builtin_popcountll(x ^ y);
  }
  return d;
}

// An image and a depth map as their owner holds them, without an OpenCV type: what cv::Mat's data, cols, rows, step (bytes) say, the
// bytes per pixel of the image (1: gray; 3, 4: colour in the context's pli_set_image_format) and the element type of the depth map
// (the context's pli_set_depth_format).  adapters/tracking_grab.hpp makes them from the Mats of Tracking::GrabImage*.
struct ImageView { const uint8_t* data; int cols, rows; int64_t step; int channels; };
struct DepthView { const void* data; int cols, rows; int64_t step; pli_depth_type type; };

// One context = the four extractors of Tracking (ORB left/right, LSD left/right) plus the stereo matchers,
// sharing device-resident pyramids and tables (reference Tracking.cc:87-98,743-749 and Frame.cc:98-228).
// Thread safety: every pli_* call on a context holds the context's own lock inside the library
// (include/pli_frontend.h, "Conventions"), so the methods below may be called from several threads at once —
// the four std::threads of Frame.cc:128-135 — and run one after the other; this class adds no state of its own
// that would need a second lock.
class Frontend {
 public:
  explicit Frontend(const pli_frontend_config& cfg, int device = 0) : cfg_(cfg) {
    check(pli_ctx_create(&cfg_, device, &ctx_));
    check(pli_ctx_layout(ctx_, &layout_));
  }
  ~Frontend() { pli_ctx_destroy(ctx_); }
  Frontend(const Frontend&) = delete;
  Frontend& operator=(const Frontend&) = delete;

  const pli_frontend_config& config() const { return cfg_; }
  const pli_table_layout& layout() const { return layout_; }
  pli_ctx* handle() { return ctx_; }

  // ORBextractor::operator(): returns the reference's return value (count, -1 for an empty image)
  int extractORB(int eye, const uint8_t* img, int w, int h, int64_t stride, std::vector<pli_keypoint>& kps,
                 std::vector<uint8_t>& desc /* n x 32 */) {
    kps.resize(layout_.kp_cap);
    desc.resize((size_t)layout_.kp_cap * 32);
    int32_t n = 0;
    pli_status s = pli_orb_extract(ctx_, eye, img, w, h, stride, kps.data(), layout_.kp_cap, desc.data(), &n);
    if (s == PLI_ERR_EMPTY_IMAGE) { kps.clear(); desc.clear(); return -1; }
    check(s);
    kps.resize(n);
    desc.resize((size_t)n * 32);
    return n;
  }

  // Lineextractor::operator()
  void extractLines(int eye, const uint8_t* img, int w, int h, int64_t stride, std::vector<pli_keyline>& kls,
                    std::vector<uint8_t>& desc) {
    kls.resize(layout_.kl_cap);
    desc.resize((size_t)layout_.kl_cap * 32);
    int32_t n = 0;
    check(pli_line_extract(ctx_, eye, img, w, h, stride, kls.data(), layout_.kl_cap, desc.data(), &n));
    kls.resize(n);
    desc.resize((size_t)n * 32);
  }

  // the whole front-end of one Frame in one submission (pli_frame_extract): `record` = the frame's table record (layout())
  void frameExtract(const uint8_t* left, const uint8_t* right, int w, int h, int64_t strideLeft, int64_t strideRight, std::vector<uint8_t>& record) {
    record.resize((size_t)layout_.record_bytes);
    check(pli_frame_extract(ctx_, left, right, w, h, strideLeft, strideRight, record.data()));
  }
  // sizes of the device tables of the last per-call extractions: mvKeys, mvKeysRight, mvKeys_Line, mvKeysRight_Line (-1: not run)
  void lastCounts(int32_t counts[4]) { check(pli_last_counts(ctx_, counts)); }
  // the rig Frame::ComputeStereoMatches works with: mbf and fx = mK(0,0) (Frame.cc:1005-1008)
  void setStereoCamera(float bf, float fx) { check(pli_set_stereo_camera(ctx_, bf, fx)); }
  // Frame::ComputeStereoMatches
  void computeStereoMatches(std::vector<float>& uRight, std::vector<float>& depth) {
    uRight.assign(layout_.kp_cap, -1.f);
    depth.assign(layout_.kp_cap, -1.f);
    check(pli_stereo_match_points(ctx_, uRight.data(), depth.data(), layout_.kp_cap));
  }
  // Frame::ComputeStereoMatches_Lines
  void computeStereoMatchesLines(std::vector<float>& disp /* n x 2 */, std::vector<double>& le /* n x 3 */) {
    disp.assign((size_t)layout_.kl_cap * 2, -1.f);
    le.assign((size_t)layout_.kl_cap * 3, 0.0);
    check(pli_stereo_match_lines(ctx_, disp.data(), le.data(), layout_.kl_cap));
  }
  // match(desc1, desc2, nnr, matches_12), LineMatcher.cpp:201
  int matchLines(const uint8_t* d1, int n1, const uint8_t* d2, int n2, float nnr, std::vector<int>& m12) {
    m12.assign(n1, -1);
    int32_t n = 0;
    check(pli_match_lines(ctx_, d1, n1, d2, n2, nnr, m12.data(), &n));
    return n;
  }
  // ORBmatcher::DescriptorDistance for n pairs at once (one pair: pli::descriptorDistance on the host)
  void descriptorDistances(const uint8_t* a, const uint8_t* b, int n, std::vector<int>& dist) {
    dist.assign(n, 0);
    if (n) check(pli_descriptor_distance(ctx_, a, b, n, dist.data()));
  }
  // core of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, ...)
  int searchByProjection(const std::vector<pli_proj_query>& q, const uint8_t* qdesc, const std::vector<pli_keypoint>& cur,
                         const uint8_t* curDesc, const float* curURight, float minX, float maxX, float minY, float maxY,
                         bool checkOrientation, std::vector<int>& bestIdx2, const uint8_t* curOccupied = nullptr,
                         std::vector<int>* rawIdx2 = nullptr) {
    bestIdx2.assign(q.size(), -1);
    if (rawIdx2) rawIdx2->assign(q.size(), -1);
    int32_t n = 0;
    check(pli_search_by_projection(ctx_, q.data(), qdesc, (int)q.size(), cur.data(), curDesc, curURight, curOccupied, (int)cur.size(),
                                   minX, maxX, minY, maxY, checkOrientation ? 1 : 0, bestIdx2.data(),
                                   rawIdx2 ? rawIdx2->data() : nullptr, &n));
    return n;
  }
  // ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) ORBmatcher.cc:269-470 (F.Nleft == -1) of nkf keyframes against one frame
  // (include/pli_frontend.h pli_search_by_bow): matches (nkf x nf) = the keyframe feature each frame feature is matched to or -1,
  // nmatches[k] = the reference's return value for keyframe k
  void searchByBoW(int nkf, const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle, const int32_t* kfNode,
                   const uint8_t* kfValid, const uint8_t* fDesc, const float* fAngle, const int32_t* fNode, int nf, float nnratio,
                   bool checkOrientation, std::vector<int>& matches, std::vector<int>& nmatches) {
    matches.assign((size_t)nkf * nf, -1);
    nmatches.assign(nkf, 0);
    check(pli_search_by_bow(ctx_, nkf, kfOff, kfDesc, kfAngle, kfNode, kfValid, fDesc, fAngle, fNode, nf, nnratio,
                            checkOrientation ? 1 : 0, matches.data(), nmatches.data()));
  }
  // ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) ORBmatcher.cc:269-470, the branch F.Nleft != -1 (:342-369, :373-433), of nkf
  // keyframes against one frame of two cameras (include/pli_frontend.h pli_search_by_bow_two_cameras): the frame's first fNleft
  // rows are the left camera's; matches / nmatches as searchByBoW
  void searchByBoWTwoCameras(int nkf, const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle, const int32_t* kfNode,
                             const uint8_t* kfValid, const uint8_t* fDesc, const float* fAngle, const int32_t* fNode, int nf,
                             int fNleft, float nnratio, bool checkOrientation, std::vector<int>& matches, std::vector<int>& nmatches) {
    matches.assign((size_t)nkf * nf, -1);
    nmatches.assign(nkf, 0);
    check(pli_search_by_bow_two_cameras(ctx_, nkf, kfOff, kfDesc, kfAngle, kfNode, kfValid, fDesc, fAngle, fNode, nf, fNleft, nnratio,
                                        checkOrientation ? 1 : 0, matches.data(), nmatches.data()));
  }
  // ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) ORBmatcher.cc:823-963 (NLeft == -1) of one keyframe against nkf keyframes
  // (include/pli_frontend.h pli_search_by_bow_kf): matches12 (nkf x n1) = the row of keyframe k each feature of pKF1 is matched to
  // or -1, nmatches[k] = the reference's return value for keyframe k
  void searchByBoWKF(const uint8_t* desc1, const float* angle1, const int32_t* node1, const uint8_t* valid1, int n1, int nkf,
                     const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle, const int32_t* kfNode, const uint8_t* kfValid,
                     float nnratio, bool checkOrientation, std::vector<int>& matches12, std::vector<int>& nmatches) {
    matches12.assign((size_t)nkf * n1, -1);
    nmatches.assign(nkf, 0);
    check(pli_search_by_bow_kf(ctx_, desc1, angle1, node1, valid1, n1, nkf, kfOff, kfDesc, kfAngle, kfNode, kfValid, nnratio,
                               checkOrientation ? 1 : 0, matches12.data(), nmatches.data()));
  }
  // MapPoint::ComputeDistinctiveDescriptors MapPoint.cc:300-365 / MapLine::ComputeDistinctiveDescriptors MapLine.cc:246-317 of
  // off.size() - 1 features in one call (include/pli_frontend.h pli_distinctive_descriptors): feature p owns rows off[p] ..
  // off[p + 1] of desc (32 bytes a row, in the order of the reference's vDescriptors); best[p] = BestIdx within the group (-1 for an
  // empty group), bestMedian[p] = BestMedian; rowMedian (null: not wanted) = the median of every row
  void distinctiveDescriptors(const std::vector<uint8_t>& desc, const std::vector<int32_t>& off, std::vector<int>& best,
                              std::vector<int>& bestMedian, std::vector<int>* rowMedian = nullptr) {
    if (off.empty() || desc.size() != (size_t)off.back() * 32) throw std::logic_error("distinctiveDescriptors: off and desc disagree");
    const int nfeat = (int)off.size() - 1;
    best.assign(nfeat, -1);
    bestMedian.assign(nfeat, INT32_MAX);
    if (rowMedian) rowMedian->assign(off.back(), 0);
    check(pli_distinctive_descriptors(ctx_, desc.data(), off.data(), nfeat, best.data(), bestMedian.data(),
                                      rowMedian ? rowMedian->data() : nullptr));
  }
  // ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) ORBmatcher.cc:965-1206 (no second
  // cameras) of one keyframe against nkf neighbours (include/pli_frontend.h pli_search_for_triangulation): matches12 (nkf x n1) =
  // the neighbour's feature each feature of pKF1 is matched to or -1, nmatches[k] = the reference's return value for neighbour k
  void searchForTriangulation(const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1, const uint8_t* hasMp1,
                              const uint8_t* stereo1, int n1, int nkf, const int32_t* kfOff, const pli_keypoint* kfKp,
                              const uint8_t* kfDesc, const int32_t* kfNode, const uint8_t* kfHasMp, const uint8_t* kfStereo,
                              const float* F12, const float* ep, bool onlyStereo, bool coarse, bool checkOrientation,
                              std::vector<int>& matches12, std::vector<int>& nmatches) {
    matches12.assign((size_t)nkf * n1, -1);
    nmatches.assign(nkf, 0);
    check(pli_search_for_triangulation(ctx_, kp1, desc1, node1, hasMp1, stereo1, n1, nkf, kfOff, kfKp, kfDesc, kfNode, kfHasMp,
                                       kfStereo, F12, ep, onlyStereo ? 1 : 0, coarse ? 1 : 0, checkOrientation ? 1 : 0,
                                       matches12.data(), nmatches.data()));
  }
  // ORBmatcher::SearchForTriangulation ORBmatcher.cc:965-1206, the branch of keyframes with two KannalaBrandt8 cameras, of one
  // keyframe against nkf neighbours (include/pli_frontend.h pli_search_for_triangulation_two_cameras): the tables hold the left
  // camera's features first (n1Left / kfNleft = NLeft), rel = nkf x 4 x 12 floats (ll, lr, rl, rr: R12 row major, then t12);
  // matches12 (nkf x n1) = the neighbour's feature, over its N, each feature of pKF1 is matched to or -1
  void searchForTriangulationTwoCameras(const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1, const uint8_t* hasMp1,
                                        int n1, int n1Left, int nkf, const int32_t* kfOff, const int32_t* kfNleft,
                                        const pli_keypoint* kfKp, const uint8_t* kfDesc, const int32_t* kfNode, const uint8_t* kfHasMp,
                                        const pli_kb8_camera& camLeft, const pli_kb8_camera& camRight, const float* rel,
                                        bool onlyStereo, bool coarse, bool checkOrientation, std::vector<int>& matches12,
                                        std::vector<int>& nmatches) {
    matches12.assign((size_t)nkf * n1, -1);
    nmatches.assign(nkf, 0);
    check(pli_search_for_triangulation_two_cameras(ctx_, kp1, desc1, node1, hasMp1, n1, n1Left, nkf, kfOff, kfNleft, kfKp, kfDesc,
                                                   kfNode, kfHasMp, &camLeft, &camRight, rel, onlyStereo ? 1 : 0, coarse ? 1 : 0,
                                                   checkOrientation ? 1 : 0, matches12.data(), nmatches.data()));
  }
  // LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684, keyframes of one pinhole camera) of one keyframe
  // against nkf neighbours (include/pli_frontend.h pli_create_new_map_points): what the reference's sequential loop sees and creates
  // at neighbour k - matches12, status (PLI_NEWPT_*) and x3d (x 3) are nkf x n1, nmatches and nnew have nkf entries
  struct NewMapPoints {
    std::vector<int> matches12, nmatches, status, nnew;
    std::vector<float> x3d;
  };
  void createNewMapPoints(const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1, const uint8_t* hasMp1,
                          const float* uright1, const float* depth1, const float* key1, int n1, int nkf, const int32_t* kfOff,
                          const pli_keypoint* kfKp, const uint8_t* kfDesc, const int32_t* kfNode, const uint8_t* kfHasMp,
                          const float* kfUright, const float* kfDepth, const float* kfKey, const float* F12, const float* ep,
                          const float* pose1, const float* kfPose, const pli_fuse_camera& cam, float mb, bool coarse, bool farPoints,
                          float thFar, float ratioFactor, NewMapPoints& out) {
    out.matches12.assign((size_t)nkf * n1, -1);
    out.status.assign((size_t)nkf * n1, PLI_NEWPT_NOT_MATCHED);
    out.x3d.assign((size_t)nkf * n1 * 3, 0.f);
    out.nmatches.assign(nkf, 0);
    out.nnew.assign(nkf, 0);
    check(pli_create_new_map_points(ctx_, kp1, desc1, node1, hasMp1, uright1, depth1, key1, n1, nkf, kfOff, kfKp, kfDesc, kfNode,
                                    kfHasMp, kfUright, kfDepth, kfKey, F12, ep, pose1, kfPose, &cam, mb, coarse ? 1 : 0,
                                    farPoints ? 1 : 0, thFar, ratioFactor, out.matches12.data(), out.nmatches.data(),
                                    out.status.data(), out.x3d.data(), out.nnew.data()));
  }
  // The same step for keyframes of two KannalaBrandt8 cameras (LocalMapping.cc:463-528; include/pli_frontend.h
  // pli_create_new_map_points_two_cameras): the tables of searchForTriangulationTwoCameras, pose1 (2 x 15) and kfPose (nkf x 2 x 15)
  // = per keyframe the left then the right side's Rcw row major, tcw, Ow
  void createNewMapPointsTwoCameras(const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1, const uint8_t* hasMp1, int n1,
                                    int n1Left, int nkf, const int32_t* kfOff, const int32_t* kfNleft, const pli_keypoint* kfKp,
                                    const uint8_t* kfDesc, const int32_t* kfNode, const uint8_t* kfHasMp,
                                    const pli_kb8_camera& camLeft, const pli_kb8_camera& camRight, const float* rel,
                                    const float* pose1, const float* kfPose, bool coarse, bool farPoints, float thFar,
                                    float ratioFactor, NewMapPoints& out) {
    out.matches12.assign((size_t)nkf * n1, -1);
    out.status.assign((size_t)nkf * n1, PLI_NEWPT_NOT_MATCHED);
    out.x3d.assign((size_t)nkf * n1 * 3, 0.f);
    out.nmatches.assign(nkf, 0);
    out.nnew.assign(nkf, 0);
    check(pli_create_new_map_points_two_cameras(ctx_, kp1, desc1, node1, hasMp1, n1, n1Left, nkf, kfOff, kfNleft, kfKp, kfDesc, kfNode,
                                                kfHasMp, &camLeft, &camRight, rel, pose1, kfPose, coarse ? 1 : 0, farPoints ? 1 : 0,
                                                thFar, ratioFactor, out.matches12.data(), out.nmatches.data(), out.status.data(),
                                                out.x3d.data(), out.nnew.data()));
  }
  // The search half of ORBmatcher::Fuse (ORBmatcher.cc:1399-1609 without second cameras; reprojGate = false: the Sim3 overload
  // :1611-1733) of nmp map points against nkf keyframes (include/pli_frontend.h pli_fuse_search): bestIdx (nkf x nmp) = the
  // keyframe's row or -1.  levelRatio: fuseLevelRatio() of the extractor's configuration.
  void fuseSearch(const pli_fuse_point* mp, const uint8_t* mpDesc, int nmp, int nkf, const int32_t* kfOff, const pli_keypoint* kfKp,
                  const uint8_t* kfDesc, const float* kfUright, const float* kfPose, const uint8_t* skip, const pli_fuse_camera& cam,
                  float th, const std::vector<float>& levelRatio, bool reprojGate, std::vector<int>& bestIdx) {
    bestIdx.assign((size_t)nkf * nmp, -1);
    check(pli_fuse_search(ctx_, mp, mpDesc, nmp, nkf, kfOff, kfKp, kfDesc, kfUright, kfPose, skip, &cam, th, levelRatio.data(),
                          reprojGate ? 1 : 0, bestIdx.data(), nullptr));
  }
  // The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) ORBmatcher.cc:1399-1609 for keyframes with two KannalaBrandt8
  // cameras (NLeft != -1), both values of bRight of nkf keyframes in one call (include/pli_frontend.h pli_fuse_search_two_cameras):
  // the tables hold the left camera's rows first (kfNleft = NLeft), kfPose = nkf x 2 x 15 (left, right), skip = nkf x 2 x nmp or
  // null, bounds = mnMinX, mnMaxX, mnMinY, mnMaxY, sides: bit 0 = left, bit 1 = right; bestIdx (nkf x 2 x nmp) = the row over the
  // keyframe's N or -1
  void fuseSearchTwoCameras(const pli_fuse_point* mp, const uint8_t* mpDesc, int nmp, int nkf, const int32_t* kfOff,
                            const int32_t* kfNleft, const pli_keypoint* kfKp, const uint8_t* kfDesc, const float* kfPose,
                            const uint8_t* skip, const pli_kb8_camera& camLeft, const pli_kb8_camera& camRight, const float bounds[4],
                            float th, const std::vector<float>& levelRatio, int sides, std::vector<int>& bestIdx) {
    bestIdx.assign((size_t)nkf * 2 * nmp, -1);
    check(pli_fuse_search_two_cameras(ctx_, mp, mpDesc, nmp, nkf, kfOff, kfNleft, kfKp, kfDesc, kfPose, skip, &camLeft, &camRight,
                                      bounds[0], bounds[1], bounds[2], bounds[3], th, levelRatio.data(), sides, bestIdx.data(),
                                      nullptr));
  }
  // Loop closing's ORBmatcher::SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
  // ORBmatcher.cc:473-704 of nmp map points against npair (keyframe, Scw) pairs (include/pli_frontend.h
  // pli_search_by_projection_sim3): rowPoint (one per keyframe row) = the point that took the row in this call or -1,
  // nmatches[k] = the reference's return value for pair k.  projectForm: 0 = Pinhole::project (:519), 1 = :631-636.
  void searchByProjectionSim3(const pli_fuse_point* mp, const uint8_t* mpDesc, int nmp, int npair, const int32_t* kfOff,
                              const pli_keypoint* kfKp, const uint8_t* kfDesc, const float* kfPose, const uint8_t* skip,
                              const uint8_t* occupied, const pli_fuse_camera& cam, float th, const std::vector<float>& levelRatio,
                              float ratioHamming, int projectForm, std::vector<int>& rowPoint, std::vector<int>& nmatches) {
    rowPoint.assign(npair > 0 ? (size_t)kfOff[npair] : 0, -1);
    nmatches.assign(npair, 0);
    check(pli_search_by_projection_sim3(ctx_, mp, mpDesc, nmp, npair, kfOff, kfKp, kfDesc, kfPose, skip, occupied, &cam, th,
                                        levelRatio.data(), ratioHamming, projectForm, rowPoint.data(), nullptr, nmatches.data()));
  }
  // Relocalisation's ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) ORBmatcher.cc:2325-2447 of one
  // frame table (nf rows) against ncand candidates, candidate c owning rows mpOff[c] .. mpOff[c + 1] of mp / mpDesc / mpAngle
  // (include/pli_frontend.h pli_search_by_projection_reloc): rowPoint (ncand x nf) = the index within the candidate's list of the
  // point that holds the row after the rotation filter or -1, nmatches[c] = the reference's return value for candidate c.
  void searchByProjectionReloc(int ncand, const int32_t* mpOff, const pli_fuse_point* mp, const uint8_t* mpDesc, const float* mpAngle,
                               const float* pose, const pli_keypoint* fKp, const uint8_t* fDesc, int nf, const uint8_t* occupied,
                               const pli_fuse_camera& cam, float th, const std::vector<float>& levelRatio, int orbDist,
                               bool checkOrientation, std::vector<int>& rowPoint, std::vector<int>& nmatches) {
    rowPoint.assign((size_t)ncand * nf, -1);
    nmatches.assign(ncand, 0);
    check(pli_search_by_projection_reloc(ctx_, ncand, mpOff, mp, mpDesc, mpAngle, pose, fKp, fDesc, nf, occupied, &cam, th,
                                         levelRatio.data(), orbDist, checkOrientation ? 1 : 0, rowPoint.data(), nullptr,
                                         nmatches.data()));
  }
  // Monocular initialisation's ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
  // ORBmatcher.cc:706-821 (include/pli_frontend.h pli_search_for_initialization): matches12 = vnMatches12 after the rotation
  // filter; prevMatched (n1 x 2: x, y) is read, the update :816-818 is the caller's.  Returns the reference's return value.
  int searchForInitialization(const std::vector<pli_keypoint>& kp1, const uint8_t* desc1, const float* prevMatched,
                              const std::vector<pli_keypoint>& kp2, const uint8_t* desc2, float minX, float maxX, float minY,
                              float maxY, int windowSize, float nnratio, bool checkOrientation, std::vector<int>& matches12,
                              std::vector<int>* raw12 = nullptr) {
    matches12.assign(kp1.size(), -1);
    if (raw12) raw12->assign(kp1.size(), -1);
    int32_t n = 0;
    check(pli_search_for_initialization(ctx_, kp1.data(), desc1, (int)kp1.size(), prevMatched, kp2.data(), desc2, (int)kp2.size(), minX,
                                        maxX, minY, maxY, windowSize, nnratio, checkOrientation ? 1 : 0, matches12.data(),
                                        raw12 ? raw12->data() : nullptr, &n));
    return n;
  }
  // level_ratio of pli_fuse_search from the HOST's own MapPoint::PredictScale expression: levelOf(ratio) must be the tree's
  // expression compiled by the tree's compiler (ceil(log(ratio) / mfLogScaleFactor) with its clamps), so that whichever overload
  // of log its toolchain selects is the one the thresholds describe.  For n = 0 .. nlevels-2 the largest float for which
  // levelOf gives a level <= n, by bisection over the bit patterns of the positive floats.
  template <class LevelOf>
  static std::vector<float> fuseLevelRatio(int nlevels, LevelOf levelOf) {
    std::vector<float> out(nlevels > 1 ? nlevels - 1 : 0);
    for (int n = 0; n + 1 < nlevels; ++n) {
      uint32_t lo = 1u, hi = 0x7F800000u;                 // the smallest subnormal: level 0; +inf: the top level
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        float r;
        std::memcpy(&r, &mid, 4);
        if (levelOf(r) <= n) lo = mid; else hi = mid;
      }
      std::memcpy(&out[n], &lo, 4);
    }
    return out;
  }
  // Frame::ComputeStereoFromRGBD(imDepth) Frame.cc:1309 (depth: CV_32F, row stride in floats)
  void computeStereoFromRGBD(const float* depth, int64_t strideFloats, std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
    mvuRight.assign(layout_.kp_cap, -1.f); mvDepth.assign(layout_.kp_cap, -1.f);
    check(pli_stereo_from_depth(ctx_, depth, strideFloats, mvuRight.data(), mvDepth.data(), layout_.kp_cap));
  }
  // cv::remap(im, imRect, M1, M2, INTER_LINEAR) of the stereo driver (stereo_euroc.cc:166), fused into the ingest
  void setRectifyMaps(int eye, const float* mapx, const float* mapy) { check(pli_set_rectify_maps(ctx_, eye, mapx, mapy)); }
  // the cvtColor and the depth convertTo at the head of Tracking::GrabImage* (Tracking.cc:889-914, :979-980), fused into the ingest
  // and into ComputeStereoFromRGBD (adapters/tracking_grab.hpp picks the arguments as the reference does)
  void setImageFormat(pli_image_format fmt) { check(pli_set_image_format(ctx_, fmt)); }
  void setDepthFormat(pli_depth_type type, float scale) { check(pli_set_depth_format(ctx_, type, scale)); }
  // core of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...) ORBmatcher.cc:44
  int searchLocalMap(const std::vector<pli_proj_query>& q, const uint8_t* qdesc, const std::vector<pli_keypoint>& cur,
                     const uint8_t* curDesc, const float* curURight, const uint8_t* curOccupied, float minX, float maxX,
                     float minY, float maxY, float nnratio, std::vector<int>& bestIdx2) {
    bestIdx2.assign(q.size(), -1);
    int32_t n = 0;
    check(pli_search_local_map(ctx_, q.data(), qdesc, (int)q.size(), cur.data(), curDesc, curURight, curOccupied,
                               (int)cur.size(), minX, maxX, minY, maxY, nnratio, bestIdx2.data(), &n));
    return n;
  }
  // the same for a frame of two fisheye cameras (F.Nleft != -1), ORBmatcher.cc:44-214: both halves of F.mvpMapPoints
  // (mpLeft[k] / mpRight[k] = index into vpMapPoints of the point the call left in slot k / k + Nleft, or -1)
  int searchLocalMapFishEye(const std::vector<pli_proj_query>& qLeft, const std::vector<pli_proj_query>& qRight, const uint8_t* qdesc,
                            const std::vector<pli_keypoint>& kpLeft, const uint8_t* descLeft, const uint8_t* occLeft,
                            const std::vector<int>& leftToRight, const std::vector<pli_keypoint>& kpRight,
                            const uint8_t* descRight, const uint8_t* occRight, const std::vector<int>& rightToLeft, float minX,
                            float maxX, float minY, float maxY, float nnratio, std::vector<int>& mpLeft, std::vector<int>& mpRight) {
    mpLeft.assign(kpLeft.size(), -1); mpRight.assign(kpRight.size(), -1);
    int32_t n = 0;
    check(pli_search_local_map_fisheye(ctx_, qLeft.data(), qRight.data(), qdesc, (int)qLeft.size(), kpLeft.data(), descLeft, occLeft,
                                       leftToRight.data(), (int)kpLeft.size(), kpRight.data(), descRight, occRight,
                                       rightToLeft.data(), (int)kpRight.size(), minX, maxX, minY, maxY, nnratio, mpLeft.data(),
                                       mpRight.data(), &n));
    return n;
  }
  // core of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for a current frame of two cameras
  // (CurrentFrame.Nleft != -1), ORBmatcher.cc:1961-2177 (include/pli_frontend.h pli_search_by_projection_two_cameras): bestLeft[i] /
  // bestRight[i] = the keypoint of that camera row i holds after the rotation filter or -1, rawLeft / rawRight the same before it
  int searchByProjectionTwoCameras(const std::vector<pli_proj_query>& qLeft, const std::vector<pli_proj_query>& qRight,
                                   const uint8_t* qdesc, const std::vector<pli_keypoint>& kpLeft, const uint8_t* descLeft,
                                   const uint8_t* occLeft, const std::vector<pli_keypoint>& kpRight, const uint8_t* descRight,
                                   const uint8_t* occRight, float minX, float maxX, float minY, float maxY, bool checkOrientation,
                                   std::vector<int>& bestLeft, std::vector<int>& bestRight, std::vector<int>* rawLeft = nullptr,
                                   std::vector<int>* rawRight = nullptr) {
    if (qLeft.size() != qRight.size()) throw std::logic_error("searchByProjectionTwoCameras: one right query per left query");
    bestLeft.assign(qLeft.size(), -1); bestRight.assign(qLeft.size(), -1);
    if (rawLeft) rawLeft->assign(qLeft.size(), -1);
    if (rawRight) rawRight->assign(qLeft.size(), -1);
    int32_t n = 0;
    check(pli_search_by_projection_two_cameras(ctx_, qLeft.data(), qRight.data(), qdesc, (int)qLeft.size(), kpLeft.data(), descLeft,
                                               occLeft, (int)kpLeft.size(), kpRight.data(), descRight, occRight, (int)kpRight.size(),
                                               minX, maxX, minY, maxY, checkOrientation ? 1 : 0, bestLeft.data(), bestRight.data(),
                                               rawLeft ? rawLeft->data() : nullptr, rawRight ? rawRight->data() : nullptr, &n));
    return n;
  }
  // int match(const vector<MapLine*>&, Frame&, nnr, matches_12) LineMatcher.cpp:161 on the descriptor tables
  int matchNNR(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr, std::vector<int>& matches12) {
    matches12.assign(n1, -1);
    int32_t n = 0;
    check(pli_match_nnr(ctx_, desc1, n1, desc2, n2, nnr, matches12.data(), &n));
    return n;
  }
  // Tracking.cc:3809-3855 for a frame of one camera (include/pli_frontend.h pli_search_local_points): Frame::isInFrustum of every
  // local map point, the queries of ORBmatcher.cc:53-73 and the search, projection and queries on the device.  view[i]: what the
  // call leaves in point i; bestIdx2[i]: the keypoint it took or -1; nInView = nToMatch.  Returns the reference's nmatches.
  int searchLocalPoints(const std::vector<pli_fuse_point>& mp, const uint8_t* mpDesc, const float pose[15], const pli_fuse_camera& cam,
                        float viewingCosLimit, float th, bool farPoints, float thFar, float nnratio,
                        const std::vector<float>& levelRatio, const std::vector<pli_keypoint>& cur, const uint8_t* curDesc,
                        const float* curURight, const uint8_t* curOccupied, std::vector<pli_local_view>& view,
                        std::vector<int>& bestIdx2, int& nInView) {
    view.assign(mp.size(), pli_local_view{});
    bestIdx2.assign(mp.size(), -1);
    int32_t n = 0, nv = 0;
    check(pli_search_local_points(ctx_, mp.data(), mpDesc, (int)mp.size(), pose, &cam, viewingCosLimit, th, farPoints ? 1 : 0, thFar,
                                  nnratio, levelRatio.data(), cur.data(), curDesc, curURight, curOccupied, (int)cur.size(),
                                  view.data(), bestIdx2.data(), &nv, &n));
    nInView = nv;
    return n;
  }
  // Tracking.cc:3862-3883 (include/pli_frontend.h pli_search_local_lines): Frame::isInFrustum_l of every local map line, the list
  // mvpLocalMapLines_InFrustum (inFrustum[k] = list index of its k-th line) and match(..., nnr, matches12) on it.  sp: nl x 3.
  int searchLocalLines(const std::vector<float>& sp, const std::vector<uint8_t>& valid, const uint8_t* desc, const float pose[15],
                       const pli_fuse_camera& cam, const uint8_t* curDesc, int n2, float nnr, std::vector<int>& inView,
                       std::vector<float>& projS, std::vector<int>& inFrustum, std::vector<int>& matches12) {
    const size_t nl = valid.size();
    if (sp.size() != 3 * nl) throw std::logic_error("searchLocalLines: three coordinates per line");
    inView.assign(nl, 0); projS.assign(2 * nl, 0.0f); inFrustum.assign(nl, -1); matches12.assign(nl, -1);
    int32_t n = 0, nv = 0;
    check(pli_search_local_lines(ctx_, sp.data(), valid.data(), desc, (int)nl, pose, &cam, curDesc, n2, nnr, inView.data(),
                                 projS.data(), inFrustum.data(), matches12.data(), &nv, &n));
    inFrustum.resize(nv); matches12.resize(nv);
    return n;
  }
  // Frame::ComputeStereoFishEyeMatches Frame.cc:1577-1618 on the Frame's own tables (mvKeys / mDescriptors / monoLeft, ...);
  // fills mvLeftToRightMatch, mvRightToLeftMatch, mvDepth, mvStereo3Dpoints (x, y, z per left keypoint) and returns nMatches
  int stereoFishEye(const std::vector<pli_keypoint>& kpLeft, const uint8_t* descLeft, int monoLeft,
                    const std::vector<pli_keypoint>& kpRight, const uint8_t* descRight, int monoRight, const pli_kb8_camera& cam1,
                    const pli_kb8_camera& cam2, const float* Rlr, const float* tlr, std::vector<int>& leftToRight,
                    std::vector<int>& rightToLeft, std::vector<float>& depth, std::vector<float>& points3d) {
    leftToRight.assign(kpLeft.size(), -1);
    rightToLeft.assign(kpRight.size(), -1);
    depth.assign(kpLeft.size(), -1.0f);
    points3d.assign(kpLeft.size() * 3, 0.0f);
    int32_t n = 0;
    check(pli_stereo_fisheye_tables(ctx_, kpLeft.data(), descLeft, (int)kpLeft.size(), monoLeft, kpRight.data(), descRight,
                                    (int)kpRight.size(), monoRight, &cam1, &cam2, Rlr, tlr, leftToRight.data(), rightToLeft.data(),
                                    depth.data(), points3d.data(), &n));
    return n;
  }

 private:
  pli_frontend_config cfg_;
  pli_table_layout layout_{};
  pli_ctx* ctx_ = nullptr;
};

// DBoW2::TemplatedVocabulary<cv::Mat, FORB> as Frame::ComputeBoW uses it (Frame.cc:858-870): the descents run on the
// device (pli_bow_transform); BowVector::addWeight / FeatureVector::addFeature in feature order and the L1
// normalisation in word order are the reference's own host arithmetic (TemplatedVocabulary.h:1139-1208,
// BowVector.cpp:33-81), so the two maps are identical to DBoW2's.
using BowVector = std::map<unsigned, double>;
using FeatureVector = std::map<unsigned, std::vector<unsigned>>;

class Vocabulary {
 public:
  // node list as loadFromTextFile reads it from ORBvoc.txt: node i+1 has parent[i], isLeaf[i], desc[32*i..], weight[i]
  Vocabulary(Frontend& fe, int k, int L, int nnodes, const int32_t* parent, const uint8_t* isLeaf, const uint8_t* desc,
             const double* weight) : fe_(fe) {
    check(pli_vocab_create(fe.handle(), k, L, nnodes, parent, isLeaf, desc, weight, &v_));
  }
  ~Vocabulary() { pli_vocab_destroy(v_); }
  Vocabulary(const Vocabulary&) = delete;
  Vocabulary& operator=(const Vocabulary&) = delete;

  // transform(features, v, fv, levelsup) for TF-IDF weighting and L1 scoring (the ORB / LBD vocabularies)
  void transform(const uint8_t* desc, int n, BowVector& v, FeatureVector& fv, int levelsup) const {
    v.clear();
    fv.clear();
    std::vector<int32_t> word(n), node(n);
    std::vector<double> w(n);
    check(pli_bow_transform(fe_.handle(), v_, desc, n, levelsup, word.data(), w.data(), node.data()));
    for (int i = 0; i < n; ++i)
      if (w[i] > 0) {                       // not a stopped word
        v[(unsigned)word[i]] += w[i];
        fv[(unsigned)node[i]].push_back((unsigned)i);
      }
    double norm = 0.0;
    for (auto& kv : v) norm += std::fabs(kv.second);
    if (norm > 0.0)
      for (auto& kv : v) kv.second /= norm;
  }

 private:
  Frontend& fe_;
  pli_vocab* v_ = nullptr;
};

}  // namespace pli
