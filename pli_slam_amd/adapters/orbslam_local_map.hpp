// Tracking::SearchLocalPointsAndLines (Tracking.cc:3806-3919) on the device, for frames of one camera (Nleft == -1): two functions
// that replace the two loops over the local map and the matcher calls behind them.  INTEGRATION.md §2 has the edit recipe.
//
//   PliSearchLocalPoints   :3809-3855: Frame::isInFrustum of every local map point, IncreaseVisible(), mmProjectPoints and
//                          ORBmatcher(nnratio).SearchByProjection(F, vpLocalMapPoints, th, bFarPoints, thFarPoints), one call of
//                          pli_search_local_points.  The caller keeps the choice of th (:3832-3852).  A point that :3813 skips
//                          but that still has mbTrackInView set from an earlier frame (for one camera Tracking.cc:2996-3004
//                          resets only mbTrackInViewR) is searched by the reference with the fields it holds, and here too: it
//                          enters the call in its list position as a stored view.
//   PliSearchLocalLines    :3862-3919: Frame::isInFrustum_l, the list mvpLocalMapLines_InFrustum and match() on the device
//                          (pli_search_local_lines); mnTrackangle and the loop :3886-3919 here, on the fields as they stand (the
//                          reference never writes mTrackProjeX / mTrackProjeY).
//
// The types are template parameters, so that a test can put stubs in their place.  FrameT needs mnId, N, Nleft, mRcw, mtcw, mOw
// (CV_32F), fx, fy, cx, cy, mbf, mnMinX .. mnMaxY, mnScaleLevels, mfLogScaleFactor, mvKeysUn, mDescriptors, mvuRight, mvpMapPoints,
// mmProjectPoints and, for the lines, mDescriptors_Line, mvKeysUn_Line, mvDisparity_l and mvpMapLines.  MapPointT needs what
// PliORBmatcher::Fuse needs (GetWorldPos, GetNormal, the distance accessors and GetMaxDistance(): INTEGRATION.md gives the
// one-line accessor) plus mnId, mnLastFrameSeen, the mTrack* fields and IncreaseVisible(); MapLineT needs mnLastFrameSeen, isBad(),
// GetWorldPos() (indexable 0..2), GetDescriptor(), Observations(), IncreaseVisible(), mbTrackInView, mTrackProjsX / Y,
// mTrackProjeX / Y and mnTrackangle.
#pragma once
#include "orbslam_adapters.hpp"
#include <cmath>
#include <mutex>

namespace ORB_SLAM3 {

namespace pli_detail {

template <class FrameT>
inline void localMapPose(FrameT& F, float pose[15], pli_fuse_camera& cam) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) pose[3 * r + c] = F.mRcw.template at<float>(r, c);
    pose[9 + r] = F.mtcw.template at<float>(r);
    pose[12 + r] = F.mOw.template at<float>(r);
  }
  cam = pli_fuse_camera{F.fx, F.fy, F.cx, F.cy, F.mbf, (float)F.mnMinX, (float)F.mnMaxX, (float)F.mnMinY, (float)F.mnMaxY};
}

// the pli_fuse_point of a map point that is set and not bad, as PliORBmatcher::fusePoint makes it
template <class MapPointT>
inline pli_fuse_point localMapPoint(MapPointT* pMP) {
  pli_fuse_point P = {};
  if (!pMP || pMP->isBad()) return P;
  const cv::Mat p = pMP->GetWorldPos(), nrm = pMP->GetNormal();
  for (int i = 0; i < 3; ++i) { P.pos[i] = p.template at<float>(i); P.normal[i] = nrm.template at<float>(i); }
  P.min_dist_inv = pMP->GetMinDistanceInvariance();
  P.max_dist_inv = pMP->GetMaxDistanceInvariance();
  P.max_dist = pMP->GetMaxDistance();
  P.valid = (std::isfinite(P.max_dist) && P.max_dist > 0.f) ? 1 : 0;        // (the reference converts a NaN to int there)
  return P;
}

// The level_ratio table of pli_search_local_points for a frame's pyramid: MapPoint::PredictScale, MapPoint.cc:457-461, as MapPoint.cc
// compiles it (PliORBmatcher::fuseLevelRatio), made once per (mnScaleLevels, mfLogScaleFactor).
inline const std::vector<float>& localMapLevelRatio(int nlevels, float logSf) {
  static std::mutex mu;
  static std::vector<float> table;
  static int tableLevels = -1;
  static float tableLogSf = 0.0f;
  std::lock_guard<std::mutex> lock(mu);
  if (tableLevels != nlevels || tableLogSf != logSf) {
    table = pli::Frontend::fuseLevelRatio(nlevels, [nlevels, logSf](float ratio) {
      using namespace std;
      if (!(ratio > 0.0f)) return 0;
      if (std::isinf(ratio)) return nlevels - 1;
      int nScale = ceil(log(ratio) / logSf);
      if (nScale < 0) nScale = 0;
      else if (nScale >= nlevels) nScale = nlevels - 1;
      return nScale;
    });
    tableLevels = nlevels;
    tableLogSf = logSf;
  }
  return table;
}

}  // namespace pli_detail

// Returns the reference's nmatches (0 when nothing is in view: :3829).
template <class FrameT, class MapPointT>
int PliSearchLocalPoints(FrameT& F, std::vector<MapPointT*>& vpLocalMapPoints, float nnratio, float th, bool bFarPoints,
                         float thFarPoints) {
  if (F.Nleft != -1) throw std::logic_error("PliSearchLocalPoints: frames of two cameras are not covered");
  const size_t nq = vpLocalMapPoints.size();
  std::vector<pli_fuse_point> pts(nq);
  std::vector<uint8_t> desc(nq * 32, 0), live(nq, 0);
  for (size_t i = 0; i < nq; ++i) {
    MapPointT* pMP = vpLocalMapPoints[i];
    pts[i] = pli_fuse_point{};
    if (pMP->mnLastFrameSeen == F.mnId) {                                    // :3813
      // isInFrustum is skipped, but ORBmatcher.cc:53-62 still searches a point that kept mbTrackInView from an earlier frame
      // (one camera: Tracking.cc:2996-3004 resets only mbTrackInViewR), with the fields it holds
      if (!pMP->mbTrackInView || pMP->isBad()) continue;
      if (pMP->Observations() <= 0)
        throw std::logic_error("PliSearchLocalPoints: a point in view without observations is not covered");
      pli_fuse_point& P = pts[i];
      P.pos[0] = pMP->mTrackProjX; P.pos[1] = pMP->mTrackProjY; P.pos[2] = pMP->mTrackProjXR;
      P.normal[0] = pMP->mTrackDepth; P.normal[1] = pMP->mTrackViewCos; P.normal[2] = (float)pMP->mnTrackScaleLevel;
      P.valid = PLI_LOCAL_STORED_VIEW;
      std::memcpy(&desc[i * 32], pMP->GetDescriptor().template ptr<uint8_t>(), 32);
      continue;
    }
    if (pMP->isBad()) continue;                                              // :3815
    live[i] = 1;
    pts[i] = pli_detail::localMapPoint(pMP);
    if (pts[i].valid) std::memcpy(&desc[i * 32], pMP->GetDescriptor().template ptr<uint8_t>(), 32);
  }
  const int M = F.N;
  std::vector<pli_keypoint> kp((size_t)M);
  std::vector<uint8_t> occupied((size_t)M, 0);
  for (int j = 0; j < M; ++j) {
    kp[j] = pli_detail::keypoint(F.mvKeysUn[j]);
    if (F.mvpMapPoints[j] && F.mvpMapPoints[j]->Observations() > 0) occupied[j] = 1;        // ORBmatcher.cc:89-91
  }
  float pose[15];
  pli_fuse_camera cam;
  pli_detail::localMapPose(F, pose, cam);
  const std::vector<float>& levelRatio = pli_detail::localMapLevelRatio(F.mnScaleLevels, F.mfLogScaleFactor);
  std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("PliSearchLocalPoints");
  std::vector<pli_local_view> view;
  std::vector<int> best;
  int nToMatch = 0;
  const int nmatches = fe->searchLocalPoints(pts, desc.data(), pose, cam, 0.5f, th, bFarPoints, thFarPoints, nnratio, levelRatio, kp,
                                             F.mDescriptors.data, F.mvuRight.data(), occupied.data(), view, best, nToMatch);
  for (size_t i = 0; i < nq; ++i) {
    if (!live[i]) continue;
    MapPointT* pMP = vpLocalMapPoints[i];
    // Frame.cc:588-590 for every point that reaches isInFrustum, also one the device call left out (GetMaxDistance() not finite
    // and positive: its record is zero); :612-613
    const pli_local_view V = pts[i].valid ? view[i] : pli_local_view{-1.0f, -1.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0};
    pMP->mbTrackInView = V.in_view != 0;
    pMP->mTrackProjX = V.proj_x;
    pMP->mTrackProjY = V.proj_y;
    if (!V.in_view) continue;
    if (pMP->Observations() <= 0)
      throw std::logic_error("PliSearchLocalPoints: a point in view without observations is not covered");
    pMP->mTrackProjXR = V.proj_xr;                                           // :636-644
    pMP->mTrackDepth = V.depth;
    pMP->mnTrackScaleLevel = V.level;
    pMP->mTrackViewCos = V.view_cos;
    pMP->IncreaseVisible();                                                  // Tracking.cc:3820
    F.mmProjectPoints[pMP->mnId] = cv::Point2f(V.proj_x, V.proj_y);          // :3825
  }
  if (nToMatch == 0) return 0;                                               // :3829
  for (size_t i = 0; i < nq; ++i)
    if (best[i] >= 0) F.mvpMapPoints[best[i]] = vpLocalMapPoints[i];         // ORBmatcher.cc:130
  return nmatches;
}

// matches_12 is the reference's vector after the loop :3888-3919; vpInFrustum its mvpLocalMapLines_InFrustum.
template <class FrameT, class MapLineT>
void PliSearchLocalLines(FrameT& F, std::vector<MapLineT*>& vpLocalMapLines, float nnr, std::vector<MapLineT*>& vpInFrustum,
                         std::vector<int>& matches_12) {
  if (F.Nleft != -1) throw std::logic_error("PliSearchLocalLines: frames of two cameras are not covered");
  const size_t nl = vpLocalMapLines.size();
  std::vector<float> sp(3 * nl, 0.0f);
  std::vector<uint8_t> valid(nl, 0), desc(nl * 32, 0);
  for (size_t i = 0; i < nl; ++i) {
    MapLineT* pML = vpLocalMapLines[i];
    if (pML->mnLastFrameSeen == F.mnId) continue;                            // :3865
    if (pML->isBad()) continue;                                              // :3867
    valid[i] = 1;
    const auto sep = pML->GetWorldPos();
    for (int a = 0; a < 3; ++a) sp[3 * i + a] = (float)sep(a);               // Converter::toCvMat(sep.head(3))
    std::memcpy(&desc[i * 32], pML->GetDescriptor().template ptr<uint8_t>(), 32);
  }
  float pose[15];
  pli_fuse_camera cam;
  pli_detail::localMapPose(F, pose, cam);
  std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("PliSearchLocalLines");
  std::vector<int> inView, list;
  std::vector<float> projS;
  fe->searchLocalLines(sp, valid, desc.data(), pose, cam, F.mDescriptors_Line.data, F.mDescriptors_Line.rows, nnr, inView, projS, list,
                       matches_12);
  for (size_t i = 0; i < nl; ++i) {
    if (!valid[i]) continue;
    MapLineT* pML = vpLocalMapLines[i];
    pML->mbTrackInView = inView[i] != 0;                                     // Frame.cc:663
    if (!inView[i]) continue;
    pML->mTrackProjsX = projS[2 * i];                                        // :692-693
    pML->mTrackProjsY = projS[2 * i + 1];
    // :698, unqualified as there: the overload is the one the tree's headers select for two floats
    pML->mnTrackangle = atan2(pML->mTrackProjeY - pML->mTrackProjsY, pML->mTrackProjeX - pML->mTrackProjsX);
    pML->IncreaseVisible();                                                  // Tracking.cc:3873
  }
  vpInFrustum.clear();
  for (int i : list) vpInFrustum.push_back(vpLocalMapLines[i]);
  const double deltaWidth = (F.mnMaxX - F.mnMinX) * 0.1;                     // :3886-3887
  const double deltaHeight = (F.mnMaxY - F.mnMinY) * 0.1;
  for (int i1 = 0, n12 = (int)matches_12.size(); i1 < n12; ++i1) {
    const int i2 = matches_12[i1];
    if (i2 < 0) continue;
    if (F.mvDisparity_l[i2].first < 0 || F.mvDisparity_l[i2].second < 0) continue;
    if (F.mvpMapLines[i2])
      if (F.mvpMapLines[i2]->Observations() > 0) continue;
    MapLineT* pML = vpInFrustum[i1];
    const float& sX_curr = F.mvKeysUn_Line[i2].startPointX;
    const float& sX_last = pML->mTrackProjsX;
    const float& sY_curr = F.mvKeysUn_Line[i2].startPointY;
    const float& sY_last = pML->mTrackProjsY;
    const float& eX_curr = F.mvKeysUn_Line[i2].endPointX;
    const float& eX_last = pML->mTrackProjeX;
    const float& eY_curr = F.mvKeysUn_Line[i2].endPointY;
    const float& eY_last = pML->mTrackProjeY;
    if (fabs(sX_curr - sX_last) > deltaWidth || fabs(eX_curr - eX_last) > deltaWidth || fabs(sY_curr - sY_last) > deltaHeight ||
        fabs(eY_curr - eY_last) > deltaHeight) {
      matches_12[i1] = -1;
      continue;
    }
    F.mvpMapLines[i2] = pML;
  }
}

}  // namespace ORB_SLAM3
