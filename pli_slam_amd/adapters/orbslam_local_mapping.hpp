// LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684) for keyframes of one pinhole camera (NLeft == -1,
// no mpCamera2: monocular, rectified stereo, RGB-D), on the device: SearchForTriangulation against every neighbour, the
// triangulation and every gate of :530-667 in ONE call (pli_create_new_map_points), then :670-683 replayed on the host in the
// reference's order.  INTEGRATION.md §2 shows the edit of LocalMapping::CreateNewMapPoints.
//
// The reference's loop is sequential along the neighbours: a feature of mpCurrentKeyFrame that received a map point from
// neighbour k (AddMapPoint, :675) is skipped by the search of neighbour k + 1 (ORBmatcher.cc:1033-1039).  The batch form of
// PliORBmatcher::SearchForTriangulation searches every neighbour on the map-point state at entry and cannot know the
// triangulation's verdict, so one feature may come back matched in several neighbours; the device call here resolves it (the first
// neighbour in which the feature is matched and accepted keeps it) and its results are the sequential loop's exactly.
#pragma once
#include "orbslam_adapters.hpp"
#include <list>

namespace ORB_SLAM3 {

namespace pli_detail {
// :670-683 for what one device call created, in the reference's order; `if(i>0 && CheckNewKeyFrames()) return;` (:389) before
// neighbour k > 0 is applied.  Shared by PliCreateNewMapPoints and PliCreateNewMapPointsTwoCameras.
template <class MapPointT, class KeyFrameT, class AtlasT, class StopFn>
int replayNewMapPoints(const pli::Frontend::NewMapPoints& out, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs,
                       AtlasT* mpAtlas, std::list<MapPointT*>& mlpRecentAddedMapPoints, StopFn checkNewKeyFrames) {
  const int nkf = (int)vpNeighKFs.size(), n1 = pKF1->N;
  int created = 0;
  for (int k = 0; k < nkf; ++k) {
    if (k > 0 && checkNewKeyFrames()) return created;                  // :389
    KeyFrameT* pKF2 = vpNeighKFs[k];
    for (int idx1 = 0; idx1 < n1; ++idx1) {                            // vMatchedIndices is vMatches12 read in index order
      const size_t p = (size_t)k * n1 + idx1;
      if (out.status[p] != PLI_NEWPT_CREATED) continue;
      const int idx2 = out.matches12[p];
      cv::Mat x3D(3, 1, CV_32F);
      for (int r = 0; r < 3; ++r) x3D.template at<float>(r) = out.x3d[3 * p + r];
      MapPointT* pMP = new MapPointT(x3D, pKF1, mpAtlas->GetCurrentMap());          // :670
      pMP->AddObservation(pKF1, idx1);
      pMP->AddObservation(pKF2, idx2);
      pKF1->AddMapPoint(pMP, idx1);
      pKF2->AddMapPoint(pMP, idx2);
      pMP->ComputeDistinctiveDescriptors();
      pMP->UpdateNormalAndDepth();
      mpAtlas->AddMapPoint(pMP);
      mlpRecentAddedMapPoints.push_back(pMP);
      ++created;
    }
  }
  return created;
}
}  // namespace pli_detail

// vpNeighKFs: the neighbours that passed the baseline / median-depth test of :396-413 (it stays with the caller), in the
// reference's order.  bCoarse: :420-422.  checkNewKeyFrames: asked before neighbour k > 0 is applied, as `if(i>0 &&
// CheckNewKeyFrames()) return;` (:389); whatever was not applied is dropped.  First-accepted-wins is a prefix property, so the
// state after an early return equals the reference's.  Returns the number of map points created.
// Per created point, in the reference's order (neighbour by neighbour, idx1 ascending within a neighbour): new MapPoint(x3D,
// pKF1, mpAtlas->GetCurrentMap()), both AddObservation, both AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth,
// mpAtlas->AddMapPoint, mlpRecentAddedMapPoints.push_back (:670-683).
// KeyFrameT needs what PliORBmatcher::SearchForTriangulation reads, and mvKeys, mvDepth, fx, fy, cx, cy, mbf, mb, mfScaleFactor,
// AddMapPoint(pMP, idx).  A keyframe of two cameras throws std::logic_error: the branch :463-528 is
// PliCreateNewMapPointsTwoCameras (orbslam_local_mapping_two_cameras.hpp), which forwards here when no keyframe has a second camera.
template <class MapPointT, class KeyFrameT, class AtlasT, class StopFn>
int PliCreateNewMapPoints(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, AtlasT* mpAtlas,
                          std::list<MapPointT*>& mlpRecentAddedMapPoints, bool bCoarse, bool mbFarPoints, float mThFarPoints,
                          StopFn checkNewKeyFrames) {
  // the search's tables (the gather of the batch SearchForTriangulation), and what :530-667 read beyond them
  struct Table : pli_detail::TriangulationTable {
    std::vector<float> uright, depth, key, pose;
  };
  auto gather = [](KeyFrameT* pKF, Table& T, const char* what) {
    pli_detail::gatherTriangulationTable(pKF, T, "CreateNewMapPoints", what);
    for (int i = 0; i < pKF->N; ++i) {
      T.uright.push_back(pKF->mvuRight[i]);
      T.depth.push_back(pKF->mvDepth[i]);
      T.key.push_back(pKF->mvKeys[i].pt.x);                            // KeyFrame::UnprojectStereo reads mvKeys (KeyFrame.cc:937-938)
      T.key.push_back(pKF->mvKeys[i].pt.y);
    }
    const cv::Mat Ow = pKF->GetCameraCenter();                         // the stored value
    T.pose.insert(T.pose.end(), T.R, T.R + 9);
    T.pose.insert(T.pose.end(), T.t, T.t + 3);
    for (int i = 0; i < 3; ++i) T.pose.push_back(Ow.template at<float>(i));
  };
  const int nkf = (int)vpNeighKFs.size();
  if (nkf == 0) return 0;
  Table T1, T2;
  gather(pKF1, T1, "CreateNewMapPoints: mpCurrentKeyFrame->mFeatVec");
  const int n1 = pKF1->N;
  std::vector<float> F12((size_t)nkf * 9), ep((size_t)nkf * 2);
  for (int k = 0; k < nkf; ++k) {
    gather(vpNeighKFs[k], T2, "CreateNewMapPoints: pKF2->mFeatVec");
    pli_detail::triangulationGeometry(T1.R, T1.t, &T1.pose[12], T1.K, T2.R, T2.t, T2.K, &F12[(size_t)k * 9], &ep[(size_t)k * 2]);
  }
  // fx1..cy1 / fx2..cy2 and mpCurrentKeyFrame->mbf (:377-382, :432-437, :616, :641): one camera serves the call
  pli_fuse_camera cam = {};
  cam.fx = pKF1->fx; cam.fy = pKF1->fy; cam.cx = pKF1->cx; cam.cy = pKF1->cy; cam.bf = pKF1->mbf;
  for (KeyFrameT* pKF2 : vpNeighKFs)
    if (pKF2->fx != cam.fx || pKF2->fy != cam.fy || pKF2->cx != cam.cx || pKF2->cy != cam.cy || pKF2->mb != pKF1->mb)
      throw std::logic_error("CreateNewMapPoints: the keyframes of one call must share their camera parameters");
  const float ratioFactor = 1.5f * pKF1->mfScaleFactor;                // :384
  pli::Frontend::NewMapPoints out;
  pli_detail::deviceContext("CreateNewMapPoints")
      ->createNewMapPoints(T1.kp.data(), T1.desc.data(), T1.node.data(), T1.hasMp.data(), T1.uright.data(), T1.depth.data(),
                           T1.key.data(), n1, nkf, T2.off.data(), T2.kp.data(), T2.desc.data(), T2.node.data(), T2.hasMp.data(),
                           T2.uright.data(), T2.depth.data(), T2.key.data(), F12.data(), ep.data(), T1.pose.data(), T2.pose.data(),
                           cam, pKF1->mb, bCoarse, mbFarPoints, mThFarPoints, ratioFactor, out);
  return pli_detail::replayNewMapPoints(out, pKF1, vpNeighKFs, mpAtlas, mlpRecentAddedMapPoints, checkNewKeyFrames);
}

}  // namespace ORB_SLAM3
