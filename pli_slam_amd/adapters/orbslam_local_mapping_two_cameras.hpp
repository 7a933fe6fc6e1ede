// LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684) for keyframes of a rig of two KannalaBrandt8
// cameras (NLeft != -1, mpCamera2 set), the branch `mpCurrentKeyFrame->mpCamera2 && pKF2->mpCamera2` (:463-528), on the device:
// SearchForTriangulation against every neighbour, the triangulation and every gate of :530-667 with the pose and the camera that
// (bRight1, bRight2) pick per pair, in ONE call (pli_create_new_map_points_two_cameras), then :670-683 replayed on the host in the
// reference's order.  INTEGRATION.md §2 shows the edit of LocalMapping::CreateNewMapPoints.  What orbslam_local_mapping.hpp says
// about the loop's only coupling (a feature that received a map point from neighbour k is invisible to neighbour k + 1) holds here
// unchanged, and so does the answer: the first neighbour in which a feature is matched and accepted keeps it.
#pragma once
#include "orbslam_local_mapping.hpp"
#include "orbslam_two_cameras.hpp"

namespace ORB_SLAM3 {

// The signature and the rules of PliCreateNewMapPoints (vpNeighKFs, bCoarse, checkNewKeyFrames, the order of :670-683, the return
// value).  If no keyframe of the call has a second camera the call IS PliCreateNewMapPoints.  A call in which some keyframes have
// one and others have none throws std::logic_error (the reference falls through :463 with the poses left over from the previous
// pair), and so do cameras that differ between the keyframes of a call.
// KeyFrameT needs what PliORBmatcherTwoCameras::SearchForTriangulation reads, and GetCameraCenter(), GetRightCameraCenter(),
// mfScaleFactor, AddMapPoint(pMP, idx); what PliCreateNewMapPoints reads too when a call is forwarded.  mvKeysUn, mvuRight and
// mvDepth are not read for keyframes of two cameras, as the reference does not use them there (:446-459).
template <class MapPointT, class KeyFrameT, class AtlasT, class StopFn>
int PliCreateNewMapPointsTwoCameras(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, AtlasT* mpAtlas,
                                    std::list<MapPointT*>& mlpRecentAddedMapPoints, bool bCoarse, bool mbFarPoints,
                                    float mThFarPoints, StopFn checkNewKeyFrames) {
  const int nkf = (int)vpNeighKFs.size();
  int two = pKF1->mpCamera2 ? 1 : 0;
  for (KeyFrameT* pKF2 : vpNeighKFs) two += pKF2->mpCamera2 ? 1 : 0;
  if (two == 0)
    return PliCreateNewMapPoints<MapPointT>(pKF1, vpNeighKFs, mpAtlas, mlpRecentAddedMapPoints, bCoarse, mbFarPoints, mThFarPoints,
                                            checkNewKeyFrames);
  if (two != nkf + 1)
    throw std::logic_error("CreateNewMapPoints: keyframes with and without mpCamera2 in one call are not supported");
  if (nkf == 0) return 0;
  typedef pli_detail::TwoCameraTriangulationTable Table;
  pli_kb8_camera cam[2];
  pli_detail::kb8Cameras(pKF1, cam);
  Table T1, T2;
  pli_detail::gatherTwoCameraTriangulationTable(pKF1, cam, T1, "CreateNewMapPoints", "CreateNewMapPoints: mpCurrentKeyFrame->mFeatVec");
  const int n1 = pKF1->N;
  // per keyframe both sides' Rcw, tcw, Ow through the reference's getters (:464-527; GetPose / GetRightPose are the same floats)
  std::vector<float> rel((size_t)nkf * 48), pose1(30), kfPose((size_t)nkf * 30);
  pli_detail::fusePosesTwoCameras(pKF1, pose1.data());
  for (int k = 0; k < nkf; ++k) {
    KeyFrameT* pKF2 = vpNeighKFs[k];
    pli_detail::gatherTwoCameraTriangulationTable(pKF2, cam, T2, "CreateNewMapPoints", "CreateNewMapPoints: pKF2->mFeatVec");
    pli_detail::relativePosesTwoCameras(pKF1, pKF2, &rel[(size_t)k * 48]);                         // ORBmatcher.cc:995-1003
    pli_detail::fusePosesTwoCameras(pKF2, &kfPose[(size_t)k * 30]);
  }
  const float ratioFactor = 1.5f * pKF1->mfScaleFactor;                // :384
  pli::Frontend::NewMapPoints out;
  pli_detail::deviceContext("CreateNewMapPoints")
      ->createNewMapPointsTwoCameras(T1.kp.data(), T1.desc.data(), T1.node.data(), T1.hasMp.data(), n1, pKF1->NLeft, nkf, T2.off.data(),
                                     T2.nleft.data(), T2.kp.data(), T2.desc.data(), T2.node.data(), T2.hasMp.data(), cam[0], cam[1],
                                     rel.data(), pose1.data(), kfPose.data(), bCoarse, mbFarPoints, mThFarPoints, ratioFactor, out);
  return pli_detail::replayNewMapPoints(out, pKF1, vpNeighKFs, mpAtlas, mlpRecentAddedMapPoints, checkNewKeyFrames);
}

}  // namespace ORB_SLAM3
