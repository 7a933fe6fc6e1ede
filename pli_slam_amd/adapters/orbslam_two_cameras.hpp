// The two SearchByProjection forms of ORB_SLAM3::ORBmatcher that run on every tracked frame, for a frame of two cameras
// (Frame::Nleft != -1, the fisheye-stereo rig), SearchForTriangulation and Fuse(pKF, vpMapPoints, th, bRight) for keyframes of two
// cameras (mpCamera2 set, NLeft != -1), SearchByBoW(pKF, F, vpMapPointMatches) for such frames and keyframes and
// SearchByBoW(pKF1, pKF2, vpMatches12) for such keyframes: a matcher that is PliORBmatcher in everything else.
//
//   inside the PLI-SLAM tree:  using ORBmatcher = ORB_SLAM3::PliORBmatcherTwoCameras<Frame, MapPoint>;
//
// PliORBmatcher itself keeps refusing such frames and keyframes (its users' types need no second-camera members); this class
// hides the members below and forwards each to it when the frame or every keyframe of the call has one camera.
#pragma once
#include "orbslam_adapters.hpp"
#include <algorithm>
#include <cstring>
#include <utility>

namespace ORB_SLAM3 {

namespace pli_detail {

// The four relative poses of ORBmatcher.cc:995-1003 for (pKF1, pKF2), the reference's own cv::Mat expressions: rel[4 x 12] = ll, lr,
// rl, rr, each R12 row major and then t12.  Host arithmetic only (tests compile it without a device).
template <class KeyFrameT>
inline void relativePosesTwoCameras(KeyFrameT* pKF1, KeyFrameT* pKF2, float* rel) {
  const cv::Mat R[4] = {pKF1->GetRotation() * pKF2->GetRotation().t(), pKF1->GetRotation() * pKF2->GetRightRotation().t(),        // :995-998
                        pKF1->GetRightRotation() * pKF2->GetRotation().t(), pKF1->GetRightRotation() * pKF2->GetRightRotation().t()};
  const cv::Mat t[4] = {                                                                                                           // :1000-1003
      pKF1->GetRotation() * (-pKF2->GetRotation().t() * pKF2->GetTranslation()) + pKF1->GetTranslation(),
      pKF1->GetRotation() * (-pKF2->GetRightRotation().t() * pKF2->GetRightTranslation()) + pKF1->GetTranslation(),
      pKF1->GetRightRotation() * (-pKF2->GetRotation().t() * pKF2->GetTranslation()) + pKF1->GetRightTranslation(),
      pKF1->GetRightRotation() * (-pKF2->GetRightRotation().t() * pKF2->GetRightTranslation()) + pKF1->GetRightTranslation()};
  for (int p = 0; p < 4; ++p) {
    float* out = rel + p * 12;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) out[i * 3 + j] = R[p].template at<float>(i, j);
      out[9 + i] = t[p].template at<float>(i);
    }
  }
}

// The two poses Fuse(pKF, vpMapPoints, th, bRight) reads (:1404-1417): pose[2 x 15] = left, right, each Rcw row major, tcw, Ow.
template <class KeyFrameT>
inline void fusePosesTwoCameras(KeyFrameT* pKF, float* pose) {
  const cv::Mat R[2] = {pKF->GetRotation(), pKF->GetRightRotation()}, t[2] = {pKF->GetTranslation(), pKF->GetRightTranslation()},
                Ow[2] = {pKF->GetCameraCenter(), pKF->GetRightCameraCenter()};
  for (int e = 0; e < 2; ++e)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) pose[e * 15 + i * 3 + j] = R[e].template at<float>(i, j);
      pose[e * 15 + 9 + i] = t[e].template at<float>(i);
      pose[e * 15 + 12 + i] = Ow[e].template at<float>(i);
    }
}

// mpCamera / mpCamera2 of a keyframe of two cameras: eight KannalaBrandt8 parameters each (GeometricCamera.h:77-80)
template <class KeyFrameT>
inline void kb8Cameras(KeyFrameT* pKF, pli_kb8_camera cam[2]) {
  if (!pKF->mpCamera || !pKF->mpCamera2 || pKF->mpCamera->size() != 8 || pKF->mpCamera2->size() != 8)
    throw std::logic_error("PliORBmatcherTwoCameras: a keyframe of two cameras needs two KannalaBrandt8 cameras (8 parameters each)");
  for (int e = 0; e < 2; ++e) {
    float v[8];
    for (int i = 0; i < 8; ++i) v[i] = e ? pKF->mpCamera2->getParameter(i) : pKF->mpCamera->getParameter(i);
    cam[e] = pli_kb8_camera{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
  }
}

// The tables of SearchForTriangulation for keyframes of two cameras (the batch search and PliCreateNewMapPointsTwoCameras): a
// keyframe's rows are mvKeys then mvKeysRight (:1048-1050, :1083-1085), its cameras must be `cam`, the call's.
struct TwoCameraTriangulationTable : KfTable {
  std::vector<pli_keypoint> kp;
  std::vector<uint8_t> hasMp;
  std::vector<int32_t> nleft;
};
template <class KeyFrameT>
inline void gatherTwoCameraTriangulationTable(KeyFrameT* pKF, const pli_kb8_camera cam[2], TwoCameraTriangulationTable& T,
                                              const std::string& who, const char* what) {
  const int n = pKF->N, nl = pKF->NLeft;
  if (nl < 0 || nl > n || (int)pKF->mvKeys.size() < nl || (int)pKF->mvKeysRight.size() < n - nl || pKF->mDescriptors.rows < n)
    throw std::logic_error(who + ": a keyframe's tables do not hold NLeft + NRight rows");
  pli_kb8_camera own[2];
  kb8Cameras(pKF, own);
  if (std::memcmp(own, cam, sizeof(own)) != 0)
    throw std::logic_error(who + ": the keyframes of one call must share their camera parameters");
  appendNodes(T, pKF->mFeatVec, n, what);
  appendDescriptors(T, pKF->mDescriptors, n);
  for (int i = 0; i < n; ++i) {
    T.kp.push_back(keypoint(i < nl ? pKF->mvKeys[i] : pKF->mvKeysRight[i - nl]));      // :1048-1050, :1083-1085
    T.hasMp.push_back(pKF->GetMapPoint(i) ? 1 : 0);                 // (:1033-1039, :1064-1068: isBad() is not asked)
  }
  T.nleft.push_back(nl);
}

}  // namespace pli_detail

// FrameT needs, beyond what PliORBmatcher reads: Nleft, Nright, mvKeys, mvKeysRight, mDescriptors (Nleft + Nright rows, the left
// camera's first), mvpMapPoints (Nleft + Nright slots), mTrl (3 x 4, CV_32F), mpCamera (with project(cv::Mat) -> cv::Point2f),
// mvLeftToRightMatch and mvRightToLeftMatch.  MapPointT needs mbTrackInViewR, mTrackProjXR / YR, mTrackViewCosR and
// mnTrackScaleLevelR.
template <class FrameT, class MapPointT>
class PliORBmatcherTwoCameras : public PliORBmatcher<FrameT, MapPointT> {
  typedef PliORBmatcher<FrameT, MapPointT> Base;

 public:
  PliORBmatcherTwoCameras(float nnratio = 0.6, bool checkOri = true) : Base(nnratio, checkOri) {}

  using Base::SearchByProjection;            // every other form stays visible; the two below hide theirs
  using Base::SearchForTriangulation;        // likewise: both forms below hide theirs and forward to them
  using Base::Fuse;                          // the Sim3 form stays the base's; the two forms below hide theirs
  using Base::SearchByBoW;                   // the (KF, F) and the (KF, KF) forms below hide theirs and forward to them

  // ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono),
  // ORBmatcher.cc:1961-2177 (Tracking::TrackWithMotionModel, Tracking.cc:2961, :2969).  For CurrentFrame.Nleft != -1 the two
  // projections (:1971-2013, :2084-2092) are the reference's own cv::Mat expressions and the frame's mpCamera->project, run here;
  // both cameras' window searches, the "already taken" exclusion per camera, TH_HIGH, the joint rotation histogram and
  // ComputeThreeMaxima run on the device (pli_search_by_projection_two_cameras).
  int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono) {
    if (CurrentFrame.Nleft == -1) return Base::SearchByProjection(CurrentFrame, LastFrame, th, bMono);
    const cv::Mat Rcw = CurrentFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const cv::Mat tcw = CurrentFrame.mTcw.rowRange(0, 3).col(3);
    const cv::Mat twc = -Rcw.t() * tcw;
    const cv::Mat Rlw = LastFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const cv::Mat tlw = LastFrame.mTcw.rowRange(0, 3).col(3);
    const cv::Mat tlc = Rlw * twc + tlw;
    const bool bForward = tlc.at<float>(2) > CurrentFrame.mb && !bMono;
    const bool bBackward = -tlc.at<float>(2) > CurrentFrame.mb && !bMono;
    const int N = LastFrame.N;
    std::vector<pli_proj_query> qL((size_t)N), qR((size_t)N);
    std::vector<uint8_t> qdesc((size_t)N * 32, 0);
    for (int i = 0; i < N; i++) {
      std::memset(&qL[i], 0, sizeof(pli_proj_query));
      std::memset(&qR[i], 0, sizeof(pli_proj_query));
      qL[i].max_level = qR[i].max_level = -1;
      MapPointT* pMP = LastFrame.mvpMapPoints[i];
      if (!pMP || LastFrame.mvbOutlier[i]) continue;
      cv::Mat x3Dw = pMP->GetWorldPos();
      cv::Mat x3Dc = Rcw * x3Dw + tcw;
      const float invzc = 1.0 / x3Dc.at<float>(2);
      if (invzc < 0) continue;
      const cv::Point2f uv = CurrentFrame.mpCamera->project(x3Dc);
      const bool lastLeft = LastFrame.Nleft == -1 || i < LastFrame.Nleft;
      const int nLastOctave = lastLeft ? LastFrame.mvKeys[i].octave : LastFrame.mvKeysRight[i - LastFrame.Nleft].octave;   // :2009
      const float radius = th * CurrentFrame.mvScaleFactors[nLastOctave];
      pli_proj_query& Q = qL[i];
      Q.u = uv.x; Q.v = uv.y; Q.radius = radius;
      if (bForward) { Q.min_level = nLastOctave; Q.max_level = -1; }
      else if (bBackward) { Q.min_level = 0; Q.max_level = nLastOctave; }
      else { Q.min_level = nLastOctave - 1; Q.max_level = nLastOctave + 1; }
      const cv::KeyPoint& kpLF = (LastFrame.Nleft == -1) ? LastFrame.mvKeysUn[i]                                           // :2066-2068
                                                        : lastLeft ? LastFrame.mvKeys[i] : LastFrame.mvKeysRight[i - LastFrame.Nleft];
      Q.angle = kpLF.angle;
      // (the image gate :2004-2007 and the two `continue`s that leave the right camera unsearched are the library's)
      Q.valid = pMP->Observations() > 0 ? 1 : (1 | PLI_PROJ_NO_OBSERVATIONS);
      cv::Mat x3Dr = CurrentFrame.mTrl.colRange(0, 3).rowRange(0, 3) * x3Dc + CurrentFrame.mTrl.col(3);                   // :2084
      const cv::Point2f uvr = CurrentFrame.mpCamera->project(x3Dr);                                                        // :2086
      qR[i] = Q;
      qR[i].u = uvr.x; qR[i].v = uvr.y;
      const cv::Mat dMP = pMP->GetDescriptor();
      std::memcpy(&qdesc[(size_t)i * 32], dMP.template ptr<uint8_t>(), 32);
    }
    Tables T(CurrentFrame);
    std::vector<int> bestL, bestR, rawL, rawR;
    const int nmatches = pli_detail::deviceContext("SearchByProjection(CurrentFrame, LastFrame)")->searchByProjectionTwoCameras(
        qL, qR, qdesc.data(), T.kpL, T.descL, T.occL.data(), T.kpR, T.descR, T.occR.data(), CurrentFrame.mnMinX, CurrentFrame.mnMaxX,
        CurrentFrame.mnMinY, CurrentFrame.mnMaxY, this->mbCheckOrientation, bestL, bestR, &rawL, &rawR);
    // the reference's writes, replayed in its order: per row the left match, then the right one (:2061, :2128: the last writer
    // holds the slot), then the rotation filter's removals (:2169)
    const int Nleft = CurrentFrame.Nleft;
    for (int i = 0; i < N; ++i) {
      if (rawL[i] >= 0) CurrentFrame.mvpMapPoints[rawL[i]] = LastFrame.mvpMapPoints[i];
      if (rawR[i] >= 0) CurrentFrame.mvpMapPoints[rawR[i] + Nleft] = LastFrame.mvpMapPoints[i];
    }
    for (int i = 0; i < N; ++i) {
      if (rawL[i] >= 0 && bestL[i] < 0) CurrentFrame.mvpMapPoints[rawL[i]] = static_cast<MapPointT*>(nullptr);
      if (rawR[i] >= 0 && bestR[i] < 0) CurrentFrame.mvpMapPoints[rawR[i] + Nleft] = static_cast<MapPointT*>(nullptr);
    }
    return nmatches;
  }

  // ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th, const bool bFarPoints, const
  // float thFarPoints), ORBmatcher.cc:44-214 (Tracking::SearchLocalPoints, Tracking.cc:3854).  For F.Nleft != -1 the gates :53-62
  // and RadiusByViewingCos are the reference's own expressions, run here; both cameras' windows, the ratio tests and the writes
  // to the stereo partners run on the device (pli_search_local_map_fisheye).  Refused, as by PliORBmatcher and for its reason: a
  // point that searches and has Observations() == 0 (the reference would leave the slot it takes open, the device closes it).
  int SearchByProjection(FrameT& F, const std::vector<MapPointT*>& vpMapPoints, const float th = 3, const bool bFarPoints = false,
                         const float thFarPoints = 50.0f) {
    if (F.Nleft == -1) return Base::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints);
    const bool bFactor = th != 1.0;
    const size_t nq = vpMapPoints.size();
    std::vector<pli_proj_query> qL(nq), qR(nq);
    std::vector<uint8_t> qdesc(nq * 32, 0);
    for (size_t iMP = 0; iMP < nq; ++iMP) {
      std::memset(&qL[iMP], 0, sizeof(pli_proj_query));
      std::memset(&qR[iMP], 0, sizeof(pli_proj_query));
      MapPointT* pMP = vpMapPoints[iMP];
      if (!pMP->mbTrackInView && !pMP->mbTrackInViewR) continue;             // :53
      if (bFarPoints && pMP->mTrackDepth > thFarPoints) continue;            // :56
      if (pMP->isBad()) continue;                                            // :59
      if (pMP->mbTrackInView) {                                              // :62-73
        const int nPredictedLevel = pMP->mnTrackScaleLevel;
        float r = pMP->mTrackViewCos > 0.998 ? 2.5 : 4.0;                    // RadiusByViewingCos :216-222
        if (bFactor) r *= th;
        pli_proj_query& Q = qL[iMP];
        Q.u = pMP->mTrackProjX; Q.v = pMP->mTrackProjY;
        Q.radius = r * F.mvScaleFactors[nPredictedLevel];
        Q.min_level = nPredictedLevel - 1; Q.max_level = nPredictedLevel;
        Q.valid = 1;
      }
      if (pMP->mbTrackInViewR && pMP->mnTrackScaleLevelR != -1) {            // :145-151 (no th factor)
        const int nPredictedLevel = pMP->mnTrackScaleLevelR;
        const float r = pMP->mTrackViewCosR > 0.998 ? 2.5 : 4.0;
        pli_proj_query& Q = qR[iMP];
        Q.u = pMP->mTrackProjXR; Q.v = pMP->mTrackProjYR;
        Q.radius = r * F.mvScaleFactors[nPredictedLevel];
        Q.min_level = nPredictedLevel - 1; Q.max_level = nPredictedLevel;
        Q.valid = 1;
      }
      if (!qL[iMP].valid && !qR[iMP].valid) continue;
      if (pMP->Observations() <= 0)
        throw std::logic_error("SearchByProjection(F, vpMapPoints): a point in view without observations is not covered");
      const cv::Mat dMP = pMP->GetDescriptor();
      std::memcpy(&qdesc[iMP * 32], dMP.template ptr<uint8_t>(), 32);
    }
    Tables T(F);
    if ((int)F.mvLeftToRightMatch.size() != F.Nleft || (int)F.mvRightToLeftMatch.size() != F.Nright)
      throw std::logic_error("SearchByProjection(F, vpMapPoints): mvLeftToRightMatch / mvRightToLeftMatch do not fit Nleft / Nright");
    const std::vector<int> l2r(F.mvLeftToRightMatch.begin(), F.mvLeftToRightMatch.end());
    const std::vector<int> r2l(F.mvRightToLeftMatch.begin(), F.mvRightToLeftMatch.end());
    std::vector<int> mpL, mpR;
    const int nmatches = pli_detail::deviceContext("SearchByProjection(F, vpMapPoints)")->searchLocalMapFishEye(
        qL, qR, qdesc.data(), T.kpL, T.descL, T.occL.data(), l2r, T.kpR, T.descR, T.occR.data(), r2l, F.mnMinX, F.mnMaxX, F.mnMinY,
        F.mnMaxY, this->mfNNratio, mpL, mpR);
    for (int k = 0; k < F.Nleft; ++k)
      if (mpL[k] >= 0) F.mvpMapPoints[k] = vpMapPoints[mpL[k]];              // :130, :200
    for (int k = 0; k < F.Nright; ++k)
      if (mpR[k] >= 0) F.mvpMapPoints[k + F.Nleft] = vpMapPoints[mpR[k]];    // :133, :206
    return nmatches;
  }

  // ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vector<pair<size_t, size_t>>& vMatchedPairs,
  // const bool bOnlyStereo, const bool bCoarse), ORBmatcher.cc:965-1206 (LocalMapping::CreateNewMapPoints, LocalMapping.cc:387-423;
  // Tracking.cc:4705).  For keyframes with mpCamera2 the four relative poses of :995-1003 are the reference's own cv::Mat
  // expressions, run here; the BoW-node walk and KannalaBrandt8::epipolarConstrain per candidate run on the device
  // (pli_search_for_triangulation_two_cameras).  F12 is not read, as the reference does not read it.  KeyFrameT needs, beyond
  // what PliORBmatcher::SearchForTriangulation reads when it is forwarded to: mvKeys, mvKeysRight, GetRightRotation(),
  // GetRightTranslation(), and cameras with getParameter(i) and size() (GeometricCamera.h:77-80), the 8 KannalaBrandt8 parameters.
  template <class KeyFrameT>
  int SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, cv::Mat /*F12*/, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                             const bool bOnlyStereo, const bool bCoarse = false) {
    std::vector<std::vector<std::pair<size_t, size_t>>> pairs;
    std::vector<int> nmatches;
    SearchForTriangulation(pKF1, std::vector<KeyFrameT*>(1, pKF2), pairs, nmatches, bOnlyStereo, bCoarse);
    vMatchedPairs.swap(pairs[0]);
    return nmatches[0];
  }

  // (not in the reference) The same for every neighbour of vpKF2 in ONE device call, as the base's batch form.  Every keyframe
  // of the call has two cameras with the same parameters, or none has (then the base's form runs); anything else throws.
  template <class KeyFrameT>
  void SearchForTriangulation(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpKF2,
                              std::vector<std::vector<std::pair<size_t, size_t>>>& vvMatchedPairs, std::vector<int>& vnmatches,
                              const bool bOnlyStereo, const bool bCoarse = false) {
    const int nkf = (int)vpKF2.size();
    int two = pKF1->mpCamera2 ? 1 : 0;
    for (KeyFrameT* pKF2 : vpKF2) two += pKF2->mpCamera2 ? 1 : 0;
    if (two == 0) {
      Base::SearchForTriangulation(pKF1, vpKF2, vvMatchedPairs, vnmatches, bOnlyStereo, bCoarse);
      return;
    }
    if (two != nkf + 1)     // (the reference multiplies by an empty R12 for such a pair)
      throw std::logic_error("SearchForTriangulation: keyframes with and without mpCamera2 in one call are not supported");
    typedef pli_detail::TwoCameraTriangulationTable Table;
    pli_kb8_camera cam[2];
    kb8Cameras(pKF1, cam);
    auto gather = [&](KeyFrameT* pKF, Table& T, const char* what) {
      pli_detail::gatherTwoCameraTriangulationTable(pKF, cam, T, "SearchForTriangulation", what);
    };
    Table T1, T2;
    gather(pKF1, T1, "SearchForTriangulation: pKF1->mFeatVec");
    const int n1 = pKF1->N;
    std::vector<float> rel((size_t)nkf * 48 + 1);
    for (int k = 0; k < nkf; ++k) {
      KeyFrameT* pKF2 = vpKF2[k];
      gather(pKF2, T2, "SearchForTriangulation: pKF2->mFeatVec");
      pli_detail::relativePosesTwoCameras(pKF1, pKF2, &rel[(size_t)k * 48]);                       // :995-1003
    }
    std::vector<int> matches;
    pli_detail::deviceContext("SearchForTriangulation")
        ->searchForTriangulationTwoCameras(T1.kp.data(), T1.desc.data(), T1.node.data(), T1.hasMp.data(), n1, pKF1->NLeft, nkf,
                                           T2.off.data(), T2.nleft.data(), T2.kp.data(), T2.desc.data(), T2.node.data(), T2.hasMp.data(),
                                           cam[0], cam[1], rel.data(), bOnlyStereo, bCoarse, this->mbCheckOrientation, matches, vnmatches);
    vvMatchedPairs.assign((size_t)nkf, std::vector<std::pair<size_t, size_t>>());
    for (int k = 0; k < nkf; ++k) vvMatchedPairs[k].reserve(vnmatches[k]);
    pli_detail::forEachMatch(matches, nkf, n1, [&](int k, int i, int j) {      // vMatches12 read in index order (:1198-1203)
      vvMatchedPairs[k].push_back(std::make_pair((size_t)i, (size_t)j));
    });
  }

  // ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th, const bool bRight), ORBmatcher.cc:
  // 1399-1609, for a keyframe of two KannalaBrandt8 cameras (NLeft != -1): the pose of the side (GetRotation() ... or
  // GetRightRotation() / GetRightTranslation() / GetRightCameraCenter(), KeyFrame.cc:1343-1373) is read here, the projection with
  // the side's camera and the window search over the side's grid run on the device (pli_fuse_search_two_cameras), :1572-1594 and
  // the gates isBad() / IsInKeyFrame here (the base's replay).  A keyframe with NLeft == -1 goes to the base.
  // There is no stereo bound for such a keyframe: the fisheye constructor sets every mvuRight to -1 (Frame.cc:1589), and :1533
  // reads mvuRight[idx] with the camera-local idx, on a vector of Nleft entries - out of range for a right row >= Nleft.  So a
  // keyframe with NLeft != -1 and any mvuRight[i] >= 0 throws std::logic_error.
  // KeyFrameT needs, beyond what PliORBmatcher::Fuse reads: mvKeys, mvKeysRight, mpCamera / mpCamera2 (getParameter(i), size()) and
  // the three right-pose getters.
  template <class KeyFrameT>
  int Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th = 3.0, const bool bRight = false) {
    if (pKF->NLeft == -1) return Base::Fuse(pKF, vpMapPoints, th, bRight);
    std::vector<int> nFused;
    fuseTwoCameras(std::vector<KeyFrameT*>(1, pKF), vpMapPoints, th, bRight ? 2 : 1, nFused, nullptr);
    return nFused[0];
  }

  // (not in the reference) The loop of LocalMapping::SearchInNeighbors, LocalMapping.cc:743-749 - Fuse(pKFi, vpMapPointMatches) and
  // Fuse(pKFi, vpMapPointMatches, 3.0, true) for every target keyframe - with ONE device search for all targets and both cameras,
  // replayed in the reference's order: keyframe k left, keyframe k right, keyframe k + 1 left, ...  nFused[2 k] and nFused[2 k + 1]
  // are the two return values for keyframe k.  The replay and its three rules are the base's (fuseReplay): a point added to
  // keyframe k on the left is in the keyframe when the right camera's turn comes and is skipped there (:1448).  When no target has
  // two cameras the base's form runs (nFused[k]); targets with and without throw std::logic_error.
  template <class KeyFrameT>
  void Fuse(const std::vector<KeyFrameT*>& vpTargetKFs, const std::vector<MapPointT*>& vpMapPoints, const float th,
            std::vector<int>& nFused, int* pnResearch = nullptr) {
    int two = 0;
    for (KeyFrameT* pKF : vpTargetKFs) two += pKF->NLeft != -1 ? 1 : 0;
    if (two == 0) {
      Base::Fuse(vpTargetKFs, vpMapPoints, th, nFused, pnResearch);
      return;
    }
    if (two != (int)vpTargetKFs.size())
      throw std::logic_error("Fuse: keyframes with and without a second camera (NLeft != -1) in one call are not supported");
    fuseTwoCameras(vpTargetKFs, vpMapPoints, th, 3, nFused, pnResearch);
  }

  // ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches), ORBmatcher.cc:269-470, with the
  // two-camera text: a frame with F.Nleft != -1 goes to pli_search_by_bow_two_cameras (:342-369, :373-433; the frame's angles from
  // mvKeys / mvKeysRight by Nleft, :386-389, :416-419); a frame of one camera against a keyframe with mpCamera2 goes to
  // pli_search_by_bow with the keyframe's angles from mvKeys / mvKeysRight by NLeft (:379-382); anything else to the base.
  // vpMapPointMatches is written as the reference writes it.
  template <class KeyFrameT>
  int SearchByBoW(KeyFrameT* pKF, FrameT& F, std::vector<MapPointT*>& vpMapPointMatches) {
    std::vector<std::vector<MapPointT*>> matches;
    std::vector<int> nmatches;
    SearchByBoW(std::vector<KeyFrameT*>(1, pKF), F, matches, nmatches);
    vpMapPointMatches.swap(matches[0]);
    return nmatches[0];
  }

  // (not in the reference) The same for every keyframe of vpKFs in ONE device call (Tracking::Relocalization, Tracking.cc:4205-4230).
  template <class KeyFrameT>
  void SearchByBoW(const std::vector<KeyFrameT*>& vpKFs, FrameT& F, std::vector<std::vector<MapPointT*>>& vvpMapPointMatches,
                   std::vector<int>& vnmatches) {
    bool anyTwo = F.Nleft != -1;
    for (KeyFrameT* pKF : vpKFs) anyTwo = anyTwo || pKF->mpCamera2;
    if (!anyTwo) {
      Base::SearchByBoW(vpKFs, F, vvpMapPointMatches, vnmatches);
      return;
    }
    const int nf = F.N, nkf = (int)vpKFs.size(), nl = F.Nleft;
    if (nl != -1 && (nl < 0 || nl > nf || (int)F.mvKeys.size() < nl || (int)F.mvKeysRight.size() < nf - nl))
      throw std::logic_error("SearchByBoW: the frame's tables do not hold Nleft + Nright rows");
    pli_detail::KfTable TF;
    pli_detail::appendNodes(TF, F.mFeatVec, nf, "SearchByBoW: F.mFeatVec");
    pli_detail::appendDescriptors(TF, F.mDescriptors, nf);
    std::vector<float> fAngle((size_t)nf);
    for (int i = 0; i < nf; ++i) fAngle[i] = (nl == -1 || i < nl) ? F.mvKeys[i].angle : F.mvKeysRight[i - nl].angle;   // :386-389, :416-419
    std::vector<std::vector<MapPointT*>> kfPoints((size_t)nkf);
    typename Base::BowTable T;
    for (int k = 0; k < nkf; ++k) {
      KeyFrameT* pKF = vpKFs[k];
      kfPoints[k] = pKF->GetMapPointMatches();
      if (!pKF->mpCamera2) {                                                 // mvKeysUn, :380
        Base::bowGatherKeyFrame(pKF, kfPoints[k], "SearchByBoW: pKF->mFeatVec", T);
        continue;
      }
      const int n = pKF->N, knl = pKF->NLeft;                                // mvKeys / mvKeysRight by NLeft, :381-382
      if (knl < 0 || knl > n || (int)pKF->mvKeys.size() < knl || (int)pKF->mvKeysRight.size() < n - knl)
        throw std::logic_error("SearchByBoW: a keyframe's tables do not hold NLeft + NRight rows");
      pli_detail::appendNodes(T, pKF->mFeatVec, n, "SearchByBoW: pKF->mFeatVec");
      pli_detail::appendDescriptors(T, pKF->mDescriptors, n);
      for (int i = 0; i < n; ++i) {
        MapPointT* pMP = kfPoints[k][i];
        T.valid.push_back(pMP && !pMP->isBad() ? 1 : 0);
        T.angle.push_back(i < knl ? pKF->mvKeys[i].angle : pKF->mvKeysRight[i - knl].angle);
      }
    }
    std::vector<int> matches;
    std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("SearchByBoW");
    if (nl != -1)
      fe->searchByBoWTwoCameras(nkf, T.off.data(), T.desc.data(), T.angle.data(), T.node.data(), T.valid.data(), TF.desc.data(),
                                fAngle.data(), TF.node.data(), nf, nl, this->mfNNratio, this->mbCheckOrientation, matches, vnmatches);
    else
      fe->searchByBoW(nkf, T.off.data(), T.desc.data(), T.angle.data(), T.node.data(), T.valid.data(), TF.desc.data(), fAngle.data(),
                      TF.node.data(), nf, this->mfNNratio, this->mbCheckOrientation, matches, vnmatches);
    vvpMapPointMatches.assign((size_t)nkf, std::vector<MapPointT*>((size_t)nf, static_cast<MapPointT*>(nullptr)));
    pli_detail::forEachMatch(matches, nkf, nf, [&](int k, int i, int j) { vvpMapPointMatches[k][i] = kfPoints[k][j]; });
  }

  // ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12), ORBmatcher.cc:823-963
  // (LoopClosing.cc:533), with the two-camera text: for a keyframe with NLeft != -1 a feature idx >= mvKeysUn.size() is skipped, on
  // either side (the two `continue`s at :858-860 and :878-880), and the angles of the others come from mvKeysUn (:915).  The skipped
  // rows enter pli_search_by_bow_kf with valid = 0 and angle 0, which is what the entry's valid tables express; the device call is
  // the base's.  vpMatches12 has GetMapPointMatches().size() entries.  Keyframes with NLeft == -1 are gathered as the base gathers
  // them, and a call in which every keyframe is such a one goes to the base.
  template <class KeyFrameT>
  int SearchByBoW(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12) {
    std::vector<std::vector<MapPointT*>> matches;
    std::vector<int> nmatches;
    SearchByBoW(pKF1, std::vector<KeyFrameT*>(1, pKF2), matches, nmatches);
    vpMatches12.swap(matches[0]);
    return nmatches[0];
  }

  // (not in the reference) The same for every keyframe of vpKF2 in ONE device call, as the base's batch form.
  template <class KeyFrameT>
  void SearchByBoW(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpKF2, std::vector<std::vector<MapPointT*>>& vvpMatches12,
                   std::vector<int>& vnmatches) {
    bool anyTwo = pKF1->NLeft != -1;
    for (KeyFrameT* pKF2 : vpKF2) anyTwo = anyTwo || pKF2->NLeft != -1;
    if (!anyTwo) {
      Base::SearchByBoW(pKF1, vpKF2, vvpMatches12, vnmatches);
      return;
    }
    typedef typename Base::BowTable BowTable;
    auto gather = [](KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const char* what, BowTable& T) {
      if (pKF->NLeft == -1) {
        Base::bowGatherKeyFrame(pKF, vpMapPoints, what, T);
        return;
      }
      const int n = pKF->N, nun = (int)std::min(pKF->mvKeysUn.size(), (size_t)n);
      if ((int)vpMapPoints.size() < n || pKF->mDescriptors.rows < n)
        throw std::logic_error("SearchByBoW: a keyframe's tables do not hold N rows");
      pli_detail::appendNodes(T, pKF->mFeatVec, n, what);
      pli_detail::appendDescriptors(T, pKF->mDescriptors, n);
      for (int i = 0; i < n; ++i) {
        MapPointT* pMP = i < nun ? vpMapPoints[i] : nullptr;           // idx >= mvKeysUn.size(): :858-860, :878-880
        T.valid.push_back(pMP && !pMP->isBad() ? 1 : 0);
        T.angle.push_back(i < nun ? pKF->mvKeysUn[i].angle : 0.f);     // :915
      }
    };
    const int nkf = (int)vpKF2.size(), n1 = pKF1->N;
    BowTable T1, T2;
    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
    gather(pKF1, vpMapPoints1, "SearchByBoW: pKF1->mFeatVec", T1);
    std::vector<std::vector<MapPointT*>> kfPoints((size_t)nkf);
    for (int k = 0; k < nkf; ++k) {
      kfPoints[k] = vpKF2[k]->GetMapPointMatches();
      gather(vpKF2[k], kfPoints[k], "SearchByBoW: pKF2->mFeatVec", T2);
    }
    std::vector<int> matches;
    pli_detail::deviceContext("SearchByBoW")->searchByBoWKF(T1.desc.data(), T1.angle.data(), T1.node.data(), T1.valid.data(), n1, nkf,
                                                           T2.off.data(), T2.desc.data(), T2.angle.data(), T2.node.data(),
                                                           T2.valid.data(), this->mfNNratio, this->mbCheckOrientation, matches,
                                                           vnmatches);
    vvpMatches12.assign((size_t)nkf, std::vector<MapPointT*>(vpMapPoints1.size(), static_cast<MapPointT*>(nullptr)));
    pli_detail::forEachMatch(matches, nkf, n1, [&](int k, int i, int j) { vvpMatches12[k][i] = kfPoints[k][j]; });   // :910
  }

 private:
  template <class KeyFrameT>
  static void kb8Cameras(KeyFrameT* pKF, pli_kb8_camera cam[2]) { pli_detail::kb8Cameras(pKF, cam); }

  // What the two Fuse forms share.  sides: 1 = the left camera of every target, 2 = the right one, 3 = both, left then right;
  // nFused has one entry per replayed (keyframe, side).
  template <class KeyFrameT>
  void fuseTwoCameras(const std::vector<KeyFrameT*>& vpTargetKFs, const std::vector<MapPointT*>& vpMapPoints, const float th,
                      const int sides, std::vector<int>& nFused, int* pnResearch) {
    const int nkf = (int)vpTargetKFs.size(), nmp = (int)vpMapPoints.size(), per = sides == 3 ? 2 : 1;
    nFused.assign((size_t)nkf * per, 0);
    if (pnResearch) *pnResearch = 0;
    if (nkf == 0) return;
    struct Table : pli_detail::KfTable {
      std::vector<pli_keypoint> kp;
      std::vector<int32_t> nleft;
      std::vector<float> pose;
    } T;
    pli_kb8_camera cam[2];
    kb8Cameras(vpTargetKFs[0], cam);
    KeyFrameT* first = vpTargetKFs[0];
    const float bounds[4] = {(float)first->mnMinX, (float)first->mnMaxX, (float)first->mnMinY, (float)first->mnMaxY};
    for (KeyFrameT* pKF : vpTargetKFs) {
      const int n = pKF->N, nl = pKF->NLeft;
      if (nl < 0 || nl > n || (int)pKF->mvKeys.size() < nl || (int)pKF->mvKeysRight.size() < n - nl || pKF->mDescriptors.rows < n)
        throw std::logic_error("Fuse: a keyframe's tables do not hold NLeft + NRight rows");
      for (size_t i = 0; i < pKF->mvuRight.size(); ++i)
        if (pKF->mvuRight[i] >= 0)
          throw std::logic_error("Fuse: a keyframe of two cameras with mvuRight >= 0 (the reference reads mvuRight out of range there)");
      pli_kb8_camera own[2];
      kb8Cameras(pKF, own);
      const float b[4] = {(float)pKF->mnMinX, (float)pKF->mnMaxX, (float)pKF->mnMinY, (float)pKF->mnMaxY};
      if (std::memcmp(own, cam, sizeof(own)) != 0 || std::memcmp(b, bounds, sizeof(b)) != 0)
        throw std::logic_error("Fuse: the target keyframes of one call must share the cameras and the image bounds");
      pli_detail::appendDescriptors(T, pKF->mDescriptors, n);
      for (int i = 0; i < n; ++i) T.kp.push_back(pli_detail::keypoint(i < nl ? pKF->mvKeys[i] : pKF->mvKeysRight[i - nl]));   // :1524-1526
      T.nleft.push_back(nl);
      float pose[30];
      pli_detail::fusePosesTwoCameras(pKF, pose);                                                   // :1404-1417
      T.pose.insert(T.pose.end(), pose, pose + 30);
    }
    std::vector<pli_fuse_point> pts(nmp);
    std::vector<uint8_t> desc((size_t)nmp * 32, 0), skip((size_t)nkf * 2 * nmp, 0);
    for (int i = 0; i < nmp; ++i) {
      MapPointT* pMP = vpMapPoints[i];
      pts[i] = Base::fusePoint(pMP);
      if (!pts[i].valid) continue;
      std::memcpy(&desc[(size_t)i * 32], pMP->GetDescriptor().template ptr<uint8_t>(), 32);
      for (int k = 0; k < nkf; ++k)
        skip[((size_t)k * 2) * nmp + i] = skip[((size_t)k * 2 + 1) * nmp + i] = pMP->IsInKeyFrame(vpTargetKFs[k]) ? 1 : 0;
    }
    std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("Fuse");
    const std::vector<float>& levelRatio = this->fuseLevelRatio(first);
    std::vector<int> all;
    fe->fuseSearchTwoCameras(pts.data(), desc.data(), nmp, nkf, T.off.data(), T.nleft.data(), T.kp.data(), T.desc.data(), T.pose.data(),
                             skip.data(), cam[0], cam[1], bounds, th, levelRatio, sides, all);
    // the replayed views: (keyframe, side) for every side asked for, in the reference's order
    std::vector<KeyFrameT*> viewKF;
    std::vector<int> viewRow;                                                // the view's row of `all` (keyframe * 2 + side)
    for (int k = 0; k < nkf; ++k)
      for (int side = 0; side < 2; ++side)
        if ((sides >> side) & 1) { viewKF.push_back(vpTargetKFs[k]); viewRow.push_back(k * 2 + side); }
    std::vector<int> best(viewKF.size() * (size_t)nmp);
    for (size_t v = 0; v < viewKF.size(); ++v)
      std::copy(all.begin() + (size_t)viewRow[v] * nmp, all.begin() + ((size_t)viewRow[v] + 1) * nmp, best.begin() + v * nmp);
    this->fuseReplay(viewKF, vpMapPoints, best, nFused, pnResearch,
                     [&](int v, const std::vector<int>& which, const std::vector<pli_fuse_point>& p2, const std::vector<uint8_t>& d2) {
                       const int k0 = viewRow[v] / 2;                        // the keyframes k0..end, the same sides
                       std::vector<int32_t> off2(T.off.begin() + k0, T.off.end());
                       for (size_t j = off2.size(); j-- > 0;) off2[j] -= off2[0];
                       const size_t row0 = (size_t)T.off[k0];
                       std::vector<int> b2;
                       fe->fuseSearchTwoCameras(p2.data(), d2.data(), (int)which.size(), nkf - k0, off2.data(), T.nleft.data() + k0,
                                                T.kp.data() + row0, T.desc.data() + row0 * 32, T.pose.data() + (size_t)k0 * 30, nullptr,
                                                cam[0], cam[1], bounds, th, levelRatio, sides, b2);
                       for (size_t vv = (size_t)v; vv < viewKF.size(); ++vv)
                         for (size_t j = 0; j < which.size(); ++j)
                           best[vv * nmp + which[j]] = b2[(size_t)(viewRow[vv] - 2 * k0) * which.size() + j];
                     });
  }

  // the two cameras of a frame as the library's tables: mvKeys / mvKeysRight, the two halves of mDescriptors, and per slot
  // "holds a map point with observations" (:2036-2038, :2111-2113; :89-91, :169-171)
  struct Tables {
    std::vector<pli_keypoint> kpL, kpR;
    std::vector<uint8_t> occL, occR;
    const uint8_t* descL = nullptr;
    const uint8_t* descR = nullptr;
    explicit Tables(FrameT& F) {
      const int nL = F.Nleft, nR = F.Nright;
      if (nL < 0 || nR < 0 || (int)F.mvKeys.size() < nL || (int)F.mvKeysRight.size() < nR || F.mDescriptors.rows < nL + nR ||
          (int)F.mvpMapPoints.size() < nL + nR)
        throw std::logic_error("PliORBmatcherTwoCameras: the frame's tables do not hold Nleft + Nright rows");
      kpL.resize((size_t)nL); kpR.resize((size_t)nR);
      occL.assign((size_t)nL + 1, 0); occR.assign((size_t)nR + 1, 0);
      for (int k = 0; k < nL; ++k) {
        kpL[k] = pli_detail::keypoint(F.mvKeys[k]);
        if (F.mvpMapPoints[k] && F.mvpMapPoints[k]->Observations() > 0) occL[k] = 1;
      }
      for (int k = 0; k < nR; ++k) {
        kpR[k] = pli_detail::keypoint(F.mvKeysRight[k]);
        if (F.mvpMapPoints[k + nL] && F.mvpMapPoints[k + nL]->Observations() > 0) occR[k] = 1;
      }
      if (nL > 0) descL = F.mDescriptors.template ptr<uint8_t>(0);
      if (nR > 0) descR = F.mDescriptors.template ptr<uint8_t>(nL);
    }
  };
};

}  // namespace ORB_SLAM3
