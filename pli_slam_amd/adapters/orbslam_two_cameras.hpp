// The two SearchByProjection forms of ORB_SLAM3::ORBmatcher that run on every tracked frame, for a frame of two cameras
// (Frame::Nleft != -1, the fisheye-stereo rig): a matcher that is PliORBmatcher in everything else.
//
//   inside the PLI-SLAM tree:  using ORBmatcher = ORB_SLAM3::PliORBmatcherTwoCameras<Frame, MapPoint>;
//
// PliORBmatcher itself keeps refusing such frames (its users' Frame types need no second-camera members); this class hides
// exactly two of its members and forwards both to it when the frame has one camera.
#pragma once
#include "orbslam_adapters.hpp"

namespace ORB_SLAM3 {

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

 private:
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
