// The body of the reference's two single-camera Frame constructors for a pinhole camera with distortion coefficients — monocular
// (src/Frame.cc:334-448) and RGB-D (:231-331) — on one call of pli_frame_extract_single (include/pli_frontend.h):
//
//   ExtractORB(0, imGray, x0, x1); ExtractLine(0, imGray);        :360-361 / :258-259   -> mvKeys, mDescriptors, monoLeft,
//                                                                                          mvKeys_Line, mDescriptors_Line
//   if (mvKeys.empty()) return;                                    :372-373 / :270-271   -> extract() returns false
//   UndistortKeyPoints();                                          :872-905              -> mvKeysUn
//   UndistortKeyLines();                                           :907-945              -> mvKeysUn_Line
//   ComputeStereoFromRGBD(imDepth) / "no stereo information"       :1309-1330 / :384-385 -> mvuRight, mvDepth
//   ComputeImageBounds(imGray) under mbInitialComputations         :947-974              -> mnMinX .. mnMaxY
//   AssignFeaturesToGrid()                                         :451-482              -> mGrid
//
// INTEGRATION.md 2 shows the constructor edit.  FrameT is the reference's Frame (or a stand-in with the members named above: the host
// test runs it on a stub, tests/cpp/single_frame_harness.cpp); the key line type is whatever mvKeys_Line holds.  Header only.
#pragma once
#include <opencv2/core/core.hpp>
#include <cstring>
#include <stdexcept>
#include <type_traits>
#include <vector>
#include "pli_cpp.hpp"

namespace ORB_SLAM3 {

template <class FrameT>
class PliSingleCameraFrame {
 public:
  // K: 3x3 CV_32F (mK / Pinhole::toK()); distCoef: mDistCoef, 4 or 5 rows of CV_32F (k1, k2, p1, p2[, k3]).  Sets the context's
  // camera; call it again after a change of the calibration (where the reference sets mbInitialComputations again).
  PliSingleCameraFrame(pli::Frontend& fe, const cv::Mat& K, const cv::Mat& distCoef) : fe_(fe) {
    if (K.rows != 3 || K.cols != 3 || K.type() != CV_32F) throw std::invalid_argument("PliSingleCameraFrame: K must be 3x3 CV_32F");
    const int nc = distCoef.rows * distCoef.cols;
    if (distCoef.type() != CV_32F || (nc != 4 && nc != 5)) throw std::invalid_argument("PliSingleCameraFrame: mDistCoef must hold 4 or 5 floats");
    cam_.fx = K.at<float>(0, 0); cam_.fy = K.at<float>(1, 1); cam_.cx = K.at<float>(0, 2); cam_.cy = K.at<float>(1, 2);
    cam_.k1 = distCoef.at<float>(0); cam_.k2 = distCoef.at<float>(1); cam_.p1 = distCoef.at<float>(2); cam_.p2 = distCoef.at<float>(3);
    cam_.k3 = nc == 5 ? distCoef.at<float>(4) : 0.0f;
    pli::check(pli_set_pinhole_distortion(fe_.handle(), &cam_, bounds_));
  }

  const float* bounds() const { return bounds_; }       // mnMinX, mnMaxX, mnMinY, mnMaxY

  // The constructor's front-end.  imDepth: the RGB-D constructor's depth image (CV_32F), or null for the monocular one; x0, x1: the
  // lapping area ExtractORB passes (:360 0, 1000; :258 0, 0).  false: mvKeys is empty and the constructor returns (:270-271,
  // :372-373) — the extractors' outputs are filled, nothing behind them is touched.
  bool extract(FrameT& F, const cv::Mat& imGray, const cv::Mat* imDepth, int x0, int x1) {
    if (imGray.empty() || imGray.type() != CV_8UC1) throw std::invalid_argument("PliSingleCameraFrame: 8-bit single-channel image expected");
    if (imDepth && (imDepth->type() != CV_32F || imDepth->rows != imGray.rows || imDepth->cols != imGray.cols))
      throw std::invalid_argument("PliSingleCameraFrame: the depth image must be CV_32F of the image's size");
    const pli::ImageView im{imGray.data, imGray.cols, imGray.rows, (int64_t)imGray.step, 1};
    const pli::DepthView dv{imDepth ? imDepth->data : nullptr, imGray.cols, imGray.rows, imDepth ? (int64_t)imDepth->step : 0, PLI_DEPTH_F32};
    return extractRaw(F, im, imDepth ? &dv : nullptr, x0, x1);
  }

  // ... on the images as Tracking::GrabImageRGBD / GrabImageMonocular RECEIVE them (adapters/tracking_grab.hpp: PliGrabImage has set
  // the context's image and depth formats to what the views hold): a colour image of 3 or 4 bytes per pixel, a raw uint16 or
  // float depth map.  Pointers and strides go to the library as they are; the image's stride stays in bytes, the depth map's is
  // handed over in elements of its type.  The views are the caller's word: what extract() checks about its Mats is not checked here.
  bool extractRaw(FrameT& F, const pli::ImageView& im, const pli::DepthView* depth, int x0, int x1) {
    const pli_table_layout& Y = fe_.layout();
    if (depth) fe_.setStereoCamera(F.mbf, cam_.fx);            // ComputeStereoFromRGBD divides mbf (:1327)
    record_.resize((size_t)Y.record_bytes);
    kpUn_.resize((size_t)Y.kp_cap * 2);
    klUn_.resize((size_t)Y.kl_cap * 4);
    cell_.resize((size_t)Y.kp_cap);
    int32_t nMono = 0;
    const int64_t depthElem = depth && depth->type == PLI_DEPTH_U16 ? (int64_t)sizeof(uint16_t) : (int64_t)sizeof(float);
    pli::check(pli_frame_extract_single(fe_.handle(), im.data, im.cols, im.rows, im.step, x0, x1,
                                        depth ? reinterpret_cast<const float*>(depth->data) : nullptr,
                                        depth ? depth->step / depthElem : 0, record_.data(), kpUn_.data(), klUn_.data(),
                                        cell_.data(), &nMono));
    const uint8_t* rec = record_.data();
    const int32_t* counts = reinterpret_cast<const int32_t*>(rec + Y.off_counts);
    const int N = counts[0], Nl = counts[2];

    // ExtractORB (:484-491): monoLeft = (*mpORBextractorLeft)(im, cv::Mat(), mvKeys, mDescriptors, vLapping)
    const pli_keypoint* kp = reinterpret_cast<const pli_keypoint*>(rec + Y.off_kp[0]);
    F.mvKeys.resize(N);
    for (int i = 0; i < N; ++i) F.mvKeys[i] = cv::KeyPoint(kp[i].x, kp[i].y, kp[i].size, kp[i].angle, kp[i].response, kp[i].octave, -1);
    if (N == 0) {
      F.mDescriptors.release();                                // ORBextractor.cc:1083-1084
    } else {
      F.mDescriptors.create(N, 32, CV_8UC1);
      for (int i = 0; i < N; ++i) std::memcpy(F.mDescriptors.ptr(i), rec + Y.off_desc[0] + (size_t)i * 32, 32);
    }
    F.monoLeft = nMono;
    // ExtractLine (:493-497)
    typedef typename std::decay<decltype(F.mvKeys_Line[0])>::type KeyLineT;
    const pli_keyline* kl = reinterpret_cast<const pli_keyline*>(rec + Y.off_kl[0]);
    F.mvKeys_Line.resize(Nl);
    for (int i = 0; i < Nl; ++i) {
      KeyLineT& k = F.mvKeys_Line[i];
      const pli_keyline& s = kl[i];
      k.angle = s.angle; k.class_id = s.class_id; k.octave = s.octave; k.pt = cv::Point2f(s.pt_x, s.pt_y);
      k.response = s.response; k.size = s.size;
      k.startPointX = s.startPointX; k.startPointY = s.startPointY; k.endPointX = s.endPointX; k.endPointY = s.endPointY;
      k.sPointInOctaveX = s.sPointInOctaveX; k.sPointInOctaveY = s.sPointInOctaveY;
      k.ePointInOctaveX = s.ePointInOctaveX; k.ePointInOctaveY = s.ePointInOctaveY;
      k.lineLength = s.lineLength; k.numOfPixels = s.numOfPixels;
    }
    if (Nl > 0) {                                              // (the reference leaves descriptors_line untouched when no line survives)
      F.mDescriptors_Line.create(Nl, 32, CV_8UC1);
      for (int i = 0; i < Nl; ++i) std::memcpy(F.mDescriptors_Line.ptr(i), rec + Y.off_ldesc[0] + (size_t)i * 32, 32);
    }
    if (F.mvKeys.empty()) return false;

    // UndistortKeyPoints (:872-905): a copy of mvKeys with pt replaced (:899-902); with k1 == 0 the device returns mvKeys' own pt
    F.mvKeysUn.resize(N);
    for (int i = 0; i < N; ++i) {
      cv::KeyPoint k = F.mvKeys[i];
      k.pt.x = kpUn_[2 * (size_t)i];
      k.pt.y = kpUn_[2 * (size_t)i + 1];
      F.mvKeysUn[i] = k;
    }
    // UndistortKeyLines (:907-945): with k1 == 0 a copy of mvKeys_Line (:911), otherwise fresh key lines whose four end point
    // coordinates alone are set (:937-944)
    if (cam_.k1 == 0.0f) {
      F.mvKeysUn_Line = F.mvKeys_Line;
    } else {
      F.mvKeysUn_Line.clear();
      F.mvKeysUn_Line.resize(Nl);
      for (int i = 0; i < Nl; ++i) {
        KeyLineT& k = F.mvKeysUn_Line[i];
        k.startPointX = klUn_[4 * (size_t)i]; k.startPointY = klUn_[4 * (size_t)i + 1];
        k.endPointX = klUn_[4 * (size_t)i + 2]; k.endPointY = klUn_[4 * (size_t)i + 3];
      }
    }
    // ComputeStereoFromRGBD (:1309-1330), or mvuRight = mvDepth = vector<float>(N, -1) (:384-385)
    const float* ur = reinterpret_cast<const float*>(rec + Y.off_uright);
    const float* dp = reinterpret_cast<const float*>(rec + Y.off_depth);
    F.mvuRight.assign(ur, ur + N);
    F.mvDepth.assign(dp, dp + N);
    // ComputeImageBounds (:947-974), on the first Frame only; the rest of that block (:297-307, :402-412) stays in the constructor
    if (FrameT::mbInitialComputations) {
      FrameT::mnMinX = bounds_[0]; FrameT::mnMaxX = bounds_[1]; FrameT::mnMinY = bounds_[2]; FrameT::mnMaxY = bounds_[3];
    }
    // AssignFeaturesToGrid (:451-482) on mvKeysUn: ascending i is push_back order
    const int nReserve = (int)(0.5f * N / (64 * 48));
    for (int i = 0; i < 64; ++i)
      for (int j = 0; j < 48; ++j) F.mGrid[i][j].reserve(nReserve);
    for (int i = 0; i < N; ++i) {
      const int c = cell_[i];
      if (c >= 0) F.mGrid[c / 48][c % 48].push_back(i);
    }
    return true;
  }

 private:
  pli::Frontend& fe_;
  pli_pinhole_distortion cam_{};
  float bounds_[4] = {0, 0, 0, 0};
  std::vector<uint8_t> record_;
  std::vector<float> kpUn_, klUn_;
  std::vector<int32_t> cell_;
};

}  // namespace ORB_SLAM3
