// The head of the reference's three Tracking::GrabImage* functions (src/Tracking.cc) without a host pass over the frame:
//
//   cvtColor(mImGray, mImGray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY)      :889-914 (both eyes, the branch chosen by
//                                                                                             the LEFT image), :964-977, :1014-1027
//   if ((fabs(mDepthMapFactor - 1.0f) > 1e-5) || imDepth.type() != CV_32F)
//     imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor);                                    :979-980
//
// PliGrabImage picks the context's image format (pli_set_image_format) from channels() and mbRGB, and its depth format
// (pli_set_depth_format) from the depth map's type and mDepthMapFactor, as those lines do, calls the two setters only when something
// changed, and hands out plain views of the Mats as they came in.  The library then converts in its ingest kernel and scales the
// depth at the keypoints (include/pli_frontend.h).  INTEGRATION.md 2 shows the edit of GrabImageRGBD.
//
// The core works on plain numbers (channels, OpenCV's depth code, the factor); the cv::Mat reading is a template that uses only
// channels(), depth(), data, cols, rows, step, so that a host test can run it on a Mat-like struct of its own
// (tests/cpp/grab_image_harness.cpp).  Header only.
#pragma once
#include <cmath>
#include <stdexcept>
#include "pli_cpp.hpp"

namespace ORB_SLAM3 {

class PliGrabImage {
 public:
  // OpenCV's depth codes (CV_MAT_DEPTH of a type; cv::Mat::depth()) of what GrabImage* can be handed
  enum { kDepth8U = 0, kDepth16U = 2, kDepth32F = 5 };

  // rgb: Tracking::mbRGB ("Camera.RGB"); depthMapFactor: Tracking::mDepthMapFactor AS TRACKING HOLDS IT, the reciprocal of the
  // settings' "DepthMapFactor" (Tracking.cc: mDepthMapFactor = 1.0f / mDepthMapFactor), 1 for the sensors without a depth map
  PliGrabImage(pli::Frontend& fe, bool rgb, float depthMapFactor = 1.0f) : fe_(fe), rgb_(rgb), factor_(depthMapFactor) {}

  // :889-914 and its two copies: 1 channel passes through, 3 and 4 are converted in the order mbRGB says
  static pli_image_format formatOf(int channels, bool rgb) {
    switch (channels) {
      case 1: return PLI_IMAGE_GRAY8;
      case 3: return rgb ? PLI_IMAGE_RGB8 : PLI_IMAGE_BGR8;
      case 4: return rgb ? PLI_IMAGE_RGBA8 : PLI_IMAGE_BGRA8;
      default: throw std::invalid_argument("PliGrabImage: an image of 1, 3 or 4 channels expected");
    }
  }

  // :979-980: a CV_32F map whose factor is within 1e-5 of 1 is left alone (scale 1.0f: the library hands its bits through), every
  // other one is converted with the factor — a CV_16U map also with factor 1
  static void depthFormatOf(int cvDepth, float factor, pli_depth_type* type, float* scale) {
    if (cvDepth != kDepth32F && cvDepth != kDepth16U) throw std::invalid_argument("PliGrabImage: a CV_32F or CV_16U depth map expected");
    const bool convert = (std::fabs(factor - 1.0f) > 1e-5) || cvDepth != kDepth32F;
    *type = cvDepth == kDepth16U ? PLI_DEPTH_U16 : PLI_DEPTH_F32;
    *scale = convert ? factor : 1.0f;
  }

  // the two settings, sent to the context when they differ from what it was last sent (a fresh context: gray, CV_32F x 1)
  void useImage(int channels) {
    const pli_image_format f = formatOf(channels, rgb_);
    if (f == format_) return;
    fe_.setImageFormat(f);
    format_ = f;
  }
  void useDepth(int cvDepth) {
    pli_depth_type t;
    float s;
    depthFormatOf(cvDepth, factor_, &t, &s);
    if (t == depthType_ && s == depthScale_) return;
    fe_.setDepthFormat(t, s);
    depthType_ = t;
    depthScale_ = s;
  }

  // mImGray = im; cvtColor(...): the image of GrabImageRGBD / GrabImageMonocular, or the LEFT one of GrabImageStereo, whose channel
  // count chooses the branch for both eyes (:889, :902)
  template <class MatT>
  pli::ImageView image(const MatT& im) {
    if (im.depth() != kDepth8U) throw std::invalid_argument("PliGrabImage: an 8-bit image expected");
    useImage(im.channels());
    return view(im);
  }
  // ... and the right one: read in the format the left image chose, as the reference converts it (:894, :899, :907, :912) — which
  // presumes the same channel count
  template <class MatT>
  pli::ImageView imageRight(const MatT& im) const {
    if (im.depth() != kDepth8U || channelsOf(format_) != im.channels())
      throw std::invalid_argument("PliGrabImage: the right image must have the left image's type");
    return view(im);
  }
  // imDepth = imD; convertTo(...)
  template <class MatT>
  pli::DepthView depth(const MatT& imD) {
    if (imD.channels() != 1) throw std::invalid_argument("PliGrabImage: a single-channel depth map expected");
    useDepth(imD.depth());
    return pli::DepthView{imD.data, imD.cols, imD.rows, (int64_t)imD.step, depthType_};
  }

  pli_image_format format() const { return format_; }
  pli_depth_type depthType() const { return depthType_; }
  float depthScale() const { return depthScale_; }

 private:
  static int channelsOf(pli_image_format f) { return f == PLI_IMAGE_GRAY8 ? 1 : (f == PLI_IMAGE_RGB8 || f == PLI_IMAGE_BGR8) ? 3 : 4; }
  template <class MatT>
  static pli::ImageView view(const MatT& im) { return pli::ImageView{im.data, im.cols, im.rows, (int64_t)im.step, im.channels()}; }

  pli::Frontend& fe_;
  bool rgb_;
  float factor_;
  pli_image_format format_ = PLI_IMAGE_GRAY8;
  pli_depth_type depthType_ = PLI_DEPTH_F32;
  float depthScale_ = 1.0f;
};

}  // namespace ORB_SLAM3
