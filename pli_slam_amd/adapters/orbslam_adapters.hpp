// Drop-in shims with the reference's EXACT signatures (build inside the PLI-SLAM tree, where OpenCV 3 exists):
//
//   ORB_SLAM3::ORBextractor   include/ORBextractor.h:46-115   ctor (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST),
//                                                             functor, scale getters, mvImagePyramid
//   ORB_SLAM3::Lineextractor  include/LineExtractor.h:41-74   both constructors, functor
//   ORB_SLAM3::match          include/LineMatcher.h:63        match(desc1, desc2, nnr, matches_12)
//   ORB_SLAM3::ORBmatcher::DescriptorDistance                 include/ORBmatcher.h:42  (host inline: 32 bytes never go to the GPU)
//   ORB_SLAM3::ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono, match12)   include/ORBmatcher.h:51,
//                                                             src/ORBmatcher.cc:2179-2323 (projection on the host with the
//                                                             reference's own cv::Mat expressions, window search on the GPU)
//   ORB_SLAM3::ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches)   include/ORBmatcher.h, src/ORBmatcher.cc:269-470 (F.Nleft == -1;
//                                                             + a batch form for Tracking::Relocalization's candidate loop)
//   ORB_SLAM3::ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse)   include/ORBmatcher.h,
//                                                             src/ORBmatcher.cc:965-1206 (no second cameras; + a batch form for
//                                                             LocalMapping::CreateNewMapPoints' neighbour loop)
//   ORB_SLAM3::ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)   include/ORBmatcher.h,
//                                                             src/ORBmatcher.cc:1399-1609, :1611-1733 (no second cameras; + a batch
//                                                             form for LocalMapping::SearchInNeighbors' loop over target keyframes)
//   ORB_SLAM3::ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) and (pKF, Scw, vpPoints, vpPointsKFs,
//                                                             vpMatched, vpMatchedKF, th, ratioHamming)   include/ORBmatcher.h,
//                                                             src/ORBmatcher.cc:473-586, :588-704 (no second cameras; + a batch
//                                                             form for LoopClosing's loop over covisible keyframes)
//   ORB_SLAM3::ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)   include/ORBmatcher.h,
//                                                             src/ORBmatcher.cc:2325-2447 (relocalisation, Tracking.cc:4290 and :4304;
//                                                             no second cameras; + a batch form over the candidate keyframes)
//
// Frame.cc / Tracking.cc keep calling these names unchanged; INTEGRATION.md lists the edits (swap the headers).
//
// How four independent extractor objects end up on ONE device context (the stereo matchers need both eyes' pyramids and
// tables on the device): extractors register in construction order.  Tracking.cc:87-98,743-749 builds
//   mpORBextractorLeft, mpLineextractorLeft, mpORBextractorRight, mpLineextractorRight, mpIniORBextractor, mpIniLineextractor;
// the second ORBextractor / Lineextractor constructed with the SAME parameters as an existing one becomes the right eye of
// that one's group, different parameters (the 2x-feature initial extractors) open a new group; the k-th ORB group and the
// k-th line group share a context, created lazily at the first operator() call for the size of the image it is given.
#pragma once
#if !__has_include(<opencv2/core/core.hpp>)
#error "orbslam_adapters.hpp needs OpenCV 3 (it is meant to be compiled inside the PLI-SLAM tree)"
#endif
#include <opencv2/core/core.hpp>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "pli_cpp.hpp"
#ifndef PLI_ADAPTER_NO_KEYLINE_HEADER
#include "line_descriptor_custom.hpp"   // cv::line_descriptor::KeyLine (Thirdparty/line_descriptor)
#endif

namespace ORB_SLAM3 {

namespace pli_detail {

struct OrbParams {
  int nfeatures, nlevels, iniThFAST, minThFAST;
  float scaleFactor;
  bool operator==(const OrbParams& o) const {
    return nfeatures == o.nfeatures && nlevels == o.nlevels && iniThFAST == o.iniThFAST && minThFAST == o.minThFAST && scaleFactor == o.scaleFactor;
  }
};
struct LineParams {
  int lsd_nfeatures, lsd_refine, lsd_n_bins;
  double min_line_length, lsd_scale, lsd_sigma_scale, lsd_quant, lsd_ang_th, lsd_log_eps, lsd_density_th;
  bool bFLD;
  bool operator==(const LineParams& o) const {
    return lsd_nfeatures == o.lsd_nfeatures && lsd_refine == o.lsd_refine && lsd_n_bins == o.lsd_n_bins &&
           min_line_length == o.min_line_length && lsd_scale == o.lsd_scale && lsd_sigma_scale == o.lsd_sigma_scale &&
           lsd_quant == o.lsd_quant && lsd_ang_th == o.lsd_ang_th && lsd_log_eps == o.lsd_log_eps &&
           lsd_density_th == o.lsd_density_th && bFLD == o.bFLD;
  }
};

// Frame fusion.  Frame::Frame calls the four extractors of a group from four threads at the same time (Frame.cc:128-135).  When all
// four calls of a frame are in flight together they are funnelled into ONE submission (pli_frame_extract: both eyes, points and
// lines, and the two stereo matchers on top), and every thread takes its part from the frame's record: 2.7 ms per Frame instead of
// 6.5 ms for four calls that queue behind the context's lock.  The results are the same bytes either way
// (tests/test_cpp_dropin.py compares the two).
//
// A call that waits kWaitMs without its three partners withdraws and takes the per-call path — ONE frame is unfused, the next frame
// tries again (a late thread on a host busy with LocalMapping / LoopClosing / the viewer must not cost every later Frame the fused
// path).  Misses are counted per FRAME, not per call: the timed-out calls of one Frame — three waiters and the late-comer, or the
// four calls of an integrator that calls the extractors one after the other — are one miss (a Frame is over when all four kinds
// have timed out, or a kind times out again).  Only kMaxMisses unfused Frames in a row put the fusion to sleep, for kCoolOff calls
// (32 Frames); then ONE Frame probes, and if it does not fuse either the fusion sleeps again at once, twice as long (up to
// kMaxCoolOff calls): a sequential integrator pays the 2 ms waits on 8 Frames once, then on one Frame in 33, 65, 129, 257.  The four calls of a Frame must
// agree: the line extractors must be given the images (pointer, stride, size) the ORB extractors of the same eye were given, as
// Frame.cc:128-135 does; if they differ (a ROI, a preprocessed copy) nobody is fused and every caller extracts from ITS image.
// stats(): how many Frames went which way.
struct FrameFusion {
  static constexpr int kOrbL = 0, kOrbR = 1, kLineL = 2, kLineR = 3;
  static constexpr int kWaitMs = 2, kMaxMisses = 8, kCoolOff = 128, kMaxCoolOff = 1024;
  // (PLI_FUSION_WAIT_MS: the rendezvous wait for test runs under a sanitizer, where a thread start alone takes milliseconds)
  static int waitMs() {
    static const int ms = [] { const char* e = std::getenv("PLI_FUSION_WAIT_MS"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : kWaitMs; }();
    return ms;
  }
  struct Stats { uint64_t fused = 0, unfusedCalls = 0, timeouts = 0, mismatched = 0, sleeps = 0, missedFrames = 0; };
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  int misses = 0;                            // Frames that ended in timeouts since the last fused frame
  int missKinds = 0;                         // kinds (bit per extractor) that have timed out in the Frame being counted
  int asleep = 0;                            // calls left to skip before the next probe
  int coolOff = kCoolOff;                    // length of the next sleep (doubles while the probes keep failing)
  uint64_t gen = 0;                          // frames collected so far (fused or released)
  bool lastFused = false;                    // outcome of generation gen - 1
  const uint8_t* img[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t stride[4] = {0, 0, 0, 0};
  int iw[4] = {0, 0, 0, 0}, ih[4] = {0, 0, 0, 0};
  // table record of the last fused frame (pli_table_layout).  Every caller of that frame takes a reference under the lock and reads
  // its part outside it: a Frame that (against the protocol) starts before the previous one's callers have copied their parts
  // gets a record of its own, it cannot overwrite theirs
  std::shared_ptr<std::vector<uint8_t>> record;
  typedef std::shared_ptr<const std::vector<uint8_t>> RecordRef;
  std::exception_ptr error;                  // what the fused submission threw (every caller of that frame rethrows it)
  Stats st;

  Stats stats() { std::lock_guard<std::mutex> lk(m); return st; }
  // (under the lock) a Frame ended unfused by timeouts
  void missed() {
    ++st.missedFrames;
    if (++misses >= kMaxMisses) {
      // asleep for coolOff calls; the Frame after that is a probe: one more miss and the fusion sleeps again, twice as long
      misses = kMaxMisses - 1;
      asleep = coolOff;
      coolOff = coolOff * 2 > kMaxCoolOff ? kMaxCoolOff : coolOff * 2;
      ++st.sleeps;
    }
  }

  // true: the frame was extracted in one submission and `record` holds it; false: take the per-call path
  bool join(int kind, pli::Frontend& fe, const uint8_t* data, int w, int h, int64_t strideBytes, RecordRef& rec) {
    std::unique_lock<std::mutex> lk(m);
    if (asleep > 0) { --asleep; ++st.unfusedCalls; return false; }
    if (img[kind] != nullptr) { ++st.unfusedCalls; return false; }     // (a second call of the same kind while a frame is collecting: not a Frame)
    img[kind] = data; stride[kind] = strideBytes; iw[kind] = w; ih[kind] = h;
    const uint64_t myGen = gen;
    if (++arrived == 4) {
      error = nullptr;
      const bool agree = img[kLineL] == img[kOrbL] && img[kLineR] == img[kOrbR] && stride[kLineL] == stride[kOrbL] &&
                         stride[kLineR] == stride[kOrbR] && iw[kOrbL] == iw[kOrbR] && ih[kOrbL] == ih[kOrbR] &&
                         iw[kLineL] == iw[kOrbL] && ih[kLineL] == ih[kOrbL] && iw[kLineR] == iw[kOrbL] && ih[kLineR] == ih[kOrbL];
      if (agree) {
        if (!record || record.use_count() > 1) record = std::make_shared<std::vector<uint8_t>>();     // (recycled once its readers are gone)
        try {
          fe.frameExtract(img[kOrbL], img[kOrbR], iw[kOrbL], ih[kOrbL], stride[kOrbL], stride[kOrbR], *record);
        } catch (...) {
          error = std::current_exception();
        }
        ++st.fused;
        misses = 0; missKinds = 0; coolOff = kCoolOff;
      } else {
        ++st.mismatched;
        st.unfusedCalls += 4;
      }
      lastFused = agree;
      arrived = 0;
      for (int k = 0; k < 4; ++k) img[k] = nullptr;
      ++gen;
      cv.notify_all();
    } else if (!cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::milliseconds(waitMs()), [&] { return gen != myGen; })) {
      // (system_clock: pthread_cond_timedwait, which gcc 11's ThreadSanitizer intercepts; the steady-clock wait is pthread_cond_clockwait)
      img[kind] = nullptr;                   // the partners did not come in time: withdraw, this call goes alone
      --arrived;
      ++st.timeouts; ++st.unfusedCalls;
      // one miss per Frame: this kind has timed out already -> that Frame is over and this call opens the next one; all four
      // kinds have timed out -> the Frame is complete
      if (missKinds & (1 << kind)) { missed(); missKinds = 0; }
      missKinds |= 1 << kind;
      if (missKinds == 15) { missed(); missKinds = 0; }
      return false;
    }
    // (one Frame at a time per group: generation myGen's outcome is read before generation myGen + 1 can complete, because that
    // needs this thread's next call)
    if (!lastFused) return false;
    if (error) std::rethrow_exception(error);
    rec = record;
    return true;
  }
};

// One group = the extractors of one Frame constructor: ORB left/right + LSD left/right on one device context per image size.
// orbMask / lineMask: which eye slots (bit 0 = left, bit 1 = right) are held by a living extractor (atomics: operator() reads
// them while pliBind / a destructor may write them under the registry's lock).
struct Group {
  bool hasOrb = false, hasLine = false;
  OrbParams orb{};
  LineParams line{};
  std::atomic<int> orbMask{0}, lineMask{0};
  FrameFusion fusion;
  std::mutex mu;
  std::map<std::pair<int, int>, std::shared_ptr<pli::Frontend>> ctx;     // by image size
  float rigBf = 0.f, rigFx = 0.f;            // the stereo rig (mbf, fx), once a Frame or pliSetStereoCamera has named it

  std::shared_ptr<pli::Frontend> context(int w, int h) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = ctx.find({w, h});
    if (it != ctx.end()) return it->second;
    pli_frontend_config c;
    pli_config_default(&c, w, h);
    if (rigBf > 0 && rigFx > 0) { c.bf = rigBf; c.fx = rigFx; }
    if (hasOrb) {
      c.orb_nfeatures = orb.nfeatures; c.orb_scale_factor = orb.scaleFactor; c.orb_nlevels = orb.nlevels;
      c.orb_ini_th_fast = orb.iniThFAST; c.orb_min_th_fast = orb.minThFAST;
    }
    if (hasLine) {
      c.lsd_nfeatures = line.lsd_nfeatures; c.lsd_refine = line.lsd_refine; c.lsd_n_bins = line.lsd_n_bins;
      c.min_line_length = line.min_line_length; c.lsd_scale = line.lsd_scale; c.lsd_sigma_scale = line.lsd_sigma_scale;
      c.lsd_quant = line.lsd_quant; c.lsd_ang_th = line.lsd_ang_th; c.lsd_log_eps = line.lsd_log_eps;
      c.lsd_density_th = line.lsd_density_th;
      if (c.lsd_nfeatures > c.max_lines) c.max_lines = c.lsd_nfeatures;
    }
    auto fe = std::make_shared<pli::Frontend>(c);      // throws pli::Error (e.g. lsd_refine != 0, no gfx950 device)
    ctx[{w, h}] = fe;
    return fe;
  }
  // The rig Frame::ComputeStereoMatches works with (mbf, fx = mK(0,0); Frame.cc:1005-1008).  The extractors' constructors do not
  // know it (Tracking.cc:743-746), so a context starts with pli_config_default's EuRoC rig until the first Frame names its own:
  // every context of the group — existing and future — takes it; a fused Frame that was matched with the old rig is matched
  // again on its resident tables by the next ComputeStereoMatches (pli_set_stereo_camera drops the cached result).
  void setRig(float bf, float fx) {
    std::lock_guard<std::mutex> lk(mu);
    if (bf == rigBf && fx == rigFx) return;
    rigBf = bf; rigFx = fx;
    for (auto& kv : ctx) kv.second->setStereoCamera(bf, fx);
  }
};

inline int freeEye(int mask) { return (mask & 1) ? 1 : 0; }

struct Registry {
  std::mutex mu;
  std::vector<std::shared_ptr<Group>> groups;
  static Registry& get() { static Registry r; return r; }
  // the group of the k-th distinct parameter set of its kind; eye = the free slot taken (left first)
  std::shared_ptr<Group> joinOrb(const OrbParams& p, int& eye) {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& g : groups)
      if (g->hasOrb && g->orb == p && g->orbMask.load() != 3) { eye = freeEye(g->orbMask.load()); g->orbMask |= 1 << eye; return g; }
    for (auto& g : groups)
      if (!g->hasOrb) { g->hasOrb = true; g->orb = p; eye = 0; g->orbMask = 1; return g; }
    groups.push_back(std::make_shared<Group>());
    auto& g = groups.back();
    g->hasOrb = true; g->orb = p; eye = 0; g->orbMask = 1;
    return g;
  }
  std::shared_ptr<Group> joinLine(const LineParams& p, int& eye) {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& g : groups)
      if (g->hasLine && g->line == p && g->lineMask.load() != 3) { eye = freeEye(g->lineMask.load()); g->lineMask |= 1 << eye; return g; }
    for (auto& g : groups)
      if (!g->hasLine) { g->hasLine = true; g->line = p; eye = 0; g->lineMask = 1; return g; }
    groups.push_back(std::make_shared<Group>());
    auto& g = groups.back();
    g->hasLine = true; g->line = p; eye = 0; g->lineMask = 1;
    return g;
  }
  // an extractor dies (or is re-bound): its eye slot is free again; a kind without extractors forgets its parameters, and a
  // group without extractors leaves the registry — its device contexts go with the last shared_ptr (a Frame-level matcher
  // still running on one keeps it alive until it returns).
  void leave(const std::shared_ptr<Group>& g, bool isOrb, int eye) {
    if (!g) return;
    std::lock_guard<std::mutex> lk(mu);
    if (isOrb) { g->orbMask &= ~(1 << eye); if (!g->orbMask.load()) g->hasOrb = false; }
    else { g->lineMask &= ~(1 << eye); if (!g->lineMask.load()) g->hasLine = false; }
    if (!g->orbMask.load() && !g->lineMask.load())
      for (size_t i = 0; i < groups.size(); ++i)
        if (groups[i] == g) { groups.erase(groups.begin() + i); break; }
  }
  void adopt(const std::shared_ptr<Group>& g) {
    std::lock_guard<std::mutex> lk(mu);
    groups.push_back(g);
  }
  // a context for the stateless matchers (any group will do)
  std::shared_ptr<pli::Frontend> any() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& g : groups) {
      std::lock_guard<std::mutex> lk2(g->mu);
      if (!g->ctx.empty()) return g->ctx.begin()->second;
    }
    return nullptr;
  }
};

inline void checkGray(const cv::Mat& m, const char* who) {
  if (m.type() != CV_8UC1) throw std::invalid_argument(std::string(who) + ": the image must be CV_8UC1 (the reference asserts the same)");
}

}  // namespace pli_detail

class ORBextractor;
class Lineextractor;
// (not in the reference) Explicit pairing instead of the construction-order rule above: the four extractors of a stereo
// Tracking (Tracking.cc:87-98,743-749) — or the two of a monocular one (right = nullptr) — move onto ONE fresh group /
// device context.  Call it once after construction when the order or the parameters make the implicit rule ambiguous
// (e.g. initial extractors built with the same parameters as the main ones).
inline void pliBind(ORBextractor* orbLeft, ORBextractor* orbRight, Lineextractor* lineLeft, Lineextractor* lineRight);

class ORBextractor {
  friend void pliBind(ORBextractor*, ORBextractor*, Lineextractor*, Lineextractor*);
 public:
  enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
      : mvImagePyramid(nlevels), nfeatures(nfeatures), scaleFactor(scaleFactor), nlevels(nlevels), iniThFAST(iniThFAST), minThFAST(minThFAST) {
    mvScaleFactor.resize(nlevels); mvLevelSigma2.resize(nlevels);
    mvScaleFactor[0] = 1.0f; mvLevelSigma2[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) { mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor; mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i]; }
    mvInvScaleFactor.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
    for (int i = 0; i < nlevels; i++) { mvInvScaleFactor[i] = 1.0f / mvScaleFactor[i]; mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i]; }
    group_ = pli_detail::Registry::get().joinOrb({nfeatures, nlevels, iniThFAST, minThFAST, scaleFactor}, eye_);
  }
  ~ORBextractor() { pli_detail::Registry::get().leave(group_, true, eye_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // Compute the ORB features and descriptors on an image (mask ignored like the reference; vLappingArea: see below).
  int operator()(cv::InputArray _image, cv::InputArray /*_mask*/, std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors,
                 std::vector<int>& vLappingArea) {
    if (_image.empty()) return -1;
    cv::Mat image = _image.getMat();
    pli_detail::checkGray(image, "ORBextractor");
    std::shared_ptr<pli::Frontend> fe = group_->context(image.cols, image.rows);
    lastW_ = image.cols; lastH_ = image.rows;
    std::vector<pli_keypoint> kps;
    std::vector<uint8_t> desc;
    int n;
    pli_detail::FrameFusion::RecordRef fused;
    if (group_->orbMask.load() == 3 && group_->lineMask.load() == 3 &&
        group_->fusion.join(eye_ ? pli_detail::FrameFusion::kOrbR : pli_detail::FrameFusion::kOrbL, *fe, image.data, image.cols, image.rows,
                            (int64_t)image.step, fused)) {
      // the frame's record: counts, then this eye's keypoint table and descriptors
      const pli_table_layout& Y = fe->layout();
      const uint8_t* rec = fused->data();
      n = reinterpret_cast<const int32_t*>(rec + Y.off_counts)[eye_];
      kps.resize(n);
      desc.resize((size_t)n * 32);
      if (n) {
        std::memcpy(kps.data(), rec + Y.off_kp[eye_], (size_t)n * sizeof(pli_keypoint));
        std::memcpy(desc.data(), rec + Y.off_desc[eye_], (size_t)n * 32);
      }
    } else {
      n = fe->extractORB(eye_, image.data, image.cols, image.rows, (int64_t)image.step, kps, desc);
    }
    if (n < 0) return -1;
    // ORBextractor.cc:1135-1144: keypoints inside [vLappingArea[0], vLappingArea[1]] (level-0 x) go to the back of the
    // arrays (filled from the end), the others to the front in order; the return value is the number of front entries.
    // On the rectified stereo path vLappingArea = {0, 0}, where this is the identity except for keypoints at x == 0
    // (none: the extractor keeps a 16-px border).
    std::vector<int> order(n);
    int mono = 0, stereo = n - 1;
    for (int i = 0; i < n; ++i) {
      const bool lapping = vLappingArea.size() >= 2 && kps[i].x >= vLappingArea[0] && kps[i].x <= vLappingArea[1];
      if (lapping) order[stereo--] = i; else order[mono++] = i;
    }
    _keypoints.resize(n);
    if (n == 0) _descriptors.release();
    else _descriptors.create(n, 32, CV_8U);
    cv::Mat D = n ? _descriptors.getMat() : cv::Mat();
    for (int j = 0; j < n; ++j) {
      const pli_keypoint& k = kps[order[j]];
      _keypoints[j] = cv::KeyPoint(k.x, k.y, k.size, k.angle, k.response, k.octave, -1);
      std::memcpy(D.ptr(j), desc.data() + (size_t)order[j] * 32, 32);
    }
    // public member the stereo matcher and drawers read (ORBextractor.h:87); levels come back without the border.  An integrator
    // that uses adapters/frame_stereo.hpp (the stereo matchers run on the device, on the resident pyramids) and no drawer of the
    // pyramid can switch the copy off — pliCopyPyramidBack(false): 1.3 MB per eye and Frame stay on the device, the member is left empty
    if (pliPyramidFlag().load(std::memory_order_relaxed)) {
      for (int l = 0; l < nlevels; ++l) {
        int w = 0, h = 0;
        pli::check(pli_orb_pyramid_level(fe->handle(), eye_, l, nullptr, 0, &w, &h));
        mvImagePyramid[l].create(h, w, CV_8U);
        pli::check(pli_orb_pyramid_level(fe->handle(), eye_, l, mvImagePyramid[l].data, (int64_t)w * h, &w, &h));
      }
    } else {
      for (int l = 0; l < nlevels; ++l) mvImagePyramid[l].release();
    }
    return mono;
  }
  // (not in the reference) whether operator() fills mvImagePyramid (default: yes, as the reference's ComputePyramid does); process-wide
  static void pliCopyPyramidBack(bool on) { pliPyramidFlag().store(on, std::memory_order_relaxed); }

  int inline GetLevels() { return nlevels; }
  float inline GetScaleFactor() { return scaleFactor; }
  std::vector<float> inline GetScaleFactors() { return mvScaleFactor; }
  std::vector<float> inline GetInverseScaleFactors() { return mvInvScaleFactor; }
  std::vector<float> inline GetScaleSigmaSquares() { return mvLevelSigma2; }
  std::vector<float> inline GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

  std::vector<cv::Mat> mvImagePyramid;

  // (not in the reference) the shared device context for an image size: Frame's stereo matchers run on it
  std::shared_ptr<pli::Frontend> pliContext(int w, int h) { return group_->context(w, h); }
  int pliEye() const { return eye_; }
  // (not in the reference) size of the image of the last operator() call (0 x 0 before the first): what mvImagePyramid[0] says when it is copied back
  void pliLastImageSize(int& w, int& h) const { w = lastW_; h = lastH_; }
  // (not in the reference) the rig of the Frames this extractor serves: mbf and fx (Frame.cc:1005-1008).  Frame::ComputeStereoMatches
  // (adapters/frame_stereo.hpp) calls it for every Frame; an integrator may call it once after reading the calibration
  // (Tracking.cc:620-640) so that even the first fused Frame is matched with the right rig in its one submission.
  void pliSetStereoCamera(float bf, float fx) { group_->setRig(bf, fx); }
  // (not in the reference) Frames fused / calls that went alone / timeouts / mismatched frames / sleeps of this extractor's group
  pli_detail::FrameFusion::Stats pliFusionStats() { return group_->fusion.stats(); }

 protected:
  static std::atomic<bool>& pliPyramidFlag() { static std::atomic<bool> on{true}; return on; }
  int lastW_ = 0, lastH_ = 0;
  int nfeatures;
  double scaleFactor;
  int nlevels, iniThFAST, minThFAST;
  std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
  std::shared_ptr<pli_detail::Group> group_;
  int eye_ = 0;
};

#ifdef PLI_ADAPTER_KEYLINE_TYPE
typedef PLI_ADAPTER_KEYLINE_TYPE PliKeyLine;
#else
typedef cv::line_descriptor::KeyLine PliKeyLine;
#endif

class Lineextractor {
  friend void pliBind(ORBextractor*, ORBextractor*, Lineextractor*, Lineextractor*);
 public:
  Lineextractor(int _lsd_nfeatures, double _llength_th, bool _bFLD = false)
      : Lineextractor(_lsd_nfeatures, _llength_th, 0, 0.8, 0.6, 2.0, 22.5, 1.0, 0.7, 1024, _bFLD) {}   // LSDOptions defaults, LineExtractor.cc:31-48
  Lineextractor(int _lsd_nfeatures, double _llength_th, int _lsd_refine, double _lsd_scale, double _lsd_sigma_scale, double _lsd_quant,
                double _lsd_ang_th, double _lsd_log_eps, double _lsd_density_th, int _lsd_n_bins, bool _bFLD = false)
      : lsd_nfeatures(_lsd_nfeatures), min_line_length(_llength_th), lsd_refine(_lsd_refine), lsd_scale(_lsd_scale),
        lsd_sigma_scale(_lsd_sigma_scale), lsd_quant(_lsd_quant), lsd_ang_th(_lsd_ang_th), lsd_log_eps(_lsd_log_eps),
        lsd_density_th(_lsd_density_th), lsd_n_bins(_lsd_n_bins), bFLD(_bFLD) {
    if (bFLD) throw std::invalid_argument("Lineextractor: the FLD detector is not on the reference path (bFLD = false everywhere)");
    group_ = pli_detail::Registry::get().joinLine({lsd_nfeatures, lsd_refine, lsd_n_bins, min_line_length, lsd_scale, lsd_sigma_scale,
                                                   lsd_quant, lsd_ang_th, lsd_log_eps, lsd_density_th, bFLD}, eye_);
  }
  ~Lineextractor() { pli_detail::Registry::get().leave(group_, false, eye_); }
  Lineextractor(const Lineextractor&) = delete;
  Lineextractor& operator=(const Lineextractor&) = delete;

  void operator()(const cv::Mat& image, const cv::Mat& /*mask*/, std::vector<PliKeyLine>& keylines, cv::Mat& descriptors_line) {
    pli_detail::checkGray(image, "Lineextractor");
    std::shared_ptr<pli::Frontend> fe = group_->context(image.cols, image.rows);
    std::vector<pli_keyline> kls;
    std::vector<uint8_t> desc;
    pli_detail::FrameFusion::RecordRef fused;
    if (group_->orbMask.load() == 3 && group_->lineMask.load() == 3 &&
        group_->fusion.join(eye_ ? pli_detail::FrameFusion::kLineR : pli_detail::FrameFusion::kLineL, *fe, image.data, image.cols, image.rows,
                            (int64_t)image.step, fused)) {
      const pli_table_layout& Y = fe->layout();
      const uint8_t* rec = fused->data();
      const int n = reinterpret_cast<const int32_t*>(rec + Y.off_counts)[2 + eye_];
      kls.resize(n);
      desc.resize((size_t)n * 32);
      if (n) {
        std::memcpy(kls.data(), rec + Y.off_kl[eye_], (size_t)n * sizeof(pli_keyline));
        std::memcpy(desc.data(), rec + Y.off_ldesc[eye_], (size_t)n * 32);
      }
    } else {
      fe->extractLines(eye_, image.data, image.cols, image.rows, (int64_t)image.step, kls, desc);
    }
    keylines.resize(kls.size());
    for (size_t i = 0; i < kls.size(); ++i) {
      PliKeyLine& k = keylines[i];
      const pli_keyline& s = kls[i];
      k.angle = s.angle; k.class_id = s.class_id; k.octave = s.octave; k.pt = cv::Point2f(s.pt_x, s.pt_y);
      k.response = s.response; k.size = s.size;
      k.startPointX = s.startPointX; k.startPointY = s.startPointY; k.endPointX = s.endPointX; k.endPointY = s.endPointY;
      k.sPointInOctaveX = s.sPointInOctaveX; k.sPointInOctaveY = s.sPointInOctaveY;
      k.ePointInOctaveX = s.ePointInOctaveX; k.ePointInOctaveY = s.ePointInOctaveY;
      k.lineLength = s.lineLength; k.numOfPixels = s.numOfPixels;
    }
    if (!kls.empty()) {     // the reference leaves descriptors_line untouched when no line survives
      descriptors_line.create((int)kls.size(), 32, CV_8UC1);
      std::memcpy(descriptors_line.data, desc.data(), desc.size());
    }
  }

  std::shared_ptr<pli::Frontend> pliContext(int w, int h) { return group_->context(w, h); }
  int pliEye() const { return eye_; }

 protected:
  int lsd_nfeatures;
  double min_line_length;
  int lsd_refine;
  double lsd_scale, lsd_sigma_scale, lsd_quant, lsd_ang_th, lsd_log_eps, lsd_density_th;
  int lsd_n_bins;
  bool bFLD;
  std::shared_ptr<pli_detail::Group> group_;
  int eye_ = 0;
};

inline void pliBind(ORBextractor* orbLeft, ORBextractor* orbRight, Lineextractor* lineLeft, Lineextractor* lineRight) {
  using namespace pli_detail;
  if (!orbLeft && !lineLeft) throw std::invalid_argument("pliBind: no left extractor");
  if ((orbRight && !orbLeft) || (lineRight && !lineLeft)) throw std::invalid_argument("pliBind: a right extractor without its left one");
  auto orbParams = [](ORBextractor* e) { return OrbParams{e->nfeatures, e->nlevels, e->iniThFAST, e->minThFAST, (float)e->scaleFactor}; };
  auto lineParams = [](Lineextractor* e) {
    return LineParams{e->lsd_nfeatures, e->lsd_refine, e->lsd_n_bins, e->min_line_length, e->lsd_scale, e->lsd_sigma_scale,
                      e->lsd_quant, e->lsd_ang_th, e->lsd_log_eps, e->lsd_density_th, e->bFLD};
  };
  if (orbRight && !(orbParams(orbLeft) == orbParams(orbRight))) throw std::invalid_argument("pliBind: the two ORB extractors differ");
  if (lineRight && !(lineParams(lineLeft) == lineParams(lineRight))) throw std::invalid_argument("pliBind: the two line extractors differ");
  auto g = std::make_shared<Group>();
  Registry& R = Registry::get();
  if (orbLeft) {
    g->hasOrb = true; g->orb = orbParams(orbLeft);
    R.leave(orbLeft->group_, true, orbLeft->eye_);
    orbLeft->group_ = g; orbLeft->eye_ = 0; g->orbMask |= 1;
    if (orbRight) { R.leave(orbRight->group_, true, orbRight->eye_); orbRight->group_ = g; orbRight->eye_ = 1; g->orbMask |= 2; }
  }
  if (lineLeft) {
    g->hasLine = true; g->line = lineParams(lineLeft);
    R.leave(lineLeft->group_, false, lineLeft->eye_);
    lineLeft->group_ = g; lineLeft->eye_ = 0; g->lineMask |= 1;
    if (lineRight) { R.leave(lineRight->group_, false, lineRight->eye_); lineRight->group_ = g; lineRight->eye_ = 1; g->lineMask |= 2; }
  }
  R.adopt(g);
}

// int match(const cv::Mat& desc1, const cv::Mat& desc2, float nnr, std::vector<int>& matches_12), LineMatcher.h:63 /
// LineMatcher.cpp:201-229 (uses the context of the extractors that produced the descriptors; they exist by then)
inline int match(const cv::Mat& desc1, const cv::Mat& desc2, float nnr, std::vector<int>& matches_12) {
  std::shared_ptr<pli::Frontend> fe = pli_detail::Registry::get().any();
  if (!fe) throw std::logic_error("ORB_SLAM3::match: no extractor has run yet (no device context)");
  matches_12.assign(desc1.rows, -1);
  if (desc1.rows == 0) return 0;
  return fe->matchLines(desc1.data, desc1.rows, desc2.data, desc2.rows, nnr, matches_12);
}

namespace pli_detail {
// A DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) as one node id per feature, -1 = listed in no node.  DBoW2's
// transform() lists every feature once, in ascending order within its node; anything else was not built by transform().
template <class FeatVecT>
std::vector<int32_t> featureNodes(const FeatVecT& fv, int n, const char* what) {
  std::vector<int32_t> node((size_t)n, -1);
  for (const auto& kv : fv) {
    if ((uint64_t)kv.first > (uint64_t)INT32_MAX) throw std::logic_error(std::string(what) + ": node id beyond 2^31 - 1");
    for (size_t t = 0; t < kv.second.size(); ++t) {
      const uint64_t i = kv.second[t];
      if (i >= (uint64_t)n) throw std::logic_error(std::string(what) + ": feature index beyond N");
      if (t > 0 && kv.second[t - 1] >= kv.second[t])
        throw std::logic_error(std::string(what) + ": a node's feature list is not ascending (not built by transform)");
      if (node[i] != -1) throw std::logic_error(std::string(what) + ": a feature listed in two nodes (not built by transform)");
      node[i] = (int32_t)kv.first;
    }
  }
  return node;
}

// ---- what the searches against a batch of keyframes (SearchByBoW, SearchForTriangulation, Fuse) share on the host ----
// The device context the extractors created; `who` names the caller in the message.
inline std::shared_ptr<pli::Frontend> deviceContext(const char* who) {
  std::shared_ptr<pli::Frontend> fe = Registry::get().any();
  if (!fe) throw std::logic_error(std::string(who) + ": no extractor has run yet (no device context)");
  return fe;
}

inline pli_keypoint keypoint(const cv::KeyPoint& k) { return pli_keypoint{k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave}; }

// The flat tables of a batch: keyframe k is rows off[k] .. off[k + 1].  A matcher derives from it and adds its own columns.
struct KfTable {
  std::vector<int32_t> off = std::vector<int32_t>(1, 0), node;
  std::vector<uint8_t> desc;
};
// appends the n rows of a keyframe's (or frame's) mDescriptors and closes its row range
template <class MatT>
void appendDescriptors(KfTable& T, const MatT& descriptors, int n) {
  for (int i = 0; i < n; ++i) {
    const uint8_t* d = descriptors.template ptr<uint8_t>(i);
    T.desc.insert(T.desc.end(), d, d + 32);
  }
  T.off.push_back(T.off.back() + n);
}
// appends the node of each of its n features (featureNodes; `what` names the FeatureVector in its messages)
template <class FeatVecT>
void appendNodes(KfTable& T, const FeatVecT& fv, int n, const char* what) {
  const std::vector<int32_t> node = featureNodes(fv, n, what);
  T.node.insert(T.node.end(), node.begin(), node.end());
}
// The nkf x n table of indices a batched search returns: fn(k, i, j) for every match j >= 0 of item i in keyframe k, in index order.
template <class Fn>
void forEachMatch(const std::vector<int>& matches, int nkf, int n, Fn fn) {
  for (int k = 0; k < nkf; ++k)
    for (int i = 0; i < n; ++i) {
      const int j = matches[(size_t)k * n + i];
      if (j >= 0) fn(k, i, j);
    }
}

// The host geometry of ORBmatcher::SearchForTriangulation for keyframes of one pinhole camera each: the epipole
// ep = pKF2->mpCamera->project(R2w * Cw + t2w) (ORBmatcher.cc:972-977, Pinhole.cpp:30-33), R12 = R1w * R2w.t(),
// t12 = -R1w * R2w.t() * t2w + t1w (:991-992) and F12 = K1.t().inv() * t12x * R12 * K2.inv() (Pinhole.cpp:124-127).
// R*: 3 x 3 row major, K*: fx, fy, cx, cy.
// Arithmetic convention (PARITY UNPINNED: OpenCV's own arithmetic, no OpenCV here to compare with): every cv::Mat product is one
// CV_32F gemm by the convention DESIGN.md §9 lists - products and sum in double, `+ C` inside the same sum, one rounding to float
// per element - and a chain A * B * C materialises (A * B) as float first; -R1w * R2w.t() is the gemm with alpha = -1; inv() of a
// 3 x 3 CV_32F matrix is OpenCV's closed form: the determinant and the cofactors in double, each element (float)(cofactor * (1 /
// det)), all zeros for det == 0.  project() is the reference's float expression fx * x / z + cx, left to right.
inline void triangulationGeometry(const float R1w[9], const float t1w[3], const float Cw[3], const float K1[4], const float R2w[9],
                                  const float t2w[3], const float K2[4], float F12[9], float ep[2]) {
  auto gemm = [](const float* A, bool transA, double alpha, const float* B, bool transB, int cols, const float* C, float* out) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < cols; ++j) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k)
          d += (double)(transA ? A[k * 3 + i] : A[i * 3 + k]) * (double)(transB ? B[j * 3 + k] : B[k * cols + j]);
        out[i * cols + j] = (float)(alpha * d + (C ? (double)C[i * cols + j] : 0.0));
      }
  };
  auto inv3 = [](const float* S, float* out) {
    const double det = S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) +
                       S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
    if (det == 0.0) { for (int i = 0; i < 9; ++i) out[i] = 0.f; return; }
    const double d = 1.0 / det;
    out[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
    out[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
    out[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
    out[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
    out[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
    out[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
    out[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
    out[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
    out[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
  };
  float C2[3];
  gemm(R2w, false, 1.0, Cw, false, 1, t2w, C2);
  ep[0] = K2[0] * C2[0] / C2[2] + K2[2];
  ep[1] = K2[1] * C2[1] / C2[2] + K2[3];
  float R12[9], negR12[9], t12[3];
  gemm(R1w, false, 1.0, R2w, true, 3, nullptr, R12);
  gemm(R1w, false, -1.0, R2w, true, 3, nullptr, negR12);
  gemm(negR12, false, 1.0, t2w, false, 1, t1w, t12);
  const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};      // SkewSymmetricMatrix
  const float K1t[9] = {K1[0], 0.f, 0.f, 0.f, K1[1], 0.f, K1[2], K1[3], 1.f};
  const float K2m[9] = {K2[0], 0.f, K2[2], 0.f, K2[1], K2[3], 0.f, 0.f, 1.f};
  float K1ti[9], K2i[9], A[9], B[9];
  inv3(K1t, K1ti);
  inv3(K2m, K2i);
  gemm(K1ti, false, 1.0, t12x, false, 3, nullptr, A);
  gemm(A, false, 1.0, R12, false, 3, nullptr, B);
  gemm(B, false, 1.0, K2i, false, 3, nullptr, F12);
}

// One keyframe's side of SearchForTriangulation for keyframes of one pinhole camera each, as the batch form and
// PliCreateNewMapPoints (orbslam_local_mapping.hpp) gather it: the flat tables, and the pose and intrinsics of the keyframe
// gathered last (triangulationGeometry reads them).
struct TriangulationTable : KfTable {
  std::vector<pli_keypoint> kp;
  std::vector<uint8_t> hasMp, stereo;
  float R[9], t[3], K[4];
};
// appends pKF's rows; `who` names the caller and `what` the FeatureVector in the messages.  A keyframe of two cameras is refused.
template <class KeyFrameT>
void gatherTriangulationTable(KeyFrameT* pKF, TriangulationTable& T, const char* who, const char* what) {
  if (pKF->mpCamera2 || pKF->NLeft != -1)
    throw std::logic_error(std::string(who) + ": a keyframe of two cameras (mpCamera2 set, NLeft != -1) is not supported");
  const int n = pKF->N;
  appendNodes(T, pKF->mFeatVec, n, what);
  appendDescriptors(T, pKF->mDescriptors, n);
  for (int i = 0; i < n; ++i) {
    T.kp.push_back(keypoint(pKF->mvKeysUn[i]));
    T.hasMp.push_back(pKF->GetMapPoint(i) ? 1 : 0);                 // (ORBmatcher.cc:1033-1039, :1064-1068: isBad() is not asked)
    T.stereo.push_back(pKF->mvuRight[i] >= 0 ? 1 : 0);
  }
  const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), K = pKF->mpCamera->toK();
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T.R[i * 3 + j] = R.template at<float>(i, j);
    T.t[i] = t.template at<float>(i);
  }
  T.K[0] = K.template at<float>(0, 0); T.K[1] = K.template at<float>(1, 1);
  T.K[2] = K.template at<float>(0, 2); T.K[3] = K.template at<float>(1, 2);
}

// Where the two SearchByProjection(CurrentFrame, LastFrame, ...) overloads put a camera-frame point in the image, in the reference's
// float operation order: pinholeProject = CurrentFrame.mpCamera->project(x3Dc) of the overload without match12 (ORBmatcher.cc:2002,
// Pinhole.cpp:30-33: fx * x / z + cx); otherwise the overload with match12 (:2222-2223: fx * xc * invzc + cx, invzc = 1.0 / zc).
inline void lastFrameProjection(float fx, float fy, float cx, float cy, float xc, float yc, float zc, float invzc, bool pinholeProject,
                                float& u, float& v) {
  if (pinholeProject) {
    u = fx * xc / zc + cx;
    v = fy * yc / zc + cy;
  } else {
    u = fx * xc * invzc + cx;
    v = fy * yc * invzc + cy;
  }
}
}  // namespace pli_detail

// The parts of ORB_SLAM3::ORBmatcher on the hot path.  Template on the tree's Frame / MapPoint so that this header does
// not need Frame.h; inside the PLI-SLAM tree: `using ORBmatcher = ORB_SLAM3::PliORBmatcher<Frame, MapPoint>;`.
template <class FrameT, class MapPointT>
class PliORBmatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
  PliORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

  // ORBmatcher.cc:2495-2511 (bit-twiddling popcount over 8 x 32 bits): the same number as 4 x popcount(64)
  static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) { return pli::descriptorDistance(a.ptr<uint8_t>(), b.ptr<uint8_t>()); }

  // ORBmatcher.cc:1961-2177 (Nleft == -1).  It differs from the overload below in ONE expression: it projects with
  // CurrentFrame.mpCamera->project(x3Dc), Pinhole.cpp:30-33: fx * x / z + cx (:2002), where the other has fx * xc * invzc + cx (:2222);
  // the two round differently (tests/golden/match_ref/frame_forms.npz: the reference's own answers tell them apart).
  int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono) {
    std::map<int, int> m;
    return searchLastFrame(CurrentFrame, LastFrame, th, bMono, m, true);
  }

  // ORBmatcher.cc:2179-2323.  The projection (lines 2190-2244) is the reference's own cv::Mat arithmetic, run here on the host;
  // the window search, the "already taken" exclusion, TH_HIGH, the rotation histogram and ComputeThreeMaxima run on the GPU.
  int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono, std::map<int, int>& match12) {
    return searchLastFrame(CurrentFrame, LastFrame, th, bMono, match12, false);
  }

 protected:
  // What the two SearchByProjection(CurrentFrame, LastFrame, ...) overloads share; pinholeProject: the projection of :2002.
  int searchLastFrame(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono, std::map<int, int>& match12,
                      const bool pinholeProject) {
    match12.clear();
    const cv::Mat Rcw = CurrentFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const cv::Mat tcw = CurrentFrame.mTcw.rowRange(0, 3).col(3);
    const cv::Mat twc = -Rcw.t() * tcw;
    const cv::Mat Rlw = LastFrame.mTcw.rowRange(0, 3).colRange(0, 3);
    const cv::Mat tlw = LastFrame.mTcw.rowRange(0, 3).col(3);
    const cv::Mat tlc = Rlw * twc + tlw;
    const bool bForward = tlc.at<float>(2) > CurrentFrame.mb && !bMono;
    const bool bBackward = -tlc.at<float>(2) > CurrentFrame.mb && !bMono;
    const int N = LastFrame.N;
    std::vector<pli_proj_query> q((size_t)N);
    std::vector<uint8_t> qdesc((size_t)N * 32, 0);
    for (int i = 0; i < N; i++) {
      pli_proj_query& Q = q[i];
      std::memset(&Q, 0, sizeof(Q));
      Q.max_level = -1;
      MapPointT* pMP = LastFrame.mvpMapPoints[i];
      if (!pMP || LastFrame.mvbOutlier[i]) continue;
      cv::Mat x3Dw = pMP->GetWorldPos();
      cv::Mat x3Dc = Rcw * x3Dw + tcw;
      const float xc = x3Dc.at<float>(0);
      const float yc = x3Dc.at<float>(1);
      const float invzc = 1.0 / x3Dc.at<float>(2);
      if (invzc < 0) continue;
      pli_detail::lastFrameProjection(CurrentFrame.fx, CurrentFrame.fy, CurrentFrame.cx, CurrentFrame.cy, xc, yc, x3Dc.at<float>(2), invzc,
                                      pinholeProject, Q.u, Q.v);
      const int nLastOctave = LastFrame.mvKeys[i].octave;
      Q.radius = th * CurrentFrame.mvScaleFactors[nLastOctave];
      if (bForward) { Q.min_level = nLastOctave; Q.max_level = -1; }
      else if (bBackward) { Q.min_level = 0; Q.max_level = nLastOctave; }
      else { Q.min_level = nLastOctave - 1; Q.max_level = nLastOctave + 1; }
      Q.ur = Q.u - CurrentFrame.mbf * invzc;
      Q.angle = LastFrame.mvKeysUn[i].angle;
      // (the image-bounds test :2225-2228 is done by the library; a map point without observations — UpdateLastFrame's temporal points in
      // localisation mode — does not make the keypoint it is written to unavailable to the queries behind it, :2255-2257)
      Q.valid = pMP->Observations() > 0 ? 1 : (1 | PLI_PROJ_NO_OBSERVATIONS);
      const cv::Mat dMP = pMP->GetDescriptor();
      std::memcpy(&qdesc[(size_t)i * 32], dMP.ptr<uint8_t>(), 32);
    }
    // the current frame: keypoints, descriptors, mvuRight; keypoints that already hold a map point with observations are
    // not available (:2255-2257): handed over as the `cur_occupied` mask
    const int M = CurrentFrame.N;
    std::vector<pli_keypoint> kp((size_t)M);
    for (int j = 0; j < M; ++j) {
      const cv::KeyPoint& k = CurrentFrame.mvKeysUn[j];
      kp[j].x = k.pt.x; kp[j].y = k.pt.y; kp[j].size = k.size; kp[j].angle = k.angle; kp[j].response = k.response; kp[j].octave = k.octave;
    }
    std::vector<uint8_t> occupied((size_t)M, 0);
    bool anyOccupied = false;
    for (int j = 0; j < M; ++j)
      if (CurrentFrame.mvpMapPoints[j] && CurrentFrame.mvpMapPoints[j]->Observations() > 0) { occupied[j] = 1; anyOccupied = true; }
    std::shared_ptr<pli::Frontend> fe = pli_detail::Registry::get().any();
    if (!fe) throw std::logic_error("SearchByProjection: no extractor has run yet (no device context)");
    std::vector<int> best, raw;
    const int nmatches = fe->searchByProjection(q, qdesc.data(), kp, CurrentFrame.mDescriptors.data, CurrentFrame.mvuRight.data(),
                                                CurrentFrame.mnMinX, CurrentFrame.mnMaxX, CurrentFrame.mnMinY, CurrentFrame.mnMaxY,
                                                mbCheckOrientation, best, anyOccupied ? occupied.data() : nullptr, &raw);
    // the reference's writes, replayed in its order: every match as it was made (:2280-2282: the last writer holds the keypoint,
    // std::map::insert keeps the first pair of a key), then the rotation filter's removals (:2315-2317)
    for (int i = 0; i < N; ++i)
      if (raw[i] >= 0) {
        CurrentFrame.mvpMapPoints[raw[i]] = LastFrame.mvpMapPoints[i];
        match12.insert(std::pair<int, int>(raw[i], i));
      }
    for (int i = 0; i < N; ++i)
      if (raw[i] >= 0 && best[i] < 0) {
        CurrentFrame.mvpMapPoints[raw[i]] = static_cast<MapPointT*>(nullptr);
        match12.erase(raw[i]);
      }
    return nmatches;
  }

 public:
  // ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches), ORBmatcher.cc:269-470, for a frame of
  // one camera or rectified stereo (F.Nleft == -1) and a keyframe without a second camera: the node walk, TH_LOW, the ratio test,
  // the rotation histogram and ComputeThreeMaxima run on the GPU.  KeyFrameT needs N, mDescriptors, mvKeysUn, mFeatVec,
  // mpCamera2 and GetMapPointMatches(); FrameT N, Nleft, mDescriptors, mvKeys and mFeatVec (both FeatureVectors from transform).
  template <class KeyFrameT>
  int SearchByBoW(KeyFrameT* pKF, FrameT& F, std::vector<MapPointT*>& vpMapPointMatches) {
    std::vector<std::vector<MapPointT*>> matches;
    std::vector<int> nmatches;
    SearchByBoW(std::vector<KeyFrameT*>(1, pKF), F, matches, nmatches);
    vpMapPointMatches.swap(matches[0]);
    return nmatches[0];
  }

  // (not in the reference) The same for every keyframe of vpKFs in ONE device call: what Tracking::Relocalization's loop over its
  // candidates (Tracking.cc:4205-4230) computes, one vpMapPointMatches and one return value per keyframe.
  template <class KeyFrameT>
  void SearchByBoW(const std::vector<KeyFrameT*>& vpKFs, FrameT& F, std::vector<std::vector<MapPointT*>>& vvpMapPointMatches,
                   std::vector<int>& vnmatches) {
    if (F.Nleft != -1) throw std::logic_error("SearchByBoW: a frame of two cameras (F.Nleft != -1) is not supported");
    const int nf = F.N, nkf = (int)vpKFs.size();
    pli_detail::KfTable TF;
    pli_detail::appendNodes(TF, F.mFeatVec, nf, "SearchByBoW: F.mFeatVec");
    pli_detail::appendDescriptors(TF, F.mDescriptors, nf);
    std::vector<float> fAngle((size_t)nf);
    for (int i = 0; i < nf; ++i) fAngle[i] = F.mvKeys[i].angle;
    std::vector<std::vector<MapPointT*>> kfPoints((size_t)nkf);
    BowTable T;
    for (int k = 0; k < nkf; ++k) {
      if (vpKFs[k]->mpCamera2) throw std::logic_error("SearchByBoW: a keyframe of two cameras (mpCamera2 set) is not supported");
      kfPoints[k] = vpKFs[k]->GetMapPointMatches();
      bowGatherKeyFrame(vpKFs[k], kfPoints[k], "SearchByBoW: pKF->mFeatVec", T);
    }
    std::vector<int> matches;
    pli_detail::deviceContext("SearchByBoW")->searchByBoW(nkf, T.off.data(), T.desc.data(), T.angle.data(), T.node.data(), T.valid.data(),
                                                         TF.desc.data(), fAngle.data(), TF.node.data(), nf, mfNNratio,
                                                         mbCheckOrientation, matches, vnmatches);
    vvpMapPointMatches.assign((size_t)nkf, std::vector<MapPointT*>((size_t)nf, static_cast<MapPointT*>(nullptr)));
    pli_detail::forEachMatch(matches, nkf, nf, [&](int k, int i, int j) { vvpMapPointMatches[k][i] = kfPoints[k][j]; });
  }

  // ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12), ORBmatcher.cc:823-963, for keyframes
  // of one camera each (NLeft == -1, mpCamera2 == nullptr): the node walk in pKF1's order, vbMatched2, bestDist1 < TH_LOW, the ratio
  // test, the rotation histogram and ComputeThreeMaxima run on the GPU.  KeyFrameT needs N, NLeft, mDescriptors, mvKeysUn, mFeatVec
  // (from transform), mpCamera2 and GetMapPointMatches().
  template <class KeyFrameT>
  int SearchByBoW(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12) {
    std::vector<std::vector<MapPointT*>> matches;
    std::vector<int> nmatches;
    SearchByBoW(pKF1, std::vector<KeyFrameT*>(1, pKF2), matches, nmatches);
    vpMatches12.swap(matches[0]);
    return nmatches[0];
  }

  // (not in the reference) The same for every keyframe of vpKF2 in ONE device call: what the loop of
  // LoopClosing::DetectCommonRegionsFromBoW over a candidate's covisible keyframes (LoopClosing.cc:528-540) computes, one
  // vpMatches12 and one return value per keyframe.  GetMapPointMatches() is taken once per keyframe, at entry.
  template <class KeyFrameT>
  void SearchByBoW(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpKF2, std::vector<std::vector<MapPointT*>>& vvpMatches12,
                   std::vector<int>& vnmatches) {
    auto gather = [](KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const char* what, BowTable& T) {
      if (pKF->mpCamera2 || pKF->NLeft != -1)
        throw std::logic_error("SearchByBoW: a keyframe of two cameras (mpCamera2 set, NLeft != -1) is not supported");
      bowGatherKeyFrame(pKF, vpMapPoints, what, T);                    // :862-866, :882-888
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
                                                           T2.valid.data(), mfNNratio, mbCheckOrientation, matches, vnmatches);
    vvpMatches12.assign((size_t)nkf, std::vector<MapPointT*>(vpMapPoints1.size(), static_cast<MapPointT*>(nullptr)));
    pli_detail::forEachMatch(matches, nkf, n1, [&](int k, int i, int j) { vvpMatches12[k][i] = kfPoints[k][j]; });   // :910
  }

  // ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vector<pair<size_t, size_t>>& vMatchedPairs,
  // const bool bOnlyStereo, const bool bCoarse), ORBmatcher.cc:965-1206, for keyframes of one pinhole camera each (mpCamera2 ==
  // nullptr, NLeft == -1).  F12 is ignored, as the reference ignores it: its gate is mpCamera->epipolarConstrain, which forms its
  // own matrix from the two poses (pli_detail::triangulationGeometry here).  KeyFrameT needs N, NLeft, mDescriptors, mvKeysUn,
  // mvuRight, mFeatVec (from transform), mpCamera (with toK()), mpCamera2, GetMapPoint(i), GetRotation(), GetTranslation() and
  // GetCameraCenter().
  template <class KeyFrameT>
  int SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, cv::Mat /*F12*/, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                             const bool bOnlyStereo, const bool bCoarse = false) {
    std::vector<std::vector<std::pair<size_t, size_t>>> pairs;
    std::vector<int> nmatches;
    SearchForTriangulation(pKF1, std::vector<KeyFrameT*>(1, pKF2), pairs, nmatches, bOnlyStereo, bCoarse);
    vMatchedPairs.swap(pairs[0]);
    return nmatches[0];
  }

  // (not in the reference) The same for every neighbour of vpKF2 in ONE device call: what the loop of
  // LocalMapping::CreateNewMapPoints (LocalMapping.cc:343-423) computes, one vMatchedPairs and one return value per neighbour.
  template <class KeyFrameT>
  void SearchForTriangulation(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpKF2,
                              std::vector<std::vector<std::pair<size_t, size_t>>>& vvMatchedPairs, std::vector<int>& vnmatches,
                              const bool bOnlyStereo, const bool bCoarse = false) {
    const int nkf = (int)vpKF2.size();
    pli_detail::TriangulationTable T1, T2;
    pli_detail::gatherTriangulationTable(pKF1, T1, "SearchForTriangulation", "SearchForTriangulation: pKF1->mFeatVec");
    const int n1 = pKF1->N;
    const cv::Mat Cw = pKF1->GetCameraCenter();
    const float cw[3] = {Cw.template at<float>(0), Cw.template at<float>(1), Cw.template at<float>(2)};
    std::vector<float> F12((size_t)nkf * 9 + 1), ep((size_t)nkf * 2 + 1);
    for (int k = 0; k < nkf; ++k) {
      pli_detail::gatherTriangulationTable(vpKF2[k], T2, "SearchForTriangulation", "SearchForTriangulation: pKF2->mFeatVec");
      pli_detail::triangulationGeometry(T1.R, T1.t, cw, T1.K, T2.R, T2.t, T2.K, &F12[(size_t)k * 9], &ep[(size_t)k * 2]);
    }
    std::vector<int> matches;
    pli_detail::deviceContext("SearchForTriangulation")
        ->searchForTriangulation(T1.kp.data(), T1.desc.data(), T1.node.data(), T1.hasMp.data(), T1.stereo.data(), n1, nkf, T2.off.data(),
                                 T2.kp.data(), T2.desc.data(), T2.node.data(), T2.hasMp.data(), T2.stereo.data(), F12.data(), ep.data(),
                                 bOnlyStereo, bCoarse, mbCheckOrientation, matches, vnmatches);
    vvMatchedPairs.assign((size_t)nkf, std::vector<std::pair<size_t, size_t>>());
    for (int k = 0; k < nkf; ++k) vvMatchedPairs[k].reserve(vnmatches[k]);
    pli_detail::forEachMatch(matches, nkf, n1, [&](int k, int i, int j) {      // vMatches12 read in index order (:1198-1203)
      vvMatchedPairs[k].push_back(std::make_pair((size_t)i, (size_t)j));
    });
  }

  // ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th, const bool bRight), ORBmatcher.cc:
  // 1399-1609, for a keyframe of one pinhole camera (bRight == false, NLeft == -1): the projection and the window search run on
  // the device (pli_fuse_search), :1572-1594 (Replace / AddObservation / AddMapPoint) and the gates isBad() / IsInKeyFrame here.
  // KeyFrameT needs N, NLeft, mvKeysUn, mvuRight, mDescriptors, fx, fy, cx, cy, mbf, mnMinX, mnMaxX, mnMinY, mnMaxY,
  // mnScaleLevels, mfLogScaleFactor, GetRotation(), GetTranslation(), GetCameraCenter(), GetMapPoint(idx), AddMapPoint(pMP, idx)
  // (and GetMapPoints() for the Sim3 form); MapPointT needs isBad(), IsInKeyFrame(pKF), GetWorldPos(), GetNormal(),
  // GetMinDistanceInvariance(), GetMaxDistanceInvariance(), GetDescriptor(), Observations(), Replace(pMP), AddObservation(pKF,
  // idx) and GetMaxDistance(): mfMaxDistance is protected in the reference's MapPoint, INTEGRATION.md gives the one-line accessor.
  template <class KeyFrameT>
  int Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th = 3.0, const bool bRight = false) {
    if (bRight) throw std::logic_error("Fuse: the right camera of a two-camera keyframe (bRight) is not supported");
    std::vector<int> nFused;
    Fuse(std::vector<KeyFrameT*>(1, pKF), vpMapPoints, th, nFused);
    return nFused[0];
  }

  // (not in the reference) The loop of LocalMapping::SearchInNeighbors, LocalMapping.cc:743-749 - Fuse(pKFi, vpMapPointMatches)
  // for every target keyframe - with ONE device search for all targets.  nFused[k] and every side effect equal the reference's
  // keyframe-after-keyframe loop exactly, although Fuse(KF_k) changes state that Fuse(KF_k+1) reads:
  //   * the device searches with the state at entry; the keyframes are then replayed in order on the host, running :1572-1594;
  //   * isBad() and IsInKeyFrame(pKF) are evaluated at replay time, when the point's turn comes, not taken from the uploaded
  //     skip table (which only saves work: inside Fuse a good point never leaves a keyframe and a bad one never recovers);
  //   * the point that survives a Replace has had ComputeDistinctiveDescriptors() run on it (MapPoint.cc:268), so its descriptor
  //     may differ from the one that was searched: the 32 bytes are compared before and after every Replace performed here, and
  //     before keyframe k is replayed every list point whose descriptor changed is searched again, in one call, against the
  //     keyframes k..end.  (Inside keyframe k itself such a point is in the keyframe, so its result there is never read.)
  //     Position, normal and the distances do not change inside Fuse.
  // pnResearch (may be null): the number of such repeated searches.
  template <class KeyFrameT>
  void Fuse(const std::vector<KeyFrameT*>& vpTargetKFs, const std::vector<MapPointT*>& vpMapPoints, const float th,
            std::vector<int>& nFused, int* pnResearch = nullptr) {
    const int nkf = (int)vpTargetKFs.size(), nmp = (int)vpMapPoints.size();
    nFused.assign(nkf, 0);
    if (pnResearch) *pnResearch = 0;
    if (nkf == 0) return;
    FuseTables T;
    for (int k = 0; k < nkf; ++k) {
      KeyFrameT* pKF = vpTargetKFs[k];
      const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
      float pose[15];
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) pose[i * 3 + j] = R.template at<float>(i, j);
        pose[9 + i] = t.template at<float>(i);
        pose[12 + i] = Ow.template at<float>(i);
      }
      fuseGatherKeyFrame(pKF, pose, T);
    }
    std::vector<pli_fuse_point> pts(nmp);
    std::vector<uint8_t> desc((size_t)nmp * 32, 0), skip((size_t)nkf * nmp, 0);
    for (int i = 0; i < nmp; ++i) {
      MapPointT* pMP = vpMapPoints[i];
      pts[i] = fusePoint(pMP);
      if (!pts[i].valid) continue;
      std::memcpy(&desc[(size_t)i * 32], pMP->GetDescriptor().template ptr<uint8_t>(), 32);
      for (int k = 0; k < nkf; ++k) skip[(size_t)k * nmp + i] = pMP->IsInKeyFrame(vpTargetKFs[k]) ? 1 : 0;
    }
    std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("Fuse");
    const std::vector<float>& levelRatio = fuseLevelRatio(vpTargetKFs[0]);
    std::vector<int> best;
    fe->fuseSearch(pts.data(), desc.data(), nmp, nkf, T.off.data(), T.kp.data(), T.desc.data(), T.uright.data(), T.pose.data(),
                   skip.data(), T.cam, th, levelRatio, true, best);
    fuseReplay(vpTargetKFs, vpMapPoints, best, nFused, pnResearch,
               [&](int k, const std::vector<int>& which, const std::vector<pli_fuse_point>& p2, const std::vector<uint8_t>& d2) {
                 std::vector<int32_t> off2(T.off.begin() + k, T.off.end());
                 for (size_t j = off2.size(); j-- > 0;) off2[j] -= off2[0];
                 const size_t row0 = (size_t)T.off[k];
                 std::vector<int> b2;
                 fe->fuseSearch(p2.data(), d2.data(), (int)which.size(), nkf - k, off2.data(), T.kp.data() + row0, T.desc.data() + row0 * 32,
                                T.uright.data() + row0, T.pose.data() + (size_t)k * 15, nullptr, T.cam, th, levelRatio, true, b2);
                 for (int kk = k; kk < nkf; ++kk)
                   for (size_t j = 0; j < which.size(); ++j) best[(size_t)kk * nmp + which[j]] = b2[(size_t)(kk - k) * which.size() + j];
               });
  }

 protected:
  // The host half of a sequence of Fuse calls that ONE device search answered (the three rules above): view v is one call of the
  // reference - keyframe viewKF[v], or one camera of it when a keyframe of two cameras takes two views in a row
  // (PliORBmatcherTwoCameras) - and best (views x points) holds the search's bestIdx.  The views are replayed in order with
  // :1572-1594; research(v, which, p2, d2) searches the points `which` (their tables p2 / d2) again against the views v..end and
  // writes their entries of best.
  template <class KeyFrameT, class Research>
  void fuseReplay(const std::vector<KeyFrameT*>& viewKF, const std::vector<MapPointT*>& vpMapPoints, std::vector<int>& best,
                  std::vector<int>& nFused, int* pnResearch, Research research) {
    const int nview = (int)viewKF.size(), nmp = (int)vpMapPoints.size();
    std::vector<uint8_t> changed(nmp, 0);
    bool anyChanged = false;
    for (int k = 0; k < nview; ++k) {
      KeyFrameT* pKF = viewKF[k];
      if (anyChanged) {                         // the points whose descriptor a Replace changed, against the views k..end
        std::vector<int> which;
        std::vector<pli_fuse_point> p2;
        std::vector<uint8_t> d2;
        for (int i = 0; i < nmp; ++i)
          if (changed[i]) {
            which.push_back(i);
            p2.push_back(fusePoint(vpMapPoints[i]));
            const size_t at = d2.size();
            d2.resize(at + 32, 0);
            if (p2.back().valid) std::memcpy(&d2[at], vpMapPoints[i]->GetDescriptor().template ptr<uint8_t>(), 32);
            changed[i] = 0;
          }
        research(k, which, p2, d2);
        anyChanged = false;
        if (pnResearch) ++*pnResearch;
      }
      int n = 0;
      for (int i = 0; i < nmp; ++i) {
        MapPointT* pMP = vpMapPoints[i];
        if (!pMP) continue;                                                  // :1424
        if (pMP->isBad()) continue;                                          // :1432
        if (pMP->IsInKeyFrame(pKF)) continue;                                // :1437
        const int bestIdx = best[(size_t)k * nmp + i];
        if (bestIdx < 0) continue;                                           // every other exit, and bestDist > TH_LOW
        MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx);                      // :1572-1594
        if (pMPinKF) {
          if (!pMPinKF->isBad()) {
            MapPointT* survivor = pMPinKF->Observations() > pMP->Observations() ? pMPinKF : pMP;
            uint8_t before[32];
            std::memcpy(before, survivor->GetDescriptor().template ptr<uint8_t>(), 32);
            if (survivor == pMPinKF) pMP->Replace(pMPinKF);
            else pMPinKF->Replace(pMP);
            if (std::memcmp(before, survivor->GetDescriptor().template ptr<uint8_t>(), 32) != 0)
              for (int j = 0; j < nmp; ++j)
                if (vpMapPoints[j] == survivor) { changed[j] = 1; anyChanged = true; }
          }
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        n++;
      }
      nFused[k] = n;
    }
  }

 public:
  // ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint),
  // ORBmatcher.cc:1611-1733 (LoopClosing::SearchAndFuse).  The Sim3 decomposition :1620-1624 runs here (PARITY UNPINNED: OpenCV's
  // arithmetic, by the conventions DESIGN.md §9 lists - Mat::dot sums in double, sqrt of that double rounded to float; Mat / s is
  // (float)(x * (1.0 / s)); -Rcw.t() * tcw is one gemm with alpha = -1, one rounding).  No chi-square gate in this overload.
  // Not batched over keyframes: the caller's own Replace runs between them.
  template <class KeyFrameT>
  int Fuse(KeyFrameT* pKF, cv::Mat Scw, const std::vector<MapPointT*>& vpPoints, float th, std::vector<MapPointT*>& vpReplacePoint) {
    float pose[15];
    sim3Pose(Scw, pose);
    FuseTables T;
    fuseGatherKeyFrame(pKF, pose, T);
    const auto spAlreadyFound = pKF->GetMapPoints();
    const int nmp = (int)vpPoints.size();
    std::vector<pli_fuse_point> pts(nmp);
    std::vector<uint8_t> desc((size_t)nmp * 32, 0), skip(nmp, 0);
    for (int i = 0; i < nmp; ++i) {
      pts[i] = fusePoint(vpPoints[i]);
      if (!pts[i].valid) continue;
      std::memcpy(&desc[(size_t)i * 32], vpPoints[i]->GetDescriptor().template ptr<uint8_t>(), 32);
      skip[i] = spAlreadyFound.count(vpPoints[i]) ? 1 : 0;                  // :1639
    }
    std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("Fuse");
    std::vector<int> best;
    fe->fuseSearch(pts.data(), desc.data(), nmp, 1, T.off.data(), T.kp.data(), T.desc.data(), T.uright.data(), T.pose.data(), skip.data(),
                   T.cam, th, fuseLevelRatio(pKF), false, best);
    int nFused = 0;
    for (int i = 0; i < nmp; ++i) {
      const int bestIdx = best[i];
      if (bestIdx < 0) continue;
      MapPointT* pMP = vpPoints[i];
      MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx);                        // :1717-1728
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
    return nFused;
  }

  // ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched,
  // int th, float ratioHamming), ORBmatcher.cc:473-586 (LoopClosing.cc:656 and :852): the whole loop runs on the device
  // (pli_search_by_projection_sim3, Pinhole::project's arithmetic :519); the decomposition of Scw :483-487 runs here, as in the
  // Sim3 Fuse above.  vpMatched[row] = vpPoints[i] for every row a point took; the return value is the reference's.
  template <class KeyFrameT>
  int SearchByProjection(KeyFrameT* pKF, cv::Mat Scw, const std::vector<MapPointT*>& vpPoints, std::vector<MapPointT*>& vpMatched, int th,
                         float ratioHamming = 1.0) {
    std::vector<std::vector<MapPointT*>> vvpMatched(1);
    vvpMatched[0].swap(vpMatched);
    std::vector<int> vnmatches;
    try {
      sim3Projection(std::vector<KeyFrameT*>(1, pKF), std::vector<cv::Mat>(1, Scw), vpPoints, vvpMatched, th, ratioHamming, 0, vnmatches,
                     [](int, int, int) {});
    } catch (...) {
      vpMatched.swap(vvpMatched[0]);
      throw;
    }
    vpMatched.swap(vvpMatched[0]);
    return vnmatches[0];
  }

  // ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, const vector<KeyFrame*>&
  // vpPointsKFs, vector<MapPoint*>& vpMatched, vector<KeyFrame*>& vpMatchedKF, int th, float ratioHamming), ORBmatcher.cc:588-704
  // (LoopClosing.cc:631): the same search with the projection written out as :631-636 (invz = 1/z; x*invz; fx*x + cx), which rounds
  // differently from Pinhole::project; vpMatchedKF[row] = vpPointsKFs[i] beside vpMatched[row] = vpPoints[i] (:696-697).
  template <class KeyFrameT>
  int SearchByProjection(KeyFrameT* pKF, cv::Mat Scw, const std::vector<MapPointT*>& vpPoints, const std::vector<KeyFrameT*>& vpPointsKFs,
                         std::vector<MapPointT*>& vpMatched, std::vector<KeyFrameT*>& vpMatchedKF, int th, float ratioHamming = 1.0) {
    if (vpPointsKFs.size() < vpPoints.size() || vpMatchedKF.size() < vpMatched.size())
      throw std::logic_error("SearchByProjection: vpPointsKFs / vpMatchedKF are shorter than vpPoints / vpMatched");
    std::vector<std::vector<MapPointT*>> vvpMatched(1);
    vvpMatched[0].swap(vpMatched);
    std::vector<int> vnmatches;
    try {
      sim3Projection(std::vector<KeyFrameT*>(1, pKF), std::vector<cv::Mat>(1, Scw), vpPoints, vvpMatched, th, ratioHamming, 1, vnmatches,
                     [&](int, int row, int i) { vpMatchedKF[row] = vpPointsKFs[i]; });
    } catch (...) {
      vpMatched.swap(vvpMatched[0]);
      throw;
    }
    vpMatched.swap(vvpMatched[0]);
    return vnmatches[0];
  }

  // (not in the reference) The loop of LoopClosing.cc:698-730 - FindMatchesByProjection (:852: th = 3, ratio = 1.5) for up to five
  // covisibles of the current keyframe, each with its own Scw, against ONE list of points - with ONE device search.  vvpMatched[k]
  // is keyframe k's vpMatched (sized by the caller, as :851 does; non-null entries are occupied rows and already-found points),
  // vnmatches[k] the reference's return value.  The pairs do not share state, so every result equals the single call's.  The
  // reference's loop stops after three valid keyframes; this form has searched all of them by then.
  template <class KeyFrameT>
  void SearchByProjection(const std::vector<KeyFrameT*>& vpKFs, const std::vector<cv::Mat>& vScw, const std::vector<MapPointT*>& vpPoints,
                          std::vector<std::vector<MapPointT*>>& vvpMatched, int th, float ratioHamming, std::vector<int>& vnmatches) {
    sim3Projection(vpKFs, vScw, vpPoints, vvpMatched, th, ratioHamming, 0, vnmatches, [](int, int, int) {});
  }

  // ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th, const
  // int ORBdist), ORBmatcher.cc:2325-2447 (Tracking::Relocalization, Tracking.cc:4290 and :4304): the whole loop, the rotation
  // histogram and ComputeThreeMaxima run on the device (pli_search_by_projection_reloc); Rcw, tcw and Ow = -Rcw.t()*tcw (:2329-2331)
  // are the reference's own cv::Mat expressions, run here.  CurrentFrame.mvpMapPoints[row] = vpMPs[i] for every row a point holds
  // after the rotation filter; the return value is the reference's.  FrameT needs mTcw, N, Nleft, mvKeysUn, mDescriptors,
  // mvpMapPoints, fx, fy, cx, cy, mbf, mnMinX .. mnMaxY, mnScaleLevels and mfLogScaleFactor; KeyFrameT mpCamera2, mvKeysUn and
  // GetMapPointMatches().
  template <class KeyFrameT>
  int SearchByProjection(FrameT& CurrentFrame, KeyFrameT* pKF, const std::set<MapPointT*>& sAlreadyFound, const float th, const int ORBdist) {
    std::vector<std::vector<MapPointT*>> vvpMapPoints;
    std::vector<int> vnmatches;
    relocProjection(CurrentFrame, std::vector<KeyFrameT*>(1, pKF), std::vector<cv::Mat>(1, CurrentFrame.mTcw),
                    std::vector<const std::set<MapPointT*>*>(1, &sAlreadyFound),
                    std::vector<const std::vector<MapPointT*>*>(1, &CurrentFrame.mvpMapPoints), th, ORBdist, vvpMapPoints, vnmatches);
    CurrentFrame.mvpMapPoints.swap(vvpMapPoints[0]);                         // :2405, :2439
    return vnmatches[0];
  }

  // (not in the reference) The same search for several candidates of Tracking::Relocalization with ONE device call, for an
  // integrator who runs PnP and the pose optimisation for every candidate first: candidate k has its own pose vTcw[k] (what
  // CurrentFrame.mTcw would be at :4290), its own sAlreadyFound and its own state of mvpMapPoints at entry (vvpEntry[k], N
  // entries).  vvpMapPoints[k] is what CurrentFrame.mvpMapPoints would hold after the single call, vnmatches[k] its return value;
  // CurrentFrame itself is not written.  The candidates do not share state, so every result equals the single call's.  The
  // reference's loop stops at the first candidate with enough inliers (bMatch); this form has searched the later ones by then.
  template <class KeyFrameT>
  void SearchByProjection(const FrameT& CurrentFrame, const std::vector<KeyFrameT*>& vpKFs, const std::vector<cv::Mat>& vTcw,
                          const std::vector<std::set<MapPointT*>>& vsAlreadyFound, const std::vector<std::vector<MapPointT*>>& vvpEntry,
                          const float th, const int ORBdist, std::vector<std::vector<MapPointT*>>& vvpMapPoints,
                          std::vector<int>& vnmatches) {
    if (vsAlreadyFound.size() != vpKFs.size() || vvpEntry.size() != vpKFs.size())
      throw std::logic_error("SearchByProjection: one sAlreadyFound and one state of mvpMapPoints per candidate");
    std::vector<const std::set<MapPointT*>*> found;
    std::vector<const std::vector<MapPointT*>*> entry;
    for (size_t k = 0; k < vpKFs.size(); ++k) { found.push_back(&vsAlreadyFound[k]); entry.push_back(&vvpEntry[k]); }
    relocProjection(CurrentFrame, vpKFs, vTcw, found, entry, th, ORBdist, vvpMapPoints, vnmatches);
  }

  // ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12, int
  // windowSize), ORBmatcher.cc:706-821 (Tracking::MonocularInitialization, Tracking.cc:2109-2110): the windows, the ordered walk
  // with its evictions, the rotation histogram and ComputeThreeMaxima run on the device (pli_search_for_initialization);
  // vnMatches12 is the reference's, vbPrevMatched gets the update :816-818, the return value is the reference's.  Frames of one
  // camera only (Nleft == -1).  FrameT needs Nleft, mvKeysUn, mDescriptors and mnMinX .. mnMaxY.
  int SearchForInitialization(FrameT& F1, FrameT& F2, std::vector<cv::Point2f>& vbPrevMatched, std::vector<int>& vnMatches12,
                              int windowSize = 10) {
    if (F1.Nleft != -1 || F2.Nleft != -1) throw std::logic_error("SearchForInitialization: frames of two cameras are not covered");
    const size_t n1 = F1.mvKeysUn.size(), n2 = F2.mvKeysUn.size();
    if (vbPrevMatched.size() != n1) throw std::logic_error("SearchForInitialization: vbPrevMatched needs one point per keypoint of F1");
    std::vector<pli_keypoint> kp1(n1), kp2(n2);
    std::vector<float> prev(2 * n1);
    for (size_t i = 0; i < n1; ++i) {
      kp1[i] = pli_detail::keypoint(F1.mvKeysUn[i]);
      prev[2 * i] = vbPrevMatched[i].x;
      prev[2 * i + 1] = vbPrevMatched[i].y;
    }
    for (size_t i = 0; i < n2; ++i) kp2[i] = pli_detail::keypoint(F2.mvKeysUn[i]);
    std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("SearchForInitialization");
    const int nmatches = fe->searchForInitialization(kp1, F1.mDescriptors.data, prev.data(), kp2, F2.mDescriptors.data, F2.mnMinX,
                                                     F2.mnMaxX, F2.mnMinY, F2.mnMaxY, windowSize, mfNNratio,
                                                     mbCheckOrientation, vnMatches12);
    for (size_t i1 = 0; i1 < n1; ++i1)                                       // :816-818
      if (vnMatches12[i1] >= 0) vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt;
    return nmatches;
  }

  // ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th, const bool bFarPoints, const
  // float thFarPoints), ORBmatcher.cc:44-143 for a frame of one camera or rectified stereo (F.Nleft == -1;
  // Tracking::SearchLocalPoints, Tracking.cc:3854): the gates :53-62, RadiusByViewingCos (:216-222) and the window radius are the
  // reference's own expressions, run here; the windows, best and second-best, TH_HIGH and the ratio test run on the device
  // (pli_search_local_map).  F.mvpMapPoints[bestIdx] = pMP for every row taken; the return value is the reference's.
  // One case is refused: a point in view that is not bad and has Observations() == 0.  The reference would not close the row such
  // a point takes (:89-91 reads Observations() of the row's point), the device closes every row taken.
  // FrameT needs N, Nleft, mvKeysUn, mDescriptors, mvuRight, mvpMapPoints, mvScaleFactors and mnMinX .. mnMaxY;
  // MapPointT mbTrackInView, mTrackDepth, isBad(), mnTrackScaleLevel, mTrackViewCos, mTrackProjX / Y / XR, GetDescriptor() and
  // Observations().
  int SearchByProjection(FrameT& F, const std::vector<MapPointT*>& vpMapPoints, const float th = 3, const bool bFarPoints = false,
                         const float thFarPoints = 50.0f) {
    if (F.Nleft != -1) throw std::logic_error("SearchByProjection(F, vpMapPoints): frames of two cameras are not covered");
    const bool bFactor = th != 1.0;
    const size_t nq = vpMapPoints.size();
    std::vector<pli_proj_query> q(nq);
    std::vector<uint8_t> qdesc(nq * 32, 0);
    for (size_t iMP = 0; iMP < nq; ++iMP) {
      pli_proj_query& Q = q[iMP];
      std::memset(&Q, 0, sizeof(Q));
      MapPointT* pMP = vpMapPoints[iMP];
      if (!pMP->mbTrackInView) continue;                                     // :53, :62 (no right camera)
      if (bFarPoints && pMP->mTrackDepth > thFarPoints) continue;            // :56
      if (pMP->isBad()) continue;                                            // :59
      if (pMP->Observations() <= 0)
        throw std::logic_error("SearchByProjection(F, vpMapPoints): a point in view without observations is not covered");
      const int nPredictedLevel = pMP->mnTrackScaleLevel;
      float r = pMP->mTrackViewCos > 0.998 ? 2.5 : 4.0;                      // RadiusByViewingCos :216-222
      if (bFactor) r *= th;
      Q.u = pMP->mTrackProjX;
      Q.v = pMP->mTrackProjY;
      Q.radius = r * F.mvScaleFactors[nPredictedLevel];                      // :73, :96
      Q.ur = pMP->mTrackProjXR;
      Q.min_level = nPredictedLevel - 1;
      Q.max_level = nPredictedLevel;
      Q.valid = 1;
      const cv::Mat dMP = pMP->GetDescriptor();
      std::memcpy(&qdesc[iMP * 32], dMP.ptr<uint8_t>(), 32);
    }
    const int M = F.N;
    std::vector<pli_keypoint> kp((size_t)M);
    std::vector<uint8_t> occupied((size_t)M, 0);
    for (int j = 0; j < M; ++j) {
      kp[j] = pli_detail::keypoint(F.mvKeysUn[j]);
      if (F.mvpMapPoints[j] && F.mvpMapPoints[j]->Observations() > 0) occupied[j] = 1;      // :89-91
    }
    std::shared_ptr<pli::Frontend> fe = pli_detail::deviceContext("SearchByProjection(F, vpMapPoints)");
    std::vector<int> best;
    const int nmatches = fe->searchLocalMap(q, qdesc.data(), kp, F.mDescriptors.data, F.mvuRight.data(), occupied.data(), F.mnMinX,
                                            F.mnMaxX, F.mnMinY, F.mnMaxY, mfNNratio, best);
    for (size_t iMP = 0; iMP < nq; ++iMP)
      if (best[iMP] >= 0) F.mvpMapPoints[best[iMP]] = vpMapPoints[iMP];      // :130
    return nmatches;
  }

  // the level_ratio table the Fuse adapters hand to pli_fuse_search (tests read it)
  template <class KeyFrameT>
  const std::vector<float>& fuseLevelRatio(KeyFrameT* pKF) {
    const int nlevels = pKF->mnScaleLevels;
    const float logSf = pKF->mfLogScaleFactor;
    if (mvFuseLevelRatio.empty() || mnFuseLevels != nlevels || mfFuseLogSf != logSf) {
      // MapPoint::PredictScale, MapPoint.cc:457-461, as MapPoint.cc compiles it (it is `using namespace std`, so log(float) is
      // whichever overload this toolchain selects there)
      mvFuseLevelRatio = pli::Frontend::fuseLevelRatio(nlevels, [nlevels, logSf](float ratio) {
        using namespace std;
        if (!(ratio > 0.0f)) return 0;
        if (std::isinf(ratio)) return nlevels - 1;
        int nScale = ceil(log(ratio) / logSf);
        if (nScale < 0) nScale = 0;
        else if (nScale >= nlevels) nScale = nlevels - 1;
        return nScale;
      });
      mnFuseLevels = nlevels;
      mfFuseLogSf = logSf;
    }
    return mvFuseLevelRatio;
  }

  // Rcw (row major), tcw and Ow = -Rcw.t()*tcw of a frame pose, the reference's own cv::Mat expressions ORBmatcher.cc:2329-2331;
  // tests read it
  static void relocPose(const cv::Mat& Tcw, float pose[15]) {
    const cv::Mat Rcw = Tcw.rowRange(0, 3).colRange(0, 3);
    const cv::Mat tcw = Tcw.rowRange(0, 3).col(3);
    const cv::Mat Ow = -Rcw.t() * tcw;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) pose[i * 3 + j] = Rcw.template at<float>(i, j);
    for (int i = 0; i < 3; ++i) { pose[9 + i] = tcw.template at<float>(i); pose[12 + i] = Ow.template at<float>(i); }
  }

  // The decomposition of a Sim3 matrix, ORBmatcher.cc:483-487 / :1620-1624, into Rcw (row major), tcw, Ow; tests read it (PARITY UNPINNED:
  // OpenCV's arithmetic, by the conventions DESIGN.md §9 lists - Mat::dot sums in double, sqrt of that double rounded to float;
  // Mat / s is (float)(x * (1.0 / s)); -Rcw.t() * tcw is one gemm with alpha = -1, one rounding)
  static void sim3Pose(const cv::Mat& Scw, float pose[15]) {
    double dd = 0.0;
    for (int j = 0; j < 3; ++j) dd += (double)Scw.template at<float>(0, j) * (double)Scw.template at<float>(0, j);
    const float scw = (float)std::sqrt(dd);
    const double inv = 1.0 / (double)scw;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) pose[i * 3 + j] = (float)((double)Scw.template at<float>(i, j) * inv);
      pose[9 + i] = (float)((double)Scw.template at<float>(i, 3) * inv);
    }
    for (int i = 0; i < 3; ++i)
      pose[12 + i] = (float)(-1.0 * ((double)pose[i] * (double)pose[9] + (double)pose[3 + i] * (double)pose[10] + (double)pose[6 + i] * (double)pose[11]));
  }

 protected:
  // the keyframe side of both SearchByBoW forms; valid = the map point is set and not bad
  struct BowTable : pli_detail::KfTable {
    std::vector<float> angle;
    std::vector<uint8_t> valid;
  };
  template <class KeyFrameT>
  static void bowGatherKeyFrame(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const char* what, BowTable& T) {
    const int n = pKF->N;
    pli_detail::appendNodes(T, pKF->mFeatVec, n, what);
    pli_detail::appendDescriptors(T, pKF->mDescriptors, n);
    for (int i = 0; i < n; ++i) {
      MapPointT* pMP = vpMapPoints[i];
      T.valid.push_back(pMP && !pMP->isBad() ? 1 : 0);
      T.angle.push_back(pKF->mvKeysUn[i].angle);
    }
  }
  // What the three SearchByProjection(KeyFrame, Scw, ...) forms share: the tables, one device search, vpMatched written from
  // row_point.  onMatch(pair, row, point) runs for every row taken.
  template <class KeyFrameT, class OnMatch>
  void sim3Projection(const std::vector<KeyFrameT*>& vpKFs, const std::vector<cv::Mat>& vScw, const std::vector<MapPointT*>& vpPoints,
                      std::vector<std::vector<MapPointT*>>& vvpMatched, int th, float ratioHamming, int projectForm,
                      std::vector<int>& vnmatches, OnMatch onMatch) {
    const int npair = (int)vpKFs.size(), nmp = (int)vpPoints.size();
    if (vScw.size() != vpKFs.size() || vvpMatched.size() != vpKFs.size())
      throw std::logic_error("SearchByProjection: one Scw and one vpMatched per keyframe");
    vnmatches.assign(npair, 0);
    if (npair == 0) return;
    FuseTables T;
    std::vector<uint8_t> occupied, skip((size_t)npair * nmp, 0);
    std::vector<pli_fuse_point> pts(nmp);
    std::vector<uint8_t> desc((size_t)nmp * 32, 0);
    for (int i = 0; i < nmp; ++i) {
      pts[i] = fusePoint(vpPoints[i]);                                       // isBad() :501
      if (pts[i].valid) std::memcpy(&desc[(size_t)i * 32], vpPoints[i]->GetDescriptor().template ptr<uint8_t>(), 32);
    }
    for (int k = 0; k < npair; ++k) {
      KeyFrameT* pKF = vpKFs[k];
      if (pKF->NLeft != -1) throw std::logic_error("SearchByProjection: a keyframe of two cameras (NLeft != -1) is not supported");
      if (pKF->mpCamera2) throw std::logic_error("SearchByProjection: a keyframe with mpCamera2 is not supported");
      if ((int)vvpMatched[k].size() < pKF->N) throw std::logic_error("SearchByProjection: vpMatched is shorter than the keyframe");
      float pose[15];
      sim3Pose(vScw[k], pose);
      fuseGatherKeyFrame(pKF, pose, T);
      const std::set<MapPointT*> spAlreadyFound(vvpMatched[k].begin(), vvpMatched[k].end());      // :490-491
      for (int i = 0; i < pKF->N; ++i) occupied.push_back(vvpMatched[k][i] ? 1 : 0);
      for (int i = 0; i < nmp; ++i)
        if (vpPoints[i] && spAlreadyFound.count(vpPoints[i])) skip[(size_t)k * nmp + i] = 1;
    }
    std::vector<int> rowPoint;
    pli_detail::deviceContext("SearchByProjection")
        ->searchByProjectionSim3(pts.data(), desc.data(), nmp, npair, T.off.data(), T.kp.data(), T.desc.data(), T.pose.data(), skip.data(),
                                 occupied.data(), T.cam, (float)th, fuseLevelRatio(vpKFs[0]), ratioHamming, projectForm, rowPoint,
                                 vnmatches);
    for (int k = 0; k < npair; ++k)
      for (int r = T.off[k]; r < T.off[k + 1]; ++r) {
        const int i = rowPoint[r];
        if (i < 0) continue;
        vvpMatched[k][r - T.off[k]] = vpPoints[i];                            // :579 / :696
        onMatch(k, r - T.off[k], i);
      }
  }
  // What the two SearchByProjection(Frame, KeyFrame, sAlreadyFound, ...) forms share: the candidates' point lists, the frame's
  // table, one device search; vvpMapPoints[k] = the entry state with the rows candidate k's points hold written over it.
  template <class KeyFrameT>
  void relocProjection(const FrameT& F, const std::vector<KeyFrameT*>& vpKFs, const std::vector<cv::Mat>& vTcw,
                       const std::vector<const std::set<MapPointT*>*>& vsFound,
                       const std::vector<const std::vector<MapPointT*>*>& vEntry, float th, int ORBdist,
                       std::vector<std::vector<MapPointT*>>& vvpMapPoints, std::vector<int>& vnmatches) {
    const int ncand = (int)vpKFs.size(), nf = F.N;
    if (vTcw.size() != vpKFs.size()) throw std::logic_error("SearchByProjection: one Tcw per candidate");
    if (F.Nleft != -1) throw std::logic_error("SearchByProjection: a frame of two cameras (Nleft != -1) is not supported");
    vnmatches.assign(ncand, 0);
    vvpMapPoints.assign(ncand, std::vector<MapPointT*>());
    if (ncand == 0) return;
    std::vector<std::vector<MapPointT*>> vvpMPs(ncand);
    std::vector<int32_t> off(1, 0);
    std::vector<pli_fuse_point> pts;
    std::vector<uint8_t> desc, occupied((size_t)ncand * nf, 0);
    std::vector<float> angle, pose;
    for (int k = 0; k < ncand; ++k) {
      KeyFrameT* pKF = vpKFs[k];
      if (pKF->mpCamera2) throw std::logic_error("SearchByProjection: a keyframe with mpCamera2 is not supported");
      if ((int)vEntry[k]->size() < nf) throw std::logic_error("SearchByProjection: mvpMapPoints is shorter than the frame");
      float T[15];
      relocPose(vTcw[k], T);
      pose.insert(pose.end(), T, T + 15);
      vvpMPs[k] = pKF->GetMapPointMatches();                                 // :2339
      const std::vector<MapPointT*>& vpMPs = vvpMPs[k];
      if (vpMPs.size() > pKF->mvKeysUn.size()) throw std::logic_error("SearchByProjection: more map points than keypoints in a keyframe");
      for (size_t i = 0; i < vpMPs.size(); ++i) {
        pli_fuse_point P = fusePoint(vpMPs[i]);                              // pMP, !isBad() :2345-2347
        if (P.valid && vsFound[k]->count(vpMPs[i])) P.valid = 0;             // !sAlreadyFound.count(pMP)
        pts.push_back(P);
        desc.insert(desc.end(), 32, (uint8_t)0);
        if (P.valid) std::memcpy(&desc[desc.size() - 32], vpMPs[i]->GetDescriptor().template ptr<uint8_t>(), 32);
        angle.push_back(pKF->mvKeysUn[i].angle);                             // :2410
      }
      off.push_back((int32_t)pts.size());
      for (int j = 0; j < nf; ++j) occupied[(size_t)k * nf + j] = (*vEntry[k])[j] ? 1 : 0;      // :2389
    }
    std::vector<pli_keypoint> kp((size_t)nf);
    for (int j = 0; j < nf; ++j) kp[j] = pli_detail::keypoint(F.mvKeysUn[j]);
    const pli_fuse_camera cam = {F.fx, F.fy, F.cx, F.cy, F.mbf, (float)F.mnMinX, (float)F.mnMaxX, (float)F.mnMinY, (float)F.mnMaxY};
    std::vector<int> rowPoint;
    pli_detail::deviceContext("SearchByProjection")
        ->searchByProjectionReloc(ncand, off.data(), pts.data(), desc.data(), angle.data(), pose.data(), kp.data(),
                                  nf > 0 ? F.mDescriptors.template ptr<uint8_t>() : nullptr, nf, occupied.data(), cam, th,
                                  fuseLevelRatio(&F), ORBdist, mbCheckOrientation, rowPoint, vnmatches);
    for (int k = 0; k < ncand; ++k) {
      vvpMapPoints[k] = *vEntry[k];
      for (int r = 0; r < nf; ++r) {
        const int i = rowPoint[(size_t)k * nf + r];
        if (i >= 0) vvpMapPoints[k][r] = vvpMPs[k][i];                       // :2405, less the rows :2439 gives back
      }
    }
  }
  struct FuseTables : pli_detail::KfTable {
    std::vector<pli_keypoint> kp;
    std::vector<float> uright, pose;
    pli_fuse_camera cam;
    bool haveCam = false;
  };
  template <class KeyFrameT>
  static void fuseGatherKeyFrame(KeyFrameT* pKF, const float pose[15], FuseTables& T) {
    if (pKF->NLeft != -1) throw std::logic_error("Fuse: a keyframe of two cameras (NLeft != -1) is not supported");
    const pli_fuse_camera cam = {pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf, (float)pKF->mnMinX, (float)pKF->mnMaxX, (float)pKF->mnMinY,
                                 (float)pKF->mnMaxY};
    if (T.haveCam && std::memcmp(&cam, &T.cam, sizeof cam) != 0)
      throw std::logic_error("Fuse: the target keyframes of one call must share the camera and the image bounds");
    T.cam = cam;
    T.haveCam = true;
    const int n = pKF->N;
    pli_detail::appendDescriptors(T, pKF->mDescriptors, n);
    for (int i = 0; i < n; ++i) {
      T.kp.push_back(pli_detail::keypoint(pKF->mvKeysUn[i]));
      T.uright.push_back(pKF->mvuRight[i]);
    }
    T.pose.insert(T.pose.end(), pose, pose + 15);
  }
  static pli_fuse_point fusePoint(MapPointT* pMP) {
    pli_fuse_point P = {};
    if (!pMP || pMP->isBad()) return P;
    const cv::Mat p = pMP->GetWorldPos(), nrm = pMP->GetNormal();
    for (int i = 0; i < 3; ++i) { P.pos[i] = p.template at<float>(i); P.normal[i] = nrm.template at<float>(i); }
    P.min_dist_inv = pMP->GetMinDistanceInvariance();
    P.max_dist_inv = pMP->GetMaxDistanceInvariance();
    P.max_dist = pMP->GetMaxDistance();
    P.valid = (std::isfinite(P.max_dist) && P.max_dist > 0.f) ? 1 : 0;      // (the reference converts a NaN to int there)
    return P;
  }

  float mfNNratio;
  bool mbCheckOrientation;
  std::vector<float> mvFuseLevelRatio;
  int mnFuseLevels = 0;
  float mfFuseLogSf = 0.f;
};

}  // namespace ORB_SLAM3
