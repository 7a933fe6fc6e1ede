// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:300-365) and MapLine::ComputeDistinctiveDescriptors
// (src/MapLine.cc:246-317) for a whole list of features in ONE device call (pli_distinctive_descriptors, include/pli_frontend.h).
// The reference runs them one feature at a time on the local-mapping thread: LocalMapping.cc:267-286 (every map point of a new
// keyframe), :780-793 (every map point of the current keyframe after Fuse), LoopClosing.cc:1012, MapPoint.cc:268, MapLine.cc:216.
//
// What stays on the host is the reference's own walk, statement by statement: the bad-feature test (:309-310), the copy of
// GetObservations() and its iteration in the map's own order (:319-325), the bad-keyframe test (:323) and the two early returns that
// leave mDescriptor untouched (:314-315 no observations, :327-328 no descriptor left).  Groups of one or two descriptors are answered
// here (every median is 0: BestIdx = 0) and are not uploaded; all other groups go to the device together.
//
// Batching is exact: a feature's answer depends on its own observations alone.  The order of the observations is the order of a
// std::map<KeyFrame*, size_t>, that is, of heap addresses; ties for the least median are therefore resolved as the reference
// resolves them in the same process, and not reproducibly across runs — the reference behaves the same way.
//
// The tree's MapPoint / MapLine need one setter, which the reference lacks:
//   void SetDescriptor(const cv::Mat& d) { unique_lock<mutex> lock(mMutexFeatures); mDescriptor = d.clone(); }
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>
#include "orbslam_adapters.hpp"

namespace ORB_SLAM3 {

// features: the list as the call site holds it (NULL and isBad() entries are skipped, as the call sites' own `if` and :309 do);
// rowOf(pKF, idx) -> const uint8_t*: the 32 bytes of the keyframe's descriptor row idx; apply(feature, pKF, idx): stores the chosen
// observation's row as the feature's descriptor.  Returns the number of groups that went to the device (0: no device call was made).
template <class FeatureT, class RowOf, class ApplyT>
int PliComputeDistinctiveDescriptors(const std::vector<FeatureT*>& features, RowOf rowOf, ApplyT apply) {
  typedef typename std::decay<decltype(std::declval<FeatureT>().GetObservations())>::type ObservationsT;
  typedef typename ObservationsT::key_type KeyFramePtr;
  struct Group { FeatureT* feature; size_t first, n; };                  // rows first .. first + n of `rows`
  std::vector<Group> groups;
  std::vector<std::pair<KeyFramePtr, size_t>> rows;                       // vDescriptors of every feature, one after another
  for (FeatureT* f : features) {
    if (!f || f->isBad()) continue;                                       // (:309-310)
    const ObservationsT observations = f->GetObservations();              // (:311: a copy, taken under the feature's mutex)
    if (observations.empty()) continue;                                   // (:314-315)
    const size_t first = rows.size();
    for (typename ObservationsT::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; ++mit) {
      KeyFramePtr pKF = mit->first;
      if (!pKF->isBad()) rows.emplace_back(pKF, (size_t)mit->second);     // (:323-324)
    }
    if (rows.size() == first) continue;                                   // (:327-328)
    groups.push_back(Group{f, first, rows.size() - first});
  }
  std::vector<uint8_t> desc;
  std::vector<int32_t> off(1, 0);
  std::vector<size_t> sent;                                               // the groups of three or more rows
  for (size_t g = 0; g < groups.size(); ++g) {
    const Group& G = groups[g];
    if (G.n <= 2) continue;
    sent.push_back(g);
    const size_t at = desc.size();
    desc.resize(at + G.n * 32);
    for (size_t i = 0; i < G.n; ++i) std::memcpy(&desc[at + i * 32], rowOf(rows[G.first + i].first, rows[G.first + i].second), 32);
    off.push_back((int32_t)(desc.size() / 32));
  }
  std::vector<int> best, bestMedian;
  if (!sent.empty()) pli_detail::deviceContext("ComputeDistinctiveDescriptors")->distinctiveDescriptors(desc, off, best, bestMedian);
  size_t s = 0;
  for (size_t g = 0; g < groups.size(); ++g) {
    const Group& G = groups[g];
    const size_t bestIdx = G.n <= 2 ? 0 : (size_t)best[s++];              // N = 1, 2: every median is 0, the first row wins (:354)
    apply(G.feature, rows[G.first + bestIdx].first, rows[G.first + bestIdx].second);      // (:363)
  }
  return (int)sent.size();
}

// MapPoint::ComputeDistinctiveDescriptors of every point of the list: pKF->mDescriptors.row(idx) (MapPoint.cc:324)
template <class MapPointT>
int PliComputeDistinctiveDescriptorsOfPoints(const std::vector<MapPointT*>& vpMapPoints) {
  return PliComputeDistinctiveDescriptors(
      vpMapPoints, [](const auto& pKF, size_t idx) { return pKF->mDescriptors.template ptr<uint8_t>((int)idx); },
      [](MapPointT* pMP, const auto& pKF, size_t idx) { pMP->SetDescriptor(pKF->mDescriptors.row((int)idx)); });
}

// MapLine::ComputeDistinctiveDescriptors of every line of the list: pKF->mDescriptors_l.row(idx) (MapLine.cc:271)
template <class MapLineT>
int PliComputeDistinctiveDescriptorsOfLines(const std::vector<MapLineT*>& vpMapLines) {
  return PliComputeDistinctiveDescriptors(
      vpMapLines, [](const auto& pKF, size_t idx) { return pKF->mDescriptors_l.template ptr<uint8_t>((int)idx); },
      [](MapLineT* pML, const auto& pKF, size_t idx) { pML->SetDescriptor(pKF->mDescriptors_l.row((int)idx)); });
}

}  // namespace ORB_SLAM3
