// Drop-in for ORB_SLAM3::KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc): the keyframes' BowVectors live on
// the device (pli_kfdb, include/pli_frontend.h), and the two live queries — DetectRelocalizationCandidates (Tracking.cc:4184) and
// DetectNBestCandidates (LoopClosing.cc:395) — make ONE pli_kfdb_query call each: the shared-word count, the first shared word and
// DBoW2's L1 score of EVERY keyframe come back from one launch.  Everything after that is the reference's small, ordered, stateful
// host logic, replayed here statement by statement on the tree's own KeyFrame members, so that the candidates come back in the
// reference's order and every member is left as the reference leaves it — its quirks included:
//   * mRelocScore / mPlaceRecognitionScore are written only above minCommonWords but read for every neighbour whose query id
//     matches: a score of an earlier query (or the constructor's 0) is added;
//   * DetectNBestCandidates never pushes a keyframe of GetConnectedKeyFrames() and never sets its query id; its word counter is
//     reset at every shared word and ends at 1; it takes no part in maxCommonWords;
//   * a keyframe whose stored query id already equals the query's (the members start at 0, and ids start at 0) is not pushed, and
//     its word counter goes on from the stale value;
//   * DetectRelocalizationCandidates tests the map after the 0.75f gate and before the duplicate test;
//   * DetectNBestCandidates fills each of the two vectors up to nNumCandidates, skips merge candidates of a bad map, and enters a
//     keyframe into the duplicate set even when its vector was already full.
// Deliberate differences, both where the reference misbehaves: a bad keyframe in the sorted list of DetectNBestCandidates (the
// reference's `continue` at :929 advances nothing: it hangs) and a second add() of a keyframe that is still in the database (the
// reference would list it twice; no call site does it) throw std::logic_error.
// erase() leaves mBowVec_l alone: the reference's add() never fills the line inverted file, so that half of its erase() finds nothing.
// Not provided (no call site): DetectLoopCandidates, DetectCandidates, DetectBestCandidates, the two ...WithLine forms, PreSave,
// PostLoad, serialize.  The device's three numbers per keyframe are all they would need.
//
// Inside the PLI-SLAM tree: `using KeyFrameDatabase = ORB_SLAM3::PliKeyFrameDatabase<KeyFrame, Frame, Map>;`.
// Thread safety: the reference guards its inverted file with one mutex; so does this class (tables and members), and the device
// calls hold the context's lock.
#pragma once
#include <algorithm>
#include <list>
#include <mutex>
#include <set>
#include <stdexcept>
#include <unordered_map>
#include <utility>
#include <vector>
#include "pli_cpp.hpp"

namespace ORB_SLAM3 {

template <class KeyFrameT, class FrameT, class MapT>
class PliKeyFrameDatabase {
 public:
  // KeyFrameDatabase(const ORBVocabulary& voc) / (voc, voc_l): the vocabularies are not read (the BowVectors arrive transformed)
  explicit PliKeyFrameDatabase(pli::Frontend& fe) : fe_(fe) { pli::check(pli_kfdb_create(fe_.handle(), &db_)); }
  template <class VocT>
  PliKeyFrameDatabase(pli::Frontend& fe, const VocT&) : PliKeyFrameDatabase(fe) {}
  template <class VocT, class LineVocT>
  PliKeyFrameDatabase(pli::Frontend& fe, const VocT&, const LineVocT&) : PliKeyFrameDatabase(fe) {}
  ~PliKeyFrameDatabase() { pli_kfdb_destroy(db_); }
  PliKeyFrameDatabase(const PliKeyFrameDatabase&) = delete;
  PliKeyFrameDatabase& operator=(const PliKeyFrameDatabase&) = delete;

  void add(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    if (slotOf_.count(pKF)) throw std::logic_error("PliKeyFrameDatabase::add: the keyframe is already in the database");
    std::vector<uint32_t> w;
    std::vector<double> v;
    flatten(pKF->mBowVec, w, v);
    int32_t slot = -1;
    pli::check(pli_kfdb_add(fe_.handle(), db_, w.data(), v.data(), (int32_t)w.size(), &slot));
    if ((size_t)slot >= kf_.size()) { kf_.resize((size_t)slot + 1, nullptr); seq_.resize((size_t)slot + 1, 0); }
    kf_[slot] = pKF;
    seq_[slot] = nextSeq_++;
    slotOf_[pKF] = slot;
  }

  void erase(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    eraseLocked(pKF);
  }

  void clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    pli::check(pli_kfdb_clear(fe_.handle(), db_));
    kf_.clear(); seq_.clear(); slotOf_.clear();
  }

  void clearMap(MapT* pMap) {
    std::unique_lock<std::mutex> lock(mMutex);
    for (size_t s = 0; s < kf_.size(); ++s)
      if (kf_[s] && kf_[s]->GetMap() == pMap) eraseLocked(kf_[s]);
  }

  // KeyFrameDatabase.cc:977-1089
  std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F, MapT* pMap) {
    std::list<KeyFrameT*> lKFsSharingWords;
    std::vector<float> vScores;                                // mpVoc->score(F->mBowVec, pKFi->mBowVec) per entry of the list, as the float it is stored in
    {
      std::unique_lock<std::mutex> lock(mMutex);
      std::vector<int32_t> common;
      std::vector<double> score;
      for (int32_t s : query(F->mBowVec, common, score)) {
        KeyFrameT* pKFi = kf_[s];
        if (pKFi->mnRelocQuery != F->mnId) {
          pKFi->mnRelocWords = 0;
          pKFi->mnRelocQuery = F->mnId;
          lKFsSharingWords.push_back(pKFi);
          vScores.push_back((float)score[s]);
        }
        pKFi->mnRelocWords += common[s];
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrameT*>();

    int maxCommonWords = 0;
    for (KeyFrameT* k : lKFsSharingWords)
      if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
    int minCommonWords = maxCommonWords * 0.8f;

    std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
    size_t nth = 0;
    for (KeyFrameT* pKFi : lKFsSharingWords) {
      float si = vScores[nth++];
      if (pKFi->mnRelocWords > minCommonWords) {
        pKFi->mRelocScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();

    std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
    float bestAccScore = 0;
    for (auto it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); ++it) {
      KeyFrameT* pKFi = it->second;
      std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrameT* pBestKF = pKFi;
      for (KeyFrameT* pKF2 : vpNeighs) {
        if (pKF2->mnRelocQuery != F->mnId) continue;
        accScore += pKF2->mRelocScore;                       // (possibly a score of an earlier query)
        if (pKF2->mRelocScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }

    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrameT*> spAlreadyAddedKF;
    std::vector<KeyFrameT*> vpRelocCandidates;
    vpRelocCandidates.reserve(lAccScoreAndMatch.size());
    for (auto it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end(); ++it) {
      const float& si = it->first;
      if (si > minScoreToRetain) {
        KeyFrameT* pKFi = it->second;
        if (pKFi->GetMap() != pMap) continue;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpRelocCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    return vpRelocCandidates;
  }

  // KeyFrameDatabase.cc:806-974
  void DetectNBestCandidates(KeyFrameT* pKF, std::vector<KeyFrameT*>& vpLoopCand, std::vector<KeyFrameT*>& vpMergeCand, int nNumCandidates) {
    std::list<KeyFrameT*> lKFsSharingWords;
    std::vector<float> vScores;
    std::set<KeyFrameT*> spConnectedKF;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      spConnectedKF = pKF->GetConnectedKeyFrames();
      std::vector<int32_t> common;
      std::vector<double> score;
      for (int32_t s : query(pKF->mBowVec, common, score)) {
        KeyFrameT* pKFi = kf_[s];
        if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) {
          if (spConnectedKF.count(pKFi)) {                   // reset at every shared word, never pushed, query id never set
            pKFi->mnPlaceRecognitionWords = 1;
            continue;
          }
          pKFi->mnPlaceRecognitionWords = 0;
          pKFi->mnPlaceRecognitionQuery = pKF->mnId;
          lKFsSharingWords.push_back(pKFi);
          vScores.push_back((float)score[s]);
        }
        pKFi->mnPlaceRecognitionWords += common[s];
      }
    }
    if (lKFsSharingWords.empty()) return;

    int maxCommonWords = 0;
    for (KeyFrameT* k : lKFsSharingWords)
      if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;
    int minCommonWords = maxCommonWords * 0.8f;

    std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
    size_t nth = 0;
    for (KeyFrameT* pKFi : lKFsSharingWords) {
      float si = vScores[nth++];
      if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
        pKFi->mPlaceRecognitionScore = si;
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return;

    std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
    for (auto it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); ++it) {
      KeyFrameT* pKFi = it->second;
      std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KeyFrameT* pBestKF = pKFi;
      for (KeyFrameT* pKF2 : vpNeighs) {
        if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;
        accScore += pKF2->mPlaceRecognitionScore;
        if (pKF2->mPlaceRecognitionScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mPlaceRecognitionScore;
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
    }

    lAccScoreAndMatch.sort([](const std::pair<float, KeyFrameT*>& a, const std::pair<float, KeyFrameT*>& b) { return a.first > b.first; });

    vpLoopCand.reserve(nNumCandidates);
    vpMergeCand.reserve(nNumCandidates);
    std::set<KeyFrameT*> spAlreadyAddedKF;
    size_t i = 0;
    auto it = lAccScoreAndMatch.begin();
    while (i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates)) {
      KeyFrameT* pKFi = it->second;
      if (pKFi->isBad())
        throw std::logic_error("PliKeyFrameDatabase::DetectNBestCandidates: a bad keyframe in the candidate list (the reference loops for ever here)");
      if (!spAlreadyAddedKF.count(pKFi)) {
        if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) {
          vpLoopCand.push_back(pKFi);
        } else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) {
          vpMergeCand.push_back(pKFi);
        }
        spAlreadyAddedKF.insert(pKFi);
      }
      i++;
      it++;
    }
  }

  // what the device holds (struct pli_kfdb_stats)
  struct pli_kfdb_stats pliStats() const {
    struct pli_kfdb_stats st;
    pli::check(pli_kfdb_stats(db_, &st));
    return st;
  }

 private:
  template <class BowT>
  static void flatten(const BowT& bow, std::vector<uint32_t>& w, std::vector<double>& v) {
    w.clear(); v.clear();
    w.reserve(bow.size()); v.reserve(bow.size());
    for (auto it = bow.begin(); it != bow.end(); ++it) { w.push_back((uint32_t)it->first); v.push_back((double)it->second); }
  }

  void eraseLocked(KeyFrameT* pKF) {
    auto it = slotOf_.find(pKF);
    if (it == slotOf_.end()) return;                         // (the reference finds nothing to erase either)
    pli::check(pli_kfdb_erase(fe_.handle(), db_, it->second));
    kf_[it->second] = nullptr;
    slotOf_.erase(it);
  }

  // One device query; returns the slots that share a word with `bow` in the order in which the reference's walk over the inverted
  // file first meets their keyframes: by first shared word, and within a word by the order of the add() calls.
  template <class BowT>
  std::vector<int32_t> query(const BowT& bow, std::vector<int32_t>& common, std::vector<double>& score) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    flatten(bow, w, v);
    const int32_t n = (int32_t)kf_.size();
    std::vector<int32_t> first((size_t)n);
    common.assign((size_t)n, 0);
    score.assign((size_t)n, 0.0);
    pli::check(pli_kfdb_query(fe_.handle(), db_, w.data(), v.data(), (int32_t)w.size(), n, common.data(), first.data(), score.data()));
    std::vector<int32_t> order;
    for (int32_t s = 0; s < n; ++s)
      if (kf_[s] && common[s] > 0) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      return first[a] != first[b] ? first[a] < first[b] : seq_[a] < seq_[b];
    });
    return order;
  }

  pli::Frontend& fe_;
  pli_kfdb* db_ = nullptr;
  std::mutex mMutex;
  std::vector<KeyFrameT*> kf_;                                // slot -> keyframe (nullptr: free)
  std::vector<uint64_t> seq_;                                 // slot -> number of the add() call that filled it
  uint64_t nextSeq_ = 0;
  std::unordered_map<KeyFrameT*, int32_t> slotOf_;
};

}  // namespace ORB_SLAM3
