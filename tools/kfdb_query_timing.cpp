// GPU box (built and run by tools/kfdb_query_timing.py): host-inclusive latency of pli_kfdb_query and of the adapter's whole
// PliKeyFrameDatabase::DetectRelocalizationCandidates against a plain host inverted-file implementation of our own (std::list per
// word, std::map BowVectors, the score by a two-map merge), on the same box, for databases of N synthetic keyframes with about 1000
// words each out of a vocabulary of a million.  The two implementations must return the same candidates, or the program fails.
//
//   kfdb_query_timing N [calls] [warmup]   ->   one JSON object on stdout
#include "pli_slam_amd/adapters/orbslam_keyframe_database.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

namespace {

struct Map { bool IsBad() { return false; } };
struct KeyFrame {
  long unsigned int mnId = 0;
  pli::BowVector mBowVec;
  long unsigned int mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
  int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
  float mRelocScore = 0, mPlaceRecognitionScore = 0;
  std::vector<KeyFrame*> ordered;
  Map* map = nullptr;
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n) {
    return std::vector<KeyFrame*>(ordered.begin(), ordered.begin() + std::min(ordered.size(), (size_t)n));
  }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(ordered.begin(), ordered.end()); }
  Map* GetMap() { return map; }
  bool isBad() { return false; }
};
struct Frame { long unsigned int mnId = 0; pli::BowVector mBowVec; };

constexpr unsigned kWords = 1000000;

double l1Score(const pli::BowVector& a, const pli::BowVector& b) {
  double s = 0;
  auto i = a.begin(), j = b.begin();
  while (i != a.end() && j != b.end()) {
    if (i->first < j->first) ++i;
    else if (j->first < i->first) ++j;
    else { s += std::fabs(i->second - j->second) - std::fabs(i->second) - std::fabs(j->second); ++i; ++j; }
  }
  return -s / 2.0;
}

// the plain host form: an inverted file walked per query word, then the score of every keyframe that shares enough words
struct HostDatabase {
  std::vector<std::list<KeyFrame*> > inverted{kWords};
  void add(KeyFrame* k) { for (auto& wv : k->mBowVec) inverted[wv.first].push_back(k); }
  std::vector<KeyFrame*> relocalizationCandidates(Frame* F, Map* pMap) {
    std::list<KeyFrame*> sharing;
    for (auto& wv : F->mBowVec)
      for (KeyFrame* k : inverted[wv.first]) {
        if (k->mnRelocQuery != F->mnId) { k->mnRelocWords = 0; k->mnRelocQuery = F->mnId; sharing.push_back(k); }
        k->mnRelocWords++;
      }
    int maxCommon = 0;
    for (KeyFrame* k : sharing) maxCommon = std::max(maxCommon, k->mnRelocWords);
    const int minCommon = maxCommon * 0.8f;
    std::vector<std::pair<float, KeyFrame*> > scored, acc;
    for (KeyFrame* k : sharing)
      if (k->mnRelocWords > minCommon) { k->mRelocScore = (float)l1Score(F->mBowVec, k->mBowVec); scored.emplace_back(k->mRelocScore, k); }
    float bestAcc = 0;
    for (auto& sk : scored) {
      float best = sk.first, sum = sk.first;
      KeyFrame* bestKF = sk.second;
      for (KeyFrame* n : sk.second->GetBestCovisibilityKeyFrames(10)) {
        if (n->mnRelocQuery != F->mnId) continue;
        sum += n->mRelocScore;
        if (n->mRelocScore > best) { best = n->mRelocScore; bestKF = n; }
      }
      acc.emplace_back(sum, bestKF);
      bestAcc = std::max(bestAcc, sum);
    }
    std::vector<KeyFrame*> out;
    std::set<KeyFrame*> seen;
    for (auto& ak : acc)
      if (ak.first > 0.75f * bestAcc && ak.second->GetMap() == pMap && seen.insert(ak.second).second) out.push_back(ak.second);
    return out;
  }
};

double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char** argv) {
  const int N = argc > 1 ? std::atoi(argv[1]) : 1000, calls = argc > 2 ? std::atoi(argv[2]) : 30, warmup = argc > 3 ? std::atoi(argv[3]) : 5;
  std::mt19937 rng(12345);
  // locations of 1500 words, 50 keyframes each, every keyframe sees about 950 of its location's words and 50 of 400 common ones
  const int perLoc = 50, nloc = (N + perLoc - 1) / perLoc;
  std::vector<unsigned> common(400);
  for (auto& w : common) w = rng() % kWords;
  std::vector<std::vector<unsigned> > loc((size_t)nloc, std::vector<unsigned>(1500));
  for (auto& l : loc) for (auto& w : l) w = rng() % kWords;
  auto draw = [&](int l, pli::BowVector& b) {
    std::uniform_real_distribution<double> u(0.5, 9.0);
    for (unsigned w : loc[(size_t)l]) if (rng() % 1500 < 950) b[w] += u(rng);
    for (int i = 0; i < 50; ++i) b[common[rng() % common.size()]] += u(rng);
    double norm = 0;
    for (auto& wv : b) norm += std::fabs(wv.second);
    for (auto& wv : b) wv.second /= norm;
  };
  Map map;
  std::vector<std::unique_ptr<KeyFrame> > kfs((size_t)N), twins((size_t)N);
  for (int i = 0; i < N; ++i) {
    kfs[i].reset(new KeyFrame()); twins[i].reset(new KeyFrame());
    kfs[i]->mnId = twins[i]->mnId = (long unsigned int)i + 1;
    kfs[i]->map = twins[i]->map = &map;
    draw(i / perLoc, kfs[i]->mBowVec);
    twins[i]->mBowVec = kfs[i]->mBowVec;
  }
  for (int i = 0; i < N; ++i)
    for (int d = 1; d <= 6; ++d)
      for (int j : {i - d, i + d})
        if (j >= 0 && j < N && j / perLoc == i / perLoc) { kfs[i]->ordered.push_back(kfs[j].get()); twins[i]->ordered.push_back(twins[j].get()); }
  std::vector<Frame> frames((size_t)(calls + warmup));
  for (size_t q = 0; q < frames.size(); ++q) { frames[q].mnId = 1000000 + q; draw((int)(rng() % nloc), frames[q].mBowVec); }
  double words = 0;
  for (auto& k : kfs) words += (double)k->mBowVec.size();

  try {
    pli_frontend_config cfg;
    pli_config_default(&cfg, 128, 96);
    cfg.orb_nfeatures = 100; cfg.lsd_nfeatures = 0;
    pli::Frontend fe(cfg);
    ORB_SLAM3::PliKeyFrameDatabase<KeyFrame, Frame, Map> db(fe);
    HostDatabase host;
    double t0 = nowMs();
    for (auto& k : kfs) db.add(k.get());
    const double addMs = (nowMs() - t0) / N;
    for (auto& k : twins) host.add(k.get());

    // the query alone, through the C entry point
    pli_kfdb* raw = nullptr;
    pli::check(pli_kfdb_create(fe.handle(), &raw));
    std::vector<uint32_t> w; std::vector<double> v;
    for (auto& k : kfs) {
      w.clear(); v.clear();
      for (auto& wv : k->mBowVec) { w.push_back(wv.first); v.push_back(wv.second); }
      int32_t slot;
      pli::check(pli_kfdb_add(fe.handle(), raw, w.data(), v.data(), (int32_t)w.size(), &slot));
    }
    std::vector<int32_t> cm((size_t)N), fi((size_t)N);
    std::vector<double> sc((size_t)N);
    std::vector<double> tq, ta, th;
    size_t ncand = 0;
    for (size_t q = 0; q < frames.size(); ++q) {
      w.clear(); v.clear();
      for (auto& wv : frames[q].mBowVec) { w.push_back(wv.first); v.push_back(wv.second); }
      t0 = nowMs();
      pli::check(pli_kfdb_query(fe.handle(), raw, w.data(), v.data(), (int32_t)w.size(), N, cm.data(), fi.data(), sc.data()));
      const double dq = nowMs() - t0;
      t0 = nowMs();
      std::vector<KeyFrame*> a = db.DetectRelocalizationCandidates(&frames[q], &map);
      const double da = nowMs() - t0;
      t0 = nowMs();
      std::vector<KeyFrame*> h = host.relocalizationCandidates(&frames[q], &map);
      const double dh = nowMs() - t0;
      if (a.size() != h.size()) { std::fprintf(stderr, "query %zu: %zu candidates on the device path, %zu on the host\n", q, a.size(), h.size()); return 3; }
      for (size_t i = 0; i < a.size(); ++i)
        if (a[i]->mnId != h[i]->mnId) { std::fprintf(stderr, "query %zu: candidate %zu differs\n", q, i); return 3; }
      if ((int)q >= warmup) { tq.push_back(dq); ta.push_back(da); th.push_back(dh); ncand += a.size(); }
    }
    pli_kfdb_destroy(raw);
    std::printf("{\"keyframes\": %d, \"words_per_keyframe\": %.0f, \"calls\": %d, \"query_ms\": %.4f, \"adapter_reloc_ms\": %.4f, "
                "\"host_inverted_file_ms\": %.4f, \"add_ms\": %.4f, \"candidates_per_query\": %.1f}\n",
                N, words / N, calls, median(tq), median(ta), median(th), addMs, (double)ncand / calls);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
