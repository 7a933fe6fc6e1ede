// PIN — DEV-TIME TEST INFRASTRUCTURE ONLY (tools/gen_kfdb_ref.py builds and runs this once per fixture, outside the tree).
// Stand-alone driver over the reference's own src/KeyFrameDatabase.cc and Thirdparty/DBoW2, both compiled where they lie,
// unmodified, against standins.h (force-included), shim/ and oracle/ref_recipe/bow_shim.  Replays one "world" on ONE
// KeyFrameDatabase, so that what a query leaves in the keyframes' members is there for the next one.
//
//   pli_ref_kfdb REQUEST RESPONSE
//
// REQUEST : int32 path length, vocabulary text file path; int32 levelsup; int32 nmaps, nmaps x uint8 IsBad;
//           int32 nkf, per keyframe {int64 mnId, int32 map, int32 nfeat, nfeat x 32 descriptor bytes, int32 ncov, ncov x int32
//           (ordered covisibility list, keyframe indices), int32 nconn, nconn x int32 (connected set)};
//           int32 nops, per op int32 kind: 0 add k | 1 erase k | 2 DetectRelocalizationCandidates {int64 frame mnId, int32 map,
//           int32 nfeat, descriptors} | 3 DetectNBestCandidates {int32 k, int32 nNumCandidates} | 4 clearMap m | 5 clear.
// RESPONSE: int32 vocabulary.size(); per keyframe {int32 n, n x {uint32 word, float64 value}} (its BowVector, by the reference's
//           transform); per query op, in order: the query's BowVector in the same form; nkf x int32 shared words and nkf x float64
//           vocabulary.score(query, keyframe) against EVERY keyframe of the world; int32 nloop, nloop x int64 mnId; int32 nmerge,
//           nmerge x int64 mnId (relocalisation: its return value as "loop", nmerge = 0); then per keyframe {uint64 mnRelocQuery,
//           int32 mnRelocWords, float mRelocScore, uint64 mnPlaceRecognitionQuery, int32 mnPlaceRecognitionWords,
//           float mPlaceRecognitionScore} as the call left them.
#include "KeyFrameDatabase.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

namespace {

FILE* in = nullptr;
FILE* out = nullptr;

void get(void* p, size_t n) {
  if (n && std::fread(p, 1, n, in) != n) { std::fprintf(stderr, "short request\n"); std::exit(2); }
}
template <class T> T get() { T v; get(&v, sizeof(T)); return v; }
void put(const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, out) != n) { std::perror("write"); std::exit(2); }
}
template <class T> void put(T v) { put(&v, sizeof(T)); }

std::vector<cv::Mat> features() {
  const int32_t n = get<int32_t>();
  std::vector<cv::Mat> f((size_t)n);
  for (int i = 0; i < n; ++i) { f[i].create(1, 32, CV_8U); get(f[i].data, 32); }
  return f;
}

void putBow(const DBoW2::BowVector& bv) {
  put<int32_t>((int32_t)bv.size());
  for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it) { put<uint32_t>(it->first); put<double>(it->second); }
}

int shared(const DBoW2::BowVector& a, const DBoW2::BowVector& b) {
  int n = 0;
  for (DBoW2::BowVector::const_iterator it = a.begin(); it != a.end(); ++it) n += (int)b.count(it->first);
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace ORB_SLAM3;
  if (argc != 3) { std::fprintf(stderr, "usage: %s REQUEST RESPONSE\n", argv[0]); return 2; }
  in = std::fopen(argv[1], "rb");
  out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::perror("open"); return 2; }
  std::string path((size_t)get<int32_t>(), '\0');
  get(&path[0], path.size());
  const int levelsup = get<int32_t>();
  ORBVocabulary voc;
  if (!voc.loadFromTextFile(path)) { std::fprintf(stderr, "loadFromTextFile refused %s\n", path.c_str()); return 3; }
  put<int32_t>((int32_t)voc.size());

  std::vector<std::unique_ptr<Map>> maps((size_t)get<int32_t>());
  for (size_t m = 0; m < maps.size(); ++m) { maps[m].reset(new Map()); maps[m]->index = (int)m; maps[m]->mbBad = get<uint8_t>() != 0; }
  std::vector<std::unique_ptr<KeyFrame>> kfs((size_t)get<int32_t>());
  for (auto& k : kfs) k.reset(new KeyFrame());
  for (auto& k : kfs) {
    k->mnId = (long unsigned int)get<int64_t>();
    k->mpMap = maps.at((size_t)get<int32_t>()).get();
    std::vector<cv::Mat> f = features();
    DBoW2::FeatureVector fv;
    voc.transform(f, k->mBowVec, fv, levelsup);
    k->N = (int)f.size();
    for (int32_t i = 0, n = get<int32_t>(); i < n; ++i) k->mvpOrderedConnectedKeyFrames.push_back(kfs.at((size_t)get<int32_t>()).get());
    for (int32_t i = 0, n = get<int32_t>(); i < n; ++i) k->mConnected.push_back(kfs.at((size_t)get<int32_t>()).get());
    putBow(k->mBowVec);
  }

  KeyFrameDatabase db(voc, voc);      // (the two-vocabulary form: clear() reads mpVoc_l)
  for (int32_t op = 0, nops = get<int32_t>(); op < nops; ++op) {
    const int32_t kind = get<int32_t>();
    if (kind == 0) db.add(kfs.at((size_t)get<int32_t>()).get());
    else if (kind == 1) db.erase(kfs.at((size_t)get<int32_t>()).get());
    else if (kind == 4) db.clearMap(maps.at((size_t)get<int32_t>()).get());
    else if (kind == 5) db.clear();
    else if (kind == 2 || kind == 3) {
      std::vector<KeyFrame*> loop, merge;
      const DBoW2::BowVector* q = nullptr;
      Frame F;
      if (kind == 2) {
        F.mnId = (long unsigned int)get<int64_t>();
        Map* pMap = maps.at((size_t)get<int32_t>()).get();
        std::vector<cv::Mat> f = features();
        DBoW2::FeatureVector fv;
        voc.transform(f, F.mBowVec, fv, levelsup);
        F.N = (int)f.size();
        q = &F.mBowVec;
        loop = db.DetectRelocalizationCandidates(&F, pMap);
      } else {
        KeyFrame* pKF = kfs.at((size_t)get<int32_t>()).get();
        const int nNum = get<int32_t>();
        q = &pKF->mBowVec;
        db.DetectNBestCandidates(pKF, loop, merge, nNum);
      }
      putBow(*q);
      for (auto& k : kfs) put<int32_t>(shared(*q, k->mBowVec));
      for (auto& k : kfs) put<double>(voc.score(*q, k->mBowVec));
      put<int32_t>((int32_t)loop.size());
      for (KeyFrame* k : loop) put<int64_t>((int64_t)k->mnId);
      put<int32_t>((int32_t)merge.size());
      for (KeyFrame* k : merge) put<int64_t>((int64_t)k->mnId);
      for (auto& k : kfs) {
        put<uint64_t>(k->mnRelocQuery); put<int32_t>(k->mnRelocWords); put<float>(k->mRelocScore);
        put<uint64_t>(k->mnPlaceRecognitionQuery); put<int32_t>(k->mnPlaceRecognitionWords); put<float>(k->mPlaceRecognitionScore);
      }
    } else { std::fprintf(stderr, "unknown op %d\n", kind); return 2; }
  }
  std::fclose(in);
  if (std::fclose(out) != 0) { std::perror("close"); return 2; }
  return 0;
}
