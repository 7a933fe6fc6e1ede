// TEST HARNESS for pli_slam_amd/adapters/orbslam_keyframe_database.hpp (tests/test_cpp_kfdb.py): PliKeyFrameDatabase on stub
// KeyFrame / Frame / Map types replays a recorded world (tests/golden/kfdb_ref, tests/helpers_kfdb.py) and dumps the candidates and
// the members of every keyframe after every query; then a second add() and a bad keyframe in DetectNBestCandidates' sorted list
// must throw std::logic_error.  Linked against libpli_frontend.so (on the GPU) or tests/cpp/mock_pli_kfdb.cpp (host only, sanitizers).
//
//   kfdb_harness INPUT OUTPUT
//
// INPUT : int32 nmaps, nmaps x uint8 IsBad; int32 nkf, per keyframe {int64 mnId, int32 map, int32 n, n x uint32 word, n x float64
//         value, int32 ncov, ncov x int32, int32 nconn, nconn x int32}; int32 nq, per query BowVector {int32 n, words, values};
//         int32 nops, per op {int32 kind, int64 a, int32 b, int32 c} (kinds of tests/helpers_kfdb.py; c: the query BowVector of a
//         relocalisation); int32 the keyframe that asks in the bad-keyframe check.
// OUTPUT: per query {int32 nloop, nloop x int64 mnId, int32 nmerge, nmerge x int64 mnId, per keyframe {uint64 mnRelocQuery,
//         int32 mnRelocWords, float mRelocScore, uint64 mnPlaceRecognitionQuery, int32 mnPlaceRecognitionWords,
//         float mPlaceRecognitionScore}}.
#include "pli_slam_amd/adapters/orbslam_keyframe_database.hpp"
#include <cstdio>
#include <cstdlib>
#include <memory>

struct Map {
  bool bad = false;
  bool IsBad() { return bad; }
};

struct KeyFrame {
  long unsigned int mnId = 0;
  pli::BowVector mBowVec;
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0;
  long unsigned int mnPlaceRecognitionQuery = 0;
  int mnPlaceRecognitionWords = 0;
  float mPlaceRecognitionScore = 0;
  std::vector<KeyFrame*> ordered;
  std::set<KeyFrame*> connected;
  Map* map = nullptr;
  bool bad = false;
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n) {
    return std::vector<KeyFrame*>(ordered.begin(), ordered.begin() + std::min(ordered.size(), (size_t)n));
  }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
  Map* GetMap() { return map; }
  bool isBad() { return bad; }
  void reset() {
    mnRelocQuery = mnPlaceRecognitionQuery = 0;
    mnRelocWords = mnPlaceRecognitionWords = 0;
    mRelocScore = mPlaceRecognitionScore = 0;
  }
};

struct Frame {
  long unsigned int mnId = 0;
  pli::BowVector mBowVec;
};

typedef ORB_SLAM3::PliKeyFrameDatabase<KeyFrame, Frame, Map> KeyFrameDatabase;

static FILE* in = nullptr;
static FILE* out = nullptr;
static void rd(void* p, size_t n) {
  if (n && std::fread(p, 1, n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
}
template <class T> static T rd() { T v; rd(&v, sizeof(T)); return v; }
template <class T> static void wr(T v) {
  if (std::fwrite(&v, sizeof(T), 1, out) != 1) { std::perror("write"); std::exit(2); }
}
static pli::BowVector bow() {
  const int32_t n = rd<int32_t>();
  std::vector<uint32_t> w((size_t)n);
  std::vector<double> v((size_t)n);
  rd(w.data(), (size_t)n * 4);
  rd(v.data(), (size_t)n * 8);
  pli::BowVector b;
  for (int i = 0; i < n; ++i) b[w[i]] = v[i];
  return b;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<std::unique_ptr<Map>> maps((size_t)rd<int32_t>());
  for (auto& m : maps) { m.reset(new Map()); m->bad = rd<uint8_t>() != 0; }
  std::vector<std::unique_ptr<KeyFrame>> kfs((size_t)rd<int32_t>());
  for (auto& k : kfs) k.reset(new KeyFrame());
  for (auto& k : kfs) {
    k->mnId = (long unsigned int)rd<int64_t>();
    k->map = maps.at((size_t)rd<int32_t>()).get();
    k->mBowVec = bow();
    for (int32_t i = 0, n = rd<int32_t>(); i < n; ++i) k->ordered.push_back(kfs.at((size_t)rd<int32_t>()).get());
    for (int32_t i = 0, n = rd<int32_t>(); i < n; ++i) k->connected.insert(kfs.at((size_t)rd<int32_t>()).get());
  }
  std::vector<pli::BowVector> queries((size_t)rd<int32_t>());
  for (auto& q : queries) q = bow();
  struct Op { int32_t kind; int64_t a; int32_t b, c; };
  std::vector<Op> ops((size_t)rd<int32_t>());
  for (auto& o : ops) { o.kind = rd<int32_t>(); o.a = rd<int64_t>(); o.b = rd<int32_t>(); o.c = rd<int32_t>(); }
  const int32_t asks = rd<int32_t>();
  std::fclose(in);

  try {
    pli_frontend_config cfg;
    pli_config_default(&cfg, 128, 96);            // the database needs a context, not its image buffers
    cfg.orb_nfeatures = 100;
    cfg.lsd_nfeatures = 0;
    pli::Frontend fe(cfg);
    out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    {
      KeyFrameDatabase db(fe, 0, 0);              // (voc, voc_l): not read
      for (const Op& o : ops) {
        if (o.kind == 0) db.add(kfs.at((size_t)o.a).get());
        else if (o.kind == 1) db.erase(kfs.at((size_t)o.a).get());
        else if (o.kind == 4) db.clearMap(maps.at((size_t)o.a).get());
        else if (o.kind == 5) db.clear();
        else {
          std::vector<KeyFrame*> loop, merge;
          if (o.kind == 2) {
            Frame F;
            F.mnId = (long unsigned int)o.a;
            F.mBowVec = queries.at((size_t)o.c);
            loop = db.DetectRelocalizationCandidates(&F, maps.at((size_t)o.b).get());
          } else {
            db.DetectNBestCandidates(kfs.at((size_t)o.a).get(), loop, merge, o.b);
          }
          wr<int32_t>((int32_t)loop.size());
          for (KeyFrame* k : loop) wr<int64_t>((int64_t)k->mnId);
          wr<int32_t>((int32_t)merge.size());
          for (KeyFrame* k : merge) wr<int64_t>((int64_t)k->mnId);
          for (auto& k : kfs) {
            wr<uint64_t>(k->mnRelocQuery); wr<int32_t>(k->mnRelocWords); wr<float>(k->mRelocScore);
            wr<uint64_t>(k->mnPlaceRecognitionQuery); wr<int32_t>(k->mnPlaceRecognitionWords); wr<float>(k->mPlaceRecognitionScore);
          }
        }
      }
    }
    std::fclose(out);

    // the two deliberate differences from the reference
    KeyFrameDatabase db(fe);
    for (auto& k : kfs) k->reset();
    for (size_t i = 0; i < kfs.size(); ++i)
      if ((int32_t)i != asks) db.add(kfs[i].get());
    int thrown = 0;
    try { db.add(kfs.at(asks == 0 ? 1 : 0).get()); } catch (const std::logic_error&) { ++thrown; }
    const struct pli_kfdb_stats st = db.pliStats();
    if (st.live_keyframes != (int32_t)kfs.size() - 1) { std::fprintf(stderr, "a refused add changed the database\n"); return 3; }
    for (auto& k : kfs) k->bad = true;
    std::vector<KeyFrame*> loop, merge;
    try { db.DetectNBestCandidates(kfs.at((size_t)asks).get(), loop, merge, 3); } catch (const std::logic_error&) { ++thrown; }
    if (thrown != 2) { std::fprintf(stderr, "expected two std::logic_error, got %d\n", thrown); return 3; }
    db.erase(kfs.at((size_t)asks).get());         // not in the database: nothing happens, as in the reference
    db.clear();
    if (db.pliStats().slot_high_water != 0) { std::fprintf(stderr, "clear left slots\n"); return 3; }
    std::printf("kfdb_harness: ok\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
