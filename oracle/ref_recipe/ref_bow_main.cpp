// ORACLE — TEST INFRASTRUCTURE ONLY.
// Stand-alone driver over the reference's own Thirdparty/DBoW2 (TemplatedVocabulary.h, FORB.cpp,
// BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp, DUtils/Random.cpp, DUtils/Timestamp.cpp),
// which oracle/Makefile compiles from the reference tree (never copied) against bow_shim/.
//
//   pli_ref_bow REQUEST RESPONSE
//
// REQUEST : int32 path length, the path of a vocabulary text file (ORBvoc.txt form), int32 levelsup,
//           int32 n, n x 32 descriptor bytes.
// RESPONSE: int32 nwords (vocabulary.size()), n, determinate;
//           n x uint32 word id, n x float64 weight, n x uint32 node id: what the protected per-feature
//           transform(feature, id, weight, &nid, levelsup) stored, with nid preset to 0xFFFFFFFF, so a
//           node id the reference never wrote stays 0xFFFFFFFF;
//           then, only when determinate (no feature left its node id unset: the set-level transform
//           declares `NodeId nid;` uninitialised, so otherwise its FeatureVector is indeterminate):
//           int32 nb, nb x {uint32 word, float64 value} in map order: the BowVector of
//           transform(features, BowVector, FeatureVector, levelsup);
//           int32 nf, nf x {uint32 node, int32 count, count x uint32 feature index}: its FeatureVector.
#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace {

const uint32_t kUnset = 0xFFFFFFFFu;

struct Voc : DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> {
  void feature(const cv::Mat& f, uint32_t& word, double& weight, uint32_t& node, int levelsup) const {
    DBoW2::WordId id = 0;
    DBoW2::WordValue w = 0;
    DBoW2::NodeId nid = kUnset;
    transform(f, id, w, &nid, levelsup);
    word = id; weight = w; node = nid;
  }
};

bool readAll(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
void put(FILE* f, const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, f) != n) { std::perror("write"); std::exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s REQUEST RESPONSE\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t plen = 0, levelsup = 0, n = 0;
  if (!readAll(in, &plen, 4) || plen <= 0 || plen > 4096) { std::fprintf(stderr, "bad request header\n"); return 2; }
  std::string path((size_t)plen, '\0');
  if (!readAll(in, &path[0], (size_t)plen) || !readAll(in, &levelsup, 4) || !readAll(in, &n, 4) || n < 0 || n > (1 << 20)) {
    std::fprintf(stderr, "bad request header\n");
    return 2;
  }
  std::vector<cv::Mat> features((size_t)n);
  for (int i = 0; i < n; ++i) {
    features[i].create(1, 32, CV_8U);
    if (!readAll(in, features[i].data, 32)) { std::fprintf(stderr, "short request\n"); return 2; }
  }
  std::fclose(in);

  Voc voc;
  if (!voc.loadFromTextFile(path)) { std::fprintf(stderr, "loadFromTextFile refused %s\n", path.c_str()); return 3; }

  std::vector<uint32_t> word((size_t)n), node((size_t)n);
  std::vector<double> weight((size_t)n);
  int32_t determinate = 1;
  for (int i = 0; i < n; ++i) {
    voc.feature(features[i], word[i], weight[i], node[i], levelsup);
    if (node[i] == kUnset) determinate = 0;
  }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const int32_t nwords = (int32_t)voc.size();
  put(out, &nwords, 4);
  put(out, &n, 4);
  put(out, &determinate, 4);
  put(out, word.data(), (size_t)n * 4);
  put(out, weight.data(), (size_t)n * 8);
  put(out, node.data(), (size_t)n * 4);
  if (determinate) {
    DBoW2::BowVector bv;
    DBoW2::FeatureVector fv;
    voc.transform(features, bv, fv, levelsup);
    const int32_t nb = (int32_t)bv.size();
    put(out, &nb, 4);
    for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it) {
      const uint32_t w = it->first;
      const double v = it->second;
      put(out, &w, 4);
      put(out, &v, 8);
    }
    const int32_t nf = (int32_t)fv.size();
    put(out, &nf, 4);
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
      const uint32_t nd = it->first;
      const int32_t cnt = (int32_t)it->second.size();
      put(out, &nd, 4);
      put(out, &cnt, 4);
      put(out, it->second.data(), (size_t)cnt * 4);
    }
  }
  std::fclose(out);
  return 0;
}
