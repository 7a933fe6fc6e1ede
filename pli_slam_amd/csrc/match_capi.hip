// Host side of the stateless entry points of include/pli_frontend.h: the descriptor matchers, the projection, local-map and two-camera
// searches, the searches of one item against a batch of keyframes (BoW, triangulation, Fuse, Sim3, relocalisation), the initialisation
// search, the vocabulary and BoW transform, the keyframe database and the distinctive descriptors.  Each reads: checks, the tables
// declared one line each (scratch_plan.hpp), commitScratch, launches, downloads.  From the context they take the stream, the scratch
// buffer and the level tables only (capi_host.hpp).
#include "capi_host.hpp"
#include <cmath>
#include <cstring>
#include <algorithm>
#include <memory>
#include <set>

namespace {

// ---- the searches of one item against a batch of keyframes ------------------------
// pli_search_by_bow, pli_search_by_bow_kf, pli_search_for_triangulation, pli_fuse_search and pli_search_by_projection_sim3 take their
// keyframes as flat tables (pli_search_by_projection_reloc: its candidates' point lists, mp_off):
// keyframe k is rows kf_off[k] .. kf_off[k + 1].  What they share on the host is here; every entry point checks in the same order:
// null / negative arguments, nkf == 0 (OK), kf_off and the per-keyframe cap (kfBatch), the other side's cap, null tables for
// total > 0, the values, the empty other side (OK, zeroed counts).
struct KfBatch {
  int nkf = 0;
  const int32_t* off = nullptr;
  int64_t total = 0;                                        // rows of all keyframes
  int maxNk = 0;                                            // rows of the largest keyframe
};

// PLI_ERR_INVALID for a kf_off that does not start at 0 or decreases, PLI_ERR_CAPACITY (capMsg) for a keyframe above the cap
pli_status kfBatch(int32_t nkf, const int32_t* kfOff, const char* capMsg, KfBatch& B) {
  if (kfOff[0] != 0) { g_err = "kf_off[0] must be 0"; return PLI_ERR_INVALID; }
  B.nkf = nkf; B.off = kfOff; B.maxNk = 0;
  for (int k = 0; k < nkf; ++k) {
    if (kfOff[k + 1] < kfOff[k]) { g_err = "kf_off must not decrease"; return PLI_ERR_INVALID; }
    const int nk = kfOff[k + 1] - kfOff[k];
    if (nk > PLI_BOW_MAX_FEATURES) { g_err = capMsg; return PLI_ERR_CAPACITY; }
    B.maxNk = std::max(B.maxNk, nk);
  }
  B.total = kfOff[nkf];
  return PLI_OK;
}

bool nodesOk(const int32_t* node, int64_t n, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (node[i] < -1) { g_err = std::string(what) + ": a node id or -1"; return false; }
  return true;
}

// (the rotation histogram's bin of an angle outside [0, 360) would be undefined in the reference, an assert)
inline float angleOf(float a) { return a; }
inline float angleOf(const pli_keypoint& k) { return k.angle; }
template <class T>
bool anglesOk(const T* p, int64_t n, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (!(angleOf(p[i]) >= 0.f && angleOf(p[i]) < 360.f)) { g_err = std::string(what) + " outside [0, 360)"; return false; }
  return true;
}

// (the octaves index the level tables: outside them the reference reads past a vector)
bool octavesOk(const pli_ctx* c, const pli_keypoint* kp, int64_t n, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (kp[i].octave < 0 || kp[i].octave >= c->hp.nlevels) { g_err = std::string(what) + ": octave outside the context's levels"; return false; }
  return true;
}

// (the two-camera searches: a keypoint's coordinates enter float arithmetic whose result picks cells and gates)
bool finiteOk(const pli_keypoint* kp, int64_t n, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(kp[i].x) || !std::isfinite(kp[i].y)) { g_err = std::string(what) + ": a keypoint's coordinates are not finite"; return false; }
  return true;
}

// (pli_create_new_map_points: mvuRight, mvDepth, mvKeys[i].pt and the poses enter float arithmetic whose results decide gates)
bool floatsFinite(const float* v, int64_t n, const char* what) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) { g_err = std::string(what) + ": a value is not finite"; return false; }
  return true;
}

// kf_nleft[k] = NLeft of keyframe k, inside its rows
bool nleftOk(int32_t nkf, const int32_t* kfOff, const int32_t* kfNleft, const char* msg) {
  for (int k = 0; k < nkf; ++k)
    if (kfNleft[k] < 0 || kfNleft[k] > kfOff[k + 1] - kfOff[k]) { g_err = msg; return false; }
  return true;
}

int pow2Ceil(int m) {
  int n = 1;
  while (n < m) n <<= 1;
  return n;
}

// mvScaleFactors, mvLevelSigma2 and mvInvLevelSigma2 = 1.0f / mvLevelSigma2 (ORBextractor.cc:420-431) as the device compares
// against them; each a table of MAX_LEVELS floats or NULL
void levelTables(const pli_ctx* c, float* scale, float* sigma2, float* invSigma2) {
  for (int l = 0; l < c->hp.nlevels; ++l) {
    const float s = c->hp.lv[l].scale;
    if (scale) scale[l] = s;
    if (sigma2) sigma2[l] = s * s;
    if (invSigma2) invSigma2[l] = 1.0f / (s * s);
  }
}

// The projection searches (pli_fuse_search, pli_search_by_projection_sim3 / _reloc) predict a point's level by comparing against
// level_ratio, nlevels - 1 thresholds that must not decrease, and sort a table into the 64 x 48 grid of its image bounds.
bool levelRatioOk(const pli_ctx* c, const float* levelRatio) {
  for (int n = 0; n < c->hp.nlevels - 1; ++n)
    if (std::isnan(levelRatio[n]) || (n > 0 && levelRatio[n] < levelRatio[n - 1])) { g_err = "level_ratio must not decrease"; return false; }
  return true;
}
bool imageBoundsOk(float minX, float maxX, float minY, float maxY) {
  if (!(maxX > minX) || !(maxY > minY)) { g_err = "empty image bounds"; return false; }
  return true;
}
// their level block for the device: level_ratio, mvScaleFactors and (ntables 3: Fuse's chi-square gate) mvInvLevelSigma2
struct LevelBlock {
  float v[3 * MAX_LEVELS] = {};
  LevelBlock(const pli_ctx* c, const float* levelRatio, int ntables) {
    std::copy(levelRatio, levelRatio + std::max(c->hp.nlevels - 1, 0), v);
    levelTables(c, v + MAX_LEVELS, nullptr, ntables == 3 ? v + 2 * MAX_LEVELS : nullptr);
  }
};
// one table as the single "keyframe" of k_fuse_grid: its offset list {0, n} (the caller's object: it lives until the synchronise)
struct OneTableOff { const int off[2]; explicit OneTableOff(int n) : off{0, n} {} };

// the candidate list of one slot of pli_search_by_projection_sim3 / _reloc: 16 keys (DESIGN.md §9, Sim3 projection; the ordered
// wave reads a list with one load, so 64 is the most; the development build can run the other widths)
int sim3ListWidth() {
  if (const char* e = DEVENV("PLI_SIM3_WIDTH")) return std::min(64, std::max(1, atoi(e)));
  return 16;
}

// the tables that the two SearchForTriangulation entry points share: pKF1's, the neighbours', the node sort's and the results
struct TriTables {
  ScratchBlock<pli_keypoint> dK1; ScratchBlock<uint8_t> dD1; ScratchBlock<int> dN1; ScratchBlock<uint8_t> dM1;
  ScratchBlock<int> dOff; ScratchBlock<pli_keypoint> dKk; ScratchBlock<uint8_t> dKd; ScratchBlock<int> dKn; ScratchBlock<uint8_t> dKm;
  ScratchBlock<uint32_t> dSn; ScratchBlock<uint16_t> dSi; ScratchBlock<int> dListed;
  ScratchBlock<int> dStat;                                  // per neighbour: 30 histogram bins, [30] the match counter
  ScratchBlock<int> dM;
};
TriTables triTables(ScratchPlan& plan, const KfBatch& B, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                    const uint8_t* hasMp1, int n1, const pli_keypoint* kfKp, const uint8_t* kfDesc, const int32_t* kfNode,
                    const uint8_t* kfHasMp) {
  const size_t total = (size_t)B.total, nkf = (size_t)B.nkf;
  TriTables T;
  T.dK1 = plan.in(kp1, n1);
  T.dD1 = plan.in(desc1, (size_t)n1 * 32);
  T.dN1 = plan.in(node1, n1);
  T.dM1 = plan.in(hasMp1, n1);
  T.dOff = plan.in(B.off, nkf + 1);
  T.dKk = plan.in(kfKp, total);
  T.dKd = plan.in(kfDesc, total * 32);
  T.dKn = plan.in(kfNode, total);
  T.dKm = plan.in(kfHasMp, total);
  T.dSn = plan.add<uint32_t>(total);
  T.dSi = plan.add<uint16_t>(total);
  T.dListed = plan.add<int>(nkf);
  T.dStat = plan.add<int>(nkf * 32);
  T.dM = plan.add<int>(nkf * n1);
  return T;
}

// the tail of the two SearchForTriangulation entry points
pli_status triEnd(pli_ctx* c, const KfBatch& B, int n1, const TriTables& T, int checkOri, int32_t* matches12, int32_t* nmatches) {
  if (checkOri) LAUNCH(c, "k_tri_finish", k_tri_finish, dim3(B.nkf), dim3(256), 0, T.dK1, n1, T.dOff, T.dKk, T.dM, T.dStat);
  HIPCHK(download(c, matches12, T.dM));
  std::vector<int> hstat((size_t)B.nkf * 32);
  HIPCHK(download(c, hstat.data(), T.dStat));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < B.nkf; ++k) nmatches[k] = hstat[(size_t)k * 32 + 30];
  return PLI_OK;
}
}  // namespace

extern "C" {

pli_status pli_descriptor_distance(pli_ctx* c, const uint8_t* a, const uint8_t* b, int32_t n, int32_t* dist) {
  CtxGuard guard__(c);
  if (!c || n < 0 || (n > 0 && (!a || !b || !dist))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (n == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto da = plan.in(a, (size_t)n * 32);
  auto db = plan.in(b, (size_t)n * 32);
  auto dd = plan.add<int>(n);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  LAUNCH(c, "k_distance", k_distance, dim3((n + 255) / 256), dim3(256), 0, da, db, n, dd);
  HIPCHK(download(c, dist, dd));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_hamming_knn2(pli_ctx* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t* idx, int32_t* dist) {
  CtxGuard guard__(c);
  if (!c || nq < 0 || nt < 0 || (nq > 0 && (!q || !idx || !dist)) || (nt > 0 && !t)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nq == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto dq = plan.in(q, (size_t)nq * 32);
  auto dt = plan.in(t, (size_t)nt * 32);
  auto di = plan.add<int>((size_t)nq * 2);               // k_knn2: two ints per query, the indices ...
  auto dd = plan.add<int>((size_t)nq * 2);               // ... and the distances
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  LAUNCH(c, "k_knn2", k_knn2, dim3(nq), dim3(64), 0, dq, nq, dt, nt, di, dd);
  HIPCHK(download(c, idx, di));
  HIPCHK(download(c, dist, dd));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

// knnMatch(k = 2), the ratio test and (mutual) the check the other way, on tables that are already on the device
struct MatchTables {
  ScratchBlock<uint8_t> d1, d2;
  ScratchBlock<int> i1, ds1, i2, ds2, m12, m21, count;
};
// (d1 / d2 null: a block that a kernel fills)
static MatchTables matchTables(ScratchPlan& plan, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2) {
  MatchTables T;
  T.d1 = plan.in(d1, (size_t)n1 * 32);
  T.d2 = plan.in(d2, (size_t)n2 * 32);
  T.i1 = plan.add<int>((size_t)n1 * 2);                  // k_knn2: two ints per query, the indices ...
  T.ds1 = plan.add<int>((size_t)n1 * 2);                 // ... and the distances
  T.i2 = plan.add<int>((size_t)n2 * 2);
  T.ds2 = plan.add<int>((size_t)n2 * 2);
  T.m12 = plan.add<int>(n1);
  T.m21 = plan.add<int>(n2);
  T.count = plan.add<int>(1);
  return T;
}
// the first n1 rows of T.d1 (n1 > 0, at most as declared) against T.d2
static pli_status matchLaunch(pli_ctx* c, const MatchTables& T, int32_t n1, int32_t n2, float nnr, bool mutual) {
  HIPCHK(hipMemsetAsync(T.count, 0, 4, c->stream));
  LAUNCH(c, "k_knn2", k_knn2, dim3(n1), dim3(64), 0, T.d1, n1, T.d2, n2, T.i1, T.ds1);
  LAUNCH(c, "k_ratio", k_ratio, dim3((n1 + 255) / 256), dim3(256), 0, T.i1, T.ds1, n1, n2, nnr, T.m12);
  const bool lr = mutual;
  if (lr && n2 > 0) {
    LAUNCH(c, "k_knn2", k_knn2, dim3(n2), dim3(64), 0, T.d2, n2, T.d1, n1, T.i2, T.ds2);
    LAUNCH(c, "k_ratio", k_ratio, dim3((n2 + 255) / 256), dim3(256), 0, T.i2, T.ds2, n2, n1, nnr, T.m21);
  }
  LAUNCH(c, "k_mutual", k_mutual, dim3((n1 + 255) / 256), dim3(256), 0, T.m12, (lr && n2 > 0) ? (int*)T.m21 : (int*)nullptr, n1, T.count);
  return PLI_OK;
}

static pli_status matchDescriptors(pli_ctx* c, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2, float nnr,
                                   bool mutual, int32_t* m12, int32_t* nmatches) {
  if (!c || n1 < 0 || n2 < 0 || (n1 > 0 && (!d1 || !m12)) || (n2 > 0 && !d2)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nmatches) *nmatches = 0;
  if (n1 == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  const MatchTables T = matchTables(plan, d1, n1, d2, n2);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  if ((st = matchLaunch(c, T, n1, n2, nnr, mutual)) != PLI_OK) return st;
  HIPCHK(download(c, m12, T.m12));
  return fetchCount(c, T.count, nmatches);
}

pli_status pli_match_lines(pli_ctx* c, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2, float nnr,
                           int32_t* m12, int32_t* nmatches) {
  CtxGuard guard__(c);
  return matchDescriptors(c, d1, n1, d2, n2, nnr, c && c->cfg.best_lr_matches != 0, m12, nmatches);
}

pli_status pli_match_nnr(pli_ctx* c, const uint8_t* d1, int32_t n1, const uint8_t* d2, int32_t n2, float nnr,
                         int32_t* m12, int32_t* nmatches) {
  CtxGuard guard__(c);
  return matchDescriptors(c, d1, n1, d2, n2, nnr, false, m12, nmatches);
}

// Both projection searches: mode 0 frame-to-frame (ORBmatcher.cc:2179-2323), mode 1 local map (:44-143).
// Frames whose keypoints fit the LDS owner table take the two-phase form (candidates in parallel, then the ordered
// assignment); larger ones the ordered assignment alone, owner table in global memory, which scans the frame per query.
constexpr int PROJ_LDS_KEYPOINTS = 15360;

// The tables of one search: the queries and their descriptors, the frame, the results (q null: a kernel writes the queries)
struct ProjTables {
  ScratchBlock<pli_proj_query> q; ScratchBlock<uint8_t> qd;
  ScratchBlock<pli_keypoint> k; ScratchBlock<uint8_t> dsc; ScratchBlock<float> u; ScratchBlock<uint8_t> occ;
  ScratchBlock<int> own, best, raw; ScratchBlock<unsigned long long> keys; ScratchBlock<int> cc, cnt;
};
static ProjTables projTables(ScratchPlan& plan, const pli_proj_query* q, const uint8_t* qdesc, int32_t nq, const pli_keypoint* kp,
                             const uint8_t* desc, const float* uright, const uint8_t* occupied, int32_t ncur) {
  const bool ownerInLds = ncur <= PROJ_LDS_KEYPOINTS;
  ProjTables T;
  T.q = plan.in(q, nq);
  T.qd = plan.in(qdesc, (size_t)nq * 32);
  T.k = plan.in(kp, ncur);
  T.dsc = plan.in(desc, (size_t)ncur * 32);
  T.u = plan.in(uright, ncur);
  T.own = plan.add<int>(ownerInLds ? 0 : ncur);
  T.best = plan.add<int>(nq);
  T.raw = plan.add<int>(nq);
  T.occ = plan.inOpt(occupied, ncur);
  T.keys = plan.add<unsigned long long>(ownerInLds ? (size_t)nq * PROJ_K : 0);
  T.cc = plan.add<int>(ownerInLds ? nq : 0);
  T.cnt = plan.add<int>(1);
  return T;
}
// the search on tables that are on the device (nq > 0); T.best, T.cnt and (mode 0, wantRaw) T.raw hold the answer
static pli_status projLaunch(pli_ctx* c, int mode, const ProjTables& T, int32_t nq, int32_t ncur, float minX, float maxX, float minY,
                             float maxY, int32_t checkOri, float nnratio, bool wantRaw) {
  const int nc = std::max(ncur, 1);
  int* rawOut = (mode == 0 && wantRaw) ? (int*)T.raw : (int*)nullptr;
  if (ncur <= PROJ_LDS_KEYPOINTS) {
    // a second-best farther than 100 / nnratio can no longer reject a best of <= 100 (ORBmatcher.cc:124-126)
    int limit = 100;
    if (mode == 1) limit = (nnratio > 0.4f) ? std::min(255, (int)(100.0f / nnratio) + 2) : 255;
    LAUNCH(c, "k_proj_candidates", k_proj_candidates, dim3(nq), dim3(64), 0, T.q, T.qd, nq, T.k, T.dsc, T.u, ncur, minX, maxX, minY, maxY,
           mode == 0 ? 1 : 0, limit, T.keys, T.cc);
    LAUNCH(c, "k_proj_assign", k_proj_assign, dim3(1), dim3(64), (size_t)nc * 4, T.q, T.qd, nq, T.k, T.dsc, T.u, T.occ, ncur, minX, maxX,
           minY, maxY, mode, checkOri, nnratio, T.keys, T.cc, T.best, T.cnt, rawOut);
  } else {
    LAUNCH(c, "k_proj_assign_scan", k_proj_assign_scan, dim3(1), dim3(64), 0, T.q, T.qd, nq, T.k, T.dsc, T.u, T.occ, ncur, minX, maxX,
           minY, maxY, mode, checkOri, nnratio, T.own, T.best, T.cnt, rawOut);
  }
  return PLI_OK;
}

static pli_status projectionSearch(pli_ctx* c, int mode, const pli_proj_query* q, const uint8_t* qdesc, int32_t nq,
                                   const pli_keypoint* kp, const uint8_t* desc, const float* uright, const uint8_t* occupied,
                                   int32_t ncur, float minX, float maxX, float minY, float maxY, int32_t checkOri,
                                   float nnratio, int32_t* best, int32_t* nmatches, int32_t* raw = nullptr) {
  if (!c || nq < 0 || ncur < 0 || (nq > 0 && (!q || !qdesc || !best)) || (ncur > 0 && (!kp || !desc || !uright))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nmatches) *nmatches = 0;
  if (nq == 0) return PLI_OK;
  if (ncur >= (1 << 28)) { g_err = "too many keypoints"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < nq; ++i)
    if (mode == 0 && (q[i].valid & ~3)) { g_err = "pli_proj_query.valid: 0, 1 or 1 | PLI_PROJ_NO_OBSERVATIONS"; return PLI_ERR_INVALID; }
  ScratchPlan plan;
  const ProjTables T = projTables(plan, q, qdesc, nq, kp, desc, uright, occupied, ncur);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const bool wantRaw = mode == 0 && raw;
  if ((st = projLaunch(c, mode, T, nq, ncur, minX, maxX, minY, maxY, checkOri, nnratio, wantRaw)) != PLI_OK) return st;
  HIPCHK(download(c, best, T.best));
  if (wantRaw) HIPCHK(download(c, raw, T.raw));
  return fetchCount(c, T.cnt, nmatches);
}

pli_status pli_search_by_projection(pli_ctx* c, const pli_proj_query* q, const uint8_t* qdesc, int32_t nq,
                                    const pli_keypoint* kp, const uint8_t* desc, const float* uright,
                                    const uint8_t* occupied, int32_t ncur,
                                    float minX, float maxX, float minY, float maxY, int32_t checkOri,
                                    int32_t* best, int32_t* raw, int32_t* nmatches) {
  CtxGuard guard__(c);
  return projectionSearch(c, 0, q, qdesc, nq, kp, desc, uright, occupied, ncur, minX, maxX, minY, maxY, checkOri, 0.0f, best, nmatches, raw);
}

pli_status pli_search_local_map(pli_ctx* c, const pli_proj_query* q, const uint8_t* qdesc, int32_t nq,
                                const pli_keypoint* kp, const uint8_t* desc, const float* uright,
                                const uint8_t* occupied, int32_t ncur, float minX, float maxX, float minY, float maxY,
                                float nnratio, int32_t* best, int32_t* nmatches) {
  CtxGuard guard__(c);
  return projectionSearch(c, 1, q, qdesc, nq, kp, desc, uright, occupied, ncur, minX, maxX, minY, maxY, 0, nnratio, best, nmatches);
}

// Tracking.cc:3809-3855 in one call: k_local_project writes the view records and the queries, the mode-1 search reads the queries
// where they lie.
pli_status pli_search_local_points(pli_ctx* c, const pli_fuse_point* mp, const uint8_t* mpDesc, int32_t nq, const float* pose,
                                   const pli_fuse_camera* cam, float viewingCosLimit, float th, int32_t farPoints, float thFar,
                                   float nnratio, const float* levelRatio, const pli_keypoint* kp, const uint8_t* desc,
                                   const float* uright, const uint8_t* occupied, int32_t ncur, pli_local_view* view,
                                   int32_t* best, int32_t* nInView, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || nq < 0 || ncur < 0 || !pose || !cam || !levelRatio || (nq > 0 && (!mp || !mpDesc || !view || !best)) ||
      (ncur > 0 && (!kp || !desc || !uright))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nInView) *nInView = 0;
  if (nmatches) *nmatches = 0;
  if (!levelRatioOk(c, levelRatio) || !imageBoundsOk(cam->min_x, cam->max_x, cam->min_y, cam->max_y)) return PLI_ERR_INVALID;
  if (ncur >= (1 << 28)) { g_err = "too many keypoints"; return PLI_ERR_INVALID; }
  if (!octavesOk(c, kp, ncur, "cur_kp")) return PLI_ERR_INVALID;
  for (int i = 0; i < nq; ++i)                                // (a stored level indexes mvScaleFactors)
    if (mp[i].valid == PLI_LOCAL_STORED_VIEW && !(mp[i].normal[2] >= 0.0f && mp[i].normal[2] < (float)c->hp.nlevels)) {
      g_err = "a stored view's level outside [0, orb_nlevels)";
      return PLI_ERR_INVALID;
    }
  if (nq == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  const LevelBlock lv(c, levelRatio, 2);
  ScratchPlan plan;
  auto dmp = plan.in(mp, nq);
  auto dpose = plan.in(pose, 15);
  auto dlv = plan.in(lv.v, 2 * MAX_LEVELS);
  auto dview = plan.add<pli_local_view>(nq);
  auto dcnt = plan.add<int>(1);                               // the points in view
  const ProjTables T = projTables(plan, nullptr, mpDesc, nq, kp, desc, uright, occupied, ncur);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemsetAsync(dcnt, 0, 4, c->stream));
  LAUNCH(c, "k_local_project", k_local_project, dim3((nq + 255) / 256), dim3(256), 0, dmp, nq, dpose, *cam, viewingCosLimit, th,
         farPoints ? 1 : 0, thFar, dlv, c->hp.nlevels, dlv + MAX_LEVELS, dview, T.q, dcnt);
  if ((st = projLaunch(c, 1, T, nq, ncur, cam->min_x, cam->max_x, cam->min_y, cam->max_y, 0, nnratio, false)) != PLI_OK) return st;
  HIPCHK(download(c, view, dview));
  HIPCHK(download(c, best, T.best));
  HIPCHK(download(c, nInView, dcnt, 0, 1));
  return fetchCount(c, T.cnt, nmatches);
}

// Tracking.cc:3862-3883 in one call: k_local_lines_project leaves the list and its descriptors, matchNNR runs on them.
pli_status pli_search_local_lines(pli_ctx* c, const float* sp, const uint8_t* valid, const uint8_t* desc, int32_t nl,
                                  const float* pose, const pli_fuse_camera* cam, const uint8_t* curDesc, int32_t n2, float nnr,
                                  int32_t* inView, float* projS, int32_t* inFrustum, int32_t* matches12, int32_t* nInView,
                                  int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || nl < 0 || n2 < 0 || !pose || !cam || (nl > 0 && (!sp || !valid || !desc || !inView || !projS || !inFrustum || !matches12)) ||
      (n2 > 0 && !curDesc)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nInView) *nInView = 0;
  if (nmatches) *nmatches = 0;
  if (nl == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto dsp = plan.in(sp, (size_t)nl * 3);
  auto dvalid = plan.in(valid, nl);
  auto ddesc = plan.in(desc, (size_t)nl * 32);
  auto dpose = plan.in(pose, 15);
  auto din = plan.add<int>(nl);
  auto dproj = plan.add<float>((size_t)nl * 2);
  auto dlist = plan.add<int>(nl);
  const MatchTables T = matchTables(plan, nullptr, nl, curDesc, n2);      // T.d1: the descriptors of the lines in view, gathered
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  LAUNCH(c, "k_local_lines_project", k_local_lines_project, dim3(1), dim3(1024), 0, dsp, dvalid, ddesc, nl, dpose, *cam, din, dproj, dlist,
         T.d1, T.count);
  HIPCHK(download(c, inView, din));
  HIPCHK(download(c, projS, dproj));
  int n1 = 0;
  if ((st = fetchCount(c, T.count, &n1)) != PLI_OK) return st;            // the list's length sizes the match
  if (nInView) *nInView = n1;
  if (n1 == 0) return PLI_OK;
  if ((st = matchLaunch(c, T, n1, n2, nnr, false)) != PLI_OK) return st;
  HIPCHK(download(c, inFrustum, dlist, 0, n1));
  HIPCHK(download(c, matches12, T.m12, 0, n1));
  return fetchCount(c, T.count, nmatches);
}

pli_status pli_search_local_map_fisheye(pli_ctx* c, const pli_proj_query* qL, const pli_proj_query* qR, const uint8_t* qdesc,
                                        int32_t nq, const pli_keypoint* kpL, const uint8_t* descL, const uint8_t* occL,
                                        const int32_t* l2r, int32_t nL, const pli_keypoint* kpR, const uint8_t* descR,
                                        const uint8_t* occR, const int32_t* r2l, int32_t nR, float minX, float maxX, float minY,
                                        float maxY, float nnratio, int32_t* mpL, int32_t* mpR, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || nq < 0 || nL < 0 || nR < 0 || (nq > 0 && (!qL || !qR || !qdesc)) || (nL > 0 && (!kpL || !descL || !l2r || !mpL)) ||
      (nR > 0 && (!kpR || !descR || !r2l || !mpR))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nmatches) *nmatches = 0;
  for (int i = 0; i < nL; ++i) {
    mpL[i] = -1;
    if (l2r[i] < -1 || l2r[i] >= nR) { g_err = "left_to_right out of range"; return PLI_ERR_INVALID; }
  }
  for (int i = 0; i < nR; ++i) {
    mpR[i] = -1;
    if (r2l[i] < -1 || r2l[i] >= nL) { g_err = "right_to_left out of range"; return PLI_ERR_INVALID; }
  }
  if (nq == 0 || nL + nR == 0) return PLI_OK;
  if (nL + nR > PROJ_LDS_KEYPOINTS) { g_err = "too many keypoints for the LDS slot tables of the fisheye local-map search"; return PLI_ERR_CAPACITY; }
  HIPCHK(hipSetDevice(c->device));
  const int ncM = std::max(std::max(nL, nR), 1);
  ScratchPlan plan;
  auto dqL = plan.in(qL, nq);
  auto dqR = plan.in(qR, nq);
  auto dqd = plan.in(qdesc, (size_t)nq * 32);
  auto dkL = plan.in(kpL, nL);
  auto ddL = plan.in(descL, (size_t)nL * 32);
  auto doL = plan.inOpt(occL, nL);
  auto dl2r = plan.in(l2r, nL);
  auto dmpL = plan.add<int>(nL);
  auto dkR = plan.in(kpR, nR);
  auto ddR = plan.in(descR, (size_t)nR * 32);
  auto doR = plan.inOpt(occR, nR);
  auto dr2l = plan.in(r2l, nR);
  auto dmpR = plan.add<int>(nR);
  auto du = plan.add<float>(ncM);
  auto dkeysL = plan.add<unsigned long long>((size_t)nq * PROJ_K);
  auto dkeysR = plan.add<unsigned long long>((size_t)nq * PROJ_K);
  auto dccL = plan.add<int>(nq);
  auto dccR = plan.add<int>(nq);
  auto dcnt = plan.add<int>(1);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  // (the fisheye branch has no mvuRight gate: a plane of -1 switches it off in the shared candidate kernel)
  LAUNCH(c, "k_fill_f32", k_fill_f32, dim3((ncM + 255) / 256), dim3(256), 0, du, ncM, -1.0f);
  const int limit = (nnratio > 0.4f) ? std::min(255, (int)(100.0f / nnratio) + 2) : 255;
  LAUNCH(c, "k_proj_candidates", k_proj_candidates, dim3(nq), dim3(64), 0, dqL, dqd, nq, dkL, ddL, du, nL, minX, maxX, minY, maxY, 0, limit,
         dkeysL, dccL);
  LAUNCH(c, "k_proj_candidates", k_proj_candidates, dim3(nq), dim3(64), 0, dqR, dqd, nq, dkR, ddR, du, nR, minX, maxX, minY, maxY, 0, limit,
         dkeysR, dccR);
  LAUNCH(c, "k_proj_assign_fisheye", k_proj_assign_fisheye, dim3(1), dim3(64), (size_t)(nL + nR) * 4, dqL, dqR, dqd, nq, dkL, ddL, doL,
         dl2r, nL, dkR, ddR, doR, dr2l, nR, du, minX, maxX, minY, maxY, nnratio, dkeysL, dccL, dkeysR, dccR, dmpL, dmpR, dcnt);
  HIPCHK(download(c, mpL, dmpL));
  HIPCHK(download(c, mpR, dmpR));
  return fetchCount(c, dcnt, nmatches);
}

// SearchByProjection(CurrentFrame, LastFrame) for a current frame of two cameras (match_kernels.hip: k_proj2_*)
pli_status pli_search_by_projection_two_cameras(pli_ctx* c, const pli_proj_query* qL, const pli_proj_query* qR, const uint8_t* qdesc,
                                                int32_t nq, const pli_keypoint* kpL, const uint8_t* descL, const uint8_t* occL,
                                                int32_t nL, const pli_keypoint* kpR, const uint8_t* descR, const uint8_t* occR,
                                                int32_t nR, float minX, float maxX, float minY, float maxY, int32_t checkOri,
                                                int32_t* bestL, int32_t* bestR, int32_t* rawL, int32_t* rawR, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || nq < 0 || nL < 0 || nR < 0 || (nq > 0 && (!qL || !qR || !qdesc || !bestL || !bestR)) || (nL > 0 && (!kpL || !descL)) ||
      (nR > 0 && (!kpR || !descR))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nmatches) *nmatches = 0;
  for (int i = 0; i < nq; ++i)
    if (qL[i].valid & ~3) { g_err = "pli_proj_query.valid: 0, 1 or 1 | PLI_PROJ_NO_OBSERVATIONS"; return PLI_ERR_INVALID; }
  if ((int64_t)nL + nR > PROJ_LDS_KEYPOINTS) { g_err = "too many keypoints for the LDS owner tables of the two-camera projection search"; return PLI_ERR_CAPACITY; }
  if (nq == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  const int ncM = std::max(std::max(nL, nR), 1);
  // both cameras' queries in one block: the left as given, then the right with the left's valid and angle (the only fields the
  // reference takes from the last frame's row for both cameras); q2 lives until the synchronisation in fetchCount
  std::vector<pli_proj_query> q2((size_t)2 * nq);
  for (int i = 0; i < nq; ++i) {
    q2[i] = qL[i];
    pli_proj_query r = qR[i];
    r.ur = 0.0f; r.angle = qL[i].angle; r.valid = qL[i].valid;
    q2[(size_t)nq + i] = r;
  }
  ScratchPlan plan;
  auto dq = plan.in(q2.data(), (size_t)2 * nq);
  auto dqd = plan.in(qdesc, (size_t)nq * 32);
  auto dkL = plan.in(kpL, nL);
  auto ddL = plan.in(descL, (size_t)nL * 32);
  auto doL = plan.inOpt(occL, nL);
  auto dkR = plan.in(kpR, nR);
  auto ddR = plan.in(descR, (size_t)nR * 32);
  auto doR = plan.inOpt(occR, nR);
  auto du = plan.add<float>(ncM);
  auto dkeys = plan.add<unsigned long long>((size_t)2 * nq * PROJ_K);
  auto dcc = plan.add<int>((size_t)2 * nq);
  auto dopen = plan.add<int>(nq);
  auto draw = plan.add<int>((size_t)2 * nq);
  auto dbest = plan.add<int>((size_t)2 * nq);
  auto dhist = plan.add<int>(2 * 30);                    // [2][HISTO_LENGTH]
  auto dacc = plan.add<int>(2);
  auto dcnt = plan.add<int>(1);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  LAUNCH(c, "k_fill_f32", k_fill_f32, dim3((ncM + 255) / 256), dim3(256), 0, du, ncM, -1.0f);
  LAUNCH(c, "k_proj2_candidates", k_proj2_candidates, dim3(nq, 2), dim3(64), 0, dq, dqd, nq, dkL, ddL, nL, dkR, ddR, nR, du, minX, maxX,
         minY, maxY, dkeys, dcc, dopen);
  LAUNCH(c, "k_proj2_assign", k_proj2_assign, dim3(2), dim3(64), (size_t)ncM * 4, dq, dqd, nq, dkL, ddL, doL, nL, dkR, ddR, doR, nR, du,
         minX, maxX, minY, maxY, checkOri, dkeys, dcc, dopen, draw, dhist, dacc);
  LAUNCH(c, "k_proj2_finish", k_proj2_finish, dim3(1), dim3(64), 0, dq, nq, dkL, dkR, checkOri, draw, dhist, dacc, dbest, dcnt);
  HIPCHK(download(c, bestL, dbest, 0, nq));                 // both cameras' halves of one block
  HIPCHK(download(c, bestR, dbest, nq, nq));
  HIPCHK(download(c, rawL, draw, 0, nq));
  HIPCHK(download(c, rawR, draw, nq, nq));
  return fetchCount(c, dcnt, nmatches);
}

// ---- bag of words (DBoW2 vocabulary tree) -------------------------------------
struct pli_vocab {
  int device = 0, k = 0, L = 0, nnodes = 0, nwords = 0;     // nnodes counts the root
  int* childOff = nullptr; int* childList = nullptr; uint8_t* desc = nullptr; int* word = nullptr; double* weight = nullptr;
};

void pli_vocab_destroy(pli_vocab* v) {
  if (!v) return;
  hipSetDevice(v->device);
  hipFree(v->childOff); hipFree(v->childList); hipFree(v->desc); hipFree(v->word); hipFree(v->weight);
  delete v;
}

pli_status pli_vocab_create(pli_ctx* c, int32_t k, int32_t L, int32_t n, const int32_t* parent, const uint8_t* isLeaf,
                            const uint8_t* desc, const double* weight, pli_vocab** out) {
  CtxGuard guard__(c);
  if (!c || !out || n < 1 || !parent || !isLeaf || !desc || !weight || k < 1 || L < 1) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  *out = nullptr;
  const int N = n + 1;                                      // + root (TemplatedVocabulary.h:1387)
  std::vector<int> cnt(N + 1, 0), off(N + 1, 0), list(n), word(N, -1);
  std::vector<double> w(N, 0.0);
  std::vector<uint8_t> d((size_t)N * 32, 0);
  int nwords = 0;
  for (int i = 0; i < n; ++i) {
    const int nid = i + 1, pid = parent[i];
    if (pid < 0 || pid >= nid) { g_err = "vocabulary: a node's parent must precede it"; return PLI_ERR_INVALID; }
    cnt[pid]++;
    std::memcpy(&d[(size_t)nid * 32], desc + (size_t)i * 32, 32);
    w[nid] = weight[i];
    if (isLeaf[i]) word[nid] = nwords++;                   // word ids in file order (:1421-1427)
  }
  for (int i = 0; i < N; ++i) off[i + 1] = off[i] + cnt[i];
  std::vector<int> fill(off.begin(), off.end() - 1);
  for (int i = 0; i < n; ++i) list[fill[parent[i]]++] = i + 1;   // children in file order (:1402)
  for (int i = 1; i < N; ++i)
    if (cnt[i] == 0 && word[i] < 0) { g_err = "vocabulary: a node without children is not flagged as a word"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<pli_vocab, void (*)(pli_vocab*)> v(new pli_vocab(), pli_vocab_destroy);
  v->device = c->device; v->k = k; v->L = L; v->nnodes = N; v->nwords = nwords;
  HIPCHK(hipMalloc(&v->childOff, (size_t)(N + 1) * 4));
  HIPCHK(hipMalloc(&v->childList, (size_t)n * 4));
  HIPCHK(hipMalloc(&v->desc, (size_t)N * 32));
  HIPCHK(hipMalloc(&v->word, (size_t)N * 4));
  HIPCHK(hipMalloc(&v->weight, (size_t)N * 8));
  HIPCHK(hipMemcpy(v->childOff, off.data(), (size_t)(N + 1) * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v->childList, list.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v->desc, d.data(), (size_t)N * 32, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v->word, word.data(), (size_t)N * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v->weight, w.data(), (size_t)N * 8, hipMemcpyHostToDevice));
  *out = v.release();
  return PLI_OK;
}

pli_status pli_bow_transform(pli_ctx* c, const pli_vocab* v, const uint8_t* desc, int32_t n, int32_t levelsup, int32_t* wordId,
                             double* weight, int32_t* nodeId) {
  CtxGuard guard__(c);
  if (!c || !v || n < 0 || (n > 0 && (!desc || !wordId || !weight || !nodeId))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (n == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto dd = plan.in(desc, (size_t)n * 32);
  auto dwt = plan.add<double>(n);
  auto dword = plan.add<int>(n);
  auto dnode = plan.add<int>(n);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  LAUNCH(c, "k_bow_descend", k_bow_descend, dim3(n), dim3(64), 0, dd, n, v->childOff, v->childList, v->desc, v->word, v->weight,
         v->L - levelsup, dword, dwt, dnode);
  HIPCHK(download(c, wordId, dword));
  HIPCHK(download(c, weight, dwt));
  HIPCHK(download(c, nodeId, dnode));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

// ---- the keyframe database (include/pli_frontend.h "place-recognition queries"; kfdb_kernels.hip) ---------------
// The device holds a CSR arena (word / value) and a slot table; the host keeps a mirror of the live vectors (for the rebuild) and of
// the slot table.  Every mutation ends with the stream idle, so the host vectors it copied from may change afterwards.
struct pli_kfdb {
  pli_ctx* ctx = nullptr;
  uint32_t* dWord = nullptr; double* dValue = nullptr; KfdbSlot* dSlots = nullptr;
  int64_t cap = 0, used = 0, liveWords = 0;               // arena words: capacity, appended (live + holes), live
  int slotCap = 0, live = 0, rebuilds = 0, growths = 0;
  std::vector<KfdbSlot> slots;                             // size = the high-water mark; count < 0: free
  std::vector<std::vector<uint32_t>> hWord; std::vector<std::vector<double>> hValue;     // per slot, live ones
  std::set<int> freeSlots;
  std::vector<uint8_t> qStage; std::vector<KfdbAnswer> aStage;                         // a query's upload and download
};

namespace {

constexpr int64_t KFDB_FIRST_ARENA = 1 << 14;             // words; doubles from here
constexpr int KFDB_FIRST_SLOTS = 1024;

bool ascending(const uint32_t* w, int n) {
  for (int i = 1; i < n; ++i)
    if (w[i] <= w[i - 1]) return false;
  return true;
}

// what the device reads for a slot: a free slot is an empty run
KfdbSlot deviceSlot(const KfdbSlot& s) { return KfdbSlot{s.count < 0 ? 0 : s.off, s.count < 0 ? 0 : s.count, 0}; }

pli_status kfdbAllocArena(pli_kfdb* db, int64_t words, uint32_t** w, double** v) {
  *w = nullptr; *v = nullptr;
  HIPCHK(hipMalloc(w, (size_t)words * 4));
  hipError_t e = hipMalloc(v, (size_t)words * 8);
  if (e != hipSuccess) { hipFree(*w); *w = nullptr; g_err = std::string("hipMalloc (keyframe database arena): ") + hipGetErrorString(e); return PLI_ERR_HIP; }
  return PLI_OK;
}

// the slot table holds at least n entries (doubling); the whole host table goes up again after a reallocation
pli_status kfdbSlotTable(pli_ctx* c, pli_kfdb* db, int n) {
  if (n <= db->slotCap) return PLI_OK;
  int cap = db->slotCap ? db->slotCap : KFDB_FIRST_SLOTS;
  while (cap < n) cap *= 2;
  KfdbSlot* t = nullptr;
  HIPCHK(hipMalloc(&t, (size_t)cap * sizeof(KfdbSlot)));
  std::vector<KfdbSlot> img(db->slots.size());
  for (size_t i = 0; i < img.size(); ++i) img[i] = deviceSlot(db->slots[i]);
  hipError_t e = img.empty() ? hipSuccess : hipMemcpyAsync(t, img.data(), img.size() * sizeof(KfdbSlot), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { hipFree(t); g_err = std::string("keyframe database slot table: ") + hipGetErrorString(e); return PLI_ERR_HIP; }
  hipFree(db->dSlots);
  db->dSlots = t; db->slotCap = cap;
  return PLI_OK;
}

// The arena rebuilt from the host mirror, with (word, value, n) appended for `slot`: the live vectors in slot order, no holes.
pli_status kfdbRebuild(pli_ctx* c, pli_kfdb* db, int slot, const uint32_t* word, const double* value, int n) {
  const int64_t total = db->liveWords + n;
  int64_t cap = db->cap;
  while (cap < total) cap *= 2;
  std::vector<uint32_t> w((size_t)total);
  std::vector<double> v((size_t)total);
  std::vector<KfdbSlot> table(db->slots);
  if ((int)table.size() <= slot) table.resize(slot + 1, KfdbSlot{0, -1, 0});
  int64_t at = 0;
  for (int s = 0; s < (int)table.size(); ++s) {
    const bool isNew = s == slot;
    if (!isNew && table[s].count < 0) continue;
    const int cnt = isNew ? n : table[s].count;
    const uint32_t* sw = isNew ? word : db->hWord[s].data();
    const double* sv = isNew ? value : db->hValue[s].data();
    if (cnt) { std::memcpy(&w[at], sw, (size_t)cnt * 4); std::memcpy(&v[at], sv, (size_t)cnt * 8); }
    table[s] = KfdbSlot{at, cnt, 0};
    at += cnt;
  }
  uint32_t* nw = db->dWord; double* nv = db->dValue;
  if (cap != db->cap) {
    pli_status st = kfdbAllocArena(db, cap, &nw, &nv);
    if (st != PLI_OK) return st;
  }
  pli_status st = kfdbSlotTable(c, db, (int)table.size());
  std::vector<KfdbSlot> img(table.size());
  for (size_t i = 0; i < img.size(); ++i) img[i] = deviceSlot(table[i]);
  hipError_t e = hipSuccess;
  if (st == PLI_OK) {
    if (total) e = hipMemcpyAsync(nw, w.data(), (size_t)total * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && total) e = hipMemcpyAsync(nv, v.data(), (size_t)total * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db->dSlots, img.data(), img.size() * sizeof(KfdbSlot), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { g_err = std::string("keyframe database rebuild: ") + hipGetErrorString(e); st = PLI_ERR_HIP; }
  }
  if (st != PLI_OK) {
    if (cap != db->cap) { hipFree(nw); hipFree(nv); }
    return st;
  }
  if (cap != db->cap) { hipFree(db->dWord); hipFree(db->dValue); db->dWord = nw; db->dValue = nv; db->cap = cap; db->growths++; }
  db->slots.swap(table);
  db->used = total;
  db->rebuilds++;
  return PLI_OK;
}

}  // namespace

pli_status pli_kfdb_create(pli_ctx* c, pli_kfdb** out) {
  CtxGuard guard__(c);
  if (!c || !out) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  *out = nullptr;
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<pli_kfdb, void (*)(pli_kfdb*)> db(new pli_kfdb(), pli_kfdb_destroy);
  db->ctx = c;
  pli_status st = kfdbAllocArena(db.get(), KFDB_FIRST_ARENA, &db->dWord, &db->dValue);
  if (st != PLI_OK) return st;
  db->cap = KFDB_FIRST_ARENA;
  if ((st = kfdbSlotTable(c, db.get(), 1)) != PLI_OK) return st;
  *out = db.release();
  return PLI_OK;
}

void pli_kfdb_destroy(pli_kfdb* db) {
  if (!db) return;
  CtxGuard guard__(db->ctx);          // (recursive: pli_kfdb_create's failure path comes here with the lock held)
  hipSetDevice(db->ctx->device);
  hipFree(db->dWord); hipFree(db->dValue); hipFree(db->dSlots);
  delete db;
}

pli_status pli_kfdb_add(pli_ctx* c, pli_kfdb* db, const uint32_t* word, const double* value, int32_t n, int32_t* slotOut) {
  CtxGuard guard__(c);
  if (!c || !db || db->ctx != c || !slotOut || n < 0 || (n > 0 && (!word || !value))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (n > PLI_BOW_MAX_FEATURES) { g_err = "a BowVector has at most PLI_BOW_MAX_FEATURES words"; return PLI_ERR_CAPACITY; }
  if (!ascending(word, n)) { g_err = "word ids must ascend strictly"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const int slot = db->freeSlots.empty() ? (int)db->slots.size() : *db->freeSlots.begin();
  if (2 * (db->used - db->liveWords) > db->used) {                    // holes exceed half of the arena's words
    pli_status st = kfdbRebuild(c, db, slot, word, value, n);
    if (st != PLI_OK) return st;
  } else {
    pli_status st = kfdbSlotTable(c, db, slot + 1);
    if (st != PLI_OK) return st;
    if (db->used + n > db->cap) {                                      // full: double, device to device
      int64_t cap = db->cap;
      while (cap < db->used + n) cap *= 2;
      uint32_t* nw; double* nv;
      if ((st = kfdbAllocArena(db, cap, &nw, &nv)) != PLI_OK) return st;
      hipError_t e = hipSuccess;
      if (db->used) e = hipMemcpyAsync(nw, db->dWord, (size_t)db->used * 4, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess && db->used) e = hipMemcpyAsync(nv, db->dValue, (size_t)db->used * 8, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) { hipFree(nw); hipFree(nv); g_err = std::string("keyframe database growth: ") + hipGetErrorString(e); return PLI_ERR_HIP; }
      hipFree(db->dWord); hipFree(db->dValue);
      db->dWord = nw; db->dValue = nv; db->cap = cap; db->growths++;
    }
    const KfdbSlot entry{db->used, n, 0};
    if (n) {
      HIPCHK(hipMemcpyAsync(db->dWord + db->used, word, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(db->dValue + db->used, value, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(db->dSlots + slot, &entry, sizeof(entry), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (slot == (int)db->slots.size()) db->slots.push_back(entry); else db->slots[slot] = entry;
    db->used += n;
  }
  if ((int)db->hWord.size() <= slot) { db->hWord.resize(slot + 1); db->hValue.resize(slot + 1); }
  db->hWord[slot].assign(word, word + n);
  db->hValue[slot].assign(value, value + n);
  db->freeSlots.erase(slot);
  db->liveWords += n; db->live++;
  *slotOut = slot;
  return PLI_OK;
}

pli_status pli_kfdb_erase(pli_ctx* c, pli_kfdb* db, int32_t slot) {
  CtxGuard guard__(c);
  if (!c || !db || db->ctx != c) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (slot < 0 || slot >= (int)db->slots.size() || db->slots[slot].count < 0) { g_err = "the slot holds no keyframe"; return PLI_ERR_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const KfdbSlot empty{0, 0, 0};
  HIPCHK(hipMemcpyAsync(db->dSlots + slot, &empty, sizeof(empty), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  db->liveWords -= db->slots[slot].count; db->live--;
  db->slots[slot].count = -1;
  std::vector<uint32_t>().swap(db->hWord[slot]);
  std::vector<double>().swap(db->hValue[slot]);
  db->freeSlots.insert(slot);
  return PLI_OK;
}

pli_status pli_kfdb_clear(pli_ctx* c, pli_kfdb* db) {
  CtxGuard guard__(c);
  if (!c || !db || db->ctx != c) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  db->slots.clear(); db->hWord.clear(); db->hValue.clear(); db->freeSlots.clear();
  db->used = db->liveWords = 0; db->live = 0;
  return PLI_OK;
}

pli_status pli_kfdb_stats(const pli_kfdb* db, struct pli_kfdb_stats* out) {
  if (!db || !out) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  CtxGuard guard__(db->ctx);
  out->slot_high_water = (int32_t)db->slots.size(); out->live_keyframes = db->live;
  out->live_words = db->liveWords; out->arena_words = db->used; out->arena_capacity = db->cap;
  out->rebuilds = db->rebuilds; out->growths = db->growths;
  return PLI_OK;
}

pli_status pli_kfdb_query(pli_ctx* c, pli_kfdb* db, const uint32_t* qword, const double* qvalue, int32_t nq, int32_t nslots,
                          int32_t* common, int32_t* first, double* score) {
  CtxGuard guard__(c);
  if (!c || !db || db->ctx != c || nq < 0 || nslots < 0 || (nq > 0 && (!qword || !qvalue)) ||
      (nslots > 0 && (!common || !first || !score))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nq > PLI_BOW_MAX_FEATURES) { g_err = "a BowVector has at most PLI_BOW_MAX_FEATURES words"; return PLI_ERR_CAPACITY; }
  if (!ascending(qword, nq)) { g_err = "word ids must ascend strictly"; return PLI_ERR_INVALID; }
  if (nslots != (int)db->slots.size()) { g_err = "nslots differs from the database's slot high-water mark"; return PLI_ERR_INVALID; }
  if (nslots == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  db->qStage.resize((size_t)nq * 12);
  if (nq) { std::memcpy(db->qStage.data(), qvalue, (size_t)nq * 8); std::memcpy(db->qStage.data() + (size_t)nq * 8, qword, (size_t)nq * 4); }
  db->aStage.resize(nslots);
  ScratchPlan plan;
  auto dq = plan.in(db->qStage.data(), (size_t)nq * 12);  // nq values (8-byte aligned), then nq word ids: one upload
  auto da = plan.add<KfdbAnswer>(nslots);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  uint8_t* q8 = dq;
  const int blocks = std::min((nslots + KFDB_QUERY_BLOCK / 64 - 1) / (KFDB_QUERY_BLOCK / 64), KFDB_QUERY_MAX_BLOCKS);
  LAUNCH(c, "k_kfdb_query", k_kfdb_query, dim3(blocks), dim3(KFDB_QUERY_BLOCK), (size_t)nq * 4, (const uint32_t*)(q8 + (size_t)nq * 8),
         (const double*)q8, nq, db->dSlots, nslots, db->dWord, db->dValue, (KfdbAnswer*)da);
  HIPCHK(download(c, db->aStage.data(), da));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int s = 0; s < nslots; ++s) { common[s] = db->aStage[s].common; first[s] = db->aStage[s].first; score[s] = db->aStage[s].score; }
  return PLI_OK;
}

// ---- MapPoint / MapLine::ComputeDistinctiveDescriptors for a batch of features (MapPoint.cc:300-365, MapLine.cc:246-317;
// mapfeat_kernels.hip) ----
// The host sorts the groups into the two size classes from `off` and cuts the large ones into chunks of rows; the callers' tables are
// read and written with memcpy (any alignment).  One upload of the offsets, the class lists and the chunks, one of the descriptors,
// one launch for the small class and two for the large one (where a class has groups), one download of best | best_median |
// row_median.
pli_status pli_distinctive_descriptors(pli_ctx* c, const uint8_t* desc, const int32_t* off, int32_t nfeat, int32_t* best,
                                       int32_t* bestMedian, int32_t* rowMedian) {
  CtxGuard guard__(c);
  if (!c || nfeat < 0 || !off || (nfeat > 0 && !best)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  // meta: off (nfeat + 1), then nfeat entries with the small class's group ids from the front and the large class's from the back,
  // then the large class's chunks
  std::vector<int32_t> meta((size_t)nfeat * 2 + 1);
  std::memcpy(meta.data(), off, ((size_t)nfeat + 1) * sizeof(int32_t));
  if (meta[0] != 0) { g_err = "off[0] must be 0"; return PLI_ERR_INVALID; }
  int nSmall = 0, nLarge = 0, maxN = 0;
  for (int p = 0; p < nfeat; ++p) {
    if (meta[p + 1] < meta[p]) { g_err = "off must not decrease"; return PLI_ERR_INVALID; }
    const int n = meta[p + 1] - meta[p];
    if (n > PLI_DISTINCTIVE_MAX_OBS) { g_err = "a feature has more observations than the cap of distinctive descriptors"; return PLI_ERR_CAPACITY; }
    maxN = std::max(maxN, n);
    int32_t* list = meta.data() + nfeat + 1;
    if (n > DISTINCTIVE_WAVE_ROWS) list[nfeat - 1 - nLarge++] = p;
    else if (n > 0) list[nSmall++] = p;
  }
  const int64_t total = meta[nfeat];
  if (total > 0 && !desc) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nfeat == 0) return PLI_OK;
  const size_t chunkAt = meta.size();
  for (int g = 0; g < nLarge; ++g) {
    const int p = meta[(size_t)nfeat + 1 + (nfeat - nLarge) + g], n = meta[p + 1] - meta[p];
    for (int first = 0; first < n; first += DISTINCTIVE_BLOCK) { meta.push_back(p); meta.push_back(first); }
  }
  const int nChunks = (int)((meta.size() - chunkAt) / 2);
  std::vector<int32_t> out((size_t)nfeat * 2 + (rowMedian ? total : 0));
  if (total > 0) {
    HIPCHK(hipSetDevice(c->device));
    ScratchPlan plan;
    auto dDesc = plan.in(desc, (size_t)total * 32);
    auto dMeta = plan.in(meta.data(), meta.size());
    auto dOut = plan.add<int32_t>((size_t)nfeat * 2 + total);      // (the kernels always write row_median: the large class picks from it)
    pli_status st = commitScratch(c, plan);
    if (st != PLI_OK) return st;
    int32_t *dm = dMeta, *dout = dOut;
    const int* dOff = dm;
    const int* dList = dm + nfeat + 1;
    int* dBest = dout;
    int* dMed = dout + nfeat;
    int* dRow = dout + (size_t)nfeat * 2;
    const int perBlock = DISTINCTIVE_BLOCK / 64;
    if (nSmall)
      LAUNCH(c, "k_distinctive_wave", k_distinctive_wave, dim3(std::min((nSmall + perBlock - 1) / perBlock, DISTINCTIVE_MAX_BLOCKS)),
             dim3(DISTINCTIVE_BLOCK), 0, (const uint8_t*)dDesc, dOff, dList, nSmall, dBest, dMed, dRow);
    if (nLarge) {      // (LDS: the longest group's descriptors, 64 KiB at the cap)
      static_assert(sizeof(DistinctiveChunk) == 2 * sizeof(int32_t), "a chunk is two ints of meta");
      LAUNCH(c, "k_distinctive_block", k_distinctive_block, dim3(std::min(nChunks, DISTINCTIVE_MAX_BLOCKS)), dim3(DISTINCTIVE_BLOCK),
             (size_t)maxN * 32, (const uint8_t*)dDesc, dOff, reinterpret_cast<const DistinctiveChunk*>(dm + chunkAt), nChunks, dRow);
      LAUNCH(c, "k_distinctive_pick", k_distinctive_pick, dim3(std::min((nLarge + perBlock - 1) / perBlock, DISTINCTIVE_MAX_BLOCKS)),
             dim3(DISTINCTIVE_BLOCK), 0, dOff, dList + (nfeat - nLarge), nLarge, (const int*)dRow, dBest, dMed);
    }
    HIPCHK(download(c, out.data(), dOut, 0, out.size()));    // (without row_median where the caller does not ask for it)
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  for (int p = 0; p < nfeat; ++p)
    if (meta[p + 1] == meta[p]) { out[p] = -1; out[(size_t)nfeat + p] = INT32_MAX; }     // an empty group has no answer (:314-315, :327-328)
  std::memcpy(best, out.data(), (size_t)nfeat * sizeof(int32_t));
  if (bestMedian) std::memcpy(bestMedian, out.data() + nfeat, (size_t)nfeat * sizeof(int32_t));
  if (rowMedian && total > 0) std::memcpy(rowMedian, out.data() + (size_t)nfeat * 2, (size_t)total * sizeof(int32_t));
  return PLI_OK;
}

// ---- the searches of one item against a batch of keyframes (shared host part: KfBatch and the checks above) ----
// pli_search_by_bow (fNleft < 0: F.Nleft == -1) and pli_search_by_bow_two_cameras (the frame's first fNleft rows are the left camera's)
static pli_status searchByBow(pli_ctx* c, int32_t nkf, const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle,
                              const int32_t* kfNode, const uint8_t* kfValid, const uint8_t* fDesc, const float* fAngle,
                              const int32_t* fNode, int32_t nf, int32_t fNleft, float nnratio, int32_t checkOri, int32_t* matches,
                              int32_t* nmatches) {
  if (!c || nkf < 0 || nf < 0 || (nkf > 0 && (!kfOff || !nmatches)) || (nf > 0 && (!fDesc || !fNode || (checkOri && !fAngle))) ||
      (nkf > 0 && nf > 0 && !matches)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a keyframe has more features than the SearchByBoW cap", B);
  if (st != PLI_OK) return st;
  if (nf > PLI_BOW_MAX_FEATURES) { g_err = "the frame has more features than the SearchByBoW cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total;
  if (total > 0 && (!kfDesc || !kfNode || !kfValid || (checkOri && !kfAngle))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nodesOk(kfNode, total, "kf_node") || !nodesOk(fNode, nf, "f_node")) return PLI_ERR_INVALID;
  if (checkOri && (!anglesOk(kfAngle, total, "kf_angle") || !anglesOk(fAngle, nf, "f_angle"))) return PLI_ERR_INVALID;
  if (nf == 0) { std::fill(nmatches, nmatches + nkf, 0); return PLI_OK; }
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto dOff = plan.in(kfOff, (size_t)nkf + 1);
  auto dKd = plan.in(kfDesc, (size_t)total * 32);
  auto dKa = plan.in(checkOri ? kfAngle : nullptr, total);   // (the angles are read with checkOri only)
  auto dKn = plan.in(kfNode, total);
  auto dKv = plan.in(kfValid, total);
  auto dFd = plan.in(fDesc, (size_t)nf * 32);
  auto dFa = plan.in(checkOri ? fAngle : nullptr, nf);
  auto dFn = plan.in(fNode, nf);
  auto dSn = plan.add<uint32_t>(nf);
  auto dSi = plan.add<uint16_t>(nf);
  auto dM = plan.add<int>((size_t)nkf * nf);
  auto dN = plan.add<int>(nkf);
  auto dListed = plan.add<int>(1);
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const int sortN = pow2Ceil(nf), keyCap = pow2Ceil(B.maxNk);
  // the frame is one table without an offset list: every feature listed in a node (no flag, no stereo table, no stat)
  LAUNCH(c, "k_node_sort", k_node_sort, dim3(1), dim3(1024), (size_t)sortN * 6, (const int*)nullptr, nf, dFn, (const uint8_t*)nullptr, 0,
         (const uint8_t*)nullptr, 0, sortN, dSn, dSi, dListed, (int*)nullptr);
  const size_t lds = 48 * 4 + (size_t)keyCap * 4 + alignUp((size_t)nf * 2, 16);
  if (fNleft < 0)
    LAUNCH(c, "k_search_by_bow", k_search_by_bow, dim3(nkf), dim3(512), lds, dOff, dKd, dKa, dKn, dKv, dFd, dFa, dSn, dSi, dListed, nf,
           keyCap, nnratio, checkOri ? 1 : 0, dM, dN);
  else
    LAUNCH(c, "k_search_by_bow_two_cameras", k_search_by_bow_two_cameras, dim3(nkf), dim3(512), lds, dOff, dKd, dKa, dKn, dKv, dFd, dFa,
           dSn, dSi, dListed, nf, fNleft, keyCap, nnratio, checkOri ? 1 : 0, dM, dN);
  HIPCHK(download(c, matches, dM));
  HIPCHK(download(c, nmatches, dN));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_search_by_bow(pli_ctx* c, int32_t nkf, const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle,
                             const int32_t* kfNode, const uint8_t* kfValid, const uint8_t* fDesc, const float* fAngle,
                             const int32_t* fNode, int32_t nf, float nnratio, int32_t checkOri, int32_t* matches, int32_t* nmatches) {
  CtxGuard guard__(c);
  return searchByBow(c, nkf, kfOff, kfDesc, kfAngle, kfNode, kfValid, fDesc, fAngle, fNode, nf, -1, nnratio, checkOri, matches, nmatches);
}

pli_status pli_search_by_bow_two_cameras(pli_ctx* c, int32_t nkf, const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle,
                                         const int32_t* kfNode, const uint8_t* kfValid, const uint8_t* fDesc, const float* fAngle,
                                         const int32_t* fNode, int32_t nf, int32_t fNleft, float nnratio, int32_t checkOri,
                                         int32_t* matches, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (fNleft < 0 || fNleft > nf) { g_err = "f_nleft outside [0, nf]"; return PLI_ERR_INVALID; }
  return searchByBow(c, nkf, kfOff, kfDesc, kfAngle, kfNode, kfValid, fDesc, fAngle, fNode, nf, fNleft, nnratio, checkOri, matches, nmatches);
}

pli_status pli_search_by_bow_kf(pli_ctx* c, const uint8_t* desc1, const float* angle1, const int32_t* node1, const uint8_t* valid1,
                                int32_t n1, int32_t nkf, const int32_t* kfOff, const uint8_t* kfDesc, const float* kfAngle,
                                const int32_t* kfNode, const uint8_t* kfValid, float nnratio, int32_t checkOri, int32_t* matches12,
                                int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || n1 < 0 || nkf < 0 || (n1 > 0 && (!desc1 || !node1 || !valid1 || (checkOri && !angle1))) ||
      (nkf > 0 && (!kfOff || !nmatches)) || (nkf > 0 && n1 > 0 && !matches12)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a keyframe has more features than the SearchByBoW cap", B);
  if (st != PLI_OK) return st;
  if (n1 > PLI_BOW_MAX_FEATURES) { g_err = "pKF1 has more features than the SearchByBoW cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total;
  if (total > 0 && (!kfDesc || !kfNode || !kfValid || (checkOri && !kfAngle))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nodesOk(kfNode, total, "kf_node") || !nodesOk(node1, n1, "node1")) return PLI_ERR_INVALID;
  if (checkOri && (!anglesOk(kfAngle, total, "kf_angle") || !anglesOk(angle1, n1, "angle1"))) return PLI_ERR_INVALID;
  if (n1 == 0) { std::fill(nmatches, nmatches + nkf, 0); return PLI_OK; }
  HIPCHK(hipSetDevice(c->device));
  ScratchPlan plan;
  auto dD1 = plan.in(desc1, (size_t)n1 * 32);
  auto dA1 = plan.in(checkOri ? angle1 : nullptr, n1);       // (the angles are read with checkOri only)
  auto dN1 = plan.in(node1, n1);
  auto dV1 = plan.in(valid1, n1);
  auto dOff = plan.in(kfOff, (size_t)nkf + 1);
  auto dKd = plan.in(kfDesc, (size_t)total * 32);
  auto dKa = plan.in(checkOri ? kfAngle : nullptr, total);
  auto dKn = plan.in(kfNode, total);
  auto dKv = plan.in(kfValid, total);
  auto dSn = plan.add<uint32_t>(total);
  auto dSi = plan.add<uint16_t>(total);
  auto dListed = plan.add<int>(nkf);
  auto dM = plan.add<int>((size_t)nkf * n1);
  auto dN = plan.add<int>(nkf);
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const int sortCap = pow2Ceil(B.maxNk), keyCap = pow2Ceil(n1);
  LAUNCH(c, "k_node_sort", k_node_sort, dim3(nkf), dim3(1024), (size_t)sortCap * 6, dOff, 0, dKn, dKv, 1, (const uint8_t*)nullptr, 0, sortCap,
         dSn, dSi, dListed, (int*)nullptr);
  LAUNCH(c, "k_search_by_bow_kf", k_search_by_bow_kf, dim3(nkf), dim3(512), 48 * 4 + (size_t)keyCap * 4 + alignUp((size_t)B.maxNk * 2, 16),
         dD1, dA1, dN1, dV1, n1, dOff, dKd, dKa, dSn, dSi, dListed, keyCap, nnratio, checkOri ? 1 : 0, dM, dN);
  HIPCHK(download(c, matches12, dM));
  HIPCHK(download(c, nmatches, dN));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_search_for_triangulation(pli_ctx* c, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                        const uint8_t* hasMp1, const uint8_t* stereo1, int32_t n1, int32_t nkf, const int32_t* kfOff,
                                        const pli_keypoint* kfKp, const uint8_t* kfDesc, const int32_t* kfNode, const uint8_t* kfHasMp,
                                        const uint8_t* kfStereo, const float* F12, const float* ep, int32_t onlyStereo, int32_t coarse,
                                        int32_t checkOri, int32_t* matches12, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || n1 < 0 || nkf < 0 || (n1 > 0 && (!kp1 || !desc1 || !node1 || !hasMp1 || !stereo1)) ||
      (nkf > 0 && (!kfOff || !F12 || !ep || !nmatches)) || (nkf > 0 && n1 > 0 && !matches12)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a neighbour has more features than the SearchForTriangulation cap", B);
  if (st != PLI_OK) return st;
  if (n1 > PLI_BOW_MAX_FEATURES) { g_err = "pKF1 has more features than the SearchForTriangulation cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total;
  if (total > 0 && (!kfKp || !kfDesc || !kfNode || !kfHasMp || !kfStereo)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nodesOk(node1, n1, "node1") || !octavesOk(c, kp1, n1, "kp1") || (checkOri && !anglesOk(kp1, n1, "kp1: angle"))) return PLI_ERR_INVALID;
  if (!nodesOk(kfNode, total, "kf_node") || !octavesOk(c, kfKp, total, "kf_kp") || (checkOri && !anglesOk(kfKp, total, "kf_kp: angle")))
    return PLI_ERR_INVALID;
  if (n1 == 0) { std::fill(nmatches, nmatches + nkf, 0); return PLI_OK; }
  HIPCHK(hipSetDevice(c->device));
  float hlv[2 * MAX_LEVELS] = {};
  levelTables(c, hlv, hlv + MAX_LEVELS, nullptr);
  ScratchPlan plan;
  const TriTables T = triTables(plan, B, kp1, desc1, node1, hasMp1, n1, kfKp, kfDesc, kfNode, kfHasMp);
  auto dS1 = plan.in(stereo1, n1);
  auto dKs = plan.in(kfStereo, total);
  auto dF = plan.in(F12, (size_t)nkf * 9);
  auto dEp = plan.in(ep, (size_t)nkf * 2);
  auto dLv = plan.in(hlv, 2 * MAX_LEVELS);                 // mvScaleFactors, then mvLevelSigma2
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const int keyCap = pow2Ceil(B.maxNk);
  const int perBlock = 4 * 4;                                            // k_tri_match: 4 waves x TRI_PER_WAVE features of pKF1
  LAUNCH(c, "k_node_sort", k_node_sort, dim3(nkf), dim3(1024), (size_t)keyCap * 6, T.dOff, 0, T.dKn, T.dKm, 0, dKs, onlyStereo ? 1 : 0,
         keyCap, T.dSn, T.dSi, T.dListed, T.dStat);
  LAUNCH(c, "k_tri_match", k_tri_match, dim3((n1 + perBlock - 1) / perBlock, nkf), dim3(256), 0, T.dK1, T.dD1, T.dN1, T.dM1, dS1, n1,
         T.dOff, T.dKk, T.dKd, dKs, T.dSn, T.dSi, T.dListed, dF, dEp, (const float*)dLv, (const float*)dLv + MAX_LEVELS,
         onlyStereo ? 1 : 0, coarse ? 1 : 0, checkOri ? 1 : 0, T.dM, T.dStat);
  return triEnd(c, B, n1, T, checkOri, matches12, nmatches);
}

pli_status pli_search_for_triangulation_two_cameras(pli_ctx* c, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                                    const uint8_t* hasMp1, int32_t n1, int32_t n1Left, int32_t nkf,
                                                    const int32_t* kfOff, const int32_t* kfNleft, const pli_keypoint* kfKp,
                                                    const uint8_t* kfDesc, const int32_t* kfNode, const uint8_t* kfHasMp,
                                                    const pli_kb8_camera* camLeft, const pli_kb8_camera* camRight, const float* rel,
                                                    int32_t onlyStereo, int32_t coarse, int32_t checkOri, int32_t* matches12,
                                                    int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || n1 < 0 || nkf < 0 || !camLeft || !camRight || (n1 > 0 && (!kp1 || !desc1 || !node1 || !hasMp1)) ||
      (nkf > 0 && (!kfOff || !kfNleft || !rel || !nmatches)) || (nkf > 0 && n1 > 0 && !matches12)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (n1Left < 0 || n1Left > n1) { g_err = "n1_left outside [0, n1]"; return PLI_ERR_INVALID; }
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a neighbour has more features than the SearchForTriangulation cap", B);
  if (st != PLI_OK) return st;
  if (n1 > PLI_BOW_MAX_FEATURES) { g_err = "pKF1 has more features than the SearchForTriangulation cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total;
  if (total > 0 && (!kfKp || !kfDesc || !kfNode || !kfHasMp)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nleftOk(nkf, kfOff, kfNleft, "kf_nleft outside [0, the neighbour's rows]")) return PLI_ERR_INVALID;
  // the gate projects with the coordinates and indexes mvLevelSigma2 by the octaves: the rule of pli_stereo_fisheye_tables
  if (!nodesOk(node1, n1, "node1") || !octavesOk(c, kp1, n1, "kp1") || !finiteOk(kp1, n1, "kp1") ||
      (checkOri && !anglesOk(kp1, n1, "kp1: angle")))
    return PLI_ERR_INVALID;
  if (!nodesOk(kfNode, total, "kf_node") || !octavesOk(c, kfKp, total, "kf_kp") || !finiteOk(kfKp, total, "kf_kp") ||
      (checkOri && !anglesOk(kfKp, total, "kf_kp: angle")))
    return PLI_ERR_INVALID;
  for (int64_t i = 0; i < (int64_t)nkf * 48; ++i)
    if (!std::isfinite(rel[i])) { g_err = "rel: a relative pose is not finite"; return PLI_ERR_INVALID; }
  std::fill(nmatches, nmatches + nkf, 0);
  if (n1 == 0) return PLI_OK;
  if (onlyStereo) {                                         // bStereo1 is false for every feature (:1041): :1043-1045 skips them all
    std::fill(matches12, matches12 + (size_t)nkf * n1, -1);
    return PLI_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  float hlv[MAX_LEVELS] = {};
  levelTables(c, nullptr, hlv, nullptr);
  ScratchPlan plan;
  const TriTables T = triTables(plan, B, kp1, desc1, node1, hasMp1, n1, kfKp, kfDesc, kfNode, kfHasMp);
  auto dR1 = plan.add<float2>(n1);
  auto dNl = plan.in(kfNleft, nkf);
  auto dKr = plan.add<float2>(total);
  auto dRel = plan.in(rel, (size_t)nkf * 48);
  auto dLv = plan.in(hlv, MAX_LEVELS);                     // mvLevelSigma2
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  Kb8 cl, cr;
  memcpy(&cl, camLeft, sizeof(cl));
  memcpy(&cr, camRight, sizeof(cr));
  const int keyCap = pow2Ceil(B.maxNk);
  const int perBlock = 4 * 4;                                            // k_tri_match_kb8: 4 waves x TRI_PER_WAVE features of pKF1
  const int64_t nray = (int64_t)n1 + total;
  if (!coarse)                                                           // (bCoarse: the gate, the only reader of the rays, does not run)
    LAUNCH(c, "k_kb8_rays", k_kb8_rays, dim3((unsigned)((nray + 255) / 256)), dim3(256), 0, (const pli_keypoint*)T.dK1, n1, n1Left,
           (const pli_keypoint*)T.dKk, (const int*)T.dOff, (const int*)dNl, nkf, cl, cr, (float2*)dR1, (float2*)dKr);
  LAUNCH(c, "k_node_sort", k_node_sort, dim3(nkf), dim3(1024), (size_t)keyCap * 6, T.dOff, 0, T.dKn, T.dKm, 0, (const uint8_t*)nullptr, 0,
         keyCap, T.dSn, T.dSi, T.dListed, T.dStat);
  LAUNCH(c, "k_tri_match_kb8", k_tri_match_kb8, dim3((n1 + perBlock - 1) / perBlock, nkf), dim3(256), 0, T.dK1, T.dD1, T.dN1, T.dM1,
         (const float2*)dR1, n1, n1Left, T.dOff, (const int*)dNl, T.dKk, T.dKd, (const float2*)dKr, T.dSn, T.dSi, T.dListed,
         (const float*)dRel, cl, cr, (const float*)dLv, coarse ? 1 : 0, checkOri ? 1 : 0, T.dM, T.dStat);
  return triEnd(c, B, n1, T, checkOri, matches12, nmatches);
}

pli_status pli_create_new_map_points(pli_ctx* c, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                     const uint8_t* hasMp1, const float* uright1, const float* depth1, const float* key1, int32_t n1,
                                     int32_t nkf, const int32_t* kfOff, const pli_keypoint* kfKp, const uint8_t* kfDesc,
                                     const int32_t* kfNode, const uint8_t* kfHasMp, const float* kfUright, const float* kfDepth,
                                     const float* kfKey, const float* F12, const float* ep, const float* pose1, const float* kfPose,
                                     const pli_fuse_camera* cam, float mb, int32_t coarse, int32_t farPoints, float thFar,
                                     float ratioFactor, int32_t* matches12, int32_t* nmatches, int32_t* status, float* x3d,
                                     int32_t* nnew) {
  CtxGuard guard__(c);
  if (!c || n1 < 0 || nkf < 0 || !cam || !pose1 ||
      (n1 > 0 && (!kp1 || !desc1 || !node1 || !hasMp1 || !uright1 || !depth1 || !key1)) ||
      (nkf > 0 && (!kfOff || !F12 || !ep || !kfPose || !nmatches || !nnew)) ||
      (nkf > 0 && n1 > 0 && (!matches12 || !status || !x3d))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a neighbour has more features than the CreateNewMapPoints cap", B);
  if (st != PLI_OK) return st;
  if (n1 > PLI_BOW_MAX_FEATURES) { g_err = "pKF1 has more features than the CreateNewMapPoints cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total, npairs = (int64_t)nkf * n1;
  // (k_newpt_list indexes a pair with an int, rounded up to its block of 256)
  if (npairs > INT32_MAX - 256) { g_err = "nkf x n1 does not fit the pair index"; return PLI_ERR_CAPACITY; }
  if (total > 0 && (!kfKp || !kfDesc || !kfNode || !kfHasMp || !kfUright || !kfDepth || !kfKey)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nodesOk(node1, n1, "node1") || !octavesOk(c, kp1, n1, "kp1") || !finiteOk(kp1, n1, "kp1")) return PLI_ERR_INVALID;
  if (!nodesOk(kfNode, total, "kf_node") || !octavesOk(c, kfKp, total, "kf_kp") || !finiteOk(kfKp, total, "kf_kp")) return PLI_ERR_INVALID;
  if (!floatsFinite(uright1, n1, "uright1") || !floatsFinite(depth1, n1, "depth1") || !floatsFinite(key1, 2 * (int64_t)n1, "key1") ||
      !floatsFinite(kfUright, total, "kf_uright") || !floatsFinite(kfDepth, total, "kf_depth") ||
      !floatsFinite(kfKey, 2 * total, "kf_key") || !floatsFinite(pose1, 15, "pose1") ||
      !floatsFinite(kfPose, 15 * (int64_t)nkf, "kf_pose"))
    return PLI_ERR_INVALID;
  std::fill(nmatches, nmatches + nkf, 0);
  std::fill(nnew, nnew + nkf, 0);
  if (n1 == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  float hlv[2 * MAX_LEVELS] = {};
  levelTables(c, hlv, hlv + MAX_LEVELS, nullptr);
  // bStereo = mvuRight >= 0 (ORBmatcher.cc:1041, :1070; LocalMapping.cc:450, :459): the flag tables of the search
  std::vector<uint8_t> stereo1(n1), kfStereo((size_t)total);
  for (int i = 0; i < n1; ++i) stereo1[i] = uright1[i] >= 0;
  for (int64_t i = 0; i < total; ++i) kfStereo[i] = kfUright[i] >= 0;
  ScratchPlan plan;
  const TriTables T = triTables(plan, B, kp1, desc1, node1, hasMp1, n1, kfKp, kfDesc, kfNode, kfHasMp);
  auto dS1 = plan.in(stereo1.data(), n1);
  auto dKs = plan.in(kfStereo.data(), total);
  auto dF = plan.in(F12, (size_t)nkf * 9);
  auto dEp = plan.in(ep, (size_t)nkf * 2);
  auto dLv = plan.in(hlv, 2 * MAX_LEVELS);                 // mvScaleFactors, then mvLevelSigma2
  auto dU1 = plan.in(uright1, n1);
  auto dZ1 = plan.in(depth1, n1);
  auto dP1 = plan.in(key1, (size_t)n1 * 2);
  auto dKu = plan.in(kfUright, total);
  auto dKz = plan.in(kfDepth, total);
  auto dKp = plan.in(kfKey, (size_t)total * 2);
  auto dPose1 = plan.in(pose1, 15);
  auto dKpose = plan.in(kfPose, (size_t)nkf * 15);
  auto dList = plan.add<int>(npairs);
  auto dCnt = plan.add<int>(1 + 2 * (size_t)nkf);          // the list's length, nmatches[nkf], nnew[nkf]
  auto dStatus = plan.add<int>(npairs);
  auto dX = plan.add<float>((size_t)npairs * 3);
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemsetAsync(dCnt, 0, (1 + 2 * (size_t)nkf) * sizeof(int), c->stream));
  const int keyCap = pow2Ceil(B.maxNk);
  const int perBlock = 4 * 4;                                            // k_tri_match: 4 waves x TRI_PER_WAVE features of pKF1
  LAUNCH(c, "k_node_sort", k_node_sort, dim3(nkf), dim3(1024), (size_t)keyCap * 6, T.dOff, 0, T.dKn, T.dKm, 0, dKs, 0,
         keyCap, T.dSn, T.dSi, T.dListed, T.dStat);
  LAUNCH(c, "k_tri_match", k_tri_match, dim3((n1 + perBlock - 1) / perBlock, nkf), dim3(256), 0, T.dK1, T.dD1, T.dN1, T.dM1, dS1, n1,
         T.dOff, T.dKk, T.dKd, dKs, T.dSn, T.dSi, T.dListed, dF, dEp, (const float*)dLv, (const float*)dLv + MAX_LEVELS,
         0, coarse ? 1 : 0, 0, T.dM, T.dStat);
  int* cnt = dCnt;
  LAUNCH(c, "k_newpt_list", k_newpt_list, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, (const int*)T.dM, (int)npairs,
         (int*)dList, cnt, (int*)dStatus, (float*)dX);
  const NewPtTables D = {T.dK1, dU1, dZ1, (const float2*)(float*)dP1, dPose1, n1, T.dOff, T.dKk, dKu, dKz, (const float2*)(float*)dKp,
                         dKpose, (const float*)dLv, (const float*)dLv + MAX_LEVELS};
  const unsigned geoBlocks = (unsigned)std::min<int64_t>((npairs + 63) / 64, 2048);
  LAUNCH(c, "k_newpt_geometry", k_newpt_geometry, dim3(geoBlocks), dim3(64), 0, D, *cam, mb, farPoints ? 1 : 0, thFar, ratioFactor,
         (const int*)T.dM, (const int*)dList, (const int*)cnt, (int*)dStatus, (float*)dX);
  LAUNCH(c, "k_newpt_pick", k_newpt_pick, dim3((n1 + 255) / 256), dim3(256), 0, n1, nkf, (int*)T.dM, (int*)dStatus, cnt + 1, cnt + 1 + nkf);
  HIPCHK(download(c, matches12, T.dM));
  HIPCHK(download(c, status, dStatus));
  HIPCHK(download(c, x3d, dX));
  HIPCHK(download(c, nmatches, dCnt, 1, nkf));
  HIPCHK(download(c, nnew, dCnt, 1 + nkf, nkf));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_create_new_map_points_two_cameras(pli_ctx* c, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                                 const uint8_t* hasMp1, int32_t n1, int32_t n1Left, int32_t nkf, const int32_t* kfOff,
                                                 const int32_t* kfNleft, const pli_keypoint* kfKp, const uint8_t* kfDesc,
                                                 const int32_t* kfNode, const uint8_t* kfHasMp, const pli_kb8_camera* camLeft,
                                                 const pli_kb8_camera* camRight, const float* rel, const float* pose1,
                                                 const float* kfPose, int32_t coarse, int32_t farPoints, float thFar,
                                                 float ratioFactor, int32_t* matches12, int32_t* nmatches, int32_t* status, float* x3d,
                                                 int32_t* nnew) {
  CtxGuard guard__(c);
  if (!c || n1 < 0 || nkf < 0 || !camLeft || !camRight || !pose1 || (n1 > 0 && (!kp1 || !desc1 || !node1 || !hasMp1)) ||
      (nkf > 0 && (!kfOff || !kfNleft || !rel || !kfPose || !nmatches || !nnew)) ||
      (nkf > 0 && n1 > 0 && (!matches12 || !status || !x3d))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (n1Left < 0 || n1Left > n1) { g_err = "n1_left outside [0, n1]"; return PLI_ERR_INVALID; }
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a neighbour has more features than the CreateNewMapPoints cap", B);
  if (st != PLI_OK) return st;
  if (n1 > PLI_BOW_MAX_FEATURES) { g_err = "pKF1 has more features than the CreateNewMapPoints cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total, npairs = (int64_t)nkf * n1;
  // (k_newpt_list indexes a pair with an int, rounded up to its block of 256)
  if (npairs > INT32_MAX - 256) { g_err = "nkf x n1 does not fit the pair index"; return PLI_ERR_CAPACITY; }
  if (total > 0 && (!kfKp || !kfDesc || !kfNode || !kfHasMp)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nleftOk(nkf, kfOff, kfNleft, "kf_nleft outside [0, the neighbour's rows]")) return PLI_ERR_INVALID;
  if (!nodesOk(node1, n1, "node1") || !octavesOk(c, kp1, n1, "kp1") || !finiteOk(kp1, n1, "kp1")) return PLI_ERR_INVALID;
  if (!nodesOk(kfNode, total, "kf_node") || !octavesOk(c, kfKp, total, "kf_kp") || !finiteOk(kfKp, total, "kf_kp")) return PLI_ERR_INVALID;
  if (!floatsFinite(rel, 48 * (int64_t)nkf, "rel") || !floatsFinite(pose1, 30, "pose1") ||
      !floatsFinite(kfPose, 30 * (int64_t)nkf, "kf_pose"))
    return PLI_ERR_INVALID;
  std::fill(nmatches, nmatches + nkf, 0);
  std::fill(nnew, nnew + nkf, 0);
  if (n1 == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  float hlv[2 * MAX_LEVELS] = {};
  levelTables(c, hlv, hlv + MAX_LEVELS, nullptr);
  ScratchPlan plan;
  const TriTables T = triTables(plan, B, kp1, desc1, node1, hasMp1, n1, kfKp, kfDesc, kfNode, kfHasMp);
  auto dR1 = plan.add<float2>(n1);
  auto dNl = plan.in(kfNleft, nkf);
  auto dKr = plan.add<float2>(total);
  auto dRel = plan.in(rel, (size_t)nkf * 48);
  auto dLv = plan.in(hlv, 2 * MAX_LEVELS);                 // mvScaleFactors, then mvLevelSigma2
  auto dPose1 = plan.in(pose1, 30);
  auto dKpose = plan.in(kfPose, (size_t)nkf * 30);
  auto dList = plan.add<int>(npairs);
  auto dCnt = plan.add<int>(1 + 2 * (size_t)nkf);          // the list's length, nmatches[nkf], nnew[nkf]
  auto dStatus = plan.add<int>(npairs);
  auto dX = plan.add<float>((size_t)npairs * 3);
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemsetAsync(dCnt, 0, (1 + 2 * (size_t)nkf) * sizeof(int), c->stream));
  Kb8 cl, cr;
  memcpy(&cl, camLeft, sizeof(cl));
  memcpy(&cr, camRight, sizeof(cr));
  const int keyCap = pow2Ceil(B.maxNk);
  const int perBlock = 4 * 4;                                            // k_tri_match_kb8: 4 waves x TRI_PER_WAVE features of pKF1
  const int64_t nray = (int64_t)n1 + total;
  const float* sigma2 = (const float*)dLv + MAX_LEVELS;
  // (also when bCoarse: the search's gate does not run then, but the geometry reads the rays)
  LAUNCH(c, "k_kb8_rays", k_kb8_rays, dim3((unsigned)((nray + 255) / 256)), dim3(256), 0, (const pli_keypoint*)T.dK1, n1, n1Left,
         (const pli_keypoint*)T.dKk, (const int*)T.dOff, (const int*)dNl, nkf, cl, cr, (float2*)dR1, (float2*)dKr);
  LAUNCH(c, "k_node_sort", k_node_sort, dim3(nkf), dim3(1024), (size_t)keyCap * 6, T.dOff, 0, T.dKn, T.dKm, 0, (const uint8_t*)nullptr, 0,
         keyCap, T.dSn, T.dSi, T.dListed, T.dStat);
  LAUNCH(c, "k_tri_match_kb8", k_tri_match_kb8, dim3((n1 + perBlock - 1) / perBlock, nkf), dim3(256), 0, T.dK1, T.dD1, T.dN1, T.dM1,
         (const float2*)dR1, n1, n1Left, T.dOff, (const int*)dNl, T.dKk, T.dKd, (const float2*)dKr, T.dSn, T.dSi, T.dListed,
         (const float*)dRel, cl, cr, sigma2, coarse ? 1 : 0, 0, T.dM, T.dStat);
  int* cnt = dCnt;
  LAUNCH(c, "k_newpt_list", k_newpt_list, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, (const int*)T.dM, (int)npairs,
         (int*)dList, cnt, (int*)dStatus, (float*)dX);
  const NewPtKb8Tables D = {T.dK1, (const float2*)dR1, dPose1, n1, n1Left, T.dOff, dNl, T.dKk, (const float2*)dKr, dKpose,
                            (const float*)dLv, sigma2};
  const unsigned geoBlocks = (unsigned)std::min<int64_t>((npairs + 63) / 64, 2048);
  LAUNCH(c, "k_newpt_geometry_kb8", k_newpt_geometry_kb8, dim3(geoBlocks), dim3(64), 0, D, cl, cr, farPoints ? 1 : 0, thFar,
         ratioFactor, (const int*)T.dM, (const int*)dList, (const int*)cnt, (int*)dStatus, (float*)dX);
  LAUNCH(c, "k_newpt_pick", k_newpt_pick, dim3((n1 + 255) / 256), dim3(256), 0, n1, nkf, (int*)T.dM, (int*)dStatus, cnt + 1, cnt + 1 + nkf);
  HIPCHK(download(c, matches12, T.dM));
  HIPCHK(download(c, status, dStatus));
  HIPCHK(download(c, x3d, dX));
  HIPCHK(download(c, nmatches, dCnt, 1, nkf));
  HIPCHK(download(c, nnew, dCnt, 1 + nkf, nkf));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

// The tables that the projection launch of a Fuse entry point reads and writes (lv: level_ratio, then mvScaleFactors)
struct FuseProjectTables {
  const pli_fuse_point* mp; const float* pose; const uint8_t* skip; const float* lv;
  FuseSurvivor* surv; int* nSurv; int* bestIdx; int* bestDist;
};

// pli_fuse_search (a view = a keyframe) and pli_fuse_search_two_cameras (a view = a keyframe's left or right rows) from the plan to the
// synchronise.  viewOff: nview + 1 ascending offsets into the keyframes' rows; pose: 15 floats per view; cam: the camera of k_fuse_grid
// and of the window walk; kfUright: mvuRight, or null where `match` does not read it; project: the entry's projection launch; match: its
// k_fuse_match instantiation.
static pli_status fuseSearch(pli_ctx* c, const pli_fuse_point* mp, const uint8_t* mpDesc, int32_t nmp, int32_t nview, const int32_t* viewOff,
                             const pli_keypoint* kfKp, const uint8_t* kfDesc, bool withUright, const float* kfUright, const float* pose,
                             const uint8_t* skip, const pli_fuse_camera& cam, const float* levelRatio, int32_t reprojGate,
                             const std::function<pli_status(const FuseProjectTables&)>& project, decltype(&k_fuse_match<8, false>) match,
                             int32_t* bestIdx, int32_t* bestDist) {
  const size_t npairs = (size_t)nview * nmp, total = (size_t)viewOff[nview];
  const LevelBlock hlv(c, levelRatio, 3);
  ScratchPlan plan;
  auto dMp = plan.in(mp, nmp);
  auto dMd = plan.in(mpDesc, (size_t)nmp * 32);
  auto dOff = plan.in(viewOff, (size_t)nview + 1);
  auto dKk = plan.in(kfKp, total);
  auto dKd = plan.in(kfDesc, total * 32);
  auto dKu = withUright ? plan.in(kfUright, total) : plan.addIf<float>(false, 0);
  auto dPose = plan.in(pose, (size_t)nview * 15);
  auto dSkip = plan.inOpt(skip, npairs);
  auto dLv = plan.in(hlv.v, 3 * MAX_LEVELS);                // level_ratio, mvScaleFactors, mvInvLevelSigma2
  auto dCell = plan.add<int>((size_t)nview * (GRID_COLS * GRID_ROWS + 1));
  auto dSi = plan.add<uint16_t>(total);
  auto dSurv = plan.add<FuseSurvivor>(npairs);
  auto dNs = plan.add<int>(1);
  auto dBi = plan.add<int>(npairs);
  auto dBd = plan.addIf<int>(bestDist != nullptr, npairs);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  HIPCHK(hipMemsetAsync(dNs, 0, sizeof(int), c->stream));
  const float* lv = dLv;
  LAUNCH(c, "k_fuse_grid", k_fuse_grid, dim3(nview), dim3(256), 0, dOff, dKk, cam, dCell, dSi);
  if ((st = project(FuseProjectTables{dMp, dPose, dSkip, lv, dSurv, dNs, dBi, dBd})) != PLI_OK) return st;
  LAUNCH(c, "k_fuse_match", match, dim3(1024), dim3(256), 0, dSurv, dNs, nmp, dMd, dOff, dKk, dKd, dKu, dCell, dSi, cam, lv + 2 * MAX_LEVELS,
         reprojGate ? 1 : 0, dBi, dBd);
  HIPCHK(download(c, bestIdx, dBi));
  HIPCHK(download(c, bestDist, dBd));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_fuse_search(pli_ctx* c, const pli_fuse_point* mp, const uint8_t* mpDesc, int32_t nmp, int32_t nkf, const int32_t* kfOff,
                           const pli_keypoint* kfKp, const uint8_t* kfDesc, const float* kfUright, const float* kfPose,
                           const uint8_t* skip, const pli_fuse_camera* cam, float th, const float* levelRatio, int32_t reprojGate,
                           int32_t* bestIdx, int32_t* bestDist) {
  CtxGuard guard__(c);
  if (!c || nmp < 0 || nkf < 0 || !cam || !levelRatio || (nmp > 0 && (!mp || !mpDesc)) || (nkf > 0 && (!kfOff || !kfPose)) ||
      (nkf > 0 && nmp > 0 && !bestIdx)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!levelRatioOk(c, levelRatio) || !imageBoundsOk(cam->min_x, cam->max_x, cam->min_y, cam->max_y)) return PLI_ERR_INVALID;
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a keyframe has more features than the Fuse cap", B);
  if (st != PLI_OK) return st;
  const int64_t total = B.total;
  if (total > 0 && (!kfKp || !kfDesc || (reprojGate && !kfUright))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!octavesOk(c, kfKp, total, "kf_kp")) return PLI_ERR_INVALID;
  if (nmp == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t npairs = (size_t)nkf * nmp;
  auto project = [&](const FuseProjectTables& D) -> pli_status {
    LAUNCH(c, "k_fuse_project", k_fuse_project, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, D.mp, nmp, nkf, D.pose, D.skip, *cam,
           th, D.lv, c->hp.nlevels, D.lv + MAX_LEVELS, D.surv, D.nSurv, D.bestIdx, D.bestDist);
    return PLI_OK;
  };
  // lanes per surviving pair (Fuse: 8 measured best; the development build can run the other widths)
  int lanes = 8;
  if (const char* e = DEVENV("PLI_FUSE_LANES")) lanes = atoi(e);
  const auto match = lanes == 16 ? k_fuse_match<16, false> : lanes == 64 ? k_fuse_match<64, false> : k_fuse_match<8, false>;
  // (mvuRight is read by the chi-square gate only)
  return fuseSearch(c, mp, mpDesc, nmp, nkf, kfOff, kfKp, kfDesc, true, reprojGate ? kfUright : nullptr, kfPose, skip, *cam, levelRatio,
                    reprojGate, project, match, bestIdx, bestDist);
}

pli_status pli_fuse_search_two_cameras(pli_ctx* c, const pli_fuse_point* mp, const uint8_t* mpDesc, int32_t nmp, int32_t nkf,
                                       const int32_t* kfOff, const int32_t* kfNleft, const pli_keypoint* kfKp, const uint8_t* kfDesc,
                                       const float* kfPose, const uint8_t* skip, const pli_kb8_camera* camLeft,
                                       const pli_kb8_camera* camRight, float minX, float maxX, float minY, float maxY, float th,
                                       const float* levelRatio, int32_t sides, int32_t* bestIdx, int32_t* bestDist) {
  CtxGuard guard__(c);
  if (!c || nmp < 0 || nkf < 0 || !camLeft || !camRight || !levelRatio || (nmp > 0 && (!mp || !mpDesc)) ||
      (nkf > 0 && (!kfOff || !kfNleft || !kfPose)) || (nkf > 0 && nmp > 0 && !bestIdx)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (sides < 1 || sides > 3) { g_err = "sides: bit 0 = left, bit 1 = right, at least one"; return PLI_ERR_INVALID; }
  if (!levelRatioOk(c, levelRatio) || !imageBoundsOk(minX, maxX, minY, maxY)) return PLI_ERR_INVALID;
  if (nkf == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(nkf, kfOff, "a keyframe has more features than the Fuse cap", B);
  if (st != PLI_OK) return st;
  const int64_t total = B.total;
  if (total > 0 && (!kfKp || !kfDesc)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!nleftOk(nkf, kfOff, kfNleft, "kf_nleft outside [0, the keyframe's rows]")) return PLI_ERR_INVALID;
  if (!octavesOk(c, kfKp, total, "kf_kp") || !finiteOk(kfKp, total, "kf_kp")) return PLI_ERR_INVALID;
  for (int64_t i = 0; i < (int64_t)nkf * 30; ++i)
    if (!std::isfinite(kfPose[i])) { g_err = "kf_pose: a pose is not finite"; return PLI_ERR_INVALID; }
  if (nmp == 0) return PLI_OK;
  HIPCHK(hipSetDevice(c->device));
  const int nview = 2 * nkf;
  const size_t npairs = (size_t)nview * nmp;
  // view 2k = keyframe k's left rows, view 2k + 1 its right rows: one ascending offset list for k_fuse_grid and the window walk
  std::vector<int> viewOff((size_t)nview + 1);
  for (int k = 0; k < nkf; ++k) { viewOff[2 * k] = kfOff[k]; viewOff[2 * k + 1] = kfOff[k] + kfNleft[k]; }
  viewOff[nview] = kfOff[nkf];
  Kb8 cl, cr;
  memcpy(&cl, camLeft, sizeof(cl));
  memcpy(&cr, camRight, sizeof(cr));
  pli_fuse_camera bounds = {};                              // only the bounds are read (IsInImage, the 64 x 48 grid)
  bounds.min_x = minX; bounds.max_x = maxX; bounds.min_y = minY; bounds.max_y = maxY;
  auto project = [&](const FuseProjectTables& D) -> pli_status {
    LAUNCH(c, "k_fuse_project_views", k_fuse_project_views, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, D.mp, nmp, nkf, D.pose,
           D.skip, cl, cr, bounds, sides, th, D.lv, c->hp.nlevels, D.lv + MAX_LEVELS, D.surv, D.nSurv, D.bestIdx, D.bestDist);
    return PLI_OK;
  };
  // (the views' gate is the monocular one: no mvuRight)
  return fuseSearch(c, mp, mpDesc, nmp, nview, viewOff.data(), kfKp, kfDesc, false, nullptr, kfPose, skip, bounds, levelRatio, 1, project,
                    k_fuse_match<8, true>, bestIdx, bestDist);
}

pli_status pli_search_by_projection_sim3(pli_ctx* c, const pli_fuse_point* mp, const uint8_t* mpDesc, int32_t nmp, int32_t npair,
                                         const int32_t* kfOff, const pli_keypoint* kfKp, const uint8_t* kfDesc, const float* kfPose,
                                         const uint8_t* skip, const uint8_t* occupied, const pli_fuse_camera* cam, float th,
                                         const float* levelRatio, float ratioHamming, int32_t projectForm, int32_t* rowPoint,
                                         int32_t* bestIdx, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || nmp < 0 || npair < 0 || !cam || !levelRatio || (nmp > 0 && (!mp || !mpDesc)) || (npair > 0 && (!kfOff || !kfPose || !nmatches)) ||
      (projectForm != 0 && projectForm != 1)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!levelRatioOk(c, levelRatio) || !imageBoundsOk(cam->min_x, cam->max_x, cam->min_y, cam->max_y)) return PLI_ERR_INVALID;
  // bestDist <= TH_LOW * ratioHamming (ORBmatcher.cc:577): a float product, one rounding.  With no candidate the reference holds
  // bestDist = 256, bestIdx = -1 and would write vpMatched[-1] if the product reached 256
  const float limit = 50.0f * ratioHamming;
  if (!std::isfinite(ratioHamming) || !(ratioHamming > 0.f) || !(limit < 256.0f)) {
    g_err = "ratio_hamming must be finite, > 0 and 50 * ratio_hamming < 256";
    return PLI_ERR_INVALID;
  }
  const int distLimit = (int)std::floor(limit);             // (float)d <= limit  <=>  d <= floor(limit) for the integers d < 256
  if (npair == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(npair, kfOff, "a keyframe has more features than the projection search cap", B);
  if (st != PLI_OK) return st;
  const int64_t total = B.total;
  if (total > 0 && (!kfKp || !kfDesc || !rowPoint)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!octavesOk(c, kfKp, total, "kf_kp")) return PLI_ERR_INVALID;
  std::fill(nmatches, nmatches + npair, 0);
  if (nmp == 0 || total == 0) {
    if (total > 0) std::fill(rowPoint, rowPoint + total, -1);
    if (bestIdx) std::fill(bestIdx, bestIdx + (size_t)npair * nmp, -1);
    return PLI_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  const int width = sim3ListWidth();
  const size_t nslot = (size_t)npair * nmp;
  const LevelBlock hlv(c, levelRatio, 2);
  ScratchPlan plan;
  auto dMp = plan.in(mp, nmp);
  auto dMd = plan.in(mpDesc, (size_t)nmp * 32);
  auto dOff = plan.in(kfOff, (size_t)npair + 1);
  auto dKk = plan.in(kfKp, total);
  auto dKd = plan.in(kfDesc, (size_t)total * 32);
  auto dPose = plan.in(kfPose, (size_t)npair * 15);
  auto dSkip = plan.inOpt(skip, nslot);
  auto dOcc = plan.inOpt(occupied, total);
  auto dLv = plan.in(hlv.v, 2 * MAX_LEVELS);                // level_ratio, mvScaleFactors
  auto dCell = plan.add<int>((size_t)npair * (GRID_COLS * GRID_ROWS + 1));
  auto dSi = plan.add<uint16_t>(total);
  auto dSurv = plan.add<FuseSurvivor>(nslot);
  auto dKeys = plan.add<unsigned long long>(nslot * width);
  auto dCnt = plan.add<int>(nslot);
  auto dRow = plan.add<int>(total);
  auto dBi = plan.addIf<int>(bestIdx != nullptr, nslot);
  auto dNm = plan.add<int>(npair);
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const float* lv = dLv;
  LAUNCH(c, "k_fuse_grid", k_fuse_grid, dim3(npair), dim3(256), 0, dOff, dKk, *cam, dCell, dSi);
  LAUNCH(c, "k_sim3_project", k_sim3_project, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, dMp, nmp, npair, dPose, dSkip, *cam,
         th, lv, c->hp.nlevels, lv + MAX_LEVELS, projectForm, dSurv, dCnt, dBi);
  LAUNCH(c, "k_sim3_candidates", k_window_candidates<0>, dim3(1024), dim3(256), 0, dSurv, (int64_t)nslot, dMd, dOff, dKk, dKd, dCell, dSi, *cam,
         distLimit, width, dKeys, dCnt);
  LAUNCH(c, "k_sim3_assign", k_sim3_assign, dim3(npair), dim3(64), (size_t)B.maxNk * sizeof(int), dSurv, nmp, dMd, dOff, dKk, dKd, dOcc,
         dCell, dSi, *cam, distLimit, width, dKeys, dCnt, dRow, dBi, dNm);
  HIPCHK(download(c, rowPoint, dRow));
  HIPCHK(download(c, bestIdx, dBi));
  HIPCHK(download(c, nmatches, dNm));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

pli_status pli_search_by_projection_reloc(pli_ctx* c, int32_t ncand, const int32_t* mpOff, const pli_fuse_point* mp,
                                          const uint8_t* mpDesc, const float* mpAngle, const float* pose, const pli_keypoint* fKp,
                                          const uint8_t* fDesc, int32_t nf, const uint8_t* occupied, const pli_fuse_camera* cam,
                                          float th, const float* levelRatio, int32_t orbDist, int32_t checkOri, int32_t* rowPoint,
                                          int32_t* bestIdx, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || ncand < 0 || nf < 0 || !cam || !levelRatio || (ncand > 0 && (!mpOff || !pose || !nmatches)) || (nf > 0 && (!fKp || !fDesc)) ||
      (ncand > 0 && nf > 0 && !rowPoint)) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!levelRatioOk(c, levelRatio) || !imageBoundsOk(cam->min_x, cam->max_x, cam->min_y, cam->max_y)) return PLI_ERR_INVALID;
  // bestDist <= ORBdist (ORBmatcher.cc:2403): with no candidate the reference holds bestDist = 256, bestIdx2 = -1 and would write
  // mvpMapPoints[-1] at 256
  if (orbDist < 0 || orbDist > 255) { g_err = "orb_dist must lie in [0, 255]"; return PLI_ERR_INVALID; }
  if (ncand == 0) return PLI_OK;
  KfBatch B;
  pli_status st = kfBatch(ncand, mpOff, "a candidate lists more points than the projection search cap", B);
  if (st != PLI_OK) return st;
  if (nf > PLI_BOW_MAX_FEATURES) { g_err = "the frame has more features than the projection search cap"; return PLI_ERR_CAPACITY; }
  const int64_t total = B.total;
  if (total > 0 && (!mp || !mpDesc || (checkOri && !mpAngle))) { g_err = "bad argument"; return PLI_ERR_INVALID; }
  if (!octavesOk(c, fKp, nf, "f_kp")) return PLI_ERR_INVALID;
  if (checkOri && (!anglesOk(mpAngle, total, "mp_angle") || !anglesOk(fKp, nf, "f_kp angle"))) return PLI_ERR_INVALID;
  std::fill(nmatches, nmatches + ncand, 0);
  if (total == 0 || nf == 0) {
    if (nf > 0) std::fill(rowPoint, rowPoint + (size_t)ncand * nf, -1);
    if (bestIdx) std::fill(bestIdx, bestIdx + total, -1);
    return PLI_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  const int width = sim3ListWidth();
  const size_t nrow = (size_t)ncand * nf;
  const LevelBlock hlv(c, levelRatio, 2);
  const OneTableOff fOff(nf);
  ScratchPlan plan;
  auto dOff = plan.in(mpOff, (size_t)ncand + 1);
  auto dMp = plan.in(mp, total);
  auto dMd = plan.in(mpDesc, (size_t)total * 32);
  auto dMa = plan.inOpt(checkOri ? mpAngle : nullptr, total);
  auto dPose = plan.in(pose, (size_t)ncand * 15);
  auto dFoff = plan.in(fOff.off, 2);                        // the frame as the one table of k_fuse_grid: {0, nf}
  auto dKk = plan.in(fKp, nf);
  auto dKd = plan.in(fDesc, (size_t)nf * 32);
  auto dOcc = plan.inOpt(occupied, nrow);
  auto dLv = plan.in(hlv.v, 2 * MAX_LEVELS);                // level_ratio, mvScaleFactors
  auto dCell = plan.add<int>(GRID_COLS * GRID_ROWS + 1);
  auto dSi = plan.add<uint16_t>(nf);
  auto dSurv = plan.add<FuseSurvivor>(total);
  auto dKeys = plan.add<unsigned long long>((size_t)total * width);
  auto dCnt = plan.add<int>(total);
  auto dRow = plan.add<int>(nrow);
  auto dBi = plan.addIf<int>(bestIdx != nullptr, total);
  auto dNm = plan.add<int>(ncand);
  st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  const float* lv = dLv;
  LAUNCH(c, "k_fuse_grid", k_fuse_grid, dim3(1), dim3(256), 0, dFoff, dKk, *cam, dCell, dSi);
  LAUNCH(c, "k_reloc_project", k_reloc_project, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dMp, dOff, ncand, dPose, *cam, th, lv,
         c->hp.nlevels, lv + MAX_LEVELS, dSurv, dCnt, dBi);
  LAUNCH(c, "k_reloc_candidates", k_window_candidates<1>, dim3(1024), dim3(256), 0, dSurv, (int64_t)total, dMd, dFoff, dKk, dKd, dCell, dSi,
         *cam, orbDist, width, dKeys, dCnt);
  LAUNCH(c, "k_reloc_assign", k_reloc_assign, dim3(ncand), dim3(64), (size_t)(48 + nf) * sizeof(int), dSurv, dOff, dMd, dMa, dFoff, dKk,
         dKd, nf, dOcc, dCell, dSi, *cam, orbDist, width, checkOri ? 1 : 0, dKeys, dCnt, dRow, dBi, dNm);
  HIPCHK(download(c, rowPoint, dRow));
  HIPCHK(download(c, bestIdx, dBi));
  HIPCHK(download(c, nmatches, dNm));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

constexpr int INIT_LIST_WIDTH = 16;

pli_status pli_search_for_initialization(pli_ctx* c, const pli_keypoint* kp1, const uint8_t* desc1, int32_t n1,
                                         const float* prevMatched, const pli_keypoint* kp2, const uint8_t* desc2, int32_t n2,
                                         float minX, float maxX, float minY, float maxY, int32_t windowSize, float nnratio,
                                         int32_t checkOri, int32_t* matches12, int32_t* raw12, int32_t* nmatches) {
  CtxGuard guard__(c);
  if (!c || n1 < 0 || n2 < 0 || !nmatches || (n1 > 0 && (!kp1 || !desc1 || !prevMatched || !matches12)) || (n2 > 0 && (!kp2 || !desc2))) {
    g_err = "bad argument"; return PLI_ERR_INVALID;
  }
  if (windowSize < 0) { g_err = "window_size must not be negative"; return PLI_ERR_INVALID; }
  if (!std::isfinite(nnratio) || !(nnratio > 0.f)) { g_err = "nnratio must be finite and positive"; return PLI_ERR_INVALID; }
  if (!imageBoundsOk(minX, maxX, minY, maxY)) return PLI_ERR_INVALID;
  if (n1 > PLI_BOW_MAX_FEATURES) { g_err = "F1 has more features than the initialisation search cap"; return PLI_ERR_CAPACITY; }
  if (n2 > PLI_BOW_MAX_FEATURES) { g_err = "F2 has more features than the initialisation search cap"; return PLI_ERR_CAPACITY; }
  if (!octavesOk(c, kp1, n1, "kp1") || !octavesOk(c, kp2, n2, "kp2")) return PLI_ERR_INVALID;
  if (checkOri && (!anglesOk(kp1, n1, "kp1 angle") || !anglesOk(kp2, n2, "kp2 angle"))) return PLI_ERR_INVALID;
  for (int64_t i = 0; i < 2 * (int64_t)n1; ++i)
    if (std::isnan(prevMatched[i])) { g_err = "prev_matched holds a NaN"; return PLI_ERR_INVALID; }
  *nmatches = 0;
  if (n1 == 0 || n2 == 0) {
    std::fill(matches12, matches12 + n1, -1);
    if (raw12) std::fill(raw12, raw12 + n1, -1);
    return PLI_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  // The limit of the per-i1 candidate lists.  A candidate at distance d can bear on a decision in two ways only.  As a best: :760
  // needs d <= TH_LOW.  As a second-best that rejects a best b <= TH_LOW: :762 rejects when b >= (float)d * nnratio, and with
  // b <= 50 that needs (float)d * nnratio <= 50.0f, which is monotone in d for nnratio > 0.  A candidate above both bounds is
  // never a best that is accepted (if it were the minimum, every other candidate would be above TH_LOW too) and as a second-best
  // it behaves like INT_MAX: (float)d * nnratio > 50.0f >= b accepts, as does a missing second-best.  Whether it is left out by
  // vMatchedDistance (:745) changes nothing either, and it never enters vMatchedDistance, which only holds accepted distances.
  // So the lists keep d <= max(TH_LOW, the largest d with (float)d * nnratio <= 50.0f): 55 for 0.9.
  int distLimit = 50;
  while (distLimit < 256 && (float)(distLimit + 1) * nnratio <= 50.0f) ++distLimit;
  const int width = INIT_LIST_WIDTH;
  const OneTableOff off2(n2);
  ScratchPlan plan;
  auto dOff = plan.in(off2.off, 2);                         // F2 as the one table of k_fuse_grid: {0, n2}
  auto dK1 = plan.in(kp1, n1);
  auto dD1 = plan.in(desc1, (size_t)n1 * 32);
  auto dPrev = plan.in(prevMatched, (size_t)n1 * 2);
  auto dK2 = plan.in(kp2, n2);
  auto dD2 = plan.in(desc2, (size_t)n2 * 32);
  auto dCell = plan.add<int>(GRID_COLS * GRID_ROWS + 1);
  auto dSi = plan.add<uint16_t>(n2);
  auto dKeys = plan.add<unsigned long long>((size_t)n1 * width);
  auto dCnt = plan.add<int>(n1);
  auto dM12 = plan.add<int>(n1);
  auto dRaw = plan.addIf<int>(raw12 != nullptr, n1);
  auto dNm = plan.add<int>(1);
  pli_status st = commitScratch(c, plan);
  if (st != PLI_OK) return st;
  pli_fuse_camera cam = {};                                 // only the bounds are read (the 64 x 48 grid)
  cam.min_x = minX; cam.max_x = maxX; cam.min_y = minY; cam.max_y = maxY;
  const float radius = (float)windowSize;                   // const float& r of GetFeaturesInArea takes the int (:726)
  LAUNCH(c, "k_fuse_grid", k_fuse_grid, dim3(1), dim3(256), 0, dOff, dK2, cam, dCell, dSi);
  LAUNCH(c, "k_init_candidates", k_init_candidates, dim3((unsigned)std::min(1024, (n1 + 3) / 4)), dim3(256), 0, dK1, dD1, n1, dPrev, dK2, dD2,
         dCell, dSi, cam, radius, distLimit, width, dKeys, dCnt);
  LAUNCH(c, "k_init_assign", k_init_assign, dim3(1), dim3(64), (size_t)(48 + n2) * sizeof(int) + (size_t)n1 * sizeof(short), dK1, dD1, n1,
         dPrev, dK2, dD2, n2, dCell, dSi, cam, radius, distLimit, width, nnratio, checkOri ? 1 : 0, dKeys, dCnt, dM12, dRaw, dNm);
  HIPCHK(download(c, matches12, dM12));
  HIPCHK(download(c, raw12, dRaw));
  HIPCHK(download(c, nmatches, dNm));
  HIPCHK(hipStreamSynchronize(c->stream));
  return PLI_OK;
}

}  // extern "C"
