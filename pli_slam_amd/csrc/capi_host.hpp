// What the host translation units of libpli_frontend.so share (pli_capi.hip: context, ingest, ORB chain, stereo stages, entry points,
// measurement; line_chain.hip: the line chain, runLines and its stages; match_capi.hip: the stateless matcher entry points): the context,
// the error string, the launch and trace macros, the line chain's entry points and the scratch of one call.
// Host only.
#pragma once
#include "kernels.hpp"
#include "scratch_plan.hpp"
#include <cstdlib>
#include <string>
#include <vector>
#include <functional>
#include <mutex>
#include <atomic>
#include <dlfcn.h>

using namespace pli;

// Development switches (tools/README.md "Environment switches"): schedules and kernels that were measured and shelved, test switches,
// tuning knobs.  They are read ONLY by the development build of the library (make dev: -DPLI_DEV -> libpli_frontend_dev.so, which the dev-switch
// tests and the tools load); in the product library DEVENV is a null constant — the variable names are not even in the binary, and a
// stray variable in an integrator's environment cannot change a schedule.  The product reads four documented variables: PLI_ROCTX (roctx
// ranges), PLI_SYNC_DEBUG (synchronise after every launch), PLI_TX_TAIL (= 0: no persistent kernel, include/pli_frontend.h "Sharing a
// device") and PLI_LSD_MODE (overrides pli_frontend_config.lsd_mode).
#ifdef PLI_DEV
#define DEVENV(name) getenv(name)
#else
static inline const char* pli_no_devenv() { return nullptr; }
#define DEVENV(name) (pli_no_devenv())
#endif

// (one per library and not exported; defined in pli_capi.hip: pli_last_error reads it)
extern __attribute__((visibility("hidden"))) thread_local std::string g_err;

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e__);                            \
      return PLI_ERR_HIP;                                                                    \
    }                                                                                        \
  } while (0)

inline int64_t alignUp(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct ProfEntry { const char* name; hipEvent_t a, b; };

// the forms of the CV_64F front pass (lsd_f64.hip): k_lsd_blur64 -> k_lsd_resize64 -> k_lsd_grad64, k_lsd_front64, k_lsd_front64s
enum class LsdFront { Unfused, Tiled, Stream };

struct pli_ctx {
  // Every entry point that takes a context holds this lock for the whole call: the reference drives its four extractors
  // from four std::threads (Frame.cc:128-135) and the adapters put them on ONE context, so concurrent calls on a context
  // are legal and are serialised here (recursive: entry points call each other).  Different contexts run concurrently.
  mutable std::recursive_mutex mu;
  pli_frontend_config cfg;
  DevParams hp;
  DevParams* dP = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  bool ownStream = true;
  // side stream: for small batches the ORB chain runs beside the line chain (fork after the ingest, join before the stereo
  // stage); both chains are launch/latency bound there (+4 % on a single pair, +2.5 % at 32 frames, nothing from 256 frames on)
  hipStream_t aux = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr, evLbdPre = nullptr;
  hipStream_t aux2 = nullptr;        // round 1's region2rect pass beside round 2's pass over the owner map (line_chain.hip: tileRect)
  hipEvent_t evRectFork = nullptr, evRectDone = nullptr;
  std::function<pli_status()> sideChain;     // runChainsBeside (pli_capi.hip) -> relaxTile (line_chain.hip): enqueues the side stream's work
  bool lbdPreOnSide = false;                 // the LBD's blur + Sobel of this call ran on the side stream (runChainsBeside)
  bool syncDebug = getenv("PLI_SYNC_DEBUG") != nullptr;
  int NI = 0;
  pli_table_layout lay;
  std::vector<void*> allocs;
  // ORB
  uint8_t *pyr = nullptr, *blur = nullptr;
  int* resizeTab[MAX_LEVELS] = {nullptr};
  uint32_t* cellCand = nullptr; int* cellCount = nullptr;
  uint32_t* candAll = nullptr; unsigned short* nodeOf = nullptr; int* candCount = nullptr;
  uint32_t* kpSel = nullptr; int* kpSelCount = nullptr;
  BlurJob *jobOrb = nullptr, *jobLsd = nullptr, *jobLbd = nullptr;
  int orbTiles = 0, l0Tiles = 0;
  // LSD / LBD
  uint8_t *tmp8 = nullptr, *lsdScaled = nullptr;
  int64_t tmp8Stride = 0, lsdStride = 0;
  int tmpPitch = 0;
  int* lsdTab = nullptr;
  float4* rec = nullptr; int* g2 = nullptr; int* maxG2 = nullptr;
  // CV_64F pipeline of the LSD front (PLI_PARITY_LSD_F64, lsd_f64.hip)
  bool lsdF64 = false; double* mg = nullptr; unsigned long long* maxMg = nullptr; double* tmp64 = nullptr; double* kern64 = nullptr;
  int* lsdTab64 = nullptr; int lsdRadius = 0;
  LsdFront lsdFront = LsdFront::Unfused;     // the form of the front pass that applies to the geometry (a debug context runs Unfused)
  int2* hot = nullptr;                       // tile relaxation, CV_64F detector: round 1's 8-byte hot records {angle, owner word} (lsd_tile.hip)
  float2* cold = nullptr;                    // ... and the records' exact {cos, sin}: written instead of the 16-byte records when every round runs on the hot ones
  int2* own = nullptr; RxSeed* smallSeeds = nullptr; RxSeed* bigSeeds = nullptr; int bigCap = 0;
  RxHand* hand = nullptr; int handCap = 0; RxRect* rects = nullptr; int rectCap = 0; int* rankOf = nullptr; int2* rgBox = nullptr; float4* rgSeg = nullptr; uint8_t* rgClean = nullptr;
  int* rgLost = nullptr;                     // tile relaxation: round in which a region last lost a contested claim (per rank)
  // rgDirty and rgLost hold ROUND STAMPS, and a stamp is only ever compared with a round of the call that reads it.  So the planes are not
  // cleared per call: every call of the tile relaxation stamps with lineStampNext + t and leaves lineStampNext above everything it could
  // have written (planRelaxation, line_chain.hip).  Words of earlier calls, under whatever pixels, are below the base and match no round.  One counter per
  // context (the planes are indexed by image slot; calls are ordered by the context's lock and the stream).  Zeroed when allocated and
  // when the counter would pass INT_MAX.  Dev switch PLI_TX_STAMP0: where the counter starts.
  int lineStampNext = 0;
  int* tileTouch = nullptr;                  // tile relaxation: round in which a grower last claimed a pixel of the 8x8 cell
  int* tileMin = nullptr; int* tileAct = nullptr; int* rgDirty = nullptr; int tilesW = 0, tilesH = 0; int* rxChunkCnt = nullptr; int rxChunks = 0;
  int* lastSize = nullptr; int* arena = nullptr; int arenaCap = 0; int arenaFactor = 0;    // (arena words per scaled pixel the context got)
  RxCtl* jrCtl = nullptr;
  int2* txList = nullptr; int* txTileCnt = nullptr; int txTs = 64, txNtx = 0, txNty = 0;   // tile-sequential relaxation (lsd_tile.hip)
  bool txKeys = false; int txPixBits = 0; int* txCand = nullptr; int* txCandCnt = nullptr;  // ... its key mode (region id = gradient bin | seed pixel: no ordered list)
  int2* txDirtyList = nullptr; int* txDirtyCnt = nullptr;                                  // per tile: the seeds stamped dirty in a round
  std::vector<RxCtl> jrHost;
  int rxImages = 0;    // images the relaxations' buffers are sized for
  int lsdMode = 0;     // 0 auto, 1 relaxation, 2 sequential, 3 tile-sequential relaxation (cfg.lsd_mode, or PLI_LSD_MODE)
  bool lsdSpec = !(DEVENV("PLI_LSD_SPEC") != nullptr && atoi(DEVENV("PLI_LSD_SPEC")) == 0);  // speculative sequential grower (PLI_LSD_SPEC=0: the plain one)
  int rxLastRounds = 0; // rounds the relaxation needed in an earlier call (the last one whose control blocks the host has seen)
  // Rounds without a host look (the default once rxLastRounds is known): the call launches rxLastRounds + rxMargin rounds — kernels
  // of a settled image leave at once —, k_lsd_grow_unsettled redoes, on the device, whatever image did not settle in them, and the
  // control blocks come back asynchronously (rxSeen / evRxSeen) to be read at the start of a later call.  The call never drains the
  // stream, so copies and kernels of neighbouring calls overlap (pli_batch_submit_host, the multi-GPU gather).
  // the rounds t >= tail t0 of the tile relaxation run in one persistent launch (lsd_tile.hip: k_tx_tail)
  unsigned* tailBar = nullptr;      // [0] barrier arrivals, [32] abort word
  int* txPerm = nullptr;            // round 1: (image, tile) pairs in order of decreasing seed count (k_tx_order)
  int tailBlocks = 0;               // resident grid: CUs x blocks per CU (from the kernel's occupancy)
  int* txCellList = nullptr;        // rounds >= 3 of large batches: the cells with work, listed (k_tx_cells) ...
  int* txCellCnt = nullptr;         // ... and the lists' lengths, two per round (zeroed with the control blocks)
  bool tailLaunched = false;        // this call launched k_tx_tail ...
  bool rxSeenTail = false;          // ... and so did the call whose control blocks are on their way to the host (rxSeen)
  int rxMargin = 3;
  int rxPlanned = 0;                // rounds the last call launched without looking (0: it looked)
  int* rxSeen = nullptr;            // pinned: {state, changed, overflow, rounds} per image of the last look-free call
  hipEvent_t evRxSeen = nullptr;
  int rxSeenImages = 0;             // images behind rxSeen while the copy is in flight (0: nothing pending)
  int64_t rxSlowImages = 0;         // images that took the device-side fallback so far (pli_prof_report prints it)
  unsigned short* chunkHist = nullptr; int* chunkBase = nullptr; int* nDefined = nullptr;
  int* order = nullptr; uint2* regScratch = nullptr; float* seg = nullptr; int* nSeg = nullptr;
  LsdRectItem* rectItems = nullptr;          // sequential grower -> k_lsd_rect (maxSeg per image)
  double* rectW = nullptr;                   // CV_64F pipeline: the weights of the listed pixels, beside the lists
  double* scaled64Dbg = nullptr;             // debug copy of the CV_64F scaled image (its plane is reused as the growers' arena)
  int nChunks = 0, maxSeg = 0;
  int scanGroups = 0, scanChunksPerGroup = 0; int* scanGroupOff = nullptr;     // ordered-list scan of large images, in groups of chunks
  pli_keyline* tmpKL = nullptr;
  short2* dxy = nullptr;           // Sobel (dx, dy) of level 0, interleaved
  LbdCoef* lbdCoef = nullptr;
  // stereo
  int *sad = nullptr, *bestIdx = nullptr;
  unsigned long long* lmask = nullptr; double* ldir = nullptr; short* dmat = nullptr; int *m12 = nullptr, *m21 = nullptr;
  // drop-in state
  uint8_t* inStage[2] = {nullptr, nullptr};
  float2* rectMap[2] = {nullptr, nullptr};   // per eye: (mapx, mapy) of the driver's rectification, or null
  int imgFormat = PLI_IMAGE_GRAY8;           // pli_set_image_format: how every entry point reads its images ...
  int imgChannels = 1;                       // ... and the bytes per pixel of that format (inStage holds W * H of them per eye)
  DepthFormat depthFmt{0, 1.0f};             // pli_set_depth_format: the depth image of the two ComputeStereoFromRGBD kernels
  uint8_t* ownTable = nullptr;
  std::vector<uint8_t> hostRec;
  bool orbDone[2] = {false, false}, lineDone[2] = {false, false};
  bool frameFresh = false;                   // ownTable / hostRec hold the COMPLETE record of one Frame (pli_frame_extract): the stereo
                                             // matchers hand it out without running again; any per-call extraction ends that
  bool pointsFresh = false;                  // ... and its mvuRight / mvDepth were computed with the CURRENT rig (pli_set_stereo_camera
                                             // clears it: the point matcher then re-runs on the resident tables)
  uint8_t* recPinned = nullptr;              // pinned staging of that record
  size_t recPinnedBytes = 0;                 // ... where pli_frame_extract_single sized it: the record and the caller's columns behind it
  uint8_t* pyrHost[2] = {nullptr, nullptr};  // pinned copy of an eye's pyramid block (pli_orb_pyramid_level)
  bool pyrHostValid[2] = {false, false};     // ... is the one of the last extraction on that eye
  int orbCount[2] = {0, 0};                  // keypoints the last pli_orb_extract(_lapping) left in each eye's table
  int lineCount[2] = {0, 0};                 // keylines the last pli_line_extract left in each eye's table
  int monoCount[2] = {0, 0};                 // pli_orb_extract_lapping: first lapping-area keypoint of each eye's table
  PinholeUndist pinhole{};                   // pli_set_pinhole_distortion: the camera of the single-camera Frames and its image bounds
                                             // (no camera, or k1 == 0: on = 0 and the bounds {0, W, 0, H}; pli_ctx_create sets that)
  // pipelined host entry point: two slots of device staging (images + table), H2D and D2H copy streams
  struct HostSlot { uint8_t* dimg = nullptr; uint8_t* dtab = nullptr; size_t imgBytes = 0, tabBytes = 0;
                    hipEvent_t h2d = nullptr, kern = nullptr, d2h = nullptr; bool busy = false; };
  HostSlot hs[2];
  hipStream_t sH2D = nullptr, sD2H = nullptr;
  uint64_t hsSubmitted = 0, hsWaited = 0;
  // generic scratch for the stateless matchers
  void* scratch = nullptr; size_t scratchBytes = 0;
  // debug
  bool debug = false;
  float* angDbg = nullptr; float* lbdFloat = nullptr;
  // profiling
  bool prof = false;
  std::vector<ProfEntry> profLog;
  std::vector<hipEvent_t> evPool;
  size_t evNext = 0;

  template <class T> pli_status dalloc(T** p, size_t n) {
    void* q = nullptr;
    if (n == 0) n = 1;
    HIPCHK(hipMalloc(&q, n * sizeof(T)));
    allocs.push_back(q);
    *p = (T*)q;
    return PLI_OK;
  }
  hipEvent_t ev() {
    if (evNext == evPool.size()) {
      hipEvent_t e;
      hipEventCreate(&e);
      evPool.push_back(e);
    }
    return evPool[evNext++];
  }
  void profBegin(const char* name) {
    if (!prof) return;
    ProfEntry pe{name, ev(), ev()};
    hipEventRecord(pe.a, stream);
    profLog.push_back(pe);
  }
  void profEnd() {
    if (!prof) return;
    hipEventRecord(profLog.back().b, stream);
  }
};

// roctx ranges ("rocprofv3 counters + roctx ranges per kernel").  With PLI_ROCTX=1 in the environment every stage of a call
// (ingest, ORB chain, line chain, the two stereo matchers, the entry points themselves) and every kernel launch is bracketed by
// roctxRangePush / roctxRangePop, so that `rocprofv3 --kernel-trace --marker-trace` shows which call and stage a kernel belongs
// to.  The marker library is looked up at run time (rocprofiler-sdk's, then roctracer's): no link-time dependency, nothing is
// loaded and nothing is pushed without the switch.  pli_trace_ranges() counts the ranges pushed so far.
struct PliRoctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  std::atomic<long long> pushed{0};
  PliRoctx() {
    const char* e = getenv("PLI_ROCTX");
    if (!e || atoi(e) == 0) return;
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
      if (!h) continue;
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (push && pop) break;
      push = nullptr; pop = nullptr;
    }
  }
};
// (one per library and not exported; defined in pli_capi.hip: pli_trace_ranges returns its counter)
extern __attribute__((visibility("hidden"))) PliRoctx g_roctx;
struct TraceRange {
  bool on;
  explicit TraceRange(const char* name) : on(g_roctx.push != nullptr) {
    if (on) { g_roctx.push(name); g_roctx.pushed.fetch_add(1, std::memory_order_relaxed); }
  }
  ~TraceRange() { if (on) g_roctx.pop(); }
  TraceRange(const TraceRange&) = delete;
  TraceRange& operator=(const TraceRange&) = delete;
};

struct CtxGuard {
  const pli_ctx* c;
  explicit CtxGuard(const pli_ctx* c_) : c(c_) { if (c) c->mu.lock(); }
  ~CtxGuard() { if (c) c->mu.unlock(); }
  CtxGuard(const CtxGuard&) = delete;
  CtxGuard& operator=(const CtxGuard&) = delete;
};

// the launches of a scope go to another stream (LAUNCH takes c->stream): the context's own is back on every way out
struct StreamScope {
  pli_ctx* c;
  hipStream_t saved;
  StreamScope(pli_ctx* c_, hipStream_t s) : c(c_), saved(c_->stream) { c->stream = s; }
  ~StreamScope() { c->stream = saved; }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
};

#define LAUNCH(c, name, kern, grid, block, shmem, ...)                       \
  do {                                                                       \
    TraceRange tr__(name);                                                   \
    (c)->profBegin(name);                                                    \
    hipLaunchKernelGGL(kern, grid, block, shmem, (c)->stream, __VA_ARGS__);  \
    (c)->profEnd();                                                          \
    HIPCHK(hipGetLastError());                                               \
    if ((c)->syncDebug) {   /* PLI_SYNC_DEBUG: find the kernel that faults */ \
      std::fprintf(stderr, "[pli] %s ...", name);                            \
      HIPCHK(hipStreamSynchronize((c)->stream));                             \
      std::fprintf(stderr, " ok\n");                                         \
    }                                                                        \
  } while (0)

// ---- the line chain (line_chain.hip) and what pli_capi.hip sizes for it or calls of it ----
// lsd_mode auto: batches of at least this many images (2 per stereo frame) take the sequential wave grower (one wave
// per image: work-efficient, its throughput keeps growing with the batch); below it the tile-sequential relaxation
// (lsd_tile.hip: parallel inside an image, ~1.5x the sequential work per frame at large batches).  Measured, 752x480,
// stereo frames/s (end of round 3, tile vs sequential): 768 frames 5489 vs 3715, 1024 frames 5440 vs 4584, 1280 frames 5497 vs 5435,
// 1536 frames 5550 vs 5250, 1792 frames 5557 vs 5702, 2048 frames 5995 (sequential).  (Round 2: crossover at 1024 frames.)
// The hand-over is put at 1280 frames, where the two are level: the relaxations' buffers cost 25 MB per image, and a context of
// 1600 frames with them would take 250 of the 288 GB.
constexpr int RX_AUTO_IMAGES = 2560;     // images (2 per stereo frame): 1280 frames
constexpr int TX_CELL_ROUNDS = 100;   // rounds of a call that can run on cell lists (two list lengths per round and image, zeroed per call)
// scaled rows per wave of the streaming front: each chunk enters 6 source rows to warm its window up, and a strip's chunks are what
// fills the chip
constexpr int LSD_FRONT_CHUNK = 64;

// The arguments of launchFront64: one call of the CV_64F front pass (lsd_f64.hip) in a given form.
struct FrontSrc { const uint8_t* p; int64_t imgStride; int w, h, pitch; };       // u8 images
struct FrontGeom {
  const double* kern; int radius;       // the blur (lsdGauss64)
  const int* tab;                       // buildResizeTab64, or null: lsd_scale 1 (Unfused only: the u8 image as doubles is the scaled image)
  int dw, dh, dp;                       // scaled width and height, row pitch of the planes written
  int chunk;                            // Stream: scaled rows per wave
  double rho;
  int trigF32;                          // PLI_PARITY_TRIG_F32_LSD
};
struct FrontUnfused {                   // Unfused: the double planes between its kernels (images blurStride / scaledStride apart)
  double* blurred; int64_t blurStride;
  double* scaled; int64_t scaledStride;       // rows of the TRUE width dw
  float* angDbg;                        // or null: the debug plane of the angles
};
#pragma GCC visibility push(hidden)     // (shared by the library's translation units, not exported)
pli_status launchFront64(pli_ctx* c, LsdFront form, const FrontSrc& S, const FrontGeom& G, const LsdFrontPlanes& planes,
                         unsigned long long* maxMg, int img0, int n, const FrontUnfused& U = {});   // (the front-pass self-tests call it too)
pli_status runLines(pli_ctx* c, int img0, int nimg, uint8_t* table);
pli_status runLbdPre(pli_ctx* c, int img0, int nimg);
bool sequentialGrower(const pli_ctx* c, int nimg);
int foldRoundStats(pli_ctx* c);
#pragma GCC visibility pop

inline pli_status ensureScratch(pli_ctx* c, size_t bytes) {
  if (bytes <= c->scratchBytes) return PLI_OK;
  if (c->scratch) hipFree(c->scratch);
  c->scratch = nullptr; c->scratchBytes = 0;
  HIPCHK(hipMalloc(&c->scratch, bytes));
  c->scratchBytes = bytes;
  return PLI_OK;
}

// The scratch of one call (scratch_plan.hpp): the context's grow-only buffer takes the plan's total, the plan's blocks point into it,
// and the plan's inputs are copied from the host on the context's stream (their sources live until the call synchronises).
inline pli_status commitScratch(pli_ctx* c, ScratchPlan& plan) {
  const pli_status st = ensureScratch(c, plan.bytes());
  if (st != PLI_OK) return st;
  plan.bind(c->scratch);
  for (const ScratchCopy& k : plan.copies()) HIPCHK(hipMemcpyAsync(plan.base() + k.off, k.src, k.bytes, hipMemcpyHostToDevice, c->stream));
  return PLI_OK;
}

// elements first .. first + n of a scratch block to the host, on the context's stream (nothing for a null pointer or n == 0) ...
template <typename T>
hipError_t download(pli_ctx* c, T* dst, ScratchBlock<T> src, size_t first, size_t n) {
  return dst && n ? hipMemcpyAsync(dst, (T*)src + first, n * sizeof(T), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}
// ... and the whole block, as it was declared
template <typename T>
hipError_t download(pli_ctx* c, T* dst, ScratchBlock<T> src) { return download(c, dst, src, 0, src.n); }

// The tail of the matchers: waits for the stream and hands out the device's match counter.
inline pli_status fetchCount(pli_ctx* c, const int* dcount, int32_t* nmatches) {
  int cnt = 0;
  HIPCHK(hipMemcpyAsync(&cnt, dcount, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (nmatches) *nmatches = cnt;
  return PLI_OK;
}
