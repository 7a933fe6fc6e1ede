// The line chain of libpli_frontend.so, host side: LSD front pass, ordered list, one of three growers (the tile-sequential relaxation,
// the sequential wave grower, the development build's lane relaxation), segments, keylines and LBD — runLines, a sequence of stages on the
// context's stream, and what only this chain uses (the CV_64F front's launch path, the round plan's feedback, the persistent tail's
// process-wide state).  pli_capi.hip holds the context and the entry points that call it; what they share: capi_host.hpp.
#include "capi_host.hpp"
#include <algorithm>
#include <climits>
#include <set>

// the last k_tx_tail launch on every device of this process (see the launch site)
static std::mutex g_tailMu;
constexpr int TAIL_MAX_DEVICES = 64;
static hipEvent_t g_tailEv[TAIL_MAX_DEVICES] = {};
// ... and whether a tail of this process has ever been ABORTED on a device (its grid barrier timed out: somebody else — another
// process — holds compute units the resident grid needs).  From then on this process runs the planned-rounds schedule on that device
// instead of stalling a second per call (include/pli_frontend.h "Sharing a device").
static std::atomic<bool> g_tailAborted[TAIL_MAX_DEVICES] = {};       // (read without the mutex by every call: relaxed atomics)
static bool g_tailWarned = false;

// One call of the CV_64F front pass (lsd_f64.hip) in the given form on images img0 .. img0 + n - 1: the image's largest norm cleared,
// then the form's kernels.  The forms share their profile names (k_lsd_front: either fused form).
pli_status launchFront64(pli_ctx* c, LsdFront form, const FrontSrc& S, const FrontGeom& G, const LsdFrontPlanes& planes,
                         unsigned long long* maxMg, int img0, int n, const FrontUnfused& U) {
  HIPCHK(hipMemsetAsync(maxMg + img0, 0, sizeof(unsigned long long) * n, c->stream));
  if (form == LsdFront::Stream) {
    // one wave per strip of 64 scaled columns and chunk of rows, no tile and no barrier
    const int strips = (G.dw + 63) / 64;
    LAUNCH(c, "k_lsd_front", k_lsd_front64s, dim3((strips + LSD_FRONT_STREAM_WAVES - 1) / LSD_FRONT_STREAM_WAVES, (G.dh + G.chunk - 1) / G.chunk, n),
           dim3(64 * LSD_FRONT_STREAM_WAVES), 0, S.p, S.imgStride, S.w, S.h, S.pitch, G.kern, G.tab, G.dw, G.dh, G.dp, G.rho, planes, maxMg,
           img0, G.trigF32, G.chunk);
  } else if (form == LsdFront::Tiled) {
    // blur -> resize -> gradient in one pass over LDS tiles: neither double plane goes to HBM
    LAUNCH(c, "k_lsd_front", k_lsd_front64, dim3((G.dp + 63) / 64, (G.dh + 15) / 16, n), dim3(256), 0, S.p, S.imgStride, S.w, S.h, S.pitch,
           G.kern, G.radius, G.tab, G.dw, G.dh, G.dp, G.rho, planes, maxMg, img0, G.trigF32);
  } else {
    // (lsd_scale 1: radius 0 and the kernel {1} — the blur writes the scaled plane itself)
    LAUNCH(c, "k_blur_lsd", k_lsd_blur64, dim3((S.w + 63) / 64, (S.h + 15) / 16, n), dim3(256), 0, S.p, S.imgStride, S.w, S.h, S.pitch, G.kern,
           G.radius, G.tab ? U.blurred : U.scaled, G.tab ? U.blurStride : U.scaledStride, img0);
    if (G.tab)
      LAUNCH(c, "k_resize_lsd", k_lsd_resize64, dim3((G.dw + 255) / 256, G.dh, n), dim3(256), 0, U.blurred, S.w, S.h, U.scaled, G.dw, G.dh,
             U.scaledStride, G.tab, img0);
    LAUNCH(c, "k_lsd_grad", k_lsd_grad64, dim3((G.dp + 255) / 256, (G.dh + 15) / 16, n), dim3(256), 0, U.scaled, G.dw, G.dh, G.dp, U.scaledStride,
           G.rho, planes, maxMg, U.angDbg, img0, G.trigF32);
  }
  return PLI_OK;
}

// Folds the control blocks a look-free call sent back (rxSeen) into the plan of the next call.  Returns the rounds the slowest
// settled image needed, or -1 when an image took the device-side fallback.
int foldRoundStats(pli_ctx* c) {
  int settled = 0, unsettled = 0, overflowed = 0;
  for (int i = 0; i < c->rxSeenImages; ++i) {
    const int* h = c->rxSeen + 4 * i;
    if (h[2]) ++overflowed;                            // a capacity ran out (adversarial images): more rounds would not help
    else if (h[0] != 2) ++unsettled;
    else settled = std::max(settled, h[3]);
  }
  c->rxSlowImages += unsettled + overflowed;
  // An image that has not settled although the self-terminating tail kernel ran (it walks up to 96 rounds): the tail was aborted —
  // its grid barrier timed out because the resident grid did not fit beside somebody else's work (another PROCESS on the device).
  // This process runs the planned-rounds schedule on that device from now on instead of stalling ~1 s in every call.
  // (the abort word of the tail's grid barrier came back with the control blocks: an image that merely needed more than the 96 rounds the
  // tail walks — or a small PLI_RX_MAXROUNDS — is not an aborted tail and does not switch the process's schedule)
  const bool aborted = c->rxSeen[4 * (size_t)c->NI] != 0;
  if (unsettled && c->rxSeenTail && aborted && c->device >= 0 && c->device < TAIL_MAX_DEVICES) {
    std::lock_guard<std::mutex> lk(g_tailMu);
    g_tailAborted[c->device].store(true, std::memory_order_relaxed);
    if (!g_tailWarned) {
      g_tailWarned = true;
      std::fprintf(stderr, "pli_frontend: the persistent relaxation kernel did not finish on device %d (another process on the device?); "
                           "this process uses the planned-rounds schedule there from now on (as with PLI_TX_TAIL=0)\n", c->device);
    }
  }
  if (unsettled) c->rxLastRounds = std::min(96, c->rxLastRounds + c->rxMargin);        // not enough rounds: plan more next time
  else if (settled > 0) c->rxLastRounds = std::max(settled, c->rxLastRounds - 1);       // (follows a calmer stream down slowly)
  c->rxSeenImages = 0;
  return (unsettled || overflowed) ? -1 : settled;
}

// BinaryDescriptor::compute's image work (binary_descriptor_custom.cpp:350-398): GaussianBlur 5x5 + Sobel of level 0.  It
// needs the image only, not the lines: pli_batch_run puts it on the side stream (after the ORB chain) when the LSD front does
// not use the u8 scratch plane itself (CV_64F detector).
pli_status runLbdPre(pli_ctx* c, int img0, int nimg) {
  TraceRange range__("pli:lbd blur+sobel");
  const DevParams& P = c->hp;
  LAUNCH(c, "k_sobel", k_sobel, dim3(c->l0Tiles, nimg), dim3(256), 0, c->jobLbd, c->pyr, P.pyrBlock, c->dxy, img0);
  return PLI_OK;
}

// this call takes the sequential grower: asked for, or auto mode with a batch the relaxations' buffers are not meant (or not sized) for
bool sequentialGrower(const pli_ctx* c, int nimg) {
  return c->lsdMode == 2 || (c->lsdMode == 0 && (nimg >= RX_AUTO_IMAGES || nimg > c->rxImages));
}

namespace {

// What one call of the line chain runs, resolved once at its head (resolveLineCall) and read-only from then on: the schedule, the
// tile relaxation's dev switches that later stages ask about, the rules they add up to, and the planes the kernels take.
struct LineCall {
  int img0, nimg, npix;
  bool sequential, tile;
  bool cellRule, fullRound2, oldMark, fullDiff, noDirtyList, specEnv, orderEnv, xcdEnv;
  bool lostRule, fuseRound2, fusedDM, keyMode;
  int packMode, hotLevel;
  int2 *ownPlane, *hotPlane, *hotLater;
  float4* recPlane;
  float2* coldPlane;
  int trigF32;
};

// The plan of a relaxation's rounds (planRelaxation), and what the rounds change in it: the round they are in, whether a host look
// found every image settled.
struct RelaxPlan {
  bool trace, perRound;           // PLI_RX_TRACE; PLI_RX_PROFROUNDS: profile names carry the round number
  int rectBlocks, maxRounds;
  bool tailPossible, blocking;
  int stampBase, firstLook;
  int curT;
  bool allDone;
};

// what relaxTile sets up once for its rounds: the argument records, the fork point, which passes run aside or on lists
struct TileRounds {
  TxKeys keys;
  TxRound txr, first;             // (the dirty lists: txr.DL)
  TxDirtyLists noDL;
  int ntile;
  bool pack1;
  int sideForkRound;
  bool rectOnSide, rectAside, useCells;
  int tailT0;
  bool tailForceAbort;
};

// a profile name, with the round under PLI_RX_PROFROUNDS.  The names live as long as the process: profLog holds them after the call.
// (one pool for every context, and different contexts run concurrently: a lock of its own)
const char* rxn(const RelaxPlan& R, const char* n) {
  if (!R.perRound) return n;
  static std::mutex mu;
  static std::set<std::string> pool;
  char b[64];
  std::snprintf(b, sizeof(b), "%s@%02d", n, R.curT);
  std::lock_guard<std::mutex> lk(mu);
  return pool.insert(b).first->c_str();
}

// LAUNCH plus, under PLI_RX_TRACE, a sync and a line on stderr (finds a kernel that does not return); R: the call's RelaxPlan
#define TRL(c, name, ...)                                                      \
  do {                                                                         \
    LAUNCH(c, rxn(R, name), __VA_ARGS__);                                      \
    if (R.trace) {                                                             \
      HIPCHK(hipStreamSynchronize((c)->stream));                               \
      std::fprintf(stderr, "[rx] %s done\n", name);                           \
    }                                                                          \
  } while (0)

LineCall resolveLineCall(const pli_ctx* c, int img0, int nimg) {
  const DevParams& P = c->hp;
  LineCall L{};
  L.img0 = img0; L.nimg = nimg;
  L.npix = P.LW * P.LH;
  L.sequential = sequentialGrower(c, nimg);
  // (the owner plane's start value: the lane relaxation takes it from the front pass; the tile relaxation's k_tx_sort writes the
  // trivial map for every pixel itself — 8 bytes per scaled pixel less for the front pass to store)
  L.ownPlane = (L.sequential || c->lsdMode != 1) ? (int2*)nullptr : c->own;
  L.tile = !L.sequential && c->lsdMode != 1;      // auto below RX_AUTO_IMAGES and mode 3: the tile-sequential relaxation
  // The tile relaxation's dev switches that choose kernels, each read here once per call (the front pass already needs keyMode, packMode
  // and hotLevel; tests change the environment between contexts of one process, so nothing is kept across calls).
  auto devOn = [](const char* e) { return e && atoi(e) != 0; };
  const bool boxRule = DEVENV("PLI_TX_BOXRULE") != nullptr;         // the conservative round-2 rule
  L.cellRule = DEVENV("PLI_TX_CELLRULE") != nullptr;                // ... of rounds >= 3
  L.fullRound2 = DEVENV("PLI_TX_FULL2") != nullptr;                 // regrow everything in round 2
  L.oldMark = DEVENV("PLI_TX_OLDMARK") != nullptr;                  // k_rx_mark instead of k_tx_mark
  L.fullDiff = DEVENV("PLI_TX_FULLDIFF") != nullptr;                // k_rx_diff over every cell, not the touched ones
  const bool noFuse2 = DEVENV("PLI_TX_NOFUSE2") != nullptr;         // round 2's diff and prep as two passes
  const bool noFuseDM = DEVENV("PLI_TX_NOFUSEDM") != nullptr;       // rounds >= 3: diff and mark as two passes
  L.noDirtyList = DEVENV("PLI_TX_NODIRTYLIST") != nullptr;          // every active tile walks its whole seed list
  L.specEnv = devOn(DEVENV("PLI_TX_SPEC")); L.orderEnv = devOn(DEVENV("PLI_TX_ORDER")); L.xcdEnv = devOn(DEVENV("PLI_TX_XCD"));
  // ... and the rules they add up to, each named once
  L.lostRule = c->lsdMode != 1 && !boxRule;                         // round 2 regrows the regions that lost a contested pixel
  L.fuseRound2 = L.lostRule && !L.fullRound2 && !noFuse2;           // round 2's pass over the owner map is k_tx_round2
  // rounds >= 3: k_rx_diff + k_tx_mark as one kernel (k_tx_diffmark; the dev rules keep the separate passes)
  L.fusedDM = L.lostRule && !L.fullRound2 && !L.cellRule && !L.oldMark && !L.fullDiff && !noFuseDM;
  // key mode of the tile relaxation (lsd_tile.hip): no ordered list — it is only built, at the end, for images left to the sequential grower
  L.keyMode = L.tile && c->txKeys && !c->debug && L.lostRule && !L.fullRound2 && !L.oldMark && !L.cellRule;   // (k_rx_mark, lsd_relax.hip, indexes the region planes by rank)
  // packed round 1 (lsd_tile.hip, tx_load_rec16): owner_1 lives in the fourth word of the pixel records during round 1 — one
  // 16-byte gather per neighbour instead of two.  Needs the CV_64F detector (the word is free: the gradient norms have their own
  // plane) and the default schedule (k_tx_round2 moves the result into the owner plane).  In key mode the front pass writes the
  // unclaimed words itself (2: LAZY ids), otherwise k_tx_sort does (1).  Dev switch PLI_TX_PACK1=0 / 1.
  int packMode = 0;
  if (L.tile && c->lsdF64 && c->mg && !c->debug && L.fuseRound2 && !L.specEnv && !L.orderEnv)
    packMode = (L.keyMode && P.nBins > 128) ? 2 : 1;      // (the lazy form's fixed-point bin width needs maxGrad / (nBins - 1) < 4: tests/test_lazy_ids_cpu.py)
  const int packCap = packMode;                           // (what this call could do: the choice follows the hot-record level below)
  // round 6: round 1's words in 8-byte hot records of their own (lsd_tile.hip "HOT RECORDS"); dev switch PLI_TX_HOT=0 / 1
  // 2 (the default): every round — the later rounds take the angle from the hot record and the owner pair from the owner plane, nobody
  // reads the 16-byte records, and the front pass does not write them (the device-side fallback of an unsettled image rebuilds them
  // from the hot records first: k_tx_rec_from_hot); 1: round 1 only; 0: the 16-byte records everywhere (round 5's form)
  int hotLevel = (packMode != 0 && c->hot != nullptr && P.prec <= 1.0 && P.alignFilter != 0) ? 2 : 0;
  if (const char* e = DEVENV("PLI_TX_HOT")) hotLevel = std::min(hotLevel, std::max(0, atoi(e)));
  if (hotLevel == 2 && L.noDirtyList) hotLevel = 1;     // (a dev schedule that keeps to the plain later-round kernels)
  // On the hot records the ids are SORT-WRITTEN (1) by default, in key mode too: k_tx_sort stores `unclaimed | id` into the second word
  // of every 8-byte record — 4-byte stores, read-modify-writes of sectors — and round 1 does without the lazy-id test, ~23 of a step's
  // ~150 vector instructions: k_tx_grow 18.6 -> 17.1 ms, k_tx_sort 2.1 -> 3.2.  (Rewriting the whole record, the angle with it, was
  // measured and is slower: k_tx_sort 3.8 ms — the extra loads cost more than the partial sectors, lsd_tile.hip k_tx_sort; DESIGN.md 5
  // "Round 6".)  On the 16-byte records the same trade was a wash (round 5) and lazy ids stay the default there.  Dev switch
  // PLI_TX_PACK1 = 0 / 1 / 2.
  if (hotLevel != 0 && packMode == 2) packMode = 1;
  if (const char* e = DEVENV("PLI_TX_PACK1")) packMode = std::min(packCap, std::max(0, atoi(e)));
  if (packMode == 0) hotLevel = 0;
  L.packMode = packMode; L.hotLevel = hotLevel;
  const bool hotMode = hotLevel != 0, hotAll = hotLevel == 2;
  L.hotPlane = hotMode ? c->hot : (int2*)nullptr;
  L.hotLater = hotAll ? c->hot : (int2*)nullptr;
  L.recPlane = hotAll ? (float4*)nullptr : c->rec;         // (what the front pass writes: the 16-byte records, or the cold plane)
  L.coldPlane = hotAll ? c->cold : (float2*)nullptr;
  L.trigF32 = (c->cfg.parity_flags & PLI_PARITY_TRIG_F32_LSD) ? 1 : 0;
  return L;
}

// the front pass: the pixel records (or the hot and cold planes), the gradient norms and each image's largest
pli_status lineFront(pli_ctx* c, const LineCall& L) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg, npix = L.npix;
  if (c->lsdF64) {
    // OpenCV 3.x: the detector works on the CV_64FC1 copy of the image (lsd_f64.hip).  The three kernels' scaled double image lives
    // in the grower's overflow area (same size, not in use before the growers run): rows of the TRUE width, images npix = pitch x
    // height apart.  A debug context runs them: PLI_DBG_LSD_SCALED wants the plane.
    double* scaled64 = reinterpret_cast<double*>(c->regScratch);
    const pli_status st = launchFront64(
        c, c->debug ? LsdFront::Unfused : c->lsdFront, FrontSrc{c->pyr + P.lv[0].offset, P.pyrBlock, P.W, P.H, P.lv[0].pitch},
        FrontGeom{c->kern64, c->lsdRadius, c->lsdTab64, P.LWt, P.LH, P.LW, LSD_FRONT_CHUNK, P.rho, L.trigF32},
        LsdFrontPlanes{L.recPlane, c->mg, L.ownPlane, L.hotPlane, L.coldPlane, L.packMode == 2}, c->maxMg, img0, nimg,
        FrontUnfused{c->tmp64, (int64_t)P.W * P.H, scaled64, (int64_t)npix, c->debug ? c->angDbg : (float*)nullptr});
    if (st != PLI_OK) return st;
    if (c->debug && c->scaled64Dbg)                    // the plane becomes the growers' arena: keep a copy for PLI_DBG_LSD_SCALED
      HIPCHK(hipMemcpyAsync(c->scaled64Dbg + (int64_t)img0 * npix, scaled64 + (int64_t)img0 * npix, (size_t)nimg * npix * 8,
                            hipMemcpyDeviceToDevice, c->stream));
  } else {
    const uint8_t* scaled;
    int64_t sStride;
    int sPitch;
    if (c->cfg.lsd_scale != 1) {
      LAUNCH(c, "k_blur_lsd", k_blur, dim3(c->l0Tiles, nimg), dim3(256), 0, c->jobLsd, c->pyr, P.pyrBlock, c->tmp8, c->tmp8Stride, img0);
      dim3 g((P.LWt + 255) / 256, (P.LH + 15) / 16, nimg);
      LAUNCH(c, "k_resize_lsd", k_resize_level, g, dim3(256), 0, c->tmp8, c->tmp8Stride, P.W, P.H, c->tmpPitch, c->lsdScaled,
             c->lsdStride, P.LWt, P.LH, P.lpitch, c->lsdTab, img0);
      scaled = c->lsdScaled; sStride = c->lsdStride; sPitch = P.lpitch;
    } else {
      scaled = c->pyr + P.lv[0].offset; sStride = P.pyrBlock; sPitch = P.lv[0].pitch;
    }
    HIPCHK(hipMemsetAsync(c->maxG2 + img0, 0, sizeof(int) * nimg, c->stream));
    dim3 g((P.LW + 255) / 256, (P.LH + 15) / 16, nimg);   // 16 = LSD_GRAD_ROWS
    LAUNCH(c, "k_lsd_grad", k_lsd_grad, g, dim3(256), 0, scaled, sStride, P.LWt, P.LH, P.LW, sPitch, P.g2Thresh, c->rec, c->g2, L.ownPlane,
           c->maxG2, c->debug ? c->angDbg : (float*)nullptr, img0, L.trigF32);
  }
  return PLI_OK;
}

// the ordered list (pixels by gradient bin): of every image, or of the images that `only` leaves to the sequential grower
pli_status lineOrder(pli_ctx* c, const LineCall& L, const RxCtl* only) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg, npix = L.npix;
  LAUNCH(c, "k_lsd_hist", k_lsd_hist, dim3(c->nChunks, nimg), dim3(256), 0, c->g2, npix, P.g2Thresh, P.nBins, c->maxG2,
         c->chunkHist, c->nChunks, img0, c->mg, c->maxMg, P.rho, only);
  // (thousands of chunks per image — 4K —: the scan over the chunks in groups, lsd_scanGroups > 0)
  if (c->scanGroups > 0) {
    LAUNCH(c, "k_lsd_scan", k_lsd_scan_part, dim3(nimg, c->scanGroups), dim3(1024), 0, c->chunkHist, c->nChunks, P.nBins,
           c->scanChunksPerGroup, c->chunkBase, c->scanGroupOff, img0, only);
    LAUNCH(c, "k_lsd_scan", k_lsd_scan_groups, dim3(nimg), dim3(1024), 0, c->scanGroups, P.nBins, c->scanGroupOff, c->nDefined, img0, only);
  } else
    LAUNCH(c, "k_lsd_scan", k_lsd_scan, dim3(nimg), dim3(1024), 0, c->chunkHist, c->nChunks, P.nBins, c->chunkBase, c->nDefined, img0, only);
  // 16 KB of unused dynamic LDS per single-wave workgroup caps the scatter at 8 waves per CU: with all chunks of an image on
  // one XCD (see the kernel) that keeps the ordered lists "open" in an XCD's 4 MB L2 to ~2 images, so the 4-byte stores of
  // different chunks merge into whole lines before they are evicted (2048 frames: 21.8 -> 15.3 ms; 32 KB starves the CUs)
  constexpr size_t scatterOccupancyPad = 16384;
  LAUNCH(c, "k_lsd_scatter", k_lsd_scatter, dim3((unsigned)(8 * ((nimg + 7) / 8) * c->nChunks)), dim3(64), scatterOccupancyPad, c->g2, npix, P.g2Thresh,
         P.nBins, c->maxG2, c->chunkBase, c->nChunks, c->order, img0, nimg, c->mg, c->maxMg, P.rho,
         (L.sequential || only) ? (int*)nullptr : c->rankOf, (const int*)(c->scanGroups > 0 ? c->scanGroupOff : nullptr), c->scanChunksPerGroup,
         c->scanGroups, only);
  return PLI_OK;
}

// the sequential wave grower: one wave (or two) per image, segments straight from the grower
pli_status lineGrowSequential(pli_ctx* c, const LineCall& L) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg;
  // speculative form (line_kernels.hip: lsd_grow_image_spec): the small regions of 64 seeds at a time, one per lane
  const bool spec = c->lsdSpec && P.minRegSize >= 2;
  const bool two = nimg >= 64;
  // region2rect off the grower's serial chain: the spec grower leaves the pixel lists in the arena, k_lsd_rect does the segments
  LsdRectItem* items = (spec && DEVENV("PLI_LSD_RECT_OFFLOAD")) ? c->rectItems : (LsdRectItem*)nullptr;      // dev switch: measured, not a gain
  if (two && spec)
    LAUNCH(c, "k_lsd_grow2", k_lsd_grow2_spec, dim3((nimg + 1) / 2), dim3(128), 0, c->dP, c->rec, c->mg, c->order, c->nDefined,
           c->regScratch, c->seg, c->nSeg, c->maxSeg, img0, nimg, items, c->rectW);
  else if (two)
    LAUNCH(c, "k_lsd_grow2", k_lsd_grow2, dim3((nimg + 1) / 2), dim3(128), 0, c->dP, c->rec, c->mg, c->order, c->nDefined,
           c->regScratch, c->seg, c->nSeg, c->maxSeg, img0, nimg);
  else if (spec)
    LAUNCH(c, "k_lsd_grow", k_lsd_grow_spec, dim3(nimg), dim3(64), 0, c->dP, c->rec, c->mg, c->order, c->nDefined,
           c->regScratch, c->seg, c->nSeg, c->maxSeg, img0, nimg, items, c->rectW);
  else
    LAUNCH(c, "k_lsd_grow", k_lsd_grow, dim3(nimg), dim3(64), 0, c->dP, c->rec, c->mg, c->order, c->nDefined,
           c->regScratch, c->seg, c->nSeg, c->maxSeg, img0, nimg);
#ifdef PLI_DEV
  if (items)
    LAUNCH(c, "k_lsd_rect", k_lsd_rect, dim3(16, nimg), dim3(64), 0, c->dP, (const LsdRectItem*)items, (const uint2*)c->regScratch,
           (const double*)c->mg, (const double*)c->rectW, (const int*)c->nSeg, c->seg, c->maxSeg, img0);     // 16 = RECT_WPI
#endif
  return PLI_OK;
}

// Plans the rounds of a relaxation (incremental rank-ordered relaxation, lsd_relax.hip: rounds until every image's owner map is a
// fixed point) and zeroes the call's state: how many rounds at most, whether the host looks at them, whether the persistent tail can
// take the late ones, the call's stamp base.
pli_status planRelaxation(pli_ctx* c, const LineCall& L, RelaxPlan& R) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg, npix = L.npix;
  const bool trace = R.trace = DEVENV("PLI_RX_TRACE") != nullptr;
  const bool perRound = R.perRound = DEVENV("PLI_RX_PROFROUNDS") != nullptr;    // profile names carry the round number
  const char* const maxRoundsEnv = DEVENV("PLI_RX_MAXROUNDS");
  const char* const planEnv = DEVENV("PLI_RX_PLAN");               // dev / test: a fixed number of look-free rounds (too few: the device-side fallback)
  const char* const tailEnv = getenv("PLI_TX_TAIL");               // = 0: no persistent kernel (include/pli_frontend.h "Sharing a device")
  R.curT = 0;
  const int64_t npix64 = (int64_t)npix;
  R.rectBlocks = std::max(64, std::min(2048, 32768 / nimg));      // waves per image of k_rx_rect
  int maxRounds = maxRoundsEnv ? std::max(1, std::min(1 << 20, atoi(maxRoundsEnv))) : 96;
  if (c->rgClean) HIPCHK(hipMemsetAsync(c->rgClean + (int64_t)img0 * npix, 0, npix64 * nimg, c->stream));   // round stamps
  {
    // everything the relaxation wants zeroed at the start of a call, in one launch (k_zero_ranges): control blocks, the cell tables,
    // the tile relaxation's per-tile dirty counters (cleared by their consumers from then on), the barrier words of k_tx_tail and the
    // candidate counters of k_tx_collect.  NOT the two per-pixel stamp planes (rgDirty, rgLost) of the tile relaxation, whatever its
    // dev switches: their stamps sit above a base that moves with every call (pli_ctx::lineStampNext), nobody clears them per call.
    const int64_t cells = (int64_t)c->tilesW * c->tilesH;
    const int64_t ntile64 = (int64_t)c->txNtx * c->txNty;
    static_assert(sizeof(RxCtl) % 4 == 0, "RxCtl is cleared as words");
    ZeroRanges Z{};
    int zr = 0;
    constexpr int zmax = (int)(sizeof(Z.p) / sizeof(Z.p[0]));
    bool zfull = false;
    auto add = [&](void* p, int64_t words) {
      if (!p || words <= 0) return;
      if (zr == zmax) { zfull = true; return; }
      Z.p[zr] = (uint32_t*)p; Z.words[zr] = words; ++zr;
    };
    add(c->jrCtl + img0, (int64_t)(sizeof(RxCtl) / 4) * nimg);
    // (the lane relaxation — development build, lsd_mode 1 — keeps its fill and stamps with the plain round: k_rx_seed_sparse and the byte
    // plane rgClean beside it compare with t, the schedule is a cross-check and not a speed item, and a context has one mode for life,
    // so its planes never meet the other schedules' stamps)
    if (c->lsdMode == 1) add(c->rgDirty + (int64_t)img0 * npix, npix64 * nimg);
    add(c->tileTouch + (int64_t)img0 * cells, cells * nimg);
    add(c->tileAct + (int64_t)img0 * cells, cells * nimg);
    if (c->txDirtyCnt) add(c->txDirtyCnt + (int64_t)img0 * ntile64, ntile64 * nimg);
    if (c->tailBar) add(c->tailBar, 64);
    if (c->txCellCnt) add(c->txCellCnt, (int64_t)2 * TX_CELL_ROUNDS * c->rxImages);
    if (c->txCandCnt) add(c->txCandCnt + img0, nimg);
    if (zfull) { g_err = "k_zero_ranges: more buffers than ZeroRanges holds"; return PLI_ERR_INVALID; }
    const int zb = (int)std::max<int64_t>(1, std::min<int64_t>(8192, (npix64 * nimg / 4 + 255) / 256));
    LAUNCH(c, "k_zero_ranges", k_zero_ranges, dim3(zb, zr), dim3(256), 0, Z);
  }
  // (the rank plane was written by k_lsd_scatter)
  R.allDone = false;
  // what the last look-free call left behind (if its copy has arrived): how many rounds its slowest image needed
  if (c->rxSeenImages > 0 && hipEventQuery(c->evRxSeen) == hipSuccess) foldRoundStats(c);
  if (L.tile && c->tailBar && c->tailBlocks == 0) {       // the resident grid of k_tx_tail: one block per CU (-1: it does not fit)
    int perCu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_tx_tail, 256, 0));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->tailBlocks = perCu < 1 ? -1 : std::max(1, cus);
  }
  c->tailLaunched = false;
  const bool tailLatched = c->device < 0 || c->device >= TAIL_MAX_DEVICES || g_tailAborted[c->device].load(std::memory_order_relaxed);   // (no chain slot for the device: no tail)
  // (the tail is k_tx_diffmark's rounds on the dirty lists: fusedDM, and the lists, which a tile context allocates with the barrier words)
  const bool tailPossible = R.tailPossible = L.tile && c->tailBar && c->tailBlocks > 0 && !tailLatched && !planEnv && !trace && !perRound &&
                                             !(tailEnv && atoi(tailEnv) == 0) && L.fusedDM && !L.noDirtyList;
  const bool blocking = R.blocking = !tailPossible && (c->rxLastRounds == 0 || trace);
  if (!blocking && !tailPossible) maxRounds = std::min(maxRounds, c->rxLastRounds + c->rxMargin);
  if (!blocking && planEnv) maxRounds = std::max(1, std::min(1 << 20, atoi(planEnv)));   // (a plan that is too short: test_look_free_rounds_and_device_side_fallback)
  c->rxPlanned = blocking ? 0 : (tailPossible ? -1 : maxRounds);
  R.maxRounds = maxRounds;
  // The call's stamp base (pli_ctx::lineStampNext).  No round of this call is above maxRounds — the host loop below and k_tx_tail, which
  // counts its own rounds, both end there — so the next call starts maxRounds + 1 higher.  Before the counter would pass INT_MAX (once in
  // some 10^7 calls) both planes are zeroed whole, in stream order behind every earlier call, and the counter starts again.
  // (That order holds because every kernel that reads or writes the two planes runs on c->stream.  Round 1's region2rect pass, the one
  // kernel of the line chain on another stream — aux / aux2 —, touches neither; a kernel that did would need an event before this fill.)
  R.stampBase = 0;
  if (L.tile) {
    if ((int64_t)c->lineStampNext + maxRounds + 1 > (int64_t)INT_MAX) {
      HIPCHK(hipMemsetAsync(c->rgDirty, 0, sizeof(int) * (size_t)npix * c->rxImages, c->stream));
      HIPCHK(hipMemsetAsync(c->rgLost, 0, sizeof(int) * (size_t)npix * c->rxImages, c->stream));
      c->lineStampNext = 0;
    }
    R.stampBase = c->lineStampNext;
    c->lineStampNext += maxRounds + 1;
  }
  R.firstLook = c->rxLastRounds > 0 ? std::max(4, c->rxLastRounds) : 4;
  return PLI_OK;
}

// the end of round t of a relaxation that looks (RelaxPlan::blocking): whether every image has settled
pli_status look(pli_ctx* c, const LineCall& L, RelaxPlan& R, int t) {
  // the host looks at the state every second round, starting where the previous call on this context ended (a
  // stream of similar frames settles after a similar number of rounds; each look drains the stream)
  if (!R.blocking) return PLI_OK;
  if ((t >= R.firstLook && ((t - R.firstLook) % 2) == 0) || t == R.maxRounds) {
    HIPCHK(hipMemcpyAsync(c->jrHost.data(), c->jrCtl + L.img0, sizeof(RxCtl) * L.nimg, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    R.allDone = true;
    int settled = 0;
    for (int i = 0; i < L.nimg; ++i) {
      R.allDone = R.allDone && (c->jrHost[i].state == 2 || c->jrHost[i].overflow);
      settled = std::max(settled, c->jrHost[i].rounds);
    }
    if (R.allDone) c->rxLastRounds = settled;       // the round in which the last image reached its fixed point
  }
  return PLI_OK;
}

// The schedules of the development build that the stages below hand over to, in one place: the product's path through a round does not
// have to be read around them.  The product library has none of their kernels, and the switches that lead here read as unset (DEVENV).
#ifdef PLI_DEV
// the pass over the owner map of round t >= 2 as separate passes — what the dev switches leave of k_tx_round2 (round 2) and of
// k_tx_diffmark or the cell lists (rounds >= 3) — and k_tx_prep behind them
pli_status tileOwnerPassDev(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S, int t) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg;
  const TxRound& txr = S.txr;
  const bool lostRule = L.lostRule, fullRound2 = L.fullRound2, cellRule = L.cellRule, oldMark = L.oldMark;
  if (t < 2) return PLI_OK;               // (round 1 starts from the trivial map: nothing to compare, the control block is zeroed)
  // (the per-tile dirty counters: cleared once per call with the control blocks, then by the wave that takes a tile's list;
  // the dev schedule that regrows everything in round 2 does not read the lists it stamped)
  if (t == 3 && txr.DL.list && fullRound2)
    HIPCHK(hipMemsetAsync(c->txDirtyCnt + (int64_t)img0 * S.ntile, 0, sizeof(int) * (size_t)S.ntile * nimg, c->stream));
  // (the unfused passes of the dev switches: the product's round 2 is k_tx_round2, its rounds >= 3 k_tx_diffmark or the cell lists)
  if (t == 2 && !fullRound2)
    TRL(c, "k_tx_diff2", k_tx_diff2, dim3((P.LW + 31) / 32, c->tilesH, nimg), dim3(256), 0, txr, t, c->tileMin);
  else
    TRL(c, "k_rx_diff", k_rx_diff, dim3((P.LW + 31) / 32, (c->tilesH + 7) / 8, nimg), dim3(256), 0, c->jrCtl, c->own, c->tileMin, c->tileAct,
        P.LW, P.LH, c->tilesW, c->tilesH, t, img0,
        (t >= 3 && !fullRound2 && !L.fullDiff) ? (const int*)c->tileTouch : (const int*)nullptr);
  if (t == 2 && fullRound2) return PLI_OK;          // (round 2 regrows everything, as round 1 did: no marks, no k_tx_prep)
  // (round 2 under the lost-pixel rule: k_tx_diff2 has stamped the regions itself, k_rx_mark would find nothing)
  if (lostRule && t >= 3 && !cellRule && !oldMark)
    TRL(c, "k_rx_mark", k_tx_mark, dim3((P.LW + 31) / 32, (c->tilesH + 7) / 8, nimg), dim3(256), 0, txr, t, (const int*)c->tileMin);
  else if (t >= 3 || !lostRule)
    TRL(c, "k_rx_mark", k_rx_mark, dim3((P.LW + 31) / 32, (c->tilesH + 7) / 8, nimg), dim3(256), 0, c->jrCtl, c->own, c->rankOf, c->rgBox,
        c->rgDirty, c->tileMin, c->tileAct, P.LW, P.LH, c->tilesW, c->tilesH, t, img0, t >= 3 ? 1 : 0,
        (lostRule && t >= 3 && !cellRule) ? (const int*)c->rgLost : (const int*)nullptr, txr.DL);
  TxRound prep = txr;                           // (after separate diff and mark passes — dev schedules — no cell stamps, one flag)
  if (!L.fusedDM) prep.tileTouch = nullptr;
  TRL(c, "k_tx_prep", k_tx_prep, dim3((P.LW + 31) / 32, (P.LH + 31) / 32, nimg), dim3(256), 0, prep, t, t == 2 ? 1 : 0);
  return PLI_OK;
}

// Round 1's dev forms.  PLI_TX_SPEC launches the growth itself (`grown`); PLI_TX_XCD and PLI_TX_ORDER change where the plain forms'
// workgroups go (r1.DL).
pli_status tileGrowFirstDev(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S, TxRound& r1, int t, bool& grown) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg, ntile = S.ntile;
  // round 1 in the speculative schedule (lanes grow the small regions of 64 alive seeds at a time, lsd_tile.hip): exact, built
  // and measured in round 3, NOT the default — 37 ms against 22 ms of the plain schedule at 256 frames (the
  // divergent per-lane accept path costs more instructions than the whole-wave steps it replaces).  Dev switch PLI_TX_SPEC=1.
  if (L.lostRule && P.minRegSize >= 3 && L.specEnv) {
    TRL(c, "k_tx_grow", k_tx_grow_spec, dim3(ntile, nimg), dim3(64), 0, r1, t);
    grown = true;
    return PLI_OK;
  }
  // dev switch PLI_TX_ORDER=1: the heaviest tiles first (k_tx_order).  Measured, not the default: the launch does end on fewer
  // stragglers, but consecutive workgroups no longer grow neighbouring tiles of one image and k_tx_grow goes from 23.2 to
  // 31.3 ms at 256 frames (4K: 33.1 -> 44.2 ms) — the grid order's locality is worth more than the balance
  if ((nimg % 8) == 0 && L.xcdEnv) r1.DL.xcdAffine = 1;
  if (L.orderEnv) {
    TRL(c, "k_tx_order", k_tx_order, dim3(1), dim3(1024), 0, (const int*)c->txTileCnt, ntile, nimg, img0, c->txPerm + (int64_t)img0 * ntile);
    r1.DL.perm = c->txPerm + (int64_t)img0 * ntile;
  }
  return PLI_OK;
}

// the lane relaxation (lsd_relax.hip, lsd_mode 1: round 1's schedule, kept for cross-checks)
pli_status relaxLane(pli_ctx* c, const LineCall& L, RelaxPlan& R) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg;
  const int rectBlocks = R.rectBlocks;
  const dim3 raster((P.LW + 255) / 256, P.LH, nimg);
  // grid sizes of the lane growers, the size from which a region counts as large
  const int growBlocks = std::max(16, std::min(256, 2048 / nimg)), bigBlocks = std::max(64, std::min(1024, 16384 / nimg)), bigThresh = RX_HAND;
  const float precDeg = (float)(P.prec * 180.0 / 3.14159265358979323846);
  TRL(c, "k_rx_guess", k_rx_guess, raster, dim3(256), 0, c->rec, c->rankOf, c->own, P.LW, P.LH, precDeg, img0);
  for (int t = 1; t <= R.maxRounds && !R.allDone; ++t) {
    R.curT = t;
    TRL(c, "k_rx_diff", k_rx_diff, dim3((P.LW + 31) / 32, (c->tilesH + 7) / 8, nimg), dim3(256), 0, c->jrCtl, c->own, c->tileMin, c->tileAct,
           P.LW, P.LH, c->tilesW, c->tilesH, t, img0, (const int*)nullptr);
    if (t >= 3) {
      // bookkeeping only where something happened (lsd_relax.hip)
      TRL(c, "k_rx_mark", k_rx_mark, dim3((P.LW + 31) / 32, (c->tilesH + 7) / 8, nimg), dim3(256), 0, c->jrCtl, c->own, c->rankOf, c->rgBox,
          c->rgDirty, c->tileMin, c->tileAct, P.LW, P.LH, c->tilesW, c->tilesH, t, img0, 1, (const int*)nullptr, TxDirtyLists{});
      TRL(c, "k_rx_seed_sparse", k_rx_seed_sparse, dim3((P.LW + 31) / 32, (P.LH + 31) / 32, nimg), dim3(1024), 0, c->jrCtl, c->own, c->rankOf,
          c->rec, c->lastSize, c->rgDirty, c->tileAct, c->smallSeeds, c->bigSeeds, c->bigCap, P.LW, P.LH, c->tilesW, c->tilesH,
          bigThresh, t, img0);
    } else {
      if (t >= 2)
        TRL(c, "k_rx_classify", k_rx_classify, raster, dim3(256), 0, c->jrCtl, c->own, c->rankOf, c->rgBox,
               c->rgClean, c->tileMin, P.LW, P.LH, c->tilesW, c->tilesH, t, img0);
      TRL(c, "k_rx_seed", k_rx_seed, dim3((P.LW + 1023) / 1024, P.LH, nimg), dim3(1024), 0, c->jrCtl, c->own, c->rankOf, c->rec, c->lastSize,
             c->rgClean, c->smallSeeds, c->bigSeeds, c->bigCap, P.LW, P.LH, bigThresh, t, img0);
    }
    TRL(c, "k_rx_grow", k_rx_grow, dim3(growBlocks, nimg), dim3(256), 0, c->dP, c->jrCtl, c->rec, c->own, c->smallSeeds,
           c->lastSize, c->rgBox, c->hand, c->handCap, c->arena, c->arenaCap, c->rects, c->rectCap, img0, t);
    if (nimg <= 4)
      TRL(c, "k_rx_grow_wave", k_rx_grow_wave, dim3(bigBlocks * 4, nimg), dim3(64), 0, c->dP, c->jrCtl, c->rec, c->own, c->bigSeeds,
          c->bigCap, c->hand, c->handCap, c->lastSize, c->rgBox, c->arena, c->arenaCap, c->rects, c->rectCap, img0, t);
    else
      TRL(c, "k_rx_grow_big", k_rx_grow_big, dim3(bigBlocks, nimg), dim3(64), 0, c->dP, c->jrCtl, c->rec, c->own, c->bigSeeds,
          c->bigCap, c->hand, c->handCap, c->lastSize, c->rgBox, c->arena, c->arenaCap, c->rects, c->rectCap, img0, t);
    TRL(c, "k_rx_rect", k_rx_rect, dim3(rectBlocks, nimg), dim3(64), 0, c->dP, c->jrCtl, c->rec, c->arena, c->arenaCap, c->rects,
        c->rectCap, c->rgSeg, img0, c->mg, -1, (const int2*)nullptr, (const float2*)nullptr);
    if (R.trace) {
      HIPCHK(hipMemcpyAsync(c->jrHost.data(), c->jrCtl + img0, sizeof(RxCtl) * nimg, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      const RxCtl& h = c->jrHost[0];
      std::fprintf(stderr, "[rx] t=%d state=%d changed=%d overflow=%d small=%d big=%d hand=%d nextBig=%d rect=%d arena=%lld races=%d\n", t,
                   h.state, h.changed, h.overflow, h.nSmall, h.nBig, h.nHand, h.nextBig, (int)(h.rectArena >> RX_ARENA_BITS),
                   (long long)(h.rectArena & ((1ull << RX_ARENA_BITS) - 1ull)), h.races);
    }
    { pli_status ls_ = look(c, L, R, t); if (ls_ != PLI_OK) return ls_; }
  }
  return PLI_OK;
}
#else
pli_status tileOwnerPassDev(pli_ctx*, const LineCall&, const RelaxPlan&, const TileRounds&, int) { return PLI_OK; }
pli_status tileGrowFirstDev(pli_ctx*, const LineCall&, const RelaxPlan&, const TileRounds&, TxRound&, int, bool&) { return PLI_OK; }
pli_status relaxLane(pli_ctx*, const LineCall&, RelaxPlan&) {
  g_err = "lsd_mode 1 (the lane relaxation) is a development schedule: libpli_frontend_dev.so";
  return PLI_ERR_INVALID;
}
#endif

// region2rect of the regions a round completed, on whatever c->stream is at the call
pli_status tileRectPass(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S) {
  TRL(c, "k_rx_rect", k_rx_rect, dim3(R.rectBlocks, L.nimg), dim3(64), 0, c->dP, c->jrCtl, c->rec, c->arena, c->arenaCap, c->rects,
      c->rectCap, c->rgSeg, L.img0, c->mg, S.txr.DL.rmask, (const int2*)L.hotPlane, (const float2*)L.coldPlane);
  return PLI_OK;
}

// the ORB chain forks from the line chain behind `step` (runChainsBeside, pli_capi.hip, handed it over): the growth of round `step`, or round 2's owner pass (-2)
pli_status forkSideChainBehind(pli_ctx* c, const TileRounds& S, int step) {
  if (!c->sideChain || step != S.sideForkRound) return PLI_OK;
  auto f = std::move(c->sideChain);
  c->sideChain = nullptr;
  return f();
}

// a round, 1: the rounds from t on go to the persistent kernel, which ends by itself
pli_status tileTailHandOver(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S, int t) {
  // (the dirty counters are zero: every list of the last round was taken by its tile's wave; the barrier words were cleared
  // with the control blocks)
  TxTailArgs ta{S.txr, t, R.maxRounds, c->tailBar};
  // (a grid barrier costs 8 us with 256 workgroups and less with fewer: a few images do not need the whole chip in the late rounds)
  // (single pair: k_tx_tail 149 us with 256 workgroups, 90 with 64)
  const int tb = std::min(c->tailBlocks, std::max(64, 8 * L.nimg));
  // k_tx_tail spins on a grid barrier, so its grid must be co-resident; the grid is sized for a device it has to itself.  Two
  // tails in flight at once (two contexts of this process on one device) could each hold a part of the other's slots and spin
  // until the barrier's timeout: tails of one process are chained per device — a tail starts when the previous one has ended.
  // (Other PROCESSES on the device are out of reach of this chain: PLI_TX_TAIL=0 selects the planned-rounds schedule there,
  // include/pli_frontend.h "Sharing a device".)
  std::lock_guard<std::mutex> lk(g_tailMu);
  hipEvent_t& ev = g_tailEv[c->device];             // (0 <= device < TAIL_MAX_DEVICES: tailPossible)
  c->tailLaunched = true;
  ta.forceAbort = S.tailForceAbort ? 1 : 0;
  if (ev) HIPCHK(hipStreamWaitEvent(c->stream, ev, 0));
  else HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  LAUNCH(c, "k_tx_tail", k_tx_tail, dim3(tb), dim3(256), 0, ta);
  HIPCHK(hipEventRecord(ev, c->stream));
  return PLI_OK;
}

// a round, 2: the pass over the owner map — what round t - 1 changed, and from it the regions and tiles round t regrows.  Round 2:
// k_tx_round2; later rounds: the cell lists, or k_tx_diffmark and k_tx_prep.  (Round 1 has none; dev switches: tileOwnerPassDev.)
pli_status tileOwnerPass(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S, int t) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg;
  const TxRound& txr = S.txr;
  if (t == 2 && L.fuseRound2) {
    TRL(c, "k_tx_round2", k_tx_round2, dim3((P.LW + 31) / 32, (P.LH + 31) / 32, nimg), dim3(256), 0, S.first, t,
        (S.pack1 && !L.hotPlane) ? (const float4*)c->rec : (const float4*)nullptr, S.rectAside ? 1 : 0);
    if (S.rectAside) {                               // (round 1's region2rect pass has run beside this kernel: join, then the counter)
      HIPCHK(hipStreamWaitEvent(c->stream, c->evRectDone, 0));
      TRL(c, "k_tx_reset_rect", k_tx_reset_rect, dim3((nimg + 255) / 256), dim3(256), 0, c->jrCtl, nimg, img0);
    }
    return forkSideChainBehind(c, S, -2);       // (before round 2's growth)
  }
  if (t >= 3 && L.fusedDM && S.useCells && t < TX_CELL_ROUNDS) {
    // cell lists (lsd_tile.hip "CELL LISTS"): the cells touched in round t - 1 -> their changed pixels' marks -> the active cells
    // -> their owner words.  A list and its length per image (and round: zeroed once per call) stay on the device; a few
    // workgroups per image stride over its list.
    const int ncell = c->tilesW * c->tilesH;
    // (2048 = TX_CELL_CHUNK cells per listing workgroup; the consumers: 32 waves per image, more for large images)
    const dim3 lg((unsigned)((ncell + 2047) / 2048), nimg), wg((unsigned)(4 * std::max(8, std::min(256, std::max(ncell / 1024, 4096 / nimg)))), nimg);      // (single-wave workgroups)
    int* cntA = c->txCellCnt + ((int64_t)2 * t) * c->rxImages + img0;
    int* cntB = c->txCellCnt + ((int64_t)2 * t + 1) * c->rxImages + img0;
    int* lst = c->txCellList + (int64_t)img0 * ncell;
    TRL(c, "k_tx_cells", k_tx_cells, lg, dim3(256), 0, c->jrCtl, (const int*)c->tileTouch, c->tileTouch, ncell, nimg, img0, t, 0, lst, cntA);
    TRL(c, "k_tx_diffmark", k_tx_diffmark_cells, wg, dim3(64), 0, txr, t, (const int*)lst, (const int*)cntA);
    TRL(c, "k_tx_cells", k_tx_cells, lg, dim3(256), 0, c->jrCtl, (const int*)c->tileAct, c->tileTouch, ncell, nimg, img0, t, 1, lst, cntB);
    TRL(c, "k_tx_prep", k_tx_prep_cells, wg, dim3(64), 0, txr, t, (const int*)lst, (const int*)cntB);
    return PLI_OK;
  }
  if (t >= 3 && L.fusedDM) {
    TRL(c, "k_tx_diffmark", k_tx_diffmark, dim3((P.LW + 31) / 32, (c->tilesH + 7) / 8, nimg), dim3(256), 0, txr, t);
    // (k_tx_diffmark has done the marks)
    TRL(c, "k_tx_prep", k_tx_prep, dim3((P.LW + 31) / 32, (P.LH + 31) / 32, nimg), dim3(256), 0, txr, t, 0);
    return PLI_OK;
  }
  return tileOwnerPassDev(c, L, R, S, t);
}

// a round, 3: the growth — round 1 (and a dev round 2 that regrows everything) from the tiles' seed lists, later rounds from their
// dirty lists
pli_status tileGrow(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S, int t) {
  const int nimg = L.nimg, ntile = S.ntile;
  if (t >= 3 || (t == 2 && !L.fullRound2)) {
    TxRound grow = S.txr;                           // (dev: a round 2 that regrows everything walks the seed lists, not the dirty lists)
    if (L.fullRound2 && t == 2) grow.DL = S.noDL;
    if (L.hotLater) TRL(c, "k_tx_grow_sparse", k_tx_grow_sparse_h, dim3(ntile, nimg), dim3(64), 0, grow, t);
    else TRL(c, "k_tx_grow_sparse", k_tx_grow_sparse, dim3(ntile, nimg), dim3(64), 0, grow, t);
    return PLI_OK;
  }
  TxRound r1 = S.first;                             // (round 1: no dirty lists yet, every tile walks its seed list)
  r1.DL = S.noDL;
  bool grown = false;
  const pli_status ds = tileGrowFirstDev(c, L, R, S, r1, t, grown);
  if (ds != PLI_OK || grown) return ds;
  // (the forms with owner_1 packed into the records, 16-byte or hot, take the keys beside the planes)
  void (*const packed)(TxRound, int, TxKeys) = (L.hotPlane && L.packMode == 2) ? k_tx_grow_h2 : L.packMode == 2 ? k_tx_grow_p2 :
                                               (!L.hotPlane && L.packMode == 1) ? k_tx_grow_p1 : nullptr;
  if (packed) TRL(c, "k_tx_grow", packed, dim3(ntile, nimg), dim3(64), 0, r1, t, S.keys);
  else if (L.hotPlane)       // (the default: the one kernel with its planes as `__restrict__` parameters, lsd_tile.hip k_tx_grow_h1)
    TRL(c, "k_tx_grow", k_tx_grow_h1, dim3(ntile, nimg), dim3(64), 0, r1.Pp, r1.ctl, r1.rec, r1.own, r1.list, r1.tileCnt, r1.ts,
        r1.ntx, r1.nty, r1.rgSize, r1.rgBox, (const int*)r1.rgDirty, (const int*)r1.tileAct, r1.TW, r1.TH, r1.arena, r1.arenaCap,
        r1.rects, r1.rectCap, r1.img0, t, r1.rank, r1.rgLost, r1.tileTouch, r1.DL, S.keys);
  else TRL(c, "k_tx_grow", k_tx_grow, dim3(ntile, nimg), dim3(64), 0, r1, t);
  return PLI_OK;
}

// a round, 4: region2rect of the regions the round completed — round 1's, in the default schedule, on a side stream beside round 2's
// pass over the owner map
pli_status tileRect(pli_ctx* c, const LineCall& L, const RelaxPlan& R, const TileRounds& S, int t) {
  if (t != 1 || !S.rectAside) return tileRectPass(c, L, R, S);
  // Round 1's region2rect pass (gather / latency bound, 2.9 ms at 256 frames) beside round 2's pass over the owner map (bandwidth
  // bound, 2.1 ms): the two touch disjoint data — the pass reads the round's pixel lists and writes the segment plane, k_tx_round2
  // reads the packed owner words and writes the owner plane — except the list counter, which k_tx_round2 leaves alone here and
  // k_tx_reset_rect clears after the join, before round 2's growth allocates from it.
  if (!c->evRectFork) {
    HIPCHK(hipEventCreateWithFlags(&c->evRectFork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evRectDone, hipEventDisableTiming));
  }
  // Which stream: the runtime maps streams onto FOUR hardware queues, and a context that pipelines host batches already has
  // four (kernels, the ORB chain's side stream, the two copy streams) — a fifth shares a queue with a copy stream, and the
  // host-inclusive rate fell from 0.99x to 0.93x of the resident one.  The ORB chain's stream is idle until the chain forks
  // (behind round 2 in large batches): the pass borrows it then; otherwise a stream of its own, unless the host pipeline is in use.
  hipStream_t rectS = S.rectOnSide ? c->aux : c->aux2;
  if (!rectS) {
    HIPCHK(hipStreamCreateWithFlags(&c->aux2, hipStreamNonBlocking));
    rectS = c->aux2;
  }
  HIPCHK(hipEventRecord(c->evRectFork, c->stream));
  HIPCHK(hipStreamWaitEvent(rectS, c->evRectFork, 0));
  {
    StreamScope onSide(c, rectS);
    const pli_status rs = tileRectPass(c, L, R, S);
    if (rs != PLI_OK) return rs;
  }
  HIPCHK(hipEventRecord(c->evRectDone, rectS));
  return PLI_OK;
}

// tile-sequential relaxation (lsd_tile.hip): per-tile seed lists once, then rounds of one wave per tile
pli_status relaxTile(pli_ctx* c, const LineCall& L, RelaxPlan& R) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg;
  const int64_t npix64 = (int64_t)L.npix;
  const bool keyMode = L.keyMode, fusedDM = L.fusedDM;
  const bool trace = R.trace, perRound = R.perRound, blocking = R.blocking;
  const int maxRounds = R.maxRounds;
  int2* const hotPlane = L.hotPlane;
  float2* const coldPlane = L.coldPlane;
  const int ts = c->txTs, ntile = c->txNtx * c->txNty;
  // (test switch: a wide margin sends every unclaimed pixel of the LAZY form through the double plane; the results must not change)
  const char* const lazyMarginEnv = DEVENV("PLI_TX_LAZY_MARGIN");
  const char* const forkRoundEnv = DEVENV("PLI_SIDE_FORK_ROUND");
  const char* const rectAsideEnv = DEVENV("PLI_RECT_ASIDE");
  const char* const cellsEnv = DEVENV("PLI_TX_CELLS");
  const char* const tailT0Env = DEVENV("PLI_TX_TAIL_T0");
  const bool tailForceAbort = DEVENV("PLI_TX_TAIL_FORCE_ABORT") != nullptr;   // test switch: the kernel leaves at once, as after a barrier timeout
  TxKeys keys{};
  if (keyMode) keys = TxKeys{c->mg, c->maxMg, P.rho, P.nBins, c->txPixBits, c->rankOf};
  const bool pack1 = L.packMode != 0;
  if (pack1) { keys.recPack = c->rec; keys.pack = L.packMode; keys.hot = hotPlane; keys.cold = coldPlane; }
  if (lazyMarginEnv) keys.lazyMargin = std::max(4, std::min(0x3FFFFFFF, atoi(lazyMarginEnv)));
#ifdef PLI_DEV
  if (ts == 128)
    TRL(c, "k_tx_sort", k_tx_sort128, dim3(ntile, nimg), dim3(1024), 0, c->rankOf, c->order, c->own, c->txList,
        c->txTileCnt, P.LW, P.LH, ts, c->txNtx, c->txNty, img0, keys);
  else
#endif
    TRL(c, "k_tx_sort", k_tx_sort, dim3(ntile, nimg), dim3(256), 0, c->rankOf, c->order, c->own, c->txList,
        c->txTileCnt, P.LW, P.LH, ts, c->txNtx, c->txNty, img0, keys);
  TxDirtyLists DL{c->txDirtyList, c->txDirtyCnt, c->order, ts, c->txNtx, c->txNty, P.LW, npix64};
  if (keyMode) DL.rmask = (1 << c->txPixBits) - 1;
  DL.stamp = R.stampBase;
  if (L.noDirtyList) DL.list = nullptr;
  TxDirtyLists noDL = DL; noDL.list = nullptr;
  // The planes of the relaxation, the one argument record of every kernel of a round (TxRound, common.hpp).  A launch that differs in
  // a field takes a copy: `first` — round 1 and round 2's pass over the owner map read ROUND 1's hot records, the later rounds theirs.
  const TxRound txr{c->dP, c->jrCtl, c->rec, c->own, c->txList, c->txTileCnt, ts, c->txNtx, c->txNty, c->lastSize, c->rgBox, c->rgDirty,
                    c->tileAct, c->tileTouch, P.LW, P.LH, c->tilesW, c->tilesH, c->arena, c->arenaCap, c->rects, c->rectCap, c->rgSeg,
                    c->mg, c->rankOf, L.lostRule ? c->rgLost : (int*)nullptr, DL, img0, nimg, L.hotLater, coldPlane};
  TxRound first = txr; first.hot = hotPlane;
  // Where the deferred ORB chain forks from the line chain (runChainsBeside, pli_capi.hip): behind round 1's growth up to 64 images, behind round 2's
  // pass over the owner map (-2) above — what waits in a large batch is the END of the line chain (the 1024-thread / 64 KB workgroups
  // of k_tx_emit_sorted, the gated k_lsd_scan, k_keylines find no room while the ORB chain fills every hole), so the chain should end
  // early, and k_tx_round2, which the ORB kernels stretch most, should run alone.  Same box, 256 frames, fork behind round 1 /
  // round 2's owner pass / round 2 / round 3: synthetic 45.0 / 45.0 / 45.4-45.5 / 46.2 ms, photographs 28.6 / 28.5 / 29.5 / 30.0
  // (DESIGN.md 5 has the history).  Dev switch PLI_SIDE_FORK_ROUND: a round t >= 2 (behind its growth), -2, anything else round 1.
  const int forkRoundAsked = forkRoundEnv ? atoi(forkRoundEnv) : 0;
  const int sideForkRound = forkRoundAsked == 0 ? (nimg <= 64 ? 1 : -2) : forkRoundAsked == -2 ? -2 : std::max(1, forkRoundAsked);
  // (round 1's region2rect pass on a stream of its own beside k_tx_round2: the default schedule only; dev switch PLI_RECT_ASIDE=0)
  // (a single pair pays 0.06 ms for the two events and the reset launch and has nothing to overlap: from 8 images on)
  // (the ORB chain's stream when the chain is waiting to fork behind round 2 or later: idle until then)
  const bool rectOnSide = c->sideChain && c->aux && sideForkRound != 1;
  const bool rectAside = L.fuseRound2 && !trace && !perRound && !blocking && maxRounds >= 2 && !c->syncDebug &&
                         (rectAsideEnv ? atoi(rectAsideEnv) != 0 : (nimg >= 8 && (rectOnSide || c->sH2D == nullptr)));
  // rounds 3 .. tail start of a large batch by cell lists (six lean launches per round instead of four that walk every block;
  // a small batch keeps the four: launches are what it pays for).  Dev switch PLI_TX_CELLS=0 / 1.
  // (measured: 256 frames of 752 x 480 +2 %, 64 of 1280 x 720 +1 %, 16 of 4K +2 %; 32 frames of 752 x 480 -4 %: a million cells is the line)
  bool useCells = fusedDM && DL.list && c->txCellList && (int64_t)c->tilesW * c->tilesH * nimg >= (1 << 20);
  if (cellsEnv) useCells = atoi(cellsEnv) != 0 && fusedDM && DL.list && c->txCellList;
  // Rounds >= tailT0 in one persistent launch that ends by itself when every image is at its fixed point (no host look, no planned
  // round count; switches: PLI_TX_TAIL=0, PLI_TX_TAIL_T0).
  // The persistent kernel takes over at round 8 — at round 12 when the rounds before it run on cell lists: their launches are lean, and
  // a large batch still has the ORB chain on the chip around round 8, beside which the tail's 256 workgroups of 50 KB LDS, which must
  // ALL be resident, wait for their compute units (k_tx_tail 0.7 ms alone, 2.6 ms in the default line).  256 frames, same box, start
  // at 8 / 12 / 14 / 16: synthetic 46.0-46.1 / 45.7 / 45.6 / 45.6 ms, photographs 29.2-29.3 / 29.3 / 29.4 / 29.7.
  int tailT0 = useCells ? 12 : 8;
  if (tailT0Env) tailT0 = std::max(3, atoi(tailT0Env));
  const TileRounds S{keys, txr, first, noDL, ntile, pack1, sideForkRound, rectOnSide, rectAside, useCells, tailT0, tailForceAbort};
  pli_status st;
  for (int t = 1; t <= maxRounds && !R.allDone; ++t) {
    R.curT = t;
    if (R.tailPossible && t == tailT0) return tileTailHandOver(c, L, R, S, t);
    if ((st = tileOwnerPass(c, L, R, S, t)) != PLI_OK) return st;
    if ((st = tileGrow(c, L, R, S, t)) != PLI_OK) return st;
    if ((st = forkSideChainBehind(c, S, t)) != PLI_OK) return st;         // (pli_batch_run: behind round 1's growth by default, a later round's by the dev switch)
    if ((st = tileRect(c, L, R, S, t)) != PLI_OK) return st;
    if (trace) {
      HIPCHK(hipMemcpyAsync(c->jrHost.data(), c->jrCtl + img0, sizeof(RxCtl) * nimg, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      const RxCtl& h = c->jrHost[0];
      std::fprintf(stderr, "[tx] t=%d state=%d changed=%d overflow=%d rect=%d arena=%lld\n", t, h.state, h.changed, h.overflow,
                   (int)(h.rectArena >> RX_ARENA_BITS), (long long)(h.rectArena & ((1ull << RX_ARENA_BITS) - 1ull)));
    }
    if ((st = look(c, L, R, t)) != PLI_OK) return st;
  }
  return PLI_OK;
}

// the segments of the relaxed owner maps; the images that ran out of a capacity or did not settle go through the sequential grower;
// the call's round counts start their way to the host
pli_status lineEmit(pli_ctx* c, const LineCall& L, const RelaxPlan& R) {
  const DevParams& P = c->hp;
  const int img0 = L.img0, nimg = L.nimg;
  const int64_t npix64 = (int64_t)L.npix;
  const bool keyMode = L.keyMode, blocking = R.blocking;
  if (keyMode) {
    int emitCap = TX_EMIT_CAP;                   // (test switch: a small list, so that images take the overflow path to the sequential grower)
    if (const char* e = DEVENV("PLI_TX_EMITCAP")) emitCap = std::max(1, std::min(TX_EMIT_CAP, atoi(e)));
    TRL(c, "k_tx_collect", k_tx_collect, dim3(std::max(1, std::min(64, (int)((npix64 + 2047) / 2048))), nimg), dim3(256), 0, c->jrCtl,
        (const int*)c->rankOf, (const int2*)c->own, (const int*)c->lastSize, npix64, P.minRegSize, c->txCand, c->txCandCnt, img0, emitCap,
        (const int2*)c->rgBox, P.segBoxCut);
    TRL(c, "k_tx_emit_sorted", k_tx_emit_sorted, dim3(nimg), dim3(1024), TX_EMIT_CAP * 4, (const RxCtl*)c->jrCtl, (const int*)c->txCand,
        (const int*)c->txCandCnt, (const float4*)c->rgSeg, npix64, (1 << c->txPixBits) - 1, c->seg, c->nSeg, c->maxSeg, img0, emitCap);
    // (the ordered lists of the images left to the sequential grower, decided on the device: normally none, and the three passes end at once)
    pli_status os = lineOrder(c, L, c->jrCtl);
    if (os != PLI_OK) return os;
  } else {
    TRL(c, "k_rx_count", k_rx_count, dim3(c->rxChunks, nimg), dim3(256), 0, c->jrCtl, c->order, c->nDefined, c->own, c->lastSize,
           c->rxChunkCnt, c->rxChunks, npix64, P.minRegSize, img0, (const int2*)c->rgBox, P.segBoxCut);
    TRL(c, "k_rx_emit", k_rx_emit, dim3(c->rxChunks, nimg), dim3(256), 0, c->jrCtl, c->order, c->nDefined, c->own, c->lastSize,
           c->rgSeg, c->rxChunkCnt, c->rxChunks, npix64, P.minRegSize, c->seg, c->nSeg, c->maxSeg, img0,
           (const int2*)c->rgBox, P.segBoxCut);
  }
  // images that ran out of a capacity (or did not settle) take the sequential grower
  // (... which reads the 16-byte records: with every round on the hot records nobody has written them — for those images, now)
  if (L.hotLevel == 2)
    LAUNCH(c, "k_tx_rec_from_hot", k_tx_rec_from_hot, dim3(std::max(1, std::min(64, (int)((npix64 + 4095) / 4096))), nimg), dim3(256), 0,
           (const RxCtl*)c->jrCtl, (const int2*)c->hot, (const float2*)c->cold, c->rec, npix64, img0);
  if (blocking && !keyMode) {
    for (int i = 0; i < nimg; ++i) {
      if (c->jrHost[i].overflow || c->jrHost[i].state != 2) {
        LAUNCH(c, "k_lsd_grow", k_lsd_grow, dim3(1), dim3(64), 0, c->dP, c->rec, c->mg, c->order, c->nDefined,
               c->regScratch, c->seg, c->nSeg, c->maxSeg, img0 + i, 1);
      }
    }
    return PLI_OK;
  }
  // ... decided on the device: the waves of the settled images leave at once
  LAUNCH(c, "k_lsd_grow_unsettled", k_lsd_grow_unsettled, dim3(nimg), dim3(64), 0, c->dP, c->rec, c->mg, c->order, c->nDefined,
         c->regScratch, c->seg, c->nSeg, c->maxSeg, img0, nimg, c->jrCtl);
  if (blocking) return PLI_OK;
  if (!c->rxSeen) {
    HIPCHK(hipHostMalloc((void**)&c->rxSeen, sizeof(int) * (4 * (size_t)c->NI + 1), hipHostMallocDefault));     // (+ the tail's abort word)
    c->rxSeen[4 * (size_t)c->NI] = 0;
    HIPCHK(hipEventCreateWithFlags(&c->evRxSeen, hipEventDisableTiming));
  }
  if (c->rxSeenImages == 0) {                       // (an earlier copy still in flight keeps the buffer: this call is not sampled)
    HIPCHK(hipMemcpy2DAsync(c->rxSeen, 16, c->jrCtl + img0, sizeof(RxCtl), 16, nimg, hipMemcpyDeviceToHost, c->stream));
    if (c->tailBar && c->tailLaunched)
      HIPCHK(hipMemcpyAsync(c->rxSeen + 4 * (size_t)c->NI, c->tailBar + 32, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    else c->rxSeen[4 * (size_t)c->NI] = 0;
    HIPCHK(hipEventRecord(c->evRxSeen, c->stream));
    c->rxSeenImages = nimg;
    c->rxSeenTail = c->tailLaunched;
  }
  return PLI_OK;
}

// keylines from the segments, and their LBD descriptors
pli_status lineDescribe(pli_ctx* c, const LineCall& L, uint8_t* table) {
  const DevParams& P = c->hp;
  const pli_table_layout& Y = c->lay;
  const int img0 = L.img0, nimg = L.nimg;
  LAUNCH(c, "k_keylines", k_keylines, dim3(nimg), dim3(256), 0, c->dP, c->seg, c->nSeg, c->maxSeg, c->tmpKL, table,
         Y.record_bytes, Y.off_counts, Y.off_kl[0], Y.off_kl[1], img0);
  if (c->lbdPreOnSide) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->evLbdPre, 0));   // (the blur + Sobel of the LBD ran on the side stream, see runChainsBeside in pli_capi.hip)
  } else {
    pli_status ls = runLbdPre(c, img0, nimg);
    if (ls != PLI_OK) return ls;
  }
  LAUNCH(c, "k_lbd", k_lbd, dim3(P.klCap, nimg), dim3(64), 0, c->dP, c->lbdCoef, c->dxy, table, Y.record_bytes,
         Y.off_counts, Y.off_kl[0], Y.off_kl[1], Y.off_ldesc[0], Y.off_ldesc[1], c->debug ? c->lbdFloat : (float*)nullptr, img0);
  return PLI_OK;
}

}  // namespace

// The line chain of images img0 .. img0 + nimg - 1 on the context's stream: keylines and LBD descriptors into their tables.
pli_status runLines(pli_ctx* c, int img0, int nimg, uint8_t* table) {
  TraceRange range__("pli:line chain");
  const LineCall L = resolveLineCall(c, img0, nimg);
  pli_status st;
  if ((st = lineFront(c, L)) != PLI_OK) return st;
  // (key mode has no ordered list: lineEmit builds it for the images left to the sequential grower)
  if (!L.keyMode && (st = lineOrder(c, L, nullptr)) != PLI_OK) return st;
  if (L.sequential) {
    if ((st = lineGrowSequential(c, L)) != PLI_OK) return st;
  } else {
    RelaxPlan R{};
    if ((st = planRelaxation(c, L, R)) != PLI_OK) return st;
    if ((st = L.tile ? relaxTile(c, L, R) : relaxLane(c, L, R)) != PLI_OK) return st;
    if ((st = lineEmit(c, L, R)) != PLI_OK) return st;
  }
  return lineDescribe(c, L, table);
}
