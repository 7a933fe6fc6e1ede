/*
 * pli_frontend.h — C ABI of the MI355X-native point+line front-end.
 *
 * This is the drop-in boundary underneath PLI-SLAM's per-frame front-end
 * (Frame::Frame stereo ctor, reference src/Frame.cc:98-228).  The reference has
 * no FFI of its own: its boundary is a set of C++ call sites.  Every entry
 * point below names the reference call it replaces (file:line under the
 * reference tree).  The C++ adapters in pli_slam_amd/adapters/ keep the
 * reference's functor signatures and call these functions; INTEGRATION.md
 * shows the binding a maintainer adds to Frame.cc / Tracking.cc.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary; every function
 *     returns a pli_status (0 = ok, negative = error).
 *   - caller owns all buffers; outputs are caller-allocated with a capacity and
 *     the function returns the produced count.
 *   - "host" pointers are ordinary memory; "dev" pointers are HIP device
 *     memory of the context's device.
 *   - a context owns its HIP streams and all scratch for `max_frames` stereo
 *     frames of `width x height`.  Every entry point that takes a context is
 *     THREAD-SAFE: it holds the context's own lock for the whole call, so
 *     concurrent calls on ONE context are legal and run one after the other
 *     (the reference drives its four extractors from four std::threads,
 *     Frame.cc:128-135, and the adapters put the four on one context — the
 *     stereo matchers need both eyes' tables on the device).  Calls on
 *     DIFFERENT contexts run concurrently.  What the lock does not order is
 *     the caller's own protocol: pli_stereo_match_* read the tables of the LAST
 *     extract calls, so a second Frame must not start extracting on a context
 *     while the first Frame's stereo matchers have not run yet.
 *     pli_ctx_destroy must not race with other calls on that context.
 *   - Sharing a device.  Several contexts of ONE process may share a device
 *     freely.  The late rounds of the LSD tile relaxation run in a persistent
 *     kernel with a grid barrier (k_tx_tail) whose grid is sized for a device
 *     it has to itself; the library starts such a kernel only when the
 *     previous one of this process on that device has ended.  Several
 *     PROCESSES on one device (ranks sharing a GPU) should set PLI_TX_TAIL=0
 *     in their environment (the planned-rounds schedule, no spinning kernel):
 *     without it two processes' tail kernels can each hold part of the
 *     compute units the other needs; every barrier wait is bounded (about a
 *     second), the kernels then give up and the images that had not settled
 *     are redone by the sequential grower — results stay exact, the call
 *     stalls, and pli_lsd_round_stats out[2] counts the images.  A process
 *     that sees this happen once (the control blocks of a call come back with
 *     unsettled images although the persistent kernel ran) switches itself to
 *     the planned-rounds schedule on that device for the rest of its life and
 *     says so once on stderr: the stall is paid at most twice, not per call.
 */
#ifndef PLI_FRONTEND_H
#define PLI_FRONTEND_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t pli_status;
enum {
  PLI_OK = 0,
  PLI_ERR_INVALID = -1,     /* bad argument (null pointer, size mismatch, ...)            */
  PLI_ERR_EMPTY_IMAGE = -2, /* ORBextractor::operator() returns -1, ORBextractor.cc:1072  */
  PLI_ERR_CAPACITY = -3,    /* caller buffer too small                                     */
  PLI_ERR_HIP = -4,         /* HIP runtime failure (see pli_last_error)                    */
  PLI_ERR_NO_DEVICE = -5,   /* no usable gfx950 device: the product path has no CPU fallback */
  PLI_ERR_STATE = -6        /* call order violated (e.g. stereo match before extract)      */
};

/* cv::KeyPoint fields that leave the extractor (ORBextractor.cc:868-877,1131):
 * pt, size, angle, response, octave.  class_id is always -1 there. 24 bytes. */
typedef struct pli_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
} pli_keypoint;

/* cv::line_descriptor::KeyLine, field for field
 * (Thirdparty/line_descriptor/include/line_descriptor/descriptor_custom.hpp:105-144). 68 bytes. */
typedef struct pli_keyline {
  float angle;
  int32_t class_id;
  int32_t octave;
  float pt_x, pt_y;
  float response;
  float size;
  float startPointX, startPointY, endPointX, endPointY;
  float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
  float lineLength;
  int32_t numOfPixels;
} pli_keyline;

/* Parameters of the path.  Sources: ORBextractor ctor (ORBextractor.cc:408),
 * Lineextractor ctor (LineExtractor.h:44), Tracking.cc:75-98,683-736,
 * Config.cpp:26-160, Examples/Stereo/Config/EuRoC.yaml. */
typedef struct pli_frontend_config {
  int32_t width, height;      /* image size the context is built for                     */
  int32_t max_frames;         /* stereo frames per batch the context can hold (>=1)       */
  /* ORB */
  int32_t orb_nfeatures;      /* ORBextractor.nFeatures   (EuRoC.yaml:91)  1200            */
  float   orb_scale_factor;   /* ORBextractor.scaleFactor (EuRoC.yaml:94)  1.2             */
  int32_t orb_nlevels;        /* ORBextractor.nLevels     (EuRoC.yaml:97)  8               */
  int32_t orb_ini_th_fast;    /* ORBextractor.iniThFAST   (EuRoC.yaml:103) 20              */
  int32_t orb_min_th_fast;    /* ORBextractor.minThFAST   (EuRoC.yaml:104) 7               */
  /* LSD / LBD */
  int32_t lsd_nfeatures;      /* EuRoC.yaml:156 (500); 0 = keep all                        */
  int32_t lsd_refine;         /* only 0 (LSD_REFINE_NONE) is on the reference path         */
  int32_t lsd_n_bins;         /* 1024                                                      */
  int32_t max_lines;          /* capacity for detected segments before the top-N cut      */
  double  min_line_length;    /* 0.025 (x min(W,H))                                        */
  double  lsd_scale;          /* 1.2                                                       */
  double  lsd_sigma_scale;    /* 0.6                                                       */
  double  lsd_quant;          /* 2.0                                                       */
  double  lsd_ang_th;         /* 22.5                                                      */
  double  lsd_log_eps;        /* 1.0  (unused with refine 0)                               */
  double  lsd_density_th;     /* 0.6  (unused with refine 0)                               */
  /* stereo points (Frame.cc:976-1154) */
  float   bf;                 /* Camera.bf (EuRoC.yaml:28) 47.90639384423901               */
  float   fx;                 /* Camera.fx (EuRoC.yaml:9)  435.2046959714599               */
  int32_t stereo_maxd_inf;    /* 0: maxD = bf/(bf/fx) as intended; 1: maxD = +inf
                                 (what an uninitialised mb gives)       */
  /* stereo lines (Frame.cc:1156-1307, LineMatcher.cpp:317-396, Config.cpp) */
  int32_t matching_s_ws;      /* 10                                                        */
  int32_t best_lr_matches;    /* 1                                                         */
  double  line_sim_th;        /* 0.75                                                      */
  double  stereo_overlap_th;  /* 0.75                                                      */
  double  min_ratio_12_l;     /* 0.9                                                       */
  double  ls_min_disp_ratio;  /* 0.7                                                       */
  double  min_disp;           /* 1.0                                                       */
  double  line_horiz_th;      /* 0.1                                                       */
  /* execution strategy of the LSD region grower (results are identical):
     0 = auto (by batch size: 3 below 1280 frames per call, 2 from there on — capi_host.hpp: RX_AUTO_IMAGES, a measured crossover; a context created for 1280 frames or more keeps the buffers of mode 3 for 1023 frames only),
     1 = rank-ordered relaxation, one region per lane / lane group (lsd_relax.hip),
     2 = sequential, one wave per image (line_kernels.hip: k_lsd_grow),
     3 = tile-sequential relaxation, one wave per 64x64 tile (lsd_tile.hip) */
  int32_t lsd_mode;
  /* Arithmetic the reference leaves to its toolchain (PLI_PARITY_*, below): which libm function an unqualified
     cos(float) resolves to, and which OpenCV generation's LineSegmentDetector is linked.  Oracle and kernels honour the
     same flags; DESIGN.md "Oracle" says what is known about each. */
  int32_t parity_flags;
} pli_frontend_config;

enum {
  /* cos/sin of the FLOAT angle in computeOrbDescriptor (ORBextractor.cc:110-111; the file says `using namespace std;`,
     so the float overload std::cos(float) = cosf is selected): 1 = cosf/sinf as glibc >= 2.28 computes them,
     0 = correctly rounded ((float)cos((double)x)).  Default 1. */
  PLI_PARITY_TRIG_F32_ORB = 1,
  /* the same choice for `cos(float(angle))` in OpenCV's lsd.cpp region_grow (inside namespace cv, no using-directive:
     the overload depends on whether the C++ <math.h> wrapper is in scope).  Default 0. */
  PLI_PARITY_TRIG_F32_LSD = 2,
  /* ... and for `cos(direction)` in BinaryDescriptor::computeLBD (binary_descriptor_custom.cpp:1130).  Default 0.
     Measured (tests/test_ref_pin_line.py, DESIGN.md "Oracle"): compiled where it lies with GCC 11 / libstdc++, that file
     selects the FLOAT overload (= 1), because the reference's own bitarray_custom.hpp includes <math.h>, whose C++ wrapper
     (libstdc++ of GCC 6 and later) puts the float overloads into the global namespace; the stand-in headers' own regime
     made no difference.  That contradicts this default, which is kept: an OpenCV 3.3.1 header set and a pre-GCC-6
     libstdc++ (whose <math.h> is the C header: double) were not measured. */
  PLI_PARITY_TRIG_F32_LBD = 4,
  /* LineSegmentDetector on the CV_64FC1 copy of the image (OpenCV 3.0 .. 3.4: double Gaussian blur, double bilinear
     resize, double gradient) instead of the CV_8UC1 pipeline of the detector re-added in 4.5.x.  Default 1: the reference
     pins OpenCV 3.3.1 (README.md:18-20). */
  PLI_PARITY_LSD_F64 = 8,
  /* the same choice for `atan2( endPointY - startPointY, endPointX - startPointX )` of KeyLine::angle in
     LSDDetectorC::detectImpl (LSDDetector_custom.cpp:298, two float arguments, inside namespace cv::line_descriptor):
     1 = atan2f as glibc up to 2.40 computes it (the fdlibm float algorithm), 0 = correctly rounded
     ((float)atan2((double)y, (double)x)).  Default 0; the same measurement as for PLI_PARITY_TRIG_F32_LBD found 1. */
  PLI_PARITY_TRIG_F32_KEYLINE = 16
};

/* Fill `cfg` with the values of Examples/Stereo/Config/EuRoC.yaml for a w x h image
 * (parity_flags = PLI_PARITY_TRIG_F32_ORB | PLI_PARITY_LSD_F64). */
void pli_config_default(pli_frontend_config* cfg, int32_t width, int32_t height);

/* Capacities derived from a config (sizes of the per-eye tables). */
int32_t pli_kp_capacity(const pli_frontend_config* cfg);   /* >= nfeatures + 3*nlevels    */
int32_t pli_kl_capacity(const pli_frontend_config* cfg);   /* lsd_nfeatures or max_lines  */
/* The short-segment cut of a plain (non-debug) context: a line-support region whose bounding box in the scaled image has
 * bw^2 + bh^2 <= this value cannot yield a segment longer than min_line_length * min(width, height), so the detector computes
 * no segment for it (the key-line tables do not change: such a segment fails the length test anyway).  -1: no cut. */
int32_t pli_lsd_segment_box_cut(const pli_frontend_config* cfg);

/* ------------------------------------------------------------------------ */
/* Result table: one fixed-stride record per stereo frame, written on the    */
/* device by pli_batch_run.  Layout (all offsets from the record start, in  */
/* bytes) is described by pli_table_layout so that the caller can slice it   */
/* from any language; eye 0 = left, eye 1 = right.                           */
/* ------------------------------------------------------------------------ */
typedef struct pli_table_layout {
  int64_t record_bytes;       /* stride between consecutive frames                         */
  int32_t kp_cap, kl_cap;
  int64_t off_counts;         /* int32[8]: n_kp[2], n_kl[2], n_stereo_pts, n_stereo_lines, truncation flags, 1 reserved.
                                 Flags = 4 bytes: [0],[1] lines of eye 0 / 1: more segments passed the length cut than
                                 max_lines holds (the top-N selection did not see all of them); [2],[3] keypoints of eye
                                 0 / 1 cut at kp_cap.  The per-call entry points return PLI_ERR_CAPACITY for them. */
  int64_t off_kp[2];          /* pli_keypoint[kp_cap]                                       */
  int64_t off_desc[2];        /* uint8[kp_cap][32]   (mDescriptors / mDescriptorsRight)     */
  int64_t off_uright;         /* float[kp_cap]       (mvuRight)                             */
  int64_t off_depth;          /* float[kp_cap]       (mvDepth)                              */
  int64_t off_kl[2];          /* pli_keyline[kl_cap]                                        */
  int64_t off_ldesc[2];       /* uint8[kl_cap][32]   (mDescriptors_Line / ..Right_Line)     */
  int64_t off_disp;           /* float[kl_cap][2]    (mvDisparity_l)                        */
  int64_t off_le;             /* double[kl_cap][3]   (mvle_l)                               */
} pli_table_layout;

typedef struct pli_ctx pli_ctx;

/* Create / destroy.  Replaces the construction of the four extractors in
 * Tracking.cc:87-98,743-749 (tables, rBRIEF pattern, LBD weights go to the device). */
pli_status pli_ctx_create(const pli_frontend_config* cfg, int32_t device, pli_ctx** out);
void       pli_ctx_destroy(pli_ctx* ctx);
const char* pli_last_error(void);                    /* thread-local message             */
pli_status pli_ctx_layout(const pli_ctx* ctx, pli_table_layout* out);
/* Use an existing hipStream_t (e.g. the caller framework's current stream). NULL = own stream. */
pli_status pli_ctx_set_stream(pli_ctx* ctx, void* hip_stream);
pli_status pli_ctx_sync(pli_ctx* ctx);

/* ------------------------------------------------------------------------ */
/* Batch (throughput) path: the whole Frame::Frame front-end for `nframes`   */
/* stereo pairs in one go — ExtractORB x2, ExtractLine x2 (Frame.cc:128-135),*/
/* ComputeStereoMatches_Lines (:160), ComputeStereoMatches (:163).           */
/* Images: device pointers, u8, row stride `stride`, consecutive frames      */
/* `frame_stride` bytes apart (no alignment needed).  Output: `dev_table` =  */
/* nframes records, 16-byte aligned (PLI_ERR_INVALID otherwise).             */
/* Asynchronous on the context stream; pli_ctx_sync() to wait.               */
/* Monocular / RGB-D colour streams (Frame.cc:231,334: one image per frame):  */
/* pass frame 0 as `left`, frame 1 as `right`, frame_stride = two frames,     */
/* nframes = half the stream, stages = PLI_RUN_ORB | PLI_RUN_LINES — frames   */
/* 2i and 2i+1 then fill the two eye slots of record i.                       */
/* ------------------------------------------------------------------------ */
enum {
  PLI_RUN_ORB = 1, PLI_RUN_LINES = 2, PLI_RUN_STEREO_POINTS = 4, PLI_RUN_STEREO_LINES = 8,
  PLI_RUN_ALL = 15
};
pli_status pli_batch_run(pli_ctx* ctx, int32_t nframes,
                         const uint8_t* dev_left, const uint8_t* dev_right,
                         int64_t stride, int64_t frame_stride,
                         uint32_t stages, void* dev_table);
/* Same with host images and a host table (does the H2D / D2H copies, synchronous). */
pli_status pli_batch_run_host(pli_ctx* ctx, int32_t nframes,
                              const uint8_t* left, const uint8_t* right,
                              int64_t stride, int64_t frame_stride,
                              uint32_t stages, void* table);

/* Pipelined host entry point (throughput with images in HOST memory): pli_batch_submit_host returns
 * after enqueueing the H2D copies (own copy stream), the kernels and the D2H copy of the table (second copy stream);
 * two submits may be in flight, so the copies of batch i+1 / i-1 overlap the kernels of batch i; a third submit first
 * waits for the oldest.  `left`, `right` and `table` should be pinned (pli_host_alloc, or memory the caller registered
 * with hipHostRegister) — pageable memory works but makes the copies synchronous.  pli_batch_wait(ctx, 0) waits for
 * the oldest outstanding submit (its table is then complete), pli_batch_wait(ctx, 1) for all of them.
 * Footprint: the first submit allocates, beside the context's own buffers, two device staging slots of max_frames frames each
 * (2 x width x height x max_frames bytes of images + max_frames table records per slot: 0.9 MB per frame at 752x480) and keeps
 * them until pli_ctx_destroy. */
pli_status pli_host_alloc(size_t bytes, void** out);
void       pli_host_free(void* p);
pli_status pli_batch_submit_host(pli_ctx* ctx, int32_t nframes,
                                 const uint8_t* left, const uint8_t* right,
                                 int64_t stride, int64_t frame_stride,
                                 uint32_t stages, void* table);
pli_status pli_batch_wait(pli_ctx* ctx, int32_t all);

/* ------------------------------------------------------------------------ */
/* Per-call drop-ins (host buffers, synchronous).                            */
/* ------------------------------------------------------------------------ */

/* The front-end of ONE Frame in one submission: what Frame::Frame (Frame.cc:128-163) does with four extractor calls on four
 * threads and two member calls — ExtractORB x2, ExtractLine x2, ComputeStereoMatches_Lines, ComputeStereoMatches — for a host
 * stereo pair.  `record` receives the frame's table record (pli_table_layout, record_bytes); the context is left as if
 * pli_orb_extract / pli_line_extract had run for both eyes (pli_last_counts, pli_orb_pyramid_level), and
 * pli_stereo_match_points / pli_stereo_match_lines hand out the matches of this submission without running again, until the next
 * per-call extraction.  The adapters funnel the four concurrent operator() calls of a Frame into one call of this
 * (orbslam_adapters.hpp: FrameFusion): 2.7 ms per Frame instead of 6.5 ms for the four calls one after the other. */
pli_status pli_frame_extract(pli_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t w, int32_t h,
                             int64_t stride_left, int64_t stride_right, void* record);

/* ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea)
 * ORBextractor.h:61-63 / ORBextractor.cc:1068-1150, with vLappingArea = {0,0}
 * as Frame::ExtractORB passes (Frame.cc:484-491).  `eye` selects which of the
 * two device-resident table sets (0 = left extractor, 1 = right extractor) is
 * filled; they feed pli_stereo_match_*.  Returns PLI_ERR_EMPTY_IMAGE for a
 * null/zero-sized image like the reference's -1. */
pli_status pli_orb_extract(pli_ctx* ctx, int32_t eye,
                           const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                           pli_keypoint* kp, int32_t cap, uint8_t* desc /* cap x 32 */,
                           int32_t* n);

/* ORBextractor::mvImagePyramid[level] (public member, ORBextractor.h:87) copied
 * to `dst` (w*h bytes, no border).  Valid after pli_orb_extract on that eye. */
pli_status pli_orb_pyramid_level(pli_ctx* ctx, int32_t eye, int32_t level,
                                 uint8_t* dst, int64_t dst_bytes, int32_t* w, int32_t* h);

/* Lineextractor::operator()(image, mask, keylines, descriptors_line)
 * LineExtractor.h:49-51 / LineExtractor.cc:31-70. */
pli_status pli_line_extract(pli_ctx* ctx, int32_t eye,
                            const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                            pli_keyline* kl, int32_t cap, uint8_t* desc /* cap x 32 */,
                            int32_t* n);

/* Diagnostics of the LSD relaxation schedule (lsd_mode 1 / 3; results never depend on it).  After the first call on a context
 * the relaxation rounds are launched WITHOUT a host look: as many as the slowest image of an earlier call needed plus a margin,
 * an image that is not at its fixed point after them is redone on the device by the sequential grower (exact, slow), and no
 * entry point drains the stream in the middle of a call.  (The tile relaxation needs no plan: its rounds from the third or fourth on
 * run in one persistent launch that ends when every image is at its fixed point.)  Synchronises the context.
 *   out[0] rounds the last call launched without looking; -1: the tile relaxation's persistent tail kernel ran the late rounds and
 *          stopped by itself at the fixed point (the default schedule of lsd_mode 3 / auto); 0: the host looked at the state
 *   out[1] rounds the slowest image of that call needed (-1: at least one image did not settle and took the slow path)
 *   out[2] images that took the slow path since the context was created
 *   out[3] the round count the next call plans from */
pli_status pli_lsd_round_stats(pli_ctx* ctx, int32_t out[4]);

/* Words of arena per scaled LSD pixel the context's relaxation got (region pixel lists and queue overflow blocks): 16 unless the
 * context is large or the device was short of free memory when it was created (then 3..15: results are unchanged, but batches of
 * long parallel structures may run out of it and take the slow device-side fallback, counted in pli_lsd_round_stats out[2]; the
 * library says so once on stderr); 0 for lsd_mode 2. */
pli_status pli_lsd_arena_words(pli_ctx* ctx, int32_t* words_per_pixel);

/* Self-test of the device the context runs on (not a reference function): the largest absolute error of the hardware cosine / sine
 * (v_cos_f32 / v_sin_f32 of angle / 360) against cos / sin of EVERY float angle in [0, 360] degrees.  Round 1 of the LSD tile
 * relaxation runs its vector filter on those (csrc/lsd_tile.hip "HOT RECORDS"); its error budget assumes 4e-6, and the GPU suite
 * asserts that this call reports less.  About a second of device time. */
pli_status pli_selftest_hot_trig(pli_ctx* ctx, double* max_abs_err);

/* Self-test of the LSD front pass (not a reference function): runs the three forms of the CV_64F front (csrc/lsd_f64.hip) on n
 * caller-supplied u8 images of w x h (rows of w bytes, images w * h bytes apart) at LSD scale `scale` (> 1) — the three separate kernels
 * (blur, resize, gradient), the tiled fused pass and the streaming fused pass — and compares what they write on the device.  The size
 * and the scale are the call's own (from 1 x 1 on), the context lends its device, rho and parity flags.  flags bit 0: the owner
 * words carry the unclaimed-norm word; bit 1: the forms write the 16-byte records and the owner plane (what the schedules off the hot
 * records take from the front pass) instead of the hot and cold planes.  out[0..3]: 4-byte words in which the streaming form differs
 * from the tiled one, per plane (hot, cold, norm, largest norm; with bit 1: records, owner plane, norm, largest norm); out[4..7]: the
 * same against the three kernels; out[8]: scaled rows per wave of the streaming form; out[9]: 1 if the streaming form applies to this
 * size — if not, out[0..3] are 0 and out[4..7] compare the tiled form, which the library then runs.  PLI_ERR_INVALID where no fused
 * form applies. */
pli_status pli_selftest_front_stream(pli_ctx* ctx, const uint8_t* imgs, int32_t n, int32_t w, int32_t h, double scale, int32_t flags,
                                     int32_t out[10]);

/* Self-test of the LSD front pass (not a reference function): runs ONE form of the CV_64F front (csrc/lsd_f64.hip) on n caller-supplied
 * u8 images — arguments, geometry and what the context lends as for pli_selftest_front_stream — and copies its planes to the host, for
 * tests that compare them with an independent computation.  form: 0 the three separate kernels, 1 the tiled fused pass, 2 the
 * streaming fused pass; PLI_ERR_INVALID where that form does not apply to the size or the blur radius (another form never stands in).
 * All planes have rows of dp = dw rounded up to a multiple of 16 pixels (dw = cvRound(w * scale), dh = cvRound(h * scale)), images
 * dp * dh pixels apart; `pixels` must be n * dp * dh.  flags bit 0: the owner words carry the unclaimed-norm word.  flags bit 1 clear:
 * plane_a = the hot records (8 bytes a pixel: the bits of the float angle in degrees, the owner word), plane_b = the cold plane
 * (two floats a pixel: cos, sin); bit 1 set: plane_a = the 16-byte records (angle, cos, sin, owner word as float bits), plane_b = the
 * owner plane (two int32 a pixel).  norm: the gradient norm, a double a pixel; max_bits[n]: per image the bits of the largest norm
 * above rho as a double, 0 where no pixel is above rho; scaled (form 0 only, may be null otherwise): the blurred and enlarged image,
 * rows of dw doubles, images dw * dh apart.  The device buffers are filled with the byte 0xA5 before the form runs: a word that it
 * does not write shows as 0xA5A5A5A5. */
pli_status pli_selftest_front_planes(pli_ctx* ctx, const uint8_t* imgs, int32_t n, int32_t w, int32_t h, double scale, int32_t form,
                                     int32_t flags, int64_t pixels, void* plane_a, void* plane_b, double* norm, uint64_t* max_bits,
                                     double* scaled);

/* The stereo rig of Frame::ComputeStereoMatches (Frame.cc:1005-1008: minZ = mb, maxD = mbf / minZ, depth = mbf / disparity):
 * replaces pli_frontend_config.bf / .fx of an existing context (the extractors' constructors, which create the context in
 * the adapters, do not know the camera; the Frame does: mbf and mK(0,0)).  A no-op when the values are the ones in use. */
pli_status pli_set_stereo_camera(pli_ctx* ctx, float bf, float fx);

/* Sizes of the tables the context holds from the last per-call extractions: counts[0], [1] = keypoints of eye 0 / 1
 * (mvKeys.size(), mvKeysRight.size()), counts[2], [3] = keylines of eye 0 / 1 (mvKeys_Line.size(),
 * mvKeysRight_Line.size()); -1 where that extractor has not run on this context.  The Frame-level stereo matchers of
 * the adapters check their vectors against these before they read the device tables (Frame.cc:976, :1156). */
pli_status pli_last_counts(pli_ctx* ctx, int32_t counts[4]);

/* Frame::ComputeStereoMatches() Frame.cc:976-1154 on the tables + pyramids left
 * on the device by the last pli_orb_extract(eye 0) / (eye 1).
 * uright/depth: N floats each (N = left keypoint count), -1 = no stereo. */
pli_status pli_stereo_match_points(pli_ctx* ctx, float* uright, float* depth, int32_t cap);

/* Frame::ComputeStereoMatches_Lines() Frame.cc:1156-1259 on the line tables of
 * the last pli_line_extract(eye 0) / (eye 1).
 * disp: N_l x 2 floats (mvDisparity_l, -1 = mono); le: N_l x 3 doubles (mvle_l). */
pli_status pli_stereo_match_lines(pli_ctx* ctx, float* disp, double* le, int32_t cap);

/* ORBmatcher::DescriptorDistance ORBmatcher.cc:2495-2511 / distance()
 * LineMatcher.cpp:231-247, batched: dist[i] = hamming(a[i], b[i]), 32-byte rows. */
pli_status pli_descriptor_distance(pli_ctx* ctx, const uint8_t* a, const uint8_t* b,
                                   int32_t n, int32_t* dist);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(k=2) as used by matchNNR
 * LineMatcher.cpp:139-159: per query the two smallest distances, ties to the
 * lower train index.  idx/dist: nq x 2 (idx -1 / dist INT32_MAX when nt < 2). */
pli_status pli_hamming_knn2(pli_ctx* ctx, const uint8_t* q, int32_t nq,
                            const uint8_t* t, int32_t nt, int32_t* idx, int32_t* dist);

/* int match(desc1, desc2, nnr, matches_12) LineMatcher.cpp:201-229 with
 * Config::bestLRMatches() = best_lr_matches of the context: ratio test both
 * ways + mutual check.  matches_12: n1 ints (-1 = none).  *nmatches = return value. */
pli_status pli_match_lines(pli_ctx* ctx, const uint8_t* desc1, int32_t n1,
                           const uint8_t* desc2, int32_t n2, float nnr,
                           int32_t* matches_12, int32_t* nmatches);

/* Core of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono, match12)
 * ORBmatcher.cc:2179-2323: the caller projects LastFrame's map points with the
 * predicted pose (SLAM state stays on the host) and passes, per query i in
 * LastFrame order: projected (u,v), search radius, octave window
 * [min_level,max_level] (max_level < 0 = unbounded as GetFeaturesInArea
 * Frame.cc:774-843), the map point descriptor and the predicted right
 * coordinate ur = u - bf*invz (compared with mvuRight[i2] whenever that is > 0,
 * :2259-2265).  Queries with valid == 0 (no map point / outlier / behind the
 * camera) are skipped.  The current frame is described by its keypoints, descriptors,
 * mvuRight and the image bounds used by the 64x48 grid (mnMinX..mnMaxY).
 * "Not available" is the reference's test :2255-2257 — CurrentFrame.mvpMapPoints[i2] is set AND has
 * Observations() > 0 — in both of its uses: cur_occupied[i2] != 0 (may be NULL) marks the keypoints that hold
 * such a map point BEFORE the call, and a match made in this call takes its keypoint away from the queries
 * behind it unless the query says its own map point has no observations (valid = 1 | PLI_PROJ_NO_OBSERVATIONS:
 * the temporal points Tracking::UpdateLastFrame creates in localisation mode; such a keypoint can be matched
 * again and the last writer holds it).  TH_HIGH = 100, the 30-bin rotation histogram and
 * ComputeThreeMaxima (:2449-2490) run on the device.
 * best_idx2[i] = matched current keypoint or -1 after the rotation filter; raw_idx2 (may be NULL) = the same
 * before it (a maintainer replays :2280-2282 from raw_idx2 in query order and :2315-2317 for the queries with
 * raw_idx2[i] >= 0 > best_idx2[i], as the adapter does).  *nmatches as the reference. */
#define PLI_PROJ_NO_OBSERVATIONS 2
typedef struct pli_proj_query {
  float u, v, radius, ur;
  int32_t min_level, max_level;
  float angle;          /* LastFrame.mvKeysUn[i].angle */
  int32_t valid;
} pli_proj_query;
pli_status pli_search_by_projection(pli_ctx* ctx,
                                    const pli_proj_query* q, const uint8_t* qdesc, int32_t nq,
                                    const pli_keypoint* cur_kp, const uint8_t* cur_desc,
                                    const float* cur_uright, const uint8_t* cur_occupied, int32_t ncur,
                                    float min_x, float max_x, float min_y, float max_y,
                                    int32_t check_orientation,
                                    int32_t* best_idx2, int32_t* raw_idx2, int32_t* nmatches);

/* --- Frame-to-frame track matching of a batch (BASELINE config 3), on the device tables of pli_batch_run ---
 * Frame i (i >= 1) of the batch against frame i-1, as Tracking::TrackWithMotionModel does per frame:
 *   points: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono, match12) ORBmatcher.cc:2179-2323, the last
 *           frame's stereo points (mvDepth > 0) standing for its map points as Tracking::UpdateLastFrame creates them
 *           (Frame::UnprojectStereo, Frame.cc:1334-1350);
 *   lines:  match(LastFrame.mDescriptors_Line, CurrentFrame.mDescriptors_Line, nnr, matches_12) LineMatcher.cpp:201-229
 *           (Tracking.cc:3058), left eye.
 * dev_poses: nframes x 12 floats on the device, mTcw (world -> camera, row major 3x4) of every frame — the motion-model
 * prediction for the current frame, the optimised pose for the last.  dev_track: nframes records of pli_track_layout
 * (record 0 is left untouched): counts = {nq = last N, point matches, n1 = last line count, line matches},
 * best_idx2[j] = current keypoint matched to last keypoint j or -1, matches_12[i] = current line of last line i or -1.
 * A last keypoint whose point lies in the current camera's plane (x3Dc.z == 0: invzc = +inf is not `< 0`) projects to +-inf, which
 * the image gate refuses, or to NaN, which it does not (ORBmatcher.cc:2225-2228 compare false); a NaN projection takes no
 * keypoint, because every distance test against it is false: best_idx2[j] = -1, as for the reference's loop.
 * Asynchronous on the context stream. */
typedef struct pli_track_params {
  float fx, fy, cx, cy, bf;          /* Camera.fx/fy/cx/cy/bf (EuRoC.yaml:9-28)                        */
  float th;                          /* search window: 15 stereo / 7 mono in TrackWithMotionModel       */
  float min_x, max_x, min_y, max_y;  /* mnMinX..mnMaxY of the frame grid                               */
  int32_t mono;                      /* bMono                                                          */
  int32_t check_orientation;         /* ORBmatcher::mbCheckOrientation                                 */
  float nnr_lines;                   /* minRatio12L                                                    */
  int32_t reserved;
} pli_track_params;
typedef struct pli_track_layout {
  int64_t record_bytes;
  int64_t off_counts;                /* int32[4]                                                       */
  int64_t off_best;                  /* int32[kp_cap]                                                  */
  int64_t off_lines;                 /* int32[kl_cap]                                                  */
  int32_t kp_cap, kl_cap;
} pli_track_layout;
pli_status pli_track_layout_get(const pli_ctx* ctx, pli_track_layout* out);
pli_status pli_batch_track(pli_ctx* ctx, int32_t nframes, const void* dev_table, const float* dev_poses,
                           const pli_track_params* params, void* dev_track);

/* --- the driver's rectification fused into the ingest ---
 * Replaces cv::remap(imLeft, imLeftRect, M1l, M2l, cv::INTER_LINEAR) / (imRight, ...) of
 * Examples/Stereo/stereo_euroc.cc:166-167 (maps from cv::initUndistortRectifyMap(..., CV_32F, M1, M2) :117-118).
 * mapx / mapy: width*height floats each (host), the CV_32FC1 maps of one eye; afterwards every image of that eye
 * handed to pli_batch_run / pli_batch_run_host / pli_orb_extract / pli_line_extract is the RAW image and level 0
 * of the pyramid is its rectification (bilinear, 1/32-px coordinates, constant-0 border, OpenCV 3.3.1 fixed point).
 * NULL, NULL removes the maps of that eye. */
pli_status pli_set_rectify_maps(pli_ctx* ctx, int32_t eye, const float* mapx, const float* mapy);

/* --- the head of Tracking::GrabImageStereo / GrabImageRGBD / GrabImageMonocular fused into the ingest ---
 * Replaces cvtColor(mImGray, mImGray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) of Tracking.cc:889-914 (both eyes,
 * the branch chosen by the left image), :964-977 and :1014-1027.  Afterwards every entry point that takes images —
 * pli_orb_extract, pli_orb_extract_lapping, pli_line_extract, pli_frame_extract, pli_frame_extract_single, pli_batch_run,
 * pli_batch_run_host, pli_batch_submit_host — reads them as interleaved 8-bit pixels of that format, 3 or 4 bytes each: w and h
 * stay in pixels, stride and frame_stride in bytes, a stride below w * channels is PLI_ERR_INVALID.  Level 0 of the pyramid
 * (pli_orb_pyramid_level) is the gray image and everything behind it is as before.  The gray value is OpenCV 3.3.1's C++ path
 * RGB2Gray<uchar>: (R*4899 + G*9617 + B*1868 + 8192) >> 14, alpha ignored (parity with a real OpenCV, whose IPP builds may differ,
 * is unpinned).  With rectification maps on an eye the COLOUR image is remapped, each channel on its own and rounded to 8 bits
 * (the driver's cv::remap, stereo_euroc.cc:166-167), and the three results are converted, as the reference orders the two.
 * One format for both eyes: the reference has no other.  The default is PLI_IMAGE_GRAY8, the library as it was.  Synchronises the
 * context and resizes its image staging; PLI_ERR_INVALID for an unknown format and while a batch of pli_batch_submit_host has
 * not been waited for.  (The pli_selftest_* calls bring geometry of their own and always read gray.) */
typedef enum { PLI_IMAGE_GRAY8 = 0, PLI_IMAGE_RGB8, PLI_IMAGE_BGR8, PLI_IMAGE_RGBA8, PLI_IMAGE_BGRA8 } pli_image_format;
pli_status pli_set_image_format(pli_ctx* ctx, pli_image_format fmt);

/* imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) of Tracking::GrabImageRGBD (Tracking.cc:979-980) at the keypoint instead of
 * over the frame.  Afterwards the `depth` argument of pli_stereo_from_depth and pli_frame_extract_single holds elements of `type`
 * and the value ComputeStereoFromRGBD sees at a keypoint is
 *   PLI_DEPTH_U16:  (float)raw * scale in float, one rounding (cvtScale16u32f with shift 0); 2 bytes per pixel go up
 *   PLI_DEPTH_F32:  d * scale in float; scale == 1.0f hands d's own bits through
 * The d > 0 gate and the in-image guard act on that value as before; no pass over the frame is made.  Whether a map needs a scale
 * at all (Tracking.cc:979: fabs(factor - 1) > 1e-5 || type != CV_32F) is the caller's decision (adapters/tracking_grab.hpp).
 * The default is PLI_DEPTH_F32, 1.0f.  PLI_ERR_INVALID for an unknown type or a scale that is not finite. */
typedef enum { PLI_DEPTH_F32 = 0, PLI_DEPTH_U16 } pli_depth_type;
pli_status pli_set_depth_format(pli_ctx* ctx, pli_depth_type type, float scale);

/* --- SURVEY.md §8(f) row 4 (RGB-D front-end): Frame::ComputeStereoFromRGBD(imDepth), Frame.cc:1309-1331 ---
 * depth: CV_32F depth image registered to the left image (already scaled by mDepthMapFactor, Tracking.cc), row
 * stride in floats.  For every left keypoint of the last pli_orb_extract(eye 0): d = depth(trunc(v), trunc(u));
 * d > 0 -> mvDepth = d, mvuRight = x - bf/d, else both -1 (the rectified pipeline: mvKeysUn == mvKeys).
 * Only the rows of the keypoints are written: uright and depth_out keep what they held from the keypoint count on.
 * After pli_set_depth_format(ctx, PLI_DEPTH_U16, scale) `depth` points at uint16_t (the declared const float* is cast) and
 * stride_floats counts those elements; d is then the raw element scaled as described there, for either type. */
pli_status pli_stereo_from_depth(pli_ctx* ctx, const float* depth, int64_t stride_floats, float* uright, float* depth_out,
                                 int32_t cap);

/* --- SURVEY.md §8(f) row 4 (fisheye stereo front-end, Frame.cc:1484-1576) ---
 * ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea) with a real lapping area
 * (ORBextractor.cc:1135-1144; Frame::ExtractORB passes mpCamera->mvLappingArea, Frame.cc:488,490): keypoints whose
 * level-0 x lies in [lap0, lap1] fill the table from the back in visiting order, all others from the front.
 * *n = keypoints, *n_mono = the reference's return value (index of the first lapping-area keypoint = monoLeft /
 * monoRight, Frame.cc:1521-1522).  The device table of that eye keeps this order for pli_stereo_fisheye. */
pli_status pli_orb_extract_lapping(pli_ctx* ctx, int32_t eye,
                                   const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                                   int32_t lap0, int32_t lap1,
                                   pli_keypoint* kp, int32_t cap, uint8_t* desc /* cap x 32 */,
                                   int32_t* n, int32_t* n_mono);

/* --- single-camera Frames of a DISTORTED pinhole camera: the monocular (Frame.cc:334-448) and RGB-D (:231-331) constructors with
 * Camera.k1 != 0 (TUM RGB-D, monocular EuRoC) ---
 * K and mDistCoef as the constructors hold them (float).  k3 = 0 stands for a 4-coefficient mDistCoef: the term k[4]*r2 is then
 * exactly 0, so one struct serves both. */
typedef struct pli_pinhole_distortion { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } pli_pinhole_distortion;

/* Stores the camera on the context (NULL removes it) and writes bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY} of
 * Frame::ComputeImageBounds (Frame.cc:947-974): the corners (0,0), (W,0), (0,H), (W,H) of the context's size through the same
 * device function as the keypoints, min / max of the pairs the reference takes (:962-965).  The reference's gate is kept literally
 * (:874-878, :909-913, :949, :967-973): with k1 == 0 — whatever the other coefficients — or without a camera nothing is
 * undistorted, bounds = {0, W, 0, H} and every "undistorted" output of the two calls below is a copy of its input.  bounds may be
 * NULL.  Synchronous. */
pli_status pli_set_pinhole_distortion(pli_ctx* ctx, const pli_pinhole_distortion* cam, float bounds[4]);

/* cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), K) as Frame::UndistortKeyPoints (Frame.cc:872-905) and
 * Frame::UndistortKeyLines (:907-945) call it, for n caller points (x, y) with the context's camera: OpenCV 3.3.1's five-step
 * iteration in double, no convergence test (csrc/frame_kernels.hip states it; parity with a real OpenCV is unpinned).
 * With `cell` (may be NULL): Frame::PosInGrid (:845-855) of each result against the context's bounds, as AssignFeaturesToGrid
 * (:451-482) uses it — posX * 48 + posY, or -1 where the reference returns false.  Stateless: works on the caller's tables and
 * leaves the context's Frame state alone.  n == 0 is valid. */
pli_status pli_undistort_points(pli_ctx* ctx, const float* xy /* n x 2 */, int32_t n, float* xy_un /* n x 2 */, int32_t* cell /* n */);

/* The front-end of ONE monocular or RGB-D Frame in one submission: what Frame::Frame (Frame.cc:334-448, :231-331) does with
 * ExtractORB(0, imGray, lap0, lap1) and ExtractLine(0, imGray) one after the other (:360-361, :258-259), UndistortKeyPoints
 * (:872-905), UndistortKeyLines (:907-945), ComputeStereoFromRGBD (:1309-1330; depth == NULL: monocular, mvuRight = mvDepth = -1,
 * :384-385) and the PosInGrid of AssignFeaturesToGrid (:451-482) — image and depth up, the ORB chain beside the line chain, the
 * lapping reorder (ORBextractor.cc:1135-1144; the monocular constructor passes {0, 1000}, the RGB-D one {0, 0}) and the rest on
 * the device, one synchronisation.  depth: CV_32F, registered to the image, row stride in floats; it is read at the
 * DISTORTED keypoint and mvuRight is written from the UNDISTORTED x, with the context's bf.  After
 * pli_set_depth_format(ctx, PLI_DEPTH_U16, scale) `depth` points at uint16_t (the declared const float* is cast),
 * depth_stride_floats counts those elements and the element read is scaled as described there.  `img` is read in the format of
 * pli_set_image_format, `stride` in bytes.
 * `record` receives the frame's table record (pli_table_layout, record_bytes) with its eye-0 columns filled: kp[0], desc[0], kl[0],
 * ldesc[0], uright, depth (every row: -1 from the keypoint count on), the counts and truncation flags; everything else in it is 0.
 * kp_un: kp_cap x 2 floats (mvKeysUn[i].pt), kl_un: kl_cap x 4 floats (mvKeysUn_Line[i]: startPointX, startPointY, endPointX,
 * endPointY), cell: kp_cap ints (as pli_undistort_points), rows from the counts on 0 / -1; *n_mono: the extractor's return value
 * (monoLeft).  The context is left as after pli_orb_extract_lapping(eye 0) plus pli_line_extract(eye 0): pli_last_counts,
 * pli_orb_pyramid_level, pli_stereo_from_depth work on this Frame; eye 1 counts as not extracted.  The record and the three
 * columns come back through one pinned buffer.  PLI_ERR_CAPACITY as those two calls. */
pli_status pli_frame_extract_single(pli_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, int64_t stride,
                                    int32_t lap0, int32_t lap1, const float* depth, int64_t depth_stride_floats,
                                    void* record, float* kp_un, float* kl_un, int32_t* cell, int32_t* n_mono);

/* KannalaBrandt8::mvParameters (include/CameraModels/KannalaBrandt8.h): fx, fy, cx, cy, k0..k3. */
typedef struct pli_kb8_camera { float fx, fy, cx, cy, k0, k1, k2, k3; } pli_kb8_camera;

/* Frame::ComputeStereoFishEyeMatches() Frame.cc:1577-1618 on the tables left on the device by the last
 * pli_orb_extract_lapping(eye 0) / (eye 1): BFMatcher(NORM_HAMMING).knnMatch(k = 2) of the lapping-area descriptors,
 * Lowe ratio 0.7, KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:334-402: parallax
 * cos <= 0.9998, SVD triangulation, positive depth in both cameras, reprojection error <= 5.991 mvLevelSigma2[octave]
 * in both), depth > 0.0001.  Rlr: 3x3 row major (mRlr), tlr: 3 (mtlr) = mTlr of Frame.cc:1539-1540.
 * l2r: mvLeftToRightMatch (Nleft ints, -1 = none), r2l: mvRightToLeftMatch (Nright), depth: mvDepth (Nleft, -1),
 * p3d: mvStereo3Dpoints (Nleft x 3 floats, camera-1 coordinates, zeros where unset); *nmatches = nMatches. */
pli_status pli_stereo_fisheye(pli_ctx* ctx, const pli_kb8_camera* cam1, const pli_kb8_camera* cam2,
                              const float* Rlr, const float* tlr,
                              int32_t* l2r, int32_t cap_left, int32_t* r2l, int32_t cap_right,
                              float* depth, float* p3d, int32_t* nmatches);

/* The same on caller tables: kp_left / desc_left = mvKeys / mDescriptors (Nleft rows, lapping-area keypoints from row
 * mono_left on), kp_right / desc_right = mvKeysRight / mDescriptorsRight; octaves index the context's mvLevelSigma2.
 * Every row of both tables must have 0 <= octave < orb_nlevels and finite x, y: otherwise PLI_ERR_INVALID, before anything is
 * launched; the output arrays are left untouched and *nmatches is 0. */
pli_status pli_stereo_fisheye_tables(pli_ctx* ctx, const pli_keypoint* kp_left, const uint8_t* desc_left, int32_t nleft,
                                     int32_t mono_left, const pli_keypoint* kp_right, const uint8_t* desc_right,
                                     int32_t nright, int32_t mono_right,
                                     const pli_kb8_camera* cam1, const pli_kb8_camera* cam2,
                                     const float* Rlr, const float* tlr,
                                     int32_t* l2r, int32_t* r2l, float* depth, float* p3d, int32_t* nmatches);

/* --- local-map tracking (Tracking::SearchLocalPointsAndLines, Tracking.cc:3854,3882) --- */

/* Core of ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, ...)
 * ORBmatcher.cc:44-143 (left / rectified-stereo branch, F.Nleft == -1).  Per map point in view the caller
 * passes (u,v) = mTrackProjX/Y, radius = r*mvScaleFactors[nPredictedLevel] (r from RadiusByViewingCos, times th),
 * ur = mTrackProjXR, min_level = nPredictedLevel-1, max_level = nPredictedLevel, valid = in view, not bad, not too far.
 * cur_occupied[i] != 0 marks current keypoints that already hold a map point with observations (may be NULL).
 * Best and second-best Hamming distance in GetFeaturesInArea order, TH_HIGH = 100, ratio test only when both are
 * on the same pyramid level (mfNNratio = nnratio); accepted keypoints become occupied for the following queries.
 * best_idx2[i] = matched keypoint or -1; *nmatches = return value. */
pli_status pli_search_local_map(pli_ctx* ctx, const pli_proj_query* q, const uint8_t* qdesc, int32_t nq,
                                const pli_keypoint* cur_kp, const uint8_t* cur_desc, const float* cur_uright,
                                const uint8_t* cur_occupied, int32_t ncur,
                                float min_x, float max_x, float min_y, float max_y, float nnratio,
                                int32_t* best_idx2, int32_t* nmatches);

/* The same function for a frame of two fisheye cameras (F.Nleft != -1), ORBmatcher.cc:44-214 in full.  Per map point i:
 * q_left[i] as above (valid = mbTrackInView etc.; no mvuRight gate in this branch), then — unless the left ratio test failed,
 * whose `continue` leaves the map point (:126) — q_right[i]: (u,v) = mTrackProjXR/YR, radius = RadiusByViewingCos(
 * mTrackViewCosR)*mvScaleFactors[mnTrackScaleLevelR] (no th, :148-151), levels mnTrackScaleLevelR-1..mnTrackScaleLevelR,
 * valid = mbTrackInViewR && mnTrackScaleLevelR != -1, searched in mGridRight / mvKeysRight.  F.mvpMapPoints is one array
 * of Nleft + Nright slots: occ_left / occ_right (may be NULL) mark the slots that hold a map point with observations,
 * left_to_right / right_to_left are mvLeftToRightMatch / mvRightToLeftMatch (-1 = none) — a match is also written to the
 * keypoint's stereo partner (:133-137, :201-205).  mp_left[k] / mp_right[k] = index of the map point this call left in the
 * slot, or -1; *nmatches = return value.  nleft + nright <= 15360. */
pli_status pli_search_local_map_fisheye(pli_ctx* ctx, const pli_proj_query* q_left, const pli_proj_query* q_right,
                                        const uint8_t* qdesc, int32_t nq,
                                        const pli_keypoint* kp_left, const uint8_t* desc_left, const uint8_t* occ_left,
                                        const int32_t* left_to_right, int32_t nleft,
                                        const pli_keypoint* kp_right, const uint8_t* desc_right, const uint8_t* occ_right,
                                        const int32_t* right_to_left, int32_t nright,
                                        float min_x, float max_x, float min_y, float max_y, float nnratio,
                                        int32_t* mp_left, int32_t* mp_right, int32_t* nmatches);

/* --- Frame-to-frame tracking of a two-camera frame (Tracking::TrackWithMotionModel, Tracking.cc:2961,2969) ---
 * Core of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) ORBmatcher.cc:1961-2177 for a current frame of two
 * cameras (CurrentFrame.Nleft != -1), whose mvpMapPoints has Nleft + Nright slots.  The caller projects, as for
 * pli_search_by_projection.  Per LastFrame row i, in order:
 *   q_left[i]:  everything as for pli_search_by_projection — (u,v) = mpCamera->project(x3Dc), radius = th*mvScaleFactors[nLastOctave],
 *               the octave window, angle = the last frame's keypoint angle (mvKeys / mvKeysRight by i < LastFrame.Nleft), valid =
 *               0 (no map point / outlier / invzc < 0), 1, or 1 | PLI_PROJ_NO_OBSERVATIONS.  The image gate :2004-2007 and
 *               GetFeaturesInArea on mGrid / mvKeys (kp_left) apply; this branch has no mvuRight gate (:2040).
 *   q_right[i]: only u, v, radius, min_level and max_level are read — (u,v) = mpCamera->project(Trl*x3Dc) (:2084-2086), the same
 *               radius and window; valid and angle are those of q_left[i]; `ur` is read on neither side.  No image gate and no
 *               invz test (:2086); GetFeaturesInArea on mGridRight / mvKeysRight (kp_right).
 * The right camera of row i is searched only if the left projection passed the image gate AND the left GetFeaturesInArea
 * returned at least one keypoint (the `continue`s of :2004-2007 and :2024 leave both cameras) — judged on the window and the level
 * gate alone, before availability and before any distance: a left window whose keypoints are all taken, or all farther than TH_HIGH,
 * does not close the right camera.
 * occ_left[k] / occ_right[k] != 0 (may be NULL): slot k / Nleft + k holds a map point with Observations() > 0 before the call; a
 * match takes its keypoint away from the rows behind it on that camera unless valid has PLI_PROJ_NO_OBSERVATIONS, on both
 * cameras.  One 30-bin rotation histogram and one ComputeThreeMaxima for both cameras (:2154-2174).
 * best_left[i] / best_right[i] = the keypoint of that camera (index within the camera) row i holds after the rotation filter, or
 * -1; raw_left / raw_right (may be NULL) = the same before it: a maintainer replays :2061 / :2128 from them in row order, left
 * then right, and :2169 for the entries with raw >= 0 > best.  *nmatches = the reference's return value.
 * A NaN projection takes no keypoint (every distance test against it is false) and, on the left, leaves the right camera
 * unsearched as an empty window does; an infinite right projection falls outside the grid and takes none either.
 * nleft + nright <= 15360: more is PLI_ERR_CAPACITY, nothing is truncated.  nq, nleft and nright may be 0. */
pli_status pli_search_by_projection_two_cameras(pli_ctx* ctx,
                                                const pli_proj_query* q_left, const pli_proj_query* q_right, const uint8_t* qdesc, int32_t nq,
                                                const pli_keypoint* kp_left, const uint8_t* desc_left, const uint8_t* occ_left, int32_t nleft,
                                                const pli_keypoint* kp_right, const uint8_t* desc_right, const uint8_t* occ_right, int32_t nright,
                                                float min_x, float max_x, float min_y, float max_y, int32_t check_orientation,
                                                int32_t* best_left, int32_t* best_right, int32_t* raw_left, int32_t* raw_right,
                                                int32_t* nmatches);

/* int match(const vector<MapLine*>&, Frame&, nnr, matches_12) LineMatcher.cpp:161-171: one-directional matchNNR
 * of the local map lines' descriptors against the frame's (the reference returns before its mutual check). */
pli_status pli_match_nnr(pli_ctx* ctx, const uint8_t* desc1, int32_t n1, const uint8_t* desc2, int32_t n2, float nnr,
                         int32_t* matches_12, int32_t* nmatches);

/* --- bag-of-words of a frame (Frame::ComputeBoW, Frame.cc:858-870) ---
 * DBoW2::TemplatedVocabulary<cv::Mat, FORB> (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h): a k-ary tree of 256-bit
 * descriptors.  pli_vocab_create takes the node list exactly as loadFromTextFile (:1350-1433) reads it from
 * ORBvoc.txt: node i+1 of the file (node 0 is the root) has parent[i], its 32 descriptor bytes, its weight and its
 * "is a word" flag; children keep file order; word ids are assigned to flagged nodes in file order. */
typedef struct pli_vocab pli_vocab;
pli_status pli_vocab_create(pli_ctx* ctx, int32_t k, int32_t L, int32_t nnodes, const int32_t* parent,
                            const uint8_t* is_leaf, const uint8_t* desc, const double* weight, pli_vocab** out);
void pli_vocab_destroy(pli_vocab* v);

/* The per-feature part of transform(features, BowVector&, FeatureVector&, levelsup) (:1139-1208): the descent
 * transform(feature, id, weight, &nid, levelsup) (:1230-1272) of every descriptor — at each level the child with the
 * smallest Hamming distance, the first one on ties — giving word_id[i], weight[i] (the word's idf weight; 0 =
 * stopped word) and node_id[i] (the ancestor at level L - levelsup, 0 if that is the root).  The accumulation into
 * the two std::maps and the L1 normalisation are done by the caller in feature order (adapters/pli_cpp.hpp does it
 * with the reference's own arithmetic). */
pli_status pli_bow_transform(pli_ctx* ctx, const pli_vocab* vocab, const uint8_t* desc, int32_t n, int32_t levelsup,
                             int32_t* word_id, double* weight, int32_t* node_id);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) ORBmatcher.cc:269-470, F.Nleft == -1 branch (rectified stereo,
 * RGB-D, mono pinhole), for nkf keyframes against one frame in one call (Tracking::Relocalization's loop, Tracking.cc:4205-4230).
 * Keyframe k owns rows kf_off[k] .. kf_off[k+1]-1 of kf_desc / kf_angle / kf_node / kf_valid; kf_off[0] = 0, non-decreasing.
 * *_node[i] = the FeatureVector node that lists feature i, -1 = listed in none (stopped word): pli_bow_transform's node_id where
 * weight > 0.  kf_valid[i] != 0: the keyframe's map point i is set and not isBad().  kf_angle = pKF->mvKeysUn[i].angle,
 * f_angle = F.mvKeys[i].angle; with check_orientation every angle must lie in [0, 360) (the angles are not read without it and
 * may then be NULL).  matches: nkf x nf, the keyframe feature (row within its keyframe) that frame feature i is matched to, or
 * -1, after the rotation filter; nmatches[k] = the reference's return value.  TH_LOW = 50.
 * Caps: nf and every keyframe's feature count <= PLI_BOW_MAX_FEATURES (else PLI_ERR_CAPACITY, nothing is truncated); nkf is
 * bounded by device memory only.  nkf == 0 and nf == 0 are valid (no matches). */
#define PLI_BOW_MAX_FEATURES 8192
pli_status pli_search_by_bow(pli_ctx* ctx, int32_t nkf, const int32_t* kf_off, const uint8_t* kf_desc, const float* kf_angle,
                             const int32_t* kf_node, const uint8_t* kf_valid, const uint8_t* f_desc, const float* f_angle,
                             const int32_t* f_node, int32_t nf, float nnratio, int32_t check_orientation, int32_t* matches,
                             int32_t* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) ORBmatcher.cc:269-470, the branch F.Nleft != -1 (:342-369,
 * :403-432; a rig of two KannalaBrandt8 cameras: Tracking::TrackReferenceKeyFrame, Tracking.cc:2648 / :2708, and
 * Relocalization, :4215), batched over keyframes like pli_search_by_bow.  Tables as there, plus f_nleft = F.Nleft: the frame's
 * nf = F.N rows are the left camera's first.  The caller chooses the angles: kf_angle is mvKeysUn when !pKF->mpCamera2, else
 * mvKeys / mvKeysRight by NLeft (:379-382); f_angle is F.mvKeys / F.mvKeysRight by Nleft (:386-389, :416-419).
 * Per keyframe feature, over the still-unmatched frame features of its node in list order (:343-369): bestDist1 / bestDist2 /
 * bestIdxF run over the candidates < f_nleft, bestDist1R / bestDist2R / bestIdxFR over the candidates >= f_nleft, both with
 * strict <.  Then the reference's nesting as written (:373-433): only if bestDist1 <= TH_LOW, the left match is taken when
 * (float)bestDist1 < mfNNratio * (float)bestDist2, and - whether or not it was - the right match when bestDist1R <= TH_LOW,
 * without a ratio test (`|| true`, :405).  A right candidate of a keyframe feature that has no left candidate within TH_LOW is
 * never taken.  Each taken match closes its frame feature to the later keyframe features, counts in nmatches and, with
 * check_orientation, enters the rotation histogram with its own frame angle; ComputeThreeMaxima and the filter follow as in
 * pli_search_by_bow.  matches / nmatches, caps and errors as there; f_nleft outside [0, nf] is PLI_ERR_INVALID.  With
 * f_nleft == nf the result is pli_search_by_bow's; with f_nleft == 0 nothing is matched. */
pli_status pli_search_by_bow_two_cameras(pli_ctx* ctx, int32_t nkf, const int32_t* kf_off, const uint8_t* kf_desc,
                                         const float* kf_angle, const int32_t* kf_node, const uint8_t* kf_valid,
                                         const uint8_t* f_desc, const float* f_angle, const int32_t* f_node, int32_t nf,
                                         int32_t f_nleft, float nnratio, int32_t check_orientation, int32_t* matches,
                                         int32_t* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) ORBmatcher.cc:823-963 (NLeft == -1 on both sides: the
 * two-camera guards :858, :878 are not provided), for one keyframe pKF1 against nkf keyframes pKF2[k] in one call
 * (LoopClosing::DetectCommonRegionsFromBoW's loop, LoopClosing.cc:528-540).
 * desc1 / angle1 / node1 / valid1: n1 rows of pKF1 - mDescriptors, mvKeysUn[i].angle, the FeatureVector node that lists the
 * feature (-1 = none, as for pli_search_by_bow), GetMapPointMatches()[i] set and not isBad().  Keyframe k owns rows
 * kf_off[k] .. kf_off[k+1]-1 of kf_desc / kf_angle / kf_node / kf_valid (the same four of pKF2[k]); kf_off[0] = 0, non-decreasing.
 * pKF1's features are walked in the reference's order (nodes ascending, a node's list ascending); a feature of pKF2[k] taken by an
 * accepted match (vbMatched2) is no candidate for the later ones.  The distance test is strict: bestDist1 < TH_LOW = 50.  With
 * check_orientation every angle must lie in [0, 360) (the angles are not read without it and may then be NULL).
 * matches12: nkf x n1, the row within keyframe k that feature i of pKF1 is matched to, or -1, after the rotation filter
 * (vpMatches12 as indices); nmatches[k] = the reference's return value.
 * Caps: n1 and every keyframe's feature count <= PLI_BOW_MAX_FEATURES (else PLI_ERR_CAPACITY, nothing is truncated); nkf is
 * bounded by device memory only.  nkf == 0, n1 == 0 and empty keyframes are valid (no matches). */
pli_status pli_search_by_bow_kf(pli_ctx* ctx, const uint8_t* desc1, const float* angle1, const int32_t* node1,
                                const uint8_t* valid1, int32_t n1, int32_t nkf, const int32_t* kf_off, const uint8_t* kf_desc,
                                const float* kf_angle, const int32_t* kf_node, const uint8_t* kf_valid, float nnratio,
                                int32_t check_orientation, int32_t* matches12, int32_t* nmatches);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) ORBmatcher.cc:965-1206, the branch
 * without second cameras (mpCamera2 == nullptr on both sides, NLeft == -1, keypoints = mvKeysUn), for one keyframe pKF1 against
 * nkf neighbours pKF2[k] in one call (LocalMapping::CreateNewMapPoints' loop, LocalMapping.cc:343-423; Tracking.cc:4705).
 * kp1 / desc1 / node1 / has_mp1 / stereo1: n1 rows of pKF1 - mvKeysUn (pt, octave, angle are read), mDescriptors, the
 * FeatureVector node that lists the feature (-1 = none, as for pli_search_by_bow), GetMapPoint(i) != nullptr (isBad() is not
 * asked), mvuRight[i] >= 0.  Neighbour k owns rows kf_off[k] .. kf_off[k+1]-1 of the five kf_* tables; kf_off[0] = 0,
 * non-decreasing.  F12: nkf x 9 floats, row major, the matrix Pinhole::epipolarConstrain forms from R12, t12 and the two K
 * (Pinhole.cpp:124-127; the F12 argument of the reference's overload is not read by it); ep: nkf x 2, the epipole
 * pKF2->mpCamera->project(R2w * Cw + t2w) (:972-977).  Both are host arithmetic (PliORBmatcher computes them); the device
 * evaluates Pinhole.cpp:130-143 (float, the comparison dsqr < 3.84 * unc in double) and the epipole gate :1089-1097 on them.
 * mvScaleFactors / mvLevelSigma2 are the context's (every keyframe comes from the same extractor): octaves index them and must
 * lie in [0, orb_nlevels).  coarse = bCoarse: the epipolar expression does not decide, the other gates do.  With
 * check_orientation (mbCheckOrientation) every angle must lie in [0, 360).
 * matches12: nkf x n1, vMatches12 after the rotation filter (the row of pKF2[k] that feature i of pKF1 is matched to, -1 = none;
 * vMatchedPairs is the row read in index order); nmatches[k] = the reference's return value.  A feature of pKF2 may be matched
 * by several features of pKF1 (vbMatched2 is never set in the reference); of equally distant candidates the last listed wins.
 * Caps: n1 and every neighbour's feature count <= PLI_BOW_MAX_FEATURES (else PLI_ERR_CAPACITY, nothing is truncated); nkf is
 * bounded by device memory only.  nkf == 0 and empty tables are valid (no matches). */
pli_status pli_search_for_triangulation(pli_ctx* ctx, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                        const uint8_t* has_mp1, const uint8_t* stereo1, int32_t n1, int32_t nkf,
                                        const int32_t* kf_off, const pli_keypoint* kf_kp, const uint8_t* kf_desc,
                                        const int32_t* kf_node, const uint8_t* kf_has_mp, const uint8_t* kf_stereo,
                                        const float* F12, const float* ep, int32_t only_stereo, int32_t coarse,
                                        int32_t check_orientation, int32_t* matches12, int32_t* nmatches);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) ORBmatcher.cc:965-1206, the branch
 * pKF1->mpCamera2 && pKF2->mpCamera2 (a rig of two KannalaBrandt8 cameras, NLeft != -1), for one keyframe pKF1 against nkf
 * neighbours pKF2[k] in one call.  A keyframe has N = NLeft + NRight features, the left camera's first: kp1 / desc1 / node1 /
 * has_mp1 are n1 = N rows of pKF1 - mvKeys[i] for i < n1_left = NLeft, else mvKeysRight[i - NLeft] (:1048-1053; pt, octave, angle
 * are read; NOT mvKeysUn), mDescriptors, the FeatureVector node that lists the feature (-1 = none), GetMapPoint(i) != nullptr.
 * Neighbour k owns rows kf_off[k] .. kf_off[k+1]-1 of the four kf_* tables, laid out the same way with kf_nleft[k] = its NLeft.
 * cam_left / cam_right: mpCamera / mpCamera2, shared by every keyframe of the call as the level tables are.  rel: nkf x 4 x 12
 * floats, per neighbour the relative poses ll, lr, rl, rr of :995-1003 (host arithmetic), each R12 row major then t12; for a
 * candidate pair (bRight1, bRight2) = (idx1 >= NLeft1, idx2 >= NLeft2) picks the pose and the two cameras (:1099-1129) and the
 * gate is KannalaBrandt8::epipolarConstrain = TriangulateMatches(...) > 0.0001f (KannalaBrandt8.cpp:235-238, 334-403) with
 * mvLevelSigma2 of the two octaves, evaluated on the device with the cv::Mat conventions of pli_stereo_fisheye.  There are no
 * stereo tables, no F12 and no epipole: bStereo1 / bStereo2 are false whenever mpCamera2 is set (:1041, :1070) and the epipole
 * gate is skipped (:1089).  For the same reason only_stereo != 0 matches nothing (:1043-1045 skips every feature of pKF1): every
 * row is -1, every count 0, and nothing is launched.  coarse = bCoarse: the triangulation does not decide.  With
 * check_orientation every angle must lie in [0, 360).
 * matches12: nkf x n1, vMatches12 after the rotation filter, indices over the neighbour's N; nmatches[k] = the reference's return
 * value.  Of equally distant candidates the last listed wins, as for pli_search_for_triangulation.
 * Checked before anything is launched, PLI_ERR_INVALID: null pointers, n1_left outside [0, n1], kf_nleft[k] outside [0, n_k], a
 * decreasing kf_off, an octave outside [0, orb_nlevels), a keypoint coordinate that is not finite, a value of rel that is not
 * finite, with check_orientation an angle outside [0, 360).  PLI_ERR_CAPACITY for more than PLI_BOW_MAX_FEATURES rows in n1 or
 * in a neighbour (nothing is truncated).  nkf == 0, n1 == 0, empty neighbours, n1_left == 0 and n1_left == n1 are valid.  The
 * number of kernel launches does not depend on nkf. */
pli_status pli_search_for_triangulation_two_cameras(pli_ctx* ctx, const pli_keypoint* kp1, const uint8_t* desc1,
                                                    const int32_t* node1, const uint8_t* has_mp1, int32_t n1, int32_t n1_left,
                                                    int32_t nkf, const int32_t* kf_off, const int32_t* kf_nleft,
                                                    const pli_keypoint* kf_kp, const uint8_t* kf_desc, const int32_t* kf_node,
                                                    const uint8_t* kf_has_mp, const pli_kb8_camera* cam_left,
                                                    const pli_kb8_camera* cam_right, const float* rel, int32_t only_stereo,
                                                    int32_t coarse, int32_t check_orientation, int32_t* matches12,
                                                    int32_t* nmatches);

/* The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) ORBmatcher.cc:1399-1609 (the branch bRight == false,
 * NLeft == -1, keypoints = mvKeysUn) and of the Sim3 overload Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :1611-1733, for nmp map
 * points against nkf keyframes in one call (LocalMapping::SearchInNeighbors, LocalMapping.cc:743-749 and :776;
 * LoopClosing::SearchAndFuse, LoopClosing.cc:2097-2165).  The projection runs on the device, with the cv::Mat conventions of the
 * reference's expressions (a matrix product: double accumulation, one rounding; cv::norm and Mat::dot in double; the rest float,
 * in the written order, nothing fused).  What follows the search in the reference (Replace / AddObservation / AddMapPoint
 * :1572-1594, and the gates isBad() and IsInKeyFrame at the time a point's turn comes) is sequential and stays with the caller:
 * PliORBmatcher::Fuse replays it. */
typedef struct pli_fuse_point {   /* 40 bytes */
  float pos[3];        /* GetWorldPos() :1435 */
  float normal[3];     /* GetNormal() :1490 */
  float min_dist_inv;  /* GetMinDistanceInvariance() :1478 */
  float max_dist_inv;  /* GetMaxDistanceInvariance() :1477 */
  float max_dist;      /* mfMaxDistance, read by PredictScale (MapPoint.cc:449-464); finite and > 0 where valid */
  int32_t valid;       /* 0 = skip for every keyframe (!pMP :1424, isBad() :1432); also a point whose max_dist is not finite
                          and positive (the reference converts a NaN to int there) */
} pli_fuse_point;

typedef struct pli_fuse_camera {
  float fx, fy, cx, cy; /* pKF->fx .. cy :1419-1422 (Pinhole::project, Pinhole.cpp:30-33) */
  float bf;             /* pKF->mbf :1423 */
  float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY: KeyFrame::IsInImage (KeyFrame.cc:927-930) and the 64 x 48 grid */
} pli_fuse_camera;

/* mp / mp_desc: nmp points and their GetDescriptor() rows (32 bytes each).  Keyframe k owns rows kf_off[k] .. kf_off[k+1]-1 of
 * kf_kp (mvKeysUn: pt and octave are read), kf_desc (mDescriptors) and kf_uright (mvuRight; read only with reproj_gate, may be
 * NULL without); kf_off[0] = 0, non-decreasing.  kf_pose: nkf x 15 floats - Rcw row major (GetRotation()), tcw
 * (GetTranslation()), Ow (GetCameraCenter(): the stored value, not recomputed).  skip: nkf x nmp, may be NULL; != 0 leaves the
 * pair out (IsInKeyFrame(pKF) :1437, spAlreadyFound.count(pMP) :1639).  cam: every keyframe of a call shares it, as every
 * keyframe shares the context's mvScaleFactors / mvInvLevelSigma2 (octaves index them and must lie in [0, orb_nlevels)).
 * th: the radius is th * mvScaleFactors[level] :1502.
 * level_ratio: orb_nlevels - 1 floats, non-decreasing.  MapPoint::PredictScale's ceil(log(ratio) / mfLogScaleFactor) leaves the
 * overload of log(float) to the integrator's toolchain, and a device logarithm is not the host's; so the host supplies, for
 * n = 0 .. orb_nlevels-2, the largest float ratio for which ITS expression (with its clamps) gives a level <= n (found by
 * bisection over float bit patterns; pli_cpp.hpp fuseLevelRatio), and the device's level is the number of n with
 * ratio > level_ratio[n].
 * reproj_gate != 0: the chi-square gate :1533-1557 (7.8 where kf_uright >= 0, 5.99 otherwise) of the first overload; 0: the Sim3
 * overload, which has none.
 * best_idx: nkf x nmp, bestIdx where bestDist <= TH_LOW (50), else -1: the row within the keyframe; the strict minimum in the
 * visiting order of KeyFrame::GetFeaturesInArea (KeyFrame.cc:881-925).  best_dist (may be NULL): bestDist, 256 where no candidate
 * passed the gates.
 * Errors: PLI_ERR_INVALID for null pointers, an octave outside [0, orb_nlevels), a decreasing kf_off, a decreasing or NaN
 * level_ratio; PLI_ERR_CAPACITY for a keyframe with more than PLI_BOW_MAX_FEATURES rows (nothing is truncated).  nmp and nkf are
 * bounded by device memory only; nkf == 0, nmp == 0 and empty keyframes are valid.  The number of kernel launches does not depend
 * on nkf or nmp. */
pli_status pli_fuse_search(pli_ctx* ctx, const pli_fuse_point* mp, const uint8_t* mp_desc, int32_t nmp, int32_t nkf,
                           const int32_t* kf_off, const pli_keypoint* kf_kp, const uint8_t* kf_desc, const float* kf_uright,
                           const float* kf_pose, const uint8_t* skip, const pli_fuse_camera* cam, float th,
                           const float* level_ratio, int32_t reproj_gate, int32_t* best_idx, int32_t* best_dist);

/* The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) ORBmatcher.cc:1399-1609 for keyframes with two KannalaBrandt8
 * cameras (NLeft != -1, mpCamera2 set): both values of bRight, for nmp map points against nkf keyframes, in one call
 * (LocalMapping::SearchInNeighbors calls Fuse twice per target keyframe, LocalMapping.cc:747-748, and twice for the current one,
 * :776-777).  mp, mp_desc, th, level_ratio and the cap of PLI_BOW_MAX_FEATURES rows per keyframe as for pli_fuse_search.
 * Keyframe tables as for pli_search_for_triangulation_two_cameras: keyframe k owns rows kf_off[k] .. kf_off[k+1]-1 of kf_kp and
 * kf_desc (mDescriptors), the first kf_nleft[k] of them mvKeys, the rest mvKeysRight (:1524-1526, KeyFrame.cc:912-914; pt and
 * octave are read; NOT mvKeysUn).  kf_pose: nkf x 2 x 15 floats, left then right, each Rcw row major, tcw, Ow: GetRotation() /
 * GetTranslation() / GetCameraCenter(), and GetRightRotation() / GetRightTranslation() / GetRightCameraCenter()
 * (KeyFrame.cc:1343-1373) - the reference's own cv::Mat expressions, host arithmetic, as rel is for the triangulation call.
 * cam_left / cam_right: mpCamera / mpCamera2, shared by the call.  min_x .. max_y: mnMinX .. mnMaxY, for KeyFrame::IsInImage and
 * the 64 x 48 grids; pKF->fx .. cy and mbf are not read by this branch.  sides: bit 0 = the left camera (bRight == false), bit 1 =
 * the right; a side that is not asked for is neither projected nor searched and its rows of the result are -1 / 256.
 * skip: nkf x 2 x nmp, may be NULL (IsInKeyFrame(pKF) :1448 at the time of that side's call).
 * Per (keyframe, side, point), in the reference's order: valid / skip; p3Dc = Rcw*p3Dw + tcw with that side's pose (a cv::Mat
 * product: double accumulation, one rounding); z < 0 rejected (:1459); uv = KannalaBrandt8::project with that side's camera
 * (KannalaBrandt8.cpp:28-42, with the conventions of pli_stereo_fisheye); IsInImage; the distance range with that side's Ow;
 * PO.dot(Pn) < 0.5*dist3D; the level from level_ratio; radius = th * mvScaleFactors[level]; the window
 * GetFeaturesInArea(uv.x, uv.y, radius, bRight) over that side's own grid (mGrid from the left rows, mGridRight from the right
 * rows with camera-local indices, Frame.cc:468-481); the octave in [level-1, level]; e2 * mvInvLevelSigma2[octave] > 5.99
 * rejected; the strict minimum of the Hamming distance in visiting order = the minimum of the key (distance, cell column, cell
 * row, index), as for pli_fuse_search; bestDist <= TH_LOW.
 * There is no kf_uright and no 7.8 bound: the fisheye constructor sets every mvuRight to -1 (Frame.cc:1589), and the reference
 * reads mvuRight[idx] with the camera-local idx on a vector of Nleft entries, which is an out-of-range read for a right row
 * >= Nleft.  An adapter must refuse a keyframe with NLeft != -1 and any mvuRight[i] >= 0.
 * best_idx: nkf x 2 x nmp, the reference's bestIdx, a row over the keyframe's N (for the right camera the camera-local row +
 * NLeft, :1559), -1 where there is no match.  best_dist (may be NULL): bestDist, 256 where no candidate passed the gates.
 * Checked before anything is launched, PLI_ERR_INVALID: null pointers, sides outside 1..3, a decreasing or NaN level_ratio, empty
 * image bounds, a decreasing kf_off, kf_nleft[k] outside [0, n_k], an octave outside [0, orb_nlevels), a keypoint coordinate or a
 * pose value that is not finite.  PLI_ERR_CAPACITY for a keyframe with more than PLI_BOW_MAX_FEATURES rows.  nkf == 0, nmp == 0,
 * empty keyframes, kf_nleft[k] == 0 and kf_nleft[k] == n_k are valid.  Three kernel launches, whatever nkf and nmp. */
pli_status pli_fuse_search_two_cameras(pli_ctx* ctx, const pli_fuse_point* mp, const uint8_t* mp_desc, int32_t nmp, int32_t nkf,
                                       const int32_t* kf_off, const int32_t* kf_nleft, const pli_keypoint* kf_kp,
                                       const uint8_t* kf_desc, const float* kf_pose, const uint8_t* skip,
                                       const pli_kb8_camera* cam_left, const pli_kb8_camera* cam_right, float min_x, float max_x,
                                       float min_y, float max_y, float th, const float* level_ratio, int32_t sides,
                                       int32_t* best_idx, int32_t* best_dist);

/* LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684), for keyframes of one pinhole camera (NLeft == -1,
 * no mpCamera2: monocular, rectified stereo, RGB-D), one keyframe against nkf neighbours in one call: SearchForTriangulation
 * (bOnlyStereo = false as at :423, mbCheckOrientation = false as the matcher of :367 is built), then per matched pair the
 * unprojection, the ray and stereo parallax, the linear triangulation through cv::SVD::compute or KeyFrame::UnprojectStereo, the
 * depths, both chi-square gates, the far-point gate and the scale consistency (:530-667), on the device with the cv::Mat
 * conventions of pli_fuse_search and pli_stereo_fisheye.
 * The reference's loop is sequential along the neighbours: a feature of pKF1 that received a map point from neighbour k
 * (AddMapPoint :675) is skipped by the search of every later neighbour (ORBmatcher.cc:1033-1039).  That is its only coupling (no
 * rotation histogram, vbMatched2 is never set, the neighbours are distinct keyframes), so the call evaluates every (neighbour,
 * feature) pair on the map-point state at entry and then, per feature, keeps the FIRST neighbour in which it is matched and passes
 * every gate; in every later neighbour it is unmatched.  The results are the sequential loop's exactly.
 * What stays with the caller: the baseline / median-depth test :396-413 (only neighbours that pass it are sent), F12 and ep as
 * for pli_search_for_triangulation, and :670-683 (new MapPoint, AddObservation, AddMapPoint, ...), which
 * PliCreateNewMapPoints (adapters/orbslam_local_mapping.hpp) replays in the reference's order.
 * Tables: kp1 / desc1 / node1 / has_mp1 and the kf_* ones as for pli_search_for_triangulation.  Per feature of either side also
 * uright = mvuRight (the stereo flag is mvuRight >= 0), depth = mvDepth, key = mvKeys[i].pt as two floats, which
 * KeyFrame::UnprojectStereo reads (KeyFrame.cc:937-938; NOT mvKeysUn, which everything else reads).  pose1 / kf_pose: 15 floats per
 * keyframe as for pli_fuse_search - Rcw row major, tcw, the stored Ow; Rwc is the exact transpose and Twc's blocks are that
 * transpose and Ow (KeyFrame::SetPose).  cam: fx, fy, cx, cy and bf = mbf are read, shared by the call: fx1..cy1 and fx2..cy2 of
 * the reference are the same numbers here, and mpCurrentKeyFrame->mbf serves the second keyframe's stereo gate too (:641).  mb is
 * read by the stereo parallax (:543, :545; the second one only when the first side is not stereo, `else if` at :544).
 * far_points / th_far: mbFarPoints / mThFarPoints (:660, dist >= th_far rejects).  ratio_factor: 1.5f * mfScaleFactor, computed by
 * the caller in float (:384).  coarse: bCoarse (:420-422).
 * Outputs, nkf x n1 unless said: matches12 = what the reference's loop sees at neighbour k (a feature taken by an earlier neighbour
 * is -1); nmatches[nkf] = the size of that vMatchedIndices; status = one of the codes below per pair; x3d (nkf x n1 x 3) = x3D,
 * defined where status == PLI_NEWPT_CREATED; nnew[nkf] = the map points created per neighbour.  Two features of pKF1 may be
 * matched to the same feature of a neighbour and both be created, as in the reference.
 * Checked before anything is launched, PLI_ERR_INVALID: null pointers, negative counts, a decreasing kf_off, an octave outside
 * [0, orb_nlevels), a keypoint coordinate, mvKeys coordinate, mvuRight, mvDepth or pose value that is not finite.
 * PLI_ERR_CAPACITY for more than PLI_BOW_MAX_FEATURES rows in n1 or in a neighbour.  nkf == 0, n1 == 0 and empty neighbours are
 * valid.  The number of kernel launches does not depend on nkf. */
enum {
  PLI_NEWPT_CREATED = 0,          /* :670, a map point is created                                   */
  PLI_NEWPT_LOW_PARALLAX = 1,     /* :582, no stereo and very low parallax                          */
  PLI_NEWPT_W_ZERO = 2,           /* :565, x3D.at<float>(3) == 0                                    */
  PLI_NEWPT_EMPTY_UNPROJECT = 3,  /* :587, UnprojectStereo returned an empty Mat (mvDepth <= 0)     */
  PLI_NEWPT_Z1 = 4,               /* :590, z1 <= 0                                                  */
  PLI_NEWPT_Z2 = 5,               /* :594, z2 <= 0                                                  */
  PLI_NEWPT_REPROJ1_MONO = 6,     /* :609, > 5.991 * sigmaSquare1                                   */
  PLI_NEWPT_REPROJ1_STEREO = 7,   /* :621, > 7.8 * sigmaSquare1                                     */
  PLI_NEWPT_REPROJ2_MONO = 8,     /* :635                                                           */
  PLI_NEWPT_REPROJ2_STEREO = 9,   /* :646                                                           */
  PLI_NEWPT_DIST_ZERO = 10,       /* :657                                                           */
  PLI_NEWPT_FAR = 11,             /* :660                                                           */
  PLI_NEWPT_RATIO_LOW = 12,       /* :666, ratioDist*ratioFactor < ratioOctave                      */
  PLI_NEWPT_RATIO_HIGH = 13,      /* :666, ratioDist > ratioOctave*ratioFactor                      */
  PLI_NEWPT_TAKEN_EARLIER = 14,   /* matched on the state at entry, but an earlier neighbour created the feature's map point */
  PLI_NEWPT_NOT_MATCHED = 15      /* SearchForTriangulation found no pair for the feature           */
};
pli_status pli_create_new_map_points(pli_ctx* ctx, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                     const uint8_t* has_mp1, const float* uright1, const float* depth1, const float* key1,
                                     int32_t n1, int32_t nkf, const int32_t* kf_off, const pli_keypoint* kf_kp,
                                     const uint8_t* kf_desc, const int32_t* kf_node, const uint8_t* kf_has_mp,
                                     const float* kf_uright, const float* kf_depth, const float* kf_key, const float* F12,
                                     const float* ep, const float* pose1, const float* kf_pose, const pli_fuse_camera* cam,
                                     float mb, int32_t coarse, int32_t far_points, float th_far, float ratio_factor,
                                     int32_t* matches12, int32_t* nmatches, int32_t* status, float* x3d, int32_t* nnew);

/* The same step for keyframes of a rig of two KannalaBrandt8 cameras (NLeft != -1, mpCamera2 set), the branch
 * `mpCurrentKeyFrame->mpCamera2 && pKF2->mpCamera2` (LocalMapping.cc:463-528), one keyframe against nkf neighbours in one call:
 * pli_search_for_triangulation_two_cameras (bOnlyStereo = false, no orientation check), then per matched pair :530-667 with the
 * pose and the camera that (bRight1, bRight2) = (idx1 >= NLeft of pKF1, idx2 >= NLeft of pKF2) pick for each side, and the
 * first-accepted-wins pick of pli_create_new_map_points, which holds here unchanged.
 * What the branch reads: kp1 / kp2 are mvKeys[idx] or mvKeysRight[idx - NLeft], never mvKeysUn (:446-448, :454-456); bStereo1 and
 * bStereo2 are false (:450, :459), so mvuRight's value is never used, mvDepth is not read, and the call takes no uright, depth, key, mb,
 * bf, F12 or ep; the triangulation condition :550 is 0 < cosParallaxRays < 0.9998 and everything else PLI_NEWPT_LOW_PARALLAX;
 * xn = unprojectMat(kp.pt) is KannalaBrandt8::unproject with z = 1; both gates project with KannalaBrandt8::project against
 * 5.991 * sigmaSquare in double (:605-610, :632-636).  PLI_NEWPT_EMPTY_UNPROJECT, PLI_NEWPT_REPROJ1_STEREO and
 * PLI_NEWPT_REPROJ2_STEREO cannot occur here.
 * Tables: kp1 ... kf_has_mp, n1_left, kf_nleft, cam_left, cam_right and rel exactly as for pli_search_for_triangulation_two_cameras.
 * pose1 (2 x 15) / kf_pose (nkf x 2 x 15): per keyframe the left side, then the right side, 15 floats each as for
 * pli_fuse_search_two_cameras - Rcw row major, tcw, Ow: GetRotation / GetTranslation / GetCameraCenter, then GetRightRotation /
 * GetRightTranslation / GetRightCameraCenter (GetPose / GetRightPose are the same floats; Rwc is the exact transpose).
 * coarse, far_points, th_far, ratio_factor and the five outputs exactly as for pli_create_new_map_points.
 * A call in which one keyframe has a second camera and another has none is out of scope (the reference falls through :463 with the
 * poses of the previous pair); the caller refuses it.
 * Checked before anything is launched, PLI_ERR_INVALID: null pointers, negative counts, a decreasing kf_off, n1_left outside
 * [0, n1], a kf_nleft outside its neighbour's rows, an octave outside [0, orb_nlevels), a keypoint coordinate, rel or pose value that
 * is not finite.  PLI_ERR_CAPACITY for more than PLI_BOW_MAX_FEATURES rows in n1 or in a neighbour, or nkf x n1 beyond the pair index.
 * nkf == 0, n1 == 0, empty neighbours, n1_left == 0 and n1_left == n1 are valid.  Six kernel launches, whatever nkf is. */
pli_status pli_create_new_map_points_two_cameras(pli_ctx* ctx, const pli_keypoint* kp1, const uint8_t* desc1, const int32_t* node1,
                                                 const uint8_t* has_mp1, int32_t n1, int32_t n1_left, int32_t nkf,
                                                 const int32_t* kf_off, const int32_t* kf_nleft, const pli_keypoint* kf_kp,
                                                 const uint8_t* kf_desc, const int32_t* kf_node, const uint8_t* kf_has_mp,
                                                 const pli_kb8_camera* cam_left, const pli_kb8_camera* cam_right, const float* rel,
                                                 const float* pose1, const float* kf_pose, int32_t coarse, int32_t far_points,
                                                 float th_far, float ratio_factor, int32_t* matches12, int32_t* nmatches,
                                                 int32_t* status, float* x3d, int32_t* nnew);

/* Loop closing's ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) ORBmatcher.cc:473-586 and the
 * overload with vpPointsKFs / vpMatchedKF :588-704 (LoopClosing.cc:631, :656, :852), for ONE list of nmp map points against npair
 * (keyframe, Scw) pairs in one call.  Unlike Fuse this search is sequential across the points of a pair: vpMatched[bestIdx] = pMP
 * (:579 / :696) takes the keypoint away from every later point (:558 / :675).  Points are decided in list order; the pairs are
 * independent of each other, each with its own owner state, also when the same keyframe appears in two pairs.  A point listed
 * twice is two entries (the reference's spAlreadyFound is fixed at entry, :490).
 * Tables as pli_fuse_search: mp (max_dist / valid as there), mp_desc, kf_off, kf_kp, kf_desc, cam (bf is not read), th,
 * level_ratio; kf_pose: 15 floats per pair - Rcw, tcw, Ow decomposed from Scw on the host exactly as :483-487; skip: npair x nmp,
 * may be NULL, != 0 = spAlreadyFound.count(pMP) :501.
 * occupied: one byte per keyframe row (ragged by kf_off), may be NULL: != 0 = vpMatched[idx] != NULL at entry (:558).
 * Gates in the reference's order: valid / skip :501; z < 0 :511; the projection; KeyFrame::IsInImage :522; the distance range
 * :531; PO.dot(Pn) < 0.5*dist :537; PredictScale :540 through level_ratio; radius = th * mvScaleFactors[level] :543; an empty
 * window :547.  project_form selects the projection's arithmetic, which rounds differently: 0 = Pinhole::project, fx*x/z + cx
 * (:519); 1 = invz = 1/z; x*invz; fx*x + cx (:631-636).  Every operation is float, in the written order, nothing contracted.
 * Candidates :555-575: the rows of KeyFrame::GetFeaturesInArea, without the owned ones (occupied at entry, or taken by an earlier
 * point of this pair), octave in [level-1, level]; the strict minimum of the Hamming distance in visiting order = the minimum of
 * the key (distance, cell column, cell row, index), as in pli_fuse_search.
 * Acceptance :577: bestDist <= TH_LOW*ratioHamming is the float comparison (float)bestDist <= 50.0f * ratio_hamming (one
 * rounding).  With no candidate the reference holds bestDist = 256 and bestIdx = -1 and would write vpMatched[-1] if the product
 * reached 256: ratio_hamming must be finite, > 0 and 50.0f * ratio_hamming < 256, else PLI_ERR_INVALID.
 * row_point: one int per keyframe row: the index of the point that took the row in this call (vpMatched[row] = vpPoints[i]), -1
 * otherwise; rows occupied at entry stay -1.  best_idx (may be NULL): npair x nmp, the row a point took or -1.  nmatches[npair]:
 * the reference's return value.
 * Errors: PLI_ERR_INVALID for null pointers, project_form outside {0, 1}, an octave outside [0, orb_nlevels), a decreasing
 * kf_off, a decreasing or NaN level_ratio; PLI_ERR_CAPACITY for a keyframe with more than PLI_BOW_MAX_FEATURES rows (nothing is
 * truncated).  npair == 0, nmp == 0 and empty keyframes are valid.  The number of kernel launches does not depend on npair or
 * nmp. */
pli_status pli_search_by_projection_sim3(pli_ctx* ctx, const pli_fuse_point* mp, const uint8_t* mp_desc, int32_t nmp, int32_t npair,
                                         const int32_t* kf_off, const pli_keypoint* kf_kp, const uint8_t* kf_desc,
                                         const float* kf_pose, const uint8_t* skip, const uint8_t* occupied,
                                         const pli_fuse_camera* cam, float th, const float* level_ratio, float ratio_hamming,
                                         int32_t project_form, int32_t* row_point, int32_t* best_idx, int32_t* nmatches);

/* Relocalisation's ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) ORBmatcher.cc:2325-2447
 * (Tracking.cc:4290 with th 10, ORBdist 100 and :4304 with 3, 64), for ONE frame table against ncand candidates in one call.  The
 * roles are those of pli_search_by_projection_sim3 turned round: the searched table is the frame (f_kp = mvKeysUn: pt, octave and,
 * with check_orientation, angle are read; f_desc = mDescriptors; nf rows), the point lists belong to the candidates.  The search
 * is sequential across the points of a candidate: CurrentFrame.mvpMapPoints[bestIdx2] = pMP (:2405) closes the row to every later
 * point (:2389).  Points are decided in list order; the candidates are independent of each other, each with its own owner state,
 * also when two of them list the same points.
 * Candidate c owns rows mp_off[c] .. mp_off[c+1]-1 of mp, mp_desc and mp_angle (pKF->GetMapPointMatches() in index order, :2339):
 * mp as pli_fuse_search (normal is not read), valid = pMP && !pMP->isBad() && !sAlreadyFound.count(pMP) (:2345-2347: the lists are
 * per candidate, so there is no skip table); mp_desc = GetDescriptor(); mp_angle = pKF->mvKeysUn[i].angle, may be NULL when
 * check_orientation == 0.  pose: ncand x 15 floats - Rcw row major, tcw (of CurrentFrame.mTcw as set for that candidate) and
 * Ow = -Rcw.t()*tcw (:2329-2331), computed on the host.  occupied: ncand x nf bytes, may be NULL: != 0 =
 * CurrentFrame.mvpMapPoints[i2] != NULL at entry (:2389).  cam, th, level_ratio as pli_fuse_search (bf is not read).
 * Gates in the reference's order, which are NOT those of the Sim3 search: valid; NO z < 0 gate (a point behind the camera whose
 * projection falls into the image is searched like any other); Pinhole::project, fx*x/z + cx (:2353); the image gate :2355-2358,
 * closed on both sides (not IsInImage's half-open one); the distance range :2368; NO viewing-normal gate;
 * MapPoint::PredictScale(dist3D, &CurrentFrame) :2371 through level_ratio; radius = th * mvScaleFactors[level] :2374; an empty
 * window :2378.  Every operation is float, in the written order, nothing contracted (the matrix product and cv::norm as
 * pli_fuse_search).
 * One deviation: the reference's gate lets a NaN projection through and then converts NaN to int, which is undefined.  Here a point
 * is admitted only when u >= min_x && u <= max_x && v >= min_y && v <= max_y: for every non-NaN u, v this is the reference's gate,
 * a NaN leaves.
 * Candidates :2386-2401: the rows of Frame::GetFeaturesInArea(u, v, radius, level-1, level+1) (Frame.cc:774-843: the cells and
 * the visiting order of KeyFrame::GetFeaturesInArea, octave in [level-1, level+1]) without the owned ones (occupied at entry, or
 * taken by an earlier point of this candidate); the strict minimum of the Hamming distance in visiting order = the minimum of the
 * key (distance, cell column, cell row, index).  Acceptance :2403: bestDist <= orb_dist, integers.  With no candidate the
 * reference holds bestDist = 256 and bestIdx2 = -1 and would write mvpMapPoints[-1] at orb_dist = 256: orb_dist must lie in
 * [0, 255].
 * check_orientation (mbCheckOrientation, :2408-2444): the bin of pKF->mvKeysUn[i].angle - CurrentFrame.mvKeysUn[bestIdx2].angle
 * as in pli_search_by_bow (every angle in [0, 360)), ComputeThreeMaxima after the walk, every match in another bin set back to
 * NULL and nmatches decremented.  A row that the filter gives back was still closed during the walk.
 * row_point: ncand x nf, the index WITHIN the candidate's own list of the point that holds the row after the rotation filter
 * (CurrentFrame.mvpMapPoints[row] = vpMPs[i]), -1 otherwise; rows occupied at entry stay -1.  best_idx (may be NULL):
 * mp_off[ncand] entries, the row a point took BEFORE the filter or -1.  nmatches[ncand]: the reference's return value.
 * Errors: PLI_ERR_INVALID for null pointers, mp_off[0] != 0 or a decreasing mp_off, an octave outside [0, orb_nlevels), a
 * decreasing or NaN level_ratio, orb_dist outside [0, 255], with check_orientation an angle outside [0, 360); PLI_ERR_CAPACITY
 * for nf > PLI_BOW_MAX_FEATURES (the owner table is nf ints in LDS) or a list with more than PLI_BOW_MAX_FEATURES points (a
 * keyframe has no more rows than that); nothing is truncated.  ncand == 0, empty point lists and nf == 0 are valid.  The number of
 * kernel launches does not depend on ncand or on the number of points. */
pli_status pli_search_by_projection_reloc(pli_ctx* ctx, int32_t ncand, const int32_t* mp_off, const pli_fuse_point* mp,
                                          const uint8_t* mp_desc, const float* mp_angle, const float* pose,
                                          const pli_keypoint* f_kp, const uint8_t* f_desc, int32_t nf, const uint8_t* occupied,
                                          const pli_fuse_camera* cam, float th, const float* level_ratio, int32_t orb_dist,
                                          int32_t check_orientation, int32_t* row_point, int32_t* best_idx, int32_t* nmatches);

/* Monocular initialisation's ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * ORBmatcher.cc:706-821 (Tracking.cc:2109-2110: matcher (0.9, true), window 100) of one table against one table.  kp1 / desc1 =
 * F1.mvKeysUn / mDescriptors (n1 rows: octave and, with check_orientation, angle are read), prev_matched = vbPrevMatched as n1 x
 * (x, y), READ ONLY: the update :816-818, vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt for the matches that are left, is
 * the caller's, from matches12 and kp2 (each call's windows come from the previous call's result, so there is no batch form).
 * kp2 / desc2 = F2.mvKeysUn / mDescriptors (n2 rows: pt, octave, angle); min_x .. max_y = mnMinX .. mnMaxY of the 64 x 48 grid.
 * Only F1 keypoints with octave == 0 search (:723).  Candidates: Frame::GetFeaturesInArea(x, y, window_size, 0, 0)
 * (Frame.cc:774-843): the cells column by column and row by row, a cell's keypoints in index order, octave == 0 only, the window
 * strict (fabs(dx) < r && fabs(dy) < r); a keypoint that PosInGrid (:845-855) puts outside the grid is in no cell.
 * The walk over i1 is ordered, and a row of F2 is NOT closed once taken.  Its state is vMatchedDistance[i2] (INT_MAX at entry) and
 * vnMatches21[i2]: candidate i2 is left out for i1 when vMatchedDistance[i2] <= dist (:745) and is then neither best nor
 * second-best; a later i1 with a strictly smaller distance takes the row again and evicts the earlier owner (:764-768), an equal
 * distance does not.  Best = the first strict minimum in visiting order = the minimum of the key (distance, cell column, cell row,
 * index); bestDist2 = the second-smallest distance among the candidates not left out (equal to the best on a tie, INT_MAX with
 * fewer than two).  Acceptance :760-762: bestDist <= TH_LOW (50) and bestDist < (float)bestDist2 * nnratio in float (45 against a
 * second-best of 50 at 0.9f is rejected: 50 * 0.9f == 45.0f).
 * check_orientation (mbCheckOrientation, :774-813): the bin of F1's angle minus F2's as in pli_search_by_bow (every angle in
 * [0, 360)); rotHist records EVERY acceptance, also those evicted later, so ComputeThreeMaxima sees bin sizes that count evicted
 * i1; the filter clears only entries that still hold a match (:805).
 * matches12[n1] = vnMatches12 after the filter; raw12[n1] (may be NULL) = vnMatches12 after the walk and before the filter, the
 * evictions applied; *nmatches = the return value.
 * Errors: PLI_ERR_INVALID for null pointers, window_size < 0, nnratio not finite or <= 0, empty image bounds, an octave outside
 * [0, orb_nlevels), with check_orientation an angle outside [0, 360), a NaN in prev_matched; PLI_ERR_CAPACITY for n1 or n2 above
 * PLI_BOW_MAX_FEATURES (the row state and vnMatches12 live in LDS); nothing is truncated.  n1 == 0 and n2 == 0 are valid.  The
 * number of kernel launches does not depend on n1 or n2. */
pli_status pli_search_for_initialization(pli_ctx* ctx, const pli_keypoint* kp1, const uint8_t* desc1, int32_t n1,
                                         const float* prev_matched, const pli_keypoint* kp2, const uint8_t* desc2, int32_t n2,
                                         float min_x, float max_x, float min_y, float max_y, int32_t window_size, float nnratio,
                                         int32_t check_orientation, int32_t* matches12, int32_t* raw12, int32_t* nmatches);

/* --- The keyframe database's place-recognition queries (KeyFrameDatabase.cc:806-1089) ---
 * KeyFrameDatabase::DetectRelocalizationCandidates (Tracking.cc:4184) and DetectNBestCandidates (LoopClosing.cc:395) walk an
 * inverted file of std::list<KeyFrame*> and then score every keyframe that shares enough words with DBoW2's L1Scoring::score
 * (ScoringObject.cpp:23-68).  pli_kfdb keeps the BowVectors of the keyframes on the device instead and answers, per query and for
 * EVERY keyframe in one launch, the three numbers those functions derive from the inverted file and the score; the ordered,
 * stateful rest (minCommonWords, covisibility accumulation, the sort and the filters) stays on the host
 * (adapters/orbslam_keyframe_database.hpp).
 *
 * A database belongs to the context it was created on (as a pli_vocab does) and must be destroyed before it; every call holds the
 * context's lock and runs on its stream, so the tracking and loop-closing threads may call concurrently.  A keyframe lives in a
 * SLOT: pli_kfdb_add hands out the smallest free slot id, which stays fixed until pli_kfdb_erase frees it for reuse.  The slot
 * high-water mark is one more than the largest slot id handed out since creation or the last pli_kfdb_clear.
 *
 * Storage: a CSR arena on the device (per slot an offset and a count; word ids uint32_t, strictly ascending within a slot; values
 * double).  add appends; a full arena doubles (allocate, copy device to device on the stream, free the old one).  erase leaves a
 * hole; once the holes exceed half of the arena's words the next add rebuilds the arena from the host mirror of the live vectors. */
typedef struct pli_kfdb pli_kfdb;
struct pli_kfdb_stats {     /* (no typedef: the name is also the function's; write `struct pli_kfdb_stats`) */
  int32_t slot_high_water;  /* slots a query answers for                                      */
  int32_t live_keyframes;
  int64_t live_words;       /* words of the live keyframes                                    */
  int64_t arena_words;      /* words appended since the last rebuild / clear: live + holes    */
  int64_t arena_capacity;   /* words the device arena holds before it doubles                 */
  int32_t rebuilds;         /* since creation                                                 */
  int32_t growths;          /* since creation                                                 */
};
/* waves of one query launch: min(ceil(nslots / 4), PLI_KFDB_QUERY_MAX_WAVES / 4) workgroups of 4 waves, the slots strided over them */
#define PLI_KFDB_QUERY_MAX_WAVES 2048
pli_status pli_kfdb_create(pli_ctx* ctx, pli_kfdb** out);
void pli_kfdb_destroy(pli_kfdb* db);
/* One keyframe's BowVector in map order.  PLI_ERR_INVALID: null arguments, n < 0, word ids not strictly ascending;
 * PLI_ERR_CAPACITY: n > PLI_BOW_MAX_FEATURES (a BowVector has at most one word per feature).  n == 0 is valid.  On an error the
 * database is unchanged. */
pli_status pli_kfdb_add(pli_ctx* ctx, pli_kfdb* db, const uint32_t* word, const double* value, int32_t n, int32_t* slot);
/* PLI_ERR_INVALID for a slot that is free or was never handed out. */
pli_status pli_kfdb_erase(pli_ctx* ctx, pli_kfdb* db, int32_t slot);
/* Frees every slot; the high-water mark returns to 0, the arena keeps its capacity. */
pli_status pli_kfdb_clear(pli_ctx* ctx, pli_kfdb* db);
pli_status pli_kfdb_stats(const pli_kfdb* db, struct pli_kfdb_stats* out);
/* The query BowVector (qword strictly ascending, nq <= PLI_BOW_MAX_FEATURES else PLI_ERR_CAPACITY) against every slot below the
 * high-water mark; nslots must equal it (PLI_ERR_INVALID otherwise: the caller's tables and the database disagree).
 *   common[s] = the number of words slot s shares with the query (mnRelocWords / mnPlaceRecognitionWords of a fresh query);
 *   first[s]  = the INDEX IN THE QUERY VECTOR of the first shared word, -1 without one: the reference pushes a keyframe to
 *               lKFsSharingWords at that word, so (first, order of add) orders that list;
 *   score[s]  = L1Scoring::score(query, keyframe) as the reference's double, bit for bit: the sum in ascending word order of
 *               fabs(vi - wi) - fabs(vi) - fabs(wi), vi the query's value, then -sum / 2.0 (-0.0 when nothing is shared).
 * A free slot and an empty keyframe answer 0, -1, -0.0.  nq == 0 and an empty database are valid.  Per query: one upload of
 * 12 * nq bytes, one launch (k_kfdb_query), one download of 16 * nslots bytes. */
pli_status pli_kfdb_query(pli_ctx* ctx, pli_kfdb* db, const uint32_t* qword, const double* qvalue, int32_t nq, int32_t nslots,
                          int32_t* common, int32_t* first, double* score);

/* --- MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:300-365) and MapLine::ComputeDistinctiveDescriptors
 * (MapLine.cc:246-317) for a batch of features ---
 * The reference runs it one feature at a time on the local-mapping thread (LocalMapping.cc:267-286 and :780-793,
 * LoopClosing.cc:1012, MapPoint.cc:268, MapLine.cc:216).  A GROUP is the N descriptors (32 bytes each) that observe one feature, in
 * the order in which the reference pushed them into vDescriptors (MapPoint.cc:319-325): group p owns rows off[p] .. off[p + 1] - 1
 * of desc; off holds nfeat + 1 entries, off[0] == 0, non-decreasing.
 *   D[i][j]   = the Hamming distance of rows i and j, D[i][i] = 0 (:333-343; the line form computes every pair twice,
 *               MapLine.cc:284-293, which gives the same matrix);
 *   median_i  = the element at index int(0.5 * (N - 1)), that is (N - 1) / 2 rounded down, of row i sorted ascending (:350-352);
 *               the diagonal's zero is part of the row;
 *   BestIdx   = the LOWEST i with the least median_i (:354 tests `median < BestMedian` strictly), BestMedian that value.
 * So for N = 1 and N = 2 every median is 0 and BestIdx = 0; the largest possible median is 256 (a descriptor and its complement).
 *   best[p]        = BestIdx within group p, -1 for an empty group (the reference returns before it touches mDescriptor, :314-315
 *                    and :327-328);
 *   best_median[p] = BestMedian, INT32_MAX for an empty group; may be NULL;
 *   row_median     = off[nfeat] entries, median_i of every row (so that a test can hold every row to the reference, not only the
 *                    winner); may be NULL.
 * The answer is exact (integers): bit for bit the reference's.  A feature's answer depends on its own group alone, so batching
 * changes nothing.  PLI_ERR_INVALID: off[0] != 0, a decreasing off, null off or best, a NULL desc with rows present.
 * PLI_ERR_CAPACITY: a group of more than PLI_DISTINCTIVE_MAX_OBS rows; nothing is truncated and no output is written.  (The cap is
 * far beyond what the reference can run: its `float Distances[N][N]` is a stack array that passes 8 MiB near N = 1450.)
 * nfeat == 0 and off[nfeat] == 0 are valid.  Host pointers of any alignment are accepted.  One upload of the descriptors, one of
 * off, one download; N <= 64: one launch, a wave per group; above: a workgroup per 256 rows of a group, then a launch that picks the winners. */
#define PLI_DISTINCTIVE_MAX_OBS 2048
pli_status pli_distinctive_descriptors(pli_ctx* ctx, const uint8_t* desc, const int32_t* off, int32_t nfeat, int32_t* best,
                                       int32_t* best_median, int32_t* row_median);

/* --- Local-map tracking: the front of Tracking::SearchLocalPointsAndLines (Tracking.cc:3809-3883) for a frame of one camera ---
 * pli_search_local_points covers :3809-3855 in one call: Frame::isInFrustum (Frame.cc:585-647, the branch Nleft == -1) of every
 * local map point, the queries of ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) as
 * ORBmatcher.cc:53-73 builds them, and that search (pli_search_local_map's kernels) on the queries where the device left them.
 * mp / mp_desc: the nq points of mvpLocalMapPoints in list order as pli_fuse_point rows (valid == 0: skipped at :3813-3816,
 * mnLastFrameSeen == mnId or isBad(); also a point whose max_dist is not finite and positive) and their GetDescriptor() rows.
 * valid == PLI_LOCAL_STORED_VIEW: a point that :3813 skips (mnLastFrameSeen == mnId), is not bad, and still has mbTrackInView set
 * from an earlier frame.  The skip only bypasses isInFrustum; SearchByProjection at :3854 walks the whole list and tests
 * mbTrackInView (ORBmatcher.cc:53), so the reference searches such a point, in its list position, with the fields it holds.  This
 * happens in ordinary tracking: for a frame of one camera TrackWithMotionModel's outlier loop (:2996-3004) sets mnLastFrameSeen
 * and resets only mbTrackInViewR, and the point's row is NULL by :3770.  Such a row carries the stored fields instead of world
 * coordinates: pos = {mTrackProjX, mTrackProjY, mTrackProjXR}, normal = {mTrackDepth, mTrackViewCos, (float)mnTrackScaleLevel}
 * (the level in [0, orb_nlevels), else PLI_ERR_INVALID); the distance fields are not read.  Its query is built from them as from
 * a record (the far-point gate included), its view record is all zero and it does not count in *n_in_view.
 * pose: 15 floats, mRcw row major, mtcw, mOw (the stored values).  cam: fx .. cy of mpCamera, mbf, mnMinX .. mnMaxY.
 * viewing_cos_limit: 0.5 at :3818.  th, far_points, th_far, nnratio: the arguments of :3854 and of ORBmatcher(0.8).
 * level_ratio: as for pli_fuse_search.  cur_*: the frame's mvKeysUn, mDescriptors, mvuRight and "holds a map point with
 * Observations() > 0" as for pli_search_local_map (cur_occupied may be NULL).
 * The arithmetic is the reference's, in its order: mRcw*P + mtcw as a cv::Mat product (double accumulation, one rounding),
 * cv::norm and Mat::dot in double, the rest float and nothing fused.  The image gate is the one written at :607-610,
 * u < mnMinX || u > mnMaxX: closed at mnMaxX / mnMaxY (KeyFrame::IsInImage of pli_fuse_search is open there), and a NaN projection
 * (PcZ == 0 with PcX == 0) passes it.  The viewing angle is viewCos = (float)(PO.dot(Pn) / dist) < viewing_cos_limit, compared in
 * float (pli_fuse_search compares the dot product with 0.5 * dist in double).
 * view[i]: what the call leaves in the map point.  A skipped point: all zero.  Otherwise proj_x / proj_y = -1 until the point
 * passes the image gate and mTrackProjX / Y from there on, also where a later gate refuses it (:612-613); in_view = mbTrackInView;
 * proj_xr (mTrackProjXR), depth (mTrackDepth = cv::norm(Pc)), level (mnTrackScaleLevel) and view_cos (mTrackViewCos) are written
 * only with in_view and are 0 otherwise (the reference leaves the fields as they were).
 * The query of point i is valid when in_view and not (far_points && depth > th_far); radius = r * mvScaleFactors[level] with
 * r = view_cos > 0.998 ? 2.5 : 4.0 (the float against the double constant), times th when th != 1.0; octaves [level - 1, level].
 * A point in view takes part whatever its Observations(): as for pli_search_local_map the row it takes is closed to the points
 * behind it, so a caller with points of no observations in view replays that case itself (the adapter refuses it).
 * best_idx2[i]: the keypoint point i took, or -1.  A query whose projection is NaN takes no keypoint: every distance test against
 * it is false (the device closes such a query when it writes it; the view record keeps the NaN).  *n_in_view = nToMatch of :3821.
 * The search runs whatever it is: the reference searches only when nToMatch > 0 (:3829), so with *n_in_view == 0 a caller that
 * passed stored views ignores best_idx2 and *nmatches (the adapter does).
 * *nmatches = the reference's return value.  Frames above 15360 keypoints take the ordered scan, as pli_search_local_map.
 * PLI_ERR_INVALID before any device call: a null context, camera, pose or level_ratio, negative counts, null tables with rows
 * present, empty image bounds, a decreasing level_ratio, an octave outside [0, orb_nlevels).  nq == 0 and ncur == 0 are valid. */
#define PLI_LOCAL_STORED_VIEW 2
typedef struct pli_local_view {   /* 32 bytes */
  float proj_x, proj_y, proj_xr, depth, view_cos;
  int32_t level, in_view, pad;
} pli_local_view;
pli_status pli_search_local_points(pli_ctx* ctx, const pli_fuse_point* mp, const uint8_t* mp_desc, int32_t nq, const float* pose,
                                   const pli_fuse_camera* cam, float viewing_cos_limit, float th, int32_t far_points,
                                   float th_far, float nnratio, const float* level_ratio, const pli_keypoint* cur_kp,
                                   const uint8_t* cur_desc, const float* cur_uright, const uint8_t* cur_occupied, int32_t ncur,
                                   pli_local_view* view, int32_t* best_idx2, int32_t* n_in_view, int32_t* nmatches);

/* pli_search_local_lines covers :3862-3883: Frame::isInFrustum_l (Frame.cc:661-701) of every local map line, the ordered list
 * mvpLocalMapLines_InFrustum, and match(mvpLocalMapLines_InFrustum, mCurrentFrame, nnr, matches_12) (LineMatcher.cpp:161, the
 * one-way matchNNR of pli_match_nnr) on the descriptors of the lines in view.
 * sp: nl x 3 floats, the start point of GetWorldPos() cast to float (Converter::toCvMat of sep.head(3)); valid[i] == 0: skipped at
 * :3865-3868; desc: the GetDescriptor() rows; pose, cam as above (bf is not read); cur_desc: the n2 rows of mDescriptors_Line.
 * Per line: mRcw*sp + mtcw, out if PcZ < 0, invz = 1.0f / PcZ, u = fx*PcX*invz + cx evaluated left to right (NOT Pinhole::project's
 * fx*x/z + cx: the two round differently), the closed image gate of :687-690 (a NaN passes).
 * in_view[i] (nl ints) = mbTrackInView; proj_s[i] (nl x 2 floats) = mTrackProjsX / Y where in view, else 0 (the reference leaves
 * them as they were); in_frustum[k] = the list index of the k-th line in view, k < *n_in_view (room for nl); matches_12[k] = the
 * frame line matched to it or -1 (room for nl; the rows from *n_in_view on are not written).  *n_in_view = nToMatch,
 * *nmatches = match()'s return value; n2 < 2 matches nothing, as pli_match_nnr.  The list's length decides the match's launch, so
 * the call reads the count back once between its two halves.
 * NOT covered, and left to the caller on the fields as they stand: the reference never writes mTrackProjeX / mTrackProjeY - it
 * reads them uninitialised for mnTrackangle (Frame.cc:698) and for the position gate of Tracking.cc:3908-3911 - so mnTrackangle
 * and the loop :3886-3919 (mvDisparity_l, Observations(), the position gate, mvpMapLines[i2] = pML) stay on the host.
 * PLI_ERR_INVALID before any device call: a null context, camera or pose, negative counts, null tables with rows present. */
pli_status pli_search_local_lines(pli_ctx* ctx, const float* sp, const uint8_t* valid, const uint8_t* desc, int32_t nl,
                                  const float* pose, const pli_fuse_camera* cam, const uint8_t* cur_desc, int32_t n2, float nnr,
                                  int32_t* in_view, float* proj_s, int32_t* in_frustum, int32_t* matches_12,
                                  int32_t* n_in_view, int32_t* nmatches);

/* ------------------------------------------------------------------------ */
/* Measurement hooks (bench.py / tests only).                                */
/* ------------------------------------------------------------------------ */
/* Tracing: with PLI_ROCTX=1 in the environment when the library is loaded, every entry point, every stage of a call
 * (ingest, ORB chain, line chain, stereo matchers) and every kernel launch is bracketed by roctxRangePush / roctxRangePop
 * (rocprofiler-sdk's marker library, found at run time), so that `rocprofv3 --kernel-trace --marker-trace -- <program>` shows which
 * call and stage a kernel belongs to.  Without the switch nothing is loaded and nothing is pushed.  Returns the number of ranges
 * pushed so far by this process (0 when tracing is off). */
int64_t pli_trace_ranges(void);

/* When enabled every kernel launch of the context is bracketed by HIP events on
 * the context stream; pli_prof_report writes "name calls total_ms\n" lines. */
pli_status pli_prof_enable(pli_ctx* ctx, int32_t on);
pli_status pli_prof_reset(pli_ctx* ctx);
pli_status pli_prof_report(pli_ctx* ctx, char* buf, int64_t buf_bytes);

/* Intermediate products, for parity tests against the oracle stage by stage.
 * `what` is one of PLI_DBG_*; data are copied to `dst` (host).  *out_bytes =
 * bytes written.  image = frame*2 + eye. */
enum {
  PLI_DBG_PYRAMID_LEVEL = 1,   /* arg = level; u8 w*h                                       */
  PLI_DBG_BLUR_LEVEL = 2,      /* arg = level; u8 w*h (7x7 sigma 2)                         */
  PLI_DBG_FAST_CANDIDATES = 3, /* arg = level; int32 count then {int32 x,y,score} records, reference order */
  PLI_DBG_LEVEL_KEYPOINTS = 4, /* arg = level; int32 count then {int32 x,y,score} after the quadtree */
  PLI_DBG_LSD_SCALED = 5,      /* u8 W'*H' (blur 0.6 + x1.2 resize)                         */
  PLI_DBG_LSD_ANGLE = 6,       /* float W'*H' degrees, -1024 = NOTDEF                       */
  PLI_DBG_LSD_SEGMENTS = 7,    /* int32 count then float[4] x1,y1,x2,y2 in detection order: EVERY detected segment only in a
                                  debug context (pli_debug_enable) — a plain context omits the segments that cannot pass the
                                  length cut (pli_lsd_segment_box_cut), except on the sequential schedule, which lists them all */
  PLI_DBG_LBD_DXDY = 8,        /* int16 dx[w*h] then int16 dy[w*h]                          */
  PLI_DBG_LSD_ORDER = 9,       /* int32 count then int32 pixel index of every seed in visiting order */
  PLI_DBG_LBD_FLOAT = 10,      /* float[kl_cap][72] LBD band vector before binarisation     */
  PLI_DBG_STEREO_SAD = 11,     /* int32 sad[kp_cap] (-1 = none) then int32 bestIdxR[kp_cap] of the frame */
  PLI_DBG_LSD_OWNER = 12,      /* int32 rounds, then int32 owner rank per scaled pixel (0x7fffffff = undefined) */
  PLI_DBG_LSD_SIZES = 13       /* int32 region size recorded by the last grower of every seed rank */
};
/* Keep the extra intermediates (LSD angle map, LBD float vectors, stereo best index) during runs. */
pli_status pli_debug_enable(pli_ctx* ctx, int32_t on);
pli_status pli_debug_fetch(pli_ctx* ctx, int32_t image, int32_t what, int32_t arg,
                           void* dst, int64_t dst_bytes, int64_t* out_bytes);

const char* pli_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PLI_FRONTEND_H */
