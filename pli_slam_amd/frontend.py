"""Host-side mirror of the reference's front-end interface over the C ABI.

Names and argument meaning follow the reference classes so that parity tests
read like the reference's call sites:

  ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)(image, mask, vLappingArea)
      reference include/ORBextractor.h:53-63, src/ORBextractor.cc:1068
  Lineextractor(lsd_nfeatures, min_line_length, lsd_refine, lsd_scale, ...)(image, mask)
      reference include/LineExtractor.h:44-51, src/LineExtractor.cc:31
  Frontend.compute_stereo_matches() / compute_stereo_matches_lines()
      reference Frame::ComputeStereoMatches / _Lines, src/Frame.cc:976,1156
  DescriptorDistance, match, SearchByProjection
      reference src/ORBmatcher.cc:2495,2179 and src/LineMatcher.cpp:201

All arithmetic happens in the HIP library; this file only moves buffers.
"""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import KEYLINE_DT, KEYPOINT_DT, PROJ_QUERY_DT, check, ptr


def _u8(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim != 2:
        raise ValueError("grayscale u8 image expected")
    return img


def _colour_u8(img, channels):
    """An interleaved (H, W, channels) u8 image as the library reads it: pixels of `channels` adjacent bytes, rows any number of
    bytes apart.  A view with exactly that layout (padded rows, a base at any byte) goes through as it is, anything else is copied."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != channels:
        raise ValueError("(H, W, %d) u8 image expected under the image format that is set" % channels)
    if img.dtype != np.uint8 or img.strides[2] != 1 or img.strides[1] != channels or img.strides[0] < img.shape[1] * channels:
        img = np.ascontiguousarray(img, dtype=np.uint8)
    return img


PRODUCT_ENV = ("PLI_ROCTX", "PLI_SYNC_DEBUG", "PLI_TX_TAIL", "PLI_LSD_MODE")      # what libpli_frontend.so itself reads
PYTHON_ENV = ("PLI_LIB_PATH", "PLI_USE_DEV_LIB", "PLI_FUSION_WAIT_MS")             # read by this package / the C++ adapters


def needs_dev_library(cfg):
    """The development build is the one that knows lsd_mode 1 (the lane relaxation) and the environment switches of tools/README.md."""
    return cfg.lsd_mode == 1 or any(k.startswith("PLI_") and k not in PRODUCT_ENV + PYTHON_ENV for k in os.environ)


def predict_scale(ratio, nlevels, scale_factor):
    """MapPoint::PredictScale (MapPoint.cc:449-464) on ratio = mfMaxDistance / currentDist, a float: ceil(log(ratio) /
    mfLogScaleFactor) with mfLogScaleFactor = (float)log(mfScaleFactor) and the clamps to [0, nlevels).  The logarithm is the
    host's (math.log of the float, in double): the expression an integrator's compiler builds may select logf instead, which is
    why pli_fuse_search takes the thresholds as a table (fuse_level_ratio) and does not evaluate a logarithm itself."""
    import math
    ratio = float(np.float32(ratio))
    if not ratio > 0.0:
        return 0
    if math.isinf(ratio):
        return nlevels - 1
    log_sf = float(np.float32(math.log(float(np.float32(scale_factor)))))
    n = math.ceil(math.log(ratio) / log_sf)
    return 0 if n < 0 else nlevels - 1 if n >= nlevels else int(n)


def fuse_level_ratio(nlevels, scale_factor, level_fn=None):
    """level_ratio of pli_fuse_search: for n = 0 .. nlevels-2 the largest float r for which the host's PredictScale expression
    (level_fn(r), default predict_scale) gives a level <= n, by bisection over the bit patterns of the positive floats (the
    expression does not decrease with r).  The level of a ratio is then the number of n with ratio > level_ratio[n]."""
    fn = level_fn or (lambda r: predict_scale(r, nlevels, scale_factor))
    as_float = lambda bits: np.array([bits], np.uint32).view(np.float32)[0]
    out = np.zeros(max(nlevels - 1, 0), np.float32)
    for n in range(nlevels - 1):
        lo, hi = 1, 0x7F800000                      # the smallest subnormal: level 0; +inf: the top level
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fn(as_float(mid)) <= n:
                lo = mid
            else:
                hi = mid
        out[n] = as_float(lo)
    return out


def pack_keyframes(kfs, spec, what):
    """The flat per-feature tables of a batch of keyframes, as the batched searches take them.  kfs: one tuple per keyframe;
    spec: (position in the tuple, dtype, trailing shape) of each per-feature column.  Returns (off, columns): keyframe k is rows
    off[k] .. off[k + 1] (int32, off[0] = 0) of every column, each C-contiguous of shape (total,) + trailing shape.  A keyframe
    whose columns disagree in length raises ValueError(what)."""
    off = np.zeros(len(kfs) + 1, np.int32)
    parts = [[] for _ in spec]
    for k, kf in enumerate(kfs):
        cols = [np.asarray(kf[i], dt).reshape((-1,) + tuple(tail)) for i, dt, tail in spec]
        if any(len(col) != len(cols[0]) for col in cols):
            raise ValueError(what)
        off[k + 1] = off[k] + len(cols[0])
        for p, col in zip(parts, cols):
            p.append(col)
    return off, [np.ascontiguousarray(np.concatenate(p) if p else np.zeros((0,) + tuple(tail), dt), dt)
                 for p, (_, dt, tail) in zip(parts, spec)]


BOW_COLUMNS = ((0, np.uint8, (32,)), (1, np.float32, ()), (2, np.int32, ()), (3, np.uint8, ()))      # desc, angle, node, valid
TRI_COLUMNS = ((0, KEYPOINT_DT, ()), (1, np.uint8, (32,)), (2, np.int32, ()), (3, np.uint8, ()), (4, np.uint8, ()))
# kp, desc, node, has_mp, uright, depth, mvKeys[i].pt
NEWPT_COLUMNS = TRI_COLUMNS[:4] + ((4, np.float32, ()), (5, np.float32, ()), (6, np.float32, (2,)))
FUSE_COLUMNS = ((0, KEYPOINT_DT, ()), (1, np.uint8, (32,)), (2, np.float32, ()))                     # kp, desc, uright


class Frontend:
    """One pli_ctx: device buffers + stream for up to `max_frames` stereo frames."""

    def __init__(self, cfg, device=0, dev=None):
        """dev: the development build of the library (libpli_frontend_dev.so) instead of the product one; None = the product build
        unless the configuration or the environment asks for something only the development build has (the dev-switch tests and
        tools).  bench.py passes False: its line is the product library's."""
        self.cfg = cfg
        self.dev = needs_dev_library(cfg) if dev is None else bool(dev)
        self.L = capi.lib(dev=self.dev)
        self.h = C.c_void_p()
        check(self.L.pli_ctx_create(C.byref(cfg), device, C.byref(self.h)))
        self.layout = capi.TableLayout()
        check(self.L.pli_ctx_layout(self.h, C.byref(self.layout)))
        self.kp_cap = self.layout.kp_cap
        self.kl_cap = self.layout.kl_cap
        self.image_format, self.channels = capi.IMAGE_GRAY8, 1
        self.depth_type, self.depth_scale = capi.DEPTH_F32, np.float32(1)

    # ---- the GrabImage conversions (Tracking.cc:889-914, :964-980, :1014-1027) on the device -------------
    def set_image_format(self, fmt):
        """pli_set_image_format: every image helper below then takes (H, W, 3) (capi.IMAGE_RGB8 / IMAGE_BGR8) or (H, W, 4) (IMAGE_RGBA8 /
        IMAGE_BGRA8) u8 arrays, rows possibly padded, and level 0 of the pyramid is OpenCV 3.3.1's RGB2Gray<uchar> of them; IMAGE_GRAY8 (the
        default) takes (H, W) arrays as before."""
        fmt = int(fmt)
        check(self.L.pli_set_image_format(self.h, fmt))
        self.image_format, self.channels = fmt, capi.IMAGE_CHANNELS[fmt]

    def set_depth_format(self, type, scale=1.0):
        """pli_set_depth_format: stereo_from_depth and frame_extract_single then take uint16 depth maps (capi.DEPTH_U16) or float ones
        (capi.DEPTH_F32) and see element * scale (float) at each keypoint: imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) without a
        pass over the frame."""
        type, scale = int(type), np.float32(scale)
        check(self.L.pli_set_depth_format(self.h, type, float(scale)))
        self.depth_type, self.depth_scale = type, scale

    def _image(self, img):
        return _u8(img) if self.channels == 1 else _colour_u8(img, self.channels)

    def _depth(self, depth):
        """The depth map as the library reads it under the depth format that is set: (height, stride >= width), contiguous."""
        dt = np.uint16 if self.depth_type == capi.DEPTH_U16 else np.float32
        if self.depth_type == capi.DEPTH_U16 and np.asarray(depth).dtype != np.uint16:
            raise ValueError("uint16 depth map expected under DEPTH_U16")
        return np.ascontiguousarray(depth, dt)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.pli_ctx_destroy(self.h)
            self.h = C.c_void_p()
        for p in getattr(self, "_pinned", []):
            self.L.pli_host_free(p)
        self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- per-call drop-ins -------------------------------------------------
    def orb_extract(self, eye, image):
        """ORBextractor::operator(); returns (n, keypoints, descriptors). n = -1 for an empty image."""
        if image is None or getattr(image, "size", 0) == 0:
            n = C.c_int32()
            st = self.L.pli_orb_extract(self.h, eye, None, 0, 0, 0, None, 0, None, C.byref(n))
            if st != -2:
                check(st)
            return -1, np.zeros(0, KEYPOINT_DT), np.zeros((0, 32), np.uint8)
        image = self._image(image)
        kp = np.zeros(self.kp_cap, KEYPOINT_DT)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        n = C.c_int32()
        check(self.L.pli_orb_extract(self.h, eye, ptr(image), image.shape[1], image.shape[0], image.strides[0],
                                     ptr(kp), self.kp_cap, ptr(desc), C.byref(n)))
        return n.value, kp[:n.value].copy(), desc[:n.value].copy()

    def pyramid_level(self, eye, level):
        w, h = C.c_int32(), C.c_int32()
        check(self.L.pli_orb_pyramid_level(self.h, eye, level, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        check(self.L.pli_orb_pyramid_level(self.h, eye, level, ptr(out), out.size, C.byref(w), C.byref(h)))
        return out

    def line_extract(self, eye, image):
        """Lineextractor::operator(); returns (n, keylines, descriptors)."""
        image = self._image(image)
        kl = np.zeros(self.kl_cap, KEYLINE_DT)
        desc = np.zeros((self.kl_cap, 32), np.uint8)
        n = C.c_int32()
        check(self.L.pli_line_extract(self.h, eye, ptr(image), image.shape[1], image.shape[0], image.strides[0],
                                      ptr(kl), self.kl_cap, ptr(desc), C.byref(n)))
        return n.value, kl[:n.value].copy(), desc[:n.value].copy()

    def compute_stereo_matches(self):
        """Frame::ComputeStereoMatches: (mvuRight, mvDepth) for the left keypoints."""
        ur = np.zeros(self.kp_cap, np.float32)
        dp = np.zeros(self.kp_cap, np.float32)
        check(self.L.pli_stereo_match_points(self.h, ptr(ur), ptr(dp), self.kp_cap))
        return ur, dp

    def compute_stereo_matches_lines(self):
        """Frame::ComputeStereoMatches_Lines: (mvDisparity_l [n,2], mvle_l [n,3])."""
        disp = np.zeros((self.kl_cap, 2), np.float32)
        le = np.zeros((self.kl_cap, 3), np.float64)
        check(self.L.pli_stereo_match_lines(self.h, ptr(disp), ptr(le), self.kl_cap))
        return disp, le

    # ---- stateless matchers --------------------------------------------------
    def descriptor_distance(self, a, b):
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        out = np.zeros(a.shape[0], np.int32)
        check(self.L.pli_descriptor_distance(self.h, ptr(a), ptr(b), a.shape[0], ptr(out)))
        return out

    def knn2(self, q, t):
        q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
        idx = np.zeros((q.shape[0], 2), np.int32)
        dist = np.zeros((q.shape[0], 2), np.int32)
        check(self.L.pli_hamming_knn2(self.h, ptr(q), q.shape[0], ptr(t), t.shape[0], ptr(idx), ptr(dist)))
        return idx, dist

    def match(self, desc1, desc2, nnr):
        """int match(desc1, desc2, nnr, matches_12): returns (nmatches, matches_12)."""
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        m = np.full(d1.shape[0], -1, np.int32)
        n = C.c_int32()
        check(self.L.pli_match_lines(self.h, ptr(d1), d1.shape[0], ptr(d2), d2.shape[0], nnr, ptr(m), C.byref(n)))
        return n.value, m

    def search_by_projection(self, queries, qdesc, cur_kp, cur_desc, cur_uright, bounds, check_orientation=True, occupied=None,
                             with_raw=False):
        """pli_search_by_projection; `occupied`: per current keypoint, holds a map point with observations before the call;
        with_raw: also the matches before the rotation filter (n, best, raw)."""
        q = np.ascontiguousarray(queries, PROJ_QUERY_DT)
        qd = np.ascontiguousarray(qdesc, np.uint8)
        kp = np.ascontiguousarray(cur_kp, KEYPOINT_DT)
        de = np.ascontiguousarray(cur_desc, np.uint8)
        ur = np.ascontiguousarray(cur_uright, np.float32)
        best = np.full(q.shape[0], -1, np.int32)
        raw = np.full(q.shape[0], -1, np.int32) if with_raw else None
        oc = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        n = C.c_int32()
        check(self.L.pli_search_by_projection(self.h, ptr(q), ptr(qd), q.shape[0], ptr(kp), ptr(de), ptr(ur),
                                              None if oc is None else ptr(oc), kp.shape[0], bounds[0], bounds[1], bounds[2],
                                              bounds[3], int(check_orientation), ptr(best), None if raw is None else ptr(raw),
                                              C.byref(n)))
        return (n.value, best, raw) if with_raw else (n.value, best)

    def vocab_create(self, k, L, parent, is_leaf, desc, weight):
        """DBoW2 vocabulary (node list as in ORBvoc.txt); returns an opaque handle for bow_transform."""
        parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8); weight = np.ascontiguousarray(weight, np.float64)
        h = C.c_void_p()
        check(self.L.pli_vocab_create(self.h, k, L, parent.shape[0], ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight), C.byref(h)))
        return h

    def vocab_destroy(self, h):
        self.L.pli_vocab_destroy(h)

    def bow_transform(self, vocab, desc, levelsup=4):
        """Per-feature descent of DBoW2's transform(): (word_id, weight, node_id) arrays."""
        d = np.ascontiguousarray(desc, np.uint8)
        n = d.shape[0]
        word = np.zeros(n, np.int32); weight = np.zeros(n, np.float64); node = np.zeros(n, np.int32)
        check(self.L.pli_bow_transform(self.h, vocab, ptr(d), n, levelsup, ptr(word), ptr(weight), ptr(node)))
        return word, weight, node

    # ---- the keyframe database (KeyFrameDatabase's place-recognition queries) ----
    def kfdb_create(self):
        """A keyframe database on this context's device; destroy it (kfdb_destroy) before the context."""
        h = C.c_void_p()
        check(self.L.pli_kfdb_create(self.h, C.byref(h)))
        return h

    def kfdb_destroy(self, db):
        self.L.pli_kfdb_destroy(db)

    def kfdb_add(self, db, word, value):
        """KeyFrameDatabase::add of one BowVector (word ids strictly ascending, as the std::map iterates); returns its slot."""
        w = np.ascontiguousarray(word, np.uint32).reshape(-1)
        v = np.ascontiguousarray(value, np.float64).reshape(-1)
        if len(w) != len(v):
            raise ValueError("one value per word")
        slot = C.c_int32(-1)
        check(self.L.pli_kfdb_add(self.h, db, ptr(w), ptr(v), len(w), C.byref(slot)))
        return slot.value

    def kfdb_erase(self, db, slot):
        check(self.L.pli_kfdb_erase(self.h, db, int(slot)))

    def kfdb_clear(self, db):
        check(self.L.pli_kfdb_clear(self.h, db))

    def kfdb_stats(self, db):
        """struct pli_kfdb_stats as a dict."""
        st = capi.KfdbStats()
        check(self.L.pli_kfdb_stats(db, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in capi.KfdbStats._fields_}

    def kfdb_query(self, db, qword, qvalue, nslots=None):
        """One query BowVector against every slot: (common int32[nslots], first int32[nslots], score float64[nslots]); first is
        the index in the query vector of the first shared word (-1: none), score the reference's L1 score as its double.
        nslots: the caller's idea of the slot high-water mark (default: the database's own)."""
        w = np.ascontiguousarray(qword, np.uint32).reshape(-1)
        v = np.ascontiguousarray(qvalue, np.float64).reshape(-1)
        if len(w) != len(v):
            raise ValueError("one value per word")
        if nslots is None:
            nslots = self.kfdb_stats(db)["slot_high_water"]
        common = np.zeros(nslots, np.int32); first = np.zeros(nslots, np.int32); score = np.zeros(nslots, np.float64)
        check(self.L.pli_kfdb_query(self.h, db, ptr(w), ptr(v), len(w), nslots, ptr(common), ptr(first), ptr(score)))
        return common, first, score

    def distinctive_descriptors(self, groups):
        """MapPoint / MapLine::ComputeDistinctiveDescriptors (MapPoint.cc:300-365, MapLine.cc:246-317) of every feature of `groups`
        in one call.  groups: a list of (N_p, 32) uint8 arrays, the descriptors that observe feature p in the reference's order.
        Returns (best int32[nfeat], best_median int32[nfeat], row_median int32[total rows]): best[p] is the lowest row of group p
        with the least lower-median distance to the group's rows (-1 for an empty group), best_median[p] that median (INT32_MAX
        for an empty group), row_median the median of every row, the groups one after another."""
        off, (desc,) = pack_keyframes([(g,) for g in groups], ((0, np.uint8, (32,)),), "a group is (N, 32) uint8")
        nfeat = len(groups)
        best = np.zeros(nfeat, np.int32); best_median = np.zeros(nfeat, np.int32); row_median = np.zeros(int(off[-1]), np.int32)
        check(self.L.pli_distinctive_descriptors(self.h, ptr(desc), ptr(off), nfeat, ptr(best), ptr(best_median), ptr(row_median)))
        return best, best_median, row_median

    def search_by_bow(self, f_desc, f_angle, f_node, kfs, nnratio=0.75, check_orientation=True):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:269-470, F.Nleft == -1) of every keyframe of `kfs`
        against one frame, in one call.  kfs: list of (desc, angle, node, valid) per keyframe; node = the FeatureVector node that
        lists a feature (-1: none), valid = its map point is set and not bad.  Returns (matches[nkf, nf]: the keyframe feature
        each frame feature is matched to or -1, nmatches[nkf])."""
        fd = np.ascontiguousarray(f_desc, np.uint8).reshape(-1, 32)
        nf = fd.shape[0]
        fa = np.ascontiguousarray(f_angle, np.float32).reshape(nf)
        fn = np.ascontiguousarray(f_node, np.int32).reshape(nf)
        nkf = len(kfs)
        off, (kd, ka, kn, kv) = pack_keyframes(kfs, BOW_COLUMNS, "every keyframe needs one angle, node and valid flag per descriptor")
        matches = np.full((nkf, nf), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        check(self.L.pli_search_by_bow(self.h, nkf, ptr(off), ptr(kd), ptr(ka), ptr(kn), ptr(kv), ptr(fd), ptr(fa), ptr(fn), nf,
                                       nnratio, int(check_orientation), ptr(matches), ptr(nmatches)))
        return matches, nmatches

    def search_by_bow_two_cameras(self, kfs, f_desc, f_angle, f_node, f_nleft, nnratio=0.7, check_orientation=True):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:269-470), the branch F.Nleft != -1 (:342-369,
        :403-432: a frame of two KannalaBrandt8 cameras), of every keyframe of `kfs` against one frame, in one call.  Tables as in
        search_by_bow; f_nleft = F.Nleft, the frame's rows are the left camera's first; the angles are the caller's choice
        (kf: mvKeysUn, or mvKeys / mvKeysRight by NLeft, :379-382; frame: mvKeys / mvKeysRight by Nleft, :386-389, :416-419).
        Per keyframe feature the left candidates (< f_nleft) and the right ones keep a best and a second best each; only if
        bestDist1 <= TH_LOW the left match is taken on its ratio test and the right one when bestDist1R <= TH_LOW, without a
        ratio test (:373-433).  Returns (matches[nkf, nf], nmatches[nkf])."""
        fd = np.ascontiguousarray(f_desc, np.uint8).reshape(-1, 32)
        nf = fd.shape[0]
        fa = np.ascontiguousarray(f_angle, np.float32).reshape(nf)
        fn = np.ascontiguousarray(f_node, np.int32).reshape(nf)
        nkf = len(kfs)
        off, (kd, ka, kn, kv) = pack_keyframes(kfs, BOW_COLUMNS, "every keyframe needs one angle, node and valid flag per descriptor")
        matches = np.full((nkf, nf), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        check(self.L.pli_search_by_bow_two_cameras(self.h, nkf, ptr(off), ptr(kd), ptr(ka), ptr(kn), ptr(kv), ptr(fd), ptr(fa),
                                                   ptr(fn), nf, int(f_nleft), nnratio, int(check_orientation), ptr(matches),
                                                   ptr(nmatches)))
        return matches, nmatches

    def search_by_bow_kf(self, desc1, angle1, node1, valid1, kfs, nnratio=0.75, check_orientation=True):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:823-963, NLeft == -1) of keyframe 1 against every
        keyframe of `kfs`, in one call (loop closing).  desc1 / angle1 / node1 / valid1 and each (desc, angle, node, valid) of
        kfs as in search_by_bow; the map-point gate holds on both sides.  Returns (matches12[nkf, n1]: the row of keyframe k that
        feature i of keyframe 1 is matched to or -1, nmatches[nkf])."""
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        n1 = d1.shape[0]
        a1 = np.ascontiguousarray(angle1, np.float32).reshape(n1)
        nd1 = np.ascontiguousarray(node1, np.int32).reshape(n1)
        v1 = np.ascontiguousarray(valid1, np.uint8).reshape(n1)
        nkf = len(kfs)
        off, (kd, ka, kn, kv) = pack_keyframes(kfs, BOW_COLUMNS, "every keyframe needs one angle, node and valid flag per descriptor")
        matches = np.full((nkf, n1), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        check(self.L.pli_search_by_bow_kf(self.h, ptr(d1), ptr(a1), ptr(nd1), ptr(v1), n1, nkf, ptr(off), ptr(kd), ptr(ka), ptr(kn),
                                          ptr(kv), nnratio, int(check_orientation), ptr(matches), ptr(nmatches)))
        return matches, nmatches

    def search_for_triangulation(self, kf1, kfs, only_stereo=False, coarse=False, check_orientation=False):
        """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:965-1206, no
        second cameras) of keyframe `kf1` against every neighbour of `kfs`, in one call.  kf1: (kp, desc, node, has_mp, stereo) -
        mvKeysUn as KEYPOINT_DT rows, descriptors, the FeatureVector node that lists a feature (-1: none), map point set,
        mvuRight >= 0; kfs: list of (kp, desc, node, has_mp, stereo, F12, ep) per neighbour, F12 = the 3 x 3 matrix of
        Pinhole::epipolarConstrain, ep = the epipole in the neighbour's image.  Returns (matches12[nkf, n1]: the neighbour's
        feature that feature i of kf1 is matched to or -1, nmatches[nkf])."""
        what = "every feature needs one keypoint, descriptor, node, has_mp and stereo flag"
        k1, d1, n1, m1, s1 = pack_keyframes([kf1], TRI_COLUMNS, what)[1]
        nkf = len(kfs)
        off, (kk, kd, kn, km, ks) = pack_keyframes(kfs, TRI_COLUMNS, what)
        f12 = np.ascontiguousarray([np.asarray(kf[5], np.float32).reshape(9) for kf in kfs], np.float32).reshape(nkf, 9)
        ep = np.ascontiguousarray([np.asarray(kf[6], np.float32).reshape(2) for kf in kfs], np.float32).reshape(nkf, 2)
        matches = np.full((nkf, len(n1)), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        check(self.L.pli_search_for_triangulation(self.h, ptr(k1), ptr(d1), ptr(n1), ptr(m1), ptr(s1), len(n1), nkf, ptr(off),
                                                  ptr(kk), ptr(kd), ptr(kn), ptr(km), ptr(ks), ptr(f12), ptr(ep),
                                                  int(only_stereo), int(coarse), int(check_orientation), ptr(matches),
                                                  ptr(nmatches)))
        return matches, nmatches

    def search_for_triangulation_two_cameras(self, kf1, kfs, cam_left, cam_right, coarse=False, check_orientation=False,
                                             only_stereo=False):
        """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:965-1206), the branch of keyframes with two KannalaBrandt8 cameras
        (mpCamera2 set, NLeft != -1), of keyframe `kf1` against every neighbour of `kfs`, in one call.  kf1: (kp, desc, node,
        has_mp, nleft) - mvKeys then mvKeysRight as KEYPOINT_DT rows, mDescriptors, the FeatureVector node that lists a feature
        (-1: none), map point set, NLeft; kfs: list of (kp, desc, node, has_mp, nleft, rel[4, 12]) per neighbour, rel = the
        relative poses ll, lr, rl, rr (R12 row major, then t12).  cam_left / cam_right: the 8 KannalaBrandt8 parameters of
        mpCamera / mpCamera2.  Returns (matches12[nkf, n1]: the neighbour's feature, over its N, that feature i of kf1 is matched
        to or -1, nmatches[nkf])."""
        what = "every feature needs one keypoint, descriptor, node and has_mp flag"
        k1, d1, n1, m1 = pack_keyframes([kf1], TRI_COLUMNS[:4], what)[1]
        nkf = len(kfs)
        off, (kk, kd, kn, km) = pack_keyframes(kfs, TRI_COLUMNS[:4], what)
        nleft = np.ascontiguousarray([int(kf[4]) for kf in kfs], np.int32).reshape(nkf)
        rel = np.ascontiguousarray([np.asarray(kf[5], np.float32).reshape(48) for kf in kfs], np.float32).reshape(nkf, 48)
        cl, cr = np.ascontiguousarray(cam_left, np.float32).reshape(8), np.ascontiguousarray(cam_right, np.float32).reshape(8)
        matches = np.full((nkf, len(n1)), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        check(self.L.pli_search_for_triangulation_two_cameras(self.h, ptr(k1), ptr(d1), ptr(n1), ptr(m1), len(n1), int(kf1[4]), nkf,
                                                              ptr(off), ptr(nleft), ptr(kk), ptr(kd), ptr(kn), ptr(km), ptr(cl),
                                                              ptr(cr), ptr(rel), int(only_stereo), int(coarse),
                                                              int(check_orientation), ptr(matches), ptr(nmatches)))
        return matches, nmatches

    def create_new_map_points(self, kf1, kfs, cam, mb, ratio_factor, coarse=False, far_points=False, th_far=0.0):
        """LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684, keyframes of one pinhole camera) of
        keyframe `kf1` against every neighbour of `kfs`, in one call (include/pli_frontend.h pli_create_new_map_points).
        kf1: (kp, desc, node, has_mp, uright, depth, key, pose) - mvKeysUn as KEYPOINT_DT rows, mDescriptors, the FeatureVector
        node that lists a feature (-1: none), map point set, mvuRight, mvDepth, mvKeys[i].pt (n x 2), pose = 15 floats (Rcw row
        major, tcw, Ow); kfs: list of (kp, desc, node, has_mp, uright, depth, key, pose, F12, ep) per neighbour.  cam:
        capi.FuseCamera or its 9 values (fx, fy, cx, cy, bf are read); mb; ratio_factor = 1.5f * mfScaleFactor in float.
        Returns (matches12[nkf, n1], nmatches[nkf], status[nkf, n1] (capi.NEWPT_*), x3d[nkf, n1, 3], nnew[nkf]): what the
        reference's sequential loop sees and creates at neighbour k."""
        what = "every feature needs one keypoint, descriptor, node, has_mp flag, uright, depth and mvKeys point"
        k1, d1, n1, m1, u1, z1, p1 = pack_keyframes([kf1], NEWPT_COLUMNS, what)[1]
        nkf = len(kfs)
        off, (kk, kd, kn, km, ku, kz, kp) = pack_keyframes(kfs, NEWPT_COLUMNS, what)
        pose1 = np.ascontiguousarray(kf1[7], np.float32).reshape(15)
        pose = np.ascontiguousarray([np.asarray(kf[7], np.float32).reshape(15) for kf in kfs], np.float32).reshape(nkf, 15)
        f12 = np.ascontiguousarray([np.asarray(kf[8], np.float32).reshape(9) for kf in kfs], np.float32).reshape(nkf, 9)
        ep = np.ascontiguousarray([np.asarray(kf[9], np.float32).reshape(2) for kf in kfs], np.float32).reshape(nkf, 2)
        if not isinstance(cam, capi.FuseCamera):
            cam = capi.FuseCamera(*[float(v) for v in cam])
        n = len(n1)
        matches = np.full((nkf, n), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        status = np.full((nkf, n), capi.NEWPT_NOT_MATCHED, np.int32)
        x3d = np.zeros((nkf, n, 3), np.float32)
        nnew = np.zeros(nkf, np.int32)
        check(self.L.pli_create_new_map_points(self.h, ptr(k1), ptr(d1), ptr(n1), ptr(m1), ptr(u1), ptr(z1), ptr(p1), n, nkf,
                                               ptr(off), ptr(kk), ptr(kd), ptr(kn), ptr(km), ptr(ku), ptr(kz), ptr(kp), ptr(f12),
                                               ptr(ep), ptr(pose1), ptr(pose), C.byref(cam), float(mb), int(coarse),
                                               int(far_points), float(th_far), float(ratio_factor), ptr(matches), ptr(nmatches),
                                               ptr(status), ptr(x3d), ptr(nnew)))
        return matches, nmatches, status, x3d, nnew

    def create_new_map_points_two_cameras(self, kf1, kfs, cam_left, cam_right, ratio_factor, coarse=False, far_points=False,
                                          th_far=0.0):
        """LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684), the branch of keyframes with two
        KannalaBrandt8 cameras (:463-528), of keyframe `kf1` against every neighbour of `kfs`, in one call
        (include/pli_frontend.h pli_create_new_map_points_two_cameras).  kf1: (kp, desc, node, has_mp, nleft, pose[2, 15]) - the
        tables of search_for_triangulation_two_cameras and per side (left, right) Rcw row major, tcw, Ow; kfs: list of
        (kp, desc, node, has_mp, nleft, pose[2, 15], rel[4, 12]) per neighbour.  cam_left / cam_right: the 8 KannalaBrandt8
        parameters of mpCamera / mpCamera2; ratio_factor = 1.5f * mfScaleFactor in float.
        Returns (matches12[nkf, n1], nmatches[nkf], status[nkf, n1] (capi.NEWPT_*), x3d[nkf, n1, 3], nnew[nkf]) as
        create_new_map_points."""
        what = "every feature needs one keypoint, descriptor, node and has_mp flag"
        k1, d1, n1, m1 = pack_keyframes([kf1], TRI_COLUMNS[:4], what)[1]
        nkf = len(kfs)
        off, (kk, kd, kn, km) = pack_keyframes(kfs, TRI_COLUMNS[:4], what)
        nleft = np.ascontiguousarray([int(kf[4]) for kf in kfs], np.int32).reshape(nkf)
        pose1 = np.ascontiguousarray(kf1[5], np.float32).reshape(30)
        pose = np.ascontiguousarray([np.asarray(kf[5], np.float32).reshape(30) for kf in kfs], np.float32).reshape(nkf, 30)
        rel = np.ascontiguousarray([np.asarray(kf[6], np.float32).reshape(48) for kf in kfs], np.float32).reshape(nkf, 48)
        cl, cr = np.ascontiguousarray(cam_left, np.float32).reshape(8), np.ascontiguousarray(cam_right, np.float32).reshape(8)
        n = len(n1)
        matches = np.full((nkf, n), -1, np.int32)
        nmatches = np.zeros(nkf, np.int32)
        status = np.full((nkf, n), capi.NEWPT_NOT_MATCHED, np.int32)
        x3d = np.zeros((nkf, n, 3), np.float32)
        nnew = np.zeros(nkf, np.int32)
        check(self.L.pli_create_new_map_points_two_cameras(self.h, ptr(k1), ptr(d1), ptr(n1), ptr(m1), n, int(kf1[4]), nkf, ptr(off),
                                                           ptr(nleft), ptr(kk), ptr(kd), ptr(kn), ptr(km), ptr(cl), ptr(cr),
                                                           ptr(rel), ptr(pose1), ptr(pose), int(coarse), int(far_points),
                                                           float(th_far), float(ratio_factor), ptr(matches), ptr(nmatches),
                                                           ptr(status), ptr(x3d), ptr(nnew)))
        return matches, nmatches, status, x3d, nnew

    def _level_ratio(self, level_ratio):
        """The level_ratio table of the projection searches: the caller's, or this host's (fuse_level_ratio), made once."""
        if level_ratio is None:
            if getattr(self, "_fuse_level_ratio", None) is None:
                self._fuse_level_ratio = fuse_level_ratio(self.cfg.orb_nlevels, self.cfg.orb_scale_factor)
            level_ratio = self._fuse_level_ratio
        level_ratio = np.ascontiguousarray(level_ratio, np.float32)
        if len(level_ratio) != self.cfg.orb_nlevels - 1:
            raise ValueError("level_ratio: orb_nlevels - 1 thresholds")
        return level_ratio

    def fuse_search(self, points, descs, keyframes, cam, th=3.0, reproj_gate=True, skip=None, level_ratio=None):
        """The search half of ORBmatcher::Fuse (ORBmatcher.cc:1399-1609 without second cameras; reproj_gate=False: the Sim3
        overload :1611-1733) of the map points `points` (capi.FUSE_POINT_DT rows) with descriptors `descs` against every keyframe
        of `keyframes`, in one call.  keyframes: list of (kp, desc, uright, pose) - mvKeysUn as KEYPOINT_DT rows, mDescriptors,
        mvuRight, pose = 15 floats (Rcw row major, tcw, Ow); cam: capi.FuseCamera or its 9 values; skip: nkf x nmp, != 0 leaves a
        pair out (IsInKeyFrame).  Returns (best_idx[nkf, nmp]: the keyframe's row or -1, best_dist[nkf, nmp])."""
        pts = np.ascontiguousarray(points, capi.FUSE_POINT_DT).reshape(-1)
        d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        if len(d) != len(pts):
            raise ValueError("every map point needs one descriptor")
        nkf, nmp = len(keyframes), len(pts)
        off, (kk, kd, ku) = pack_keyframes(keyframes, FUSE_COLUMNS, "every feature needs one keypoint, descriptor and uright")
        pose = np.ascontiguousarray([np.asarray(kf[3], np.float32).reshape(15) for kf in keyframes], np.float32).reshape(nkf, 15)
        if not isinstance(cam, capi.FuseCamera):
            cam = capi.FuseCamera(*[float(v) for v in cam])
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
            if skip.shape != (nkf, nmp):
                raise ValueError("skip: nkf x nmp")
        level_ratio = self._level_ratio(level_ratio)
        best_idx = np.full((nkf, nmp), -1, np.int32)
        best_dist = np.full((nkf, nmp), 256, np.int32)
        check(self.L.pli_fuse_search(self.h, ptr(pts), ptr(d), nmp, nkf, ptr(off), ptr(kk), ptr(kd), ptr(ku), ptr(pose),
                                     ptr(skip), C.byref(cam), float(th), ptr(level_ratio), int(reproj_gate), ptr(best_idx),
                                     ptr(best_dist)))
        return best_idx, best_dist

    def fuse_search_two_cameras(self, points, descs, keyframes, cam_left, cam_right, bounds, th=3.0, sides=3, skip=None,
                                level_ratio=None):
        """The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (ORBmatcher.cc:1399-1609) for keyframes with two
        KannalaBrandt8 cameras (NLeft != -1), both values of bRight (LocalMapping.cc:747-748, :776-777) of every keyframe of
        `keyframes` in one call.  points / descs as in fuse_search; keyframes: list of (kp, desc, nleft, pose) - mvKeys then
        mvKeysRight as KEYPOINT_DT rows (:1524-1526), mDescriptors, NLeft, pose = 2 x 15 floats, left then right (Rcw row major,
        tcw, Ow; the right one from GetRightRotation() / GetRightTranslation() / GetRightCameraCenter(), KeyFrame.cc:1343-1373);
        cam_left / cam_right: the 8 KannalaBrandt8 parameters of mpCamera / mpCamera2; bounds: (mnMinX, mnMaxX, mnMinY, mnMaxY);
        sides: bit 0 = left, bit 1 = right; skip: nkf x 2 x nmp, != 0 leaves a (keyframe, side, point) out (IsInKeyFrame, :1448).
        The chi-square gate is the monocular one, 5.99 (:1555): every mvuRight of such a keyframe is -1 (Frame.cc:1589).
        Returns (best_idx[nkf, 2, nmp]: the row over the keyframe's N - a right row is its camera-local row + NLeft, :1559 - or
        -1, best_dist[nkf, 2, nmp])."""
        pts = np.ascontiguousarray(points, capi.FUSE_POINT_DT).reshape(-1)
        d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        if len(d) != len(pts):
            raise ValueError("every map point needs one descriptor")
        nkf, nmp = len(keyframes), len(pts)
        off, (kk, kd) = pack_keyframes(keyframes, FUSE_COLUMNS[:2], "every feature needs one keypoint and one descriptor")
        nleft = np.ascontiguousarray([int(kf[2]) for kf in keyframes], np.int32).reshape(nkf)
        pose = np.ascontiguousarray([np.asarray(kf[3], np.float32).reshape(30) for kf in keyframes], np.float32).reshape(nkf, 30)
        cl, cr = np.ascontiguousarray(cam_left, np.float32).reshape(8), np.ascontiguousarray(cam_right, np.float32).reshape(8)
        min_x, max_x, min_y, max_y = (float(v) for v in bounds)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
            if skip.shape != (nkf, 2, nmp):
                raise ValueError("skip: nkf x 2 x nmp")
        level_ratio = self._level_ratio(level_ratio)
        best_idx = np.full((nkf, 2, nmp), -1, np.int32)
        best_dist = np.full((nkf, 2, nmp), 256, np.int32)
        check(self.L.pli_fuse_search_two_cameras(self.h, ptr(pts), ptr(d), nmp, nkf, ptr(off), ptr(nleft), ptr(kk), ptr(kd),
                                                 ptr(pose), ptr(skip), ptr(cl), ptr(cr), min_x, max_x, min_y, max_y, float(th),
                                                 ptr(level_ratio), int(sides), ptr(best_idx), ptr(best_dist)))
        return best_idx, best_dist

    def search_by_projection_sim3(self, points, descs, pairs, cam, th=3.0, ratio_hamming=1.0, project_form=0, skip=None,
                                  level_ratio=None):
        """Loop closing's ORBmatcher::SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th,
        ratioHamming) (ORBmatcher.cc:473-704) of ONE list of map points `points` (capi.FUSE_POINT_DT rows, descriptors `descs`)
        against every (keyframe, Scw) pair of `pairs`, in one call; the points of a pair are decided in list order and a row taken
        by one is closed to the later ones.  pairs: list of (kp, desc, pose[, occupied]) - mvKeysUn as KEYPOINT_DT rows,
        mDescriptors, pose = 15 floats (Rcw row major, tcw, Ow, decomposed from Scw), occupied = one flag per row (vpMatched[idx]
        != NULL at entry; absent or None: none).  cam: capi.FuseCamera or its 9 values; skip: npair x nmp, != 0 leaves a point out
        of a pair (spAlreadyFound); project_form: 0 = Pinhole::project (:519), 1 = the inverse-depth form (:631-636).
        Returns (row_point: one int32 array per pair, the point that took each row or -1; best_idx[npair, nmp]: the row a point
        took or -1; nmatches[npair])."""
        pts = np.ascontiguousarray(points, capi.FUSE_POINT_DT).reshape(-1)
        d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        if len(d) != len(pts):
            raise ValueError("every map point needs one descriptor")
        npair, nmp = len(pairs), len(pts)
        off, (kk, kd) = pack_keyframes(pairs, FUSE_COLUMNS[:2], "every feature needs one keypoint and one descriptor")
        pose = np.ascontiguousarray([np.asarray(p[2], np.float32).reshape(15) for p in pairs], np.float32).reshape(npair, 15)
        occ = None
        if any(len(p) > 3 and p[3] is not None for p in pairs):
            occ = np.zeros(int(off[-1]), np.uint8)
            for k, p in enumerate(pairs):
                if len(p) > 3 and p[3] is not None:
                    o = np.asarray(p[3]).reshape(-1)
                    if len(o) != off[k + 1] - off[k]:
                        raise ValueError("occupied: one flag per keyframe row")
                    occ[off[k]:off[k + 1]] = o != 0
        if not isinstance(cam, capi.FuseCamera):
            cam = capi.FuseCamera(*[float(v) for v in cam])
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
            if skip.shape != (npair, nmp):
                raise ValueError("skip: npair x nmp")
        level_ratio = self._level_ratio(level_ratio)
        rows = np.full(int(off[-1]), -1, np.int32)
        best_idx = np.full((npair, nmp), -1, np.int32)
        nmatches = np.zeros(npair, np.int32)
        check(self.L.pli_search_by_projection_sim3(self.h, ptr(pts), ptr(d), nmp, npair, ptr(off), ptr(kk), ptr(kd), ptr(pose),
                                                   ptr(skip), ptr(occ), C.byref(cam), float(th), ptr(level_ratio),
                                                   float(ratio_hamming), int(project_form), ptr(rows), ptr(best_idx),
                                                   ptr(nmatches)))
        return [rows[off[k]:off[k + 1]] for k in range(npair)], best_idx, nmatches

    def search_by_projection_reloc(self, cands, frame_kp, frame_desc, cam, th=10.0, orb_dist=100, check_orientation=True,
                                   level_ratio=None):
        """Relocalisation's ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2325-2447;
        Tracking.cc:4290, :4304) of ONE frame table (frame_kp: mvKeysUn as KEYPOINT_DT rows, frame_desc: mDescriptors) against
        every candidate of `cands`, in one call; the points of a candidate are decided in list order and a row taken by one is
        closed to the later ones.  cands: list of (points, descs, angles, pose, occupied_or_None) - pKF->GetMapPointMatches() as
        capi.FUSE_POINT_DT rows (valid = set, not bad and not in sAlreadyFound; normal is not read), GetDescriptor() rows,
        pKF->mvKeysUn[i].angle (None without check_orientation), pose = 15 floats (Rcw row major, tcw, Ow = -Rcw.t()*tcw of the
        frame's Tcw for this candidate), occupied = one flag per frame row (mvpMapPoints[i2] != NULL at entry; None: none).
        cam: capi.FuseCamera or its 9 values.
        Returns (row_point[ncand, nf]: the index within the candidate's own list of the point that holds the row after the
        rotation filter or -1; best_idx: one int32 array per candidate, the row a point took before the filter or -1;
        nmatches[ncand])."""
        kk = np.ascontiguousarray(frame_kp, KEYPOINT_DT).reshape(-1)
        kd = np.ascontiguousarray(frame_desc, np.uint8).reshape(-1, 32)
        if len(kk) != len(kd):
            raise ValueError("every frame feature needs one keypoint and one descriptor")
        ncand, nf = len(cands), len(kk)
        check_orientation = bool(check_orientation)
        if check_orientation and any(cd[2] is None for cd in cands):
            raise ValueError("check_orientation needs every candidate's angles")
        lists = [(cd[0], cd[1], cd[2] if check_orientation else np.zeros(len(np.asarray(cd[0]).reshape(-1)), np.float32)) for cd in cands]
        off, (pts, d, ang) = pack_keyframes(lists, ((0, capi.FUSE_POINT_DT, ()), (1, np.uint8, (32,)), (2, np.float32, ())),
                                            "every map point needs one descriptor and one angle")
        pose = np.ascontiguousarray([np.asarray(cd[3], np.float32).reshape(15) for cd in cands], np.float32).reshape(ncand, 15)
        occ = None
        if any(len(cd) > 4 and cd[4] is not None for cd in cands):
            occ = np.zeros((ncand, nf), np.uint8)
            for k, cd in enumerate(cands):
                if len(cd) > 4 and cd[4] is not None:
                    o = np.asarray(cd[4]).reshape(-1)
                    if len(o) != nf:
                        raise ValueError("occupied: one flag per frame row")
                    occ[k] = o != 0
        if not isinstance(cam, capi.FuseCamera):
            cam = capi.FuseCamera(*[float(v) for v in cam])
        level_ratio = self._level_ratio(level_ratio)
        rows = np.full((ncand, nf), -1, np.int32)
        best_idx = np.full(int(off[-1]), -1, np.int32)
        nmatches = np.zeros(ncand, np.int32)
        check(self.L.pli_search_by_projection_reloc(self.h, ncand, ptr(off), ptr(pts), ptr(d), ptr(ang) if check_orientation else None,
                                                    ptr(pose), ptr(kk), ptr(kd), nf, ptr(occ), C.byref(cam), float(th),
                                                    ptr(level_ratio), int(orb_dist), int(check_orientation), ptr(rows),
                                                    ptr(best_idx), ptr(nmatches)))
        return rows, [best_idx[off[k]:off[k + 1]] for k in range(ncand)], nmatches

    def search_for_initialization(self, kp1, desc1, prev_matched, kp2, desc2, bounds, window_size=10, nnratio=0.9,
                                  check_orientation=True):
        """Monocular initialisation's ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
        (ORBmatcher.cc:706-821; Tracking.cc:2109-2110 with window 100) - see pli_search_for_initialization.  kp1 / kp2: mvKeysUn
        of F1 / F2 as KEYPOINT_DT rows, desc1 / desc2: mDescriptors, prev_matched: vbPrevMatched as n1 x (x, y) (not written),
        bounds: (mnMinX, mnMaxX, mnMinY, mnMaxY).
        Returns (nmatches, matches12: vnMatches12 after the rotation filter, raw12: before it with the evictions applied,
        new_prev_matched: a copy of prev_matched with the update :816-818 for the matches that are left)."""
        k1 = np.ascontiguousarray(kp1, KEYPOINT_DT).reshape(-1)
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        k2 = np.ascontiguousarray(kp2, KEYPOINT_DT).reshape(-1)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        pm = np.ascontiguousarray(prev_matched, np.float32).reshape(-1, 2)
        if len(k1) != len(d1) or len(k2) != len(d2):
            raise ValueError("every feature needs one keypoint and one descriptor")
        if len(pm) != len(k1):
            raise ValueError("prev_matched: one point per F1 keypoint")
        n1, n2 = len(k1), len(k2)
        m12 = np.full(n1, -1, np.int32)
        raw = np.full(n1, -1, np.int32)
        n = C.c_int32()
        check(self.L.pli_search_for_initialization(self.h, ptr(k1), ptr(d1), n1, ptr(pm), ptr(k2), ptr(d2), n2, float(bounds[0]),
                                                   float(bounds[1]), float(bounds[2]), float(bounds[3]), int(window_size),
                                                   float(nnratio), int(bool(check_orientation)), ptr(m12), ptr(raw), C.byref(n)))
        new_pm = pm.copy()
        hit = m12 >= 0
        new_pm[hit, 0] = k2["x"][m12[hit]]
        new_pm[hit, 1] = k2["y"][m12[hit]]
        return n.value, m12, raw, new_pm

    def orb_extract_lapping(self, eye, image, lapping):
        """ORBextractor::operator() with vLappingArea = lapping (ORBextractor.cc:1135-1144): (n, mono count, keypoints, descriptors);
        the table keeps the mono-first / lapping-from-the-back order for stereo_fisheye()."""
        image = self._image(image)
        kp = np.zeros(self.kp_cap, KEYPOINT_DT)
        desc = np.zeros((self.kp_cap, 32), np.uint8)
        n, mono = C.c_int32(), C.c_int32()
        check(self.L.pli_orb_extract_lapping(self.h, eye, ptr(image), image.shape[1], image.shape[0], image.strides[0],
                                             int(lapping[0]), int(lapping[1]), ptr(kp), self.kp_cap, ptr(desc), C.byref(n),
                                             C.byref(mono)))
        return n.value, mono.value, kp[:n.value].copy(), desc[:n.value].copy()

    def stereo_fisheye(self, cam1, cam2, Rlr, tlr, nleft, nright):
        """Frame::ComputeStereoFishEyeMatches (Frame.cc:1577-1618): (nMatches, mvLeftToRightMatch, mvRightToLeftMatch, mvDepth,
        mvStereo3Dpoints) on the tables of the last orb_extract_lapping of both eyes.  cam: the 8 KannalaBrandt8 parameters."""
        c1, c2 = np.ascontiguousarray(cam1, np.float32), np.ascontiguousarray(cam2, np.float32)
        R, t = np.ascontiguousarray(Rlr, np.float32).reshape(9), np.ascontiguousarray(tlr, np.float32).reshape(3)
        l2r, r2l = np.zeros(self.kp_cap, np.int32), np.zeros(self.kp_cap, np.int32)
        depth, p3d = np.zeros(self.kp_cap, np.float32), np.zeros((self.kp_cap, 3), np.float32)
        nm = C.c_int32()
        check(self.L.pli_stereo_fisheye(self.h, ptr(c1), ptr(c2), ptr(R), ptr(t), ptr(l2r), self.kp_cap, ptr(r2l), self.kp_cap,
                                        ptr(depth), ptr(p3d), C.byref(nm)))
        return nm.value, l2r[:nleft].copy(), r2l[:nright].copy(), depth[:nleft].copy(), p3d[:nleft].copy()

    def stereo_fisheye_tables(self, kpL, descL, mono_left, kpR, descR, mono_right, cam1, cam2, Rlr, tlr):
        """Frame::ComputeStereoFishEyeMatches on caller tables (mvKeys / mDescriptors / monoLeft, ... of the Frame)."""
        kpL, kpR = np.ascontiguousarray(kpL, KEYPOINT_DT), np.ascontiguousarray(kpR, KEYPOINT_DT)
        descL, descR = np.ascontiguousarray(descL, np.uint8), np.ascontiguousarray(descR, np.uint8)
        c1, c2 = np.ascontiguousarray(cam1, np.float32), np.ascontiguousarray(cam2, np.float32)
        R, t = np.ascontiguousarray(Rlr, np.float32).reshape(9), np.ascontiguousarray(tlr, np.float32).reshape(3)
        nl, nr = kpL.shape[0], kpR.shape[0]
        l2r, r2l = np.zeros(max(nl, 1), np.int32), np.zeros(max(nr, 1), np.int32)
        depth, p3d = np.zeros(max(nl, 1), np.float32), np.zeros((max(nl, 1), 3), np.float32)
        nm = C.c_int32()
        check(self.L.pli_stereo_fisheye_tables(self.h, ptr(kpL), ptr(descL), nl, int(mono_left), ptr(kpR), ptr(descR), nr, int(mono_right),
                                               ptr(c1), ptr(c2), ptr(R), ptr(t), ptr(l2r), ptr(r2l), ptr(depth), ptr(p3d), C.byref(nm)))
        return nm.value, l2r[:nl], r2l[:nr], depth[:nl], p3d[:nl]

    def stereo_from_depth(self, depth, stride=None):
        """Frame::ComputeStereoFromRGBD (Frame.cc:1309): (mvuRight, mvDepth) of the left keypoints from a float depth image.
        stride: row stride of `depth` in floats when its rows are padded ((height, stride) array, the image in the first `width`
        columns).  Both results have kp_cap rows; the rows beyond the keypoint count are not written by the call and stay 0."""
        d = self._depth(depth)
        if stride is None:
            stride = self.cfg.width
        assert stride >= self.cfg.width and d.shape == (self.cfg.height, stride)
        ur = np.zeros(self.kp_cap, np.float32)
        dp = np.zeros(self.kp_cap, np.float32)
        check(self.L.pli_stereo_from_depth(self.h, ptr(d), stride, ptr(ur), ptr(dp), self.kp_cap))
        return ur, dp

    def set_pinhole_distortion(self, cam):
        """The pinhole camera of the single-camera Frames (pli_set_pinhole_distortion): cam = capi.PinholeDistortion or its values
        (fx, fy, cx, cy, k1, k2, p1, p2[, k3]); None removes it.  Returns Frame::ComputeImageBounds (Frame.cc:947-974) as float32
        (mnMinX, mnMaxX, mnMinY, mnMaxY).  With k1 == 0, or without a camera, nothing is undistorted and the bounds are the image's."""
        bounds = (C.c_float * 4)()
        if cam is None:
            check(self.L.pli_set_pinhole_distortion(self.h, None, bounds))
        else:
            if not isinstance(cam, capi.PinholeDistortion):
                v = [float(x) for x in cam]
                if len(v) not in (8, 9):
                    raise ValueError("cam: fx, fy, cx, cy, k1, k2, p1, p2 and optionally k3")
                cam = capi.PinholeDistortion(*(v + [0.0] * (9 - len(v))))
            check(self.L.pli_set_pinhole_distortion(self.h, C.byref(cam), bounds))
        return np.array(bounds, np.float32)

    def undistort_points(self, xy, with_cell=True):
        """cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), K) of Frame::UndistortKeyPoints / UndistortKeyLines (Frame.cc:891,
        :931-932) with the context's camera, on caller points xy (n x 2).  Returns (xy_un float32 [n, 2], cell int32 [n] or None):
        cell = Frame::PosInGrid (:845-855) of each result against the context's bounds, posX * 48 + posY, -1 where it is false."""
        p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = len(p)
        out = np.zeros((n, 2), np.float32)
        cell = np.zeros(n, np.int32) if with_cell else None
        check(self.L.pli_undistort_points(self.h, ptr(p), n, ptr(out), ptr(cell)))
        return out, cell

    def frame_extract_single(self, image, lapping, depth=None):
        """pli_frame_extract_single: the front-end of one monocular (depth=None, Frame.cc:334-448) or RGB-D (:231-331) Frame in one
        submission.  lapping: the area ExtractORB passes ((0, 1000) monocular, (0, 0) RGB-D); depth: float image, (height, stride)
        with stride >= width.  Returns the parsed record (its eye-0 columns: kpL, descL, klL, ldescL, uright, depth, counts) plus
        kp_un [n, 2] (mvKeysUn[i].pt), kl_un [m, 4] (mvKeysUn_Line[i]: start, end), cell [n] (as undistort_points) and n_mono (the
        extractor's return value); "full" holds the call's buffers as written, every row.  Leaves the per-call state of eye 0 behind (pyramid_level, stereo_from_depth)."""
        image = self._image(image)
        d, stride = None, 0
        if depth is not None:
            d = self._depth(depth)
            assert d.ndim == 2 and d.shape[0] == self.cfg.height and d.shape[1] >= self.cfg.width
            stride = d.shape[1]
        rec = np.zeros(int(self.layout.record_bytes), np.uint8)
        kp_un = np.zeros((self.kp_cap, 2), np.float32)
        kl_un = np.zeros((self.kl_cap, 4), np.float32)
        cell = np.zeros(self.kp_cap, np.int32)
        mono = C.c_int32()
        check(self.L.pli_frame_extract_single(self.h, ptr(image), image.shape[1], image.shape[0], image.strides[0], int(lapping[0]),
                                              int(lapping[1]), ptr(d), stride, ptr(rec), ptr(kp_un), ptr(kl_un), ptr(cell),
                                              C.byref(mono)))
        out = self.parse_record(rec, 0)
        n, m = len(out["kpL"]), len(out["klL"])
        out.update(kp_un=kp_un[:n].copy(), kl_un=kl_un[:m].copy(), cell=cell[:n].copy(), n_mono=mono.value,
                   full={"kp_un": kp_un, "kl_un": kl_un, "cell": cell, "record": rec})
        return out

    def set_rectify_maps(self, eye, mapx, mapy):
        """cv::remap(im, imRect, M1, M2, INTER_LINEAR) of the stereo driver (stereo_euroc.cc:166) fused into the ingest;
        (None, None) removes the maps."""
        if mapx is None:
            check(self.L.pli_set_rectify_maps(self.h, eye, None, None))
            return
        mx = np.ascontiguousarray(mapx, np.float32)
        my = np.ascontiguousarray(mapy, np.float32)
        assert mx.shape == my.shape == (self.cfg.height, self.cfg.width)
        check(self.L.pli_set_rectify_maps(self.h, eye, ptr(mx), ptr(my)))

    def search_local_map(self, queries, qdesc, cur_kp, cur_desc, cur_uright, bounds, nnratio=0.8, cur_occupied=None):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th) ORBmatcher.cc:44 — see pli_search_local_map."""
        q = np.ascontiguousarray(queries, PROJ_QUERY_DT)
        qd = np.ascontiguousarray(qdesc, np.uint8)
        kp = np.ascontiguousarray(cur_kp, KEYPOINT_DT)
        de = np.ascontiguousarray(cur_desc, np.uint8)
        ur = np.ascontiguousarray(cur_uright, np.float32)
        occ = None if cur_occupied is None else np.ascontiguousarray(cur_occupied, np.uint8)
        best = np.full(q.shape[0], -1, np.int32)
        n = C.c_int32()
        check(self.L.pli_search_local_map(self.h, ptr(q), ptr(qd), q.shape[0], ptr(kp), ptr(de), ptr(ur), ptr(occ),
                                          kp.shape[0], bounds[0], bounds[1], bounds[2], bounds[3], nnratio, ptr(best),
                                          C.byref(n)))
        return n.value, best

    def search_local_map_fisheye(self, q_left, q_right, qdesc, kp_left, desc_left, left_to_right, kp_right, desc_right,
                                 right_to_left, bounds, nnratio=0.8, occ_left=None, occ_right=None):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th) for two fisheye cameras, ORBmatcher.cc:44-214 — see
        pli_search_local_map_fisheye.  Returns (nmatches, mp_left, mp_right)."""
        ql = np.ascontiguousarray(q_left, PROJ_QUERY_DT)
        qr = np.ascontiguousarray(q_right, PROJ_QUERY_DT)
        qd = np.ascontiguousarray(qdesc, np.uint8)
        kl, kr = np.ascontiguousarray(kp_left, KEYPOINT_DT), np.ascontiguousarray(kp_right, KEYPOINT_DT)
        dl, dr = np.ascontiguousarray(desc_left, np.uint8), np.ascontiguousarray(desc_right, np.uint8)
        l2r, r2l = np.ascontiguousarray(left_to_right, np.int32), np.ascontiguousarray(right_to_left, np.int32)
        ol = None if occ_left is None else np.ascontiguousarray(occ_left, np.uint8)
        orr = None if occ_right is None else np.ascontiguousarray(occ_right, np.uint8)
        mpl = np.full(kl.shape[0], -1, np.int32)
        mpr = np.full(kr.shape[0], -1, np.int32)
        n = C.c_int32()
        check(self.L.pli_search_local_map_fisheye(self.h, ptr(ql), ptr(qr), ptr(qd), ql.shape[0], ptr(kl), ptr(dl), ptr(ol), ptr(l2r),
                                                  kl.shape[0], ptr(kr), ptr(dr), ptr(orr), ptr(r2l), kr.shape[0], bounds[0], bounds[1],
                                                  bounds[2], bounds[3], nnratio, ptr(mpl), ptr(mpr), C.byref(n)))
        return n.value, mpl, mpr

    def search_by_projection_two_cameras(self, q_left, q_right, qdesc, kp_left, desc_left, kp_right, desc_right, bounds,
                                         check_orientation=True, occ_left=None, occ_right=None, with_raw=False):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for a current frame of two cameras,
        ORBmatcher.cc:1961-2177 — see pli_search_by_projection_two_cameras.  Returns (nmatches, best_left, best_right), with_raw:
        (nmatches, best_left, best_right, raw_left, raw_right)."""
        ql = np.ascontiguousarray(q_left, PROJ_QUERY_DT)
        qr = np.ascontiguousarray(q_right, PROJ_QUERY_DT)
        if ql.shape != qr.shape:
            raise ValueError("q_left and q_right: one row per query each")
        qd = np.ascontiguousarray(qdesc, np.uint8)
        kl, kr = np.ascontiguousarray(kp_left, KEYPOINT_DT), np.ascontiguousarray(kp_right, KEYPOINT_DT)
        dl, dr = np.ascontiguousarray(desc_left, np.uint8), np.ascontiguousarray(desc_right, np.uint8)
        ol = None if occ_left is None else np.ascontiguousarray(occ_left, np.uint8)
        orr = None if occ_right is None else np.ascontiguousarray(occ_right, np.uint8)
        nq = ql.shape[0]
        bl, br = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
        rl, rr = (np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)) if with_raw else (None, None)
        n = C.c_int32()
        check(self.L.pli_search_by_projection_two_cameras(self.h, ptr(ql), ptr(qr), ptr(qd), nq, ptr(kl), ptr(dl), ptr(ol),
                                                          kl.shape[0], ptr(kr), ptr(dr), ptr(orr), kr.shape[0], bounds[0],
                                                          bounds[1], bounds[2], bounds[3], int(check_orientation), ptr(bl), ptr(br),
                                                          ptr(rl), ptr(rr), C.byref(n)))
        return (n.value, bl, br, rl, rr) if with_raw else (n.value, bl, br)

    def match_nnr(self, desc1, desc2, nnr):
        """match(vpLocalMapLines, CurrentFrame, nnr, matches_12) LineMatcher.cpp:161 (one-way matchNNR)."""
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        m = np.full(d1.shape[0], -1, np.int32)
        n = C.c_int32()
        check(self.L.pli_match_nnr(self.h, ptr(d1), d1.shape[0], ptr(d2), d2.shape[0], nnr, ptr(m), C.byref(n)))
        return n.value, m

    def search_local_points(self, points, descs, pose, cam, cur_kp, cur_desc, cur_uright, th=1.0, far_points=False, th_far=0.0,
                            nnratio=0.8, viewing_cos_limit=0.5, cur_occupied=None, level_ratio=None):
        """Tracking.cc:3809-3855 for a frame of one camera: Frame::isInFrustum of every local map point, the queries of
        ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) and that search, the projection and the
        queries on the device - see pli_search_local_points.  points: capi.FUSE_POINT_DT rows in list order (valid == 0: skipped
        at :3813-3816; valid == capi.LOCAL_STORED_VIEW: skipped there but still mbTrackInView, searched with the fields it holds:
        pos = mTrackProjX, Y, XR, normal = mTrackDepth, mTrackViewCos, mnTrackScaleLevel), descs their GetDescriptor() rows; pose: 15 floats (mRcw row major, mtcw, mOw); cam: capi.FuseCamera or its
        9 values.  Returns (view: capi.LOCAL_VIEW_DT rows, best_idx2, n_in_view, nmatches)."""
        pts = np.ascontiguousarray(points, capi.FUSE_POINT_DT).reshape(-1)
        d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        if len(d) != len(pts):
            raise ValueError("every map point needs one descriptor")
        pose = np.ascontiguousarray(pose, np.float32).reshape(15)
        if not isinstance(cam, capi.FuseCamera):
            cam = capi.FuseCamera(*[float(v) for v in cam])
        kp = np.ascontiguousarray(cur_kp, KEYPOINT_DT)
        de = np.ascontiguousarray(cur_desc, np.uint8)
        ur = np.ascontiguousarray(cur_uright, np.float32)
        occ = None if cur_occupied is None else np.ascontiguousarray(cur_occupied, np.uint8)
        level_ratio = self._level_ratio(level_ratio)
        view = np.zeros(len(pts), capi.LOCAL_VIEW_DT)
        best = np.full(len(pts), -1, np.int32)
        nview, n = C.c_int32(), C.c_int32()
        check(self.L.pli_search_local_points(self.h, ptr(pts), ptr(d), len(pts), ptr(pose), C.byref(cam), float(viewing_cos_limit),
                                             float(th), int(bool(far_points)), float(th_far), float(nnratio), ptr(level_ratio),
                                             ptr(kp), ptr(de), ptr(ur), ptr(occ), kp.shape[0], ptr(view), ptr(best),
                                             C.byref(nview), C.byref(n)))
        return view, best, nview.value, n.value

    def search_local_lines(self, start_points, valid, descs, pose, cam, cur_desc, nnr):
        """Tracking.cc:3862-3883: Frame::isInFrustum_l of every local map line, the ordered list mvpLocalMapLines_InFrustum and
        the one-way matchNNR of its descriptors against the frame's - see pli_search_local_lines.  start_points: nl x 3 floats,
        valid: nl (0: skipped at :3865-3868), descs: nl x 32.  Returns (in_view[nl], proj_s[nl, 2], in_frustum[k], matches_12[k],
        nmatches) with k = the number of lines in view."""
        sp = np.ascontiguousarray(start_points, np.float32).reshape(-1, 3)
        va = np.ascontiguousarray(valid, np.uint8).reshape(-1)
        d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        if not len(sp) == len(va) == len(d):
            raise ValueError("every map line needs a start point, a valid flag and a descriptor")
        pose = np.ascontiguousarray(pose, np.float32).reshape(15)
        if not isinstance(cam, capi.FuseCamera):
            cam = capi.FuseCamera(*[float(v) for v in cam])
        d2 = np.ascontiguousarray(cur_desc, np.uint8).reshape(-1, 32)
        nl = len(sp)
        in_view = np.zeros(nl, np.int32)
        proj = np.zeros((nl, 2), np.float32)
        lst = np.full(nl, -1, np.int32)
        m = np.full(nl, -1, np.int32)
        nview, n = C.c_int32(), C.c_int32()
        check(self.L.pli_search_local_lines(self.h, ptr(sp), ptr(va), ptr(d), nl, ptr(pose), C.byref(cam), ptr(d2), len(d2),
                                            float(nnr), ptr(in_view), ptr(proj), ptr(lst), ptr(m), C.byref(nview), C.byref(n)))
        return in_view, proj, lst[:nview.value].copy(), m[:nview.value].copy(), n.value

    # ---- batch path ----------------------------------------------------------
    def table_bytes(self, nframes):
        return int(self.layout.record_bytes) * nframes

    def batch_run_host(self, images, stages=capi.RUN_ALL):
        """images: (nframes, 2, H, W) u8 ((nframes, 2, H, W, channels) under a colour image format).  Returns the list of parsed
        frame records."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim != (4 if self.channels == 1 else 5) or images.shape[4:] not in ((), (self.channels,)):
            raise ValueError("(nframes, 2, H, W%s) u8 images expected" % ("" if self.channels == 1 else ", %d" % self.channels))
        nf, two, H, W = images.shape[:4]
        W *= self.channels                  # bytes of a row
        assert two == 2
        left = np.ascontiguousarray(images[:, 0])
        right = np.ascontiguousarray(images[:, 1])
        table = np.zeros(self.table_bytes(nf), np.uint8)
        check(self.L.pli_batch_run_host(self.h, nf, ptr(left), ptr(right), W, W * H, stages, ptr(table)))
        return [self.parse_record(table, f) for f in range(nf)]

    def batch_run_mono_host(self, images, stages=capi.RUN_ORB | capi.RUN_LINES):
        """A monocular (or RGB-D colour) stream through the batch entry point: the frames 2i and 2i+1 take the two eye
        slots of record i (left pointer = frame 0, right pointer = frame 1, frame stride = two frames), the stereo stages
        stay off.  images: (nframes, H, W) u8, nframes even.  Returns one dict per frame: kp, desc, kl, ldesc — what the
        monocular Frame constructor (Frame.cc:334) extracts."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim != (3 if self.channels == 1 else 4) or images.shape[3:] not in ((), (self.channels,)):
            raise ValueError("(nframes, H, W%s) u8 images expected" % ("" if self.channels == 1 else ", %d" % self.channels))
        nf, H, W = images.shape[:3]
        W *= self.channels                  # bytes of a row
        assert nf % 2 == 0 and not (stages & (capi.RUN_STEREO_POINTS | capi.RUN_STEREO_LINES))
        table = np.zeros(self.table_bytes(nf // 2), np.uint8)
        base = images.ctypes.data
        check(self.L.pli_batch_run_host(self.h, nf // 2, C.c_void_p(base), C.c_void_p(base + W * H), W, 2 * W * H, stages,
                                        ptr(table)))
        out = []
        for f in range(nf):
            r = self.parse_record(table, f // 2)
            e = "LR"[f & 1]
            out.append({"kp": r["kp" + e], "desc": r["desc" + e], "kl": r["kl" + e], "ldesc": r["ldesc" + e]})
        return out

    def batch_run_device(self, nframes, dev_left, dev_right, stride, frame_stride, dev_table, stages=capi.RUN_ALL):
        """Asynchronous: device pointers (ints) in, device table out; sync() to wait."""
        # The stereo stages read their inputs from the table: counts[0..3], keypoints, descriptors, keylines and line
        # descriptors of each record, and the pyramids the context holds.  So the stereo kernels can be run on tables of
        # the caller's making: (1) stages=RUN_ALL on the images, which leaves every pyramid level in the context; (2)
        # overwrite those columns of the records on the device (offsets: pli_ctx_layout); (3) stages=RUN_STEREO_POINTS |
        # RUN_STEREO_LINES with the same images -- the ingest rewrites level 0 with the same bytes, levels 1.. stay --
        # and read uright, depth, disp, le, counts[4], counts[5] (with debug_enable: DBG_STEREO_SAD per frame).  The
        # tables must keep what the kernels assume (they index the per-level tables by octave and turn coordinates into
        # ints without a guard): tests/helpers_matchers.py validate_tables is the authority on that list -- counts within
        # kp_cap / kl_cap, (n, 32) uint8 descriptors, octave in [0, nlevels), finite coordinates, keypoint rows inside the
        # image and columns within one width of it, line end points within one image size of it.
        # tests/test_independent_matchers_gpu.py runs this route.
        check(self.L.pli_batch_run(self.h, nframes, C.c_void_p(dev_left), C.c_void_p(dev_right), stride, frame_stride,
                                   stages, C.c_void_p(dev_table)))

    def frame_extract(self, left, right):
        """pli_frame_extract: the whole front-end of one Frame (both eyes, points and lines, the two stereo matchers) in one
        submission; returns the parsed record and leaves the per-call state behind (pyramid_level, compute_stereo_matches)."""
        left, right = self._image(left), self._image(right)
        rec = np.zeros(int(self.layout.record_bytes), np.uint8)
        check(self.L.pli_frame_extract(self.h, ptr(left), ptr(right), left.shape[1], left.shape[0], left.strides[0],
                                       right.strides[0], ptr(rec)))
        return self.parse_record(rec, 0)

    def lsd_round_stats(self):
        """(rounds launched without a look by the last call, rounds its slowest image needed or -1, images that took the
        device-side fallback so far, rounds the next call plans from) — pli_lsd_round_stats; synchronises."""
        out = (C.c_int32 * 4)()
        check(self.L.pli_lsd_round_stats(self.h, out))
        return tuple(int(v) for v in out)

    def lsd_arena_words(self):
        """Arena words per scaled LSD pixel this context got (16 unless it is large or the device was short of memory) — pli_lsd_arena_words."""
        out = C.c_int32()
        check(self.L.pli_lsd_arena_words(self.h, C.byref(out)))
        return out.value

    def selftest_hot_trig(self):
        """Largest |v_cos / v_sin - cos / sin| over every float angle in [0, 360] degrees on this device (pli_selftest_hot_trig)."""
        out = C.c_double()
        check(self.L.pli_selftest_hot_trig(self.h, C.byref(out)))
        return out.value

    def selftest_front_stream(self, imgs, scale=1.2, pack_w=False, records=False):
        """The three forms of the LSD front pass on a batch of u8 images (n, h, w), compared on the device (pli_selftest_front_stream).

        Returns {"vs_tiled": (hot, cold, mg, maxMg), "vs_unfused": (...), "chunk": rows per wave, "applied": bool}: counts of differing
        4-byte words of the streaming form (of the tiled one where the streaming form does not apply) per plane.  records: the forms
        write the 16-byte records and the owner plane instead of the hot and cold planes, and the first two counts are theirs."""
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        assert imgs.ndim == 3
        n, h, w = imgs.shape
        out = (C.c_int32 * 10)()
        check(self.L.pli_selftest_front_stream(self.h, imgs.ctypes.data_as(C.POINTER(C.c_uint8)), n, w, h, float(scale),
                                               (1 if pack_w else 0) | (2 if records else 0), out))
        v = [int(x) for x in out]
        return {"vs_tiled": tuple(v[0:4]), "vs_unfused": tuple(v[4:8]), "chunk": v[8], "applied": bool(v[9])}

    def selftest_front_planes(self, imgs, form, scale=1.2, pack_w=False, records=False):
        """One form of the LSD front pass (0 the three kernels, 1 tiled, 2 streaming) on a batch of u8 images (n, h, w), its planes
        read back (pli_selftest_front_planes); PliError (PLI_ERR_INVALID) where the form does not apply to the size.

        Returns arrays of shape (n, dh, dp, ..) — dp: the planes' row pitch, the scaled width dw rounded up to 16; columns dw .. dp - 1
        are pad — under "hot" (int32 x 2: angle bits, owner word) and "cold" (float32 x 2: cos, sin), or with records=True under "rec"
        (float32 x 4: angle, cos, sin, owner word) and "own" (int32 x 2); "norm" (float64), "max_bits" (uint64 per image: the bits of
        the largest norm above rho, 0: none), "dw", and for form 0 "scaled" (float64 (n, dh, dw))."""
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        assert imgs.ndim == 3
        n, h, w = imgs.shape
        dw, dh = int(round(w * scale)), int(round(h * scale))      # (cvRound: nearest, ties to even — as Python's round)
        dp = (dw + 15) // 16 * 16
        a = np.zeros((n, dh, dp, 4), np.float32) if records else np.zeros((n, dh, dp, 2), np.int32)
        b = np.zeros((n, dh, dp, 2), np.int32 if records else np.float32)
        norm = np.zeros((n, dh, dp), np.float64)
        max_bits = np.zeros(n, np.uint64)
        scaled = np.zeros((n, dh, dw), np.float64) if form == 0 else None
        check(self.L.pli_selftest_front_planes(self.h, imgs.ctypes.data_as(C.POINTER(C.c_uint8)), n, w, h, float(scale), int(form),
                                               (1 if pack_w else 0) | (2 if records else 0), n * dh * dp, ptr(a), ptr(b), ptr(norm),
                                               ptr(max_bits), ptr(scaled) if scaled is not None else None))
        out = {"norm": norm, "max_bits": max_bits, "dw": dw}
        out.update({"rec": a, "own": b} if records else {"hot": a, "cold": b})
        if scaled is not None:
            out["scaled"] = scaled
        return out

    def sync(self):
        check(self.L.pli_ctx_sync(self.h))

    # ---- frame-to-frame track matching of a batch (BASELINE config 3) ------------------------------------------
    def track_layout(self):
        tl = capi.TrackLayout()
        check(self.L.pli_track_layout_get(self.h, C.byref(tl)))
        return tl

    def track_params(self, th=15.0, mono=False, check_orientation=True, nnr_lines=0.9, cx=None, cy=None, fy=None):
        """pli_track_params with the context's camera (fx, bf) and the image rectangle as the frame grid bounds."""
        W, H = self.cfg.width, self.cfg.height
        return capi.TrackParams(fx=self.cfg.fx, fy=self.cfg.fx if fy is None else fy, cx=W / 2.0 if cx is None else cx,
                                cy=H / 2.0 if cy is None else cy, bf=self.cfg.bf, th=th, min_x=0.0, max_x=float(W), min_y=0.0,
                                max_y=float(H), mono=int(mono), check_orientation=int(check_orientation), nnr_lines=nnr_lines,
                                reserved=0)

    def batch_track_device(self, nframes, dev_table, dev_poses, params, dev_track):
        """Asynchronous: frame i against frame i-1 on the device tables (pointers as ints)."""
        check(self.L.pli_batch_track(self.h, nframes, C.c_void_p(dev_table), C.c_void_p(dev_poses), C.byref(params),
                                     C.c_void_p(dev_track)))

    def parse_track(self, track, frame):
        tl = self.track_layout()
        rec = track[frame * tl.record_bytes:(frame + 1) * tl.record_bytes]
        counts = rec[tl.off_counts:tl.off_counts + 16].view(np.int32).copy()
        return {"counts": counts, "best": rec[tl.off_best:tl.off_best + 4 * int(counts[0])].view(np.int32).copy(),
                "lines": rec[tl.off_lines:tl.off_lines + 4 * int(counts[2])].view(np.int32).copy()}

    # ---- pipelined host entry point (pinned buffers, copies overlap the kernels) ---------------------------
    def pinned(self, nbytes):
        """numpy u8 view of `nbytes` of pinned host memory (pli_host_alloc); freed with the Frontend."""
        p = C.c_void_p()
        check(self.L.pli_host_alloc(nbytes, C.byref(p)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def host_buffers(self, nframes):
        """(left, right, tables): pinned (nframes, H*W) image planes (H*W*channels bytes each under a colour image format) and two
        pinned result tables."""
        n = self.cfg.width * self.cfg.height * self.channels
        left = self.pinned(nframes * n).reshape(nframes, n)
        right = self.pinned(nframes * n).reshape(nframes, n)
        tables = [self.pinned(self.table_bytes(nframes)) for _ in range(2)]
        return left, right, tables

    def host_submit(self, nframes, left, right, table, stages=capi.RUN_ALL):
        W, H = self.cfg.width * self.channels, self.cfg.height      # (W: bytes of a row)
        check(self.L.pli_batch_submit_host(self.h, nframes, ptr(left), ptr(right), W, W * H, stages, ptr(table)))

    def host_wait(self):
        check(self.L.pli_batch_wait(self.h, 0))

    def host_wait_all(self):
        check(self.L.pli_batch_wait(self.h, 1))

    def set_stream(self, hip_stream):
        check(self.L.pli_ctx_set_stream(self.h, C.c_void_p(hip_stream)))

    def parse_record(self, table, frame):
        """Slice one frame record (numpy u8 array of the whole table) into named arrays."""
        Y = self.layout
        rec = table[frame * Y.record_bytes:(frame + 1) * Y.record_bytes]
        counts = rec[Y.off_counts:Y.off_counts + 32].view(np.int32)
        out = {"counts": counts.copy(), "truncated": rec[Y.off_counts + 24:Y.off_counts + 28].copy()}   # lines L/R, keypoints L/R
        for e, name in ((0, "L"), (1, "R")):
            n = int(counts[e])
            out["kp" + name] = rec[Y.off_kp[e]:Y.off_kp[e] + 24 * n].view(KEYPOINT_DT).copy()
            out["desc" + name] = rec[Y.off_desc[e]:Y.off_desc[e] + 32 * n].reshape(n, 32).copy()
            m = int(counts[2 + e])
            out["kl" + name] = rec[Y.off_kl[e]:Y.off_kl[e] + 68 * m].view(KEYLINE_DT).copy()
            out["ldesc" + name] = rec[Y.off_ldesc[e]:Y.off_ldesc[e] + 32 * m].reshape(m, 32).copy()
        n, m = int(counts[0]), int(counts[2])
        out["uright"] = rec[Y.off_uright:Y.off_uright + 4 * n].view(np.float32).copy()
        out["depth"] = rec[Y.off_depth:Y.off_depth + 4 * n].view(np.float32).copy()
        out["disp"] = rec[Y.off_disp:Y.off_disp + 8 * m].view(np.float32).reshape(m, 2).copy()
        out["le"] = rec[Y.off_le:Y.off_le + 24 * m].view(np.float64).reshape(m, 3).copy()
        return out

    # ---- measurement / debug ---------------------------------------------------
    def prof_enable(self, on=True):
        check(self.L.pli_prof_enable(self.h, int(on)))

    def prof_reset(self):
        check(self.L.pli_prof_reset(self.h))

    def prof_report(self):
        """{kernel name: (calls, total_ms)} measured with HIP events on the context stream."""
        buf = C.create_string_buffer(1 << 16)
        check(self.L.pli_prof_report(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.split()
            out[name] = (int(calls), float(ms))
        return out

    def debug_enable(self, on=True):
        check(self.L.pli_debug_enable(self.h, int(on)))

    def debug_fetch(self, image, what, arg=0):
        n = C.c_int64()
        check(self.L.pli_debug_fetch(self.h, image, what, arg, None, 0, C.byref(n)))
        buf = np.zeros(max(int(n.value), 1), np.uint8)
        check(self.L.pli_debug_fetch(self.h, image, what, arg, ptr(buf), buf.size, C.byref(n)))
        return buf[:n.value]

    def debug_points(self, image, what, level):
        raw = self.debug_fetch(image, what, level).view(np.int32)
        return raw[1:1 + 3 * raw[0]].reshape(-1, 3).copy()


class ORBextractor:
    """Mirror of ORB_SLAM3::ORBextractor (include/ORBextractor.h:46-115)."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, image_size, eye=0, frontend=None):
        w, h = image_size
        self.eye = eye
        if frontend is None:
            cfg = capi.default_config(w, h, orb_nfeatures=nfeatures, orb_scale_factor=scaleFactor,
                                      orb_nlevels=nlevels, orb_ini_th_fast=iniThFAST, orb_min_th_fast=minThFAST)
            frontend = Frontend(cfg)
        self.fe = frontend
        self.nlevels = nlevels
        self.scaleFactor = np.float32(scaleFactor)

    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        """Returns (monoCount, keypoints, descriptors); -1 for an empty image like the reference."""
        n, kp, desc = self.fe.orb_extract(self.eye, image)
        return n, kp, desc

    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return float(self.scaleFactor)

    def GetScaleFactors(self):
        s = [np.float32(1.0)]
        for _ in range(1, self.nlevels):
            s.append(np.float32(s[-1] * self.scaleFactor))
        return np.array(s, np.float32)

    def GetInverseScaleFactors(self):
        return (np.float32(1.0) / self.GetScaleFactors()).astype(np.float32)

    @property
    def mvImagePyramid(self):
        return [self.fe.pyramid_level(self.eye, l) for l in range(self.nlevels)]


class Lineextractor:
    """Mirror of ORB_SLAM3::Lineextractor (include/LineExtractor.h:41-74)."""

    def __init__(self, lsd_nfeatures, min_line_length, lsd_refine, lsd_scale, lsd_sigma_scale, lsd_quant, lsd_ang_th,
                 lsd_log_eps, lsd_density_th, lsd_n_bins, image_size, eye=0, frontend=None):
        w, h = image_size
        self.eye = eye
        if frontend is None:
            cfg = capi.default_config(w, h, lsd_nfeatures=lsd_nfeatures, min_line_length=min_line_length,
                                      lsd_refine=lsd_refine, lsd_scale=lsd_scale, lsd_sigma_scale=lsd_sigma_scale,
                                      lsd_quant=lsd_quant, lsd_ang_th=lsd_ang_th, lsd_log_eps=lsd_log_eps,
                                      lsd_density_th=lsd_density_th, lsd_n_bins=lsd_n_bins)
            frontend = Frontend(cfg)
        self.fe = frontend

    def __call__(self, image, mask=None):
        """Returns (keylines, descriptors_line)."""
        n, kl, desc = self.fe.line_extract(self.eye, image)
        return kl, desc
