"""The search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (ORBmatcher.cc:1399-1609) for a keyframe with two
KannalaBrandt8 cameras (NLeft != -1, mpCamera2 set), both values of bRight, restated in Python: the checker of
pli_fuse_search_two_cameras (tests/test_fuse_two_cameras_gpu.py).  CPU only.

  fuse2_scalar   the reference's control flow for one (keyframe, bRight): the pose and the camera of the side (:1404-1417), the
                 gates :1435-1500 in their order, KeyFrame::GetFeaturesInArea(x, y, r, bRight) over the side's own grid (mGrid from
                 mvKeys, mGridRight from mvKeysRight with camera-local indices, Frame.cc:468-481; KeyFrame.cc:881-925), the level
                 gate, the chi-square gate with the monocular bound (every mvuRight of such a keyframe is -1, Frame.cc:1589, so
                 :1533 never takes the stereo branch), idx += NLeft (:1559), the running strict minimum, TH_LOW.  Every exit counted.
  fuse2_fast     the closed form the device uses: vectorised gates, the level as a count of level_ratio thresholds, the winner as the
                 minimum of the key (distance, cell column, cell row, camera-local index), + NLeft for the right camera.

Float results follow the reference's operation order in float32 (a cv::Mat product: double accumulation, one rounding; cv::norm
and Mat::dot in double); KannalaBrandt8::project is pyoracle.kb8_project (float32, libm in double and rounded).  The pose getters
GetRightRotation() / GetRightTranslation() / GetRightCameraCenter() (KeyFrame.cc:1343-1373) are one gemm per product, with the Pose
class of tests/test_triangulation_two_cameras_cpu.py.

Decided margins.  The last bit of the KannalaBrandt8 projection is not pinned (glibc's atan2 / cos / sin against the device's), so
the corpus must not depend on it: gates64() restates the same gates in float64 (hg.kb8_project64, shaped differently), and every
decision of every (keyframe, side, point[, keypoint]) - depth sign, image bounds, distance range, normal, each level_ratio
threshold, the cell window's floor and ceil, |dx| < r, |dy| < r, 5.99 - must lie further from its threshold than 8 x the worst
deviation between the float32-order and the float64 value of the compared quantity, measured over the corpus (the rule of
helpers_geometry.py).  Measured on the corpus (th = 3 and 4), again on every run (test_margins_...), which fails when a run
measures more than is recorded in MEASURED:

  depth     z of p3Dc                                    worst 4.8e-7 m      (MEASURED 1e-6)
  px        u, v of the projection                       worst 5.2e-5 px     (MEASURED 1e-4)
  dist      dist3D                                       worst 9.4e-7 m      (MEASURED 1.5e-6)
  normal    PO.dot(Pn) - 0.5 dist3D                      worst 4.5e-7 m      (MEASURED 1e-6)
  ratio     mfMaxDistance / dist3D                       worst 5.6e-7        (MEASURED 8e-7)
  cell      (u - mnMinX -+ r) * mfGridElementWidthInv    worst 8.8e-6 cells  (MEASURED 1.2e-5)
  chi       e2 * mvInvLevelSigma2[octave]                worst 4.1e-4        (MEASURED 6e-4)

(The recorded values are the worsts over a hundred seeds of the builder, rounded up; the committed seeds are the first ones for
which the builder draws nothing again.)  The builder draws a point whose pair comes out undecided again; points drawn again: 0, undecided pairs: 0 for the committed seeds
of the corpus (asserted, printed)."""
import math
import os
import re
from collections import Counter, namedtuple
from dataclasses import dataclass, replace

import numpy as np
import pytest

import helpers_geometry as hg
from helpers_matchers import GRID_COLS, GRID_ROWS, TH_LOW, c_round, hamming
from test_fuse_search_cpu import FUSE_POINT_DT, INV_SIGMA2, NLEVELS, SF, flip_bits, gemm_row, level_ratio, predict_scale, rot_xyz
from test_triangulation_two_cameras_cpu import CAMS, TLR_T, Pose, gemm, pose_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
Bounds = namedtuple("Bounds", "min_x max_x min_y max_y")
BOUNDS = Bounds(f32(0.0), f32(512.0), f32(0.0), f32(512.0))      # mnMinX .. mnMaxY of a 512 x 512 fisheye image (no undistortion)
# one keyframe: mvKeys then mvKeysRight (pt.x, pt.y, octave), mDescriptors, NLeft, pose[2, 15] (left, right: Rcw row major, tcw, Ow)
KF2 = namedtuple("KF2", "x y octave desc nleft pose")
Case = namedtuple("Case", "pts descs kfs skip redrawn")
EXITS = ("not_valid", "skip", "neg_depth", "not_in_image", "dist_range", "normal", "empty_window", "level_gate", "chi2_mono", "tie",
         "gt_th_low", "match")
MEASURED = {"depth": 1e-6, "px": 1e-4, "dist": 1.5e-6, "normal": 1e-6, "ratio": 8e-7, "cell": 1.2e-5, "chi": 6e-4}
MARGIN = {k: 8 * v for k, v in MEASURED.items()}


@dataclass(frozen=True)
class Rules:
    """The readings that the mutation tests flip; the defaults are the reference's."""
    left_pose_for_right: bool = False
    left_cam_for_right: bool = False
    left_grid_for_right: bool = False
    no_nleft: bool = False
    pinhole: bool = False
    stereo_bound: bool = False
    no_depth_gate: bool = False            # (a known answer only)


REF = Rules()


def oracle():
    from oracle import pyoracle
    return pyoracle


def kf_pose(P):
    """pose[2, 15] of a keyframe with Tcw = P: GetRotation() / GetTranslation() / GetCameraCenter() and the three right getters
    (KeyFrame.cc:1343-1373), each product one gemm."""
    out = np.zeros((2, 15), f32)
    Ow = P.centre()                                                  # Ow = -Rwc * tcw (KeyFrame::SetPose)
    out[0] = np.concatenate([P.R.reshape(9), P.t.reshape(3), Ow.reshape(3)])
    twr = gemm(P.R.T, TLR_T, 1.0, Ow)                                # Rwl * tlr + twl
    out[1] = np.concatenate([P.right_rotation().reshape(9), P.right_translation().reshape(3), twr.reshape(3)])
    return out


def side_rows(kf, right):
    return (kf.nleft, len(kf.x)) if right else (0, kf.nleft)


# ---- the reference's control flow ----------------------------------------------------------------------------------------------

def fuse2_scalar(pts, descs, kf, right, th=3.0, skip=None, exits=None, rules=REF, cams=CAMS, bounds=BOUNDS):
    """-> best_idx[nmp] (rows over the keyframe's N), best_dist[nmp] of Fuse(pKF, vpMapPoints, th, bRight = right)."""
    po = oracle()
    exits = exits if exits is not None else Counter()
    T = kf.pose[0 if (not right or rules.left_pose_for_right) else 1]
    cam = np.asarray(cams[0 if (not right or rules.left_cam_for_right) else 1], f32)
    lo, hi = side_rows(kf, right)
    kx, ky, ko = kf.x[lo:hi], kf.y[lo:hi], kf.octave[lo:hi]         # mvKeys / mvKeysRight, camera-local rows
    glo, ghi = side_rows(kf, right and not rules.left_grid_for_right)
    gw_inv = f32(f32(GRID_COLS) / f32(bounds.max_x - bounds.min_x))
    gh_inv = f32(f32(GRID_ROWS) / f32(bounds.max_y - bounds.min_y))
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
    for i in range(ghi - glo):                                       # Frame::AssignFeaturesToGrid, Frame.cc:468-481
        px = int(c_round(f32(f32(kf.x[glo + i] - bounds.min_x) * gw_inv)))
        py = int(c_round(f32(f32(kf.y[glo + i] - bounds.min_y) * gh_inv)))
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid[px][py].append(i)
    R, t, Ow = T[:9].reshape(3, 3), T[9:12], T[12:15]
    th = f32(th)
    best_idx = np.full(len(pts), -1, np.int32)
    best_dist = np.full(len(pts), 256, np.int32)
    with np.errstate(all="ignore"):
        for i, P in enumerate(pts):
            if not P["valid"]:
                exits["not_valid"] += 1; continue
            if skip is not None and skip[i]:
                exits["skip"] += 1; continue
            p = P["pos"]
            x, y, z = (gemm_row(R[r], p, t[r]) for r in range(3))
            if z < f32(0.0) and not rules.no_depth_gate:
                exits["neg_depth"] += 1; continue
            if rules.pinhole:
                u, v = f32(f32(f32(cam[0] * x) / z) + cam[2]), f32(f32(f32(cam[1] * y) / z) + cam[3])
            else:
                u, v = po.kb8_project(cam, np.array([x, y, z], f32))
            if not (u >= bounds.min_x and u < bounds.max_x and v >= bounds.min_y and v < bounds.max_y):
                exits["not_in_image"] += 1; continue
            PO = (p - Ow).astype(f32)
            dist3D = f32(math.sqrt(float(PO[0]) ** 2 + float(PO[1]) ** 2 + float(PO[2]) ** 2))
            if dist3D < P["min_dist_inv"] or dist3D > P["max_dist_inv"]:
                exits["dist_range"] += 1; continue
            Pn = P["normal"]
            if float(PO[0]) * float(Pn[0]) + float(PO[1]) * float(Pn[1]) + float(PO[2]) * float(Pn[2]) < 0.5 * float(dist3D):
                exits["normal"] += 1; continue
            level = predict_scale(f32(P["max_dist"] / dist3D))
            radius = f32(th * SF[level])
            idxs = []                                                # KeyFrame::GetFeaturesInArea(u, v, radius, bRight)
            c0 = max(0, math.floor(f32(f32(f32(u - bounds.min_x) - radius) * gw_inv)))
            c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(u - bounds.min_x) + radius) * gw_inv)))
            r0 = max(0, math.floor(f32(f32(f32(v - bounds.min_y) - radius) * gh_inv)))
            r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(v - bounds.min_y) + radius) * gh_inv)))
            if c0 < GRID_COLS and c1 >= 0 and r0 < GRID_ROWS and r1 >= 0:
                for ix in range(c0, c1 + 1):
                    for iy in range(r0, r1 + 1):
                        for j in grid[ix][iy]:
                            if j >= len(kx):                         # (left_grid_for_right only: past mvKeysRight)
                                continue
                            if abs(f32(kx[j] - u)) < radius and abs(f32(ky[j] - v)) < radius:
                                idxs.append(j)
            if not idxs:
                exits["empty_window"] += 1; continue
            bd, bi = 256, -1
            for j in idxs:
                lev = int(ko[j])
                if lev < level - 1 or lev > level:
                    exits["level_gate"] += 1; continue
                ex, ey = f32(u - kx[j]), f32(v - ky[j])             # mvuRight[idx] is -1: :1547-1557
                e2 = f32(f32(ex * ex) + f32(ey * ey))
                if float(f32(e2 * INV_SIGMA2[lev])) > (7.8 if rules.stereo_bound else 5.99):
                    exits["chi2_mono"] += 1; continue
                idx = j + (kf.nleft if right and not rules.no_nleft else 0)     # :1559
                d = int(hamming(descs[i], kf.desc[idx]))
                if d == bd and bi >= 0:
                    exits["tie"] += 1
                if d < bd:
                    bd, bi = d, idx
            best_dist[i] = bd
            if bd <= TH_LOW:
                best_idx[i] = bi
                exits["match"] += 1
            else:
                exits["gt_th_low"] += 1
    return best_idx, best_dist


# ---- the gates of one view for every point, float32 in the reference's order and float64 -----------------------------------------

def gates32(pts, T, cam, th, lr):
    po = oracle()
    pos = pts["pos"]
    R, t, Ow = T[:9].reshape(3, 3).astype(f64), T[9:12].astype(f64), T[12:15]
    n = len(pts)
    with np.errstate(all="ignore"):
        pc = np.stack([(R[r, 0] * pos[:, 0].astype(f64) + R[r, 1] * pos[:, 1].astype(f64) + R[r, 2] * pos[:, 2].astype(f64)
                        + t[r]).astype(f32) for r in range(3)], 1)
        uv = np.full((n, 2), np.nan, f32)
        c = np.asarray(cam, f32)
        for i in range(n):
            uv[i] = po.kb8_project(c, pc[i])
        PO = pos - Ow[None, :]
        assert PO.dtype == f32
        POd = PO.astype(f64)
        dist = np.sqrt(POd[:, 0] ** 2 + POd[:, 1] ** 2 + POd[:, 2] ** 2).astype(f32)
        Pn = pts["normal"].astype(f64)
        dot = POd[:, 0] * Pn[:, 0] + POd[:, 1] * Pn[:, 1] + POd[:, 2] * Pn[:, 2]
        ratio = pts["max_dist"] / dist
        level = (ratio[:, None] > lr[None, :]).sum(1)
        radius = f32(th) * SF[level]
        assert ratio.dtype == f32 and radius.dtype == f32
    return dict(z=pc[:, 2], u=uv[:, 0], v=uv[:, 1], dist=dist, normal=dot - 0.5 * dist.astype(f64), ratio=ratio, level=level,
                radius=radius)


def gates64(pts, T, cam, th, lr):
    """The same quantities in float64 from the same float32 inputs, by other expressions: the pose as one matrix product, the
    projection hg.kb8_project64 (x / hypot, y / hypot, Horner), the distance np.linalg.norm."""
    pos = pts["pos"].astype(f64)
    R, t, Ow = T[:9].reshape(3, 3).astype(f64), T[9:12].astype(f64), T[12:15].astype(f64)
    pc = pos @ R.T + t
    uv = np.array([hg.kb8_project64(cam, p) for p in pc]).reshape(-1, 2)
    PO = pos - Ow
    dist = np.linalg.norm(PO, axis=1)
    with np.errstate(all="ignore"):
        ratio = pts["max_dist"].astype(f64) / dist
    level = (ratio[:, None] > lr.astype(f64)[None, :]).sum(1)
    return dict(z=pc[:, 2], u=uv[:, 0], v=uv[:, 1], dist=dist, normal=(PO * pts["normal"].astype(f64)).sum(1) - 0.5 * dist, ratio=ratio,
                level=level, radius=float(f32(th)) * SF.astype(f64)[level])


def alive_of(pts, g, bounds, skip):
    """The pairs that reach the window search, from one set of gate quantities."""
    ok = pts["valid"] != 0
    if skip is not None:
        ok &= np.asarray(skip) == 0
    with np.errstate(all="ignore"):
        ok &= ~(g["z"] < 0) & (g["u"] >= bounds.min_x) & (g["u"] < bounds.max_x) & (g["v"] >= bounds.min_y) & (g["v"] < bounds.max_y)
        ok &= ~((g["dist"] < pts["min_dist_inv"]) | (g["dist"] > pts["max_dist_inv"])) & ~(g["normal"] < 0)
    return ok


# ---- the closed form -----------------------------------------------------------------------------------------------------------

def fuse2_fast(pts, descs, kf, right, th=3.0, skip=None, lr=None, cams=CAMS, bounds=BOUNDS, info=None):
    lr = level_ratio() if lr is None else lr
    nmp = len(pts)
    best_idx = np.full(nmp, -1, np.int32)
    best_dist = np.full(nmp, 256, np.int32)
    lo, hi = side_rows(kf, right)
    n = hi - lo
    if nmp == 0 or n == 0:
        return best_idx, best_dist
    g = gates32(pts, kf.pose[1 if right else 0], cams[1 if right else 0], th, lr)
    sel = np.nonzero(alive_of(pts, g, bounds, skip))[0]
    if len(sel) == 0:
        return best_idx, best_dist
    kx, ky, octave, kd = kf.x[lo:hi], kf.y[lo:hi], kf.octave[lo:hi].astype(np.int64), kf.desc[lo:hi]
    gw_inv = f32(f32(GRID_COLS) / f32(bounds.max_x - bounds.min_x))
    gh_inv = f32(f32(GRID_ROWS) / f32(bounds.max_y - bounds.min_y))
    rnd = lambda a: (np.sign(a) * np.floor(np.abs(a).astype(f64) + 0.5)).astype(np.int64)
    px, py = rnd((kx - bounds.min_x) * gw_inv), rnd((ky - bounds.min_y) * gh_inv)
    in_grid = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    base_key = (px << 34) | (py << 28) | np.arange(n, dtype=np.int64)
    chunk = max(1, 400000 // n)
    for s0 in range(0, len(sel), chunk):
        s = sel[s0:s0 + chunk]
        us, vs, rs, lv = g["u"][s, None], g["v"][s, None], g["radius"][s, None], g["level"][s, None]
        c0 = np.maximum(0, np.floor(((us - bounds.min_x) - rs) * gw_inv)).astype(np.int64)
        c1 = np.minimum(GRID_COLS - 1, np.ceil(((us - bounds.min_x) + rs) * gw_inv)).astype(np.int64)
        r0 = np.maximum(0, np.floor(((vs - bounds.min_y) - rs) * gh_inv)).astype(np.int64)
        r1 = np.minimum(GRID_ROWS - 1, np.ceil(((vs - bounds.min_y) + rs) * gh_inv)).astype(np.int64)
        cand = in_grid[None, :] & (px[None, :] >= c0) & (px[None, :] <= c1) & (py[None, :] >= r0) & (py[None, :] <= r1)
        cand &= (np.abs(kx[None, :] - us) < rs) & (np.abs(ky[None, :] - vs) < rs)
        if info is not None:
            info.setdefault("window_rows", np.zeros(nmp, np.int64))[s] = cand.sum(1)
        cand &= (octave[None, :] >= lv - 1) & (octave[None, :] <= lv)
        ex, ey = us - kx[None, :], vs - ky[None, :]
        e2 = ex * ex + ey * ey
        assert e2.dtype == f32
        cand &= ~((e2 * INV_SIGMA2[octave][None, :]).astype(f64) > 5.99)
        rows, cols = np.nonzero(cand)
        if len(rows) == 0:
            continue
        d = hamming(descs[s[rows]], kd[cols]).astype(np.int64)
        key = (d << 40) | base_key[cols]
        best = np.full(len(s), np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, rows, key)
        has = best != np.iinfo(np.int64).max
        bd = (best >> 40).astype(np.int32)
        best_dist[s[has]] = bd[has]
        win = has & (bd <= TH_LOW)
        best_idx[s[win]] = (best[win] & 0xFFFFFFF).astype(np.int32) + lo          # :1559
    return best_idx, best_dist


def fuse2_batch(pts, descs, kfs, th=3.0, sides=3, skip=None, fn=fuse2_fast, **kw):
    """-> best_idx[nkf, 2, nmp], best_dist[nkf, 2, nmp], as pli_fuse_search_two_cameras returns them."""
    bi = np.full((len(kfs), 2, len(pts)), -1, np.int32)
    bd = np.full((len(kfs), 2, len(pts)), 256, np.int32)
    for k, kf in enumerate(kfs):
        for right in (0, 1):
            if (sides >> right) & 1:
                bi[k, right], bd[k, right] = fn(pts, descs, kf, bool(right), th, None if skip is None else skip[k, right], **kw)
    return bi, bd


# ---- decided margins -------------------------------------------------------------------------------------------------------------

def examine(pts, kfs, th, skip=None, cams=CAMS, bounds=BOUNDS):
    """-> (dev: the worst |float32-order - float64| per category, undecided: the set of (keyframe, side, point) with a decision
    inside its margin).  A pair's decisions are looked at in the reference's order, up to the gate that rejects it."""
    lr = level_ratio()
    dev = Counter()
    undecided = set()
    gw_inv = float(f32(f32(GRID_COLS) / f32(bounds.max_x - bounds.min_x)))
    gh_inv = float(f32(f32(GRID_ROWS) / f32(bounds.max_y - bounds.min_y)))
    bmin = {"u": float(bounds.min_x), "v": float(bounds.min_y)}
    bmax = {"u": float(bounds.max_x), "v": float(bounds.max_y)}
    for k, kf in enumerate(kfs):
        for right in (0, 1):
            a, b = gates32(pts, kf.pose[right], cams[right], th, lr), gates64(pts, kf.pose[right], cams[right], th, lr)
            live = pts["valid"] != 0
            if skip is not None:
                live = live & (np.asarray(skip[k, right]) == 0)

            def stage(cat, v32, v64, thresholds, live):
                """the decision v < / > threshold for every live pair: measure, mark, return the float64 side of it"""
                w = np.nonzero(live)[0]
                if len(w) == 0:
                    return
                with np.errstate(all="ignore"):
                    d = np.abs(v32[w].astype(f64) - v64[w])
                    dev[cat] = max(dev[cat], float(np.nanmax(d)) if np.isfinite(d).any() else 0.0)
                    for thr in thresholds:                          # (a number, or one threshold per point)
                        thr = np.broadcast_to(np.asarray(thr, f64), v64.shape)
                        for i in w[np.abs(v64[w] - thr[w]) <= MARGIN[cat]]:
                            undecided.add((k, right, int(i)))

            stage("depth", a["z"], b["z"], [0.0], live)
            live = live & ~(b["z"] < 0)
            for ax in ("u", "v"):
                stage("px", a[ax], b[ax], [bmin[ax], bmax[ax]], live)
            live = live & (b["u"] >= bmin["u"]) & (b["u"] < bmax["u"]) & (b["v"] >= bmin["v"]) & (b["v"] < bmax["v"])
            stage("dist", a["dist"], b["dist"], [pts["min_dist_inv"], pts["max_dist_inv"]], live)
            live = live & ~((b["dist"] < pts["min_dist_inv"]) | (b["dist"] > pts["max_dist_inv"]))
            stage("normal", a["normal"], b["normal"], [0.0], live)
            live = live & ~(b["normal"] < 0)
            stage("ratio", a["ratio"], b["ratio"], [float(x) for x in lr], live)
            w = np.nonzero(live)[0]
            if len(w) == 0:
                continue
            assert np.array_equal(a["level"][w], b["level"][w]) or undecided
            for ax, ginv in (("u", gw_inv), ("v", gh_inv)):          # the window's floor and ceil: every integer is a threshold
                for sign in (-1.0, 1.0):
                    q32 = (f32(a[ax] - f32(bmin[ax])) + f32(sign) * a["radius"]).astype(f32) * f32(ginv)
                    q64 = (b[ax] - bmin[ax] + sign * b["radius"]) * ginv
                    d = np.abs(q32[w].astype(f64) - q64[w])
                    dev["cell"] = max(dev["cell"], float(d.max()))
                    for i in w[np.abs(q64[w] - np.round(q64[w])) <= MARGIN["cell"]]:
                        undecided.add((k, right, int(i)))
            lo, hi = side_rows(kf, bool(right))
            if hi == lo:
                continue
            kx, ky, ko = kf.x[lo:hi].astype(f64), kf.y[lo:hi].astype(f64), kf.octave[lo:hi].astype(np.int64)
            for c0 in range(0, len(w), 512):
                ww = w[c0:c0 + 512]
                r = b["radius"][ww, None]
                dx, dy = np.abs(kx[None, :] - b["u"][ww, None]), np.abs(ky[None, :] - b["v"][ww, None])
                # |dx| < r decides only where |dy| can still be inside, and the reverse (px: the deviation of u and v)
                bad = ((np.abs(dx - r) <= MARGIN["px"]) & (dy < r + MARGIN["px"])) | ((np.abs(dy - r) <= MARGIN["px"]) & (dx < r + MARGIN["px"]))
                inside = (dx < r) & (dy < r) & (ko[None, :] >= b["level"][ww, None] - 1) & (ko[None, :] <= b["level"][ww, None])
                inv = INV_SIGMA2.astype(f64)[ko][None, :]
                chi64 = (dx * dx + dy * dy) * inv
                ex, ey = a["u"][ww, None] - kf.x[None, lo:hi], a["v"][ww, None] - kf.y[None, lo:hi]
                chi32 = ((ex * ex + ey * ey) * INV_SIGMA2[ko][None, :]).astype(f64)
                if inside.any():
                    dev["chi"] = max(dev["chi"], float(np.abs(chi32 - chi64)[inside].max()))
                bad |= inside & (np.abs(chi64 - 5.99) <= MARGIN["chi"])
                for i in ww[bad.any(1)]:
                    undecided.add((k, right, int(i)))
    return dev, undecided


# ---- the corpus ----------------------------------------------------------------------------------------------------------------

def draw_point(rng, only_left_edge=False):
    """A point by its direction from the reference view's left camera (up to 100 degrees off the axis: the fisheye model projects
    a point behind the image plane, :1459 rejects it) and its range."""
    theta = rng.uniform(0.0, 1.75)
    psi = rng.uniform(-math.pi, math.pi)
    rho = rng.uniform(0.5, 15.0)
    if only_left_edge:                                               # near the left image border and close: the right camera,
        theta, psi, rho = rng.uniform(1.27, 1.33), math.pi + rng.uniform(-0.2, 0.2), rng.uniform(0.35, 0.6)     # 0.1 m to the right, sees it further in
    return rho * np.array([math.sin(theta) * math.cos(psi), math.sin(theta) * math.sin(psi), math.cos(theta)])


def fill_point(rng, pts, i, pos):
    dist = np.linalg.norm(pos)
    normal = pos / dist
    if rng.random() < 0.25:                                          # grazing: up to ~75 degrees off the viewing ray
        normal = rot_xyz(*rng.uniform(-0.9, 0.9, 3)) @ normal
    max_d = dist * float(SF[rng.integers(0, NLEVELS)]) * rng.uniform(0.9, 1.1)
    if rng.random() < 0.08:
        max_d *= rng.choice([0.2, 6.0])
    pts["pos"][i], pts["normal"][i] = pos.astype(f32), normal.astype(f32)
    pts["max_dist"][i] = f32(max_d)
    pts["min_dist_inv"][i] = f32(0.8) * f32(max_d / float(SF[-1]))
    pts["max_dist_inv"][i] = f32(1.2) * f32(max_d)


def make_points2(rng, nmp):
    pts = np.zeros(nmp, FUSE_POINT_DT)
    for i in range(nmp):
        fill_point(rng, pts, i, draw_point(rng, only_left_edge=(i % 16 == 5)))
    pts["valid"] = (rng.random(nmp) > 0.03).astype(np.int32)
    return pts, rng.integers(0, 256, (nmp, 32), dtype=np.uint8)


def make_keyframe2(rng, pts, descs, P, nfeat, noise=0.8, cams=CAMS, bounds=BOUNDS):
    """nfeat = (NLeft, NRight).  Per camera: keypoints at the projections of a share of the points it sees, with pixel noise,
    descriptors a few bits away (some far), octaves at and around the predicted level, twins (the same descriptor a pixel away)
    and random decoys."""
    pose = kf_pose(P)
    cols = []
    for right in (0, 1):
        T = pose[right].astype(f64)
        pc = pts["pos"].astype(f64) @ T[:9].reshape(3, 3).T + T[9:12]
        uv = np.array([hg.kb8_project64(cams[right], p) for p in pc]).reshape(-1, 2)
        vis = np.nonzero((pc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < float(bounds.max_x)) & (uv[:, 1] >= 0) & (uv[:, 1] < float(bounds.max_y)))[0]
        vis = rng.permutation(vis)[:int(nfeat[right] * 0.55)]
        xs, ys, octs, ds = [], [], [], []

        def add(i, x, y, d, lev_off):
            lev = predict_scale(f32(float(pts["max_dist"][i]) / np.linalg.norm(pts["pos"][i].astype(f64) - T[12:15])))
            xs.append(x); ys.append(y); ds.append(d); octs.append(int(np.clip(lev + lev_off, 0, NLEVELS - 1)))
        for i in vis:
            x, y = uv[i, 0] + rng.normal(0, noise), uv[i, 1] + rng.normal(0, noise)
            d = flip_bits(rng, descs[i], int(rng.choice([0, 3, 10, 25, 45, 50, 51, 70])))
            off = int(rng.choice([0, 0, 0, -1, -1, 1, -2]))
            add(i, x, y, d, off)
            if rng.random() < 0.25:                                  # a twin: equal distance, a pixel away
                add(i, x + rng.uniform(-1.5, 1.5), y + rng.uniform(-1.5, 1.5), d, off)
        while len(xs) < nfeat[right]:                                # decoys
            xs.append(rng.uniform(0, float(bounds.max_x))); ys.append(rng.uniform(0, float(bounds.max_y)))
            octs.append(int(rng.integers(0, NLEVELS))); ds.append(rng.integers(0, 256, 32, dtype=np.uint8))
        order = rng.permutation(len(xs))[:nfeat[right]]
        cols.append((np.array(xs, f32)[order], np.array(ys, f32)[order], np.array(octs, np.int32)[order],
                     np.array(ds, np.uint8).reshape(-1, 32)[order]))
    cat = lambda j: np.concatenate([cols[0][j], cols[1][j]])
    return KF2(cat(0), cat(1), cat(2), cat(3), int(nfeat[0]), pose)


def settle(rng, pts, kfs, ths=(3.0, 4.0), skip=None):
    """Draws every point with an undecided pair again, until none is left -> points drawn again."""
    redrawn = 0
    for _ in range(8):
        und = set()
        for th in ths:
            und |= examine(pts, kfs, th, skip)[1]
        if not und:
            return redrawn
        for i in sorted({i for _, _, i in und}):
            fill_point(rng, pts, i, draw_point(rng))
            redrawn += 1
    raise AssertionError("the case does not settle")


def fuse2_case(seed, nkf, nmp=400, nfeat=(260, 190), noise=0.8):
    """-> Case: nmp points seen from a reference view, nkf target keyframes of the rig around it (unequal NLeft / NRight, the
    second one the other way round), skip[nkf, 2, nmp]."""
    rng = np.random.default_rng(seed)
    pts, descs = make_points2(rng, nmp)
    kfs = []
    for k in range(nkf):
        P = pose_from(*rng.uniform(-0.06, 0.06, 3), rng.uniform(-0.4, 0.4, 3))
        kfs.append(make_keyframe2(rng, pts, descs, P, nfeat if k % 2 == 0 else nfeat[::-1], noise))
    skip = (rng.random((nkf, 2, nmp)) < 0.1).astype(np.uint8)
    redrawn = settle(rng, pts, kfs)
    return Case(pts, descs, kfs, skip, redrawn)


_CORPUS = {}
SEEDS = {0: 40, 1: 42, 3: 63}                                        # nkf -> seed


def corpus(nkf):
    if nkf not in _CORPUS:
        _CORPUS[nkf] = fuse2_case(SEEDS[nkf], nkf)
    return _CORPUS[nkf]


SETTINGS = [(th, sk) for th in (3.0, 4.0) for sk in (False, True)]


# ---- tests ---------------------------------------------------------------------------------------------------------------------

def test_the_two_restatements_agree_and_every_exit_is_taken_on_both_sides():
    exits = {0: Counter(), 1: Counter()}
    matches = 0
    for nkf in (1, 3):
        C = corpus(nkf)
        assert C.redrawn == 0
        for th, sk in SETTINGS:
            for k, kf in enumerate(C.kfs):
                for right in (0, 1):
                    row = C.skip[k, right] if sk else None
                    a = fuse2_scalar(C.pts, C.descs, kf, bool(right), th, row, exits[right])
                    b = fuse2_fast(C.pts, C.descs, kf, bool(right), th, row)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (nkf, k, right, th, sk)
                    lo, hi = side_rows(kf, bool(right))
                    assert ((a[0] == -1) | ((a[0] >= lo) & (a[0] < hi))).all()       # a right winner is its local row + NLeft
                    matches += int((a[0] >= 0).sum())
    print("matches %d" % matches, {s: dict(e) for s, e in exits.items()})
    for side in (0, 1):
        for name in EXITS:
            assert exits[side][name] > 0, (side, name, dict(exits[side]))


def match_count(nkf, sides=3, th=3.0, sk=False):
    C = corpus(nkf)
    return int((fuse2_batch(C.pts, C.descs, C.kfs, th, sides, C.skip if sk else None)[0] >= 0).sum())


# the restatement's own counts for the committed seeds; tests/test_fuse_two_cameras_gpu.py takes half of them as its floor
MATCHES = {(1, 3.0): 108, (1, 4.0): 108, (3, 3.0): 358, (3, 4.0): 358}


def test_the_match_counts_the_gpu_floor_is_taken_from():
    for (nkf, th), want in MATCHES.items():
        assert match_count(nkf, 3, th) == want, (nkf, th, match_count(nkf, 3, th))


def test_points_that_only_one_camera_sees():
    C = corpus(3)
    lr = level_ratio()
    only = Counter()
    for kf in C.kfs:
        inside = [alive_of(C.pts, gates32(C.pts, kf.pose[r], CAMS[r], 3.0, lr), BOUNDS, None) for r in (0, 1)]
        only["left"] += int((inside[0] & ~inside[1]).sum())
        only["right"] += int((~inside[0] & inside[1]).sum())
    print(dict(only))
    assert only["left"] > 0 and only["right"] > 0


def test_margins_are_measured_again_and_every_decision_is_decided():
    worst = Counter()
    undecided = 0
    for nkf in (1, 3):
        C = corpus(nkf)
        for th in (3.0, 4.0):
            for sk in (None, C.skip):
                dev, und = examine(C.pts, C.kfs, th, sk)
                undecided += len(und)
                for k, v in dev.items():
                    worst[k] = max(worst[k], v)
    print("measured", {k: "%.3g" % v for k, v in worst.items()}, "undecided", undecided, "redrawn",
          sum(corpus(n).redrawn for n in (1, 3)))
    assert set(worst) == set(MEASURED)
    for k, v in worst.items():
        assert 0 < v <= MEASURED[k], (k, v)
    assert undecided == 0 and all(corpus(n).redrawn == 0 for n in (1, 3))


# ---- known answers -------------------------------------------------------------------------------------------------------------

Z32 = np.zeros(32, np.uint8)
P0 = Pose(np.eye(3, dtype=f32), np.zeros(3, f32))


def one_point(pos, max_dist=None):
    """A valid point, its normal along the ray from the origin, every distance admitted, level 0 from the origin."""
    pts = np.zeros(1, FUSE_POINT_DT)
    pos = np.asarray(pos, f32)
    n = float(np.linalg.norm(pos.astype(f64)))
    pts["pos"][0], pts["normal"][0] = pos, pos / f32(n)
    pts["min_dist_inv"], pts["max_dist_inv"] = 0.0, 1e9
    pts["max_dist"] = n if max_dist is None else max_dist
    pts["valid"] = 1
    return pts


def project_side(pts, pose, right):
    T = pose[1 if right else 0]
    p = np.array([gemm_row(T[3 * r:3 * r + 3], pts["pos"][0], T[9 + r]) for r in range(3)], f32)
    return oracle().kb8_project(np.asarray(CAMS[1 if right else 0], f32), p)


def kf2_of(left, right, pose=None):
    """left / right: lists of (x, y, desc[, octave])."""
    rows = list(left) + list(right)
    return KF2(np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32),
               np.array([r[3] if len(r) > 3 else 0 for r in rows], np.int32), np.array([r[2] for r in rows], np.uint8).reshape(-1, 32),
               len(left), kf_pose(P0) if pose is None else pose)


def both(pts, descs, kf, right, th=3.0, exits=None):
    a = fuse2_scalar(pts, descs, kf, right, th, None, exits)
    b = fuse2_fast(pts, descs, kf, right, th)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return int(a[0][0]), int(a[1][0])


def test_known_answer_a_point_on_the_optical_axis_projects_to_the_principal_point():
    cam = np.asarray(CAMS[0], f32)
    u, v = oracle().kb8_project(cam, np.array([0, 0, 3], f32))     # theta = atan2(0, 3) = 0, psi = atan2(0, 0) = 0, r = 0
    assert u == cam[2] and v == cam[3]
    pts = one_point([0, 0, 3])
    assert both(pts, Z32[None], kf2_of([(cam[2], cam[3], Z32)], []), False) == (0, 0)
    # the right camera looks 2 degrees to the side from 0.1 m away: it sees the point elsewhere, under its own pose and camera
    ur, vr = project_side(pts, kf_pose(P0), True)
    assert abs(float(ur) - float(CAMS[1][2])) > 5.0
    assert both(pts, Z32[None], kf2_of([(cam[2], cam[3], Z32)], [(ur, vr, Z32)]), True) == (1, 0)


def test_known_answer_equal_distances_the_earlier_in_visiting_order_wins_and_a_right_winner_is_its_row_plus_nleft():
    # ratio 2: level 4 (radius 6.2 px, the chi-square gate admits 5.07 px at octave 4), so that a cell border is within reach
    pts = one_point([0, 0, 3], max_dist=6.0)
    pose = kf_pose(P0)
    for right in (False, True):
        u, v = (float(c) for c in project_side(pts, pose, right))
        # cell columns are 8 px wide and PosInGrid rounds: the borders lie at 8 k + 4, the nearest at most 4 px from u
        border = round((u - 4.0) / 8.0) * 8.0 + 4.0
        assert abs(border - u) <= 4.0
        other = [(10.0, 10.0, Z32, 4)] * 3                            # three rows of the other camera
        mine = [(border + 0.4, v, Z32, 4), (border - 0.4, v, Z32, 4)]          # local row 1 lies in the smaller column: visited first
        kf = kf2_of(other, mine, pose) if right else kf2_of(mine, other, pose)
        ex = Counter()
        assert both(pts, Z32[None], kf, right, exits=ex) == ((3 + 1) if right else 1, 0) and ex["tie"] == 1
        # one cell: the list is in index order, the first keeps the strict minimum
        mine = [(border + 0.4, v, Z32, 4), (border + 0.2, v, Z32, 4)]
        kf = kf2_of(other, mine, pose) if right else kf2_of(mine, other, pose)
        ex = Counter()
        assert both(pts, Z32[None], kf, right, exits=ex) == (3 if right else 0, 0) and ex["tie"] == 1


def test_known_answer_a_keypoint_exactly_at_the_radius_is_outside():
    cam = np.asarray(CAMS[0], f32)
    pts = one_point([0, 0, 3])
    # th = 2: radius = 2 * mvScaleFactors[0] = 2 (with th = 3 the chi-square gate, 9 > 5.99, would hide the window's edge).
    # u = cx; cx - 2 is exact in float32 (the same binade), so |dx| == r exactly
    x_on = f32(cam[2] - f32(2.0))
    assert f32(x_on - cam[2]) == f32(-2.0)
    ex = Counter()
    assert both(pts, Z32[None], kf2_of([(x_on, cam[3], Z32)], []), False, th=2.0, exits=ex) == (-1, 256) and ex["empty_window"] == 1
    x_in = np.nextafter(x_on, f32(np.inf))
    assert both(pts, Z32[None], kf2_of([(x_in, cam[3], Z32)], []), False, th=2.0) == (0, 0)
    y_on = f32(cam[3] + f32(2.0))
    assert f32(y_on - cam[3]) == f32(2.0)
    assert both(pts, Z32[None], kf2_of([(cam[2], y_on, Z32)], []), False, th=2.0) == (-1, 256)


def test_known_answer_a_point_behind_the_image_plane_that_the_fisheye_model_projects_is_rejected():
    cam = np.asarray(CAMS[0], f32)
    pos = np.array([0.7071, 0.7071, -0.2], f32) * f32(2.0)           # 101 degrees off the axis, towards the image corner
    u, v = oracle().kb8_project(cam, pos)
    assert 0 <= u < 512 and 0 <= v < 512                             # KannalaBrandt8::project has no depth test
    pts = one_point(pos)
    kf = kf2_of([(u, v, Z32)], [])
    ex = Counter()
    assert both(pts, Z32[None], kf, False, exits=ex) == (-1, 256) and ex["neg_depth"] == 1          # :1459
    assert fuse2_scalar(pts, Z32[None], kf, False, rules=replace(REF, no_depth_gate=True))[0][0] == 0


@pytest.mark.parametrize("switch", ["left_pose_for_right", "left_cam_for_right", "left_grid_for_right", "no_nleft", "pinhole",
                                    "stereo_bound"])
def test_the_corpus_tells_a_wrong_reading_apart(switch):
    C = corpus(3)
    changed = 0
    for k, kf in enumerate(C.kfs):
        for right in (0, 1):
            a = fuse2_scalar(C.pts, C.descs, kf, bool(right), 3.0, C.skip[k, right])
            b = fuse2_scalar(C.pts, C.descs, kf, bool(right), 3.0, C.skip[k, right], rules=replace(REF, **{switch: True}))
            changed += int((a[0] != b[0]).sum())
    print(switch, changed)
    assert changed > 0


def test_the_binding_declares_the_entry_point():
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert re.search(r"pli_status\s+pli_fuse_search_two_cameras\s*\(", hdr)
    assert "pli_fuse_search_two_cameras" in capi._PROTOS and len(capi._PROTOS["pli_fuse_search_two_cameras"][1]) == 22
    assert hasattr(Frontend, "fuse_search_two_cameras")
