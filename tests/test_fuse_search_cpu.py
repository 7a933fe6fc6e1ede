"""The search half of ORBmatcher::Fuse (ORBmatcher.cc:1399-1609, bRight == false, NLeft == -1; the Sim3 overload :1611-1733 is the
same without the chi-square gate) restated twice in Python, CPU only:

  fuse_search_scalar   the reference's control flow, literally: the grid lists of Frame::AssignFeaturesToGrid, KeyFrame::
                       GetFeaturesInArea's loops, the running strict minimum; PredictScale by the direct expression.  It counts
                       every exit.
  fuse_search_fast     the closed form pli_fuse_search uses: vectorised gates, the level as a count of thresholds (level_ratio),
                       the winner as the minimum of the key (distance, cell column, cell row, index).

Float results follow the reference's operation order in np.float32 / np.float64 (a cv::Mat product: double accumulation, one
rounding; cv::norm and Mat::dot in double).  tests/test_fuse_search_gpu.py compares the device with these exactly."""
import math
import os
import re
import subprocess
from collections import Counter, namedtuple

import numpy as np

from helpers_matchers import GRID_COLS, GRID_ROWS, TH_LOW, c_round, hamming, scale_factors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
NLEVELS, SCALE = 8, 1.2
SF = scale_factors(NLEVELS, SCALE)[0]
INV_SIGMA2 = (f32(1.0) / (SF * SF).astype(f32)).astype(f32)        # mvInvLevelSigma2, ORBextractor.cc:424-431
FUSE_POINT_DT = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist_inv", "<f4"), ("max_dist_inv", "<f4"),
                          ("max_dist", "<f4"), ("valid", "<i4")])
Cam = namedtuple("Cam", "fx fy cx cy bf min_x max_x min_y max_y")
CAM = Cam(*[f32(v) for v in (435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297, 47.90639384423901,
                             0.0, 752.0, 0.0, 480.0)])
KF = namedtuple("KF", "x y octave desc uright pose")             # pose: 15 floats, Rcw row major, tcw, Ow
EXITS = ("not_valid", "skip", "neg_depth", "not_in_image", "dist_range", "normal", "empty_window", "level_gate", "chi2_stereo",
         "chi2_mono", "tie", "gt_th_low", "match")


def predict_scale(ratio, nlevels=NLEVELS, scale=SCALE):
    """MapPoint::PredictScale (MapPoint.cc:449-464), the logarithm of the float taken in double (this host's expression)."""
    ratio = float(f32(ratio))
    if not ratio > 0.0:
        return 0
    if math.isinf(ratio):
        return nlevels - 1
    n = math.ceil(math.log(ratio) / float(f32(math.log(float(f32(scale))))))
    return 0 if n < 0 else nlevels - 1 if n >= nlevels else int(n)


def level_ratio_table(nlevels=NLEVELS, scale=SCALE):
    from pli_slam_amd.frontend import fuse_level_ratio
    return fuse_level_ratio(nlevels, scale, lambda r: predict_scale(r, nlevels, scale))


_LR = {}


def level_ratio():
    if "t" not in _LR:
        _LR["t"] = level_ratio_table()
    return _LR["t"]


def gemm_row(R, p, t):
    """One row of Rcw * p + tcw as OpenCV's CV_32F gemm: the float products and the addend summed in double, one rounding."""
    return f32(f64(R[0]) * f64(p[0]) + f64(R[1]) * f64(p[1]) + f64(R[2]) * f64(p[2]) + f64(t))


# ---- the reference's control flow ----------------------------------------------------------------------------------------------

def fuse_search_scalar(points, descs, kf, cam, th=3.0, reproj_gate=True, skip=None, exits=None, misread=()):
    """-> best_idx[nmp], best_dist[nmp] for one keyframe; exits: a Counter of EXITS.  misread: deliberate misreadings of the
    reference that tests/test_ref_pin_match.py wants rejected ("min_le": <= in the running minimum; "octave_narrow": the octave
    window one level wide; "th_low_strict": bestDist < TH_LOW; "image_closed": the image gate closed at mnMaxX)."""
    exits = exits if exits is not None else Counter()
    n = len(kf.x)
    gw_inv = f32(f32(GRID_COLS) / f32(cam.max_x - cam.min_x))
    gh_inv = f32(f32(GRID_ROWS) / f32(cam.max_y - cam.min_y))
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
    for i in range(n):                                           # Frame::AssignFeaturesToGrid / PosInGrid
        px = int(c_round(f32(f32(kf.x[i] - cam.min_x) * gw_inv)))
        py = int(c_round(f32(f32(kf.y[i] - cam.min_y) * gh_inv)))
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid[px][py].append(i)
    R, t, Ow = kf.pose[:9].reshape(3, 3), kf.pose[9:12], kf.pose[12:15]
    th = f32(th)
    best_idx = np.full(len(points), -1, np.int32)
    best_dist = np.full(len(points), 256, np.int32)
    with np.errstate(all="ignore"):
        for i, P in enumerate(points):
            if not P["valid"]:
                exits["not_valid"] += 1; continue
            if skip is not None and skip[i]:
                exits["skip"] += 1; continue
            p = P["pos"]
            x, y, z = (gemm_row(R[r], p, t[r]) for r in range(3))
            if z < f32(0.0):
                exits["neg_depth"] += 1; continue
            invz = f32(f32(1.0) / z)
            u = f32(f32(f32(cam.fx * x) / z) + cam.cx)
            v = f32(f32(f32(cam.fy * y) / z) + cam.cy)
            if not (u >= cam.min_x and (u < cam.max_x or ("image_closed" in misread and u == cam.max_x)) and v >= cam.min_y and v < cam.max_y):
                exits["not_in_image"] += 1; continue
            ur = f32(u - f32(cam.bf * invz))
            PO = (p - Ow).astype(f32)
            dist3D = f32(math.sqrt(float(PO[0]) ** 2 + float(PO[1]) ** 2 + float(PO[2]) ** 2))
            if dist3D < P["min_dist_inv"] or dist3D > P["max_dist_inv"]:
                exits["dist_range"] += 1; continue
            Pn = P["normal"]
            if float(PO[0]) * float(Pn[0]) + float(PO[1]) * float(Pn[1]) + float(PO[2]) * float(Pn[2]) < 0.5 * float(dist3D):
                exits["normal"] += 1; continue
            level = predict_scale(f32(P["max_dist"] / dist3D))
            radius = f32(th * SF[level])
            # KeyFrame::GetFeaturesInArea
            idxs = []
            c0 = max(0, math.floor(f32(f32(f32(u - cam.min_x) - radius) * gw_inv)))
            c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(u - cam.min_x) + radius) * gw_inv)))
            r0 = max(0, math.floor(f32(f32(f32(v - cam.min_y) - radius) * gh_inv)))
            r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(v - cam.min_y) + radius) * gh_inv)))
            if c0 < GRID_COLS and c1 >= 0 and r0 < GRID_ROWS and r1 >= 0:
                for ix in range(c0, c1 + 1):
                    for iy in range(r0, r1 + 1):
                        for j in grid[ix][iy]:
                            if abs(f32(kf.x[j] - u)) < radius and abs(f32(kf.y[j] - v)) < radius:
                                idxs.append(j)
            if not idxs:
                exits["empty_window"] += 1; continue
            bd, bi = 256, -1
            for j in idxs:
                lev = int(kf.octave[j])
                if lev < level - (0 if "octave_narrow" in misread else 1) or lev > level:
                    exits["level_gate"] += 1; continue
                if reproj_gate:
                    ex, ey = f32(u - kf.x[j]), f32(v - kf.y[j])
                    if kf.uright[j] >= 0:
                        er = f32(ur - kf.uright[j])
                        e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                        if float(f32(e2 * INV_SIGMA2[lev])) > 7.8:
                            exits["chi2_stereo"] += 1; continue
                    else:
                        e2 = f32(f32(ex * ex) + f32(ey * ey))
                        if float(f32(e2 * INV_SIGMA2[lev])) > 5.99:
                            exits["chi2_mono"] += 1; continue
                d = int(hamming(descs[i], kf.desc[j]))
                if d == bd and bi >= 0:
                    exits["tie"] += 1
                if d < bd or ("min_le" in misread and d == bd):
                    bd, bi = d, j
            best_dist[i] = bd
            if bd <= TH_LOW - ("th_low_strict" in misread):
                best_idx[i] = bi
                exits["match"] += 1
            else:
                exits["gt_th_low"] += 1
    return best_idx, best_dist


# ---- the closed form -----------------------------------------------------------------------------------------------------------

def fuse_search_fast(points, descs, kf, cam, th=3.0, reproj_gate=True, skip=None, lr=None, info=None):
    """info (a dict, optional): "window_rows"[nmp], the rows inside every surviving point's window before the level gate."""
    lr = level_ratio() if lr is None else lr
    nmp, n = len(points), len(kf.x)
    best_idx = np.full(nmp, -1, np.int32)
    best_dist = np.full(nmp, 256, np.int32)
    if nmp == 0:
        return best_idx, best_dist
    R, t, Ow = kf.pose[:9].reshape(3, 3).astype(f64), kf.pose[9:12].astype(f64), kf.pose[12:15]
    pos = points["pos"]
    with np.errstate(all="ignore"):
        pc = [(R[r, 0] * pos[:, 0].astype(f64) + R[r, 1] * pos[:, 1].astype(f64) + R[r, 2] * pos[:, 2].astype(f64) + t[r]).astype(f32)
              for r in range(3)]
        x, y, z = pc
        invz = f32(1.0) / z
        u = (cam.fx * x) / z + cam.cx
        v = (cam.fy * y) / z + cam.cy
        ur = u - cam.bf * invz
        PO = pos - Ow[None, :]
        assert PO.dtype == f32 and u.dtype == f32 and ur.dtype == f32
        POd = PO.astype(f64)
        dist3D = np.sqrt(POd[:, 0] ** 2 + POd[:, 1] ** 2 + POd[:, 2] ** 2).astype(f32)
        Pn = points["normal"].astype(f64)
        dot = POd[:, 0] * Pn[:, 0] + POd[:, 1] * Pn[:, 1] + POd[:, 2] * Pn[:, 2]
        ok = points["valid"] != 0
        if skip is not None:
            ok &= np.asarray(skip) == 0
        ok &= ~(z < 0) & (u >= cam.min_x) & (u < cam.max_x) & (v >= cam.min_y) & (v < cam.max_y)
        ok &= ~((dist3D < points["min_dist_inv"]) | (dist3D > points["max_dist_inv"])) & ~(dot < 0.5 * dist3D.astype(f64))
        ratio = points["max_dist"] / dist3D
        level = (ratio[:, None] > lr[None, :]).sum(1)
        radius = f32(th) * SF[level]
        assert radius.dtype == f32
    sel = np.nonzero(ok)[0]
    if n == 0 or len(sel) == 0:
        return best_idx, best_dist
    gw_inv = f32(f32(GRID_COLS) / f32(cam.max_x - cam.min_x))
    gh_inv = f32(f32(GRID_ROWS) / f32(cam.max_y - cam.min_y))
    rnd = lambda a: (np.sign(a) * np.floor(np.abs(a).astype(f64) + 0.5)).astype(np.int64)
    px, py = rnd((kf.x - cam.min_x) * gw_inv), rnd((kf.y - cam.min_y) * gh_inv)
    in_grid = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    octave = kf.octave.astype(np.int64)
    base_key = (px << 34) | (py << 28) | np.arange(n, dtype=np.int64)
    chunk = max(1, 400000 // n)
    for s0 in range(0, len(sel), chunk):
        s = sel[s0:s0 + chunk]
        us, vs, rs, lv = u[s, None], v[s, None], radius[s, None], level[s, None]
        c0 = np.maximum(0, np.floor(((us - cam.min_x) - rs) * gw_inv)).astype(np.int64)
        c1 = np.minimum(GRID_COLS - 1, np.ceil(((us - cam.min_x) + rs) * gw_inv)).astype(np.int64)
        r0 = np.maximum(0, np.floor(((vs - cam.min_y) - rs) * gh_inv)).astype(np.int64)
        r1 = np.minimum(GRID_ROWS - 1, np.ceil(((vs - cam.min_y) + rs) * gh_inv)).astype(np.int64)
        cand = in_grid[None, :] & (px[None, :] >= c0) & (px[None, :] <= c1) & (py[None, :] >= r0) & (py[None, :] <= r1)
        cand &= (np.abs(kf.x[None, :] - us) < rs) & (np.abs(kf.y[None, :] - vs) < rs)
        if info is not None:
            info.setdefault("window_rows", np.zeros(nmp, np.int64))[s] = cand.sum(1)
        cand &= (octave[None, :] >= lv - 1) & (octave[None, :] <= lv)
        if reproj_gate:
            ex, ey, er = us - kf.x[None, :], vs - kf.y[None, :], ur[s, None] - kf.uright[None, :]
            e_mono = ex * ex + ey * ey
            e_st = e_mono + er * er
            assert e_st.dtype == f32
            inv = INV_SIGMA2[octave][None, :]
            st = (kf.uright >= 0)[None, :]
            cand &= np.where(st, ~((e_st * inv).astype(f64) > 7.8), ~((e_mono * inv).astype(f64) > 5.99))
        rows, cols = np.nonzero(cand)
        if len(rows) == 0:
            continue
        d = hamming(descs[s[rows]], kf.desc[cols]).astype(np.int64)
        key = (d << 40) | base_key[cols]
        best = np.full(len(s), np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, rows, key)
        has = best != np.iinfo(np.int64).max
        bd = (best >> 40).astype(np.int32)
        best_dist[s[has]] = bd[has]
        win = has & (bd <= TH_LOW)
        best_idx[s[win]] = (best[win] & 0xFFFFFFF).astype(np.int32)
    return best_idx, best_dist


def fuse_search_batch(points, descs, kfs, cam, th=3.0, reproj_gate=True, skip=None, fn=fuse_search_fast):
    bi = np.full((len(kfs), len(points)), -1, np.int32)
    bd = np.full((len(kfs), len(points)), 256, np.int32)
    for k, kf in enumerate(kfs):
        bi[k], bd[k] = fn(points, descs, kf, cam, th, reproj_gate, None if skip is None else skip[k])
    return bi, bd


# ---- constructed scenes --------------------------------------------------------------------------------------------------------

def rot_xyz(a, b, c):
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    return (np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @
            np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))


def make_pose(R, t):
    R32, t32 = np.asarray(R, f32), np.asarray(t, f32)
    Ow = (-R32.astype(f64).T @ t32.astype(f64)).astype(f32)          # the stored camera centre
    return np.concatenate([R32.reshape(9), t32, Ow]).astype(f32)


IDENTITY = make_pose(np.eye(3), np.zeros(3))


def flip_bits(rng, desc, nbits):
    d = np.unpackbits(desc.copy())
    d[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(d)


def make_points(rng, nmp, cam=CAM):
    """Points seen from a reference view at the origin: normals towards it (some grazing), distance ranges from a random level of
    that view (some far too narrow), some behind the camera, some invalid."""
    pts = np.zeros(nmp, FUSE_POINT_DT)
    u, v, z = rng.uniform(-60, 812, nmp), rng.uniform(-40, 520, nmp), rng.uniform(2.0, 20.0, nmp)
    z[rng.random(nmp) < 0.04] *= -1
    pos = np.stack([(u - float(cam.cx)) * z / float(cam.fx), (v - float(cam.cy)) * z / float(cam.fy), z], 1)
    dist = np.linalg.norm(pos, axis=1)
    normal = pos / dist[:, None]
    for i in np.nonzero(rng.random(nmp) < 0.25)[0]:                  # grazing: up to ~75 degrees off the viewing ray
        normal[i] = rot_xyz(*rng.uniform(-0.9, 0.9, 3)) @ normal[i]
    lev = rng.integers(0, NLEVELS, nmp)
    max_d = dist * SF[lev].astype(f64) * rng.uniform(0.9, 1.1, nmp)
    narrow = rng.random(nmp) < 0.08
    max_d[narrow] *= rng.choice([0.2, 6.0], narrow.sum())
    min_d = max_d / float(SF[-1])
    pts["pos"], pts["normal"] = pos.astype(f32), normal.astype(f32)
    pts["max_dist"] = max_d.astype(f32)
    pts["min_dist_inv"] = f32(0.8) * min_d.astype(f32)
    pts["max_dist_inv"] = f32(1.2) * max_d.astype(f32)
    pts["valid"] = (rng.random(nmp) > 0.03).astype(np.int32)
    descs = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
    return pts, descs


def make_keyframe(rng, pts, descs, pose, nfeat, cam=CAM, noise=0.8):
    """Keypoints at the projections of a share of the points, with pixel noise, descriptors a few bits away (some far), octaves at
    and around the predicted level, twins (the same descriptor a pixel away) and random decoys; 60 % stereo rows."""
    R, t, Ow = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64), pose[12:15].astype(f64)
    pc = pts["pos"].astype(f64) @ R.T + t
    with np.errstate(all="ignore"):
        u = float(cam.fx) * pc[:, 0] / pc[:, 2] + float(cam.cx)
        v = float(cam.fy) * pc[:, 1] / pc[:, 2] + float(cam.cy)
    vis = np.nonzero((pc[:, 2] > 0) & (u >= 0) & (u < 752) & (v >= 0) & (v < 480))[0]
    vis = rng.permutation(vis)[:int(nfeat * 0.55)]
    xs, ys, octs, ds, urs = [], [], [], [], []

    def add(i, x, y, d, lev_off):
        dist = np.linalg.norm(pts["pos"][i].astype(f64) - Ow)
        lev = predict_scale(f32(float(pts["max_dist"][i]) / dist))
        xs.append(x); ys.append(y); ds.append(d)
        octs.append(int(np.clip(lev + lev_off, 0, NLEVELS - 1)))
        if rng.random() < 0.6:
            urs.append(x - float(cam.bf) / pc[i, 2] + rng.normal(0, noise * (3.0 if rng.random() < 0.2 else 1.0)))
        else:
            urs.append(-1.0)
    for i in vis:
        x, y = u[i] + rng.normal(0, noise), v[i] + rng.normal(0, noise)
        d = flip_bits(rng, descs[i], int(rng.choice([0, 3, 10, 25, 45, 50, 51, 70])))
        off = int(rng.choice([0, 0, 0, -1, -1, 1, -2]))
        add(i, x, y, d, off)
        if rng.random() < 0.25:                                      # a twin: equal distance, a pixel away
            add(i, x + rng.uniform(-1.5, 1.5), y + rng.uniform(-1.5, 1.5), d, off)
    while len(xs) < nfeat:                                           # decoys
        xs.append(rng.uniform(0, 752)); ys.append(rng.uniform(0, 480)); octs.append(int(rng.integers(0, NLEVELS)))
        ds.append(rng.integers(0, 256, 32, dtype=np.uint8)); urs.append(rng.choice([-1.0, rng.uniform(0, 700)]))
    order = rng.permutation(len(xs))[:nfeat]
    return KF(np.array(xs, f32)[order], np.array(ys, f32)[order], np.array(octs, np.int32)[order],
              np.array(ds, np.uint8).reshape(-1, 32)[order], np.array(urs, f32)[order], pose)


def fuse_case(rng, nkf, nmp, nfeat=400):
    """-> points, descs, [KF] * nkf, skip[nkf, nmp]"""
    pts, descs = make_points(rng, nmp)
    kfs = []
    for _ in range(nkf):
        pose = make_pose(rot_xyz(*rng.uniform(-0.06, 0.06, 3)), rng.uniform(-0.6, 0.6, 3))
        kfs.append(make_keyframe(rng, pts, descs, pose, nfeat))
    skip = (rng.random((nkf, nmp)) < 0.1).astype(np.uint8)
    return pts, descs, kfs, skip


SEEDED = [(seed, nkf, nmp) for seed, nkf, nmp in ((1, 3, 300), (2, 2, 400), (3, 4, 250))]


# ---- tests ---------------------------------------------------------------------------------------------------------------------

def test_the_two_restatements_agree_and_every_exit_is_taken():
    exits = Counter()
    for seed, nkf, nmp in SEEDED:
        rng = np.random.default_rng(seed)
        pts, descs, kfs, skip = fuse_case(rng, nkf, nmp)
        for gate, th, sk in ((True, 3.0, skip), (False, 4.0, None), (True, 4.0, None)):
            for k, kf in enumerate(kfs):
                row = None if sk is None else sk[k]
                a = fuse_search_scalar(pts, descs, kf, CAM, th, gate, row, exits)
                b = fuse_search_fast(pts, descs, kf, CAM, th, gate, row)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (seed, k, gate, th)
    print(dict(exits))
    for name in EXITS:
        assert exits[name] > 0, (name, dict(exits))


def one_point(pos, max_dist=None, normal=None):
    """A valid point in front of the identity camera, its normal along the viewing ray, every distance admitted."""
    pts = np.zeros(1, FUSE_POINT_DT)
    pos = np.asarray(pos, f32)
    pts["pos"][0] = pos
    n = np.linalg.norm(pos.astype(f64))
    pts["normal"][0] = (pos / n if n > 0 else [0, 0, 1]) if normal is None else normal
    pts["min_dist_inv"], pts["max_dist_inv"] = 0.0, 1e9
    pts["max_dist"] = n if max_dist is None else max_dist                # ratio 1: level 0
    pts["valid"] = 1
    return pts


def project(pts, pose=IDENTITY, cam=CAM):
    """u, v, ur of point 0 by the restatement's own expressions."""
    R, t = pose[:9].reshape(3, 3), pose[9:12]
    x, y, z = (gemm_row(R[r], pts["pos"][0], t[r]) for r in range(3))
    u = f32(f32(f32(cam.fx * x) / z) + cam.cx)
    v = f32(f32(f32(cam.fy * y) / z) + cam.cy)
    return u, v, f32(u - f32(cam.bf * f32(f32(1.0) / z)))


def kf_of(xs, ys, descs, octaves=None, uright=None, pose=IDENTITY):
    n = len(xs)
    return KF(np.array(xs, f32), np.array(ys, f32), np.zeros(n, np.int32) if octaves is None else np.array(octaves, np.int32),
              np.array(descs, np.uint8).reshape(n, 32), np.full(n, -1, f32) if uright is None else np.array(uright, f32), pose)


def both(pts, descs, kf, cam=CAM, th=3.0, gate=True, exits=None):
    a = fuse_search_scalar(pts, descs, kf, cam, th, gate, None, exits)
    b = fuse_search_fast(pts, descs, kf, cam, th, gate, None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return int(a[0][0]), int(a[1][0])


def point_at_pixel(u, v, z=4.0, cam=CAM):
    return one_point([(u - float(cam.cx)) * z / float(cam.fx), (v - float(cam.cy)) * z / float(cam.fy), z])


def test_known_answer_equal_distances_the_earlier_in_visiting_order_wins():
    d = np.arange(32, dtype=np.uint8)
    pts = point_at_pixel(100.0, 100.0)
    u, v, _ = project(pts)
    assert abs(u - 100) < 1e-3 and abs(v - 100) < 1e-3
    # cell columns are 11.75 px wide and PosInGrid rounds: x = 101 lies in column 9, x = 99 in column 8.  Index 1 is visited
    # first (the smaller column) although its index is larger.
    ex = Counter()
    assert both(pts, d[None], kf_of([101, 99], [100, 100], [d, d]), exits=ex) == (1, 0) and ex["tie"] == 1
    # one cell (column 9): the list is in index order, the first keeps the strict minimum
    ex = Counter()
    assert both(pts, d[None], kf_of([102, 101], [100, 100], [d, d]), exits=ex) == (0, 0) and ex["tie"] == 1
    # rows are 10 px high: y = 106 is row 11, y = 94 row 9; same column: the smaller row first
    assert both(pts, d[None], kf_of([100.5, 100.5], [106, 94], [d, d]), th=7.0, gate=False) == (1, 0)


def test_known_answer_chi_square_gates():
    rng = np.random.default_rng(0)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    d5 = flip_bits(rng, d, 5)
    pts = point_at_pixel(300.0, 200.0)
    u, v, ur = project(pts)
    # mono, octave 0 (sigma2 = 1): ex = 2.45 -> e2 = 6.0025 > 5.99 rejected; ex = 2.44 -> 5.9536 kept
    ex = Counter()
    kf = kf_of([float(u) - 2.45, float(u) - 2.44], [v, v], [d, d5])
    assert both(pts, d[None], kf, exits=ex) == (1, 5) and ex["chi2_mono"] == 1
    assert both(pts, d[None], kf, gate=False) == (0, 0)              # the Sim3 overload has no such gate
    # stereo: er = 2.80 -> 7.84 > 7.8 rejected; er = 2.79 -> 7.7841 kept (and would fail the mono limit)
    ex = Counter()
    kf = kf_of([u, u], [v, v], [d, d5], uright=[float(ur) - 2.80, float(ur) - 2.79])
    assert both(pts, d[None], kf, exits=ex) == (1, 5) and ex["chi2_stereo"] == 1
    # the same error on a mono row is not read at all
    assert both(pts, d[None], kf_of([u, u], [v, v], [d, d5]))[0] == 0


def test_known_answer_depth_zero_and_the_right_image_edge():
    d = np.zeros(32, np.uint8)
    # z == 0 is not "negative depth" (:1448 asks z < 0): the projection is inf / NaN and the image test rejects it
    ex = Counter()
    pts = one_point([1.0, 1.0, 0.0], normal=[0, 0, 1])
    assert both(pts, d[None], kf_of([10], [10], [d]), exits=ex) == (-1, 256) and ex["not_in_image"] == 1 and ex["neg_depth"] == 0
    ex = Counter()
    pts = one_point([0.0, 0.0, 0.0], normal=[0, 0, 1])
    assert both(pts, d[None], kf_of([10], [10], [d]), exits=ex) == (-1, 256) and ex["not_in_image"] == 1
    # u == max_x exactly is outside (IsInImage: x < mnMaxX); a few floats below is inside
    cam = CAM._replace(fx=f32(400.0), cx=f32(352.0), cy=f32(240.0))
    ex = Counter()
    pts = one_point([1.0, 0.0, 1.0])
    assert project(pts, cam=cam)[0] == f32(752.0)
    # (a keypoint right of x = 746.125 rounds to column 64 and is in no cell: the candidate sits at 746)
    edge = kf_of([746.0], [240], [d])
    assert both(pts, d[None], edge, cam=cam, th=7.0, gate=False, exits=ex) == (-1, 256) and ex["not_in_image"] == 1
    pts = one_point([f32(0.999999), 0.0, 1.0])
    assert project(pts, cam=cam)[0] < f32(752.0)
    assert both(pts, d[None], edge, cam=cam, th=7.0, gate=False) == (0, 0)
    assert both(pts, d[None], kf_of([751.5], [240], [d]), cam=cam, th=7.0, gate=False) == (-1, 256)


def test_known_answer_a_ratio_exactly_at_a_level_boundary():
    d = np.zeros(32, np.uint8)
    lr = level_ratio()
    for n in (0, 3, NLEVELS - 2):
        # dist3D = 4 exactly; max_dist = 4 * level_ratio[n]: the ratio IS the threshold -> level n; one float more -> n + 1.
        # A keypoint of octave n + 1 is admitted by [level - 1, level] only in the second case.
        for bump, want in ((False, -1), (True, 0)):
            r = np.nextafter(lr[n], f32(np.inf)) if bump else lr[n]
            pts = one_point([0.0, 0.0, 4.0], max_dist=f32(4.0) * r)
            assert f32(pts["max_dist"][0] / f32(4.0)) == r
            assert predict_scale(r) == n + (1 if bump else 0)
            u, v, _ = project(pts)
            assert both(pts, d[None], kf_of([u], [v], [d], octaves=[n + 1]), gate=False)[0] == want, (n, bump)


def test_level_ratio_is_the_direct_expression_as_thresholds():
    lr = level_ratio()
    assert len(lr) == NLEVELS - 1 and (np.diff(lr) > 0).all()
    count = lambda r: int((f32(r) > lr).sum())
    for n in range(NLEVELS - 1):
        bits = int(lr[n].view(np.uint32))
        near = np.arange(bits - 2000, bits + 2001, dtype=np.uint32).view(f32)
        for r in near:
            assert count(r) == predict_scale(r), (n, r)
    rng = np.random.default_rng(7)
    ratios = np.exp(rng.uniform(math.log(0.05), math.log(40.0), 1000000)).astype(f32)
    got = (ratios[:, None] > lr[None, :]).sum(1)
    lsf = float(f32(math.log(float(f32(SCALE)))))
    want = np.fromiter((min(max(math.ceil(math.log(r) / lsf), 0), NLEVELS - 1) for r in ratios.astype(f64).tolist()), np.int64,
                       len(ratios))
    assert np.array_equal(got, want)
    assert set(np.unique(got)) == set(range(NLEVELS))
    for r in (0.0, -1.0, float("inf"), 1e-45):
        assert count(r) == predict_scale(r)


def test_the_binding_declares_the_entry_point():
    from pli_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert re.search(r"pli_status\s+pli_fuse_search\s*\(", hdr) and "typedef struct pli_fuse_point" in hdr
    assert "pli_fuse_search" in capi._PROTOS and len(capi._PROTOS["pli_fuse_search"][1]) == 17
    assert capi.FUSE_POINT_DT.itemsize == 40 and capi.FUSE_POINT_DT == FUSE_POINT_DT
    import ctypes as C
    assert C.sizeof(capi.FuseCamera) == 36
    from pli_slam_amd.frontend import Frontend, fuse_level_ratio, predict_scale as ps
    assert hasattr(Frontend, "fuse_search")
    assert np.array_equal(fuse_level_ratio(NLEVELS, SCALE), level_ratio())
    assert all(ps(r, NLEVELS, SCALE) == predict_scale(r) for r in (0.3, 1.0, 1.2, 1.21, 3.0, 100.0))


def test_the_fuse_adapters_compile_against_stub_types(tmp_path):
    """A syntax check of PliORBmatcher::Fuse (three forms) against the stub KeyFrame / MapPoint of the harness."""
    src = os.path.join(ROOT, "tests", "cpp", "fuse_search_harness.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
