"""LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684), the branch of keyframes with two KannalaBrandt8
cameras (:463-528), restated for the tests of pli_create_new_map_points_two_cameras: CPU only.

  * scene                  one keyframe and up to 10 neighbours that look at shared world points: about 210 left + 180 right rows a
                           keyframe, every world point its own BoW node and code row, noise that grows with the octave, far points,
                           decoys (a neighbour's feature anywhere in the image, in the point's node) and map points already set.  A
                           point is drawn again while one of its pairs is undecided for the SEARCH's gate (the float64 gate of
                           tests/test_triangulation_two_cameras_cpu.py, its margins): the tables leave 0 undecided pairs;
  * w_zero_scene, gate_599_scene, dist_zero_scene
                           what no seeded scene reaches: one-pair calls for w == 0 (:565) and for a chi-square between 5.99 and
                           5.991 sigma2, and dist == 0 (:657) as a second pass over a seeded scene;
  * pair_kb8               :530-667 for one pair, scalar float32 in the reference's control flow and OpenCV's cv::Mat conventions
                           (helpers_new_map_points.py states them), from pyoracle.kb8_unproject / kb8_project and
                           helpers_new_map_points.svd_last_vt4: neither the camera model nor the Jacobi is stated again;
  * create_new_map_points  the literal loop: per neighbour the search (search_scalar) on the CURRENT map-point state, :530-667 per
                           pair, has_mp set on success;
  * closed_form            all pairs on the state at entry, then first-accepted-wins per feature: what the device does;
  * pair_f64               an independent float64 statement: 4x4 homogeneous poses, np.linalg.inv, np.linalg.svd,
                           helpers_geometry.kb8_unproject64 / kb8_project64; the stored Ow is not read.

What the branch reads: kp = mvKeys[idx] / mvKeysRight[idx - NLeft]; bStereo1 = bStereo2 = false, so :550 is
0 < cosParallaxRays < 0.9998 and everything else "low parallax"; per pair (bRight1, bRight2) pick pose and camera of each side.
`cosParallaxRays < 0.9998` compares a float with a double; comparing with 0.9998f instead cannot be told apart by any float, because
0.9998f = 0.99980002... lies above 0.9998 and its predecessor below (tests/test_new_map_points_two_cameras_cpu.py asserts that).

Recorded, float32 restatement against pair_f64 on SEEDS with bCoarse on and off, over the pairs whose float64 margins exceed these
very figures (tests/test_new_map_points_two_cameras_cpu.py measures them again on every run, prints them and fails when a run
measures more): MEASURED below, the figures beside it.
"""
import math
from collections import Counter, namedtuple

import numpy as np

import helpers_geometry as hg
import test_triangulation_two_cameras_cpu as two
from helpers_new_map_points import CODE, CREATED, NOT_MATCHED, STATUS, TAKEN_EARLIER, svd_last_vt4
from test_triangulation_two_cameras_cpu import (CAMS, SIGMA2, TLR_T, Gate, Neighbour, Pose, gemm, make_table, pose_from,
                                                relative_poses, search_closed, search_scalar)

F32 = np.float32
f64 = np.float64
SCALE32 = np.array([F32(1)] * two.NLEVELS, F32)                       # mvScaleFactors: 1, then * 1.2f in float (ORBextractor.cc)
for _i in range(1, two.NLEVELS):
    SCALE32[_i] = F32(SCALE32[_i - 1] * F32(1.2))
SIGMA32 = np.array([F32(s * s) for s in SCALE32], F32)               # mvLevelSigma2 = mvScaleFactor^2 in float
RATIO_FACTOR = F32(F32(1.5) * F32(1.2))
TH_FAR = 5.5

# statuses that can occur in this branch (no stereo feature: EMPTY_UNPROJECT and both *_STEREO cannot)
REACHABLE = ("created", "low_parallax", "w_zero", "z1", "z2", "reproj1_mono", "reproj2_mono", "dist_zero", "far", "ratio_low",
             "ratio_high", "taken_earlier", "not_matched")

# ---- measured on the CPU over SEEDS, both settings of bCoarse (float32 restatement against pair_f64), rounded up -------------
# worst seen over 17869 pairs: cos 2.94e-7, px 2.63e-4, z 2.66e-4 and dist 2.33e-4 relative beyond 1 m, ratio 1.33e-6, x3d 2.16e-4
# relative to its norm (the large ones are points near cos = 0.9998, tens of metres away, that bCoarse lets through); 14 pairs
# (0.08 %) have a smaller float64 margin and are excluded; the nearest 5.991 sigma2 comparison is 57360 float ulps away
MEASURED = {"cos": 3.5e-7, "px": 3.5e-4, "z": 3.5e-4, "dist": 3e-4, "ratio": 2e-6, "x3d_rel": 3e-4}
SEEDS = (5, 6, 8)

# one keyframe: its search table (mvKeys then mvKeysRight) and 2 x 15 floats of pose (left, right: Rcw row major, tcw, Ow)
KF = namedtuple("KF", "t pose")
NB = namedtuple("NB", "kf rel ep")


def pose30(p):
    """Both sides of a keyframe as the reference's getters give them (KeyFrame.cc:1343-1373): cv::Mat expressions, one gemm each."""
    Ow = p.centre()
    Owr = gemm(p.R.T, TLR_T, 1.0, Ow)                                  # GetRightCameraCenter: Rwl * tlr + twl
    left = np.concatenate([p.R.reshape(9), p.t.reshape(3), Ow.reshape(3)])
    right = np.concatenate([p.right_rotation().reshape(9), p.right_translation().reshape(3), Owr.reshape(3)])
    return np.stack([left, right]).astype(F32)


def search_nb(nb):
    return Neighbour(nb.kf.t, nb.rel, nb.ep)


# ---- the scene --------------------------------------------------------------------------------------------------------------
def _world_to_cam(pose15):
    T = np.eye(4)
    T[:3, :3] = np.asarray(pose15[:9], f64).reshape(3, 3)
    T[:3, 3] = np.asarray(pose15[9:12], f64)
    return T


def _pair_undecided(f1, f2, rel):
    r1, r2 = f1[0], f2[0]
    which = 2 * r1 + r2
    _, mg, _ = hg.fisheye_expect(f1[1:4], f2[1:4], CAMS[r1], CAMS[r2], rel[which, :9], rel[which, 9:], SIGMA2)
    corner = max(two.off_axis(CAMS[r1], f1[1], f1[2]), two.off_axis(CAMS[r2], f2[1], f2[2])) > two.CORNER_RAD
    return two.undecided(mg, corner)


_SCENES = {}


def scene(seed, nkf=10, npoints=262):
    """-> (kf1: KF, nbrs: [NB], info: dict(redrawn, seen3)).  Cached: the tables are not changed by their users."""
    if (seed, nkf, npoints) in _SCENES:
        return _SCENES[(seed, nkf, npoints)]
    rng = np.random.default_rng(seed)
    p1 = pose_from(0.01, -0.02, 0.015, (0.0, 0.0, 0.0))
    poses = []
    for k in range(nkf):
        d = rng.normal(size=3)
        d[2] *= 0.4
        c = d / np.linalg.norm(d) * rng.uniform(0.25, 0.6)
        poses.append(pose_from(*rng.uniform(-0.06, 0.06, 3), c))
    P30 = [pose30(p1)] + [pose30(p) for p in poses]
    Tw = [[_world_to_cam(p[s]) for s in (0, 1)] for p in P30]
    rels = [relative_poses(p1, p) for p in poses]
    T1inv = np.linalg.inv(Tw[0][0])
    rows = [([], []) for _ in range(nkf + 1)]                       # per keyframe: (left rows, right rows)
    redrawn, seen3 = 0, 0

    def image(kf, s, X):
        Xc = Tw[kf][s] @ np.append(X, 1.0)
        if Xc[2] < 0.05:
            return None
        uv = hg.kb8_project64(CAMS[s], Xc[:3])
        return uv if all(25 < v < 487 for v in uv) else None

    for node in range(npoints):
        kind = "decoy" if node % 11 == 3 else "far" if node % 9 == 4 else "point"
        while True:
            depth = rng.uniform(25, 70) if kind == "far" else rng.uniform(0.6, 6.0)
            X = (T1inv @ np.append(hg._direction(rng, 0.02, 0.75) * depth, 1.0))[:3]
            code = hg.code_rows(1, node % 512)[0]
            base = int(rng.integers(0, 8))
            feats = []                                            # per keyframe: [(side, x, y, octave, desc, has_mp)]
            for kf in range(nkf + 1):
                fk = []
                for s in (0, 1):
                    if rng.random() > ((0.82, 0.72)[s] if kf == 0 else (0.80, 0.69)[s]):
                        continue
                    o = int(np.clip(base + rng.integers(-2, 3), 0, 7)) if rng.random() < 0.75 else int(rng.integers(0, 8))
                    if kind == "decoy" and kf > 0:
                        uv = rng.uniform(60, 450, 2)
                    else:
                        uv = image(kf, s, X)
                        if uv is None:
                            continue
                        uv = uv + rng.normal(0, 0.7 * 1.2 ** o, 2)
                        if not all(20 < v < 492 for v in uv):
                            continue
                    mp = int(rng.random() < (0.12 if kf == 0 else 0.06))
                    fk.append((s, F32(uv[0]), F32(uv[1]), o, hg.flip_bits(code, int(rng.integers(0, 10)), rng), mp))
                feats.append(fk)
            if not any(_pair_undecided(a, b, rels[k]) for k in range(nkf) for a in feats[0] for b in feats[k + 1]):
                break
            redrawn += 1
        if feats[0] and sum(1 for k in range(nkf) if feats[k + 1]) >= 3:
            seen3 += len(feats[0])
        for kf in range(nkf + 1):
            for s, x, y, o, desc, mp in feats[kf]:
                rows[kf][s].append((x, y, o, 0.0, desc, node, mp))
    # a node that one side lists alone and a feature in no node, on either side of NLeft
    for kf in range(nkf + 1):
        for s in (0, 1):
            rows[kf][s].append((F32(100 + kf), F32(100), 0, 0.0, hg.code_rows(1, 7)[0], npoints + 1 + kf, 0))
            rows[kf][s].append((F32(120), F32(100 + kf), 0, 0.0, hg.code_rows(1, 9)[0], -1, 0))
    tabs = [two._shuffled(r, rng) for r in rows]
    kf1 = KF(tabs[0], P30[0])
    nbrs = [NB(KF(tabs[k + 1], P30[k + 1]), rels[k], two.epipole(p1, poses[k])) for k in range(nkf)]
    out = (kf1, nbrs, dict(redrawn=redrawn, seen3=seen3))
    _SCENES[(seed, nkf, npoints)] = out
    return out


_GATES = {}


def gates(kf1, nbrs):
    """One float64 gate per neighbour, remembered per pair: it reads coordinates, octaves and NLeft, never has_mp."""
    key = (id(kf1.t), tuple(id(nb.kf.t) for nb in nbrs))
    if key not in _GATES:
        _GATES[key] = [Gate(kf1.t, search_nb(nb)) for nb in nbrs]
    return _GATES[key]


def side(kf, i):
    """What :530-667 read of feature i of a keyframe."""
    t = kf.t
    r = int(i >= t.nleft)
    return dict(x=F32(t.x[i]), y=F32(t.y[i]), octave=int(t.octave[i]), right=r, pose2=kf.pose)


# ---- :530-667, scalar float32 ---------------------------------------------------------------------------------------------
def _dotd(a, b):
    return float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2])


def _normd(a):
    return math.sqrt(_dotd(a, a))


def _gemm_t(R9, r, v):
    """row r of Rcw.t() * v as a CV_32F gemm"""
    return F32(float(R9[r]) * float(v[0]) + float(R9[3 + r]) * float(v[1]) + float(R9[6 + r]) * float(v[2]))


def _pick(S1, S2, rules):
    """(pose15, camera) of each side, as (bRight1, bRight2) pick them (:463-528)."""
    r1, r2 = S1["right"], S2["right"]
    p1, p2, c1, c2 = r1, r2, r1, r2
    if "left_pose_for_right" in rules:
        p1, p2 = 0, 0
    if "left_cam_for_right" in rules:
        c1, c2 = 0, 0
    if "swap_rr_ll" in rules and r1 == r2:
        p1 = p2 = c1 = c2 = 1 - r1
    return S1["pose2"][p1], S2["pose2"][p2], CAMS[c1], CAMS[c2]


def pair_kb8(po, S1, S2, far=False, th_far=0.0, ratio_factor=RATIO_FACTOR, rules=(), q=None):
    """-> (status code, x3D as 3 float32 or None).  rules: deliberate misreadings ("left_pose_for_right", "left_cam_for_right",
    "swap_rr_ll", "gate_599").  q (a dict) takes the compared quantities."""
    q = q if q is not None else {}
    gate = 5.99 if "gate_599" in rules else 5.991
    with np.errstate(all="ignore"):
        th_far, ratio_factor = F32(th_far), F32(ratio_factor)
        T1, T2, cam1, cam2 = _pick(S1, S2, rules)
        xn1 = po.kb8_unproject(cam1, S1["x"], S1["y"])             # unprojectMat(kp.pt): KannalaBrandt8::unproject, z = 1
        xn2 = po.kb8_unproject(cam2, S2["x"], S2["y"])
        ray1 = [_gemm_t(T1, r, xn1) for r in range(3)]
        ray2 = [_gemm_t(T2, r, xn2) for r in range(3)]
        cos_rays = F32(_dotd(ray1, ray2) / (_normd(ray1) * _normd(ray2)))
        cs = F32(cos_rays + F32(1))                                # cosParallaxStereo = cosParallaxStereo1 = cosParallaxStereo2
        q["cos_rays"] = float(cos_rays)
        if not (cos_rays < cs and cos_rays > 0 and float(cos_rays) < 0.9998):
            return CODE["low_parallax"], None                      # (bStereo1 / bStereo2 are false: :576 and :580 cannot hold)
        A = np.zeros((4, 4), F32)
        for b in range(4):
            r1 = (T1[b], T1[3 + b], T1[6 + b]) if b < 3 else (T1[9], T1[10], T1[11])
            r2 = (T2[b], T2[3 + b], T2[6 + b]) if b < 3 else (T2[9], T2[10], T2[11])
            A[0, b] = F32(F32(xn1[0] * r1[2]) - r1[0])
            A[1, b] = F32(F32(xn1[1] * r1[2]) - r1[1])
            A[2, b] = F32(F32(xn2[0] * r2[2]) - r2[0])
            A[3, b] = F32(F32(xn2[1] * r2[2]) - r2[1])
        vh = svd_last_vt4(A)
        if vh[3] == 0:
            return CODE["w_zero"], None
        inv = F32(1.0 / float(vh[3]))
        x3 = [F32(F32(vh[r] * inv) + F32(0)) for r in range(3)]
        q["x3d"] = [float(v) for v in x3]
        z1 = F32(_dotd(T1[6:9], x3) + float(T1[11]))
        q["z1"] = float(z1)
        if z1 <= 0:
            return CODE["z1"], None
        z2 = F32(_dotd(T2[6:9], x3) + float(T2[11]))
        q["z2"] = float(z2)
        if z2 <= 0:
            return CODE["z2"], None
        for tag, S, T, cam, z in (("1", S1, T1, cam1, z1), ("2", S2, T2, cam2, z2)):
            x = F32(_dotd(T[0:3], x3) + float(T[9]))
            y = F32(_dotd(T[3:6], x3) + float(T[10]))
            uv = po.kb8_project(cam, np.array([x, y, z], F32))     # pCamera->project(cv::Point3f(x, y, z))
            ex, ey = F32(uv[0] - S["x"]), F32(uv[1] - S["y"])
            e2 = F32(F32(ex * ex) + F32(ey * ey))
            sig = float(SIGMA32[S["octave"]])
            q["e" + tag] = math.sqrt(float(e2))
            q["gate_ulps" + tag] = abs(float(e2) - 5.991 * sig) / float(np.spacing(F32(5.991 * sig)))
            if float(e2) > gate * sig:
                return CODE["reproj%s_mono" % tag], None
        d1 = [F32(x3[r] - T1[12 + r]) for r in range(3)]
        d2 = [F32(x3[r] - T2[12 + r]) for r in range(3)]
        dist1, dist2 = F32(_normd(d1)), F32(_normd(d2))
        q.update(dist1=float(dist1), dist2=float(dist2))
        if dist1 == 0 or dist2 == 0:
            return CODE["dist_zero"], None
        if far and (dist1 >= th_far or dist2 >= th_far):
            return CODE["far"], None
        ratio_dist = F32(dist2 / dist1)
        ratio_octave = F32(SCALE32[S1["octave"]] / SCALE32[S2["octave"]])
        q["ratio"] = float(ratio_dist)
        if F32(ratio_dist * ratio_factor) < ratio_octave:
            return CODE["ratio_low"], None
        if ratio_dist > F32(ratio_octave * ratio_factor):
            return CODE["ratio_high"], None
        return CREATED, np.array(x3, F32)


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def _empty(nkf, n1):
    return (np.full((nkf, n1), -1, np.int32), np.zeros(nkf, np.int32), np.full((nkf, n1), NOT_MATCHED, np.int32),
            np.zeros((nkf, n1, 3), F32), np.zeros(nkf, np.int32))


def create_new_map_points(po, kf1, nbrs, coarse=False, far=False, th_far=0.0, ratio_factor=RATIO_FACTOR, exits=None, rules=(),
                          order=None, stop_before=None):
    """The reference's loop.  -> (matches12[nkf, n1], nmatches[nkf], status[nkf, n1], x3d[nkf, n1, 3], nnew[nkf]).  order (a list)
    takes (k, idx1, idx2, x3D) per created map point in the order of :670-683; stop_before: CheckNewKeyFrames() answers true before
    that neighbour (:389).  The label of an unmatched feature (taken earlier / not matched) is what the search on the state at
    entry says, which the loop itself never asks: it is computed for the comparison only."""
    ex = exits if exits is not None else Counter()
    n1, nkf = len(kf1.t.node), len(nbrs)
    G = gates(kf1, nbrs)
    matches, nmatches, status, x3d, nnew = _empty(nkf, n1)
    has1 = kf1.t.has_mp.copy()
    for k, nb in enumerate(nbrs):
        if stop_before is not None and k > 0 and k >= stop_before:
            break
        m, n = search_scalar(kf1.t._replace(has_mp=has1), search_nb(nb), False, coarse, False, gate=G[k])
        m0, _ = search_closed(kf1.t, search_nb(nb), False, coarse, False, gate=G[k])          # (the label only)
        matches[k], nmatches[k] = m, n
        for i in range(n1):
            if m[i] < 0:
                if m0[i] >= 0 and has1[i] and not kf1.t.has_mp[i]:
                    status[k, i] = TAKEN_EARLIER
                    ex["taken_earlier"] += 1
                else:
                    ex["not_matched"] += 1
                continue
            st, x = pair_kb8(po, side(kf1, i), side(nb.kf, int(m[i])), far, th_far, ratio_factor, rules)
            status[k, i] = st
            ex[STATUS[st]] += 1
            if st == CREATED:
                x3d[k, i] = x
                nnew[k] += 1
                has1[i] = 1                    # AddMapPoint :675; pKF2's own flag (:676) is read by no later search of this call
                if order is not None:
                    order.append((k, i, int(m[i]), x))
    return matches, nmatches, status, x3d, nnew


def closed_form(po, kf1, nbrs, coarse=False, far=False, th_far=0.0, ratio_factor=RATIO_FACTOR, rules=()):
    """Every (neighbour, feature) pair on the map-point state at entry, then per feature the first accepted neighbour keeps it."""
    n1, nkf = len(kf1.t.node), len(nbrs)
    G = gates(kf1, nbrs)
    matches, nmatches, status, x3d, nnew = _empty(nkf, n1)
    for k, nb in enumerate(nbrs):
        matches[k], _ = search_closed(kf1.t, search_nb(nb), False, coarse, False, gate=G[k])
        for i in np.nonzero(matches[k] >= 0)[0]:
            st, x = pair_kb8(po, side(kf1, i), side(nb.kf, int(matches[k, i])), far, th_far, ratio_factor, rules)
            status[k, i] = st
            if st == CREATED:
                x3d[k, i] = x
    for i in range(n1):
        taken = False
        for k in range(nkf):
            if matches[k, i] < 0:
                continue
            if taken:
                matches[k, i], status[k, i], x3d[k, i] = -1, TAKEN_EARLIER, 0
            elif status[k, i] == CREATED:
                taken = True
    nmatches[:] = (matches >= 0).sum(1)
    nnew[:] = (status == CREATED).sum(1)
    return matches, nmatches, status, x3d, nnew


# ---- constructed calls ------------------------------------------------------------------------------------------------------
def _one(x, y, octave, right, pose):
    t = make_table([(F32(x), F32(y), octave, 0.0, np.arange(32, dtype=np.uint8), 0, 0)], 0 if right else 1)
    return KF(t, pose)


def _raw_pose30(R, t):
    """Both sides from a float32 Rcw / tcw as pose30 makes them."""
    return pose30(Pose(np.asarray(R, F32), np.asarray(t, F32)))


def w_zero_scene():
    """:565.  Both keypoints on their principal points (KannalaBrandt8::unproject gives (0, 0, 1) exactly), the second camera
    turned about y, the two displaced along y by +-0.25: the fourth column of A is (0, 0.25, 0, -0.25) and the rows 1 and 3 of
    the other columns stay equal under every Jacobi rotation (the same operations on the same numbers), so every product with the
    fourth column is exactly 0, it is never rotated into the others, and the right singular vector of the smallest singular value
    (|sin| of the turn, below 0.25 sqrt 2) keeps its fourth component exactly 0.  Left rows on both sides; bCoarse (the search's
    own gate has no exit for w == 0)."""
    c, s = math.cos(0.3), math.sin(0.3)
    p1 = _raw_pose30(np.eye(3), (0, -0.25, 0))
    p2 = _raw_pose30([[c, 0, s], [0, 1, 0], [-s, 0, c]], (0, 0.25, 0))
    cam = CAMS[0]
    kf1 = _one(F32(cam[2]), F32(cam[3]), 0, 0, p1)
    kf2 = _one(F32(cam[2]), F32(cam[3]), 0, 0, p2)
    return kf1, [NB(kf2, np.zeros((4, 12), F32) + np.tile(np.concatenate([np.eye(3).reshape(9), [0, 0, 0]]), (4, 1)).astype(F32),
                    (1e6, 1e6))]


def gate_599_scene(po):
    """A pair whose first chi-square lies between 5.99 and 5.991 sigma2 (octave 7): kp1 moved along x until it does."""
    pa, pb = pose_from(0.0, 0.0, 0.0, (0, 0, 0)), pose_from(0.0, 0.02, 0.0, (0.4, 0.0, 0.0))
    P1, P2 = pose30(pa), pose30(pb)
    X = np.array([0.3, -0.2, 2.0])
    uv1 = hg.kb8_project64(CAMS[0], (_world_to_cam(P1[0]) @ np.append(X, 1))[:3])
    uv2 = hg.kb8_project64(CAMS[0], (_world_to_cam(P2[0]) @ np.append(X, 1))[:3])
    sig = float(SIGMA32[7])

    def build(d):
        return _one(uv1[0], uv1[1] + d, 7, 0, P1), _one(uv2[0], uv2[1], 7, 0, P2)

    def chi(d):
        a, b = build(d)
        q = {}
        pair_kb8(po, side(a, 0), side(b, 0), q=q)
        return q["e1"] ** 2 / sig
    lo, hi = 0.0, 40.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if chi(mid) < 5.9905:
            lo = mid
        else:
            hi = mid
    a, b = build(lo)
    assert 5.99 < chi(lo) < 5.991, chi(lo)
    return a, [NB(b, relative_poses(pa, pb), (1e6, 1e6))]


def dist_zero_scene(kf1, nbrs, out):
    """:657, the second pass: the side of a neighbour that created a point gets that point as its stored Ow, which only the
    distances read.  -> (nbrs with that pose changed, (k, i))."""
    matches, _, status, x3d, _ = out
    k, i = [int(v[0]) for v in np.nonzero(status == CREATED)]
    nb = nbrs[k]
    pose = nb.kf.pose.copy()
    pose[int(matches[k, i] >= nb.kf.t.nleft), 12:] = x3d[k, i]
    changed = list(nbrs)
    changed[k] = nb._replace(kf=nb.kf._replace(pose=pose))
    return changed, (k, i)


# ---- the independent float64 statement ------------------------------------------------------------------------------------
def pair_f64(S1, S2, far=False, th_far=0.0, ratio_factor=RATIO_FACTOR):
    """-> (status name, x3D or None, margins {kind: the smallest distance of a compared quantity from its threshold}, q).  Kinds:
    "cos", "z" (metres, relative beyond 1 m), "px" (chi-square gates, as square roots in pixels), "dist" (the far gate, like "z"),
    "ratio" (relative)."""
    th_far, rf = float(th_far), float(ratio_factor)
    S = (S1, S2)
    cams = [CAMS[s["right"]] for s in S]
    T = [_world_to_cam(s["pose2"][s["right"]]) for s in S]
    Tinv = [np.linalg.inv(t) for t in T]
    xn = [hg.kb8_unproject64(cams[a], S[a]["x"], S[a]["y"]) for a in range(2)]
    xn = [v / v[2] for v in xn]
    rays = [Tinv[a][:3, :3] @ xn[a] for a in range(2)]
    cos_rays = float(rays[0] @ rays[1] / (np.linalg.norm(rays[0]) * np.linalg.norm(rays[1])))
    margins, q = {}, {"cos_rays": cos_rays}

    def gate(kind, a, b):
        unit = max(1.0, abs(a)) if kind in ("z", "dist") else 1.0
        margins[kind] = min(margins.get(kind, math.inf), abs(a - b) / unit)
        return a - b

    if not (gate("cos", cos_rays, 0.0) > 0 and gate("cos", cos_rays, 0.9998) < 0):
        return "low_parallax", None, margins, q
    A = np.stack([xn[0][0] * T[0][2] - T[0][0], xn[0][1] * T[0][2] - T[0][1], xn[1][0] * T[1][2] - T[1][0],
                  xn[1][1] * T[1][2] - T[1][1]])
    v = np.linalg.svd(A)[2][-1]
    if v[3] == 0:
        return "w_zero", None, margins, q
    X = v[:3] / v[3]
    q["x3d"] = [float(c) for c in X]
    Xc = [(T[a] @ np.append(X, 1.0))[:3] for a in range(2)]
    for a in range(2):
        q["z%d" % (a + 1)] = float(Xc[a][2])
        if not gate("z", float(Xc[a][2]), 0.0) > 0:
            return "z%d" % (a + 1), None, margins, q
    for a in range(2):
        uv = hg.kb8_project64(cams[a], Xc[a])
        e = math.hypot(uv[0] - float(S[a]["x"]), uv[1] - float(S[a]["y"]))
        q["e%d" % (a + 1)] = e
        if gate("px", e, math.sqrt(5.991 * float(SIGMA2[S[a]["octave"]]))) > 0:
            return "reproj%d_mono" % (a + 1), None, margins, q
    dist = [float(np.linalg.norm(X - Tinv[a][:3, 3])) for a in range(2)]
    q.update(dist1=dist[0], dist2=dist[1])
    if dist[0] == 0 or dist[1] == 0:
        return "dist_zero", None, margins, q
    if far and (gate("dist", dist[0], th_far) >= 0 or gate("dist", dist[1], th_far) >= 0):
        return "far", None, margins, q
    ratio = dist[1] / dist[0]
    ro = 1.2 ** (S1["octave"] - S2["octave"])
    q["ratio"] = ratio
    if gate("ratio", ratio * rf / ro, 1.0) < 0:
        return "ratio_low", None, margins, q
    if gate("ratio", ratio / (ro * rf), 1.0) > 0:
        return "ratio_high", None, margins, q
    return "created", X, margins, q
