"""LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684, keyframes of one pinhole camera), restated for
the tests of pli_create_new_map_points: CPU only, plain numpy.

  * constructed_scenes     the two exits no random scene reaches (w == 0, dist == 0), each as a whole call of one pair;
  * scene                  a keyframe and its neighbours on tests/test_triangulation_search_cpu.py two_view_case, with mvuRight /
                           mvDepth / mvKeys consistent with the geometry for the stereo rows and some deliberately wrong depths;
  * new_map_point_pair     :530-667 for one matched pair, scalar float32 in the reference's operation order with OpenCV's cv::Mat
                           conventions (a gemm row: double accumulation, one rounding; Mat::dot and cv::norm: sequential double;
                           s*row - row: the rounded product, then a float subtraction; Mat / s: times (float)(1/s); 1.0/z: the
                           double reciprocal rounded once; comparisons against 5.991*sigma2, 7.8*sigma2, 0.9998 in double; a libm
                           call on a float: in double, rounded).  Its SVD is the oracle's jacobiSvdLastVt4, through
                           tests/cpp/new_map_points_svd_shim.cpp and ctypes: the Jacobi is not stated a second time;
  * create_new_map_points  the reference's loop: for each neighbour in order SearchForTriangulation on the CURRENT map-point state,
                           :530-667 per pair, has_mp set on success; every exit counted;
  * closed_form            all pairs on the state at entry, then first-accepted-wins per feature: what the device does;
  * pair_f64               an independent float64 statement in the manner of helpers_geometry.py: 4x4 homogeneous poses, every
                           inverse np.linalg.inv of one (no transposes written out, the stored Ow is not read), np.linalg.svd, the
                           stereo parallax as (d^2 - h^2) / (d^2 + h^2) instead of cos(2 atan2(h, d)).  It reports the margin of
                           every comparison it makes, by kind, so that a test can tell decided pairs from undecided ones.

Recorded, float32 restatement against pair_f64 on SEEDS, over the pairs whose float64 margins exceed these very figures (7250 of
7269; tests/test_new_map_points_cpu.py measures them again on every run, prints them and fails when a run measures more): cosines
1.48e-7 (MEASURED["cos"] = 2e-7), chi-square roots 1.62e-3 px (2e-3), depths 1.21e-4 relative beyond 1 m (1.5e-4), distances
4.7e-6 (6e-6), the distance ratio 6.0e-7 (1e-6), x3d 4.2e-6 relative to its norm (5e-6).  SEEDS are chosen so that no pair lies
within 2 float ulps of the stereo-parallax comparison, the only gate that depends on a libm (the nearest: 14 ulps).
"""
import atexit
import copy
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile
from collections import Counter, namedtuple

import numpy as np

from test_triangulation_search_cpu import (K_EUROC, SCALE, SIGMA2, make_table, search_for_triangulation,
                                           search_for_triangulation_fast, two_view_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

STATUS = ("created", "low_parallax", "w_zero", "empty_unproject", "z1", "z2", "reproj1_mono", "reproj1_stereo", "reproj2_mono",
          "reproj2_stereo", "dist_zero", "far", "ratio_low", "ratio_high", "taken_earlier", "not_matched")
CODE = {name: i for i, name in enumerate(STATUS)}
CREATED, TAKEN_EARLIER, NOT_MATCHED = CODE["created"], CODE["taken_earlier"], CODE["not_matched"]

# fx, fy, cx, cy, bf (EuRoC: bf = 47.90639384423901), mb = mbf / fx in float (Frame.cc:197), 1.5f * mfScaleFactor (:384)
CAM = tuple(F32(v) for v in K_EUROC) + (F32(47.90639384423901),)
MB = F32(CAM[4] / CAM[0])
RATIO_FACTOR = F32(F32(1.5) * F32(1.2))

# one keyframe: its search table (mvKeysUn, descriptors, nodes, has_mp, stereo = mvuRight >= 0), mvuRight, mvDepth, mvKeys[i].pt
# (n x 2), pose = Rcw row major, tcw, the stored Ow; one neighbour: its keyframe, F12, the epipole, truth[idx1]
KF = namedtuple("KF", "t uright depth key pose")
NB = namedtuple("NB", "kf F12 ep truth")

# ---- measured on the CPU over SEEDS (float32 restatement against pair_f64), rounded up ----
MEASURED = {"cos": 2e-7, "px": 2e-3, "z": 1.5e-4, "dist": 6e-6, "ratio": 1e-6, "x3d_rel": 5e-6}
SEEDS = (11, 15, 21, 32)


# ---- the oracle's Jacobi --------------------------------------------------------------------------------------------------
_SVD = {}


def svd_last_vt4(A):
    """The last row of vt of cv::SVD::compute(A), A 4 x 4 float32: oracle/match_oracle.hpp jacobiSvdLastVt4."""
    if "fn" not in _SVD:
        d = tempfile.mkdtemp(prefix="pli_newpt_shim_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libnewpt_shim.so")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", ROOT,
                            os.path.join(ROOT, "tests", "cpp", "new_map_points_svd_shim.cpp"), "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        lib = C.CDLL(so)
        lib.pli_test_svd_last_vt4.restype = None
        lib.pli_test_svd_last_vt4.argtypes = [C.c_void_p, C.c_void_p]
        _SVD["fn"] = lib.pli_test_svd_last_vt4
    a = np.ascontiguousarray(A, np.float32).reshape(16)
    out = np.zeros(4, np.float32)
    _SVD["fn"](a.ctypes.data, out.ctypes.data)
    return out


# ---- the scene --------------------------------------------------------------------------------------------------------------
def make_pose(R, t):
    """15 floats as KeyFrame::SetPose leaves them: Rcw, tcw (float), Ow = -Rcw.t()*tcw as a CV_32F gemm."""
    R = np.asarray(R, np.float32).reshape(3, 3)
    t = np.asarray(t, np.float32).reshape(3)
    Ow = [F32(-(float(R[0, r]) * float(t[0]) + float(R[1, r]) * float(t[1]) + float(R[2, r]) * float(t[2]))) for r in range(3)]
    return np.concatenate([R.reshape(9), t, np.array(Ow, np.float32)]).astype(np.float32)


def _aux(rng, t, R, tw, P, stereo, bad_depth, on_points=False):
    """mvuRight / mvDepth / mvKeys for a table: the depth of a row is that of the scene point that projects nearest to it."""
    fx, fy, cx, cy, bf = (float(v) for v in CAM)
    n = len(t.node)
    x, y = t.x.astype(np.float64), t.y.astype(np.float64)
    r2 = (x - cx) ** 2 + (y - cy) ** 2
    key = np.stack([x + (x - cx) * r2 * 2e-8, y + (y - cy) * r2 * 2e-8], 1).astype(np.float32)   # (a smooth distortion, < 1 px)
    ur, depth = np.full(n, -1, np.float32), np.full(n, -1, np.float32)
    if n and len(P):
        Xc = P @ np.asarray(R).T + np.asarray(tw)
        u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        d2 = (u[None, :] - x[:, None]) ** 2 + (v[None, :] - y[:, None]) ** 2
        # (every row of the keyframe shows a scene point, 0.2 px of noise: P is the scene two_view_case drew, or this fails)
        assert not on_points or math.sqrt(d2.min(axis=1).max()) < 2.0, math.sqrt(d2.min(axis=1).max())
        z = Xc[np.argmin(d2, axis=1), 2]
        flag = {"mixed": t.stereo != 0, "mono": np.zeros(n, bool), "stereo": np.ones(n, bool)}[stereo]
        for i in np.nonzero(flag)[0]:
            ur[i] = F32(float(key[i, 0]) - bf / z[i] + rng.normal(0, 0.3))
            r = rng.random()
            depth[i] = F32(z[i] * (1 + rng.normal(0, 0.002)) if r > bad_depth else
                           z[i] * (0.5 if r > 0.6 * bad_depth else 1.7) if r > 0.25 * bad_depth else -1e-3)
        depth[ur < 0] = -1
        ur[ur < 0] = -1
    return KF(t._replace(stereo=(ur >= 0).astype(np.uint8)), ur, depth, key, make_pose(R, tw))


def scene(seed, nkf, npts, nnodes=12, stereo="mixed", bad_depth=0.12, f12_zero=True):
    """-> (kf1: KF, nbrs: [NB]).  stereo: "mixed" (two_view_case's flags), "mono" or "stereo" for every row of every table."""
    rng = np.random.default_rng(seed)
    first = copy.deepcopy(rng)                 # two_view_case draws the scene points first: the same three draws
    P = np.stack([first.uniform(-4, 4, npts), first.uniform(-2.5, 2.5, npts), first.uniform(3, 12, npts)], 1)
    poses = []
    t1, out = two_view_case(rng, nkf, npts, nnodes, poses=poses)
    R1, tw1 = (poses[0][0], poses[0][1]) if poses else (np.eye(3), np.zeros(3))
    kf1 = _aux(rng, t1, R1, tw1, P, stereo, bad_depth, on_points=nkf > 0)
    nbrs = []
    for k, (t2, F12, ep, truth) in enumerate(out):
        if not f12_zero and k == 3:            # (two_view_case zeroes F12 of neighbour 3: den == 0 for every pair)
            F12 = out[2][1]
        nbrs.append(NB(_aux(rng, t2, poses[k][2], poses[k][3], P, stereo, bad_depth), F12, ep, truth))
    return kf1, nbrs


def constructed_scenes():
    """The two exits that need an exact float coincidence, which no random scene has, as whole calls: one feature against one
    feature with the same descriptor and node, a rectified F12 (rows are epipolar lines) and a far epipole, so that the pair
    passes the search.  -> [dict(name, kf1, nbrs, cam, mb)]; cam: fx, fy, cx, cy, bf.
      w_zero (:565)     fx = fy = 1, cx = cy = 0 (a keypoint is its own normalised ray); two cameras 0.5 apart along x that look the
                        same way, the keypoints on one column and 0.5 apart in y: the fourth column of A is orthogonal to the other
                        three (every number dyadic, every product exact), so the Jacobi never rotates it into them and the singular
                        vector of the smallest singular value keeps its fourth component exactly 0.
      dist_zero (:657)  x3D = UnprojectStereo(idx1) with a depth so small that Rwc*x3Dc + Ow rounds to the stored Ow; the stored Ow
                        is an input of its own and differs from -Rcw.t()*tcw here, so the point still lies in front of the camera
                        and on the keypoint."""
    desc = np.arange(32, dtype=np.uint8)

    def one(x, y, ur, depth, pose15):
        t = make_table([(x, y, 0, 0.0, desc, 0, 0, int(ur >= 0))])
        return KF(t, np.array([ur], np.float32), np.array([depth], np.float32), np.stack([t.x, t.y], 1), pose15)

    def rectified(cam):
        Kinv = np.linalg.inv(np.array([[float(cam[0]), 0, float(cam[2])], [0, float(cam[1]), float(cam[3])], [0, 0, 1.0]]))
        return (Kinv.T @ np.array([[0, 0, 0], [0, 0, 0.5], [0, -0.5, 0]]) @ Kinv).astype(np.float32)

    far_ep = np.array([1e9, 0.0], np.float32)
    unit = (F32(1), F32(1), F32(0), F32(0), F32(0))
    w = dict(name="w_zero", cam=unit, mb=MB, kf1=one(0.125, 0.25, -1.0, -1.0, make_pose(np.eye(3), (-0.25, 0, 0))),
             nbrs=[NB(one(0.125, -0.25, -1.0, -1.0, make_pose(np.eye(3), (0.25, 0, 0))), rectified(unit), far_ep, None)])
    cam = CAM[:4] + (F32(10.0),)
    cx, cy = float(cam[2]), float(cam[3])
    p1 = make_pose(np.eye(3), (0, 0, -0.25))
    p1[12:] = (0, 0, 0.5)
    d = dict(name="dist_zero", cam=cam, mb=MB, kf1=one(cx, cy, cx - 10.0 * 4.0, 1e-30, p1),
             nbrs=[NB(one(cx, cy, -1.0, -1.0, make_pose(np.eye(3), (0, 0, 0))), rectified(cam), far_ep, None)])
    return [w, d]


def side(kf, i):
    """What :530-667 read of feature i of a keyframe."""
    t = kf.t
    return dict(x=F32(t.x[i]), y=F32(t.y[i]), octave=int(t.octave[i]), ur=F32(kf.uright[i]), depth=F32(kf.depth[i]),
                key=(F32(kf.key[i, 0]), F32(kf.key[i, 1])), pose=kf.pose)


# ---- :530-667, scalar float32 ---------------------------------------------------------------------------------------------
def _dotd(a, b):
    return float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2])


def _normd(a):
    return math.sqrt(_dotd(a, a))


def _gemm_t(R9, r, v, c):
    """row r of Rcw.t() * v + c as a CV_32F gemm"""
    return F32(float(R9[r]) * float(v[0]) + float(R9[3 + r]) * float(v[1]) + float(R9[6 + r]) * float(v[2]) + float(c))


def _unproject_stereo(S, cam, rules):
    fx, fy, cx, cy, _ = cam
    invfx, invfy = F32(F32(1) / fx), F32(F32(1) / fy)
    u, v = (S["x"], S["y"]) if "unproject_un" in rules else S["key"]
    z = S["depth"]
    xc = (F32(F32(F32(u - cx) * z) * invfx), F32(F32(F32(v - cy) * z) * invfy), z)
    T = S["pose"]
    return [_gemm_t(T, r, xc, T[12 + r]) for r in range(3)]


def _reproject(S, stereo, cam, x3, z, q, tag, bf_of=None):
    fx, fy, cx, cy, bf = cam
    bf = bf if bf_of is None else F32(bf_of)
    T = S["pose"]
    x = F32(_dotd(T[0:3], x3) + float(T[9]))
    y = F32(_dotd(T[3:6], x3) + float(T[10]))
    invz = F32(1.0 / float(z))
    sig = float(SIGMA2[S["octave"]])
    if not stereo:
        u = F32(F32(F32(fx * x) / z) + cx)
        v = F32(F32(F32(fy * y) / z) + cy)
        ex, ey = F32(u - S["x"]), F32(v - S["y"])
        e2 = F32(F32(ex * ex) + F32(ey * ey))
        q["e" + tag] = math.sqrt(float(e2))
        return 1 if float(e2) > 5.991 * sig else 0
    u = F32(F32(F32(fx * x) * invz) + cx)
    ur = F32(u - F32(bf * invz))
    v = F32(F32(F32(fy * y) * invz) + cy)
    ex, ey, er = F32(u - S["x"]), F32(v - S["y"]), F32(ur - S["ur"])
    e2 = F32(F32(F32(ex * ex) + F32(ey * ey)) + F32(er * er))
    q["e" + tag] = math.sqrt(float(e2))
    return 2 if float(e2) > 7.8 * sig else 0


MUTANTS = ("stereo2_always", "unproject_un", "far_gt", "bf_neighbour", "last_wins")


def new_map_point_pair(S1, S2, cam=CAM, mb=MB, far=False, th_far=0.0, ratio_factor=RATIO_FACTOR, rules=(), q=None):
    """-> (status code, x3D as 3 float32 or None).  rules: deliberate misreadings for the hand cases and for the fixtures of the
    reference's own code (MUTANTS; tests/test_ref_pin_map.py): "stereo2_always": the second stereo parallax also when the first
    side is stereo, against `else if` :544; "unproject_un": mvKeysUn in UnprojectStereo; "far_gt": dist > mThFarPoints at :660;
    "bf_neighbour": pKF2's mbf (S2["bf"], where a case gives the neighbour another one) in the second keyframe's stereo gate,
    against mpCurrentKeyFrame->mbf :641; "last_wins" is closed_form's: the last accepted neighbour keeps a feature.
    q (a dict) takes the compared quantities."""
    q = q if q is not None else {}
    with np.errstate(all="ignore"):
        fx, fy, cx, cy, bf = cam
        mb, th_far, ratio_factor = F32(mb), F32(th_far), F32(ratio_factor)
        stereo1, stereo2 = bool(S1["ur"] >= 0), bool(S2["ur"] >= 0)
        T1, T2 = S1["pose"], S2["pose"]
        xn1 = (F32(F32(S1["x"] - cx) / fx), F32(F32(S1["y"] - cy) / fy), F32(1))
        xn2 = (F32(F32(S2["x"] - cx) / fx), F32(F32(S2["y"] - cy) / fy), F32(1))
        ray1 = [_gemm_t(T1, r, xn1, 0.0) for r in range(3)]
        ray2 = [_gemm_t(T2, r, xn2, 0.0) for r in range(3)]
        cos_rays = F32(_dotd(ray1, ray2) / (_normd(ray1) * _normd(ray2)))
        cs = F32(cos_rays + F32(1))
        cs1 = cs2 = cs
        par = lambda d: F32(math.cos(float(F32(F32(2) * F32(math.atan2(float(F32(mb / F32(2))), float(d)))))))
        if stereo1:
            cs1 = par(S1["depth"])
        if stereo2 and (not stereo1 or "stereo2_always" in rules):
            cs2 = par(S2["depth"])
        cs = cs2 if cs2 < cs1 else cs1
        q.update(cos_rays=float(cos_rays), cs1=float(cs1), cs2=float(cs2))
        if cos_rays < cs and cos_rays > 0 and (stereo1 or stereo2 or float(cos_rays) < 0.9998):
            A = np.zeros((4, 4), np.float32)
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
            q["branch"] = "svd"
        elif stereo1 and cs1 < cs2:
            if not S1["depth"] > 0:
                return CODE["empty_unproject"], None
            x3 = _unproject_stereo(S1, cam, rules)
            q["branch"] = "stereo1"
        elif stereo2 and cs2 < cs1:
            if not S2["depth"] > 0:
                return CODE["empty_unproject"], None
            x3 = _unproject_stereo(S2, cam, rules)
            q["branch"] = "stereo2"
        else:
            return CODE["low_parallax"], None
        q["x3d"] = [float(v) for v in x3]
        z1 = F32(_dotd(T1[6:9], x3) + float(T1[11]))
        q["z1"] = float(z1)
        if z1 <= 0:
            return CODE["z1"], None
        z2 = F32(_dotd(T2[6:9], x3) + float(T2[11]))
        q["z2"] = float(z2)
        if z2 <= 0:
            return CODE["z2"], None
        g = _reproject(S1, stereo1, cam, x3, z1, q, "1")
        if g:
            return CODE["reproj1_mono" if g == 1 else "reproj1_stereo"], None
        g = _reproject(S2, stereo2, cam, x3, z2, q, "2",          # (bf is mpCurrentKeyFrame's here too, :641)
                       bf_of=S2.get("bf") if "bf_neighbour" in rules else None)
        if g:
            return CODE["reproj2_mono" if g == 1 else "reproj2_stereo"], None
        d1 = [F32(x3[r] - T1[12 + r]) for r in range(3)]
        d2 = [F32(x3[r] - T2[12 + r]) for r in range(3)]
        dist1, dist2 = F32(_normd(d1)), F32(_normd(d2))
        q.update(dist1=float(dist1), dist2=float(dist2))
        if dist1 == 0 or dist2 == 0:
            return CODE["dist_zero"], None
        if far and ((dist1 > th_far or dist2 > th_far) if "far_gt" in rules else (dist1 >= th_far or dist2 >= th_far)):
            return CODE["far"], None
        ratio_dist = F32(dist2 / dist1)
        ratio_octave = F32(SCALE[S1["octave"]] / SCALE[S2["octave"]])
        q["ratio"] = float(ratio_dist)
        if F32(ratio_dist * ratio_factor) < ratio_octave:
            return CODE["ratio_low"], None
        if ratio_dist > F32(ratio_octave * ratio_factor):
            return CODE["ratio_high"], None
        return CREATED, np.array(x3, np.float32)


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def _empty(nkf, n1):
    return (np.full((nkf, n1), -1, np.int32), np.zeros(nkf, np.int32), np.full((nkf, n1), NOT_MATCHED, np.int32),
            np.zeros((nkf, n1, 3), np.float32), np.zeros(nkf, np.int32))


def _side2(nb, j, bf2):
    S = side(nb.kf, j)
    if bf2 is not None:
        S["bf"] = bf2
    return S


def create_new_map_points(kf1, nbrs, cam=CAM, mb=MB, ratio_factor=RATIO_FACTOR, coarse=False, far=False, th_far=0.0, exits=None,
                          scalar_search=False, order=None, stop_before=None, mut=(), bf2=None):
    """The reference's loop.  -> (matches12[nkf, n1], nmatches[nkf], status[nkf, n1], x3d[nkf, n1, 3], nnew[nkf]).
    order (a list) takes (k, idx1, idx2, x3D) per created map point, in the order of :670-683; stop_before: CheckNewKeyFrames()
    answers true before that neighbour (:389); mut: MUTANTS, passed to every pair; bf2: pKF2->mbf per neighbour where it is not the
    current keyframe's (read by the mutant "bf_neighbour" alone).  The label of an unmatched feature (taken earlier / not matched) is what the search
    on the state at entry says, which the loop itself never asks: it is computed for the comparison only."""
    ex = exits if exits is not None else Counter()
    search = search_for_triangulation if scalar_search else search_for_triangulation_fast
    n1, nkf = len(kf1.t.node), len(nbrs)
    matches, nmatches, status, x3d, nnew = _empty(nkf, n1)
    has1 = kf1.t.has_mp.copy()
    for k, nb in enumerate(nbrs):
        if stop_before is not None and k > 0 and k >= stop_before:
            break
        has2 = nb.kf.t.has_mp.copy()
        m, n = search(kf1.t._replace(has_mp=has1), nb.kf.t, nb.F12, nb.ep, False, coarse, False)
        m0, _ = search(kf1.t, nb.kf.t, nb.F12, nb.ep, False, coarse, False)        # (the label only)
        matches[k], nmatches[k] = m, n
        for i in range(n1):
            if m[i] < 0:
                if m0[i] >= 0 and has1[i] and not kf1.t.has_mp[i]:
                    status[k, i] = TAKEN_EARLIER
                    ex["taken_earlier"] += 1
                else:
                    ex["not_matched"] += 1
                continue
            st, x = new_map_point_pair(side(kf1, i), _side2(nb, int(m[i]), None if bf2 is None else bf2[k]), cam, mb, far, th_far,
                                       ratio_factor, rules=mut)
            status[k, i] = st
            ex[STATUS[st]] += 1
            if st == CREATED:
                x3d[k, i] = x
                nnew[k] += 1
                has1[i] = has2[m[i]] = 1
                if order is not None:
                    order.append((k, i, int(m[i]), x))
    return matches, nmatches, status, x3d, nnew


def closed_form(kf1, nbrs, cam=CAM, mb=MB, ratio_factor=RATIO_FACTOR, coarse=False, far=False, th_far=0.0, mut=(), bf2=None):
    """Every (neighbour, feature) pair on the map-point state at entry, then per feature the first accepted neighbour keeps it
    (mut "last_wins": the last one; the other MUTANTS go to every pair)."""
    n1, nkf = len(kf1.t.node), len(nbrs)
    matches, nmatches, status, x3d, nnew = _empty(nkf, n1)
    for k, nb in enumerate(nbrs):
        matches[k], _ = search_for_triangulation_fast(kf1.t, nb.kf.t, nb.F12, nb.ep, False, coarse, False)
        for i in np.nonzero(matches[k] >= 0)[0]:
            st, x = new_map_point_pair(side(kf1, i), _side2(nb, int(matches[k, i]), None if bf2 is None else bf2[k]), cam, mb, far,
                                       th_far, ratio_factor, rules=mut)
            status[k, i] = st
            if st == CREATED:
                x3d[k, i] = x
    for i in range(n1):
        taken = False
        for k in (range(nkf - 1, -1, -1) if "last_wins" in mut else range(nkf)):
            if matches[k, i] < 0:
                continue
            if taken:
                matches[k, i], status[k, i], x3d[k, i] = -1, TAKEN_EARLIER, 0
            elif status[k, i] == CREATED:
                taken = True
    nmatches[:] = (matches >= 0).sum(1)
    nnew[:] = (status == CREATED).sum(1)
    return matches, nmatches, status, x3d, nnew


# ---- the independent float64 statement ------------------------------------------------------------------------------------
def _hom(pose):
    T = np.eye(4)
    T[:3, :3] = np.asarray(pose[:9], np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(pose[9:12], np.float64)
    return T


def pair_f64(S1, S2, cam=CAM, mb=MB, far=False, th_far=0.0, ratio_factor=RATIO_FACTOR):
    """-> (status name, x3D or None, margins: {kind: the smallest distance of a compared quantity from its threshold}, q: the
    compared quantities).  Kinds: "cos" (parallax comparisons), "z" (depths, metres, relative beyond 1 m), "px" (chi-square
    gates, as sqrt in pixels), "dist" (the far gate, like "z"), "ratio" (scale consistency, relative)."""
    fx, fy, cx, cy, bf = (float(v) for v in cam)
    mb, th_far, rf = float(mb), float(th_far), float(ratio_factor)
    Kinv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    T = [_hom(S1["pose"]), _hom(S2["pose"])]
    Tinv = [np.linalg.inv(t) for t in T]
    S = (S1, S2)
    st = [float(s["ur"]) >= 0 for s in S]
    xn = [Kinv @ np.array([float(s["x"]), float(s["y"]), 1.0]) for s in S]
    rays = [Tinv[a][:3, :3] @ xn[a] for a in range(2)]
    cos_rays = float(rays[0] @ rays[1] / (np.linalg.norm(rays[0]) * np.linalg.norm(rays[1])))
    margins, q = {}, {"cos_rays": cos_rays}

    def gate(kind, a, b):
        unit = max(1.0, abs(a)) if kind in ("z", "dist") else 1.0          # (depths and distances: relative beyond 1 m)
        margins[kind] = min(margins.get(kind, math.inf), abs(a - b) / unit)
        return a - b

    def par(d):
        d2, h2 = float(d) ** 2, (mb / 2) ** 2
        return (d2 - h2) / (d2 + h2)

    cs1 = cs2 = cos_rays + 1
    if st[0]:
        cs1 = par(S1["depth"])
    elif st[1]:
        cs2 = par(S2["depth"])
    cs = min(cs1, cs2)
    q.update(cs1=cs1, cs2=cs2)
    tri = gate("cos", cos_rays, cs) < 0 and gate("cos", cos_rays, 0.0) > 0 and (st[0] or st[1] or gate("cos", cos_rays, 0.9998) < 0)
    if tri:
        A = np.stack([xn[0][0] * T[0][2] - T[0][0], xn[0][1] * T[0][2] - T[0][1], xn[1][0] * T[1][2] - T[1][0],
                      xn[1][1] * T[1][2] - T[1][1]])
        v = np.linalg.svd(A)[2][-1]
        if v[3] == 0:
            return "w_zero", None, margins, q
        X = v[:3] / v[3]
    else:
        which = 0 if st[0] and gate("cos", cs1, cs2) < 0 else 1 if st[1] and gate("cos", cs2, cs1) < 0 else None
        if which is None:
            return "low_parallax", None, margins, q
        z = float(S[which]["depth"])
        if not gate("z", z, 0.0) > 0:
            return "empty_unproject", None, margins, q
        kn = Kinv @ np.array([float(S[which]["key"][0]), float(S[which]["key"][1]), 1.0])
        X = (Tinv[which] @ np.array([kn[0] * z, kn[1] * z, z, 1.0]))[:3]
    q["x3d"] = [float(c) for c in X]
    Xc = [(T[a] @ np.append(X, 1.0))[:3] for a in range(2)]
    for a in range(2):
        q["z%d" % (a + 1)] = float(Xc[a][2])
        if not gate("z", float(Xc[a][2]), 0.0) > 0:
            return "z%d" % (a + 1), None, margins, q
    for a in range(2):
        u, v = fx * Xc[a][0] / Xc[a][2] + cx, fy * Xc[a][1] / Xc[a][2] + cy
        e2 = (u - float(S[a]["x"])) ** 2 + (v - float(S[a]["y"])) ** 2
        thr = 5.991
        if st[a]:
            e2 += (u - bf / Xc[a][2] - float(S[a]["ur"])) ** 2
            thr = 7.8
        q["e%d" % (a + 1)] = math.sqrt(e2)
        if gate("px", math.sqrt(e2), math.sqrt(thr * float(SIGMA2[S[a]["octave"]]))) > 0:
            return "reproj%d_%s" % (a + 1, "stereo" if st[a] else "mono"), None, margins, q
    dist = [float(np.linalg.norm(X - Tinv[a][:3, 3])) for a in range(2)]
    q.update(dist1=dist[0], dist2=dist[1])
    if dist[0] == 0 or dist[1] == 0:
        return "dist_zero", None, margins, q
    if far and (gate("dist", dist[0], th_far) >= 0 or gate("dist", dist[1], th_far) >= 0):
        return "far", None, margins, q
    ratio = dist[1] / dist[0]
    ro = float(SCALE[S1["octave"]]) / float(SCALE[S2["octave"]])
    q["ratio"] = ratio
    if gate("ratio", ratio * rf / ro, 1.0) < 0:
        return "ratio_low", None, margins, q
    if gate("ratio", ratio / (ro * rf), 1.0) > 0:
        return "ratio_high", None, margins, q
    return "created", X, margins, q
