"""LocalMapping::CreateNewMapPoints from the search on (LocalMapping.cc:423-684, keyframes of one pinhole camera), without a
device: the scalar float32 restatement of the reference's sequential loop (tests/helpers_new_map_points.py), which is the checker
of pli_create_new_map_points (tests/test_new_map_points_gpu.py, tests/test_cpp_new_map_points.py), against the closed form the
device relies on, hand-worked cases for every quirk and boundary, an independent float64 statement, and the C ABI.

The generator's corpus is the seeded random scenes (H.SEEDS) and the two constructed scenes of H.constructed_scenes(): w == 0
(:565) and dist == 0 (:657) need exact float coincidences (a null vector whose last component is exactly zero; a point that is
exactly the camera centre), which no random scene has, so the generator constructs them, as whole calls that pass the search.
On that corpus the restatement takes every exit, and tests/test_new_map_points_gpu.py runs the same corpus on the device."""
import ctypes as C
import math
import os
import re
import subprocess
from collections import Counter

import numpy as np

import helpers_new_map_points as H
from helpers_new_map_points import CODE, F32, STATUS
from pli_slam_amd import capi
from pli_slam_amd.frontend import Frontend
from test_triangulation_search_cpu import SIGMA2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((False, False), (True, True))                      # (bCoarse, mbFarPoints)
TH_FAR = 9.0
_scenes = {}


def scenes():
    """The seeded scenes and the restatement's results on them, computed once and shared."""
    if not _scenes:
        for seed in H.SEEDS:
            kf1, nbrs = H.scene(seed, 6, 300)
            for coarse, far in SETTINGS:
                ex = Counter()
                res = H.create_new_map_points(kf1, nbrs, coarse=coarse, far=far, th_far=TH_FAR, exits=ex,
                                              scalar_search=(seed == H.SEEDS[0]))
                _scenes[(seed, coarse, far)] = (kf1, nbrs, res, ex)
    return _scenes


def test_the_generators_corpus_takes_every_exit():
    total = Counter()
    for (seed, coarse, far), (kf1, nbrs, res, ex) in scenes().items():
        total.update(ex)
        m, n, s, x, nn = res
        assert (nn > 0).sum() >= 3, (seed, coarse, far, nn)           # map points are created in at least three neighbours
        # a feature matched in two neighbours on the state at entry and accepted in the first: the coupling of the loop
        assert ((s == H.TAKEN_EARLIER).any(0) & (s == H.CREATED).any(0)).sum() > 0
        assert n.tolist() == (m >= 0).sum(1).tolist() and nn.tolist() == (s == H.CREATED).sum(1).tolist()
    assert [name for name in STATUS if total[name] == 0] == ["w_zero", "dist_zero"]      # (what no random scene reaches ...)
    for c in H.constructed_scenes():                                                     # (... the generator constructs)
        ex = Counter()
        m, n, s, x, nn = H.create_new_map_points(c["kf1"], c["nbrs"], cam=c["cam"], mb=c["mb"], exits=ex, scalar_search=True)
        assert n.tolist() == [1] and ex == Counter({c["name"]: 1}), (c["name"], n, ex)
        total.update(ex)
    print("exits over the generator's corpus:", dict(total))
    assert [name for name in STATUS if total[name] == 0] == []


def test_the_closed_form_equals_the_sequential_loop():
    """All pairs on the state at entry, then first-accepted-wins per feature: what the device computes."""
    for (seed, coarse, far), (kf1, nbrs, res, _) in scenes().items():
        got = H.closed_form(kf1, nbrs, coarse=coarse, far=far, th_far=TH_FAR)
        for a, b, what in zip(got, res, ("matches12", "nmatches", "status", "x3d", "nnew")):
            assert np.array_equal(a, b), (seed, coarse, far, what)


def test_an_early_return_is_a_prefix():
    kf1, nbrs, res, _ = scenes()[(H.SEEDS[1], False, False)]
    cut = H.create_new_map_points(kf1, nbrs, stop_before=2)
    for a, b in zip(cut, res):
        assert np.array_equal(a[:2], b[:2])
    assert (cut[0][2:] == -1).all() and (cut[2][2:] == H.NOT_MATCHED).all() and not cut[1][2:].any() and not cut[4][2:].any()
    assert res[4][2:].sum() > 0


# ---- hand cases -------------------------------------------------------------------------------------------------------------
I3 = (1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)


def pose(t, Ow=None, R=I3):
    p = H.make_pose(np.array(R, np.float32).reshape(3, 3), np.array(t, np.float32))
    if Ow is not None:
        p[12:] = np.array(Ow, np.float32)
    return p


def S(x, y, pose_, octave=0, ur=-1.0, depth=-1.0, key=None):
    return dict(x=F32(x), y=F32(y), octave=octave, ur=F32(ur), depth=F32(depth), pose=pose_,
                key=(F32(x), F32(y)) if key is None else (F32(key[0]), F32(key[1])))


def project(cam, p15, X):
    fx, fy, cx, cy, bf = (float(v) for v in cam)
    Xc = np.asarray(p15[:9], np.float64).reshape(3, 3) @ np.asarray(X, np.float64) + np.asarray(p15[9:12], np.float64)
    return fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy, Xc[2]


def seen(cam, p15, X, stereo=False, **kw):
    u, v, z = project(cam, p15, X)
    return S(u, v, p15, ur=u - float(cam[4]) / z if stereo else -1.0, depth=z if stereo else -1.0, **kw)


P1, P2 = pose((0, 0, 0)), pose((-0.3, 0, 0))                 # the second camera 0.3 m to the right


def test_the_second_stereo_parallax_is_computed_only_when_the_first_side_is_not_stereo():
    """`else if(bStereo2)` at :544.  Both sides stereo, the second with a wrong, very small depth: read literally its parallax is
    never computed and the pair is triangulated; computing it too would send the pair to UnprojectStereo of the second keyframe."""
    X = (0.5, 0.2, 6.0)
    s1, s2 = seen(H.CAM, P1, X, True), seen(H.CAM, P2, X, True)
    s2["depth"] = F32(0.2)
    q, q2 = {}, {}
    st, x = H.new_map_point_pair(s1, s2, q=q)
    st2, _ = H.new_map_point_pair(s1, s2, rules=("stereo2_always",), q=q2)
    assert st == H.CREATED and q["branch"] == "svd" and q["cs2"] == q["cos_rays"] + 1
    assert np.abs(x - np.array(X)).max() < 1e-2
    assert q2["branch"] == "stereo2" and st2 != H.CREATED
    # the first side mono: now the second side's parallax IS computed, and decides
    s1m = seen(H.CAM, P1, X)
    q3 = {}
    H.new_map_point_pair(s1m, s2, q=q3)
    assert q3["branch"] == "stereo2"


def test_the_second_stereo_gate_reads_the_current_keyframes_mbf():
    """:641: u2_r = u2 - mpCurrentKeyFrame->mbf*invz2.  One camera serves the call, so this is cam.bf: the pair stands with the bf
    its mvuRight was made with and falls at the second stereo gate with another."""
    X = (0.5, 0.2, 6.0)
    s1, s2 = seen(H.CAM, P1, X), seen(H.CAM, P2, X, True)
    assert H.new_map_point_pair(s1, s2)[0] == H.CREATED
    other = H.CAM[:4] + (F32(H.CAM[4] * 2),)
    assert H.new_map_point_pair(s1, s2, cam=other)[0] == CODE["reproj2_stereo"]
    s1s = seen(H.CAM, P1, X, True)
    assert H.new_map_point_pair(s1s, seen(H.CAM, P2, X), cam=other)[0] == CODE["reproj1_stereo"]


def test_unproject_stereo_reads_mvkeys_not_mvkeysun():
    """KeyFrame.cc:937-938.  A stereo feature with almost no ray parallax: x3D = UnprojectStereo(idx1), from mvKeys[idx1].pt."""
    X = (0.5, 0.2, 6.0)
    near = pose((-0.005, 0, 0))
    u, v, z = project(H.CAM, P1, X)
    s1 = seen(H.CAM, P1, X, True, key=(u + 3.0, v - 2.0))
    s2 = seen(H.CAM, near, X)
    q = {}
    st, _ = H.new_map_point_pair(s1, s2, q=q)
    fx, fy, cx, cy, _ = (float(c) for c in H.CAM)
    want = ((u + 3.0 - cx) * z / fx, (v - 2.0 - cy) * z / fy, z)
    assert q["branch"] == "stereo1" and np.abs(np.array(q["x3d"]) - want).max() < 1e-4
    q2 = {}
    H.new_map_point_pair(s1, s2, rules=("unproject_un",), q=q2)
    assert np.abs(np.array(q2["x3d"]) - np.array(X)).max() < 1e-3 and abs(q2["x3d"][0] - q["x3d"][0]) > 0.03
    # z <= 0 in UnprojectStereo: an empty Mat (:587)
    s1["depth"] = F32(-1e-3)
    assert H.new_map_point_pair(s1, s2)[0] == CODE["empty_unproject"]


UNIT = (F32(1), F32(1), F32(0), F32(0), F32(0))              # fx = fy = 1, cx = cy = 0: a keypoint is its own normalised ray


def test_w_equal_zero():
    """:565.  Two cameras 0.5 apart along x that look the same way, the keypoints on one column and 0.5 apart in y: the fourth
    column of A is orthogonal to the other three (every number dyadic, every product exact), so the Jacobi never rotates it into
    them and the singular vector of the smallest singular value keeps its fourth component exactly 0."""
    s1 = S(0.125, 0.25, pose((-0.25, 0, 0)))
    s2 = S(0.125, -0.25, pose((0.25, 0, 0)))
    q = {}
    st, x = H.new_map_point_pair(s1, s2, cam=UNIT, q=q)
    assert q["cos_rays"] < 0.9998 and st == CODE["w_zero"] and x is None


def test_dist_equal_zero():
    """:657.  x3D = UnprojectStereo(idx1) with a depth so small that Rwc*x3Dc + Ow rounds to the stored Ow; the stored Ow differs
    from -Rcw.t()*tcw here (it is an input of its own), so the point still lies in front of the camera and on the keypoint."""
    cam = H.CAM[:4] + (F32(10.0),)
    cx, cy = float(cam[2]), float(cam[3])
    p1 = pose((0, 0, -0.25), Ow=(0, 0, 0.5))
    s1 = S(cx, cy, p1, ur=cx - 10.0 * 4.0, depth=1e-30)
    s2 = S(cx, cy, pose((0, 0, 0)))
    q = {}
    st, _ = H.new_map_point_pair(s1, s2, cam=cam, q=q)
    assert q["branch"] == "stereo1" and q["z1"] == 0.25 and q["dist1"] == 0.0 and st == CODE["dist_zero"]


def test_th_far_is_inclusive():
    X = (0.5, 0.2, 6.0)
    s1, s2 = seen(H.CAM, P1, X), seen(H.CAM, P2, X)
    q = {}
    assert H.new_map_point_pair(s1, s2, q=q)[0] == H.CREATED
    far = F32(max(q["dist1"], q["dist2"]))
    assert H.new_map_point_pair(s1, s2, far=True, th_far=far)[0] == CODE["far"]                      # dist >= mThFarPoints
    assert H.new_map_point_pair(s1, s2, far=True, th_far=np.nextafter(far, F32(np.inf)))[0] == H.CREATED
    assert H.new_map_point_pair(s1, s2, far=False, th_far=F32(1.0))[0] == H.CREATED


def test_both_sides_of_the_ratio_gate():
    X = (0.5, 0.2, 6.0)
    q = {}
    assert H.new_map_point_pair(seen(H.CAM, P1, X), seen(H.CAM, P2, X), q=q)[0] == H.CREATED
    r = F32(q["ratio"])
    assert H.new_map_point_pair(seen(H.CAM, P1, X, octave=4), seen(H.CAM, P2, X, octave=0))[0] == CODE["ratio_low"]
    assert H.new_map_point_pair(seen(H.CAM, P1, X, octave=0), seen(H.CAM, P2, X, octave=4))[0] == CODE["ratio_high"]
    # on the thresholds (both strict): octaves 0 / 0, ratioOctave = 1; ratio_factor moved one float either way around 1 / ratioDist
    # and around ratioDist
    s1, s2 = seen(H.CAM, P1, X), seen(H.CAM, P2, X)
    lows = {float(f): H.new_map_point_pair(s1, s2, ratio_factor=f)[0] for f in
            [np.nextafter(F32(1 / float(r)), F32(d), dtype=np.float32) for d in (-np.inf, np.inf)] + [F32(1 / float(r))]}
    for f, st in lows.items():
        assert (st == CODE["ratio_low"]) == bool(F32(r * F32(f)) < F32(1)), (f, st)
    assert CODE["ratio_low"] in lows.values() and len(set(lows.values())) == 2
    # a point much nearer to the second camera: ratioDist < 1, the upper bound is far; nearer to the first: the lower bound is far
    # the upper bound, ratioDist > ratioOctave*ratioFactor, strict: a point nearer to the first camera (ratioDist > 1, so the lower
    # bound is far), ratioOctave = 1, ratio_factor = ratioDist itself and one float either way
    Xn = (0.01, 0.0, 0.4)
    a, b = seen(H.CAM, P1, Xn), seen(H.CAM, P2, Xn)
    q = {}
    assert H.new_map_point_pair(a, b, q=q)[0] == H.CREATED
    r = F32(q["ratio"])
    assert r > 1.2
    assert H.new_map_point_pair(a, b, ratio_factor=r)[0] == H.CREATED                                   # equal: not greater
    assert H.new_map_point_pair(a, b, ratio_factor=np.nextafter(r, F32(np.inf)))[0] == H.CREATED
    assert H.new_map_point_pair(a, b, ratio_factor=np.nextafter(r, F32(0)))[0] == CODE["ratio_high"]


def test_the_chi_square_comparison_is_in_double():
    """:609, (errX1*errX1+errY1*errY1) > 5.991*sigmaSquare1: a float against a double product.  The point lies on the first
    camera's axis (from UnprojectStereo of the second keyframe, at the same place), the principal point is 0, so errX1 = -kp1.pt.x
    exactly and the compared float is fl(x*x).  Searched: an x and an octave for which `>` in float (5.991f*sigma2) and in double
    decide differently; the restatement follows the double comparison on both sides of the bound."""
    cam = (F32(4096), F32(4096), F32(0), F32(0), F32(0))       # (long: the ray parallax stays below the stereo parallax)
    ident = pose((0, 0, 0))
    found = 0
    for octave in range(8):
        sig = SIGMA2[octave]
        bound_f, bound_d = F32(F32(5.991) * sig), 5.991 * float(sig)
        x = F32(math.sqrt(bound_d))
        for _ in range(64):
            x = np.nextafter(x, F32(0))
        for _ in range(128):
            x = np.nextafter(x, F32(np.inf))
            e2 = F32(x * x)
            in_double, in_float = float(e2) > bound_d, bool(e2 > bound_f)
            s1 = S(x, 0.0, ident, octave=octave)
            s2 = S(0.0, 0.0, ident, octave=octave, ur=0.0, depth=5.0)
            q = {}
            st, _ = H.new_map_point_pair(s1, s2, cam=cam, mb=F32(0.1), q=q)
            assert q["branch"] == "stereo2" and q["x3d"] == [0.0, 0.0, 5.0]
            assert (st == CODE["reproj1_mono"]) == in_double and (st == H.CREATED) == (not in_double), (octave, float(x))
            found += in_double != in_float
    assert found > 0


# ---- against float64 ----------------------------------------------------------------------------------------------------------
def ulp32(v):
    return float(np.spacing(F32(abs(v))))


def test_decisions_agree_with_float64_wherever_the_margin_allows():
    worst = Counter()
    undecided = decided = 0
    for (seed, coarse, far), (kf1, nbrs, res, _) in scenes().items():
        m0 = [H.search_for_triangulation_fast(kf1.t, nb.kf.t, nb.F12, nb.ep, False, coarse, False)[0] for nb in nbrs]
        for k, nb in enumerate(nbrs):
            for i in np.nonzero(m0[k] >= 0)[0]:
                s1, s2 = H.side(kf1, i), H.side(nb.kf, int(m0[k][i]))
                q32 = {}
                st32, x32 = H.new_map_point_pair(s1, s2, far=far, th_far=TH_FAR, q=q32)
                st64, x64, margins, q64 = H.pair_f64(s1, s2, far=far, th_far=TH_FAR)
                # the only libm-dependent gate: no pair within 2 float ulps of the stereo-parallax comparison
                if s1["ur"] >= 0 or s2["ur"] >= 0:
                    cs = min(q32["cs1"], q32["cs2"])
                    assert abs(q32["cos_rays"] - cs) > 2 * ulp32(cs), (seed, k, i)
                if all(v > H.MEASURED[kind] for kind, v in margins.items()):
                    decided += 1
                    assert STATUS[st32] == st64, (seed, coarse, far, k, i, STATUS[st32], st64, margins)
                    for name, kind in (("cos_rays", "cos"), ("cs1", "cos"), ("cs2", "cos"), ("z1", "z"), ("z2", "z"), ("e1", "px"),
                                       ("e2", "px"), ("dist1", "dist"), ("dist2", "dist")):
                        if name in q32 and name in q64:
                            unit = max(1.0, abs(q64[name])) if kind in ("z", "dist") else 1.0
                            worst[kind] = max(worst[kind], abs(q32[name] - q64[name]) / unit)
                    if "ratio" in q32 and "ratio" in q64:
                        worst["ratio"] = max(worst["ratio"], abs(q32["ratio"] - q64["ratio"]) / q64["ratio"])
                    if st64 == "created":
                        worst["x3d_rel"] = max(worst["x3d_rel"], float(np.abs(x32 - x64).max() / np.linalg.norm(x64)))
                else:
                    undecided += 1
    print("float32 restatement against float64, worst over the decided pairs:", dict(worst), "; decided", decided, "undecided", undecided)
    assert decided > 20 * undecided and decided > 2000
    for kind, v in worst.items():
        assert v <= H.MEASURED[kind], (kind, v)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_the_header_the_library_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    name = "pli_create_new_map_points"
    decl = re.search(r"pli_status\s+%s\s*\(([^;]*)\);" % name, hdr)
    assert decl, name
    assert name in capi._PROTOS and len(capi._PROTOS[name][1]) == 33 == decl.group(1).count(",") + 1
    assert hasattr(lib, name) and hasattr(Frontend, "create_new_map_points")
    codes = dict((n, int(v)) for n, v in re.findall(r"PLI_NEWPT_(\w+) = (\d+)", hdr))
    assert [n.lower() for n, _ in sorted(codes.items(), key=lambda kv: kv[1])] == list(capi.NEWPT_STATUS) == list(STATUS)
    assert (capi.NEWPT_CREATED, capi.NEWPT_TAKEN_EARLIER, capi.NEWPT_NOT_MATCHED) == (H.CREATED, H.TAKEN_EARLIER, H.NOT_MATCHED)


def test_a_null_context_is_refused_before_any_device_call():
    L = capi.lib()
    p = capi.ptr
    buf = np.zeros(64, np.uint8)
    cam = capi.FuseCamera(435.0, 435.0, 367.0, 252.0, 47.9, 0.0, 752.0, 0.0, 480.0)
    a = p(buf)
    assert L.pli_create_new_map_points(None, a, a, a, a, a, a, a, 0, 0, a, a, a, a, a, a, a, a, a, a, a, a, C.byref(cam), 0.1, 0, 0, 0.0,
                                       1.8, a, a, a, a, a) == -1                  # PLI_ERR_INVALID
    assert b"bad argument" in L.pli_last_error()


def test_the_adapter_is_valid_cpp_against_stub_types():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "new_map_points_harness.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
