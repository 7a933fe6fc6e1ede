"""The C++ local-map adapters, executed (-m gpu): tests/cpp/local_map_harness.cpp runs ORB_SLAM3::PliSearchLocalPoints and
PliSearchLocalLines (pli_slam_amd/adapters/orbslam_local_map.hpp; Tracking.cc:3809-3919) on stub Frame / MapPoint / MapLine types:
a local map with bad points and lines, ones already seen in this frame, points seen in this frame that still carry mbTrackInView
from an earlier one (with and without a keypoint in their stale window), rows of the frame held at entry by points and lines with and
without observations.  Every field the reference writes and both containers equal the restatement of tests/helpers_local_map.py
plus the host gate of Tracking.cc:3886-3919."""
import math
import os
import subprocess

import numpy as np
import pytest

import helpers_local_map as lm
from helpers_local_map import CAM, f32
from test_fuse_search_cpu import SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
NNRATIO, TH, TH_FAR, NNR = 0.8, 3.0, 12.0, 0.9
POINT_OUT = np.dtype([("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("depth", "<f4"),
                      ("view_cos", "<f4"), ("level", "<i4"), ("visible", "<i4")])
LINE_OUT = np.dtype([("in_view", "<i4"), ("projs_x", "<f4"), ("projs_y", "<f4"), ("visible", "<i4"), ("angle", "<f8")])
UNTOUCHED = (75.0, 76.0, 77.0, 78.0, 80.0, 79)             # the harness's initial mTrackProjX, Y, XR, depth, viewCos, level


def build(outdir):
    exe = os.path.join(outdir, "local_map_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "local_map_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def make_world(seed=31, nq=300, ncur=300, nl=200, n2=50):
    rng = np.random.default_rng(seed)
    pose, pts, descs, kp, desc, ur, _ = lm.point_scene(seed, nq, ncur)
    pts = pts.copy()
    entry = np.where(rng.random(ncur) < 0.15, rng.integers(0, nq, ncur), -1).astype(np.int32)
    state = np.where(rng.random(nq) < 0.1, 1, 0).astype(np.int32)             # 1: bad
    state[entry[entry >= 0]] = 2                                              # held by the frame: seen in this frame (:3782)
    pts["valid"] = state == 0
    # state 3: seen in this frame (an outlier of TrackWithMotionModel, Tracking.cc:2996-3004: its row is NULL by now) with
    # mbTrackInView left set by an earlier frame; most aimed at a keypoint, the rest at a spot with no keypoint within 40 px
    descs = descs.copy()
    taken = np.flatnonzero((entry < 0) & np.isin(np.arange(ncur), lm.search_local_points(pts, descs, pose, kp, desc, ur, None, th=TH, far_points=True,
                                                                            th_far=TH_FAR)[1]))
    for k, i in enumerate(np.flatnonzero((state == 0) & (rng.random(nq) < 0.08))):
        # (the first eight at a keypoint that a live point takes when they are absent: whoever is earlier in the list gets it)
        j = int(taken[(5 * k) % len(taken)]) if k < 8 else int(rng.integers(0, ncur))
        if k < 8 or rng.random() < 0.7:
            x, y = kp["x"][j] + rng.uniform(-2, 2), kp["y"][j] + rng.uniform(-2, 2)
        else:
            while True:
                x, y = rng.uniform(20, 730), rng.uniform(20, 460)
                if np.maximum(np.abs(kp["x"] - x), np.abs(kp["y"] - y)).min() > 40:
                    break
        state[i] = 3
        pts[i:i + 1] = lm.stored_view(x, y, x - rng.uniform(1, 30), rng.uniform(1, 14), rng.uniform(0.99, 1.0), int(kp["octave"][j]))
        descs[i] = desc[j]
    view = lm.is_in_frustum(pts, pose)
    nobs = np.where((view["in_view"] == 1) | (state == 3), rng.integers(1, 5, nq), rng.integers(0, 3, nq)).astype(np.int32)
    _, sp, _, ldescs, cur = lm.line_scene(seed, nl, n2)
    lentry = np.where(rng.random(n2) < 0.2, rng.integers(0, nl, n2), -1).astype(np.int32)
    lstate = np.where(rng.random(nl) < 0.1, 1, 0).astype(np.int32)
    lstate[lentry[lentry >= 0]] = 2
    lnobs = rng.integers(0, 3, nl).astype(np.int32)
    in_view, proj = lm.is_in_frustum_l(sp, lstate == 0, pose)
    # the end point's projection, as some earlier code left it: near the start point's for most lines, anywhere for the rest
    proje = np.where((rng.random(nl) < 0.7)[:, None], proj + rng.uniform(-40, 40, (nl, 2)), rng.uniform(0, 700, (nl, 2))).astype(f32)
    # frame lines: most start near the projection of a map line in view
    seen = np.flatnonzero(in_view)
    src = seen[rng.integers(0, len(seen), n2)]
    off = np.where(rng.random(n2) < 0.3, 3.0, 1.0)[:, None]                   # (the gate is 75.2 px wide, 48 px high)
    kl = np.concatenate([proj[src] + off * rng.uniform(-30, 30, (n2, 2)), proje[src] + off * rng.uniform(-30, 30, (n2, 2))], 1).astype(f32)
    cur = ldescs[src].copy()
    flip = rng.random((n2, 32)) < 0.05
    cur[flip] ^= rng.integers(1, 256, (n2, 32), dtype=np.uint8)[flip]
    disp = np.where((rng.random(n2) < 0.15)[:, None], -1.0, rng.uniform(1, 30, (n2, 2))).astype(f32)
    return dict(pose=pose, pts=pts, descs=descs, kp=kp, desc=desc, ur=ur, entry=entry, state=state, nobs=nobs, sp=sp, ldescs=ldescs,
                cur=np.ascontiguousarray(cur), lentry=lentry, lstate=lstate, lnobs=lnobs, proje=proje, kl=kl, disp=disp)


def write_input(path, w, b_far=1, frame_id=9):
    nq, ncur, nl, n2 = len(w["pts"]), len(w["kp"]), len(w["sp"]), len(w["cur"])
    with open(path, "wb") as f:
        f.write(np.array([nq, ncur, nl, n2, b_far, frame_id], np.int32).tobytes())
        f.write(w["pose"].tobytes() + np.array(list(CAM) + [NNRATIO, TH, TH_FAR, NNR], f32).tobytes() + SF.astype(f32).tobytes())
        kp = w["kp"]
        f.write(kp["x"].tobytes() + kp["y"].tobytes() + kp["octave"].astype(np.int32).tobytes() + w["desc"].tobytes() +
                w["ur"].tobytes() + w["entry"].tobytes())
        for i in range(nq):
            f.write(w["pts"][i:i + 1].tobytes() + np.array([w["state"][i], w["nobs"][i]], np.int32).tobytes() + w["descs"][i].tobytes())
        f.write(w["cur"].tobytes() + w["kl"].tobytes() + w["disp"].tobytes() + w["lentry"].tobytes())
        for i in range(nl):
            f.write(w["sp"][i].astype(f32).tobytes() + np.array([w["lstate"][i], w["lnobs"][i]], np.int32).tobytes() +
                    w["proje"][i].tobytes() + w["ldescs"][i].tobytes())


def expected(w, b_far=1):
    """What the reference leaves behind: -> nmatches, mvpMapPoints, point records, mmProjectPoints, list, matches_12, mvpMapLines,
    line records (the track angle as the two overloads of atan2 give it)."""
    nq, nl = len(w["pts"]), len(w["sp"])
    occ = np.array([e >= 0 and w["nobs"][e] > 0 for e in w["entry"].tolist()], np.uint8)
    view, best, n_in_view, nmatches, _ = lm.search_local_points(w["pts"], w["descs"], w["pose"], w["kp"], w["desc"], w["ur"], occ,
                                                                th=TH, far_points=bool(b_far), th_far=TH_FAR, nnratio=NNRATIO)
    mps = w["entry"].copy()
    for i in np.flatnonzero(best >= 0):
        mps[best[i]] = i
    rec = np.zeros(nq, POINT_OUT)
    for i in range(nq):
        V = view[i]
        x, y, xr, d, c, l = UNTOUCHED
        if w["state"][i] == 3:                                                # nothing is written; the stored fields stand
            P = w["pts"][i]
            rec[i] = (1, P["pos"][0], P["pos"][1], P["pos"][2], P["normal"][0], P["normal"][1], int(P["normal"][2]), 0)
            continue
        if w["pts"]["valid"][i]:
            x, y = V["proj_x"], V["proj_y"]
            if V["in_view"]:
                xr, d, c, l = V["proj_xr"], V["depth"], V["view_cos"], V["level"]
        rec[i] = (V["in_view"], x, y, xr, d, c, l, V["in_view"])
    project = [(i, view["proj_x"][i], view["proj_y"][i]) for i in np.flatnonzero(view["in_view"])]
    valid = w["lstate"] == 0
    in_view, proj, lst, m, _ = lm.search_local_lines(w["sp"], valid, w["ldescs"], w["pose"], w["cur"], NNR)
    projs = np.where(in_view[:, None] == 1, proj, np.array([75.0, 76.0], f32)).astype(f32)
    locc = np.array([e >= 0 and w["lnobs"][e] > 0 for e in w["lentry"].tolist()], bool)
    m_after, assigned = lm.host_line_gate(lst, m, projs, w["proje"], w["kl"][:, :2], w["kl"][:, 2:], w["disp"], locc, w["lnobs"],
                                          (CAM.min_x, CAM.max_x, CAM.min_y, CAM.max_y))
    mls = w["lentry"].copy()
    for i2, li in assigned.items():
        mls[i2] = li
    dy, dx = (w["proje"][:, 1] - projs[:, 1]).astype(f32), (w["proje"][:, 0] - projs[:, 0]).astype(f32)
    # (math.atan2 is the C library's, which the harness calls; numpy's own float64 arctan2 differs from it in the last place)
    ang = [np.where(in_view == 1, np.arctan2(dy, dx).astype(np.float64), 81.0),
           np.where(in_view == 1, np.array([math.atan2(float(a), float(b)) for a, b in zip(dy, dx)]), 81.0)]
    lrec = np.zeros(nl, LINE_OUT)
    lrec["in_view"], lrec["projs_x"], lrec["projs_y"], lrec["visible"] = in_view, projs[:, 0], projs[:, 1], in_view
    return nmatches, mps, rec, project, lst, m, m_after, mls, lrec, ang


def test_the_case_is_not_vacuous():
    w = make_world()
    nmatches, mps, rec, project, lst, m, m_after, mls, lrec, _ = expected(w)
    held = w["entry"] >= 0
    with_obs = np.array([e >= 0 and w["nobs"][e] > 0 for e in w["entry"].tolist()])
    assert nmatches > 20 and len(project) > 60 and (w["state"] == 1).sum() > 10 and (w["state"] == 2).sum() > 10
    assert with_obs.sum() > 5 and (held & ~with_obs).sum() > 3
    # the stored views: some take a keypoint, some find their window empty, and taking them out changes other points' answers
    stored = w["state"] == 3
    took = np.isin(np.flatnonzero(stored), mps[mps >= 0])
    w2 = dict(w, pts=w["pts"].copy())
    w2["pts"]["valid"][stored] = 0
    mps2 = expected(w2)[1]
    print("stored views: %d, %d took a keypoint; %d rows of mvpMapPoints differ without them" % (stored.sum(), took.sum(), (mps != mps2).sum()))
    displaced = int(((mps2 >= 0) & (w["state"][np.maximum(mps2, 0)] == 0) & (mps != mps2) & (mps2 != w["entry"])).sum())
    print("rows that a live point takes without them and loses with them:", displaced)
    assert stored.sum() >= 10 and took.sum() >= 5 and (~took).sum() >= 2 and displaced >= 2
    assert len(lst) > 50 and (m >= 0).sum() > 10
    gated, kept = int(((m >= 0) & (m_after < 0)).sum()), int((mls != w["lentry"]).sum())
    lheld = w["lentry"] >= 0
    lwith = np.array([e >= 0 and w["lnobs"][e] > 0 for e in w["lentry"].tolist()])
    print("lines: %d matches, %d refused by the position gate, %d rows written; held with / without observations: %d / %d" % (
        (m >= 0).sum(), gated, kept, lwith.sum(), (lheld & ~lwith).sum()))
    assert gated >= 3 and kept >= 3 and lwith.sum() >= 2 and (lheld & ~lwith).sum() >= 1
    assert (w["disp"][:, 0] < 0).sum() >= 3


@pytest.mark.gpu
def test_the_adapters_equal_the_restatement_and_the_host_gate(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    w = make_world()
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, w)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = open(outp, "rb").read()
    nmatches, mps, rec, project, lst, m, m_after, mls, lrec, ang = expected(w)
    nq, ncur, nl, n2 = len(w["pts"]), len(w["kp"]), len(w["sp"]), len(w["cur"])
    at = 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(raw, dt, n, at)
        at += a.nbytes
        return a
    assert take(np.int32, 1)[0] == nmatches
    assert np.array_equal(take(np.int32, ncur), mps), "mvpMapPoints"
    got = take(POINT_OUT, nq)
    for name in POINT_OUT.names:
        assert lm.canonical(got[name]) == lm.canonical(rec[name]), name
    npj = int(take(np.int32, 1)[0])
    pj = take(np.dtype([("id", "<i4"), ("x", "<f4"), ("y", "<f4")]), npj)
    assert [(int(a), f32(b), f32(c)) for a, b, c in pj.tolist()] == [(int(a), f32(b), f32(c)) for a, b, c in project], "mmProjectPoints"
    k = int(take(np.int32, 1)[0])
    assert k == len(lst) and np.array_equal(take(np.int32, k), lst), "mvpLocalMapLines_InFrustum"
    assert np.array_equal(take(np.int32, k), m_after), "matches_12"
    assert np.array_equal(take(np.int32, n2), mls), "mvpMapLines"
    gl = take(LINE_OUT, nl)
    for name in ("in_view", "projs_x", "projs_y", "visible"):
        assert gl[name].tobytes() == lrec[name].tobytes(), name
    # mnTrackangle: atan2 of two floats, unqualified as Frame.cc:698 writes it: the float or the double overload, whichever the
    # headers in scope select - exactly one of the two
    assert gl["angle"].tobytes() in (ang[0].tobytes(), ang[1].tobytes()), "mnTrackangle"
    assert at == len(raw)


def test_local_map_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    import torch
    exe = build(str(tmp_path))
    w = make_world(seed=32, nq=40, ncur=30, nl=20, n2=8)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, w)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
