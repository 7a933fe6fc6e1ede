#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_for_triangulation_two_cameras (ORBmatcher::SearchForTriangulation for keyframes of
two KannalaBrandt8 cameras, one keyframe against nkf neighbours in one call) through the Python mirror, on keyframes of about
1200 + 1200 features: the left and the right image of a synthetic stereo frame (752 x 480) through pli_orb_extract, FeatureVectors
from a synthetic DBoW2 vocabulary (k = 10, L = 4, levelsup 2), a fifth of the features holding map points, mbCheckOrientation off as
on the real call path.  The neighbours are the other frames of the sequence, read as a rig that moves sideways, so that a share of
the candidates passes the triangulation gate and a share leaves it early.
In the same run, interleaved: the same neighbours as single calls, and pli_search_for_triangulation (the one-camera entry point, the
yardstick for what the KannalaBrandt8 gate adds) on tables of the same size.  Under HIP events (pli_prof_enable): the kernels of one
call, the number of launches per call for every nkf, and the share of the call that the match kernel takes.
Prints ONE JSON line and writes it to --out.  No host loop of the reference is timed here.

  python tools/triangulation_two_cameras_timing.py [--nkf 1,6,12] [--calls 50] [--repeats 5] [--warmup 10] [--out profiles/triangulation_two_cameras_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pli_slam_amd import capi, synth  # noqa: E402
from pli_slam_amd.frontend import Frontend  # noqa: E402

KERNELS = ("k_kb8_rays", "k_node_sort", "k_tri_match_kb8", "k_tri_finish")
KERNELS_ONE = ("k_node_sort", "k_tri_match", "k_tri_finish")
# TUM-VI's distortion coefficients around the centre of a 752 x 480 image
CAM_LEFT = [250.0, 250.0, 376.0, 240.0, 0.00348238940, 0.000715034845, -0.00205323614, 0.000202936736]
CAM_RIGHT = [249.3, 249.3, 374.0, 238.5, 0.00340031805, 0.00176627874, -0.00266312161, 0.000329951911]


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(R, centre):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, -R @ np.asarray(centre, np.float64)
    return T


def relative_poses(T1, T2, Tlr):
    """ll, lr, rl, rr (ORBmatcher.cc:995-1003) as 4 x 12 floats: camera b of keyframe 2 -> camera a of keyframe 1."""
    Trl = np.linalg.inv(Tlr)
    rel = np.zeros((4, 12), np.float32)
    for a in (0, 1):
        for b in (0, 1):
            T12 = (Trl @ T1 if a else T1) @ np.linalg.inv(Trl @ T2 if b else T2)
            rel[2 * a + b, :9], rel[2 * a + b, 9:] = T12[:3, :3].reshape(9), T12[:3, 3]
    return rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nkf", default="1,6,12")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulation_two_cameras_timing.json"))
    a = ap.parse_args()
    fe = Frontend(capi.default_config(752, 480, orb_nfeatures=1200), dev=False)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))
    rng = np.random.default_rng(0)
    Tlr = pose(rot(0.0, np.deg2rad(2.0), 0.0).T, (0.0, 0.0, 0.0))
    Tlr[:3, 3] = (0.101, 0.002, -0.001)
    T1 = pose(np.eye(3), (0.0, 0.0, 0.0))

    def keyframe(t):
        """(kp, desc, node, has_mp, nleft): the left image's features, then the right image's."""
        parts = []
        for img in synth.make_stereo_pair(5, t=t):
            n, kp, desc = fe.orb_extract(0, img)
            parts.append((kp[:n].copy(), desc[:n].copy()))
        kp, desc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return (kp, desc, np.where(weight > 0, node, -1).astype(np.int32), (rng.random(len(kp)) < 0.2).astype(np.uint8), len(parts[0][0]))

    ns = [int(k) for k in a.nkf.split(",")]
    kf1 = keyframe(0)
    pool = []
    for t in range(1, max(ns) + 1):
        T2 = pose(rot(0.0, 0.0, 0.0087 * t), (-0.04 * t, -0.013 * t, 0.0))
        pool.append(keyframe(t) + (relative_poses(T1, T2, Tlr),))
    # the one-camera call on tables of the same size: every feature mono, a rectified-pair F12 (lines = rows), the epipole far away
    fx, fy, cx, cy = 458.654, 457.296, 367.215, 248.375
    Kinv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    F12 = (Kinv.T @ np.array([[0, 0, 0], [0, 0, 0.11], [0, -0.11, 0]]) @ Kinv).astype(np.float32)
    ep = np.array([1e9, cy], np.float32)
    one = lambda kf: kf[:4] + (np.zeros(len(kf[2]), np.uint8),)
    kf1_one, pool_one = one(kf1), [one(kf) + (F12, ep) for kf in pool]

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    def kernel_split(fn, names):
        """-> (ms per call by kernel, launches per call)"""
        fe.prof_enable(True)
        fe.prof_reset()
        for _ in range(a.calls):
            fn()
        rep = fe.prof_report()
        fe.prof_enable(False)
        return {k: round(rep[k][1] / a.calls, 4) for k in names if k in rep}, sum(v[0] for v in rep.values()) / a.calls

    out = {"tool": "triangulation_two_cameras_timing", "calls": a.calls, "repeats": a.repeats, "n1": int(len(kf1[2])),
           "n1_left": int(kf1[4]), "kf_features": int(np.mean([len(k[2]) for k in pool])), "nkf": {}}
    for nkf in ns:
        kfs, kfs_one = pool[:nkf], pool_one[:nkf]
        batch = lambda: fe.search_for_triangulation_two_cameras(kf1, kfs, CAM_LEFT, CAM_RIGHT)
        singles = lambda: [fe.search_for_triangulation_two_cameras(kf1, kfs[k:k + 1], CAM_LEFT, CAM_RIGHT) for k in range(nkf)]
        yard = lambda: fe.search_for_triangulation(kf1_one, kfs_one)
        res = {"matches_per_kf": round(float(batch()[1].mean()), 1), "one_camera_matches_per_kf": round(float(yard()[1].mean()), 1),
               "coarse_matches_per_kf": round(float(fe.search_for_triangulation_two_cameras(kf1, kfs, CAM_LEFT, CAM_RIGHT, coarse=True)[1].mean()), 1),
               "median_ms": [], "single_calls_median_ms": [], "one_camera_median_ms": []}
        for _ in range(a.repeats):                 # interleaved series, so that a drift of the box shows in all three
            res["median_ms"].append(median_ms(batch))
            res["single_calls_median_ms"].append(median_ms(singles))
            res["one_camera_median_ms"].append(median_ms(yard))
        ks, launches = kernel_split(batch, KERNELS)
        res["kernel_ms_per_call"], res["launches_per_call"] = ks, launches
        res["one_camera_kernel_ms_per_call"], res["one_camera_launches_per_call"] = kernel_split(yard, KERNELS_ONE)
        if "k_tri_match_kb8" in ks:
            res["match_share_of_kernels"] = round(ks["k_tri_match_kb8"] / sum(ks.values()), 3)
            res["match_share_of_call"] = round(ks["k_tri_match_kb8"] / float(np.median(res["median_ms"])), 3)
        out["nkf"][str(nkf)] = res
    fe.vocab_destroy(voc)
    fe.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
