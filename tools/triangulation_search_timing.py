#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_for_triangulation (ORBmatcher::SearchForTriangulation of one keyframe against
nkf neighbours in one call, LocalMapping::CreateNewMapPoints' loop) on 1200-feature ORB tables of synthetic sequences
(752 x 480, EuRoC defaults), FeatureVectors from a synthetic DBoW2 vocabulary (k = 10, L = 4, levelsup 2: about 100 nodes, like
ORBvoc's k = 10, L = 6 at levelsup 4), a fifth of the features holding map points, mbCheckOrientation off as on the real call
path.  The neighbours are the other frames of the keyframe's sequence and their right images under a rectified-pair geometry
(epipolar lines = rows), so a good share of the candidates passes the epipolar gate.
Prints ONE JSON line: the median over --calls calls after --warmup calls, per nkf, and for the largest nkf <= 10 the same
neighbours as single calls one after the other (what batching buys).

  python tools/triangulation_search_timing.py [--nkf 1,10,20] [--calls 50] [--warmup 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nkf", default="1,10,20")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    fe = Frontend(capi.default_config(752, 480), dev=False)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))
    rng = np.random.default_rng(0)

    def table(img):
        n, kp, desc = fe.orb_extract(0, img)
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return (kp.copy(), desc.copy(), np.where(weight > 0, node, -1).astype(np.int32), (rng.random(n) < 0.2).astype(np.uint8),
                (rng.random(n) < 0.6).astype(np.uint8))

    # x1' F12 x2 = 0 <=> y1 = y2 (a rectified pair: t12 along x, R12 = I); the epipole lies at infinity
    fx, fy, cx, cy = 458.654, 457.296, 367.215, 248.375
    Kinv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    F12 = (Kinv.T @ np.array([[0, 0, 0], [0, 0, 0.11], [0, -0.11, 0]]) @ Kinv).astype(np.float32)
    ep = np.array([1e9, cy], np.float32)
    kf1 = table(synth.make_stereo_pair(5, t=0)[0])
    pool = [table(synth.make_stereo_pair(5, t=t)[e]) + (F12, ep) for t in range(10) for e in (1, 0)][1:]
    ns = [int(k) for k in a.nkf.split(",")]
    kfs_all = [pool[i % len(pool)] for i in range(max(ns))]
    out = {"tool": "triangulation_search_timing", "n1": int(len(kf1[2])), "kf_features": int(np.mean([len(k[2]) for k in kfs_all])),
           "calls": a.calls, "median_ms": {}, "matches_per_kf": {}}

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    for nkf in ns:
        kfs = kfs_all[:nkf]
        out["median_ms"][str(nkf)] = median_ms(lambda: fe.search_for_triangulation(kf1, kfs))
        out["matches_per_kf"][str(nkf)] = round(float(fe.search_for_triangulation(kf1, kfs)[1].mean()), 1)
    single = max([n for n in ns if n <= 10] or [min(ns)])
    out["single_calls"] = {"nkf": single, "median_ms": median_ms(
        lambda: [fe.search_for_triangulation(kf1, kfs_all[k:k + 1]) for k in range(single)])}
    print(json.dumps(out))
    fe.close()


if __name__ == "__main__":
    main()
