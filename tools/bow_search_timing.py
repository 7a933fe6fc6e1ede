#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_by_bow (ORBmatcher::SearchByBoW for K keyframes against one frame in one call,
Tracking::Relocalization's loop) on 1200-feature ORB tables of synthetic sequences (752 x 480, EuRoC defaults), FeatureVectors
from a synthetic DBoW2 vocabulary (k = 10, L = 4, levelsup 2: about 100 nodes, like ORBvoc's k = 10, L = 6 at levelsup 4).
Prints ONE JSON line: the median over --calls calls after --warmup calls, per K.

  python tools/bow_search_timing.py [--k 1,8,32,128] [--calls 50] [--warmup 10]
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
    ap.add_argument("--k", default="1,8,32,128")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    fe = Frontend(capi.default_config(752, 480), dev=False)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))

    def table(img):
        n, kp, desc = fe.orb_extract(0, img)
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return desc, kp["angle"].astype(np.float32), np.where(weight > 0, node, -1).astype(np.int32)

    rng = np.random.default_rng(0)
    fd, fa, fn = table(synth.make_stereo_pair(5, t=3)[0])
    pool = [table(synth.make_stereo_pair(s, t=t)[0]) for s in (5, 6, 7, 8) for t in range(4)]
    ks = [int(k) for k in a.k.split(",")]
    kfs_all = [pool[i % len(pool)] + ((rng.random(len(pool[i % len(pool)][2])) >= 0.2).astype(np.uint8),) for i in range(max(ks))]
    out = {"tool": "bow_search_timing", "nf": int(len(fn)), "kf_features": int(np.mean([len(k[2]) for k in kfs_all])),
           "calls": a.calls, "median_ms": {}, "matches_per_kf": {}}
    for K in ks:
        kfs = kfs_all[:K]
        for _ in range(a.warmup):
            fe.search_by_bow(fd, fa, fn, kfs, 0.75, True)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            m, n = fe.search_by_bow(fd, fa, fn, kfs, 0.75, True)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["median_ms"][str(K)] = round(float(np.median(ts)), 4)
        out["matches_per_kf"][str(K)] = round(float(n.mean()), 1)
    print(json.dumps(out))
    fe.close()


if __name__ == "__main__":
    main()
