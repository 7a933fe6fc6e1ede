#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_by_bow_kf (ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) for one keyframe
against K keyframes in one call, LoopClosing::DetectCommonRegionsFromBoW's loop: 6 covisibles per candidate, up to 36 per inserted
keyframe) on 1200-feature ORB tables of synthetic sequences (752 x 480, EuRoC defaults), FeatureVectors from a synthetic DBoW2
vocabulary (k = 10, L = 4, levelsup 2: about 100 nodes, like ORBvoc's k = 10, L = 6 at levelsup 4).  Next to one batched call of
K keyframes, the same K pairs as K single calls.  Prints ONE JSON line (and writes it to --out): the median over --calls
repetitions after --warmup repetitions, per K, all in this one process.

  python tools/bow_kf_search_timing.py [--k 1,6,36] [--calls 50] [--warmup 10] [--out profiles/bow_kf_search_timing.json]
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
    ap.add_argument("--k", default="1,6,36")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fe = Frontend(capi.default_config(752, 480), dev=False)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))
    rng = np.random.default_rng(0)

    def table(img):
        n, kp, desc = fe.orb_extract(0, img)
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return (desc, kp["angle"].astype(np.float32), np.where(weight > 0, node, -1).astype(np.int32),
                (rng.random(len(node)) >= 0.2).astype(np.uint8))

    kf1 = table(synth.make_stereo_pair(5, t=3)[0])
    pool = [table(synth.make_stereo_pair(s, t=t)[0]) for s in (5, 6, 7, 8) for t in range(4)]
    ks = [int(k) for k in a.k.split(",")]
    kfs_all = [pool[i % len(pool)] for i in range(max(ks))]
    out = {"tool": "bow_kf_search_timing", "n1": int(len(kf1[2])), "kf_features": int(np.mean([len(k[2]) for k in kfs_all])),
           "calls": a.calls, "median_ms_one_call": {}, "median_ms_single_calls": {}, "matches_per_kf": {}}

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    for K in ks:
        kfs = kfs_all[:K]
        out["median_ms_one_call"][str(K)] = median_ms(lambda: fe.search_by_bow_kf(*kf1, kfs, 0.75, True))
        if K > 1:
            out["median_ms_single_calls"][str(K)] = median_ms(lambda: [fe.search_by_bow_kf(*kf1, [kf], 0.75, True) for kf in kfs])
        out["matches_per_kf"][str(K)] = round(float(fe.search_by_bow_kf(*kf1, kfs, 0.75, True)[1].mean()), 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    fe.close()


if __name__ == "__main__":
    main()
