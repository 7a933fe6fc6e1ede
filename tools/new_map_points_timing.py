#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_create_new_map_points (LocalMapping::CreateNewMapPoints from the search on, one keyframe
against nkf neighbours in one call) and, in the same run on the same tables, of pli_search_for_triangulation alone; the difference
is the cost of the list, the geometry and the pick (and of the larger upload and download).  Tables as
tools/triangulation_search_timing.py: 1200-feature ORB tables of synthetic sequences (752 x 480, EuRoC defaults), FeatureVectors
from a synthetic vocabulary, a fifth of the features holding map points, 60 % stereo with a synthetic mvuRight / mvDepth, the
neighbours under a rectified-pair geometry (epipolar lines = rows, 0.11 m apart) so that a good share of the pairs passes the
epipolar gate and reaches the triangulation.
Interleaved series: every round times one call of each form, per nkf; the medians are over the rounds.  No host loop of the
reference is timed here, so nothing is said about a speed-up over it.
Writes ONE JSON object to --out and prints it.

  python tools/new_map_points_timing.py [--nkf 1,10,20] [--rounds 50] [--warmup 10] [--out profiles/new_map_points_timing.json]
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
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_map_points_timing.json"))
    a = ap.parse_args()
    fe = Frontend(capi.default_config(752, 480), dev=False)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))
    rng = np.random.default_rng(0)
    fx, fy, cx, cy, bf = 458.654, 457.296, 367.215, 248.375, 47.90639384423901
    cam = (fx, fy, cx, cy, bf, 0.0, 752.0, 0.0, 480.0)
    mb = float(np.float32(np.float32(bf) / np.float32(fx)))
    ratio_factor = float(np.float32(np.float32(1.5) * np.float32(1.2)))

    def table(img, tx):
        """(kp, desc, node, has_mp, uright, depth, key, pose) and the stereo flags of the search-only call"""
        n, kp, desc = fe.orb_extract(0, img)
        _, weight, node = fe.bow_transform(voc, desc, 2)
        stereo = rng.random(n) < 0.6
        depth = np.where(stereo, rng.uniform(3, 12, n), -1).astype(np.float32)
        uright = np.where(stereo, kp["x"] - bf / np.maximum(depth, 1), -1).astype(np.float32)
        depth[uright < 0] = -1
        uright[uright < 0] = -1
        key = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
        pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, tx, 0, 0, -tx, 0, 0], np.float32)
        return (kp.copy(), desc.copy(), np.where(weight > 0, node, -1).astype(np.int32), (rng.random(n) < 0.2).astype(np.uint8),
                uright, depth, key, pose)

    # x1' F12 x2 = 0 <=> y1 = y2 (a rectified pair: t12 along x, R12 = I); the epipole lies at infinity
    Kinv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    F12 = (Kinv.T @ np.array([[0, 0, 0], [0, 0, 0.11], [0, -0.11, 0]]) @ Kinv).astype(np.float32)
    ep = np.array([1e9, cy], np.float32)
    kf1 = table(synth.make_stereo_pair(5, t=0)[0], 0.0)
    pool = [table(synth.make_stereo_pair(5, t=t)[e], -0.11) + (F12, ep) for t in range(10) for e in (1, 0)][1:]
    ns = [int(k) for k in a.nkf.split(",")]
    kfs_all = [pool[i % len(pool)] for i in range(max(ns))]
    search_of = lambda kf: kf[:4] + ((kf[4] >= 0).astype(np.uint8),)
    s1, skfs_all = search_of(kf1), [search_of(kf) + kf[8:] for kf in kfs_all]
    out = {"tool": "new_map_points_timing", "n1": int(len(kf1[2])), "kf_features": int(np.mean([len(k[2]) for k in kfs_all])),
           "rounds": a.rounds, "create_new_map_points_median_ms": {}, "search_for_triangulation_median_ms": {},
           "geometry_and_pick_ms": {}, "pairs_on_entry_per_kf": {}, "matches_per_kf": {}, "created_per_kf": {}}

    def ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for nkf in ns:
        kfs, skfs = kfs_all[:nkf], skfs_all[:nkf]
        new = lambda: fe.create_new_map_points(kf1, kfs, cam, mb, ratio_factor)
        search = lambda: fe.search_for_triangulation(s1, skfs)
        for _ in range(a.warmup):
            new()
            search()
        tn, ts = [], []
        for _ in range(a.rounds):                      # interleaved: one call of each form per round
            tn.append(ms(new))
            ts.append(ms(search))
        m, n, status, _, nnew = new()
        k = str(nkf)
        out["create_new_map_points_median_ms"][k] = round(float(np.median(tn)), 4)
        out["search_for_triangulation_median_ms"][k] = round(float(np.median(ts)), 4)
        out["geometry_and_pick_ms"][k] = round(float(np.median(tn)) - float(np.median(ts)), 4)
        out["pairs_on_entry_per_kf"][k] = round(float(search()[1].mean()), 1)
        out["matches_per_kf"][k] = round(float(n.mean()), 1)
        out["created_per_kf"][k] = round(float(nnew.mean()), 1)
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    fe.close()


if __name__ == "__main__":
    main()
