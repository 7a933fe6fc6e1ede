#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_fuse_search (the search half of ORBmatcher::Fuse for a list of map points against nkf
keyframes in one call, LocalMapping::SearchInNeighbors' loops) on 1200-feature ORB tables of a synthetic sequence (752 x 480,
EuRoC defaults).  The map points are the stereo keypoints of frame 0 unprojected (repeated with a small jitter to reach the
requested count); the keyframes are the frames of the sequence under small motions.
Prints ONE JSON line: the median over --calls calls after --warmup calls for nkf x 1200 points and for 1 keyframe x 30000 points,
the largest nkf <= 10 as single calls one after the other (what batching buys), and, with --lanes 8,16,64, the same through the
development build with PLI_FUSE_LANES (lanes per surviving pair in k_fuse_match), every width in this one process, interleaved.

  python tools/fuse_search_timing.py [--nkf 1,10,30] [--calls 50] [--warmup 10] [--lanes 8,16,64]
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
    ap.add_argument("--nkf", default="1,10,30")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lanes", default="")
    a = ap.parse_args()
    cfg = capi.default_config(752, 480)
    fe = Frontend(cfg, dev=False)
    rng = np.random.default_rng(0)
    fx, cx, cy, bf = float(cfg.fx), 367.215, 248.375, float(cfg.bf)
    cam = (fx, fx, cx, cy, bf, 0.0, 752.0, 0.0, 480.0)
    sf = np.float32(cfg.orb_scale_factor) ** np.arange(cfg.orb_nlevels, dtype=np.float32)
    recs = [fe.batch_run_host(np.stack(synth.make_stereo_pair(5, t=t))[None])[0] for t in range(10)]

    def points(n):
        r = recs[0]
        sel = np.nonzero(r["depth"] > 0)[0]
        sel = sel[np.arange(n) % len(sel)]
        z = r["depth"][sel].astype(np.float64) * rng.uniform(0.99, 1.01, n)
        pos = np.stack([(r["kpL"]["x"][sel] - cx) * z / fx, (r["kpL"]["y"][sel] - cy) * z / fx, z], 1)
        dist = np.linalg.norm(pos, axis=1)
        p = np.zeros(n, capi.FUSE_POINT_DT)
        p["pos"], p["normal"] = pos, pos / dist[:, None]
        p["max_dist"] = dist * sf[r["kpL"]["octave"][sel]]
        p["min_dist_inv"] = 0.8 * p["max_dist"] / sf[-1]
        p["max_dist_inv"] = 1.2 * p["max_dist"]
        p["valid"] = 1
        return p, r["descL"][sel].copy()

    def keyframe(i):
        r = recs[i % len(recs)]
        t = np.array([0.01 * (i % 7), 0.005 * (i % 3), -0.02 * (i % 5)], np.float32)
        pose = np.concatenate([np.eye(3, dtype=np.float32).reshape(9), t, -t]).astype(np.float32)
        return r["kpL"].copy(), r["descL"].copy(), r["uright"].copy(), pose

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    ns = [int(k) for k in a.nkf.split(",")]
    kfs_all = [keyframe(i) for i in range(max(ns))]
    p12, d12 = points(1200)
    p30k, d30k = points(30000)
    out = {"tool": "fuse_search_timing", "kf_features": int(np.mean([len(k[1]) for k in kfs_all])), "calls": a.calls,
           "median_ms_1200_points": {}, "matches_per_kf": {}}
    for nkf in ns:
        kfs = kfs_all[:nkf]
        out["median_ms_1200_points"][str(nkf)] = median_ms(lambda: fe.fuse_search(p12, d12, kfs, cam))
        out["matches_per_kf"][str(nkf)] = round(float((fe.fuse_search(p12, d12, kfs, cam)[0] >= 0).sum()) / nkf, 1)
    out["median_ms_1kf_30000_points"] = median_ms(lambda: fe.fuse_search(p30k, d30k, kfs_all[:1], cam))
    single = max([n for n in ns if n <= 10] or [min(ns)])
    out["single_calls"] = {"nkf": single, "median_ms": median_ms(
        lambda: [fe.fuse_search(p12, d12, kfs_all[k:k + 1], cam) for k in range(single)])}
    if a.lanes:
        dev = Frontend(cfg, dev=True)
        widths = [int(w) for w in a.lanes.split(",")]
        ts = {w: {"30kf_1200": [], "1kf_30000": []} for w in widths}
        for rnd in range(a.warmup + a.calls):
            for w in widths:
                os.environ["PLI_FUSE_LANES"] = str(w)
                for name, fn in (("30kf_1200", lambda: dev.fuse_search(p12, d12, kfs_all[:max(ns)], cam)),
                                 ("1kf_30000", lambda: dev.fuse_search(p30k, d30k, kfs_all[:1], cam))):
                    t0 = time.perf_counter()
                    fn()
                    if rnd >= a.warmup:
                        ts[w][name].append((time.perf_counter() - t0) * 1e3)
        os.environ.pop("PLI_FUSE_LANES", None)
        out["lanes_median_ms"] = {str(w): {k: round(float(np.median(v)), 4) for k, v in ts[w].items()} for w in widths}
        dev.close()
    print(json.dumps(out))
    fe.close()


if __name__ == "__main__":
    main()
