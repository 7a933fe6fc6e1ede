#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_by_projection_sim3 (loop closing's ORBmatcher::SearchByProjection(pKF, Scw, ...)
for one list of map points against npair (keyframe, Scw) pairs in one call) on 1200-feature ORB tables of a synthetic sequence
(752 x 480, EuRoC defaults), th = 8, ratio 1.5.  The map points are the stereo keypoints of frame 0 unprojected (repeated with a
small jitter to reach the requested count); the keyframes are the frames of the sequence under small motions.
Prints ONE JSON line: the median over --calls calls after --warmup calls through Frontend.search_by_projection_sim3 for npair x
--points points, the same pairs as single calls one after the other, pli_fuse_search in Sim3 mode on the same tables (the
yardstick for the parallel phases), the kernels' share of one call (pli_prof_enable: HIP events around every launch), and, with
--widths 8,16,32,64, the development build with PLI_SIM3_WIDTH (keys per candidate list), every width in this one process,
interleaved, and the two kernels the width touches under HIP events.

  python tools/sim3_projection_timing.py [--npair 1,3,6] [--points 3000] [--calls 50] [--warmup 10] [--widths 8,16,32,64]
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

TH, RATIO = 8.0, 1.5
KERNELS = ("k_fuse_grid", "k_sim3_project", "k_sim3_candidates", "k_sim3_assign")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npair", default="1,3,6")
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--widths", default="")
    a = ap.parse_args()
    cfg = capi.default_config(752, 480)
    fe = Frontend(cfg, dev=False)
    rng = np.random.default_rng(0)
    fx, cx, cy, bf = float(cfg.fx), 367.215, 248.375, float(cfg.bf)
    cam = (fx, fx, cx, cy, bf, 0.0, 752.0, 0.0, 480.0)
    sf = np.float32(cfg.orb_scale_factor) ** np.arange(cfg.orb_nlevels, dtype=np.float32)
    recs = [fe.batch_run_host(np.stack(synth.make_stereo_pair(5, t=t))[None])[0] for t in range(6)]

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

    ns = [int(k) for k in a.npair.split(",")]
    kfs_all = [keyframe(i) for i in range(max(ns))]
    pairs_all = [(k[0], k[1], k[3]) for k in kfs_all]
    pts, descs = points(a.points)
    search = lambda f, pairs: f.search_by_projection_sim3(pts, descs, pairs, cam, TH, RATIO)
    out = {"tool": "sim3_projection_timing", "kf_features": int(np.mean([len(k[1]) for k in kfs_all])), "points": a.points,
           "th": TH, "ratio_hamming": RATIO, "calls": a.calls, "median_ms": {}, "single_calls_median_ms": {},
           "fuse_search_sim3_median_ms": {}, "matches_per_pair": {}, "kernel_ms_per_call": {}}
    for n in ns:
        pairs = pairs_all[:n]
        out["median_ms"][str(n)] = median_ms(lambda: search(fe, pairs))
        out["single_calls_median_ms"][str(n)] = median_ms(lambda: [search(fe, pairs[k:k + 1]) for k in range(n)])
        out["fuse_search_sim3_median_ms"][str(n)] = median_ms(lambda: fe.fuse_search(pts, descs, kfs_all[:n], cam, TH, False))
        out["matches_per_pair"][str(n)] = round(float(search(fe, pairs)[2].mean()), 1)
        fe.prof_enable(True)
        fe.prof_reset()
        for _ in range(a.calls):
            search(fe, pairs)
        rep = fe.prof_report()
        fe.prof_enable(False)
        out["kernel_ms_per_call"][str(n)] = {k: round(rep[k][1] / rep[k][0], 4) for k in KERNELS if k in rep}
    if a.widths:
        dev = Frontend(cfg, dev=True)
        widths = [int(w) for w in a.widths.split(",")]
        pairs = pairs_all[:max(ns)]
        ts = {w: [] for w in widths}
        for rnd in range(a.warmup + a.calls):
            for w in widths:
                os.environ["PLI_SIM3_WIDTH"] = str(w)
                t0 = time.perf_counter()
                search(dev, pairs)
                if rnd >= a.warmup:
                    ts[w].append((time.perf_counter() - t0) * 1e3)
        out["widths_median_ms_%d_pairs" % max(ns)] = {str(w): round(float(np.median(ts[w])), 4) for w in widths}
        assign = {}
        for w in widths:
            os.environ["PLI_SIM3_WIDTH"] = str(w)
            dev.prof_enable(True)
            dev.prof_reset()
            for _ in range(a.calls):
                search(dev, pairs)
            rep = dev.prof_report()
            dev.prof_enable(False)
            assign[str(w)] = {k: round(rep[k][1] / rep[k][0], 4) for k in ("k_sim3_candidates", "k_sim3_assign") if k in rep}
        os.environ.pop("PLI_SIM3_WIDTH", None)
        out["widths_kernel_ms_%d_pairs" % max(ns)] = assign
        dev.close()
    print(json.dumps(out))
    fe.close()


if __name__ == "__main__":
    main()
