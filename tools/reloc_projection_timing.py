#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_by_projection_reloc (relocalisation's ORBmatcher::SearchByProjection(CurrentFrame,
pKF, sAlreadyFound, th, ORBdist) for one frame table against ncand candidates in one call) on the ORB tables of a synthetic
sequence (752 x 480, EuRoC defaults, about 1200 rows), with the two settings of Tracking.cc:4290 / :4304.  The frame is frame 0 of
the sequence; a candidate lists --points map points: the stereo keypoints of frame 0 unprojected (repeated with a small jitter to
reach the count, in an order of its own), seen through a small motion of its own; its keyframe angles are the frame's plus a common
rotation, so the rotation filter keeps most matches.
Prints ONE JSON line and writes it to --out: the median over --calls calls after --warmup calls through
Frontend.search_by_projection_reloc for ncand candidates in one call, the same candidates as single calls one after the other,
the kernels' share of one call (pli_prof_enable: HIP events around every launch), and pli_search_by_projection_sim3 on the same
tables in the same run (candidate 0's points against the frame's table as ncand pairs, the same th, ratio = ORBdist / 50): the
yardstick for the ordered walk.

  python tools/reloc_projection_timing.py [--ncand 1,2,4] [--points 1200] [--calls 50] [--warmup 10] [--out profiles/reloc_projection_timing.json]
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

SETTINGS = ((10.0, 100), (3.0, 64))                                      # Tracking.cc:4290, :4304
KERNELS = ("k_fuse_grid", "k_reloc_project", "k_reloc_candidates", "k_reloc_assign")
SIM3_KERNELS = ("k_fuse_grid", "k_sim3_project", "k_sim3_candidates", "k_sim3_assign")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncand", default="1,2,4")
    ap.add_argument("--points", type=int, default=1200)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_projection_timing.json"))
    a = ap.parse_args()
    cfg = capi.default_config(752, 480)
    fe = Frontend(cfg, dev=False)
    rng = np.random.default_rng(0)
    fx, cx, cy, bf = float(cfg.fx), 367.215, 248.375, float(cfg.bf)
    cam = (fx, fx, cx, cy, bf, 0.0, 752.0, 0.0, 480.0)
    sf = np.float32(cfg.orb_scale_factor) ** np.arange(cfg.orb_nlevels, dtype=np.float32)
    rec = fe.batch_run_host(np.stack(synth.make_stereo_pair(5, t=0))[None])[0]
    frame_kp, frame_desc = rec["kpL"].copy(), rec["descL"].copy()

    def candidate(i, n):
        sel = np.nonzero(rec["depth"] > 0)[0]
        sel = rng.permutation(sel[np.arange(n) % len(sel)])
        z = rec["depth"][sel].astype(np.float64) * rng.uniform(0.99, 1.01, n)
        pos = np.stack([(frame_kp["x"][sel] - cx) * z / fx, (frame_kp["y"][sel] - cy) * z / fx, z], 1)
        dist = np.linalg.norm(pos, axis=1)
        p = np.zeros(n, capi.FUSE_POINT_DT)
        p["pos"], p["normal"] = pos, pos / dist[:, None]
        p["max_dist"] = dist * sf[frame_kp["octave"][sel]]
        p["min_dist_inv"] = 0.8 * p["max_dist"] / sf[-1]
        p["max_dist_inv"] = 1.2 * p["max_dist"]
        p["valid"] = rng.random(n) > 0.1                                 # a tenth NULL, bad or already found
        ang = np.mod(frame_kp["angle"][sel].astype(np.float64) + 25.0 * (i + 1) + rng.normal(0, 3.0, n), 360.0).astype(np.float32)
        ang[ang >= 360.0] = 0.0
        t = np.array([0.01 * (i % 7), 0.005 * (i % 3), -0.02 * (i % 5)], np.float32)
        pose = np.concatenate([np.eye(3, dtype=np.float32).reshape(9), t, -t]).astype(np.float32)
        occupied = (rng.random(len(frame_kp)) < 0.1).astype(np.uint8)
        return p, rec["descL"][sel].copy(), ang, pose, occupied

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
        fe.prof_enable(True)
        fe.prof_reset()
        for _ in range(a.calls):
            fn()
        rep = fe.prof_report()
        fe.prof_enable(False)
        return {k: round(rep[k][1] / rep[k][0], 4) for k in names if k in rep}

    ns = [int(k) for k in a.ncand.split(",")]
    cands_all = [candidate(i, a.points) for i in range(max(ns))]
    out = {"tool": "reloc_projection_timing", "frame_features": int(len(frame_kp)), "points_per_candidate": a.points,
           "calls": a.calls, "settings": {}}
    for th, orb_dist in SETTINGS:
        search = lambda cands: fe.search_by_projection_reloc(cands, frame_kp, frame_desc, cam, th, orb_dist, True)
        c0 = cands_all[0]
        sim3 = lambda n: fe.search_by_projection_sim3(c0[0], c0[1], [(frame_kp, frame_desc, c0[3], c0[4])] * n, cam, th,
                                                      orb_dist / 50.0)
        res = {"median_ms": {}, "single_calls_median_ms": {}, "matches_per_candidate": {}, "kernel_ms_per_call": {},
               "sim3_median_ms": {}, "sim3_kernel_ms_per_call": {}, "sim3_matches_per_pair": {}}
        for n in ns:
            cands = cands_all[:n]
            res["median_ms"][str(n)] = median_ms(lambda: search(cands))
            res["single_calls_median_ms"][str(n)] = median_ms(lambda: [search(cands[k:k + 1]) for k in range(n)])
            res["matches_per_candidate"][str(n)] = round(float(search(cands)[2].mean()), 1)
            res["kernel_ms_per_call"][str(n)] = kernel_split(lambda: search(cands), KERNELS)
            res["sim3_median_ms"][str(n)] = median_ms(lambda: sim3(n))
            res["sim3_kernel_ms_per_call"][str(n)] = kernel_split(lambda: sim3(n), SIM3_KERNELS)
            res["sim3_matches_per_pair"][str(n)] = round(float(sim3(n)[2].mean()), 1)
        out["settings"]["th%g_dist%d" % (th, orb_dist)] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    fe.close()


if __name__ == "__main__":
    main()
