#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_by_projection_two_cameras (ORBmatcher::SearchByProjection(CurrentFrame, LastFrame,
th, bMono) for a current frame of two cameras, ORBmatcher.cc:1961-2177, as Tracking::TrackWithMotionModel calls it: th = 15, and 30
for the retry :2969) on the ORB tables of a synthetic stereo sequence (752 x 480, 1200 features): the last frame's rows are the left
keypoints of frame 0 standing still (u, v = their position, the right projection shifted by their stereo disparity), the current
frame's two cameras are the left and right tables of frame 1.  The yardstick, in the same run on the same tables: two sequential
calls of the existing pli_search_by_projection, one per camera — what an integrator could call before; its answers are not the
reference's (no skip, two histograms), its work is the same.
Prints ONE JSON line and writes it to --out: per th the medians of --repeats series of --calls calls each (after --warmup calls) for
both, the kernels of one call (pli_prof_enable: HIP events around every launch) and the share of the two ordered walks
(k_proj2_assign, one launch, the walks side by side) in the call.  The host loop of the reference is not timed here.

  python tools/two_camera_projection_timing.py [--th 15,30] [--calls 50] [--repeats 5] [--warmup 10] [--out profiles/two_camera_projection_timing.json]
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
from pli_slam_amd.frontend import PROJ_QUERY_DT, Frontend  # noqa: E402

KERNELS = ("k_fill_f32", "k_proj2_candidates", "k_proj2_assign", "k_proj2_finish")
KERNELS_ONE = ("k_proj_candidates", "k_proj_assign")
BOUNDS = (0.0, 752.0, 0.0, 480.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--th", default="15,30")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_camera_projection_timing.json"))
    a = ap.parse_args()
    cfg = capi.default_config(752, 480, orb_nfeatures=1200)
    fe = Frontend(cfg, dev=False)
    last = fe.batch_run_host(np.stack(synth.make_stereo_pair(5, t=0))[None])[0]
    cur = fe.batch_run_host(np.stack(synth.make_stereo_pair(5, t=1))[None])[0]
    sf = np.float32(cfg.orb_scale_factor) ** np.arange(cfg.orb_nlevels, dtype=np.float32)
    kq, nq = last["kpL"], len(last["kpL"])
    disparity = np.where(last["uright"] >= 0, last["kpL"]["x"] - last["uright"], 10.0).astype(np.float32)
    out = {"tool": "two_camera_projection_timing", "calls": a.calls, "repeats": a.repeats, "nq": int(nq), "nleft": int(len(cur["kpL"])),
           "nright": int(len(cur["kpR"])), "th": {}}

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
        return {k: round(rep[k][1] / a.calls, 4) for k in names if k in rep}

    for th in [float(t) for t in a.th.split(",")]:
        ql = np.zeros(nq, PROJ_QUERY_DT)
        ql["u"], ql["v"] = kq["x"], kq["y"]
        ql["radius"] = (np.float32(th) * sf[kq["octave"]]).astype(np.float32)
        ql["min_level"], ql["max_level"] = kq["octave"] - 1, kq["octave"] + 1
        ql["angle"], ql["valid"] = kq["angle"], 1
        qr = ql.copy()
        qr["u"] = ql["u"] - disparity
        none_l, none_r = np.full(len(cur["kpL"]), -1, np.float32), np.full(len(cur["kpR"]), -1, np.float32)
        two = lambda: fe.search_by_projection_two_cameras(ql, qr, last["descL"], cur["kpL"], cur["descL"], cur["kpR"], cur["descR"],
                                                          BOUNDS, True, with_raw=True)

        def one_per_camera():
            a_ = fe.search_by_projection(ql, last["descL"], cur["kpL"], cur["descL"], none_l, BOUNDS, True, with_raw=True)
            b_ = fe.search_by_projection(qr, last["descL"], cur["kpR"], cur["descR"], none_r, BOUNDS, True, with_raw=True)
            return a_, b_
        n, bl, br, rl, rr = two()
        (n1, _, _), (n2, _, _) = one_per_camera()
        res = {"matches": int(n), "accepts_left": int((rl >= 0).sum()), "accepts_right": int((rr >= 0).sum()),
               "two_calls_matches": int(n1 + n2)}
        # interleaved series, so that a drift of the box shows in both
        res["median_ms"], res["two_calls_median_ms"] = [], []
        for _ in range(a.repeats):
            res["median_ms"].append(median_ms(two))
            res["two_calls_median_ms"].append(median_ms(one_per_camera))
        ks = kernel_split(two, KERNELS)
        res["kernel_ms_per_call"] = ks
        res["two_calls_kernel_ms"] = kernel_split(one_per_camera, KERNELS_ONE)
        if "k_proj2_assign" in ks:
            res["walk_share_of_kernels"] = round(ks["k_proj2_assign"] / sum(ks.values()), 3)
            res["walk_share_of_call"] = round(ks["k_proj2_assign"] / float(np.median(res["median_ms"])), 3)
        out["th"]["%g" % th] = res
    fe.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
