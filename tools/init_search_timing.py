#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_for_initialization (monocular initialisation's
ORBmatcher::SearchForInitialization, ORBmatcher.cc:706-821, as Tracking.cc:2109-2110 calls it: ratio 0.9, orientation check,
window 100) on the ORB tables of a synthetic sequence (752 x 480, EuRoC defaults): F1 = the left image of frame 0, F2 = that of
frame 1, vbPrevMatched = F1's points.  Two table sizes: the default extractor's (nFeatures) and that of the monocular initial
extractor, which Tracking's constructor creates with 5 * nFeatures (Tracking.cc:749).  The device extractor's per-level quota
stops below 5 * nFeatures, so the larger tables are put together from the tables of `mult` scenes of the sequence (seeds 5, 6, ..),
frame by frame: the sizes, the octave mix and the true matches are those of extracted tables, the scenes overlap in the image.
Prints ONE JSON line and writes it to --out: per size the median over --calls calls after --warmup calls through
Frontend.search_for_initialization, the same for the second call of a chain (vbPrevMatched as the first call left it, against
frame 2), the kernels of one call (pli_prof_enable: HIP events around every launch) and the share of the ordered walk
(k_init_assign) in the kernels' sum and in the call.  The host loop of the reference is not timed here.

  python tools/init_search_timing.py [--mult 1,5] [--window 100] [--calls 50] [--warmup 10] [--out profiles/init_search_timing.json]
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

KERNELS = ("k_fuse_grid", "k_init_candidates", "k_init_assign")
BOUNDS = (0.0, 752.0, 0.0, 480.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mult", default="1,5")
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_search_timing.json"))
    a = ap.parse_args()
    nfeatures = int(capi.default_config(752, 480).orb_nfeatures)
    out = {"tool": "init_search_timing", "window": a.window, "nnratio": 0.9, "calls": a.calls, "sizes": {}}
    fe = Frontend(capi.default_config(752, 480), dev=False)
    for mult in [int(m) for m in a.mult.split(",")]:
        tabs = []
        for t in range(3):
            recs = [fe.batch_run_host(np.stack(synth.make_stereo_pair(5 + s, t=t))[None])[0] for s in range(mult)]
            tabs.append((np.concatenate([r["kpL"] for r in recs]), np.concatenate([r["descL"] for r in recs])))
        (k1, d1), (k2, d2), (k3, d3) = tabs
        prev0 = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)

        def median_ms(fn):
            for _ in range(a.warmup):
                fn()
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(ts)), 4)

        def kernel_split(fn):
            fe.prof_enable(True)
            fe.prof_reset()
            for _ in range(a.calls):
                fn()
            rep = fe.prof_report()
            fe.prof_enable(False)
            return {k: round(rep[k][1] / rep[k][0], 4) for k in KERNELS if k in rep}

        first = lambda: fe.search_for_initialization(k1, d1, prev0, k2, d2, BOUNDS, a.window, 0.9, True)
        nm, m12, raw, prev1 = first()
        second = lambda: fe.search_for_initialization(k1, d1, prev1, k3, d3, BOUNDS, a.window, 0.9, True)
        res = {"nfeatures": mult * nfeatures, "n1": int(len(k1)), "n2": int(len(k2)), "n1_octave0": int((k1["octave"] == 0).sum()),
               "n2_octave0": int((k2["octave"] == 0).sum()), "matches_after_walk": int((raw >= 0).sum()), "matches": int(nm),
               "second_call_matches": int(second()[0])}
        res["median_ms"] = median_ms(first)
        res["second_call_median_ms"] = median_ms(second)
        ks = kernel_split(first)
        res["kernel_ms_per_call"] = ks
        if "k_init_assign" in ks:
            res["walk_share_of_kernels"] = round(ks["k_init_assign"] / sum(ks.values()), 3)
            res["walk_share_of_call"] = round(ks["k_init_assign"] / res["median_ms"], 3)
        out["sizes"]["x%d" % mult] = res
    fe.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
