#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_create_new_map_points_two_cameras (LocalMapping::CreateNewMapPoints from the search on for
keyframes of two KannalaBrandt8 cameras, one keyframe against nkf neighbours in one call) and, in the same run on the same tables,
of pli_search_for_triangulation_two_cameras alone; the difference is the cost of the list, the geometry and the pick (and of the
larger upload and download, and of k_kb8_rays where the search skips it).  Tables and poses as
tools/triangulation_two_cameras_timing.py: keyframes of about 1200 + 1200 features, a rig that moves sideways.
Five interleaved series: every series takes the median of --calls calls of each form, per nkf.  The launches per call come from
HIP events (pli_prof_enable).  No host loop of the reference is timed here, so nothing is said about a speed-up over it.
Writes ONE JSON object to --out and prints it.

  python tools/new_map_points_two_cameras_timing.py [--nkf 1,10,20] [--calls 50] [--repeats 5] [--warmup 10]
                                                    [--out profiles/new_map_points_two_cameras_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pli_slam_amd import capi, synth  # noqa: E402
from pli_slam_amd.frontend import Frontend  # noqa: E402
from triangulation_two_cameras_timing import CAM_LEFT, CAM_RIGHT, pose, relative_poses, rot  # noqa: E402


def pose30(T, Tlr):
    """Left then right side of a keyframe: Rcw row major, tcw, Ow."""
    out = np.zeros((2, 15), np.float32)
    for s, Tc in enumerate((T, np.linalg.inv(Tlr) @ T)):
        out[s, :9], out[s, 9:12], out[s, 12:] = Tc[:3, :3].reshape(9), Tc[:3, 3], np.linalg.inv(Tc)[:3, 3]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nkf", default="1,10,20")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_map_points_two_cameras_timing.json"))
    a = ap.parse_args()
    fe = Frontend(capi.default_config(752, 480, orb_nfeatures=1200), dev=False)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))
    rng = np.random.default_rng(0)
    Tlr = pose(rot(0.0, np.deg2rad(2.0), 0.0).T, (0.0, 0.0, 0.0))
    Tlr[:3, 3] = (0.101, 0.002, -0.001)
    T1 = pose(np.eye(3), (0.0, 0.0, 0.0))
    ratio_factor = float(np.float32(np.float32(1.5) * np.float32(1.2)))

    def keyframe(t, T):
        """(kp, desc, node, has_mp, nleft, pose[2, 15]): the left image's features, then the right image's."""
        parts = []
        for img in synth.make_stereo_pair(5, t=t):
            n, kp, desc = fe.orb_extract(0, img)
            parts.append((kp[:n].copy(), desc[:n].copy()))
        kp, desc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return (kp, desc, np.where(weight > 0, node, -1).astype(np.int32), (rng.random(len(kp)) < 0.2).astype(np.uint8), len(parts[0][0]),
                pose30(T, Tlr))

    ns = [int(k) for k in a.nkf.split(",")]
    kf1 = keyframe(0, T1)
    pool = []
    for t in range(1, 11):
        T2 = pose(rot(0.0, 0.0, 0.0087 * t), (-0.04 * t, -0.013 * t, 0.0))
        pool.append(keyframe(t, T2) + (relative_poses(T1, T2, Tlr),))
    kfs_all = [pool[i % len(pool)] for i in range(max(ns))]
    search_of = lambda kf: kf[:5] + kf[6:]

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 4)

    out = {"tool": "new_map_points_two_cameras_timing", "calls": a.calls, "repeats": a.repeats, "n1": int(len(kf1[2])),
           "n1_left": int(kf1[4]), "kf_features": int(np.mean([len(k[2]) for k in kfs_all])), "nkf": {}}
    for nkf in ns:
        kfs = kfs_all[:nkf]
        skfs = [search_of(kf) for kf in kfs]
        new = lambda: fe.create_new_map_points_two_cameras(kf1, kfs, CAM_LEFT, CAM_RIGHT, ratio_factor)
        search = lambda: fe.search_for_triangulation_two_cameras(kf1[:5], skfs, CAM_LEFT, CAM_RIGHT)
        res = {"create_new_map_points_median_ms": [], "search_for_triangulation_median_ms": []}
        for _ in range(a.repeats):                 # interleaved series, so that a drift of the box shows in both
            res["create_new_map_points_median_ms"].append(median_ms(new))
            res["search_for_triangulation_median_ms"].append(median_ms(search))
        res["geometry_and_pick_ms"] = round(float(np.median(res["create_new_map_points_median_ms"])) -
                                            float(np.median(res["search_for_triangulation_median_ms"])), 4)
        _, n, status, _, nnew = new()
        res["pairs_on_entry_per_kf"] = round(float(search()[1].mean()), 1)
        res["matches_per_kf"] = round(float(n.mean()), 1)
        res["created_per_kf"] = round(float(nnew.mean()), 1)
        fe.prof_enable(True)
        fe.prof_reset()
        new()
        rep = fe.prof_report()
        fe.prof_enable(False)
        res["launches_per_call"] = int(sum(v[0] for v in rep.values()))
        res["kernel_ms_per_call"] = {k: round(v[1], 4) for k, v in rep.items()}
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
