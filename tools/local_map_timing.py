#!/usr/bin/env python3
"""GPU box: host-inclusive latency of pli_search_local_points and pli_search_local_lines (Tracking.cc:3809-3883 for a frame of one
camera) against the path an integrator had before them, in the same run on the same tables:

  points  old: Frame::isInFrustum and the queries of ORBmatcher.cc:53-73 on the host, then pli_search_local_map (queries uploaded)
          new: pli_search_local_points (world points uploaded, projection and queries on the device)
  lines   old: Frame::isInFrustum_l and the in-view list on the host, the descriptors gathered, then pli_match_nnr
          new: pli_search_local_lines

The host side of the old path is the adapter's expressions vectorised in numpy (float32 arrays, the sums in float64): it is NOT the
reference's scalar C++ loop, which is not timed here, so the numbers compare two ways of calling this library from one host
program and say nothing about the reference's CPU time.  Shapes: 1200 keypoints against 1000, 4000 and 10000 local points; 100
frame lines against 200 and 1000 map lines.  Per shape: --repeats series, old and new interleaved, each the median of --calls calls
after --warmup calls.  Prints ONE JSON line and writes it to --out.

  python tools/local_map_timing.py [--calls 50] [--repeats 5] [--warmup 10] [--out profiles/local_map_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pli_slam_amd import capi  # noqa: E402
from pli_slam_amd.frontend import PROJ_QUERY_DT, Frontend  # noqa: E402

CAM = tuple(np.float32(v) for v in (435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297, 47.90639384423901,
                                    0.0, 752.0, 0.0, 480.0))
BOUNDS = CAM[5:]
f32, f64 = np.float32, np.float64


def pose_of(rng):
    a, b, c = rng.uniform(-0.2, 0.2, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    R, t = Rz @ Ry @ Rx, rng.uniform(-1, 1, 3)
    return np.concatenate([R.reshape(-1), t, -R.T @ t]).astype(f32)


def world(pose, u, v, z):
    R, t = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64)
    pc = np.stack([(u - float(CAM[2])) * z / float(CAM[0]), (v - float(CAM[3])) * z / float(CAM[1]), z], -1)
    return (pc - t) @ R


def point_tables(rng, pose, nq, ncur, nlevels):
    u, v = rng.uniform(-60, 812, nq), rng.uniform(-60, 540, nq)
    z = rng.uniform(0.5, 20.0, nq) * np.where(rng.random(nq) < 1 / 16, -1.0, 1.0)
    pw = world(pose, u, v, z)
    po = pw - pose[12:15].astype(f64)
    dist = np.linalg.norm(po, axis=1)
    pts = np.zeros(nq, capi.FUSE_POINT_DT)
    pts["pos"], pts["normal"] = pw, po / dist[:, None]
    pts["max_dist"] = dist * 1.2 ** (rng.integers(0, nlevels, nq) - 0.5)
    pts["max_dist_inv"], pts["min_dist_inv"] = 1.2 * pts["max_dist"], 0.2 * pts["max_dist"]
    pts["valid"] = rng.random(nq) < 0.93
    descs = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    inside = np.flatnonzero((u > 0) & (u < 752) & (v > 0) & (v < 480) & (z > 0))
    src = inside[rng.integers(0, len(inside), ncur)]
    kp = np.zeros(ncur, capi.KEYPOINT_DT)
    kp["x"], kp["y"] = np.clip(u[src] + rng.uniform(-4, 4, ncur), 0, 751), np.clip(v[src] + rng.uniform(-4, 4, ncur), 0, 479)
    kp["octave"] = rng.integers(0, nlevels, ncur)
    desc = descs[src].copy()
    flip = rng.random((ncur, 32)) < 0.08
    desc[flip] ^= rng.integers(1, 256, (ncur, 32), dtype=np.uint8)[flip]
    ur = np.where(rng.random(ncur) < 0.5, kp["x"] - float(CAM[4]) / z[src], -1.0).astype(f32)
    return pts, descs, kp, np.ascontiguousarray(desc), ur


def camera_points(pose, p):
    R, t = pose[:9].reshape(3, 3), pose[9:12]
    return (p.astype(f64) @ R.astype(f64).T + t.astype(f64)).astype(f32)


def host_point_queries(pts, pose, lr, sf, th):
    """Frame::isInFrustum and ORBmatcher.cc:53-73 for every point, vectorised (the adapter's expressions on arrays)."""
    with np.errstate(all="ignore"):
        pc = camera_points(pose, pts["pos"])
        depth = np.sqrt((pc.astype(f64) ** 2).sum(1)).astype(f32)
        z = pc[:, 2]
        invz = f32(1.0) / z
        u, v = CAM[0] * pc[:, 0] / z + CAM[2], CAM[1] * pc[:, 1] / z + CAM[3]
        po = pts["pos"] - pose[12:15]
        dist = np.sqrt((po.astype(f64) ** 2).sum(1)).astype(f32)
        cos = ((po.astype(f64) * pts["normal"].astype(f64)).sum(1) / dist).astype(f32)
        ok = ((pts["valid"] != 0) & ~(z < 0) & ~((u < CAM[5]) | (u > CAM[6])) & ~((v < CAM[7]) | (v > CAM[8])) &
              ~((dist < pts["min_dist_inv"]) | (dist > pts["max_dist_inv"])) & ~(cos < f32(0.5)))
        level = (((pts["max_dist"] / dist)[:, None] > lr[None, :]).sum(1)).astype(np.int32)
        r = np.where(cos.astype(f64) > 0.998, f32(2.5), f32(4.0)).astype(f32)
        if th != 1.0:
            r = r * f32(th)
        q = np.zeros(len(pts), PROJ_QUERY_DT)
        q["u"], q["v"], q["ur"] = u, v, u - CAM[4] * invz
        q["radius"] = r * sf[level]
        q["min_level"], q["max_level"], q["valid"] = level - 1, level, ok
    return q, depth


def host_line_list(sp, valid, pose):
    with np.errstate(all="ignore"):
        pc = camera_points(pose, sp)
        invz = f32(1.0) / pc[:, 2]
        u, v = CAM[0] * pc[:, 0] * invz + CAM[2], CAM[1] * pc[:, 1] * invz + CAM[3]
        ok = (valid != 0) & ~(pc[:, 2] < 0) & ~((u < CAM[5]) | (u > CAM[6])) & ~((v < CAM[7]) | (v > CAM[8]))
    return np.flatnonzero(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_timing.json"))
    a = ap.parse_args()
    cfg = capi.default_config(752, 480, orb_nfeatures=1200)
    fe = Frontend(cfg, dev=False)
    nlevels = cfg.orb_nlevels
    lr = fe._level_ratio(None)
    sf = (f32(cfg.orb_scale_factor) ** np.arange(nlevels, dtype=f32)).astype(f32)
    rng = np.random.default_rng(17)
    pose = pose_of(rng)

    def series(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def compare(old, new):
        to, tn = [], []
        for _ in range(a.repeats):                      # interleaved
            to.append(series(old))
            tn.append(series(new))
        return {"old_ms": round(float(np.median(to)), 4), "new_ms": round(float(np.median(tn)), 4),
                "old_series_ms": [round(t, 4) for t in to], "new_series_ms": [round(t, 4) for t in tn],
                "new_over_old": round(float(np.median(tn) / np.median(to)), 3)}

    out = {"tool": "local_map_timing", "calls": a.calls, "repeats": a.repeats, "warmup": a.warmup,
           "host_side_of_old_path": "numpy, vectorised; not the reference's C++ loop", "points": {}, "lines": {}}
    for nq in (1000, 4000, 10000):
        pts, descs, kp, desc, ur = point_tables(rng, pose, nq, 1200, nlevels)

        def old():
            q, _ = host_point_queries(pts, pose, lr, sf, 1.0)
            return fe.search_local_map(q, descs, kp, desc, ur, BOUNDS, 0.8)

        def new():
            return fe.search_local_points(pts, descs, pose, CAM, kp, desc, ur, th=1.0, level_ratio=lr)
        n_old, n_new = old()[0], new()[3]
        r = compare(old, new)
        r.update(ncur=1200, in_view=int(new()[2]), matches_old=int(n_old), matches_new=int(n_new))
        out["points"][str(nq)] = r
    for nl in (200, 1000):
        u, v = rng.uniform(-80, 832, nl), rng.uniform(-80, 560, nl)
        sp = world(pose, u, v, rng.uniform(0.5, 20.0, nl)).astype(f32)
        valid = (rng.random(nl) < 0.9).astype(np.uint8)
        descs = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
        cur = descs[rng.integers(0, nl, 100)].copy()
        cur[:, :2] ^= rng.integers(0, 256, (100, 2), dtype=np.uint8)

        def old():
            lst = host_line_list(sp, valid, pose)
            return fe.match_nnr(descs[lst], cur, 0.9)

        def new():
            return fe.search_local_lines(sp, valid, descs, pose, CAM, cur, 0.9)
        r = compare(old, new)
        r.update(n2=100, in_view=int(len(new()[2])), matches_old=int(old()[0]), matches_new=int(new()[4]))
        out["lines"][str(nl)] = r
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
