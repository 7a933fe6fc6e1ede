#!/usr/bin/env python3
"""GPU box: host-inclusive latency of the two searches for a rig of two KannalaBrandt8 cameras, through the Python mirror.

  pli_fuse_search_two_cameras     (ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight), both values of bRight of nkf keyframes in one
      call): 2000 map points seen from a reference view against keyframes of about 1200 + 1200 keypoints (the points' projections
      through each camera with pixel noise, descriptors a few bits away, and decoys).  In the same run, interleaved: the same
      tables through pli_fuse_search, once per side (the side's rows, its pose, a pinhole camera of the same focal length, no
      stereo rows) - the same amount of work, NOT the reference's answers.
  pli_search_by_bow_two_cameras   (ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches), F.Nleft != -1, nkf keyframes in one call):
      the left and the right image of a synthetic stereo frame (752 x 480) through pli_orb_extract as the frame's two cameras,
      the other frames of the sequence as keyframes, FeatureVectors from a synthetic DBoW2 vocabulary (k = 10, L = 4, levelsup
      2), four fifths of the keyframe features holding map points.  Interleaved: the same tables through pli_search_by_bow.

Medians of --calls calls, --repeats series; under HIP events (pli_prof_enable) the kernels of one call and the launches per call.
Prints one JSON line per search and writes them to --out-fuse / --out-bow.  No host loop of the reference is timed here.

  python tools/two_cameras_fuse_bow_timing.py [--nkf 1,6,12] [--calls 50] [--repeats 5] [--warmup 10]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pli_slam_amd import capi, synth  # noqa: E402
from pli_slam_amd.frontend import Frontend, predict_scale  # noqa: E402

W, H = 752, 480
# TUM-VI's distortion coefficients around the centre of a 752 x 480 image
CAM_LEFT = [250.0, 250.0, 376.0, 240.0, 0.00348238940, 0.000715034845, -0.00205323614, 0.000202936736]
CAM_RIGHT = [249.3, 249.3, 374.0, 238.5, 0.00340031805, 0.00176627874, -0.00266312161, 0.000329951911]
BOUNDS = (0.0, float(W), 0.0, float(H))


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def kb8_project(cam, P):
    fx, fy, cx, cy, k0, k1, k2, k3 = cam
    rho = np.hypot(P[:, 0], P[:, 1])
    th = np.arctan2(rho, P[:, 2])
    t2 = th * th
    r = th * (1 + t2 * (k0 + t2 * (k1 + t2 * (k2 + t2 * k3))))
    rho = np.where(rho > 0, rho, 1.0)
    return fx * r * P[:, 0] / rho + cx, fy * r * P[:, 1] / rho + cy


def pose15(R, t):
    return np.concatenate([R.reshape(9), t, -R.T @ t]).astype(np.float32)


def fuse_workload(rng, nmp, nkf, nfeat, nlevels, scale):
    sf = scale ** np.arange(nlevels)
    d = np.stack([rng.uniform(-1.2, 1.2, nmp), rng.uniform(-0.8, 0.8, nmp), np.ones(nmp)], 1)
    pos = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(2.0, 15.0, nmp)[:, None]
    dist = np.linalg.norm(pos, axis=1)
    pts = np.zeros(nmp, capi.FUSE_POINT_DT)
    max_d = dist * sf[rng.integers(0, nlevels, nmp)]
    pts["pos"], pts["normal"] = pos, pos / dist[:, None]
    pts["max_dist"], pts["min_dist_inv"], pts["max_dist_inv"], pts["valid"] = max_d, 0.8 * max_d / sf[-1], 1.2 * max_d, 1
    descs = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
    Rrl = rot(0.0, np.deg2rad(2.0), 0.0)
    tlr = np.array([0.101, 0.002, -0.001])
    kfs = []
    for _ in range(nkf):
        R, t = rot(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.3, 0.3, 3)
        sides = [(R, t), (Rrl @ R, Rrl @ t - Rrl @ tlr)]
        rows = []
        for (Rs, ts), cam in zip(sides, (CAM_LEFT, CAM_RIGHT)):
            pc = pos @ Rs.T + ts
            u, v = kb8_project(cam, pc)
            vis = rng.permutation(np.nonzero((pc[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H))[0])[:int(nfeat * 0.6)]
            kp = np.zeros(nfeat, capi.KEYPOINT_DT)
            kd = rng.integers(0, 256, (nfeat, 32), dtype=np.uint8)
            kp["x"], kp["y"] = rng.uniform(0, W, nfeat), rng.uniform(0, H, nfeat)
            kp["octave"], kp["size"] = rng.integers(0, nlevels, nfeat), 31.0
            m = len(vis)
            kp["x"][:m], kp["y"][:m] = u[vis] + rng.normal(0, 0.8, m), v[vis] + rng.normal(0, 0.8, m)
            centre = -Rs.T @ ts
            kp["octave"][:m] = [predict_scale(float(np.float32(max_d[i] / np.linalg.norm(pos[i] - centre))), nlevels, scale) for i in vis]
            kd[:m] = descs[vis]
            for j in range(m):
                for b in rng.integers(0, 256, int(rng.integers(0, 12))):
                    kd[j, b >> 3] ^= np.uint8(1 << (b & 7))
            order = rng.permutation(nfeat)
            rows.append((kp[order], kd[order]))
        kfs.append((np.concatenate([rows[0][0], rows[1][0]]), np.concatenate([rows[0][1], rows[1][1]]), nfeat,
                    np.stack([pose15(*sides[0]), pose15(*sides[1])])))
    return pts, descs, kfs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nkf", default="1,6,12")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nmp", type=int, default=2000)
    ap.add_argument("--out-fuse", default=os.path.join(ROOT, "profiles", "fuse_two_cameras_timing.json"))
    ap.add_argument("--out-bow", default=os.path.join(ROOT, "profiles", "bow_two_cameras_timing.json"))
    a = ap.parse_args()
    fe = Frontend(capi.default_config(W, H, orb_nfeatures=1200), dev=False)
    ns = [int(k) for k in a.nkf.split(",")]
    rng = np.random.default_rng(0)

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
        """-> (ms per call by kernel, launches per call)"""
        fe.prof_enable(True)
        fe.prof_reset()
        for _ in range(a.calls):
            fn()
        rep = fe.prof_report()
        fe.prof_enable(False)
        return {k: round(v[1] / a.calls, 4) for k, v in rep.items()}, sum(v[0] for v in rep.values()) / a.calls

    def series(res, fns):
        for _ in range(a.repeats):                 # interleaved series, so that a drift of the box shows in all of them
            for name, fn in fns:
                res.setdefault(name, []).append(median_ms(fn))

    def write(out, path):
        line = json.dumps(out)
        print(line)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(line + "\n")

    # ---- Fuse ----
    pts, descs, pool = fuse_workload(rng, a.nmp, max(ns), 1200, fe.cfg.orb_nlevels, fe.cfg.orb_scale_factor)
    out = {"tool": "two_cameras_fuse_bow_timing", "search": "fuse", "calls": a.calls, "repeats": a.repeats, "nmp": a.nmp,
           "kf_features": int(len(pool[0][0])), "kf_nleft": int(pool[0][2]), "nkf": {}}
    pin = [capi.FuseCamera(*(c[:4] + [0.0] + list(BOUNDS))) for c in (CAM_LEFT, CAM_RIGHT)]
    for nkf in ns:
        kfs = pool[:nkf]
        side_kfs = [[(kp[:nl] if s == 0 else kp[nl:], kd[:nl] if s == 0 else kd[nl:],
                      np.full(nl if s == 0 else len(kp) - nl, -1.0, np.float32), pose[s]) for kp, kd, nl, pose in kfs] for s in (0, 1)]
        batch = lambda: fe.fuse_search_two_cameras(pts, descs, kfs, CAM_LEFT, CAM_RIGHT, BOUNDS)
        singles = lambda: [fe.fuse_search_two_cameras(pts, descs, kfs[k:k + 1], CAM_LEFT, CAM_RIGHT, BOUNDS, sides=s)
                           for k in range(nkf) for s in (1, 2)]
        yard = lambda: [fe.fuse_search(pts, descs, side_kfs[s], pin[s]) for s in (0, 1)]
        res = {"matches_per_kf": round(float((batch()[0] >= 0).sum()) / nkf, 1),
               "one_camera_matches_per_kf": round(float(sum((r[0] >= 0).sum() for r in yard())) / nkf, 1)}
        series(res, (("median_ms", batch), ("single_calls_per_keyframe_and_side_median_ms", singles),
                     ("one_camera_call_per_side_median_ms", yard)))
        res["kernel_ms_per_call"], res["launches_per_call"] = kernel_split(batch)
        res["one_camera_kernel_ms_both_sides"], res["one_camera_launches_both_sides"] = kernel_split(yard)
        out["nkf"][str(nkf)] = res
    write(out, a.out_fuse)

    # ---- SearchByBoW ----
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))

    def tables(t):
        """(desc, angle, node, nleft): the left image's features, then the right image's."""
        parts = []
        for img in synth.make_stereo_pair(5, t=t):
            n, kp, desc = fe.orb_extract(0, img)
            parts.append((kp[:n].copy(), desc[:n].copy()))
        kp, desc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return desc, kp["angle"].astype(np.float32), np.where(weight > 0, node, -1).astype(np.int32), len(parts[0][0])

    fd, fa, fn, nleft = tables(0)
    kpool = []
    for t in range(1, max(ns) + 1):
        kd, ka, kn, _ = tables(t)
        kpool.append((kd, ka, kn, (rng.random(len(kn)) < 0.8).astype(np.uint8)))
    out = {"tool": "two_cameras_fuse_bow_timing", "search": "bow", "calls": a.calls, "repeats": a.repeats, "nf": int(len(fn)),
           "f_nleft": int(nleft), "kf_features": int(np.mean([len(k[2]) for k in kpool])), "nkf": {}}
    for nkf in ns:
        kfs = kpool[:nkf]
        batch = lambda: fe.search_by_bow_two_cameras(kfs, fd, fa, fn, nleft)
        singles = lambda: [fe.search_by_bow_two_cameras(kfs[k:k + 1], fd, fa, fn, nleft) for k in range(nkf)]
        yard = lambda: fe.search_by_bow(fd, fa, fn, kfs, nnratio=0.7)
        res = {"matches_per_kf": round(float(batch()[1].mean()), 1), "one_camera_matches_per_kf": round(float(yard()[1].mean()), 1)}
        series(res, (("median_ms", batch), ("single_calls_median_ms", singles), ("one_camera_median_ms", yard)))
        res["kernel_ms_per_call"], res["launches_per_call"] = kernel_split(batch)
        res["one_camera_kernel_ms_per_call"], res["one_camera_launches_per_call"] = kernel_split(yard)
        out["nkf"][str(nkf)] = res
    write(out, a.out_bow)
    fe.vocab_destroy(voc)
    fe.close()


if __name__ == "__main__":
    main()
