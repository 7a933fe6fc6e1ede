"""The C++ adapter for frames of two cameras, executed (-m gpu): tests/cpp/two_camera_search_harness.cpp runs the two members that
PliORBmatcherTwoCameras hides — SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1961-2177, Tracking.cc:2961)
for a forward, a backward and a sideways motion, and SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints)
(ORBmatcher.cc:44-214, Tracking.cc:3854) — on stub Frame / MapPoint types with a second camera: mvpMapPoints partly filled at entry
with and without observations, outliers, rows without a map point, points behind the camera, bad points, points out of view,
last-frame rows of either camera.  The containers equal the restatements: two_camera_scalar of
tests/test_two_camera_projection_cpu.py and local_map_two_cameras below, which the CPU oracle confirms.  The projections are
restated in numpy float32 by the stub cv::Mat's definition of a product (one gemm: products and sum in double, one rounding)."""
import os
import subprocess

import numpy as np
import pytest

from helpers_matchers import KEYPOINT_DT, PROJ_QUERY_DT, TH_HIGH, _area, _cells, hamming
from test_fuse_search_cpu import gemm_row
from test_two_camera_projection_cpu import NO_OBS, two_camera_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
f32, f64 = np.float32, np.float64
BOUNDS = (0.0, 752.0, 0.0, 480.0)
CAM = (f32(458.0), f32(457.0), f32(367.0), f32(248.0))
TH_TRACK, TH_LOCAL, TH_FAR, MB = 15.0, 3.0, 50.0, f32(0.1)
NNRATIO_LOCAL = 0.8
POINT_DT = np.dtype([("in_view", "<i4"), ("in_view_r", "<i4"), ("bad", "<i4"), ("nobs", "<i4"), ("level", "<i4"), ("level_r", "<i4"),
                     ("depth", "<f4"), ("view_cos", "<f4"), ("view_cos_r", "<f4"), ("proj_x", "<f4"), ("proj_y", "<f4"),
                     ("proj_xr", "<f4"), ("proj_yr", "<f4"), ("pos", "<f4", (3,)), ("desc", "u1", (32,))])


def build(outdir):
    exe = os.path.join(outdir, "two_camera_search_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "two_camera_search_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def scale_factors(n=8):
    sf = [f32(1.0)]
    for _ in range(n - 1):
        sf.append(f32(sf[-1] * f32(1.2)))
    return np.array(sf, f32)


def pose(rz, t):
    T = np.eye(4, dtype=f32)
    c, s = np.cos(rz), np.sin(rz)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], f32)
    T[:3, 3] = t
    return T


def transform(R, t, p):
    """R * p + t as the stub cv::Mat evaluates it: one gemm"""
    return np.array([gemm_row(R[r], p, t[r]) for r in range(3)], f32)


def project(p):
    """the harness's Camera::project, one float operation per step"""
    fx, fy, cx, cy = CAM
    xn, yn = f32(p[0] / p[2]), f32(p[1] / p[2])
    return f32(f32(fx * xn) + cx), f32(f32(fy * yn) + cy)


def flip_bits(rng, desc, nbits):
    bits = np.unpackbits(desc)
    bits[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits)


def make_world(rng, nlast=320, nl=300, nr=260, nmp=340):
    """One pool of map points seen by a rig of two cameras.  The current frame's keypoints are projections of pool points (plus
    clutter); the last frame's rows point into the pool, rows of its right camera included."""
    Trl = np.zeros((3, 4), f32)
    Trl[:3, :3] = pose(0.004, 0)[:3, :3]
    Trl[:, 3] = (-0.11, 0.002, 0.001)
    poses = [pose(0.003, (0.02, -0.01, -0.5)), pose(-0.002, (-0.03, 0.01, 0.5)), pose(0.002, (0.015, -0.02, 0.01))]   # forward, backward, neither
    last_T = np.eye(4, dtype=f32)
    # pool points in world coordinates (the last camera's): in front of the rig, a tenth behind it
    pool = np.zeros(nmp, POINT_DT)
    z = rng.uniform(3, 12, nmp)
    z[rng.random(nmp) < 0.1] *= -1
    pool["pos"] = np.stack([rng.uniform(-0.7, 0.7, nmp) * np.abs(z), rng.uniform(-0.45, 0.45, nmp) * np.abs(z), z], 1).astype(f32)
    pool["desc"] = rng.integers(0, 256, (nmp, 32), dtype=np.uint8)
    level = rng.integers(0, 6, nmp)
    # the current frame's keypoints: where the sideways pose sees the points, a few pixels off
    Rcw, tcw = poses[2][:3, :3], poses[2][:3, 3]

    def camera(n, right):
        kp = np.zeros(n, KEYPOINT_DT)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        owner = np.full(n, -1, np.int64)
        src = rng.permutation(nmp)
        k = 0
        for p in src:
            if k >= int(0.8 * n):
                break
            x = transform(Rcw, tcw, pool["pos"][p])
            if right:
                x = transform(Trl[:, :3], Trl[:, 3], x)
            if x[2] <= 0.5:
                continue
            u, v = project(x)
            if not (5 < u < 745 and 5 < v < 475):
                continue
            kp["x"][k], kp["y"][k] = u + rng.uniform(-3, 3), v + rng.uniform(-3, 3)
            kp["octave"][k] = level[p] + rng.integers(-1, 2)
            desc[k] = flip_bits(rng, pool["desc"][p], int(rng.integers(0, 110)))
            owner[k] = p
            k += 1
        kp["x"][k:] = rng.uniform(0, 752, n - k); kp["y"][k:] = rng.uniform(0, 480, n - k); kp["octave"][k:] = rng.integers(0, 8, n - k)
        kp["octave"] = np.clip(kp["octave"], 0, 7)
        kp["angle"] = rng.choice(np.array([10.0, 10.0, 10.0, 100.0, 220.0], f32), n)
        kp["size"] = 31
        order = rng.permutation(n)
        return kp[order], desc[order], owner[order]
    kl, dl, own_l = camera(nl, False)
    kr, dr, own_r = camera(nr, True)
    # stereo partners: keypoints of one point, half of them
    l2r, r2l = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
    right_of = {int(p): k for k, p in enumerate(own_r) if p >= 0}
    for k, p in enumerate(own_l):
        if p >= 0 and int(p) in right_of and rng.random() < 0.5:
            l2r[k], r2l[right_of[int(p)]] = right_of[int(p)], k
    # the local map's view of the pool
    left_of = {int(p): k for k, p in enumerate(own_l) if p >= 0}
    for p in range(nmp):
        a, b = left_of.get(p), right_of.get(p)
        pool["proj_x"][p], pool["proj_y"][p] = (kl["x"][a], kl["y"][a]) if a is not None else (rng.uniform(0, 752), rng.uniform(0, 480))
        pool["proj_xr"][p], pool["proj_yr"][p] = (kr["x"][b], kr["y"][b]) if b is not None else (rng.uniform(0, 752), rng.uniform(0, 480))
        pool["level"][p] = kl["octave"][a] + (rng.random() < 0.4) if a is not None else level[p]
        pool["level_r"][p] = kr["octave"][b] + (rng.random() < 0.4) if b is not None else level[p]
    for f in ("proj_x", "proj_y", "proj_xr", "proj_yr"):
        pool[f] += rng.uniform(-2.5, 2.5, nmp).astype(f32)
    pool["level"], pool["level_r"] = np.clip(pool["level"], 0, 7), np.clip(pool["level_r"], 0, 7)
    pool["level_r"][rng.random(nmp) < 0.1] = -1
    pool["in_view"], pool["in_view_r"] = rng.random(nmp) < 0.8, rng.random(nmp) < 0.7
    pool["bad"] = rng.random(nmp) < 0.1
    pool["depth"] = rng.uniform(1, 70, nmp)
    pool["view_cos"], pool["view_cos_r"] = rng.uniform(0.995, 1.0, nmp), rng.uniform(0.995, 1.0, nmp)
    searching = (pool["bad"] == 0) & ((pool["in_view"] != 0) | ((pool["in_view_r"] != 0) & (pool["level_r"] != -1)))
    pool["nobs"] = np.where(searching, rng.integers(1, 5, nmp), rng.integers(0, 3, nmp))       # (a searching point has observations)
    lonely = np.flatnonzero(pool["nobs"] == 0)                                               # a quarter of the held slots: no observations
    held = np.where(rng.random(nl + nr) < 0.25, lonely[rng.integers(0, len(lonely), nl + nr)], rng.integers(0, nmp, nl + nr))
    entry = np.where(rng.random(nl + nr) < 0.15, held, -1).astype(np.int32)
    # the last frame: rows of both cameras
    nlast_l = nlast * 3 // 5
    mp = np.where(rng.random(nlast) < 0.9, rng.permutation(max(nmp, nlast))[:nlast] % nmp, -1).astype(np.int32)
    last = dict(octave=np.clip(level[np.maximum(mp, 0)] + rng.integers(-1, 2, nlast), 0, 7).astype(np.int32),
                angle=rng.choice(np.array([10.0, 10.0, 40.0, 100.0, 220.0, 300.0], f32), nlast), mp=mp,
                outlier=(rng.random(nlast) < 0.1).astype(np.int32), nleft=nlast_l)
    return dict(Trl=Trl, poses=poses, last_T=last_T, pool=pool, kl=kl, dl=dl, kr=kr, dr=dr, l2r=l2r, r2l=r2l, entry=entry, last=last)


def write_input(path, W, b_mono=0, b_far=1):
    nl, nr, last = len(W["kl"]), len(W["kr"]), W["last"]
    m = len(last["mp"])
    kp = np.concatenate([W["kl"], W["kr"]])
    with open(path, "wb") as f:
        f.write(np.array([nl, nr, last["nleft"], m - last["nleft"], len(W["pool"]), len(W["poses"]), b_mono, b_far], np.int32).tobytes())
        f.write(np.array(list(BOUNDS) + [TH_TRACK, TH_LOCAL, TH_FAR, MB], f32).tobytes() + scale_factors().tobytes())
        f.write(np.array(CAM, f32).tobytes())
        for T in W["poses"]:
            f.write(T.tobytes())
        f.write(W["last_T"].tobytes() + W["Trl"].tobytes())
        f.write(kp["x"].tobytes() + kp["y"].tobytes() + kp["octave"].astype(np.int32).tobytes() + kp["angle"].tobytes())
        f.write(np.ascontiguousarray(np.concatenate([W["dl"], W["dr"]])).tobytes() + W["entry"].tobytes())
        f.write(W["l2r"].tobytes() + W["r2l"].tobytes())
        f.write(last["octave"].tobytes() + last["angle"].tobytes() + last["mp"].tobytes() + last["outlier"].tobytes())
        f.write(W["pool"].tobytes())


def occupied(W):
    pool, entry, nl = W["pool"], W["entry"], len(W["kl"])
    occ = np.array([e >= 0 and pool["nobs"][e] > 0 for e in entry.tolist()], np.uint8)
    return occ[:nl], occ[nl:]


def expected_track(W, Tcw, b_mono=0):
    """-> nmatches, mvpMapPoints (pool indices) after SearchByProjection(CurrentFrame, LastFrame, th, bMono), direction"""
    pool, last, sf = W["pool"], W["last"], scale_factors()
    Rcw, tcw = Tcw[:3, :3], Tcw[:3, 3]
    zero = np.zeros(3, f32)
    twc = np.array([f32(-1.0 * (f64(Rcw[0, r]) * f64(tcw[0]) + f64(Rcw[1, r]) * f64(tcw[1]) + f64(Rcw[2, r]) * f64(tcw[2]))) for r in range(3)], f32)
    tlc = transform(W["last_T"][:3, :3], W["last_T"][:3, 3], twc)
    forward, backward = bool(tlc[2] > MB and not b_mono), bool(-tlc[2] > MB and not b_mono)
    m = len(last["mp"])
    ql, qr = np.zeros(m, PROJ_QUERY_DT), np.zeros(m, PROJ_QUERY_DT)
    ql["max_level"] = qr["max_level"] = -1
    behind = 0
    for i in range(m):
        p = last["mp"][i]
        if p < 0 or last["outlier"][i]:
            continue
        x = transform(Rcw, tcw, pool["pos"][p])
        invz = f32(1.0 / f64(x[2]))
        if invz < 0:
            behind += 1
            continue
        o = int(last["octave"][i])
        lo, hi = (o, -1) if forward else (0, o) if backward else (o - 1, o + 1)
        ql[i] = (*project(x), f32(f32(TH_TRACK) * sf[o]), 0.0, lo, hi, last["angle"][i], 1 if pool["nobs"][p] > 0 else 1 | NO_OBS)
        qr[i] = ql[i]
        qr["u"][i], qr["v"][i] = project(transform(W["Trl"][:, :3], W["Trl"][:, 3], x))
    occ_l, occ_r = occupied(W)
    qd = pool["desc"][np.maximum(last["mp"], 0)]
    n, bl, br, rl, rr, exits, _ = two_camera_scalar(ql, qr, qd, W["kl"], W["dl"], W["kr"], W["dr"], BOUNDS, True, occ_l, occ_r)
    out, nl = W["entry"].copy(), len(W["kl"])
    for i in range(m):                                           # the reference's writes in its order, then the filter's
        if rl[i] >= 0:
            out[rl[i]] = last["mp"][i]
        if rr[i] >= 0:
            out[nl + rr[i]] = last["mp"][i]
    for i in range(m):
        if rl[i] >= 0 > bl[i]:
            out[rl[i]] = -1
        if rr[i] >= 0 > br[i]:
            out[nl + rr[i]] = -1
    stats = dict(direction="forward" if forward else "backward" if backward else "neither", behind=behind,
                 no_obs=int(((ql["valid"] & NO_OBS) != 0).sum()), skipped=sum(1 for e in exits if e[1][:1] == ("skipped",) and e[0][0] != "invalid"),
                 right=int((rr >= 0).sum()), filtered=int((rl >= 0).sum() + (rr >= 0).sum()) - n)
    return n, out, stats


def local_map_queries(W, th=TH_LOCAL, b_far=1):
    pool, sf = W["pool"], scale_factors()
    n = len(pool)
    gate = ((pool["in_view"] != 0) | (pool["in_view_r"] != 0)) & (pool["bad"] == 0)          # :53-59
    if b_far:
        gate &= ~(pool["depth"] > f32(TH_FAR))
    ql, qr = np.zeros(n, PROJ_QUERY_DT), np.zeros(n, PROJ_QUERY_DT)
    r = np.where(pool["view_cos"] > 0.998, f32(2.5), f32(4.0)).astype(f32)
    if f32(th) != 1.0:
        r = (r * f32(th)).astype(f32)
    ql["u"], ql["v"], ql["radius"] = pool["proj_x"], pool["proj_y"], (r * sf[pool["level"]]).astype(f32)
    ql["min_level"], ql["max_level"] = pool["level"] - 1, pool["level"]
    ql["valid"] = gate & (pool["in_view"] != 0)
    rr = np.where(pool["view_cos_r"] > 0.998, f32(2.5), f32(4.0)).astype(f32)                  # no th factor, :148
    qr["u"], qr["v"], qr["radius"] = pool["proj_xr"], pool["proj_yr"], (rr * sf[np.maximum(pool["level_r"], 0)]).astype(f32)
    qr["min_level"], qr["max_level"] = pool["level_r"] - 1, pool["level_r"]
    qr["valid"] = gate & (pool["in_view_r"] != 0) & (pool["level_r"] != -1)
    for q in (ql, qr):
        for name in ("u", "v", "radius", "min_level", "max_level"):
            q[name] = np.where(q["valid"] != 0, q[name], 0)
    return ql, qr


def local_map_two_cameras(ql, qr, qdesc, kpl, dl, occl, l2r, kpr, dr, occr, r2l, bounds, nnratio):
    """ORBmatcher.cc:44-214 for F.Nleft != -1, line by line -> nmatches, mp_left, mp_right (the point this call left in the slot).
    Every searching point has observations (the adapter refuses the others), so a slot written becomes unavailable."""
    nl = len(kpl)
    cells = (_cells(kpl, bounds), _cells(kpr, bounds))
    taken = [np.asarray(occl) != 0, np.asarray(occr) != 0]
    taken = [taken[0].copy(), taken[1].copy()]
    mp = [np.full(nl, -1, np.int32), np.full(len(kpr), -1, np.int32)]
    partner = (l2r, r2l)
    nmatches = 0
    stats = dict(left=0, right=0, partner=0, ratio=0)

    def best_two(cam, Q, i):
        kp, desc = (kpl, kpr)[cam], (dl, dr)[cam]
        px, py, ingrid, gw, gh = cells[cam]
        idx = _area(Q, kp, px, py, ingrid, bounds, gw, gh, [])
        if idx is None or idx.size == 0:
            return None
        d_all = hamming(qdesc[i][None], desc[idx])
        bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
        for k, j in enumerate(idx.tolist()):
            if taken[cam][j]:
                continue
            d = int(d_all[k])
            if d < bd:
                bd2, bd, bl2, bl, bi = bd, d, bl, int(kp["octave"][j]), j
            elif d < bd2:
                bl2, bd2 = int(kp["octave"][j]), d
        return bd, bl, bd2, bl2, bi

    for i in range(len(ql)):
        if ql["valid"][i]:
            r = best_two(0, ql[i], i)
            if r is not None and r[0] <= TH_HIGH:
                bd, bl, bd2, bl2, bi = r
                if bl == bl2 and f32(bd) > f32(f32(nnratio) * f32(bd2)):
                    stats["ratio"] += 1
                    continue                                     # :126 leaves the map point: the right camera is not searched
                mp[0][bi] = i; taken[0][bi] = True
                if l2r[bi] != -1:
                    mp[1][l2r[bi]] = i; taken[1][l2r[bi]] = True
                    nmatches += 1; stats["partner"] += 1
                nmatches += 1; stats["left"] += 1
        if qr["valid"][i]:
            r = best_two(1, qr[i], i)
            if r is None:
                continue
            bd, bl, bd2, bl2, bi = r
            if bd <= TH_HIGH:
                if bl == bl2 and f32(bd) > f32(f32(nnratio) * f32(bd2)):
                    stats["ratio"] += 1
                    continue
                if r2l[bi] != -1:
                    mp[0][r2l[bi]] = i; taken[0][r2l[bi]] = True
                    nmatches += 1; stats["partner"] += 1
                mp[1][bi] = i; taken[1][bi] = True
                nmatches += 1; stats["right"] += 1
    return nmatches, mp[0], mp[1], stats


def expected_local_map(W, b_far=1):
    ql, qr = local_map_queries(W, b_far=b_far)
    occ_l, occ_r = occupied(W)
    n, mpl, mpr, stats = local_map_two_cameras(ql, qr, W["pool"]["desc"], W["kl"], W["dl"], occ_l, W["l2r"], W["kr"], W["dr"], occ_r,
                                               W["r2l"], BOUNDS, NNRATIO_LOCAL)
    out = W["entry"].copy()
    both = np.concatenate([mpl, mpr])
    out[both >= 0] = both[both >= 0]
    return n, out, stats


WORLD_SEED = 91
_WORLD = {}


def world():
    if "w" not in _WORLD:
        _WORLD["w"] = make_world(np.random.default_rng(WORLD_SEED))
    return _WORLD["w"]


@pytest.mark.gpu
def test_the_adapter_equals_the_restatements(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    W = world()
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, W)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(outp, np.int32)
    n_slots = len(W["kl"]) + len(W["kr"])
    at = 0
    for k, Tcw in enumerate(W["poses"]):
        n, out, stats = expected_track(W, Tcw)
        assert raw[at] == n and np.array_equal(raw[at + 1:at + 1 + n_slots], out), ("frame to frame", k, stats)
        at += 1 + n_slots
    n, out, _ = expected_local_map(W)
    assert raw[at] == n and np.array_equal(raw[at + 1:at + 1 + n_slots], out), "the local map"
    at += 1 + n_slots
    assert at + 2 == len(raw) and raw[at] > 10 and raw[at + 1] > 10          # the one-camera frame matched something


def test_the_world_is_not_vacuous():
    """On the CPU: the three poses are a forward, a backward and a sideways motion; rows of both last-frame cameras match; there are
    rows without a map point, outliers, points behind the camera, points without observations, slots held at entry with and without
    observations, right cameras left unsearched, right matches and filtered matches; the local map has bad points, points out of
    view, far points, matches in both cameras, partner writes and ratio rejections."""
    W = world()
    pool, last, entry = W["pool"], W["last"], W["entry"]
    directions = []
    for Tcw in W["poses"]:
        n, out, stats = expected_track(W, Tcw)
        directions.append(stats["direction"])
        assert n > 40 and stats["behind"] > 5 and stats["no_obs"] > 5 and stats["skipped"] > 5 and stats["right"] > 15 and stats["filtered"] > 0, stats
        rows = [int(np.flatnonzero(last["mp"] == p)[0]) for p in out[out != entry]]
        assert min(rows) < last["nleft"] <= max(rows)
    assert directions == ["forward", "backward", "neither"]
    assert (last["mp"] < 0).sum() > 10 and last["outlier"].sum() > 10
    with_obs = np.array([e >= 0 and pool["nobs"][e] > 0 for e in entry.tolist()])
    assert with_obs.sum() > 20 and ((entry >= 0) & ~with_obs).sum() > 3
    n, out, stats = expected_local_map(W)
    n_all, _, _ = expected_local_map(W, b_far=0)
    assert min(stats["left"], stats["right"], stats["partner"]) > 10 and stats["ratio"] > 0 and n_all > n, (stats, n_all, n)
    assert (pool["bad"] != 0).sum() > 10 and ((pool["in_view"] == 0) & (pool["in_view_r"] == 0)).sum() > 5


def test_the_local_map_restatement_equals_the_oracle(oracle):
    """local_map_two_cameras against the CPU oracle's ORBmatcher.cc:44-214 (an independent C++ restatement), on the world's tables."""
    W = world()
    for b_far in (1, 0):
        ql, qr = local_map_queries(W, b_far=b_far)
        occ_l, occ_r = occupied(W)
        n, mpl, mpr, _ = local_map_two_cameras(ql, qr, W["pool"]["desc"], W["kl"], W["dl"], occ_l, W["l2r"], W["kr"], W["dr"], occ_r,
                                               W["r2l"], BOUNDS, NNRATIO_LOCAL)
        on, ompl, ompr = oracle.search_local_map_fisheye(ql, qr, W["pool"]["desc"], W["kl"], W["dl"], occ_l, W["l2r"], W["kr"], W["dr"],
                                                         occ_r, W["r2l"], BOUNDS, NNRATIO_LOCAL)
        assert n == on and np.array_equal(mpl, ompl) and np.array_equal(mpr, ompr)
