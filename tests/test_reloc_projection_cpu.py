"""Relocalisation's ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2325-2447;
Tracking.cc:4290 with th 10, ORBdist 100 and :4304 with 3, 64) restated twice in Python, CPU only:

  reloc_search_scalar  the reference's control flow, literally: the grid lists, Frame::GetFeaturesInArea's early returns and loops
                       (Frame.cc:774-843), the running strict minimum over the rows whose mvpMapPoints entry is NULL,
                       mvpMapPoints[bestIdx2] = pMP, rotHist, ComputeThreeMaxima's loop, the rows set back to NULL.  It counts every
                       exit.
  reloc_search_fast    the closed form pli_search_by_projection_reloc uses: vectorised gates, the level as a count of thresholds,
                       every point's keys (distance, cell column, cell row, index) within ORBdist, the ordered walk that takes the
                       smallest key whose row is free, then the histogram over the rows taken and the filter.

What differs from the Sim3 search (tests/test_sim3_projection_cpu.py): no z < 0 gate, the image gate closed on both sides, no
viewing-normal gate, octaves in [level - 1, level + 1], an integer threshold, the rotation filter, and the roles (the searched
table is the frame; every candidate has its own point list, pose and occupied rows).  The one deviation from the reference, stated
in include/pli_frontend.h: a NaN projection leaves at the image gate (the reference converts it to int, which is undefined).
tests/test_reloc_projection_gpu.py compares the device with these exactly.

Exits of the constructed scenes (SEEDED, the settings of test_the_two_restatements_agree_and_every_exit_is_taken; printed by that
test): null 138, bad 146, already_found 136, outside_x 358, outside_y 322, range 218, empty_window 1230, all_owned 106,
above_threshold 674, match 672 (47 of them points behind the camera), filtered 130 (542 kept)."""
import ctypes as C
import math
import os
import re
from collections import Counter, namedtuple

import numpy as np

from helpers_matchers import GRID_COLS, GRID_ROWS, HISTO_LENGTH, c_round, hamming, three_maxima
from test_fuse_search_cpu import (CAM, FUSE_POINT_DT, IDENTITY, NLEVELS, SF, flip_bits, gemm_row, level_ratio, make_points, make_pose,
                                  point_at_pixel, predict_scale, rot_xyz)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
INT_MAX = np.iinfo(np.int32).max
FR = namedtuple("FR", "x y octave desc angle")                        # the frame's table: mvKeysUn, mDescriptors
Cand = namedtuple("Cand", "points descs angles pose occupied")        # one candidate keyframe's side of the call
# Two more are counted and cannot be taken: "cell_return" (the early returns of Frame::GetFeaturesInArea: behind the image gate
# u - radius < mnMaxX and u + radius > mnMinX always hold) and "no_candidate" (a free row in the window and bestDist still 256: a
# descriptor that differs in all 256 bits).
EXITS = ("null", "bad", "already_found", "outside_x", "outside_y", "range", "empty_window", "all_owned", "above_threshold", "match",
         "filtered")
SETTINGS = ((10.0, 100), (3.0, 64))                                   # th, ORBdist: Tracking.cc:4290, :4304
FACTOR = f32(1.0) / f32(HISTO_LENGTH)


def rot_bin(a, b, trunc=False):
    """:2410-2415 (trunc: the misreading `int bin = rot * factor`)"""
    rot = f32(f32(a) - f32(b))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = int(f32(rot * FACTOR)) if trunc else int(c_round(f32(rot * FACTOR)))
    return 0 if b == HISTO_LENGTH else b


# ---- the reference's control flow ----------------------------------------------------------------------------------------------

def reloc_search_scalar(cand, fr, cam, th=10.0, orb_dist=100, check_ori=True, exits=None, state=None, info=None, misread=()):
    """-> row_point[nf] (the point that holds the row after the filter, -1 otherwise), best_idx[nmp] (before the filter),
    nmatches.  state (optional, for the exit counts): 0 = NULL, 1 = isBad(), 2 = in sAlreadyFound, 3 = taking part; the call itself
    sees only valid = (state == 3).  info (a Counter): "behind_matched" counts the matches of points with z < 0.  misread: deliberate
    misreadings that tests/test_ref_pin_match.py wants rejected ("min_le": <= in the running minimum; "image_half_open": u >= mnMaxX
    leaves, as KeyFrame::IsInImage has it; "rot_trunc": the rotation bin by truncation; "octave_narrow": octaves [level - 1, level];
    "orb_dist_strict": bestDist < ORBdist)."""
    exits = exits if exits is not None else Counter()
    info = info if info is not None else Counter()
    points, descs = cand.points, cand.descs
    n = len(fr.x)
    gw_inv = f32(f32(GRID_COLS) / f32(cam.max_x - cam.min_x))
    gh_inv = f32(f32(GRID_ROWS) / f32(cam.max_y - cam.min_y))
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
    for i in range(n):                                               # Frame::AssignFeaturesToGrid / PosInGrid
        px = int(c_round(f32(f32(fr.x[i] - cam.min_x) * gw_inv)))
        py = int(c_round(f32(f32(fr.y[i] - cam.min_y) * gh_inv)))
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid[px][py].append(i)
    R, t, Ow = cand.pose[:9].reshape(3, 3), cand.pose[9:12], cand.pose[12:15]
    th = f32(th)
    mvp = [None if cand.occupied is None or not cand.occupied[j] else "entry" for j in range(n)]      # mvpMapPoints
    best_idx = np.full(len(points), -1, np.int32)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    with np.errstate(all="ignore"):
        for i, P in enumerate(points):
            if state is not None and state[i] != 3:
                assert not P["valid"]
                exits[("null", "bad", "already_found")[state[i]]] += 1; continue
            if not P["valid"]:
                exits["bad"] += 1; continue
            p = P["pos"]
            x, y, z = (gemm_row(R[r], p, t[r]) for r in range(3))
            u = f32(f32(f32(cam.fx * x) / z) + cam.cx)               # Pinhole::project; no z < 0 gate
            v = f32(f32(f32(cam.fy * y) / z) + cam.cy)
            if np.isnan(u) or np.isnan(v):                           # the stated deviation: a NaN leaves
                exits["outside_x"] += 1; continue
            if u < cam.min_x or u > cam.max_x or ("image_half_open" in misread and u == cam.max_x):
                exits["outside_x"] += 1; continue
            if v < cam.min_y or v > cam.max_y:
                exits["outside_y"] += 1; continue
            PO = (p - Ow).astype(f32)
            dist3D = f32(math.sqrt(float(PO[0]) ** 2 + float(PO[1]) ** 2 + float(PO[2]) ** 2))
            if dist3D < P["min_dist_inv"] or dist3D > P["max_dist_inv"]:
                exits["range"] += 1; continue
            level = predict_scale(f32(P["max_dist"] / dist3D))
            radius = f32(th * SF[level])
            min_level, max_level = level - 1, level + (0 if "octave_narrow" in misread else 1)
            idxs, returned = [], True                                # Frame::GetFeaturesInArea
            c0 = max(0, math.floor(f32(f32(f32(u - cam.min_x) - radius) * gw_inv)))
            if c0 < GRID_COLS:
                c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(u - cam.min_x) + radius) * gw_inv)))
                if c1 >= 0:
                    r0 = max(0, math.floor(f32(f32(f32(v - cam.min_y) - radius) * gh_inv)))
                    if r0 < GRID_ROWS:
                        r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(v - cam.min_y) + radius) * gh_inv)))
                        if r1 >= 0:
                            returned = False
                            check_levels = min_level > 0 or max_level >= 0
                            for ix in range(c0, c1 + 1):
                                for iy in range(r0, r1 + 1):
                                    for j in grid[ix][iy]:
                                        if check_levels:
                                            if fr.octave[j] < min_level:
                                                continue
                                            if max_level >= 0 and fr.octave[j] > max_level:
                                                continue
                                        if abs(f32(fr.x[j] - u)) < radius and abs(f32(fr.y[j] - v)) < radius:
                                            idxs.append(j)
            if not idxs:
                exits["cell_return" if returned else "empty_window"] += 1; continue
            bd, bi, owned = 256, -1, 0
            for j in idxs:
                if mvp[j] is not None:
                    owned += 1; continue
                d = int(hamming(descs[i], fr.desc[j]))
                if d < bd or ("min_le" in misread and d == bd):
                    bd, bi = d, j
            if bd <= orb_dist - ("orb_dist_strict" in misread):
                assert bi >= 0                                       # (the entry point refuses orb_dist = 256)
                mvp[bi] = i
                best_idx[i] = bi
                nmatches += 1
                exits["match"] += 1
                if z < 0:
                    info["behind_matched"] += 1
                if check_ori:
                    rot_hist[rot_bin(cand.angles[i], fr.angle[bi], "rot_trunc" in misread)].append(bi)
            elif bi >= 0:
                exits["above_threshold"] += 1
            else:
                exits["all_owned" if owned else "no_candidate"] += 1
    if check_ori:                                                    # ComputeThreeMaxima :2449-2490
        max1 = max2 = max3 = 0
        ind1 = ind2 = ind3 = -1
        for b in range(HISTO_LENGTH):
            s = len(rot_hist[b])
            if s > max1:
                max3, max2, max1 = max2, max1, s
                ind3, ind2, ind1 = ind2, ind1, b
            elif s > max2:
                max3, max2 = max2, s
                ind3, ind2 = ind2, b
            elif s > max3:
                max3, ind3 = s, b
        if max2 < f32(0.1) * f32(max1):
            ind2 = ind3 = -1
        elif max3 < f32(0.1) * f32(max1):
            ind3 = -1
        info["bins_kept"] = sum(1 for b in (ind1, ind2, ind3) if b >= 0)
        for b in range(HISTO_LENGTH):
            if b != ind1 and b != ind2 and b != ind3:
                for j in rot_hist[b]:
                    mvp[j] = None
                    nmatches -= 1
                    exits["filtered"] += 1
    row_point = np.array([m if isinstance(m, (int, np.integer)) else -1 for m in mvp], np.int32).reshape(n)
    return row_point, best_idx, nmatches


# ---- the closed form -----------------------------------------------------------------------------------------------------------

def reloc_survivors(points, pose, cam, th, lr=None):
    """The parallel gates: ok[nmp], u, v, z, level, radius."""
    lr = level_ratio() if lr is None else lr
    R, t, Ow = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64), pose[12:15]
    pos = points["pos"]
    with np.errstate(all="ignore"):
        x, y, z = [(R[r, 0] * pos[:, 0].astype(f64) + R[r, 1] * pos[:, 1].astype(f64) + R[r, 2] * pos[:, 2].astype(f64) + t[r]).astype(f32)
                   for r in range(3)]
        u, v = (cam.fx * x) / z + cam.cx, (cam.fy * y) / z + cam.cy
        assert u.dtype == f32 and v.dtype == f32
        POd = (pos - Ow[None, :]).astype(f32).astype(f64)
        dist3D = np.sqrt(POd[:, 0] ** 2 + POd[:, 1] ** 2 + POd[:, 2] ** 2).astype(f32)
        ok = points["valid"] != 0
        ok &= (u >= cam.min_x) & (u <= cam.max_x) & (v >= cam.min_y) & (v <= cam.max_y)
        ok &= ~((dist3D < points["min_dist_inv"]) | (dist3D > points["max_dist_inv"]))
        level = ((points["max_dist"] / dist3D)[:, None] > lr[None, :]).sum(1)
        radius = f32(th) * SF[level]
        assert radius.dtype == f32
    return ok, u, v, z, level, radius


def reloc_search_fast(cand, fr, cam, th=10.0, orb_dist=100, check_ori=True, lr=None, info=None):
    """info (a dict, optional): "listed"[nmp], the keys of every point within ORBdist, owned rows included (its candidate list)."""
    points, descs = cand.points, cand.descs
    nmp, n = len(points), len(fr.x)
    best_idx = np.full(nmp, -1, np.int32)
    owner = np.full(n, -1, np.int64)
    if cand.occupied is not None:
        owner[np.asarray(cand.occupied) != 0] = INT_MAX
    if nmp and n:
        ok, u, v, _, level, radius = reloc_survivors(points, cand.pose, cam, th, lr)
        gw_inv = f32(f32(GRID_COLS) / f32(cam.max_x - cam.min_x))
        gh_inv = f32(f32(GRID_ROWS) / f32(cam.max_y - cam.min_y))
        rnd = lambda a: (np.sign(a) * np.floor(np.abs(a).astype(f64) + 0.5)).astype(np.int64)
        px, py = rnd((fr.x - cam.min_x) * gw_inv), rnd((fr.y - cam.min_y) * gh_inv)
        in_grid = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
        octave = fr.octave.astype(np.int64)
        base_key = (px << 34) | (py << 28) | np.arange(n, dtype=np.int64)
        sel = np.nonzero(ok)[0]
        us, vs, rs, lv = u[sel, None], v[sel, None], radius[sel, None], level[sel, None]
        c0 = np.maximum(0, np.floor(((us - cam.min_x) - rs) * gw_inv)).astype(np.int64)
        c1 = np.minimum(GRID_COLS - 1, np.ceil(((us - cam.min_x) + rs) * gw_inv)).astype(np.int64)
        r0 = np.maximum(0, np.floor(((vs - cam.min_y) - rs) * gh_inv)).astype(np.int64)
        r1 = np.minimum(GRID_ROWS - 1, np.ceil(((vs - cam.min_y) + rs) * gh_inv)).astype(np.int64)
        cand_rows = in_grid[None, :] & (px[None, :] >= c0) & (px[None, :] <= c1) & (py[None, :] >= r0) & (py[None, :] <= r1)
        cand_rows &= (np.abs(fr.x[None, :] - us) < rs) & (np.abs(fr.y[None, :] - vs) < rs)
        cand_rows &= (octave[None, :] >= lv - 1) & (octave[None, :] <= lv + 1)
        for s, i in enumerate(sel):                                  # the ordered phase
            cols = np.nonzero(cand_rows[s])[0]
            if len(cols) == 0:
                continue
            d = hamming(descs[i][None, :], fr.desc[cols]).astype(np.int64)
            if info is not None:
                info.setdefault("listed", np.zeros(nmp, np.int64))[i] = int((d <= int(orb_dist)).sum())
            free = (d <= int(orb_dist)) & (owner[cols] == -1)
            if not free.any():
                continue
            b = int(((d[free] << 40) | base_key[cols[free]]).min() & 0xFFFFFFF)
            owner[b] = i
            best_idx[i] = b
    taken = np.nonzero((owner >= 0) & (owner != INT_MAX))[0]
    nmatches = len(taken)
    if check_ori:
        bins = np.array([rot_bin(cand.angles[owner[r]], fr.angle[r]) for r in taken], np.int64)
        sizes = np.bincount(bins, minlength=HISTO_LENGTH).tolist() if len(bins) else [0] * HISTO_LENGTH
        keep, _ = three_maxima(sizes)
        drop = ~np.isin(bins, [b for b in keep if b >= 0])
        owner[taken[drop]] = -1
        nmatches -= int(drop.sum())
    row_point = np.where((owner >= 0) & (owner != INT_MAX), owner, -1).astype(np.int32)
    return row_point, best_idx, nmatches


def reloc_search_batch(cands, fr, cam, th=10.0, orb_dist=100, check_ori=True, fn=reloc_search_fast):
    """-> row_point[ncand, nf], [best_idx per candidate], nmatches[ncand]"""
    rows, bis, nm = np.full((len(cands), len(fr.x)), -1, np.int32), [], np.zeros(len(cands), np.int32)
    for k, cd in enumerate(cands):
        rows[k], bi, nm[k] = fn(cd, fr, cam, th, orb_dist, check_ori)
        bis.append(bi)
    return rows, bis, nm


def agree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- constructed scenes --------------------------------------------------------------------------------------------------------

def wrap360(a):
    a = np.mod(np.asarray(a, f64), 360.0).astype(f32)
    a[a >= f32(360.0)] = 0.0
    return a


def make_frame(rng, pool, pdesc, pose, nfeat, cam=CAM):
    """The frame's table: keypoints at the projections of a share of the pool - in FRONT of the camera or BEHIND it, whatever
    falls into the image - with pixel noise, descriptors some bits away (around both thresholds, 64 and 100), octaves at and around
    the predicted level (up to two above), twins and random decoys.  -> FR, src[nfeat] (the pool point behind a row, -1: a decoy)"""
    R, t, Ow = pose[:9].reshape(3, 3).astype(f64), pose[9:12].astype(f64), pose[12:15].astype(f64)
    pc = pool["pos"].astype(f64) @ R.T + t
    u = float(cam.fx) * pc[:, 0] / pc[:, 2] + float(cam.cx)
    v = float(cam.fy) * pc[:, 1] / pc[:, 2] + float(cam.cy)
    vis = np.nonzero((u >= 0) & (u < 752) & (v >= 0) & (v < 480))[0]
    vis = rng.permutation(vis)[:int(nfeat * 0.6)]
    xs, ys, octs, ds, src = [], [], [], [], []

    def add(i, x, y, d, lev_off):
        dist = np.linalg.norm(pool["pos"][i].astype(f64) - Ow)
        lev = predict_scale(f32(float(pool["max_dist"][i]) / dist))
        xs.append(x); ys.append(y); ds.append(d); src.append(i)
        octs.append(int(np.clip(lev + lev_off, 0, NLEVELS - 1)))
    for i in vis:
        x, y = u[i] + rng.normal(0, 0.8), v[i] + rng.normal(0, 0.8)
        d = flip_bits(rng, pdesc[i], int(rng.choice([0, 3, 10, 25, 45, 60, 64, 65, 90, 100, 101, 130])))
        off = int(rng.choice([0, 0, 0, -1, -1, 1, 1, 2, -2]))
        add(i, x, y, d, off)
        if rng.random() < 0.25:                                      # a twin: equal distance, a pixel away
            add(i, x + rng.uniform(-1.5, 1.5), y + rng.uniform(-1.5, 1.5), d, off)
    while len(xs) < nfeat:                                           # decoys
        xs.append(rng.uniform(0, 752)); ys.append(rng.uniform(0, 480)); octs.append(int(rng.integers(0, NLEVELS)))
        ds.append(rng.integers(0, 256, 32, dtype=np.uint8)); src.append(-1)
    order = rng.permutation(len(xs))[:nfeat]
    angle = wrap360(rng.uniform(0, 360, nfeat))
    return (FR(np.array(xs, f32)[order], np.array(ys, f32)[order], np.array(octs, np.int32)[order],
               np.array(ds, np.uint8).reshape(-1, 32)[order], angle), np.array(src)[order])


def reloc_case(rng, ncand, nmp=400, nfeat=400):
    """One frame and ncand candidates in the style of sim3_case.  A pool of map points seen from the origin (make_points: some
    behind the camera, some with a range that is too narrow); the frame's table is built from it under one pose.  Every candidate
    lists nmp pool points in an order of its own and sees the frame through that pose slightly disturbed (its own PnP result), with
    a tenth of the frame's rows occupied at entry and a tenth of its points NULL, bad or already found.  Keyframe angles = the
    frame angle of the point's keypoint + a rotation common to the candidate + noise for most points, random for the rest.
    -> FR, [Cand] * ncand, [state] * ncand"""
    npool = nmp + nmp // 2
    pool, pdesc = make_points(rng, npool)
    pool["valid"] = 1
    pose0 = make_pose(rot_xyz(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.5, 0.5, 3))
    fr, src = make_frame(rng, pool, pdesc, pose0, nfeat)
    row_of = np.full(npool, -1)
    row_of[src[src >= 0][::-1]] = np.nonzero(src >= 0)[0][::-1]        # the first row built from a pool point
    cands, states = [], []
    for _ in range(ncand):
        pick = rng.permutation(npool)[:nmp]
        pts, descs = pool[pick].copy(), pdesc[pick].copy()
        state = np.full(nmp, 3)
        bad = rng.random(nmp) < 0.1
        state[bad] = rng.integers(0, 3, bad.sum())
        pts["valid"] = (state == 3).astype(np.int32)
        R0 = pose0[:9].reshape(3, 3).astype(f64)
        pose = make_pose(rot_xyz(*rng.uniform(-0.002, 0.002, 3)) @ R0, pose0[9:12] + rng.uniform(-0.01, 0.01, 3).astype(f32))
        common = rng.uniform(0, 360)
        ang = rng.uniform(0, 360, nmp)
        has = row_of[pick] >= 0
        consistent = has & (rng.random(nmp) < 0.85)
        ang[consistent] = fr.angle[row_of[pick][consistent]].astype(f64) + common + rng.normal(0, 3.0, consistent.sum())
        occupied = (rng.random(nfeat) < 0.1).astype(np.uint8)
        cands.append(Cand(pts, descs, wrap360(ang), pose, occupied))
        states.append(state)
    return fr, cands, states


SEEDED = ((1, 3), (2, 2))                                             # seed, ncand


def test_the_two_restatements_agree_and_every_exit_is_taken():
    exits, info = Counter(), Counter()
    matches = 0
    for seed, ncand in SEEDED:
        fr, cands, states = reloc_case(np.random.default_rng(seed), ncand)
        assert len(fr.x) == 400 and all(len(cd.points) == 400 for cd in cands)
        for th, orb_dist in SETTINGS:
            for k, cd in enumerate(cands):
                a = reloc_search_scalar(cd, fr, CAM, th, orb_dist, True, exits, states[k], info)
                b = reloc_search_fast(cd, fr, CAM, th, orb_dist, True)
                assert agree(a, b), (seed, k, th, orb_dist)
                assert (a[0][cd.occupied != 0] == -1).all()          # rows occupied at entry stay -1
                taken = a[1][a[1] >= 0]
                assert len(set(taken.tolist())) == len(taken)        # a row is taken once
                kept = np.nonzero(a[0] >= 0)[0]
                assert len(kept) == a[2] and (a[1][a[0][kept]] == kept).all()
                matches += a[2]
                # without the filter: the same walk, nothing set back
                c = reloc_search_scalar(cd, fr, CAM, th, orb_dist, False)
                assert agree(c, reloc_search_fast(cd, fr, CAM, th, orb_dist, False))
                assert np.array_equal(c[1], a[1]) and c[2] == len(taken)
    print(dict(exits), dict(info), "kept", matches)
    for name in EXITS:
        assert exits[name] > 0, (name, dict(exits))
    assert info["behind_matched"] > 0                                # a point with z < 0 is matched
    assert exits["filtered"] > 0 and matches > 0.5 * exits["match"]  # the filter removes some matches and keeps most


# ---- hand-worked cases ---------------------------------------------------------------------------------------------------------

def frame_of(xs, ys, descs, octaves=None, angles=None):
    n = len(xs)
    return FR(np.array(xs, f32), np.array(ys, f32), np.zeros(n, np.int32) if octaves is None else np.array(octaves, np.int32),
              np.array(descs, np.uint8).reshape(n, 32), np.zeros(n, f32) if angles is None else np.array(angles, f32))


def cand_of(points, descs, angles=None, pose=IDENTITY, occupied=None):
    n = len(points)
    return Cand(points, np.array(descs, np.uint8).reshape(n, 32), np.zeros(n, f32) if angles is None else np.array(angles, f32), pose,
                occupied)


def both(cd, fr, th=10.0, orb_dist=100, check_ori=True, exits=None, info=None, cam=CAM):
    a = reloc_search_scalar(cd, fr, cam, th, orb_dist, check_ori, exits, None, info)
    b = reloc_search_fast(cd, fr, cam, th, orb_dist, check_ori)
    assert agree(a, b)
    return a[0].tolist(), a[1].tolist(), a[2]


def stack(*points):
    return np.concatenate(points)


def behind_case():
    """A point BEHIND the camera (z = -4) whose projection is (300, 200): Pinhole::project divides by the negative z, and nothing
    in :2351-2358 asks for its sign.  -> cand, frame"""
    P = point_at_pixel(300.0, 200.0, z=-4.0)
    d = np.arange(32, dtype=np.uint8)
    return cand_of(P, [d]), frame_of([301], [200], [d])


def edge_case():
    """A point whose projection is exactly u = mnMaxX = 752 (the float x is stepped until fx*x/z + cx rounds to it), and a keypoint
    inside its window.  -> cand, frame, u"""
    d = np.arange(32, dtype=np.uint8)
    z = f32(4.0)
    target = f32(CAM.max_x)
    x = f32((float(target) - float(CAM.cx)) * float(z) / float(CAM.fx))
    for _ in range(200):                                             # walk the float x until fx*x/z + cx rounds to 752 exactly
        u = f32(f32(f32(CAM.fx * x) / z) + CAM.cx)
        if u == target:
            break
        x = np.nextafter(x, f32(np.inf) if u < target else f32(-np.inf))
    assert u == target
    P = point_at_pixel(300.0, 200.0)
    P["pos"][0] = [x, 0.0, z]
    P["max_dist"] = np.linalg.norm(P["pos"][0].astype(f64))
    return cand_of(P, [d]), frame_of([744.0], [float(CAM.cy)], [d]), u      # (x = 748 rounds to cell column 64: off the grid)


def contention_cases():
    """name -> (cand, frame, kwargs, row_point, best_idx).  Every point projects to (300, 200) at level 0 (radius 10 at th 10); the
    rows lie inside the window."""
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    near = lambda nbits: flip_bits(rng, d, nbits)
    P = point_at_pixel(300.0, 200.0)
    two, three = stack(P, P), stack(P, P, P)
    dd = lambda k: np.stack([d] * k)
    cases = {}
    # two points whose best row is the same: the second gets its second-best row ...
    cases["second_best"] = (cand_of(two, dd(2)), frame_of([300, 301], [200, 200], [near(3), near(20)]), {}, [0, 1], [0, 1])
    # ... or nothing when that row is above ORBdist
    cases["second_best_above"] = (cand_of(two, dd(2)), frame_of([300, 301], [200, 200], [near(3), near(120)]), {}, [0, -1], [0, -1])
    # a row occupied at entry is nobody's: the point takes the next one, the row stays -1
    cases["occupied"] = (cand_of(P, dd(1), occupied=np.array([1, 0], np.uint8)),
                         frame_of([300, 301], [200, 200], [near(3), near(20)]), {}, [-1, 0], [1])
    # an invalid point (NULL, bad or already found) takes nothing and leaves its row to the next one
    inv = two.copy()
    inv["valid"][0] = 0
    cases["invalid"] = (cand_of(inv, dd(2)), frame_of([300, 301], [200, 200], [near(3), near(20)]), {}, [1, -1], [-1, 0])
    # a keypoint one octave ABOVE the level wins (the Sim3 search would not see it) ...
    cases["octave_plus_one"] = (cand_of(P, dd(1)), frame_of([300, 301], [200, 200], [near(3), near(20)], octaves=[1, 0]), {},
                                [0, -1], [0])
    # ... one two octaves above does not
    cases["octave_plus_two"] = (cand_of(P, dd(1)), frame_of([300, 301], [200, 200], [near(3), near(20)], octaves=[2, 0]), {},
                                [-1, 0], [1])
    # check_orientation off: the angles are not read
    cases["orientation_off"] = (cand_of(three, dd(3), angles=[0, 0, 180]),
                                frame_of([300, 301, 302], [200, 200, 200], [near(1), near(5), near(9)]),
                                dict(check_ori=False), [0, 1, 2], [0, 1, 2])
    return cases


def test_known_answers():
    for name, (cd, fr, kw, rows, best) in contention_cases().items():
        r, b, n = both(cd, fr, **kw)
        assert (r, b) == (rows, best) and n == sum(1 for x in r if x >= 0), (name, r, b)


def test_known_answer_a_point_behind_the_camera_matches():
    cd, fr = behind_case()
    _, u, v, z, _, _ = reloc_survivors(cd.points, cd.pose, CAM, 10.0)
    assert z[0] < 0 and abs(u[0] - 300) < 1e-3 and abs(v[0] - 200) < 1e-3
    info = Counter()
    assert both(cd, fr, info=info) == ([0], [0], 1) and info["behind_matched"] == 1


def test_known_answer_the_image_gate_is_closed_at_mnMaxX():
    cd, fr, u = edge_case()
    assert u == CAM.max_x and not (u < CAM.max_x)                    # KeyFrame::IsInImage would refuse it
    assert both(cd, fr) == ([0], [0], 1)
    beyond = cd.points.copy()
    beyond["pos"][0, 0] = np.nextafter(np.nextafter(beyond["pos"][0, 0], f32(np.inf)), f32(np.inf))
    u2 = reloc_survivors(beyond, cd.pose, CAM, 10.0)[1][0]
    if u2 > CAM.max_x:
        ex = Counter()
        assert both(cd._replace(points=beyond), fr, exits=ex) == ([-1], [-1], 0) and ex["outside_x"] == 1


def test_known_answer_thresholds():
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    P = point_at_pixel(300.0, 200.0)
    for th, orb_dist in SETTINGS:
        for nbits in (orb_dist - 1, orb_dist, orb_dist + 1):
            ex = Counter()
            r, b, n = both(cand_of(P, [d]), frame_of([300], [200], [flip_bits(rng, d, nbits)]), th, orb_dist, exits=ex)
            want = 0 if nbits <= orb_dist else -1
            assert b == [want] and n == (want == 0), (orb_dist, nbits)
            assert ex["match" if want == 0 else "above_threshold"] == 1


def reversal_case():
    """A's and B's best row is r1, B's second best and C's best is r2, r3 is everybody's last.  -> points, descs, frame"""
    rng = np.random.default_rng(6)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    e, g = flip_bits(rng, d, 10), flip_bits(rng, d, 20)
    P = point_at_pixel(300.0, 200.0)
    descs = np.stack([d, flip_bits(rng, d, 1), flip_bits(rng, e, 1)])
    return stack(P, P, P), descs, frame_of([300, 301, 299.5], [200, 200, 201], [d, e, g])


def test_known_answer_two_points_contend_in_both_list_orders():
    """In list order A takes r1, B falls to r2 and C, whose best r2 is gone, to r3.  Reversed, C comes first and takes r2, B takes
    r1, and A, whose r1 and r2 are gone, is left with r3."""
    pts, descs, fr = reversal_case()
    assert both(cand_of(pts, descs), fr) == ([0, 1, 2], [0, 1, 2], 3)
    assert both(cand_of(pts[::-1].copy(), descs[::-1].copy()), fr) == ([1, 0, 2], [1, 0, 2], 3)       # entries: C, B, A


def filtered_row_case():
    """Twelve points.  Point 0 takes r0, which is the best row of point 1 too, so point 1 falls to r1; points 2 .. 11 take a row
    each elsewhere.  Point 0 votes for bin 6 (182 degrees), the other eleven for bin 0: 1 < 0.1f * 11, so ComputeThreeMaxima keeps
    bin 0 alone and r0 ends as -1 although it blocked point 1 during the walk.  -> cand, frame, row_point, best_idx, nmatches"""
    rng = np.random.default_rng(9)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    P = point_at_pixel(300.0, 200.0)
    pts = [P, P]
    descs = [d, d]
    xs, ys, fd = [300.0, 301.0], [200.0, 200.0], [flip_bits(rng, d, 2), flip_bits(rng, d, 12)]
    for k in range(10):                                              # ten more points far apart, one row each
        e = rng.integers(0, 256, 32, dtype=np.uint8)
        pts.append(point_at_pixel(100.0 + 50.0 * k, 400.0))
        descs.append(e)
        xs.append(100.0 + 50.0 * k); ys.append(400.5); fd.append(flip_bits(rng, e, 4))
    angles = [182.0] + [3.0] * 11                                    # round(182 / 30) = 6; round(3 / 30) = 0; frame angles 0
    cd = cand_of(stack(*pts), descs, angles=angles)
    fr = frame_of(xs, ys, fd)
    return cd, fr, [-1, 1] + list(range(2, 12)), [0, 1] + list(range(2, 12)), 11


def test_known_answer_a_filtered_row_still_blocks_and_ends_empty():
    cd, fr, rows, best, nm = filtered_row_case()
    ex, info = Counter(), Counter()
    assert both(cd, fr, exits=ex, info=info) == (rows, best, nm)
    assert ex["filtered"] == 1 and ex["match"] == 12 and info["bins_kept"] == 1      # the second bin is below a tenth of the first
    # without the filter the row stays
    assert both(cd, fr, check_ori=False) == ([0, 1] + list(range(2, 12)), best, 12)


def test_three_maxima_the_second_bin_below_a_tenth_of_the_first():
    sizes = [0] * HISTO_LENGTH
    sizes[4], sizes[9], sizes[20] = 21, 2, 2                        # 2 < 0.1f * 21: only bin 4 is kept
    assert three_maxima(sizes)[0] == [4, -1, -1]
    sizes[9] = 3                                                     # 3 >= 2.1: bins 4 and 9; 2 < 2.1: not 20
    assert three_maxima(sizes)[0] == [4, 9, -1]
    cd, fr, _, _, _ = filtered_row_case()
    info = Counter()
    both(cd, fr, info=info)
    assert info["bins_kept"] == 1


def test_the_binding_declares_the_entry_point():
    from pli_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert re.search(r"pli_status\s+pli_search_by_projection_reloc\s*\(", hdr)
    assert "pli_search_by_projection_reloc" in capi._PROTOS and len(capi._PROTOS["pli_search_by_projection_reloc"][1]) == 19
    assert capi.FUSE_POINT_DT == FUSE_POINT_DT
    from pli_slam_amd.frontend import Frontend
    assert hasattr(Frontend, "search_by_projection_reloc")
    lib = C.CDLL(capi.LIB_PATH)                                      # the product library exports the symbol
    assert hasattr(lib, "pli_search_by_projection_reloc")
