"""Loop closing's ORBmatcher::SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
(ORBmatcher.cc:473-586 and :588-704) restated twice in Python, CPU only:

  sim3_search_scalar   the reference's control flow, literally: the grid lists, KeyFrame::GetFeaturesInArea's loops, the running
                       strict minimum over the rows that nobody owns, vpMatched[bestIdx] = pMP.  It counts every exit.
  sim3_search_fast     the closed form pli_search_by_projection_sim3 uses: vectorised gates, the level as a count of thresholds,
                       every point's keys (distance, cell column, cell row, index) within the limit, then the ordered walk that
                       takes the smallest key whose row is free.

project_form 0 is Pinhole::project (:519, fx*x/z + cx), 1 the inverse-depth form of :631-636 (invz = 1/z; x*invz; fx*x + cx).
The scene builders are those of tests/test_fuse_search_cpu.py.  tests/test_sim3_projection_gpu.py compares the device with these
exactly.

Exits of the constructed scenes (SEEDED, both forms, the settings of test_the_two_restatements_agree_and_every_exit_is_taken;
printed by that test): bad 222, already_found 1026, behind 402, outside 3192, range 522, angle 108, empty_window 298,
all_owned 716, no_candidate 638, above_threshold 938, match 3638."""
import ctypes as C
import math
import os
import re
import subprocess
from collections import Counter

import numpy as np

from helpers_matchers import GRID_COLS, GRID_ROWS, c_round, hamming
from test_fuse_search_cpu import (CAM, FUSE_POINT_DT, KF, SF, flip_bits, gemm_row, kf_of, level_ratio, make_keyframe, make_points,
                                  make_pose, point_at_pixel, predict_scale, rot_xyz)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
TH_LOW = 50
EXITS = ("bad", "already_found", "behind", "outside", "range", "angle", "empty_window", "all_owned", "no_candidate",
         "above_threshold", "match")


def dist_limit(ratio):
    """bestDist <= TH_LOW * ratioHamming (:577): int * float -> float, one rounding; the int side converts exactly."""
    return f32(f32(TH_LOW) * f32(ratio))


def project_uv(x, y, z, cam, form):
    """u, v of the camera-frame point (float32 scalars or arrays) in the reference's operation order."""
    if form == 0:                                                    # Pinhole::project, Pinhole.cpp:30-33
        return (cam.fx * x) / z + cam.cx, (cam.fy * y) / z + cam.cy
    invz = f32(1.0) / z                                              # ORBmatcher.cc:631-636
    return cam.fx * (x * invz) + cam.cx, cam.fy * (y * invz) + cam.cy


# ---- the reference's control flow ----------------------------------------------------------------------------------------------

def sim3_search_scalar(points, descs, kf, cam, th=3.0, ratio=1.0, form=0, skip=None, occupied=None, exits=None, misread=()):
    """-> row_point[n] (the point that took the row in this call, -1 otherwise), best_idx[nmp], nmatches; one pair.  misread:
    deliberate misreadings that tests/test_ref_pin_match.py wants rejected ("min_le": <= in the running minimum; "octave_narrow":
    the octave window one level wide; "owned_after": a row somebody owns is left out only after it has won; "image_closed": the image
    gate closed at mnMaxX; "limit_strict": bestDist < TH_LOW * ratioHamming)."""
    exits = exits if exits is not None else Counter()
    n = len(kf.x)
    gw_inv = f32(f32(GRID_COLS) / f32(cam.max_x - cam.min_x))
    gh_inv = f32(f32(GRID_ROWS) / f32(cam.max_y - cam.min_y))
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
    for i in range(n):
        px = int(c_round(f32(f32(kf.x[i] - cam.min_x) * gw_inv)))
        py = int(c_round(f32(f32(kf.y[i] - cam.min_y) * gh_inv)))
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid[px][py].append(i)
    R, t, Ow = kf.pose[:9].reshape(3, 3), kf.pose[9:12], kf.pose[12:15]
    th, limit = f32(th), dist_limit(ratio)
    matched = [None if occupied is None or not occupied[j] else "entry" for j in range(n)]      # vpMatched
    best_idx = np.full(len(points), -1, np.int32)
    nmatches = 0
    with np.errstate(all="ignore"):
        for i, P in enumerate(points):
            if not P["valid"]:
                exits["bad"] += 1; continue
            if skip is not None and skip[i]:
                exits["already_found"] += 1; continue
            p = P["pos"]
            x, y, z = (gemm_row(R[r], p, t[r]) for r in range(3))
            if z < f32(0.0):
                exits["behind"] += 1; continue
            u, v = project_uv(x, y, z, cam, form)
            assert u.dtype == f32 and v.dtype == f32
            if not (u >= cam.min_x and (u < cam.max_x or ("image_closed" in misread and u == cam.max_x)) and v >= cam.min_y and v < cam.max_y):
                exits["outside"] += 1; continue
            PO = (p - Ow).astype(f32)
            dist3D = f32(math.sqrt(float(PO[0]) ** 2 + float(PO[1]) ** 2 + float(PO[2]) ** 2))
            if dist3D < P["min_dist_inv"] or dist3D > P["max_dist_inv"]:
                exits["range"] += 1; continue
            Pn = P["normal"]
            if float(PO[0]) * float(Pn[0]) + float(PO[1]) * float(Pn[1]) + float(PO[2]) * float(Pn[2]) < 0.5 * float(dist3D):
                exits["angle"] += 1; continue
            level = predict_scale(f32(P["max_dist"] / dist3D))
            radius = f32(th * SF[level])
            idxs = []                                                # KeyFrame::GetFeaturesInArea
            c0 = max(0, math.floor(f32(f32(f32(u - cam.min_x) - radius) * gw_inv)))
            c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(u - cam.min_x) + radius) * gw_inv)))
            r0 = max(0, math.floor(f32(f32(f32(v - cam.min_y) - radius) * gh_inv)))
            r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(v - cam.min_y) + radius) * gh_inv)))
            if c0 < GRID_COLS and c1 >= 0 and r0 < GRID_ROWS and r1 >= 0:
                for ix in range(c0, c1 + 1):
                    for iy in range(r0, r1 + 1):
                        for j in grid[ix][iy]:
                            if abs(f32(kf.x[j] - u)) < radius and abs(f32(kf.y[j] - v)) < radius:
                                idxs.append(j)
            if not idxs:
                exits["empty_window"] += 1; continue
            bd, bi, owned = 256, -1, 0
            for j in idxs:
                if matched[j] is not None and "owned_after" not in misread:
                    owned += 1; continue
                lev = int(kf.octave[j])
                if lev < level - (0 if "octave_narrow" in misread else 1) or lev > level:
                    continue
                d = int(hamming(descs[i], kf.desc[j]))
                if d < bd or ("min_le" in misread and d == bd):
                    bd, bi = d, j
            if "owned_after" in misread and bi >= 0 and matched[bi] is not None:
                bd, bi, owned = 256, -1, 1
            if f32(bd) < limit if "limit_strict" in misread else f32(bd) <= limit:
                assert bi >= 0                                       # (the entry point refuses a limit of 256 or more)
                matched[bi] = i
                best_idx[i] = bi
                nmatches += 1
                exits["match"] += 1
            elif bi >= 0:
                exits["above_threshold"] += 1
            else:
                exits["all_owned" if owned else "no_candidate"] += 1
    row_point = np.array([m if isinstance(m, int) else -1 for m in matched], np.int32).reshape(n)
    return row_point, best_idx, nmatches


# ---- the closed form -----------------------------------------------------------------------------------------------------------

def survivors(points, kf, cam, th, form, skip=None, lr=None):
    """The parallel gates: ok[nmp], u, v, level, radius."""
    lr = level_ratio() if lr is None else lr
    R, t, Ow = kf.pose[:9].reshape(3, 3).astype(f64), kf.pose[9:12].astype(f64), kf.pose[12:15]
    pos = points["pos"]
    with np.errstate(all="ignore"):
        x, y, z = [(R[r, 0] * pos[:, 0].astype(f64) + R[r, 1] * pos[:, 1].astype(f64) + R[r, 2] * pos[:, 2].astype(f64) + t[r]).astype(f32)
                   for r in range(3)]
        u, v = project_uv(x, y, z, cam, form)
        assert u.dtype == f32 and v.dtype == f32
        POd = (pos - Ow[None, :]).astype(f32).astype(f64)
        dist3D = np.sqrt(POd[:, 0] ** 2 + POd[:, 1] ** 2 + POd[:, 2] ** 2).astype(f32)
        Pn = points["normal"].astype(f64)
        dot = POd[:, 0] * Pn[:, 0] + POd[:, 1] * Pn[:, 1] + POd[:, 2] * Pn[:, 2]
        ok = points["valid"] != 0
        if skip is not None:
            ok &= np.asarray(skip) == 0
        ok &= ~(z < 0) & (u >= cam.min_x) & (u < cam.max_x) & (v >= cam.min_y) & (v < cam.max_y)
        ok &= ~((dist3D < points["min_dist_inv"]) | (dist3D > points["max_dist_inv"])) & ~(dot < 0.5 * dist3D.astype(f64))
        level = ((points["max_dist"] / dist3D)[:, None] > lr[None, :]).sum(1)
        radius = f32(th) * SF[level]
        assert radius.dtype == f32
    return ok, u, v, level, radius


def sim3_search_fast(points, descs, kf, cam, th=3.0, ratio=1.0, form=0, skip=None, occupied=None, lr=None, info=None):
    """info (a dict, optional): "listed"[nmp], the keys of every point within the limit, owned rows included (its candidate list)."""
    nmp, n = len(points), len(kf.x)
    best_idx = np.full(nmp, -1, np.int32)
    owner = np.full(n, -1, np.int64)
    if occupied is not None:
        owner[np.asarray(occupied) != 0] = np.iinfo(np.int32).max
    if nmp and n:
        ok, u, v, level, radius = survivors(points, kf, cam, th, form, skip, lr)
        gw_inv = f32(f32(GRID_COLS) / f32(cam.max_x - cam.min_x))
        gh_inv = f32(f32(GRID_ROWS) / f32(cam.max_y - cam.min_y))
        rnd = lambda a: (np.sign(a) * np.floor(np.abs(a).astype(f64) + 0.5)).astype(np.int64)
        px, py = rnd((kf.x - cam.min_x) * gw_inv), rnd((kf.y - cam.min_y) * gh_inv)
        in_grid = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
        octave = kf.octave.astype(np.int64)
        base_key = (px << 34) | (py << 28) | np.arange(n, dtype=np.int64)
        limit = int(math.floor(float(dist_limit(ratio))))           # (float)d <= limit  <=>  d <= floor(limit), d an integer < 256
        sel = np.nonzero(ok)[0]
        us, vs, rs, lv = u[sel, None], v[sel, None], radius[sel, None], level[sel, None]
        c0 = np.maximum(0, np.floor(((us - cam.min_x) - rs) * gw_inv)).astype(np.int64)
        c1 = np.minimum(GRID_COLS - 1, np.ceil(((us - cam.min_x) + rs) * gw_inv)).astype(np.int64)
        r0 = np.maximum(0, np.floor(((vs - cam.min_y) - rs) * gh_inv)).astype(np.int64)
        r1 = np.minimum(GRID_ROWS - 1, np.ceil(((vs - cam.min_y) + rs) * gh_inv)).astype(np.int64)
        cand = in_grid[None, :] & (px[None, :] >= c0) & (px[None, :] <= c1) & (py[None, :] >= r0) & (py[None, :] <= r1)
        cand &= (np.abs(kf.x[None, :] - us) < rs) & (np.abs(kf.y[None, :] - vs) < rs)
        cand &= (octave[None, :] >= lv - 1) & (octave[None, :] <= lv)
        for s, i in enumerate(sel):                                  # the ordered phase
            cols = np.nonzero(cand[s])[0]
            if len(cols) == 0:
                continue
            d = hamming(descs[i][None, :], kf.desc[cols]).astype(np.int64)
            if info is not None:
                info.setdefault("listed", np.zeros(nmp, np.int64))[i] = int((d <= limit).sum())
            free = (d <= limit) & (owner[cols] == -1)
            if not free.any():
                continue
            b = int(((d[free] << 40) | base_key[cols[free]]).min() & 0xFFFFFFF)
            owner[b] = i
            best_idx[i] = b
    row_point = np.where((owner >= 0) & (owner != np.iinfo(np.int32).max), owner, -1).astype(np.int32)
    return row_point, best_idx, int((best_idx >= 0).sum())


def sim3_search_batch(points, descs, kfs, cam, th=3.0, ratio=1.0, form=0, skip=None, occupied=None, fn=sim3_search_fast):
    """-> [row_point per pair], best_idx[npair, nmp], nmatches[npair]"""
    rows, bi, nm = [], np.full((len(kfs), len(points)), -1, np.int32), np.zeros(len(kfs), np.int32)
    for k, kf in enumerate(kfs):
        rp, bi[k], nm[k] = fn(points, descs, kf, cam, th, ratio, form, None if skip is None else skip[k],
                              None if occupied is None else occupied[k])
        rows.append(rp)
    return rows, bi, nm


# ---- constructed scenes --------------------------------------------------------------------------------------------------------

def sim3_case(rng, npair, nmp, nfeat=400):
    """The scene of the Fuse tests with what this search adds: a third of the points listed twice (the second entry competes with
    the first for the same rows), a tenth of every keyframe's rows occupied at entry, a tenth of the pairs skipped.
    -> points, descs, [KF] * npair, skip[npair, nmp], [occupied] * npair"""
    base = nmp - nmp // 4
    pts, descs = make_points(rng, base)
    again = rng.choice(base, nmp - base, replace=False)
    order = rng.permutation(nmp)
    pts, descs = np.concatenate([pts, pts[again]])[order], np.concatenate([descs, descs[again]])[order]
    kfs = []
    for _ in range(npair):
        pose = make_pose(rot_xyz(*rng.uniform(-0.06, 0.06, 3)), rng.uniform(-0.6, 0.6, 3))
        kfs.append(make_keyframe(rng, pts, descs, pose, nfeat))
    skip = (rng.random((npair, nmp)) < 0.1).astype(np.uint8)
    occupied = [(rng.random(len(kf.x)) < 0.1).astype(np.uint8) for kf in kfs]
    return pts, descs, kfs, skip, occupied


SEEDED = ((1, 3, 300), (2, 2, 400), (3, 1, 250))
SETTINGS = ((3.0, 1.0), (5.0, 1.5), (8.0, 1.0))                      # th, ratio


def agree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_the_two_restatements_agree_and_every_exit_is_taken():
    exits = Counter()
    for seed, npair, nmp in SEEDED:
        pts, descs, kfs, skip, occ = sim3_case(np.random.default_rng(seed), npair, nmp)
        for form in (0, 1):
            for th, ratio in SETTINGS:
                for k, kf in enumerate(kfs):
                    a = sim3_search_scalar(pts, descs, kf, CAM, th, ratio, form, skip[k], occ[k], exits)
                    b = sim3_search_fast(pts, descs, kf, CAM, th, ratio, form, skip[k], occ[k])
                    assert agree(a, b), (seed, k, form, th, ratio)
                    assert (a[0][occ[k] != 0] == -1).all()           # rows occupied at entry stay -1
                    taken = a[1][a[1] >= 0]
                    assert len(set(taken.tolist())) == len(taken) == a[2] and (a[0][taken] == np.nonzero(a[1] >= 0)[0]).all()
    print(dict(exits))
    for name in EXITS:
        assert exits[name] > 0, (name, dict(exits))


def both(pts, descs, kf, th=3.0, ratio=1.0, form=0, skip=None, occupied=None, exits=None):
    a = sim3_search_scalar(pts, descs, kf, CAM, th, ratio, form, skip, occupied, exits)
    b = sim3_search_fast(pts, descs, kf, CAM, th, ratio, form, skip, occupied)
    assert agree(a, b)
    return a[0].tolist(), a[1].tolist(), a[2]


def stack(*points):
    return np.concatenate(points)


def contention_cases():
    """The hand-worked cases: name -> (points, descs, kf, kwargs, row_point, best_idx).  Every point projects to (300, 200) at
    level 0; the rows lie inside its 3 px window, in one grid cell unless stated."""
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    near = lambda nbits: flip_bits(rng, d, nbits)
    P = point_at_pixel(300.0, 200.0)
    two, three = stack(P, P), stack(P, P, P)
    dd = lambda k: np.stack([d] * k)
    cases = {}
    # two points whose best row is the same: the second gets its second-best row ...
    cases["second_best"] = (two, dd(2), kf_of([300, 301], [200, 200], [near(3), near(20)]), {}, [0, 1], [0, 1])
    # ... or nothing when that row is above the limit
    cases["second_best_above_limit"] = (two, dd(2), kf_of([300, 301], [200, 200], [near(3), near(60)]), {}, [0, -1], [0, -1])
    # a chain: A takes r1, B falls to r2, C falls to r3
    chain_kf = kf_of([300, 301, 299.5], [200, 200, 201], [near(2), near(9), near(30)])
    cases["chain"] = (three, dd(3), chain_kf, {}, [0, 1, 2], [0, 1, 2])
    # a row occupied at entry is nobody's: the best row is closed, the point takes the next one, the row stays -1
    cases["occupied"] = (P, dd(1), kf_of([300, 301], [200, 200], [near(3), near(20)]), dict(occupied=np.array([1, 0], np.uint8)),
                         [-1, 0], [1])
    # a skipped point takes nothing and leaves its row to the next one
    cases["skipped"] = (two, dd(2), kf_of([300, 301], [200, 200], [near(3), near(20)]), dict(skip=np.array([1, 0], np.uint8)),
                        [1, -1], [-1, 0])
    # a point listed twice is two entries: the second one takes the twin
    cases["listed_twice"] = (two, dd(2), kf_of([300, 300.5], [200, 200], [near(4), near(4)]), {}, [0, 1], [0, 1])
    return cases


def test_known_answers_contention():
    for name, (pts, descs, kf, kw, rows, best) in contention_cases().items():
        for form in (0, 1):
            r, b, n = both(pts, descs, kf, form=form, **kw)
            assert (r, b) == (rows, best) and n == sum(1 for x in best if x >= 0), (name, form, r, b)


def reversal_case():
    """A's and B's best row is r1, B's second best and C's best is r2, r3 is everybody's last.  -> points, descs, kf"""
    rng = np.random.default_rng(6)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    e, g = flip_bits(rng, d, 10), flip_bits(rng, d, 20)
    P = point_at_pixel(300.0, 200.0)
    descs = np.stack([d, flip_bits(rng, d, 1), flip_bits(rng, e, 1)])
    return stack(P, P, P), descs, kf_of([300, 301, 299.5], [200, 200, 201], [d, e, g])


def test_known_answer_reversing_the_list_changes_the_answer():
    """In list order A takes r1, B falls to r2 and C, whose best r2 is gone, to r3.  Reversed, C comes first and takes r2, B takes
    r1, and A, whose r1 and r2 are gone, is left with r3."""
    pts, descs, kf = reversal_case()
    dist = hamming(descs[:, None, :], kf.desc[None, :, :])
    assert dist.argmin(1).tolist() == [0, 0, 1] and (dist <= 50).all()
    assert both(pts, descs, kf) == ([0, 1, 2], [0, 1, 2], 3)
    assert both(pts[::-1].copy(), descs[::-1].copy(), kf) == ([1, 0, 2], [1, 0, 2], 3)       # entries: C, B, A


def test_known_answer_thresholds():
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    P = point_at_pixel(300.0, 200.0)
    for ratio, inside, outside in ((1.0, (49, 50), (51,)), (1.5, (74, 75), (76,)), (1.01, (50,), (51,))):
        for nbits in inside + outside:
            kf = kf_of([300], [200], [flip_bits(rng, d, nbits)])
            ex = Counter()
            r, b, n = both(P, d[None], kf, ratio=ratio, exits=ex)
            want = 0 if nbits in inside else -1
            assert b == [want] and n == (want == 0), (ratio, nbits)
            assert ex["match" if want == 0 else "above_threshold"] == 1
    assert dist_limit(1.01) == f32(50.5) and dist_limit(1.5) == f32(75.0)


def forms_differ(seed=11, nmp=400):
    """Points of a seeded scene whose u or v differ in their bits between the two projection forms (both inside the image)."""
    rng = np.random.default_rng(seed)
    pts, descs = make_points(rng, nmp)
    pose = make_pose(rot_xyz(0.02, -0.03, 0.01), [0.3, -0.2, 0.4])
    kf = KF(np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, np.int32), np.zeros((0, 32), np.uint8), np.zeros(0, f32), pose)
    ok0, u0, v0, lev0, rad0 = survivors(pts, kf, CAM, 3.0, 0)
    ok1, u1, v1, lev1, rad1 = survivors(pts, kf, CAM, 3.0, 1)
    differ = ok0 & ok1 & ((u0.view(np.uint32) != u1.view(np.uint32)) | (v0.view(np.uint32) != v1.view(np.uint32)))
    return pts, descs, pose, differ, (u0, v0), (u1, v1), lev0, rad0


def boundary_case():
    """A point whose u differs between the forms, and ONE keypoint at the edge of its window: a float x with |x - u| < radius
    under one form and not under the other.  -> points[1], descs[1], kf, (best under form 0, best under form 1)"""
    pts, descs, pose, differ, (u0, v0), (u1, v1), level, radius = forms_differ()
    for i in np.nonzero(differ & (u0 != u1))[0]:
        r = radius[i]
        for sign in (1.0, -1.0):
            x = f32(f32(u0[i]) + f32(sign) * r)
            for _ in range(8):
                x = np.nextafter(x, f32(-np.inf))
            for _ in range(16):
                in0, in1 = abs(f32(x - u0[i])) < r, abs(f32(x - u1[i])) < r
                if in0 != in1 and 1.0 < x < 740.0:
                    kf = KF(np.array([x], f32), np.array([v0[i]], f32), np.array([level[i]], np.int32), descs[i][None].copy(),
                            np.full(1, -1, f32), pose)
                    return pts[i:i + 1], descs[i:i + 1], kf, (0 if in0 else -1, 0 if in1 else -1)
                x = np.nextafter(x, f32(np.inf))
    raise AssertionError("no boundary keypoint separates the two forms")


def test_the_two_projection_forms_round_differently():
    pts, descs, pose, differ, uv0, uv1, _, _ = forms_differ()
    print("%d of %d points differ in u or v between the forms" % (differ.sum(), len(pts)))
    assert differ.sum() > 0
    P, d, kf, (want0, want1) = boundary_case()
    assert want0 != want1
    assert both(P, d, kf, form=0)[1] == [want0]
    assert both(P, d, kf, form=1)[1] == [want1]


def test_the_binding_declares_the_entry_point():
    from pli_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert re.search(r"pli_status\s+pli_search_by_projection_sim3\s*\(", hdr)
    assert "pli_search_by_projection_sim3" in capi._PROTOS and len(capi._PROTOS["pli_search_by_projection_sim3"][1]) == 19
    assert capi.FUSE_POINT_DT == FUSE_POINT_DT
    from pli_slam_amd.frontend import Frontend
    assert hasattr(Frontend, "search_by_projection_sim3")
    lib = C.CDLL(capi.LIB_PATH)                                      # the product library exports the symbol
    assert hasattr(lib, "pli_search_by_projection_sim3")


def test_the_adapters_compile_against_stub_types():
    """A syntax check of PliORBmatcher::SearchByProjection (the two reference signatures and the batch form) against the stub
    KeyFrame / MapPoint of the harness."""
    src = os.path.join(ROOT, "tests", "cpp", "sim3_projection_harness.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
