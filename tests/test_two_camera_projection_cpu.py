"""ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for a current frame of two cameras (ORBmatcher.cc:1961-2177
with CurrentFrame.Nleft != -1), restated twice in plain numpy, CPU only:

  two_camera_scalar   the reference's control flow line by line — one loop over the last frame's rows, left camera then right, one
                      array of Nleft + Nright slots, one list of rotation entries — labelling the exit every row takes;
  two_camera_fast     the closed form the kernels of pli_search_by_projection_two_cameras use: every (row, camera) window first,
                      `left_open` from the left windows, then two independent ordered walks, then the joint histogram.

Both stand on helpers_matchers (_cells, _area, three_maxima, hamming, c_round), as search_by_projection there does; neither reads
oracle/ or a kernel.  The constructed scene takes every exit the two-camera branch has; the GPU file compares the product library
with two_camera_scalar on the same tables."""
import os
import subprocess

import numpy as np
import pytest

from helpers_matchers import (GRID_COLS, GRID_ROWS, HISTO_LENGTH, KEYPOINT_DT, PROJ_K, PROJ_QUERY_DT, TH_HIGH, _area, _cells, _flip,
                              c_round, f32, hamming, search_by_projection, three_maxima)

NO_OBS = 2                       # PLI_PROJ_NO_OBSERVATIONS
BOUNDS = (0.0, 640.0, 0.0, 480.0)
PROJ_LDS_KEYPOINTS = 15360

# ---- the argument and capacity errors, as data for the GPU file ------------------------------------------------------------------
PLI_OK, PLI_ERR_INVALID, PLI_ERR_CAPACITY = 0, -1, -3
CAPACITY_CASES = [(PROJ_LDS_KEYPOINTS // 2, PROJ_LDS_KEYPOINTS // 2, PLI_OK), (PROJ_LDS_KEYPOINTS, 0, PLI_OK),      # (nleft, nright, status)
                  (PROJ_LDS_KEYPOINTS // 2 + 1, PROJ_LDS_KEYPOINTS // 2, PLI_ERR_CAPACITY), (0, PROJ_LDS_KEYPOINTS + 1, PLI_ERR_CAPACITY)]
INVALID_VALID_VALUES = [4, 5, -1]            # valid & ~3


def rot_bin(a, b):
    """:2073-2079 (the assert included: the tests keep their angles in [0, 360))"""
    rot = f32(f32(a) - f32(b))
    if rot < 0:
        rot = f32(rot + f32(360.0))
    bn = int(c_round(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH)))))
    if bn == HISTO_LENGTH:
        bn = 0
    assert 0 <= bn < HISTO_LENGTH
    return bn


def _right_queries(q_left, q_right):
    """From q_right only u, v, radius, min_level, max_level are read; valid and angle are the left's."""
    q = np.zeros(len(q_left), PROJ_QUERY_DT)
    for f in ("u", "v", "radius", "min_level", "max_level"):
        q[f] = q_right[f]
    q["valid"], q["angle"] = q_left["valid"], q_left["angle"]
    return q


def two_camera_scalar(q_left, q_right, qdesc, kp_left, desc_left, kp_right, desc_right, bounds, check_ori=True, occ_left=None,
                      occ_right=None):
    """-> nmatches, best_left, best_right, raw_left, raw_right, exits [(left labels, right labels)], call tags."""
    nq, nl, nr = len(q_left), len(kp_left), len(kp_right)
    qr = _right_queries(q_left, q_right)
    cells = (_cells(kp_left, bounds), _cells(kp_right, bounds))
    kps, descs, qs, base = (kp_left, kp_right), (desc_left, desc_right), (q_left, qr), (0, nl)
    entry = np.zeros(nl + nr, bool)                                  # mvpMapPoints[k] && Observations() > 0 at entry
    if occ_left is not None:
        entry[:nl] = np.asarray(occ_left) != 0
    if occ_right is not None:
        entry[nl:] = np.asarray(occ_right) != 0
    taken = entry.copy()
    raw = [np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)]
    holder = {}                                                      # slot -> the row that wrote it last (for the retaken tag)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                     # entries (camera, row): the reference pushes the slot
    cam_hist = np.zeros((2, HISTO_LENGTH), np.int64)
    nmatches = 0
    exits = [None] * nq
    minx, maxx, miny, maxy = (f32(b) for b in bounds)

    def search(cam, i, dry=False):
        """one camera of row i from GetFeaturesInArea on (:2015-2082 / :2094-2147) -> labels"""
        nonlocal nmatches
        Q = qs[cam][i]
        px, py, ingrid, gw, gh = cells[cam]
        tags = []
        idx = _area(Q, kps[cam], px, py, ingrid, bounds, gw, gh, tags)
        if idx is None:
            return ("outside_grid",)
        if idx.size == 0:
            return ("window_empty",)
        d_all = hamming(qdesc[i][None], descs[cam][idx])
        nk = int((d_all <= TH_HIGH).sum())
        if nk in (PROJ_K, PROJ_K + 1):
            tags.append("window_holds_PROJ_K" if nk == PROJ_K else "window_holds_PROJ_K_plus_1")
        slots = idx + base[cam]
        if entry[slots].any():
            tags.append("occupied_at_entry")
        if (taken[slots] & ~entry[slots]).any():
            tags.append("closed_by_earlier_row")
        best_dist, best_idx = 256, -1
        for k, i2 in enumerate(idx.tolist()):                        # :2032-2057 / :2108-2124
            if taken[i2 + base[cam]]:
                continue
            if int(d_all[k]) < best_dist:
                best_dist, best_idx = int(d_all[k]), i2
        if best_idx < 0:
            return (("all_occupied" if entry[slots].all() else "none_free"),) + tuple(tags)
        if best_dist in (TH_HIGH, TH_HIGH + 1):
            tags.append("distance_eq_TH_HIGH" if best_dist == TH_HIGH else "distance_eq_TH_HIGH_plus_1")
        if best_dist > TH_HIGH:
            return (("all_above_TH_HIGH" if int(d_all.min()) > TH_HIGH else "distance_above_TH_HIGH"),) + tuple(tags)
        if dry:
            return ("matched",) + tuple(tags)
        slot = best_idx + base[cam]
        if slot in holder:
            tags.append("retaken_from_row_without_observations")
        holder[slot] = i
        if Q["valid"] & NO_OBS:
            tags.append("map_point_without_observations")            # Observations() == 0: the slot stays available
        else:
            taken[slot] = True
        raw[cam][i] = best_idx
        nmatches += 1
        if check_ori:
            bn = rot_bin(Q["angle"], kps[cam]["angle"][best_idx])
            rot_hist[bn].append((cam, i))
            cam_hist[cam, bn] += 1
        return ("matched",) + tuple(tags)

    for i in range(nq):
        Q = q_left[i]
        if not Q["valid"]:
            exits[i] = (("invalid",), ("skipped",)); continue
        if Q["u"] < minx or Q["u"] > maxx or Q["v"] < miny or Q["v"] > maxy:                  # :2004-2007
            would = search(1, i, dry=True)
            exits[i] = (("outside_bounds",), ("skipped",) + (("would_match",) if would[0] == "matched" else ())); continue
        px, py, ingrid, gw, gh = cells[0]
        idx = _area(Q, kp_left, px, py, ingrid, bounds, gw, gh, [])
        if idx is None or idx.size == 0:                                                          # :2024
            would = search(1, i, dry=True)
            exits[i] = (("window_empty" if idx is not None else "outside_grid",),
                        ("skipped",) + (("would_match",) if would[0] == "matched" else ())); continue
        left = search(0, i)
        right = search(1, i)                                                                      # :2083-2149
        exits[i] = (left, right)

    best = [raw[0].copy(), raw[1].copy()]
    ctags = set()
    if check_ori:
        keep, which = three_maxima([len(h) for h in rot_hist])
        if nmatches:
            ctags.add(which)
        for bn in range(HISTO_LENGTH):
            if bn not in keep:
                for cam, i in rot_hist[bn]:                          # :2167-2171
                    best[cam][i] = -1
                    nmatches -= 1
            elif rot_hist[bn] and not any(cam_hist[c, bn] and bn in three_maxima(list(cam_hist[c]))[0] for c in (0, 1)):
                ctags.add("bin_survives_only_jointly")
            if bn not in keep and any(cam_hist[c, bn] and bn in three_maxima(list(cam_hist[c]))[0] for c in (0, 1)):
                ctags.add("bin_dropped_only_jointly")
    return nmatches, best[0], best[1], raw[0], raw[1], exits, ctags


def _windows(q, qdesc, kp, desc, bounds, gate):
    """every row's GetFeaturesInArea list in walking order with its distances, all rows at once -> lists, dists, open"""
    px, py, ingrid, gw, gh = _cells(kp, bounds)
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    lists, dists, opened = [], [], np.zeros(len(q), bool)
    none = np.zeros(0, np.int64)
    for i, Q in enumerate(q):
        idx = none
        inside = not (Q["u"] < minx or Q["u"] > maxx or Q["v"] < miny or Q["v"] > maxy)
        if Q["valid"] and (inside or not gate):
            a = _area(Q, kp, px, py, ingrid, bounds, gw, gh, [])
            idx = none if a is None else a
        opened[i] = idx.size > 0
        lists.append(idx)
        dists.append(hamming(qdesc[i][None], desc[idx]) if idx.size else np.zeros(0, np.int32))
    return lists, dists, opened


def _walk(q, lists, dists, occ, ncur, allowed):
    """the ordered walk of one camera: the first minimum among the free keypoints of the row's list"""
    taken = np.zeros(ncur, bool) if occ is None else (np.asarray(occ) != 0).copy()
    raw = np.full(len(q), -1, np.int32)
    for i in np.flatnonzero(allowed):
        idx, d = lists[i], dists[i]
        free = ~taken[idx]
        if not free.any():
            continue
        k = int(np.argmin(np.where(free, d, 1 << 20)))
        if d[k] > TH_HIGH:
            continue
        raw[i] = idx[k]
        if not (q["valid"][i] & NO_OBS):
            taken[idx[k]] = True
    return raw


def two_camera_fast(q_left, q_right, qdesc, kp_left, desc_left, kp_right, desc_right, bounds, check_ori=True, occ_left=None,
                    occ_right=None):
    """-> nmatches, best_left, best_right, raw_left, raw_right"""
    qr = _right_queries(q_left, q_right)
    ll, dl, left_open = _windows(q_left, qdesc, kp_left, desc_left, bounds, True)
    lr, dr, _ = _windows(qr, qdesc, kp_right, desc_right, bounds, False)
    raw_l = _walk(q_left, ll, dl, occ_left, len(kp_left), left_open)
    raw_r = _walk(qr, lr, dr, occ_right, len(kp_right), left_open)
    best_l, best_r = raw_l.copy(), raw_r.copy()
    if check_ori:
        bins_l = np.array([rot_bin(q_left["angle"][i], kp_left["angle"][b]) if b >= 0 else -1 for i, b in enumerate(raw_l)], np.int64)
        bins_r = np.array([rot_bin(q_left["angle"][i], kp_right["angle"][b]) if b >= 0 else -1 for i, b in enumerate(raw_r)], np.int64)
        hist = np.bincount(np.concatenate([bins_l[bins_l >= 0], bins_r[bins_r >= 0]]), minlength=HISTO_LENGTH)
        keep, _ = three_maxima([int(h) for h in hist])
        best_l[~np.isin(bins_l, keep)] = -1
        best_r[~np.isin(bins_r, keep)] = -1
    return int((best_l >= 0).sum() + (best_r >= 0).sum()), best_l, best_r, raw_l, raw_r


# ---- tables -------------------------------------------------------------------------------------------------------------------------
class Scene:
    """Rows on a 40-pixel lattice of a 640 x 480 frame, radius 10, the right projection 3 px left of the left one: the items do
    not see each other.  The lattice fills y <= 300; the dense windows live below it."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ql, self.qr, self.qd = [], [], []
        self.kp, self.d, self.occ = ([], []), ([], []), ([], [])
        self.slot = 0
        self.mark = {}

    def place(self):
        s = self.slot; self.slot += 1
        assert s < 16 * 8
        return 20.0 + 40 * (s % 16), 20.0 + 40 * (s // 16)

    def row(self, u, v, ur=None, vr=None, radius=10.0, lo=0, hi=-1, angle=0.0, valid=1, like=None, bits=0, name=None):
        """a last-frame row; `like`: its descriptor is row `like`'s with `bits` bits flipped"""
        self.ql.append((u, v, radius, 0.0, lo, hi, angle, valid))
        self.qr.append((u - 3.0 if ur is None else ur, v if vr is None else vr, radius, 0.0, lo, hi, 0.0, 0))
        self.qd.append(self.rng.integers(0, 256, 32, dtype=np.uint8) if like is None else _flip(self.qd[like], bits))
        if name:
            self.mark[name] = len(self.ql) - 1
        return len(self.ql) - 1

    def key(self, cam, x, y, of, bits=0, octave=0, angle=0.0, occ=0):
        self.kp[cam].append((x, y, octave, angle)); self.d[cam].append(_flip(self.qd[of], bits)); self.occ[cam].append(occ)
        return len(self.kp[cam]) - 1

    def item(self, left=None, right=None, name=None, **kw):
        """one row with at most one keypoint per camera at its projection; left / right: bits flipped, or None for no keypoint"""
        u, v = self.place()
        i = self.row(u, v, name=name, **kw)
        if left is not None:
            self.key(0, u, v, i, left)
        if right is not None:
            self.key(1, u - 3.0, v, i, right)
        return i

    def tables(self, bounds=BOUNDS):
        def q_of(rows):
            q = np.zeros(len(rows), PROJ_QUERY_DT)
            for i, r in enumerate(rows):
                q[i] = r
            return q

        def kp_of(rows):
            kp = np.zeros(len(rows), KEYPOINT_DT)
            for i, (x, y, o, a) in enumerate(rows):
                kp["x"][i], kp["y"][i], kp["octave"][i], kp["angle"][i] = x, y, o, a
            kp["size"] = 31
            return kp
        return dict(q_left=q_of(self.ql), q_right=q_of(self.qr), qdesc=np.array(self.qd, np.uint8).reshape(len(self.ql), 32),
                    kp_left=kp_of(self.kp[0]), desc_left=np.array(self.d[0], np.uint8).reshape(len(self.kp[0]), 32),
                    kp_right=kp_of(self.kp[1]), desc_right=np.array(self.d[1], np.uint8).reshape(len(self.kp[1]), 32),
                    occ_left=np.array(self.occ[0], np.uint8), occ_right=np.array(self.occ[1], np.uint8), bounds=bounds)


def constructed_scene():
    """-> tables, marks (row numbers by name).  One scene that takes every exit of the two-camera branch."""
    S = Scene(71)
    # the geometric skip: the right camera is not searched although it would match
    i = S.row(-3.0, 100.0, ur=610.0, vr=300.0, name="left_out_of_bounds"); S.key(1, 610.0, 300.0, i, 3)
    S.item(None, 3, name="left_window_empty")
    # ... and what does NOT close the right camera
    u, v = S.place(); i = S.row(u, v, name="left_all_occupied"); S.key(0, u, v, i, 2, occ=1); S.key(1, u - 3, v, i, 3)
    S.item(150, 3, name="left_all_above_TH_HIGH")
    S.item(2, 4, name="both_matched")
    S.item(2, None, name="right_window_empty")
    u, v = S.place(); i = S.row(u, v, name="right_occupied_at_entry"); S.key(0, u, v, i, 2); S.key(1, u - 3, v, i, 3, occ=1)
    # a keypoint taken by the row before, on each camera: the second row gets the farther one (left) / nothing (right)
    u, v = S.place(); i = S.row(u, v, name="taken_first"); S.key(0, u, v, i, 2); S.key(0, u + 3, v, i, 30); S.key(1, u - 3, v, i, 2)
    S.row(u + 1, v, like=i, bits=1, name="taken_second")
    # no observations: the keypoints stay available and the row behind takes them again, on both cameras
    u, v = S.place(); i = S.row(u, v, valid=1 | NO_OBS, name="no_observations"); S.key(0, u, v, i, 2); S.key(1, u - 3, v, i, 2)
    S.row(u + 1, v, like=i, bits=1, name="retakes")
    S.item(3, 100, name="right_dist_100")
    S.item(3, 101, name="right_dist_101")
    S.item(100, 3, name="left_dist_100")
    S.item(101, 3, name="left_dist_101")
    # right projections outside the grid: GetFeaturesInArea's early returns (the right projection has no image gate)
    S.item(2, None, ur=5000.0, name="right_beyond_max_col")
    S.item(2, None, ur=-500.0, name="right_below_min_col")
    S.item(2, None, vr=5000.0, name="right_beyond_max_row")
    S.item(2, None, vr=-500.0, name="right_below_min_row")
    S.item(2, 2, valid=0, name="invalid")
    # the level gate decides "empty": a left keypoint outside the levels leaves the window empty
    u, v = S.place(); i = S.row(u, v, lo=2, hi=4, name="left_empty_by_level"); S.key(0, u, v, i, 2, octave=5); S.key(1, u - 3, v, i, 2, octave=3)
    # the joint histogram (rot / 30 rounds to the bin): bins 1, 2 hold four left matches each, bins 4, 5 four right ones, bin 3
    # three of each — fourth in either camera's own histogram, second in the joint one.  Everything else sits in bin 0 (35 entries:
    # four is more than a tenth of it).
    for rot, cams in ((30.0, "L"), (60.0, "L"), (120.0, "R"), (150.0, "R")):
        for _ in range(4):
            S.item(2 if cams == "L" else 150, None if cams == "L" else 2, angle=rot)
    for k in range(3):
        S.item(2, None, angle=90.0, name="bin3_left_%d" % k)
        S.item(150, 2, angle=90.0, name="bin3_right_%d" % k)
    # windows of exactly PROJ_K and PROJ_K + 1 candidates on each camera, each with a row behind it that finds the best one taken
    for n, (cam, n_c) in enumerate(((0, PROJ_K), (0, PROJ_K + 1), (1, PROJ_K), (1, PROJ_K + 1))):
        u, v = 80.0 + 160 * n, 420.0
        i = S.row(u, v, radius=30.0, name="dense_%s_%d" % ("LR"[cam], n_c))
        off = 0.0 if cam == 0 else -3.0
        for k in range(n_c):
            S.key(cam, u + off - 9 + 2 * (k % 9), v - 9 + 2 * (k // 9), i, 10 + (k * 7) % 50, octave=k % 3)
        S.key(cam, u + off + 5, v + 5, i, 150)                       # in the window, beyond TH_HIGH: not a candidate
        S.key(1 - cam, u - 3.0 - off, v, i, 3)                       # the other camera: one keypoint
        S.row(u + 1, v + 1, radius=30.0, like=i, bits=2)
    return S.tables(), S.mark


def hand_worked_cases():
    """-> [(name, tables, check_ori, nmatches, best_left, best_right, raw_left, raw_right)], the expectations written by hand"""
    cases = []
    S = Scene(72); S.item(2, 4)
    cases.append(("one_row_both_cameras", S.tables(), True, 2, [0], [0], [0], [0]))
    S = Scene(73); i = S.row(-3.0, 100.0, ur=300.0, vr=100.0); S.key(1, 300.0, 100.0, i, 3); S.key(0, 1.0, 100.0, i, 3)
    cases.append(("left_out_of_bounds_closes_the_right", S.tables(), True, 0, [-1], [-1], [-1], [-1]))
    S = Scene(74); S.item(None, 3)
    cases.append(("left_window_empty_closes_the_right", S.tables(), True, 0, [-1], [-1], [-1], [-1]))
    S = Scene(75); u, v = S.place(); i = S.row(u, v); S.key(0, u, v, i, 2, occ=1); S.key(1, u - 3, v, i, 3)
    cases.append(("left_occupied_leaves_the_right_open", S.tables(), True, 1, [-1], [0], [-1], [0]))
    S = Scene(76); u, v = S.place(); i = S.row(u, v); S.key(0, u, v, i, 2); S.key(1, u - 3, v, i, 2); S.row(u + 1, v, like=i, bits=1)
    cases.append(("second_row_finds_both_taken", S.tables(), True, 2, [0, -1], [0, -1], [0, -1], [0, -1]))
    S = Scene(77); u, v = S.place(); i = S.row(u, v, valid=3); S.key(0, u, v, i, 2); S.key(1, u - 3, v, i, 2); S.row(u + 1, v, like=i, bits=1)
    cases.append(("no_observations_is_taken_again", S.tables(), True, 4, [0, 0], [0, 0], [0, 0], [0, 0]))
    # bins: 0 (two entries, one per camera), 3, 6, 9 (one each): the three fullest are 0, 3, 6 — equal sizes go to the lower bin
    S = Scene(78); S.item(2, 2); S.item(2, None, angle=90.0); S.item(150, 2, angle=180.0); S.item(2, None, angle=270.0)
    cases.append(("joint_histogram_drops_the_fourth_bin", S.tables(), True, 4, [0, 1, -1, -1], [0, -1, 1, -1], [0, 1, -1, 3], [0, -1, 1, -1]))
    cases.append(("no_orientation_check_keeps_it", S.tables(), False, 5, [0, 1, -1, 3], [0, -1, 1, -1], [0, 1, -1, 3], [0, -1, 1, -1]))
    S = Scene(79); S.item(3, 100); S.item(3, 101)
    cases.append(("th_high_is_inclusive", S.tables(), True, 3, [0, 1], [0, -1], [0, 1], [0, -1]))
    return cases


def random_tables(seed, nq=400, nl=350, nr=300, bounds=BOUNDS, dense=False):
    """Random rows against two random cameras.  dense: wide windows over close descriptors, so that many windows hold more than
    PROJ_K candidates within TH_HIGH on either camera (the kernels' rescan path)."""
    rng = np.random.default_rng(seed)

    def camera(n):
        kp = np.zeros(n, KEYPOINT_DT)
        kp["x"] = rng.uniform(0, 640, n).astype(np.float32); kp["y"] = rng.uniform(0, 480, n).astype(np.float32)
        kp["octave"] = rng.integers(0, 8, n); kp["angle"] = rng.uniform(0, 360, n).astype(np.float32); kp["size"] = 31
        return kp
    kl, kr = camera(nl), camera(nr)
    base = rng.integers(0, 256, 32, dtype=np.uint8)

    def descs(n):
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if dense:
            d[:, 8:] = base[8:]
        return d
    dl, dr = descs(nl), descs(nr)
    ql, qr = np.zeros(nq, PROJ_QUERY_DT), np.zeros(nq, PROJ_QUERY_DT)
    sl, sr = rng.integers(0, max(nl, 1), nq), rng.integers(0, max(nr, 1), nq)
    if nl:
        ql["u"] = kl["x"][sl] + rng.uniform(-4, 4, nq).astype(np.float32); ql["v"] = kl["y"][sl] + rng.uniform(-4, 4, nq).astype(np.float32)
    else:
        ql["u"] = rng.uniform(0, 640, nq).astype(np.float32); ql["v"] = rng.uniform(0, 480, nq).astype(np.float32)
    # a tenth of the left projections miss every keypoint or the image; a tenth of the right ones leave the grid
    miss = rng.random(nq) < 0.1
    ql["u"][miss] = rng.uniform(-60, 700, int(miss.sum())).astype(np.float32)
    if nr:
        qr["u"] = kr["x"][sr] + rng.uniform(-4, 4, nq).astype(np.float32); qr["v"] = kr["y"][sr] + rng.uniform(-4, 4, nq).astype(np.float32)
    far = rng.random(nq) < 0.1
    qr["u"][far] = rng.choice(np.array([-900.0, -20.0, 660.0, 2000.0], np.float32), int(far.sum()))
    radius = (rng.uniform(60, 200, nq) if dense else np.where(rng.random(nq) < 0.7, rng.uniform(5, 30, nq), rng.uniform(40, 90, nq)))
    ql["radius"] = qr["radius"] = radius.astype(np.float32)
    ql["min_level"] = qr["min_level"] = rng.integers(-1, 3, nq)
    ql["max_level"] = qr["max_level"] = np.where(rng.random(nq) < 0.3, -1, ql["min_level"] + rng.integers(0, 6, nq))
    src_angle = kl["angle"][sl] if nl else rng.uniform(0, 360, nq).astype(np.float32)
    ql["angle"] = (src_angle + rng.choice([0.0, 0.0, 0.0, 90.0, 200.0], nq)).astype(np.float32) % 360
    ql["valid"] = np.where(rng.random(nq) < 0.93, np.where(rng.random(nq) < 0.15, 3, 1), 0)
    qr["valid"], qr["angle"], qr["ur"] = 7, np.float32(np.nan), np.float32(np.nan)                   # never read
    if dense:
        qd = np.broadcast_to(base, (nq, 32)).copy()
        qd[:, :4] ^= rng.integers(0, 256, (nq, 4), dtype=np.uint8)
    else:                                                                                                # near one camera's keypoint
        pick = rng.random(nq) < 0.5
        anyd = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        qd = np.where(pick[:, None], dl[sl] if nl else anyd, dr[sr] if nr else anyd).copy()
        flip = rng.random((nq, 32)) < 0.1
        qd[flip] ^= rng.integers(0, 256, (nq, 32), dtype=np.uint8)[flip] & 0x0F
    return dict(q_left=ql, q_right=qr, qdesc=qd, kp_left=kl, desc_left=dl, kp_right=kr, desc_right=dr,
                occ_left=(rng.random(nl) < 0.2).astype(np.uint8), occ_right=(rng.random(nr) < 0.2).astype(np.uint8), bounds=bounds)


GRID_INSIDE_BOUNDS = (100.0, 540.0, 80.0, 400.0)      # keypoints outside these bounds are in no cell (PosInGrid)

_EXPECTED = {}


def expected(name, make, check_ori=True, with_occ=True):
    """two_camera_scalar on a named table set, computed once and shared"""
    key = (name, check_ori, with_occ)
    if key not in _EXPECTED:
        T = make() if callable(make) else make
        kw = {k: T[k] for k in ("q_left", "q_right", "qdesc", "kp_left", "desc_left", "kp_right", "desc_right", "bounds")}
        occ = dict(occ_left=T["occ_left"], occ_right=T["occ_right"]) if with_occ else {}
        _EXPECTED[key] = (T, two_camera_scalar(check_ori=check_ori, **kw, **occ))
    return _EXPECTED[key]


def _fast(T, check_ori=True, with_occ=True):
    kw = {k: T[k] for k in ("q_left", "q_right", "qdesc", "kp_left", "desc_left", "kp_right", "desc_right", "bounds")}
    occ = dict(occ_left=T["occ_left"], occ_right=T["occ_right"]) if with_occ else {}
    return two_camera_fast(check_ori=check_ori, **kw, **occ)


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5]))


# ---- tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_ori", [True, False])
def test_the_two_restatements_agree_on_the_constructed_scene(check_ori):
    T, want = expected("scene", lambda: constructed_scene()[0], check_ori)
    assert _same(want, _fast(T, check_ori))
    assert want[0] > 30


def test_the_hand_worked_cases():
    for name, T, check_ori, n, bl, br, rl, rr in hand_worked_cases():
        for got in (expected("hand_" + name, T, check_ori)[1], _fast(T, check_ori)):
            assert got[0] == n, name
            for g, w in zip(got[1:5], (bl, br, rl, rr)):
                assert g.tolist() == w, (name, g, w)


def test_the_constructed_scene_takes_every_exit():
    """Counts on the scene (51 rows):
    left outside the bounds, right would match: 1; left window empty, right would match: 2 (one by the level gate);
    left all occupied, right matched: 1; left all above TH_HIGH, right matched: 13; both matched: 10; left matched and right
    window empty: 12; right occupied at entry: 1; closed by an earlier row: left 5, right 5; a row without observations whose right
    keypoint is retaken: 1; distance 100 / 101: right 1 / 1, left 1 / 1; windows of PROJ_K / PROJ_K + 1: two rows each on either
    camera (the row that fills the window and the one behind it); right projection outside the grid: 4; bin 3 survives only jointly
    (six entries, three per camera), bins 2, 4, 5 are dropped only jointly; 57 accepts (35 in bin 0), 12 of them filtered."""
    T, (n, bl, br, rl, rr, exits, ctags) = expected("scene", lambda: constructed_scene()[0])
    mark = constructed_scene()[1]

    def count(pred):
        return sum(1 for e in exits if pred(e[0], e[1]))
    assert len(exits) == 51
    assert count(lambda L, R: L[0] == "outside_bounds" and R == ("skipped", "would_match")) == 1
    assert count(lambda L, R: L[0] == "window_empty" and R == ("skipped", "would_match")) == 2
    assert count(lambda L, R: L[0] == "all_occupied" and R[0] == "matched") == 1
    assert count(lambda L, R: L[0] == "all_above_TH_HIGH" and R[0] == "matched") == 13
    assert count(lambda L, R: L[0] == "matched" and R[0] == "matched") == 10
    assert count(lambda L, R: L[0] == "matched" and R[0] == "window_empty") == 12
    assert count(lambda L, R: R[0] == "all_occupied" and "occupied_at_entry" in R) == 1
    assert count(lambda L, R: "closed_by_earlier_row" in L) == 5 and count(lambda L, R: "closed_by_earlier_row" in R) == 5
    i = mark["no_observations"]
    assert "map_point_without_observations" in exits[i][1] and "retaken_from_row_without_observations" in exits[i + 1][1]
    assert rr[i] == rr[i + 1] >= 0 and rl[i] == rl[i + 1] >= 0
    assert count(lambda L, R: "retaken_from_row_without_observations" in R) == 1
    assert count(lambda L, R: R[0] == "matched" and "distance_eq_TH_HIGH" in R) == 1
    assert count(lambda L, R: R[0] != "matched" and "distance_eq_TH_HIGH_plus_1" in R) == 1
    assert count(lambda L, R: L[0] == "matched" and "distance_eq_TH_HIGH" in L) == 1
    assert count(lambda L, R: L[0] != "matched" and "distance_eq_TH_HIGH_plus_1" in L) == 1
    for side in (0, 1):
        assert sum(1 for e in exits if "window_holds_PROJ_K" in e[side]) == 2
        assert sum(1 for e in exits if "window_holds_PROJ_K_plus_1" in e[side]) == 2
    assert count(lambda L, R: L[0] == "matched" and R[0] == "outside_grid") == 4
    assert "bin_survives_only_jointly" in ctags and "bin_dropped_only_jointly" in ctags and "maxima_three_kept" in ctags
    for k in range(3):
        assert bl[mark["bin3_left_%d" % k]] >= 0 and br[mark["bin3_right_%d" % k]] >= 0
    assert (rl >= 0).sum() + (rr >= 0).sum() == 57 and n == 45       # bins 2, 4 and 5 are filtered: 12 entries


def test_two_runs_of_the_one_camera_search_cannot_express_the_call():
    """One search_by_projection per camera (what an integrator could call before) differs from the two-camera search on the scene:
    through the skip (it searches the right camera of rows whose left search left early) and through the histogram (each run
    filters with its own three maxima)."""
    T, (n, bl, br, rl, rr, exits, ctags) = expected("scene", lambda: constructed_scene()[0])
    mark = constructed_scene()[1]
    qr = _right_queries(T["q_left"], T["q_right"])
    none_l, none_r = np.full(len(T["kp_left"]), -1, np.float32), np.full(len(T["kp_right"]), -1, np.float32)
    n_l, best_l, raw_l, _, _ = search_by_projection(T["q_left"], T["qdesc"], T["kp_left"], T["desc_left"], none_l, T["bounds"], True, T["occ_left"])
    n_r, best_r, raw_r, _, _ = search_by_projection(qr, T["qdesc"], T["kp_right"], T["desc_right"], none_r, T["bounds"], True, T["occ_right"])
    assert np.array_equal(raw_l, rl)                                 # the left walk alone is the one-camera search
    for name in ("left_out_of_bounds", "left_window_empty", "left_empty_by_level"):          # the skip
        assert raw_r[mark[name]] >= 0 and rr[mark[name]] == -1, name
    for k in range(3):                                                                       # the histogram
        assert best_l[mark["bin3_left_%d" % k]] == -1 and bl[mark["bin3_left_%d" % k]] >= 0
        assert best_r[mark["bin3_right_%d" % k]] == -1 and br[mark["bin3_right_%d" % k]] >= 0
    assert not np.array_equal(best_l, bl) and not np.array_equal(best_r, br)
    assert n_l + n_r != n


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_two_restatements_agree_on_random_tables(seed):
    T, want = expected("random_%d" % seed, lambda: random_tables(seed))
    assert _same(want, _fast(T))
    skipped = sum(1 for e in want[5] if e[1][:1] == ("skipped",) and e[0][0] != "invalid")
    assert want[0] > 50 and skipped > 10 and (want[3] >= 0).sum() + (want[4] >= 0).sum() > want[0]


def test_the_two_restatements_agree_on_dense_windows_and_on_bounds_inside_the_image():
    T, want = expected("dense", lambda: random_tables(5, nq=60, nl=300, nr=260, dense=True))
    assert _same(want, _fast(T))
    over = [sum(1 for i in range(len(T["q_left"])) if (hamming(T["qdesc"][i][None], T[d]) <= TH_HIGH).sum() > PROJ_K) for d in ("desc_left", "desc_right")]
    assert min(over) > 0 and want[0] > 20
    T, want = expected("inside", lambda: random_tables(6, bounds=GRID_INSIDE_BOUNDS))
    assert _same(want, _fast(T))
    for kp in (T["kp_left"], T["kp_right"]):
        assert (~_cells(kp, GRID_INSIDE_BOUNDS)[2]).sum() > 50
    assert want[0] > 20
    for with_occ in (True, False):
        T, want = expected("random_1", lambda: random_tables(1), True, with_occ)
        assert _same(want, _fast(T, True, with_occ))


def test_the_error_cases_are_what_the_header_states():
    assert all((nl + nr > PROJ_LDS_KEYPOINTS) == (st == PLI_ERR_CAPACITY) for nl, nr, st in CAPACITY_CASES)
    assert {nl + nr for nl, nr, _ in CAPACITY_CASES} == {PROJ_LDS_KEYPOINTS, PROJ_LDS_KEYPOINTS + 1}
    assert all(v & ~3 for v in INVALID_VALID_VALUES)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pli_frontend.h")).read()
    doc = header[header.index("Frame-to-frame tracking of a two-camera frame"):header.index("pli_status pli_search_by_projection_two_cameras")]
    assert "nleft + nright <= %d" % PROJ_LDS_KEYPOINTS in doc and "PLI_ERR_CAPACITY" in doc and "`ur` is read on neither side" in doc


def test_two_camera_search_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the first library call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the same
    program runs.  Either way it builds and links against the product library."""
    import torch
    from test_cpp_two_camera_search import build, make_world, write_input
    exe = build(str(tmp_path))
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, make_world(np.random.default_rng(1), nlast=40, nl=30, nr=25, nmp=40))
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
