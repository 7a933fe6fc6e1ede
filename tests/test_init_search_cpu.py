"""Monocular initialisation's ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
(ORBmatcher.cc:706-821; Tracking.cc:2109-2110: matcher (0.9, true), window 100) restated twice in Python, CPU only:

  init_search_scalar  the reference's control flow, line by line: the grid lists of Frame::AssignFeaturesToGrid / PosInGrid,
                      Frame::GetFeaturesInArea's early returns and loops (Frame.cc:774-855), the running best / second-best over
                      the candidates that vMatchedDistance does not leave out, the eviction, rotHist as lists that nothing ever
                      leaves, ComputeThreeMaxima, the filter over the lists, the update of vbPrevMatched.  It counts every exit.
  init_search_fast    the closed form pli_search_for_initialization uses: per i1 the keys (distance, cell column, cell row, index)
                      of its window, pruned to the distances that can bear on a decision (dist_limit) and sorted; the ordered walk
                      drops the left-out keys and reads best and second-best off the front; a histogram of counts; the filter by
                      recomputing the bin of the entries that are left.

What differs from the Sim3 and relocalisation searches: a row of F2 is not closed once taken.  Its state is (vMatchedDistance,
vnMatches21); a later i1 with a strictly smaller distance takes it again and evicts the earlier owner, an equal distance does not,
and a left-out candidate is neither best nor second-best.  The acceptance is a float comparison (45 against a second-best of 50 at
0.9f is rejected).  The histogram counts evicted entries.  tests/test_init_search_gpu.py compares the device with these exactly.

Exits of the constructed scene (SCENE_SEED, window 100, ratio 0.9; printed by test_the_constructed_scene_takes_every_exit):
level1 104, empty_window 52, left_out 1993, new_best 959, new_second 577, above_th_low 64, ratio_rejected 6, eviction 33,
filtered 30, filtered_already_evicted 9; 141 matches after the walk, 111 after the filter."""
import ctypes as C
import math
import os
import re
from collections import Counter, namedtuple

import numpy as np

from helpers_matchers import GRID_COLS, GRID_ROWS, HISTO_LENGTH, KEYPOINT_DT, c_round, hamming, three_maxima

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INT_MAX = int(np.iinfo(np.int32).max)
TH_LOW = 50
T = namedtuple("T", "x y octave desc angle")                          # one frame's table: mvKeysUn, mDescriptors
BOUNDS = (0.0, 752.0, 0.0, 480.0)                                     # mnMinX, mnMaxX, mnMinY, mnMaxY
EXITS = ("level1", "empty_window", "left_out", "new_best", "new_second", "above_th_low", "ratio_rejected", "eviction", "filtered",
         "filtered_already_evicted")
FACTOR = f32(1.0) / f32(HISTO_LENGTH)
SCENE_SEED = 3


def table(x, y, desc, octave=None, angle=None):
    n = len(x)
    return T(np.asarray(x, f32), np.asarray(y, f32), np.zeros(n, np.int32) if octave is None else np.asarray(octave, np.int32),
             np.asarray(desc, np.uint8).reshape(n, 32), np.zeros(n, f32) if angle is None else np.asarray(angle, f32))


def keypoints(t):
    kp = np.zeros(len(t.x), KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["angle"] = t.x, t.y, t.octave, t.angle
    kp["size"] = 31.0
    return kp


def points_of(t):
    """mvbPrevMatched[i] = mInitialFrame.mvKeysUn[i].pt (Tracking.cc:2072-2074)"""
    return np.stack([t.x, t.y], 1).astype(f32)


def rot_bin(a, b, trunc=False):
    """:776-781 (trunc: the misreading `int bin = rot * factor`)"""
    rot = f32(f32(a) - f32(b))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = int(f32(rot * FACTOR)) if trunc else int(c_round(f32(rot * FACTOR)))
    return 0 if b == HISTO_LENGTH else b


def grid_scale(bounds):
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    return f32(f32(GRID_COLS) / f32(maxx - minx)), f32(f32(GRID_ROWS) / f32(maxy - miny))


# ---- the reference's control flow ----------------------------------------------------------------------------------------------

def assign_features_to_grid(t, bounds):
    """Frame::AssignFeaturesToGrid with PosInGrid (Frame.cc:845-855): mGrid[column][row], index order within a cell."""
    minx, _, miny, _ = (f32(b) for b in bounds)
    gw, gh = grid_scale(bounds)
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
    for i in range(len(t.x)):
        px = int(c_round(f32(f32(t.x[i] - minx) * gw)))
        py = int(c_round(f32(f32(t.y[i] - miny) * gh)))
        if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
            continue
        grid[px][py].append(i)
    return grid


def features_in_area(t, grid, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cc:774-843)"""
    minx, _, miny, _ = (f32(b) for b in bounds)
    gw, gh = grid_scale(bounds)
    x, y, r = f32(x), f32(y), f32(r)
    out = []
    c0 = max(0, int(math.floor(f32(f32(f32(x - minx) - r) * gw))))
    if c0 >= GRID_COLS:
        return out
    c1 = min(GRID_COLS - 1, int(math.ceil(f32(f32(f32(x - minx) + r) * gw))))
    if c1 < 0:
        return out
    r0 = max(0, int(math.floor(f32(f32(f32(y - miny) - r) * gh))))
    if r0 >= GRID_ROWS:
        return out
    r1 = min(GRID_ROWS - 1, int(math.ceil(f32(f32(f32(y - miny) + r) * gh))))
    if r1 < 0:
        return out
    check_levels = min_level > 0 or max_level >= 0
    for ix in range(c0, c1 + 1):
        for iy in range(r0, r1 + 1):
            for j in grid[ix][iy]:
                if check_levels:
                    if t.octave[j] < min_level:
                        continue
                    if max_level >= 0 and t.octave[j] > max_level:
                        continue
                if abs(f32(t.x[j] - x)) < r and abs(f32(t.y[j] - y)) < r:
                    out.append(j)
    return out


def init_search_scalar(t1, t2, prev, bounds=BOUNDS, window=100, nnratio=0.9, check_ori=True, exits=None, misread=()):
    """-> raw12 (vnMatches12 after the walk), matches12 (after the filter), nmatches, vbPrevMatched after the update.  misread:
    deliberate misreadings that tests/test_ref_pin_match.py wants rejected ("min_le": <= in the running minimum; "ratio_double":
    the ratio test in double; "left_out_lt": a row is left out only when its holder is strictly closer; "rot_trunc": the rotation
    bin by truncation; "evicted_leaves_histogram": an evicted match is taken out of rotHist; "th_low_strict":
    bestDist < TH_LOW)."""
    exits = Counter() if exits is None else exits
    n1, n2 = len(t1.x), len(t2.x)
    nnratio = f32(nnratio)
    grid = assign_features_to_grid(t2, bounds)
    nmatches = 0
    m12 = [-1] * n1
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    matched_distance = [INT_MAX] * n2
    m21 = [-1] * n2
    for i1 in range(n1):
        level1 = int(t1.octave[i1])
        if level1 > 0:
            exits["level1"] += 1
            continue
        idx2 = features_in_area(t2, grid, bounds, prev[i1][0], prev[i1][1], window, level1, level1)
        if not idx2:
            exits["empty_window"] += 1
            continue
        d1 = t1.desc[i1]
        best, best2, best_idx = INT_MAX, INT_MAX, -1
        for i2 in idx2:
            dist = int(hamming(d1, t2.desc[i2]))
            if matched_distance[i2] <= dist - ("left_out_lt" in misread):
                exits["left_out"] += 1
                continue
            if dist < best or ("min_le" in misread and dist == best):
                best2, best, best_idx = best, dist, i2
                exits["new_best"] += 1
            elif dist < best2:
                best2 = dist
                exits["new_second"] += 1
        if best <= TH_LOW - ("th_low_strict" in misread):
            if (float(best) < float(best2) * float(nnratio)) if "ratio_double" in misread else f32(best) < f32(f32(best2) * nnratio):
                if m21[best_idx] >= 0:
                    if "evicted_leaves_histogram" in misread:
                        for h in rot_hist:
                            if m21[best_idx] in h:
                                h.remove(m21[best_idx])
                    m12[m21[best_idx]] = -1
                    nmatches -= 1
                    exits["eviction"] += 1
                m12[i1] = best_idx
                m21[best_idx] = i1
                matched_distance[best_idx] = best
                nmatches += 1
                if check_ori:
                    rot_hist[rot_bin(t1.angle[i1], t2.angle[best_idx], "rot_trunc" in misread)].append(i1)
            else:
                exits["ratio_rejected"] += 1
        else:
            exits["above_th_low"] += 1
    raw12 = np.array(m12, np.int32).reshape(n1)
    if check_ori:
        keep, _ = three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i1 in rot_hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nmatches -= 1
                    exits["filtered"] += 1
                else:
                    exits["filtered_already_evicted"] += 1
    new_prev = np.array(prev, f32).reshape(n1, 2).copy()
    for i1 in range(n1):
        if m12[i1] >= 0:
            new_prev[i1] = (t2.x[m12[i1]], t2.y[m12[i1]])
    return raw12, np.array(m12, np.int32).reshape(n1), nmatches, new_prev


# ---- the closed form -----------------------------------------------------------------------------------------------------------

def dist_limit(nnratio):
    """The largest distance a per-i1 list has to hold.  A candidate at distance d bears on a decision only as a best (d <= TH_LOW)
    or as a second-best that rejects some best b <= TH_LOW, which needs (float)d * nnratio <= 50.0f (monotone in d); beyond both it
    acts like a missing second-best.  55 for 0.9."""
    d = TH_LOW
    while d < 256 and f32(f32(d + 1) * f32(nnratio)) <= f32(TH_LOW):
        d += 1
    return d


def init_candidates(t1, t2, prev, bounds, window, limit):
    """Per i1 (None: does not search) the (index, distance) arrays of its window within `limit`, sorted by the key."""
    minx, _, miny, _ = (f32(b) for b in bounds)
    gw, gh = grid_scale(bounds)
    px = np.array([c_round(v) for v in ((t2.x - minx).astype(f32) * gw).astype(f32)], np.int64).reshape(-1)
    py = np.array([c_round(v) for v in ((t2.y - miny).astype(f32) * gh).astype(f32)], np.int64).reshape(-1)
    ok = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS) & (t2.octave == 0)
    r = f32(window)
    lists = []
    for i1 in range(len(t1.x)):
        if t1.octave[i1] != 0:
            lists.append(None)
            continue
        x, y = f32(prev[i1][0]), f32(prev[i1][1])
        c0 = max(0, math.floor(f32(f32(f32(x - minx) - r) * gw)))
        c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(x - minx) + r) * gw)))
        r0 = max(0, math.floor(f32(f32(f32(y - miny) - r) * gh)))
        r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(y - miny) + r) * gh)))
        m = ok & (px >= c0) & (px <= c1) & (py >= r0) & (py <= r1)
        m &= (np.abs((t2.x - x).astype(f32)) < r) & (np.abs((t2.y - y).astype(f32)) < r)
        idx = np.flatnonzero(m)
        d = hamming(t1.desc[i1][None], t2.desc[idx]) if idx.size else np.zeros(0, np.int32)
        idx, d = idx[d <= limit], d[d <= limit]
        o = np.lexsort((idx, py[idx], px[idx], d))
        lists.append((idx[o], d[o].astype(np.int64)))
    return lists


def init_search_fast(t1, t2, prev, bounds=BOUNDS, window=100, nnratio=0.9, check_ori=True, limit=None):
    n1, n2 = len(t1.x), len(t2.x)
    limit = dist_limit(nnratio) if limit is None else limit
    lists = init_candidates(t1, t2, prev, bounds, window, limit)
    md = np.full(n2, INT_MAX, np.int64)
    owner = np.full(n2, -1, np.int64)
    raw = np.full(n1, -1, np.int32)
    hist = [0] * HISTO_LENGTH
    for i1 in range(n1):
        if lists[i1] is None:
            continue
        idx, d = lists[i1]
        live = md[idx] > d
        idx, d = idx[live], d[live]
        if idx.size == 0 or d[0] > TH_LOW:
            continue
        second = int(d[1]) if idx.size > 1 else INT_MAX
        if not f32(d[0]) < f32(f32(second) * f32(nnratio)):
            continue
        b = int(idx[0])
        if owner[b] >= 0:
            raw[owner[b]] = -1
        raw[i1], owner[b], md[b] = b, i1, d[0]
        if check_ori:
            hist[rot_bin(t1.angle[i1], t2.angle[b])] += 1
    m12 = raw.copy()
    if check_ori:
        keep, _ = three_maxima(hist)
        for i1 in np.flatnonzero(raw >= 0):
            if rot_bin(t1.angle[i1], t2.angle[raw[i1]]) not in keep:
                m12[i1] = -1
    new_prev = np.array(prev, f32).reshape(n1, 2).copy()
    hit = m12 >= 0
    new_prev[hit, 0], new_prev[hit, 1] = t2.x[m12[hit]], t2.y[m12[hit]]
    return raw, m12, int(hit.sum()), new_prev


def both(t1, t2, prev=None, exits=None, **kw):
    prev = points_of(t1) if prev is None else prev
    a = init_search_scalar(t1, t2, prev, exits=exits, **kw)
    b = init_search_fast(t1, t2, prev, **kw)
    assert np.array_equal(a[0], b[0]), "raw12 of the two restatements differ"
    assert np.array_equal(a[1], b[1]), "matches12 of the two restatements differ"
    assert a[2] == b[2] and a[3].tobytes() == b[3].tobytes()
    c = init_search_fast(t1, t2, prev, limit=256, **kw)                      # the pruning changes nothing
    assert np.array_equal(b[0], c[0]) and np.array_equal(b[1], c[1])
    return a


# ---- hand-worked cases ---------------------------------------------------------------------------------------------------------

def bits(*runs):
    """A descriptor with ones in the bit runs (lo, n), ..."""
    d = np.zeros(256, np.uint8)
    for lo, n in runs:
        assert lo + n <= 256
        d[lo:lo + n] ^= 1
    return np.packbits(d)


ZERO = bits()


def hand_cases():
    """name -> (t1, t2, prev or None, kwargs, raw12, matches12, nmatches); window 10 unless stated, every angle 0 unless stated."""
    c = {}
    w = dict(window=10)
    # 30 then 20 on one row: i1 = 1 takes the row again and evicts i1 = 0; net one match
    c["eviction"] = (table([100, 102], [100, 100], [bits((0, 30)), bits((0, 20))]), table([101], [100], [ZERO]), None, w,
                     [-1, 0], [-1, 0], 1)
    # i1 = 0 holds row 0 at 20.  i1 = 1 is at 20 from row 0 as well and at 21 from row 1: row 0 is left out, so row 1 is the best
    # with no second-best and is accepted.  Had row 0 counted, it would have been the best (20 against 21: rejected by the ratio)
    # or the second-best (21 against 20: rejected)
    c["equal_distance"] = (table([100, 102], [100, 100], [bits((0, 20)), bits((20, 20))]),
                           table([101, 103], [100, 100], [ZERO, bits((20, 20), (128, 21))]), None, w, [0, 1], [0, 1], 2)
    # i1 = 0 holds row 0 at 10.  For i1 = 1, row 0 is at 22 (left out) and row 1 at 24: accepted.  With row 0 among the candidates
    # the best would be 22 against 24: 22 < 21.6 fails
    c["left_out_would_fail_ratio"] = (table([100, 102], [100, 100], [bits((0, 10)), bits((40, 22))]),
                                      table([101, 103], [100, 100], [ZERO, bits((40, 22), (128, 24))]), None, w, [0, 1], [0, 1], 2)
    # (float)50 * 0.9f == 45.0f: 45 < 45.0f fails; (float)51 * 0.9f == 45.9f: accepted
    c["ratio_45_50_45_51"] = (table([100, 300], [100, 100], [ZERO, ZERO]),
                              table([101, 103, 301, 303], [100, 100, 100, 100],
                                    [bits((0, 45)), bits((100, 50)), bits((0, 45)), bits((100, 51))]), None, w, [-1, 2], [-1, 2], 1)
    c["th_low_50_51"] = (table([100, 300], [100, 100], [ZERO, ZERO]), table([101, 301], [100, 100], [bits((0, 50)), bits((0, 51))]),
                         None, w, [0, -1], [0, -1], 1)
    # the window is strict: |dx| == 10 and |dy| == 10 are outside, 9.5 is inside
    c["window_edge"] = (table([100, 300, 500, 600], [100, 100, 100, 100], [ZERO] * 4),
                        table([110, 300, 509.5, 590], [100, 110, 100, 100], [ZERO] * 4), None, w, [-1, -1, 2, -1], [-1, -1, 2, -1], 1)
    # an F1 keypoint at octave 1 does not search; an F2 keypoint at octave 1 is no candidate
    c["octave_1"] = (table([100, 300, 500], [100, 100, 100], [ZERO] * 3, octave=[1, 0, 0]),
                     table([101, 301, 501], [100, 100, 100], [ZERO] * 3, octave=[0, 1, 0]), None, w, [-1, -1, 2], [-1, -1, 2], 1)
    # round(751.9 * 64 / 752) == 64: PosInGrid puts the keypoint outside the grid, so it is in no cell although it is in the window
    c["outside_the_grid"] = (table([748, 100], [100, 100], [ZERO] * 2), table([751.9, 101], [100, 100], [ZERO] * 2), None, w,
                             [-1, 1], [-1, 1], 1)
    # vbPrevMatched away from the keypoint: the window is around (400, 300); the identical descriptor next to the keypoint is not seen
    c["prev_matched_elsewhere"] = (table([100], [100], [ZERO]), table([100, 402], [100, 301], [ZERO, bits((0, 7))]),
                                   np.array([[400, 300]], f32), w, [1], [1], 1)
    # Bins by F1's angle (F2's are 0): bin 2 three times, bin 4 twice, bin 6 once, bin 8 once plus once evicted.  i1 = 0 (bin 8, at
    # 30) is evicted by i1 = 1 (bin 2, at 20) but stays in rotHist[8], whose size 2 beats bin 6's 1: bins 2, 4, 8 are kept and the
    # entry of bin 6 (i1 = 7) is filtered.  Without the evicted entry bins 6 and 8 would tie at 1 and the lower bin 6 would be kept
    xs1 = [100, 102] + [130 + 30 * k for k in range(7)]
    d1 = [bits((0, 30)), bits((0, 20))] + [ZERO] * 7
    ang = [240, 60, 60, 60, 120, 120, 240, 180, 0]
    xs2 = [101] + [131 + 30 * k for k in range(6)]
    t1 = table(xs1, [100] * 9, d1, angle=ang)
    t2 = table(xs2 + [400], [100] * 8, [ZERO] * 8)
    c["histogram_counts_evicted"] = (t1, t2, None, w, [-1, 0, 1, 2, 3, 4, 5, 6, -1], [-1, 0, 1, 2, 3, 4, 5, -1, -1], 6)
    return c


def test_hand_worked_cases():
    for name, (t1, t2, prev, kw, raw, m12, nm) in hand_cases().items():
        r, m, n, _ = both(t1, t2, prev, **kw)
        assert (r.tolist(), m.tolist(), n) == (raw, m12, nm), name
    t1, t2, _, kw, raw, _, _ = hand_cases()["histogram_counts_evicted"]
    r, m, n, _ = both(t1, t2, check_ori=False, **kw)                         # without the filter nothing is cleared
    assert r.tolist() == raw and m.tolist() == raw and n == 7
    ex = Counter()
    both(t1, t2, exits=ex, **kw)
    assert ex["eviction"] == 1 and ex["filtered"] == 1 and ex["filtered_already_evicted"] == 0


def test_dist_limit():
    assert dist_limit(0.9) == 55 and f32(f32(55) * f32(0.9)) <= 50 < f32(f32(56) * f32(0.9))
    assert dist_limit(1.0) == 50 and dist_limit(2.0) == 50 and dist_limit(0.5) == 100 and dist_limit(0.1) == 256
    assert f32(f32(50) * f32(0.9)) == f32(45.0)                              # the boundary of the hand-worked case


# ---- the constructed scene -----------------------------------------------------------------------------------------------------

def flip(rng, d, n):
    u = np.unpackbits(d.copy())
    u[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(u)


def wrap360(a):
    a = np.mod(np.asarray(a, np.float64), 360.0).astype(f32)
    a[a >= f32(360.0)] = 0
    return a


def scene(rng, nfam=200, motion=(6.0, 3.0), later=3):
    """F1 and `later` following frames of 2 * nfam keypoints each: families of two F1 and two F(k) keypoints that share a
    descriptor up to a few flipped bits and lie close together (contention, evictions, ratio rejections); the frames move by
    `motion` per step; most angles follow the frame, some are random (the rotation filter); the families in the right part of F1
    have their later keypoints far to the left (empty windows)."""
    W, H = 752.0, 480.0
    fam = rng.integers(0, 256, (nfam, 32), dtype=np.uint8)
    cx, cy = rng.uniform(5, W - 5, nfam), rng.uniform(5, H - 5, nfam)
    fang = rng.uniform(0, 360, nfam)
    x1 = np.repeat(cx, 2) + rng.uniform(-8, 8, 2 * nfam)
    y1 = np.repeat(cy, 2) + rng.uniform(-8, 8, 2 * nfam)
    d1 = np.stack([flip(rng, fam[k // 2], int(rng.integers(0, 12))) for k in range(2 * nfam)])
    o1 = (rng.random(2 * nfam) < 0.25).astype(np.int32) * rng.integers(1, 4, 2 * nfam)
    a1 = wrap360(np.repeat(fang, 2) + rng.normal(0, 4, 2 * nfam))
    t1 = table(np.clip(x1, 0, W - 1), np.clip(y1, 0, H - 1), d1, o1, a1)
    frames = []
    for s in range(1, later + 1):
        far = np.repeat(cx > 540, 2)
        x = np.where(far, rng.uniform(0, 300, 2 * nfam), np.repeat(cx, 2) + s * motion[0] + rng.uniform(-10, 10, 2 * nfam))
        y = np.repeat(cy, 2) + s * motion[1] + rng.uniform(-10, 10, 2 * nfam)
        d = np.stack([flip(rng, fam[k // 2], int(rng.integers(0, 45))) for k in range(2 * nfam)])
        o = (rng.random(2 * nfam) < 0.25).astype(np.int32) * rng.integers(1, 4, 2 * nfam)
        a = np.where(rng.random(2 * nfam) < 0.75, np.repeat(fang, 2) + 10 * s + rng.normal(0, 4, 2 * nfam), rng.uniform(0, 360, 2 * nfam))
        frames.append(table(np.clip(x, 0, W - 1), np.clip(y, 0, H - 1), d, o, wrap360(a)))
    return t1, frames


def test_the_constructed_scene_takes_every_exit():
    t1, (t2, _, _) = scene(np.random.default_rng(SCENE_SEED))
    assert len(t1.x) == 400 and len(t2.x) == 400
    ex = Counter()
    raw, m12, nm, _ = both(t1, t2, exits=ex, window=100, nnratio=0.9)
    print("exits:", ", ".join("%s %d" % (k, ex[k]) for k in EXITS), "; raw %d, matches %d" % (int((raw >= 0).sum()), nm))
    for k in EXITS:
        assert ex[k] > 0, k
    assert nm > 40 and nm == int((m12 >= 0).sum())
    r2, m2, n2, _ = both(t1, t2, window=100, nnratio=0.9, check_ori=False)
    assert np.array_equal(r2, raw) and np.array_equal(m2, raw) and n2 == int((raw >= 0).sum()) > nm


def chain(fn, t1, frames, **kw):
    """Tracking.cc:2072-2074 and :2109-2110: mvbPrevMatched starts as F1's points and is carried from call to call."""
    prev = points_of(t1)
    out = []
    for t in frames:
        raw, m12, nm, prev = fn(t1, t, prev, **kw)
        out.append((raw, m12, nm, prev.copy()))
    return out


def chain_scene():
    """45 x 20 px per frame: by the third frame a keypoint is outside the window around its first position"""
    return scene(np.random.default_rng(SCENE_SEED), motion=(45.0, 20.0))


def test_a_chain_of_three_calls_carries_prev_matched():
    t1, frames = chain_scene()
    a = chain(init_search_scalar, t1, frames, window=100)
    b = chain(init_search_fast, t1, frames, window=100)
    start = points_of(t1)
    for (ra, ma, na, pa), (rb, mb, nb, pb) in zip(a, b):
        assert np.array_equal(ra, rb) and np.array_equal(ma, mb) and na == nb and pa.tobytes() == pb.tobytes()
        assert na > 30
    assert (a[0][3] != start).any() and (a[1][3] != a[0][3]).any()
    alone = init_search_fast(t1, frames[2], start, window=100)                # the carried windows matter
    assert not np.array_equal(alone[1], b[2][1]) and alone[2] < b[2][2]


def test_small_windows_and_other_ratios_agree():
    t1, (t2, t3, _) = scene(np.random.default_rng(SCENE_SEED + 1))
    for window, nnratio in ((0, 0.9), (1, 0.9), (15, 0.6), (40, 1.0), (100, 0.75), (100, 3.0)):
        both(t1, t2, window=window, nnratio=nnratio)
        both(t1, t3, window=window, nnratio=nnratio, check_ori=False)
    other = (10.0, 700.0, 20.0, 470.0)                                        # bounds that put keypoints outside the grid
    raw, _, nm, _ = both(t1, t2, bounds=other, window=100)
    assert nm > 20
    empty = table([], [], np.zeros((0, 32), np.uint8))
    for a, b in ((empty, t2), (t1, empty), (empty, empty)):
        r, m, n, p = both(a, b)
        assert n == 0 and (m == -1).all() and len(m) == len(a.x)


def test_the_binding_declares_the_entry_point():
    from pli_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert re.search(r"pli_status\s+pli_search_for_initialization\s*\(", hdr)
    assert "pli_search_for_initialization" in capi._PROTOS and len(capi._PROTOS["pli_search_for_initialization"][1]) == 18
    assert capi.KEYPOINT_DT == KEYPOINT_DT
    from pli_slam_amd.frontend import Frontend
    assert hasattr(Frontend, "search_for_initialization")
    lib = C.CDLL(capi.LIB_PATH)                                               # the product library exports the symbol
    assert hasattr(lib, "pli_search_for_initialization")
