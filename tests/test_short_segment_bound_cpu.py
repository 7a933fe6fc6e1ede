"""The short-segment cut (pli_slam_amd/csrc/common.hpp "SHORT-SEGMENT CUT"): the tile relaxation computes no segment for a region whose
bounding box says that the segment cannot pass the key-line length test.  What that rests on is a bound,

    length  <=  sqrt(bw^2 + bh^2) / scale  +  1e-3          (bw, bh: the extents of the region's pixels in the scaled image),

checked here on a float64 restatement of region2rect (the one of tests/test_independent_lsd.py, item 7 and 8) followed by what the
library does with the four coordinates: the rounding to float, checkLineExtremes' clamp into the image and the float length of
k_keylines.  Seeded random 8-connected pixel sets; no GPU.  The cut value itself comes from the library (pli_lsd_segment_box_cut)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers_line_ref import clamp_segments, lengths_of

PI = math.pi


def region2rect(xs, ys, w, reg_angle, scale, prec=PI * 22.5 / 180):
    """float64: weighted centroid, main inertia axis, extent along it; back to the input image's frame.  (x1, y1, x2, y2) doubles."""
    xs = xs.astype(np.float64)
    ys = ys.astype(np.float64)
    wsum = w.sum()
    cx, cy = (xs * w).sum() / wsum, (ys * w).sum() / wsum
    Ixx = ((ys - cy) ** 2 * w).sum()
    Iyy = ((xs - cx) ** 2 * w).sum()
    Ixy = -((xs - cx) * (ys - cy) * w).sum()
    lam = 0.5 * (Ixx + Iyy - math.sqrt((Ixx - Iyy) ** 2 + 4 * Ixy * Ixy))
    theta = math.atan2(lam - Ixx, Ixy) if abs(Ixx) > abs(Iyy) else math.atan2(Ixy, lam - Iyy)
    d = theta - reg_angle
    while d <= -PI:
        d += 2 * PI
    while d > PI:
        d -= 2 * PI
    if abs(d) > prec:
        theta += PI
    dx, dy = math.cos(theta), math.sin(theta)
    ls = (xs - cx) * dx + (ys - cy) * dy
    lmin, lmax = min(0.0, ls.min()), max(0.0, ls.max())            # (l_min and l_max start from 0)
    return [(cx + lmin * dx + 0.5) / scale, (cy + lmin * dy + 0.5) / scale, (cx + lmax * dx + 0.5) / scale, (cy + lmax * dy + 0.5) / scale]


def keyline_length(seg, W, H):
    """the float rounding of the end points, checkLineExtremes, the float length: what k_keylines compares with the minimum length"""
    e, _ = clamp_segments(np.array(seg, np.float64).astype(np.float32), W, H)
    return float(lengths_of(e)[0])


def box2(xs, ys):
    bw, bh = int(xs.max() - xs.min()), int(ys.max() - ys.min())
    return bw * bw + bh * bh


def pruned(xs, ys, cut):
    """lsd_box_can_pass, negated"""
    return cut >= 0 and box2(xs, ys) <= cut


NB = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


def pixel_set(rng, kind, n):
    """an 8-connected set of n distinct pixels (fewer for a walk that crosses itself), around the origin"""
    if kind == "row":
        return np.arange(n), np.zeros(n, int)
    if kind == "col":
        return np.zeros(n, int), np.arange(n)
    if kind == "diag":
        return np.arange(n), np.arange(n) * (1 if rng.integers(2) else -1)
    if kind == "walk":
        # a walk with a preferred direction: long thin regions, the kind that yields the longest segments for its box
        pref = NB[rng.integers(8)]
        p = [(0, 0)]
        for _ in range(n - 1):
            st = pref if rng.random() < 0.7 else NB[rng.integers(8)]
            p.append((p[-1][0] + st[0], p[-1][1] + st[1]))
        p = list(dict.fromkeys(p))
    else:                                                   # blob: grown from the seed, a random frontier pixel at a time
        have = {(0, 0)}
        p = [(0, 0)]
        while len(p) < n:
            bx, by = p[rng.integers(len(p))]
            st = NB[rng.integers(8)]
            q = (bx + st[0], by + st[1])
            if q not in have:
                have.add(q)
                p.append(q)
    a = np.array(p)
    return a[:, 0], a[:, 1]


def cases():
    rng = np.random.default_rng(20240607)
    out = []
    for i in range(1500):
        kind = ("row", "col", "diag", "walk", "walk", "blob", "blob")[i % 7]
        n = int(rng.integers(1, 401)) if i % 5 else int(rng.integers(1, 12))
        xs, ys = pixel_set(rng, kind, n)
        xs, ys = xs - xs.min(), ys - ys.min()
        scale = (1.0, 1.2)[i % 2]
        place = i % 4
        LW, LH = 4608, 4608                                 # the scaled image: coordinates up to 4607
        if place == 0:                                      # anywhere
            ox, oy = int(rng.integers(0, LW - xs.max())), int(rng.integers(0, LH - ys.max()))
        elif place == 1:                                    # against the far corner: the largest coordinates, and the clamp acts
            ox, oy = LW - 1 - int(xs.max()), LH - 1 - int(ys.max())
        elif place == 2:                                    # against the origin
            ox, oy = 0, 0
        else:                                               # against the right border only
            ox, oy = LW - 1 - int(xs.max()), int(rng.integers(0, LH - ys.max()))
        xs, ys = xs + ox, ys + oy
        w = 10.0 ** rng.uniform(-3, 3, len(xs))             # gradient norms: positive, six decades
        # the input image the scaled one came from (cvRound(W * scale) = LW): its last column / row is where the clamp puts a coordinate
        W, H = int(math.floor(LW / scale)), int(math.floor(LH / scale))
        out.append((kind, xs, ys, w, float(rng.uniform(-PI, PI)), scale, W, H))
    return out


def test_length_is_bounded_by_the_box_diagonal():
    worst = -1e9
    clamped = 0
    for kind, xs, ys, w, reg_angle, scale, W, H in cases():
        assert xs.min() >= 0 and ys.min() >= 0 and xs.max() <= 4607 and ys.max() <= 4607
        seg = region2rect(xs, ys, w, reg_angle, scale)
        length = keyline_length(seg, W, H)
        clamped += any(v < 0 for v in seg) or seg[0] >= W or seg[2] >= W or seg[1] >= H or seg[3] >= H
        bound = math.sqrt(box2(xs, ys)) / scale
        worst = max(worst, length - bound)
        assert length <= bound + 1e-3, (kind, len(xs), scale, length, bound)
    print("largest length - D / scale over the sets: %.3e; sets whose end points were clamped: %d" % (worst, clamped))
    assert clamped >= 50, "the sets at the borders were meant to exercise the clamp"


def lib_cut(W, H, **kw):
    from pli_slam_amd import capi
    cfg = capi.default_config(W, H, **kw)
    return int(capi.lib().pli_lsd_segment_box_cut(C.byref(cfg)))


def test_the_cut_value_and_the_cases_at_the_cut():
    # min_line_length * min(W, H) = 12 px, scale 1.2: floor((1.2 * 11.99)^2) = floor(207.01...) = 207
    assert lib_cut(752, 480) == 207 and lib_cut(376, 240, min_line_length=0.05) == 207
    assert lib_cut(376, 240) == math.floor((1.2 * (6 - 0.01)) ** 2) == 51
    assert lib_cut(376, 240, min_line_length=0.2) == math.floor((1.2 * (48 - 0.01)) ** 2)
    assert lib_cut(376, 240, min_line_length=0.05, lsd_scale=1.0) == math.floor(11.99 ** 2) == 143
    assert lib_cut(376, 240, min_line_length=0.0) == -1                 # nothing fails `length > 0` for certain: no cut
    assert lib_cut(376, 240, min_line_length=0.01 / 240) == -1          # minLength - 0.01 <= 0
    assert lib_cut(9000, 480) == -1                                     # past the float budget of the derivation: no cut
    cut = 207
    one = np.ones
    # a row of 15 pixels: bw = 14, 196 <= 207: no segment, and rightly so: 14 / 1.2 = 11.67 px
    xs, ys = np.arange(15) + 100, np.zeros(15, int) + 50
    assert box2(xs, ys) == 196 and pruned(xs, ys, cut)
    length = keyline_length(region2rect(xs, ys, one(15), 0.0, 1.2), 752, 480)
    assert abs(length - 14 / 1.2) < 1e-4 and length < 12
    # boxes of 14 x 3 (205: cut) and 14 x 4 (212: kept) — filled rectangles of 15 x 4 and 15 x 5 pixels
    for bh, want in ((3, True), (4, False)):
        yy, xx = np.mgrid[0:bh + 1, 0:15]
        xs, ys = xx.ravel() + 100, yy.ravel() + 50
        assert box2(xs, ys) == 196 + bh * bh and pruned(xs, ys, cut) == want
        length = keyline_length(region2rect(xs, ys, one(len(xs)), 0.0, 1.2), 752, 480)
        assert length <= math.sqrt(box2(xs, ys)) / 1.2 + 1e-3
    # ... whatever the pixels inside a cut box are, the segment is too short: the two opposite corners alone, joined by a diagonal walk
    xs = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]) + 100
    ys = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]) + 50
    assert box2(xs, ys) == 205 and pruned(xs, ys, cut)
    assert keyline_length(region2rect(xs, ys, one(15), 0.2, 1.2), 752, 480) < 12 - 0.009
    assert not pruned(xs, ys, -1)                                        # -1: nothing is cut
