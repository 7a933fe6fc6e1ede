"""An independent restatement of the stereo and descriptor matchers, CPU only, plain numpy.

Written from the reference's text (Frame::ComputeStereoMatches, Frame.cc:976-1154; Frame::ComputeStereoMatches_Lines with
lineSegmentOverlapStereo and filterLineSegmentDisparity, Frame.cc:1156-1307; matchGrid / matchNNR / match,
LineMatcher.cpp:139-229, 317-396; GridStructure::get and getLineCoords, gridStructure.cpp; LineIterator.cpp) and from the
OpenCV documentation of the calls it makes (Mat::rowRange / colRange, cv::norm(NORM_L1), BFMatcher::knnMatch) -- NOT from
oracle/ and NOT from the kernels.  It is shaped differently on purpose, so that a transcription slip is not repeated:

  * no row table: a right keypoint is a candidate of a left one iff floor(y - r) <= int(vL) <= ceil(y + r);
  * no grid lists: a right line is a candidate of a left one iff one of its Bresenham cells lies in one of the two windows;
  * the running-minimum rule of bestLRMatches as a column prefix minimum over the whole distance matrix;
  * a full sort for the median, and the cut as a per-keypoint predicate.

Float results follow the reference's operation order in np.float32 / np.float64, so they are compared bit for bit.
Every function returns, per query, a tuple of labels: the exit the query took first, then the edges it touched on the way.
The tests count coverage with these labels (never with the oracle's or a kernel's output).

`Rules` holds the comparisons that the mutation tests flip; the defaults are the reference's.

Where the reference's behaviour is undefined, the project's definition is restated (and said so at the place): a window
that cv::Mat::rowRange / colRange would reject gives "no stereo"; an empty vDistIdx gives "nothing to cut".
"""
import math
from dataclasses import dataclass

import numpy as np

KEYPOINT_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
KEYLINE_DT = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                       ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                       ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"),
                       ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"), ("numOfPixels", "<i4")])
f32 = np.float32
TH_HIGH, TH_LOW = 100, 50
GRID_ROWS, GRID_COLS = 48, 64
INT_MAX = 2 ** 31 - 1


@dataclass(frozen=True)
class Rules:
    """The reference's rules; each mutation test changes one field."""
    band_end_exclusive: bool = False      # row band without its two ends
    vl_rounded: bool = False              # left row by rounding vL instead of truncating
    endu_gt: bool = False                 # `endu > cols` instead of `>=`
    orb_le: bool = False                  # `bestDist <= thOrbDist` instead of `<`
    ul_minus_001_float: bool = False      # `uL - 0.01` in float instead of double
    median_low: bool = False              # median at (M - 1) / 2 instead of M / 2
    cut_le: bool = False                  # survivors are `<= thDist` instead of `<`
    nan_dir_rejected: bool = False        # a left line with NaN direction loses its candidates
    col_equal_kept: bool = False          # an equal distance in a column is kept
    ratio_float: bool = False             # the 1st / 2nd ratio test in float
    ur_bounds_exclusive: bool = False     # `uR > minU && uR < maxU` instead of the inclusive ends
    octave_gate_narrow: bool = False      # only the left keypoint's own octave instead of levelL - 1 .. levelL + 1
    maxd_inclusive: bool = False          # `disparity <= maxD` instead of `<`
    nan_minmax: str = "std"               # "std": std::min / std::max ((b < a) ? b : a); "fmin": IEEE fmin / fmax
    length_eln_sln: bool = False          # lineSegmentOverlapStereo: `length = eln - sln` instead of `eln - spn`
    epr_from_old_spr: bool = False        # ep_r interpolated from sp_r as it was before Frame.cc:1228 overwrote it
    hamming_to_vdistidx: bool = False     # the Hamming bestDist, not the SAD that shadows it, goes to vDistIdx
    sort_ties_insertion: bool = False     # vDistIdx sorted by distance alone, equal distances in insertion order
    overlap_zero_horizontal: bool = False # lineSegmentOverlapStereo gives 0, not 1, for a horizontal left line


REF = Rules()
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


def hamming(a, b):
    """ORBmatcher::DescriptorDistance / LineMatcher's distance(): bits that differ between 256-bit rows (broadcasts)."""
    return _POP[np.bitwise_xor(a, b)].sum(-1).astype(np.int32)


def c_round(x):
    """round(): half away from zero, on a float32 value (exact in double)."""
    x = float(x)
    return math.copysign(math.floor(abs(x) + 0.5), x)


def scale_factors(nlevels, scale_factor):
    """ORBextractor's mvScaleFactor / mvInvScaleFactor (ORBextractor.cc:420-437), float arithmetic."""
    sf = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        sf[i] = f32(sf[i - 1] * f32(scale_factor))
    return sf, (f32(1.0) / sf).astype(f32)


def max_disparity(bf, fx, maxd_inf=False):
    """maxD = mbf / mb with mb = mbf / fx (Frame.cc:197, 1006-1008), or +inf (the reference reads mb before it is set)."""
    if maxd_inf:
        return f32(np.inf)
    return f32(f32(bf) / f32(f32(bf) / f32(fx)))


# ---------------------------------------------------------------------------------------------------------------------
# Frame::ComputeStereoMatches
# ---------------------------------------------------------------------------------------------------------------------
def stereo_points(kpL, descL, kpR, descR, pyrL, pyrR, sf, inv_sf, bf, maxD, rules=REF):
    """-> uright, depth, best_idx, sad, exits (tuple of labels per left keypoint), frame_tags (set: the median cut)."""
    N, Nr = len(kpL), len(kpR)
    uright = np.full(N, -1, f32); depth = np.full(N, -1, f32)
    best_idx = np.full(N, -1, np.int32); sad_out = np.full(N, -1, np.int32)
    ham_out = np.full(N, -1, np.int32)
    exits = [()] * N
    bf, maxD, minD = f32(bf), f32(maxD), f32(0)
    nlev = len(sf)
    thOrb = (TH_HIGH + TH_LOW) // 2
    # the row band of every right keypoint
    r = (f32(2.0) * sf[kpR["octave"]]).astype(f32) if Nr else np.zeros(0, f32)
    maxr = np.ceil((kpR["y"] + r).astype(f32)).astype(np.int64)
    minr = np.floor((kpR["y"] - r).astype(f32)).astype(np.int64)
    octR = kpR["octave"].astype(np.int64)
    with np.errstate(all="ignore"):
        for iL in range(N):
            tags = []
            uL, vL, lev = f32(kpL["x"][iL]), f32(kpL["y"][iL]), int(kpL["octave"][iL])
            row = int(c_round(vL)) if rules.vl_rounded else int(vL)
            if float(vL) - int(vL) >= 0.5:
                tags.append("vL_fraction_ge_half")
            if lev == 0:
                tags.append("left_octave_0")
            if lev == nlev - 1:
                tags.append("left_octave_top")
            inband = (minr < row) & (row < maxr) if rules.band_end_exclusive else (minr <= row) & (row <= maxr)
            for name, m in (("band_low_end", row == minr), ("band_high_end", row == maxr),
                            ("band_just_below", row == minr - 1), ("band_just_above", row == maxr + 1)):
                if m.any():
                    tags.append(name)
            if not inband.any():
                exits[iL] = ("no_row_candidates",) + tuple(tags); continue
            minU, maxU = f32(uL - maxD), f32(uL - minD)
            if np.isinf(maxD):
                tags.append("maxD_inf")
            if maxU < 0:
                exits[iL] = ("maxU_negative",) + tuple(tags); continue
            for name, m in (("octave_gate_low_end", octR == lev - 1), ("octave_gate_high_end", octR == lev + 1),
                            ("octave_gate_below", octR == lev - 2), ("octave_gate_above", octR == lev + 2)):
                if (m & inband).any():
                    tags.append(name)
            gate = inband & (octR == lev) if rules.octave_gate_narrow else inband & (octR >= lev - 1) & (octR <= lev + 1)
            uR = kpR["x"]
            if (gate & (uR == minU)).any():
                tags.append("uR_eq_minU")
            if (gate & (uR == maxU)).any():
                tags.append("uR_eq_maxU")
            cand = np.flatnonzero(gate & ((uR > minU) & (uR < maxU) if rules.ur_bounds_exclusive else (uR >= minU) & (uR <= maxU)))
            bestDist, bestR = TH_HIGH, 0
            if cand.size:
                d = hamming(descL[iL][None, :], descR[cand])
                for v in (74, 75, 99, 100):
                    if int(d.min()) == v:
                        tags.append("best_hamming_%d" % v)
                if int(d.min()) < TH_HIGH:
                    k = int(np.argmin(d))                       # first minimum = lowest right index (cand ascends)
                    bestDist, bestR = int(d[k]), int(cand[k])
                    if (d == d[k]).sum() > 1:
                        tags.append("equal_best_hamming")
            if not (bestDist <= thOrb if rules.orb_le else bestDist < thOrb):
                exits[iL] = ("hamming_not_below_thOrbDist" if bestDist < TH_HIGH else "no_candidate_below_TH_HIGH",) + tuple(tags)
                continue
            best_idx[iL] = bestR
            uR0 = f32(kpR["x"][bestR])
            s = inv_sf[lev]
            suL, svL, suR0 = f32(c_round(f32(uL * s))), f32(c_round(f32(vL * s))), f32(c_round(f32(uR0 * s)))
            w = L = 5
            imL, imR = pyrL[lev], pyrR[lev]
            rows, cols = imL.shape
            cy, cxl, cxr = int(svL), int(suL), int(suR0)
            # Mat::rowRange(a, b) / colRange(a, b) need 0 <= a <= b <= size; the reference aborts otherwise.  Project
            # definition: no stereo for this keypoint.
            if cy - w < 0 or cy + w + 1 > rows or cxl - w < 0 or cxl + w + 1 > cols:
                exits[iL] = ("left_window_outside_level",) + tuple(tags); continue
            for name, c in (("window_touches_top", cy - w == 0), ("window_touches_bottom", cy + w + 1 == rows),
                            ("window_touches_left", cxl - w == 0), ("window_touches_right", cxl + w + 1 == cols)):
                if c:
                    tags.append(name + ("_octave_0" if lev == 0 else "_octave_top" if lev == nlev - 1 else ""))
            iniu, endu = f32(suR0 + f32(L - w)), f32(suR0 + f32(L + w + 1))
            if iniu < 0:
                exits[iL] = ("strip_iniu_negative",) + tuple(tags); continue
            if (endu > cols) if rules.endu_gt else (endu >= cols):
                exits[iL] = ("strip_endu_ge_cols",) + tuple(tags); continue
            if cxr - L - w < 0 or cxr + L + w + 1 > cols:     # colRange of the first / last strip window
                exits[iL] = ("strip_window_outside_level",) + tuple(tags); continue
            if cxr - L - w == 0:
                tags.append("strip_touches_left" + ("_octave_0" if lev == 0 else "_octave_top" if lev == nlev - 1 else ""))
            if endu == cols - 1:
                tags.append("strip_touches_right" + ("_octave_0" if lev == 0 else "_octave_top" if lev == nlev - 1 else ""))
            IL = imL[cy - w:cy + w + 1, cxl - w:cxl + w + 1].astype(np.int64)
            IL = IL - IL[w, w]
            vd = np.zeros(2 * L + 1, f32)
            bestS, bestinc = INT_MAX, 0
            for inc in range(-L, L + 1):
                IR = imR[cy - w:cy + w + 1, cxr + inc - w:cxr + inc + w + 1].astype(np.int64)
                IR = IR - IR[w, w]
                dist = f32(np.abs(IL - IR).sum())               # cv::norm(NORM_L1) -> float
                if float(dist) < float(f32(bestS)):                # float against int: the int converts to float
                    bestS, bestinc = int(dist), inc
                vd[L + inc] = dist
            if (vd == vd.min()).sum() > 1:
                tags.append("equal_sads")
            if bestinc == -L or bestinc == L:
                exits[iL] = ("bestincR_minus_L" if bestinc == -L else "bestincR_plus_L",) + tuple(tags); continue
            d1, d2, d3 = vd[L + bestinc - 1], vd[L + bestinc], vd[L + bestinc + 1]
            deltaR = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
            if deltaR < -1 or deltaR > 1:
                exits[iL] = ("deltaR_outside",) + tuple(tags); continue
            if np.isnan(deltaR):
                tags.append("deltaR_nan")
            if abs(float(deltaR)) == 0.5:
                tags.append("deltaR_at_half")
            bestuR = f32(sf[lev] * f32(f32(suR0 + f32(bestinc)) + deltaR))
            disparity = f32(uL - bestuR)
            if not (disparity >= minD and (disparity <= maxD if rules.maxd_inclusive else disparity < maxD)):
                if disparity == maxD:
                    tags.append("disparity_eq_maxD")
                exits[iL] = ("disparity_negative" if disparity < minD else
                             "disparity_ge_maxD" if disparity >= maxD else "disparity_nan",) + tuple(tags)
                continue
            if disparity <= 0:
                tags.append("disparity_zero")
                disparity = f32(0.01)
                bestuR = f32(uL - f32(0.01)) if rules.ul_minus_001_float else f32(np.float64(uL) - 0.01)
            depth[iL] = f32(bf / disparity)
            uright[iL] = bestuR
            sad_out[iL] = bestS
            ham_out[iL] = bestDist
            exits[iL] = ("matched",) + tuple(tags)
    # the median cut (Frame.cc:1140-1153) as a predicate: sorted by (SAD, index), the tail from the first SAD that is not
    # below thDist is removed -- that is every survivor whose SAD is not below thDist.
    ftags = set()
    ok = np.flatnonzero(sad_out >= 0)
    M = ok.size
    ftags.add("survivors_none" if M == 0 else "survivors_one" if M == 1 else "survivors_even" if M % 2 == 0 else "survivors_odd")
    if M:      # (M == 0: vDistIdx[0] of an empty vector in the reference; project definition: nothing to cut)
        key = ham_out if rules.hamming_to_vdistidx else sad_out
        order = sorted((int(key[i]), int(i)) for i in ok)
        if rules.sort_ties_insertion:      # insertion order is iL order: the same sequence, and the cut does not read the order
            order = sorted(order, key=lambda o: o[0])
        med = order[(M - 1) // 2 if rules.median_low else M // 2][0]
        median = f32(med)
        thDist = f32(f32(f32(1.5) * f32(1.4)) * median)
        sads = np.array([o[0] for o in order])
        if med == 0:
            ftags.add("median_zero")
        if (sads == med).sum() >= 3 and M >= 4:
            ftags.add("equal_sads_around_median")
        if len(set(sads.tolist())) > 1 and len(set((sads & 255).tolist())) == 1:
            ftags.add("sads_differ_in_upper_bytes_only")
        if (sads.astype(f32) == thDist).any():
            ftags.add("sad_at_thDist")
        for sd, i in order:
            keep = (f32(sd) <= thDist) if rules.cut_le else (f32(sd) < thDist)
            if not keep:
                uright[i] = -1; depth[i] = -1
                exits[i] = ("matched_then_cut",) + exits[i][1:]
        if all(e[0] != "matched" for e in exits):
            ftags.add("cut_removes_everything")
    return uright, depth, best_idx, sad_out, exits, ftags


# ---------------------------------------------------------------------------------------------------------------------
# Frame::ComputeStereoMatches_Lines
# ---------------------------------------------------------------------------------------------------------------------
def line_cells(x1, y1, x2, y2):
    """getLineCoords + LineIterator: the cells (x, y) a segment walks, doubles in, Bresenham with the error term in double."""
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1, x2, y2 = y1, x1, y2, x2
    swapped = x1 > x2
    if swapped:
        x1, x2, y1, y2 = x2, x1, y2, y1
    dx, dy = x2 - x1, abs(y2 - y1)
    err = dx / 2.0
    ystep = 1 if y1 < y2 else -1
    x, y, maxx = int(x1), int(y1), int(x2)
    out = []
    while x <= maxx:
        out.append((y, x) if steep else (x, y))
        err -= dy
        if err < 0:
            y += ystep; err += dx
        x += 1
    return out, steep, swapped


def _smin(a, b, mode):
    if mode == "fmin":
        return b if a != a else a if b != b else min(a, b)
    return b if b < a else a


def _smax(a, b, mode):
    if mode == "fmin":
        return b if a != a else a if b != b else max(a, b)
    return b if a < b else a


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def overlap_stereo(spl, epl, spr, epr, th, rules=REF, tags=None):
    """Frame::lineSegmentOverlapStereo on four doubles (the rows of the two left and the two right end points)."""
    tags = [] if tags is None else tags
    mode = rules.nan_minmax
    overlap = 1.0
    if abs(epl - spl) > th:
        sln, eln = _smin(spl, epl, mode), _smax(spl, epl, mode)
        spn, epn = _smin(spr, epr, mode), _smax(spr, epr, mode)
        length = eln - sln if rules.length_eln_sln else eln - spn
        if epn < sln or spn > eln:
            overlap = 0.0; tags.append("overlap_disjoint")
        elif epn > eln and spn < sln:
            overlap = eln - sln; tags.append("overlap_right_contains_left")
        else:
            overlap = _smin(eln, epn, mode) - _smax(sln, spn, mode); tags.append("overlap_partial")
        if length > float(f32(0.01)):
            overlap = _div(overlap, length)
        else:
            overlap = 0.0; tags.append("overlap_length_le_0.01")
        if overlap > 1.0:
            overlap = 1.0; tags.append("overlap_clamped_to_1")
    else:
        tags.append("overlap_left_horizontal")
        if rules.overlap_zero_horizontal:
            overlap = 0.0
    return overlap


def filter_disparity(splx, eplx, sprx, eprx, ratio, rules=REF, tags=None):
    """Frame::filterLineSegmentDisparity on the four columns -> disp_s, disp_e."""
    tags = [] if tags is None else tags
    mode = rules.nan_minmax
    with np.errstate(all="ignore"):
        ds, de = float(np.float64(splx) - sprx), float(np.float64(eplx) - eprx)
        if (ds < 0) != (de < 0) and ds == ds and de == de:
            tags.append("disparities_of_mixed_sign")
        if ds < 0 and de < 0:
            tags.append("disparities_both_negative")
        q = _div(_smin(ds, de, mode), _smax(ds, de, mode))
        if q != q:
            tags.append("disparity_ratio_nan")
        elif q < 0:
            tags.append("disparity_ratio_negative")
        if q < float(ratio):
            ds, de = -1.0, -1.0; tags.append("disparity_ratio_reset")
    return ds, de


def stereo_lines(cfg, klL, ldL, klR, ldR, W, H, rules=REF):
    """-> disp (n1, 2) float32, le (n1, 3) float64, m12 (n1,) int32, exits."""
    n1, n2 = len(klL), len(klR)
    disp = np.full((n1, 2), -1, f32); le = np.zeros((n1, 3), np.float64); m12 = np.full(n1, -1, np.int32)
    exits = [("no_lines",)] * n1
    if n1 == 0 or n2 == 0:
        return disp, le, m12, exits
    iw, ih = GRID_COLS / float(W), GRID_ROWS / float(H)
    ws = int(cfg.matching_s_ws)
    mode = rules.nan_minmax
    # the cells of every right line, as a boolean image of the grid, and its direction
    occ = np.zeros((n2, GRID_COLS, GRID_ROWS), bool)
    dirs = np.zeros((n2, 2)); rtags = [None] * n2
    for j in range(n2):
        sx, sy = float(klR["startPointX"][j]), float(klR["startPointY"][j])
        ex, ey = float(klR["endPointX"][j]), float(klR["endPointY"][j])
        vx = float(f32(klR["endPointX"][j] - klR["startPointX"][j])) * iw
        vy = float(f32(klR["endPointY"][j] - klR["startPointY"][j])) * ih
        mag = math.sqrt(vx * vx + vy * vy)
        dirs[j] = (_div(vx, mag), _div(vy, mag))
        cells, steep, swapped = line_cells(sx * iw, sy * ih, ex * iw, ey * ih)
        t = ["right_steep" if steep else "right_shallow"] + (["right_walk_swapped"] if swapped else ["right_walk_forward"])
        for (cx, cy) in cells:
            if 0 <= cx < GRID_COLS and 0 <= cy < GRID_ROWS:
                occ[j, cx, cy] = True
            elif "right_cells_outside_grid" not in t:
                t.append("right_cells_outside_grid")
        rtags[j] = t
    # the whole distance matrix over candidate pairs (-1: not a candidate)
    D = np.full((n1, n2), -1, np.int64)
    ltags = [[] for _ in range(n1)]
    for i in range(n1):
        qs = (int(float(klL["startPointX"][i]) * iw), int(float(klL["startPointY"][i]) * ih))
        qe = (int(float(klL["endPointX"][i]) * iw), int(float(klL["endPointY"][i]) * ih))
        vx, vy = float(qe[0] - qs[0]), float(qe[1] - qs[1])
        mag = math.sqrt(vx * vx + vy * vy)
        vx, vy = _div(vx, mag), _div(vy, mag)
        nan_dir = vx != vx
        if nan_dir:
            ltags[i].append("left_endpoints_in_one_cell")
        win = np.zeros((GRID_COLS, GRID_ROWS), bool)
        for (qx, qy) in (qs, qe):
            lo, hi = max(0, qx - ws), min(GRID_COLS, qx + 0 + 1)       # GridWindow width (ws, 0), height (0, 0)
            ylo, yhi = max(0, qy), min(GRID_ROWS, qy + 1)
            if not (0 <= qx < GRID_COLS and 0 <= qy < GRID_ROWS):
                ltags[i].append("left_endpoint_outside_grid")
            if lo < hi and ylo < yhi:
                win[lo:hi, ylo:yhi] = True
                if qx - ws < 0:
                    ltags[i].append("window_clipped_at_column_0")
                if qx == GRID_COLS - 1:
                    ltags[i].append("window_at_column_63")
        cand = np.flatnonzero((occ & win[None]).any(axis=(1, 2)))
        for j in cand:
            dot = vx * dirs[j, 0] + vy * dirs[j, 1]
            if abs(dot) == cfg.line_sim_th:
                ltags[i].append("dot_eq_lineSimTh")
            if abs(dot) < cfg.line_sim_th or (nan_dir and rules.nan_dir_rejected):
                continue
            if nan_dir:
                ltags[i].append("nan_direction_candidate_kept")
            D[i, j] = int(hamming(ldL[i], ldR[j]))
            ltags[i] += rtags[j]
    # bestLRMatches: a pair counts only where it lowers the running minimum of its column
    m21 = np.full(n2, -1, np.int64)
    if cfg.best_lr_matches:
        for j in range(n2):
            run = INT_MAX
            for i in range(n1):
                d = D[i, j]
                if d < 0:
                    continue
                if d < run or (rules.col_equal_kept and d == run):
                    if d < run:
                        m21[j] = i
                    run = d
                else:
                    if d == run:
                        ltags[i].append("equal_distance_in_column_dropped")
                    D[i, j] = -1
    for i in range(n1):
        tags = ltags[i]
        if not cfg.best_lr_matches:
            tags.append("best_lr_matches_off")
        row = D[i]
        idx = np.flatnonzero(row >= 0)
        if idx.size == 0:
            exits[i] = ("no_candidates",) + tuple(tags); continue
        # first / second smallest in ascending index order (ties at the best: the ratio test rejects them for any order)
        bd, bd2, bi = INT_MAX, INT_MAX, -1
        for j in idx:
            d = int(row[j])
            if d < bd:
                bd2, bd, bi = bd, d, int(j)
            elif d < bd2:
                bd2 = d
        if idx.size == 1:
            tags.append("single_candidate")
        lim = float(f32(f32(bd2) * f32(cfg.min_ratio_12_l))) if rules.ratio_float else float(bd2) * float(cfg.min_ratio_12_l)
        if float(bd) == lim:
            tags.append("ratio_test_at_equality")
        if not (float(bd) < lim):
            exits[i] = ("ratio_test_failed",) + tuple(tags); continue
        if cfg.best_lr_matches and m21[bi] != i:
            exits[i] = ("mutual_check_failed",) + tuple(tags); continue
        m12[i] = bi
    for i in range(n1):
        j = int(m12[i])
        if j < 0:
            continue
        tags = ltags[i]
        spl = (float(klL["startPointX"][i]), float(klL["startPointY"][i])); epl = (float(klL["endPointX"][i]), float(klL["endPointY"][i]))
        l0, l1, l2 = spl[1] * 1.0 - 1.0 * epl[1], 1.0 * epl[0] - spl[0] * 1.0, spl[0] * epl[1] - spl[1] * epl[0]
        nrm = math.sqrt(l0 * l0 + l1 * l1)
        lel = (_div(l0, nrm), _div(l1, nrm), _div(l2, nrm))
        spr = [float(klR["startPointX"][j]), float(klR["startPointY"][j])]; epr = [float(klR["endPointX"][j]), float(klR["endPointY"][j])]
        th = float(cfg.line_horiz_th)
        # lineSegmentOverlapStereo(sp_l(1), ep_l(1), sp_r(1), ep_r(1))
        overlap = overlap_stereo(spl[1], epl[1], spr[1], epr[1], th, rules, tags)
        if spr[1] == epr[1]:
            tags.append("right_horizontal_division_by_zero")
        # Eigen's comma initialiser evaluates the three expressions before it assigns: the first line uses the old sp_r,
        # the second the new one.
        den = spr[1] - epr[1]
        with np.errstate(all="ignore"):
            nsx = _div(np.float64(spr[0]) * (spl[1] - epr[1]) + np.float64(epr[0]) * (spr[1] - spl[1]), den)
            if not rules.epr_from_old_spr:
                spr = [nsx, spl[1]]
            den = spr[1] - epr[1]
            nex = _div(np.float64(spr[0]) * (epl[1] - epr[1]) + np.float64(epr[0]) * (spr[1] - epl[1]), den)
            epr = [nex, epl[1]]
            spr = [nsx, spl[1]]
            ds, de = filter_disparity(spl[0], epl[0], spr[0], epr[0], cfg.ls_min_disp_ratio, rules, tags)
        md = float(cfg.min_disp)
        if ds == md or de == md:
            tags.append("disp_eq_min_disp")
        if abs(spl[1] - epl[1]) == th:
            tags.append("dy_eq_line_horiz_th")
        if overlap == float(cfg.stereo_overlap_th):
            tags.append("overlap_eq_stereo_overlap_th")
        why = None
        if not (ds >= md and de >= md):
            why = "rejected_min_disp"
        elif not abs(spl[1] - epl[1]) > th:
            why = "rejected_left_horizontal"
        elif not abs(spr[1] - epr[1]) > th:
            why = "rejected_right_horizontal"
        elif not overlap > float(cfg.stereo_overlap_th):
            why = "rejected_overlap"
        if why is None:
            disp[i] = (f32(ds), f32(de)); le[i] = lel
            why = "matched"
        exits[i] = (why,) + tuple(tags)
    return disp, le, m12, exits


# ---------------------------------------------------------------------------------------------------------------------
# BFMatcher::knnMatch(k = 2), matchNNR, match (LineMatcher.cpp:139-229)
# ---------------------------------------------------------------------------------------------------------------------
def knn2(q, t):
    """The two nearest train rows of every query row by Hamming distance, equal distances in train order (a stable sort)."""
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int32); dist = np.full((nq, 2), INT_MAX, np.int32)
    for i in range(nq):
        if nt == 0:
            continue
        d = hamming(q[i][None, :], t)
        o = np.argsort(d, kind="stable")[:2]
        idx[i, :len(o)] = o; dist[i, :len(o)] = d[o]
    return idx, dist


def match_nnr(d1, d2, nnr):
    """matchNNR; fewer than two train rows: matches_[idx][1] does not exist in the reference -- project definition: no match."""
    m = np.full(len(d1), -1, np.int32)
    if len(d2) < 2:
        return 0, m
    idx, dist = knn2(d1, d2)
    ok = dist[:, 0].astype(f32) < (dist[:, 1].astype(f32) * f32(nnr)).astype(f32)      # DMatch::distance is a float
    m[ok] = idx[ok, 0]
    return int(ok.sum()), m


def match_lines(d1, d2, nnr, best_lr=True):
    n, m12 = match_nnr(d1, d2, nnr)
    if best_lr:
        _, m21 = match_nnr(d2, d1, nnr)
        for i in range(len(m12)):
            if m12[i] >= 0 and m21[m12[i]] != i:
                m12[i] = -1; n -= 1
    return n, m12


# ---------------------------------------------------------------------------------------------------------------------
# What the stereo kernels are entitled to assume of a table: anything else is not a test case and never goes to a device.
# ---------------------------------------------------------------------------------------------------------------------
def validate_tables(case, kp_cap=None, kl_cap=None):
    """Raises ValueError unless: counts within the capacities; octave in [0, nlevels) (it indexes the per-level tables
    unguarded); finite coordinates; keypoint rows inside the image (the oracle's row table) and columns within one image
    width of it, line end points within one image size of it (the kernels turn coordinates into ints and add small offsets:
    a value near INT_MAX would wrap past their window guards)."""
    W, H, nlev = case["W"], case["H"], case["nlevels"]
    for k in ("kpL", "kpR"):
        kp = case[k]
        if kp_cap is not None and len(kp) > kp_cap:
            raise ValueError("%s: %d keypoints > kp_cap %d" % (k, len(kp), kp_cap))
        d = case["desc" + k[-1]]
        if not (isinstance(d, np.ndarray) and d.dtype == np.uint8 and d.shape == (len(kp), 32)):
            raise ValueError(k + ": descriptors must be a uint8 array of shape (n, 32), one row per keypoint")
        if kp.dtype != KEYPOINT_DT:
            raise ValueError(k + ": not a keypoint table")
        if not (np.isfinite(kp["x"]).all() and np.isfinite(kp["y"]).all()):
            raise ValueError(k + ": non-finite coordinate")
        if ((kp["octave"] < 0) | (kp["octave"] >= nlev)).any():
            raise ValueError(k + ": octave outside [0, nlevels)")
        if ((kp["y"] < 0) | (kp["y"].astype(np.int64) >= H)).any():
            raise ValueError(k + ": keypoint row outside the image")
        if ((kp["x"] < -W) | (kp["x"] > 2 * W)).any():
            raise ValueError(k + ": keypoint column further than one width from the image")
    for k in ("klL", "klR"):
        kl = case[k]
        if kl_cap is not None and len(kl) > kl_cap:
            raise ValueError("%s: %d lines > kl_cap %d" % (k, len(kl), kl_cap))
        d = case["ld" + k[-1]]
        if not (isinstance(d, np.ndarray) and d.dtype == np.uint8 and d.shape == (len(kl), 32)):
            raise ValueError(k + ": descriptors must be a uint8 array of shape (n, 32), one row per line")
        if kl.dtype != KEYLINE_DT:
            raise ValueError(k + ": not a keyline table")
        for f, lim in (("startPointX", W), ("endPointX", W), ("startPointY", H), ("endPointY", H)):
            if not np.isfinite(kl[f]).all():
                raise ValueError(k + ": non-finite end point")
            if ((kl[f] < -lim) | (kl[f] > 2 * lim)).any():
                raise ValueError(k + ": end point further than one image size from the image")
    return case


# ---------------------------------------------------------------------------------------------------------------------
# Generators shared by the CPU and the GPU tests (lifted from tests/test_gpu_parity.py; same seeds, same draws)
# ---------------------------------------------------------------------------------------------------------------------
def descriptor_tables_random_and_ties(seed=7):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (333, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    b[100:110] = a[5]                   # exact ties at distance 0
    b[200] = a[6]; b[201] = a[6]; b[201, 0] ^= 1
    # low-entropy descriptors: many equal distances
    c = (rng.integers(0, 2, (90, 32)) * 255).astype(np.uint8)
    d = (rng.integers(0, 2, (70, 32)) * 255).astype(np.uint8)
    return a, b, c, d


def nnr_float_boundary_tables():
    """Descriptor rows whose best / second distances sit on `d0 < d1 * nnr` evaluated in float: (d0, d1) = (9, 10), (18, 20),
    (27, 30), (90, 100) and their neighbours at nnr 0.9; (30, 50), (6, 10) at nnr 0.6."""
    def row(bits):
        r = np.zeros(256, np.uint8); r[:bits] = 1
        return np.packbits(r)
    pairs = [(9, 10), (8, 10), (10, 10), (18, 20), (17, 20), (27, 30), (90, 100), (89, 100), (30, 50), (29, 50), (6, 10), (5, 10)]
    out = []
    for d0, d1 in pairs:
        q = np.zeros(32, np.uint8)
        t = np.stack([row(d1), row(d0), np.full(32, 255, np.uint8)])
        out.append((q[None], t, d0, d1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The case builder: constructed tables on real pyramids.  A case is a dict: cfg overrides, the two images, the tables.
# ---------------------------------------------------------------------------------------------------------------------
def _kp(rows):
    """rows: (x, y, octave)"""
    kp = np.zeros(len(rows), KEYPOINT_DT)
    for i, (x, y, o) in enumerate(rows):
        kp["x"][i], kp["y"][i], kp["octave"][i] = x, y, o
    kp["size"] = 31; kp["angle"] = 0; kp["response"] = 20
    return kp


def _flip(desc, nbits):
    bits = np.unpackbits(desc.copy())
    bits[:nbits] ^= 1
    return np.packbits(bits)


def _kl(rows):
    """rows: (sx, sy, ex, ey)"""
    kl = np.zeros(len(rows), KEYLINE_DT)
    for i, (sx, sy, ex, ey) in enumerate(rows):
        kl["startPointX"][i], kl["startPointY"][i], kl["endPointX"][i], kl["endPointY"][i] = sx, sy, ex, ey
    return kl


def _empty_lines():
    return dict(klL=_kl([]), ldL=np.zeros((0, 32), np.uint8), klR=_kl([]), ldR=np.zeros((0, 32), np.uint8))


def _empty_points():
    return dict(kpL=_kp([]), descL=np.zeros((0, 32), np.uint8), kpR=_kp([]), descR=np.zeros((0, 32), np.uint8))


class _Pairs:
    """Collects left / right keypoints; descriptors random per left keypoint, right ones at a chosen Hamming distance."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.L, self.R, self.dL, self.dR = [], [], [], []

    def left(self, x, y, o=0):
        self.L.append((x, y, o)); self.dL.append(self.rng.integers(0, 256, 32, dtype=np.uint8))
        return len(self.L) - 1

    def right(self, x, y, o=0, of=None, bits=0):
        self.R.append((x, y, o))
        self.dR.append(_flip(self.dL[of], bits) if of is not None else self.rng.integers(0, 256, 32, dtype=np.uint8))
        return len(self.R) - 1

    def pair(self, x, y, o=0, dx=0.0, bits=0, ro=None, ry=None):
        i = self.left(x, y, o)
        self.right(f32(x) + f32(dx), y if ry is None else ry, o if ro is None else ro, of=i, bits=bits)
        return i

    def tables(self):
        n, m = len(self.L), len(self.R)
        return dict(kpL=_kp(self.L), descL=np.array(self.dL, np.uint8).reshape(n, 32), kpR=_kp(self.R),
                    descR=np.array(self.dR, np.uint8).reshape(m, 32))


def constant_pair_with_markers(W, H, slots):
    """A constant image (100) as the left eye; the right eye is the same except for marker pixels.  slots: (cx, cy, profile)
    with profile {column offset: weight}: weight w at offset j is spread over the rows cy-5..cy+5 except cy, at column
    cx + j, so that the 11x11 window centred (cx + inc, cy) sees sum(w for |j - inc| <= 5) as its SAD against the constant
    left window."""
    L = np.full((H, W), 100, np.uint8)
    R = L.copy()
    rows = [d for d in range(-5, 6) if d != 0]
    for cx, cy, prof in slots:
        for j, wgt in prof.items():
            left = int(wgt)
            for d in rows:
                put = min(left, 155)
                R[cy + d, cx + j] = 100 + put
                left -= put
            assert left == 0, "weight too large for one column"
    return L, R


def sad_profile(v, a, b, inc=0):
    """SAD v at incR = inc, v + a left of it, v + b right of it (see constant_pair_with_markers)."""
    p = {inc: v} if v else {}
    if a:
        p[inc - 6] = a
    if b:
        p[inc + 6] = b
    return p


def build_point_cases(synth_pair, photo_pair):
    """The constructed stereo-point cases.  synth_pair / photo_pair: (left, right) images of one size (752 x 480)."""
    cases = []
    SL = synth_pair[0]
    H, W = SL.shape
    sf, inv = scale_factors(8, 1.2)

    def add(name, L, R, P, **cfg):
        c = dict(name=name, W=W, H=H, nlevels=8, L=L, R=R, cfg=cfg, **P.tables(), **_empty_lines())
        cases.append(validate_tables(c))

    # --- A: the right eye equals the left one (a synthetic scene): bands, gates, Hamming limits, borders, disparity 0
    for nm, img in (("same_synth", SL), ("same_photo", photo_pair[0])):
        P = _Pairs(1)
        # row band of a right keypoint at y = 200.25, octave o: r = 2 * sf[o]
        for o in (0, 3, 7):
            r = f32(2.0) * sf[o]
            y = f32(200.25)
            lo, hi = math.floor(f32(y - r)), math.ceil(f32(y + r))
            x0 = 100 + 60 * o
            for k, row in enumerate((lo - 1, lo, hi, hi + 1)):
                # one right keypoint per left one, far apart in x from the others' disparity range is not possible (maxD =
                # fx): they are told apart by their descriptors instead
                i = P.left(x0 + 7 * k, row + 0.75, o)
                P.right(x0 + 7 * k, y, o, of=i, bits=0)
            i = P.left(x0 + 30, lo - 0.4, o); P.right(x0 + 30, y, o, of=i)          # trunc: lo - 1 (out); rounded: lo (in)
            i = P.left(x0 + 37, hi + 0.6, o); P.right(x0 + 37, y, o, of=i)          # trunc: hi (in); rounded: hi + 1 (out)
        # octave gate
        for k, ro in enumerate((1, 2, 4, 5)):
            P.pair(300 + 9 * k, 120, 3, ro=ro)
        P.pair(340, 120, 0, ro=1); P.pair(350, 120, 7, ro=6)
        # Hamming distance at the two limits
        for k, bits in enumerate((73, 74, 75, 76, 98, 99, 100, 101)):
            P.pair(200 + 13 * k, 300, 0, bits=bits)
        # equal best distances: the lower right index wins
        i = P.left(420, 330, 0); P.right(418, 330, 0, of=i, bits=10); P.right(420, 330, 0, of=i, bits=10)
        i = P.left(440, 330, 0); P.right(440, 330, 0, of=i, bits=10); P.right(437, 330, 0, of=i, bits=10)
        # shifts of the best right keypoint: bestincR from -5 to +5 on identical images
        for k, dx in enumerate((-5, -4, -3, -1, 0)):
            P.pair(150 + 40 * k, 400, 0, dx=dx)
        # borders at octave 0: the left window and the strip
        for (x, y) in ((5, 60), (4, 70), (W - 6, 80), (W - 5, 90), (300, 5), (310, 4), (320, H - 6), (330, H - 5)):
            P.pair(x, y, 0)
        P.pair(10, 100, 0); P.pair(12, 110, 0, dx=-3)                       # strip touches / leaves the left border
        i = P.left(W - 6, 130, 0); P.right(W - 12, 130, 0, of=i)              # endu == cols - 1
        i = P.left(W - 6, 140, 0); P.right(W - 11, 140, 0, of=i)              # endu == cols
        P.pair(W - 11, 170, 0)                                                # endu == cols, and a match behind it were it `>`
        i = P.left(20, 150, 0); P.right(-1, 150, 0, of=i)                     # iniu < 0
        P.pair(-2, 160, 0)                                                    # maxU < 0
        # the same at the top octave, in level coordinates c -> x = c * sf[7]
        lw, lh = int(round(W * float(inv[7]))), int(round(H * float(inv[7])))
        for (cx, cy) in ((5, 20), (4, 30), (lw - 6, 40), (lw - 5, 50), (60, 5), (70, 4), (80, lh - 6), (90, lh - 5), (10, 60), (9, 70)):
            P.pair(f32(cx) * sf[7], f32(cy) * sf[7], 7)
        i = P.left(f32(lw - 6) * sf[7], f32(80) * sf[7], 7); P.right(f32(lw - 12) * sf[7], f32(80) * sf[7], 7, of=i)
        i = P.left(f32(lw - 6) * sf[7], f32(90) * sf[7], 7); P.right(f32(lw - 11) * sf[7], f32(90) * sf[7], 7, of=i)
        P.pair(f32(lw - 11) * sf[7], f32(100) * sf[7], 7)
        add(nm, img, img, P)
    # --- B: natural pairs with sparse constructed keypoints: positive disparities, +5 exits
    for nm, (L, R) in (("synth_pair", synth_pair), ("photo_pair", photo_pair)):
        P = _Pairs(2)
        rng = np.random.default_rng(5)
        for k in range(120):
            x, y = float(rng.uniform(40, W - 40)), float(rng.uniform(20, H - 20))
            o = int(rng.integers(0, 8))
            P.pair(x, y, o, dx=-float(rng.uniform(0, 30)), bits=int(rng.integers(0, 80)))
        add(nm, L, R, P)
        add(nm + "_maxd_inf", L, R, P, stereo_maxd_inf=1)
    # --- C: the constant pair with markers: chosen SAD curves at octave 0
    def const_case(name, specs, extra=None, **cfg):
        """specs: (v, a, b, inc, uL - cxr) per keypoint, on a 40-pixel lattice"""
        P = _Pairs(3)
        slots = []
        for k, (v, a, b, inc, du) in enumerate(specs):
            cx, cy = 60 + 40 * (k % 16), 30 + 40 * (k // 16)
            slots.append((cx, cy, sad_profile(v, a, b, inc)))
            i = P.left(f32(cx + du), cy, 0); P.right(cx, cy, 0, of=i)
        L, R = constant_pair_with_markers(W, H, slots)
        if extra:
            extra(P)
        add(name, L, R, P, **cfg)
    # deltaR 0 (a == b), +-0.5 (one neighbour equal to the best: equal SADs, the first incR wins), 0.25; bestincR +-4, +-5
    const_case("const_curves", [(10, 5, 5, 0, 20), (10, 8, 0, 0, 20), (10, 24, 8, 0, 20), (0, 7, 7, -4, 20), (0, 7, 7, 4, 20),
                                (3, 9, 9, -5, 20), (3, 9, 9, 5, 20), (0, 0, 0, 0, 20),
                                # disparity exactly 0 with SAD != 0, slightly negative (-0.25), slightly positive (0.25)
                                (12, 5, 5, 0, 0), (12, 24, 8, 0, 0), (12, 8, 24, 0, 0), (12, 5, 5, -2, -2), (40, 5, 5, 0, 30)])
    # disparity == maxD (exclusive): a rig with maxD = 512 exactly; one inside by half a pixel
    const_case("const_maxd_512", [(10, 5, 5, -2, 510), (10, 5, 5, -2, 509.5), (10, 5, 5, 0, 512), (10, 5, 5, 0, 40)], bf=64.0, fx=512.0)
    # uR == minU and one float below it (default rig: maxD = fx)
    def minu(P):
        maxD = max_disparity(47.90639384423901, 435.2046959714599)
        for k, y in enumerate((400, 420)):
            uL = f32(700.0)
            mu = f32(uL - maxD)
            i = P.left(uL, y, 0)
            P.right(mu if k == 0 else np.nextafter(mu, f32(-np.inf)), y, 0, of=i)
    const_case("const_minu", [(10, 5, 5, 0, 20)], extra=minu)
    # the median cut
    th10 = None
    for m in range(1, 400):
        t = f32(f32(f32(1.5) * f32(1.4)) * f32(m))
        if float(t) == int(t):
            th10 = (m, int(t)); break
    assert th10 is not None
    med = lambda sads: [(v, 5, 5, 0, 20) for v in sads]
    const_case("median_even", med([10, 12, 14, 40]))
    const_case("median_odd", med([10, 12, 14, 16, 40]))
    const_case("median_one", med([17]))
    const_case("median_none", [(3, 9, 9, 5, 20)])
    const_case("median_zero", med([0, 0, 0, 5, 9]))
    const_case("median_equal_runs", med([7, 9, 9, 9, 9, 9, 30, 19, 18]))
    const_case("median_upper_bytes", med([256, 512, 768, 1024, 1280, 768, 512]))
    const_case("median_low_vs_high", med([10, 20, 22, 30]))                    # M/2 -> 22 (th 46.2); (M-1)/2 -> 20... see the mutation test
    const_case("median_gap", med([10, 10, 30, 30]))                            # median 30 keeps all; median 10 (low) cuts the two 30s
    const_case("median_at_threshold", med([th10[0], th10[0], th10[0], th10[1], th10[1] - 1]))
    return cases


def build_line_cases():
    """The constructed stereo-line cases (tables only; the images behind them do not matter to the line matcher)."""
    cases = []
    rng = np.random.default_rng(21)

    def add(name, W, H, L, R, dists, masks=None, **cfg):
        """L / R: end point rows; dists: {(i, j): Hamming distance} -- every other pair is far (random descriptors).
        masks = (left, right): instead, every descriptor is one base row with the given bit ranges flipped."""
        n1, n2 = len(L), len(R)
        ldL = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        ldR = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        if masks is not None:
            base = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
            def row(ranges):
                b = base.copy()
                for lo, hi in ranges:
                    b[lo:hi] ^= 1
                return np.packbits(b)
            ldL = np.array([row(r) for r in masks[0]], np.uint8).reshape(n1, 32)
            ldR = np.array([row(r) for r in masks[1]], np.uint8).reshape(n2, 32)
        done = set()
        for (i, j), d in dists.items():
            if j in done:
                # a right line shared by several left ones: the left descriptor is derived from the right one instead
                ldL[i] = _flip(ldR[j], d)
            else:
                ldR[j] = _flip(ldL[i], d); done.add(j)
        c = dict(name=name, W=W, H=H, nlevels=8, L=None, R=None, cfg=cfg, klL=_kl(L), ldL=ldL, klR=_kl(R), ldR=ldR, **_empty_points())
        cases.append(validate_tables(c))

    W, H = 752, 480
    # geometry: each left line with its own right partner (identical descriptor), vertical-ish lines 80 px long
    Ls, Rs, D = [], [], {}

    def pair(l, r, d=0):
        Ls.append(l); Rs.append(r); D[(len(Ls) - 1, len(Rs) - 1)] = d
    pair((100, 100, 104, 180), (90, 100, 94, 180))             # plain: disparity 10 at both ends
    pair((150, 100, 154, 180), (140, 180, 136, 100))           # right line stored end-first (walk swapped), steep
    pair((200, 100, 204, 180), (190, 100, 194, 175))           # partial overlap 75 / 80
    pair((250, 100, 254, 180), (240, 90, 244, 190))            # right contains left
    pair((300, 100, 304, 180), (290, 180.5, 294, 260))         # disjoint: starts in the cell row of the left end point
    pair((350, 110, 430, 114), (340, 111, 420, 111))           # horizontal right line: division by zero
    pair((400, 100, 404, 180), (410, 100, 414, 180))           # negative disparities
    pair((450, 100, 454, 180), (452, 100, 440, 180))           # mixed sign
    pair((500, 100, 504, 180), (499, 100, 503, 180))           # disparity == min_disp (1.0)
    pair((550, 100, 554, 180), (549.5, 100, 553.5, 180))       # disparity 0.5 < min_disp
    pair((600, 100, 604, 180), (580, 100, 600, 180))           # disparity ratio 4 / 20 < 0.7
    pair((100, 300, 180, 300.05), (90, 300, 170, 300.05))      # left |dy| <= line_horiz_th: overlap skipped, then rejected
    pair((200, 300, 280, 330), (190, 300, 270, 330))           # shallow pair
    pair((295, 300.5, 304, 309.5), (285, 300.5, 294, 309.5))   # both left end points in one cell (25, 30): NaN direction
    pair((5, 200, 9, 280), (2, 200, 6, 280))                   # window clipped at column 0
    pair((745, 200, 749, 280), (735, 200, 739, 280))           # window at column 63
    pair((740, 300, 770, 380), (730, 300, 760, 380))           # end point right of the image
    pair((60, 400, 64, 500), (50, 400, 54, 500))               # end point below the image
    pair((-20, 350, 20, 390), (-30, 350, 10, 390))             # start point left of the image
    pair((600, 300, 604, 300.009), (590, 300, 594, 300.009))   # length <= 0.01 needs |dy| > horizTh: see the case below
    add("lines_geometry", W, H, Ls, Rs, D)
    add("lines_geometry_no_lr", W, H, Ls, Rs, D, best_lr_matches=0)
    # thresholds that floats cannot meet with the default (decimal) settings: dyadic settings instead
    Ls, Rs, D = [], [], {}
    pair((100, 100, 104, 100.5), (90, 100, 94, 100.5))         # |dy| == line_horiz_th (0.5): rejected
    pair((150, 100, 154, 101), (140, 100, 144, 101))           # |dy| = 1 > 0.5
    pair((200, 100, 204, 200), (190, 100, 194, 175))           # overlap == stereo_overlap_th (0.75): rejected
    pair((250, 100, 254, 200), (240, 100, 244, 176))           # overlap 0.76
    pair((300, 100, 301, 100.5078125), (290, 100.5, 291, 100.5078125))   # length = eln - spn = 0.0078125 <= 0.01
    add("lines_dyadic_thresholds", W, H, Ls, Rs, D, line_horiz_th=0.5)
    # |dot| == lineSimTh: 512 x 384 makes the grid scale 1/8 exactly; left direction (1, 0), right (3, 4) / 5 and th = 0.6
    Ls, Rs, D = [], [], {}
    pair((100, 100, 180, 100), (100, 100, 124, 132))           # dot = 0.6: kept
    pair((100, 200, 180, 200), (100, 200, 123, 232))           # a little steeper: dropped
    pair((300, 100, 380, 100), (300, 100, 348, 164))           # (6, 8) / 10
    add("lines_dot_at_threshold", 512, 384, Ls, Rs, D, line_sim_th=0.6)
    # the column rule and the ratio test.  Left lines 0..3 share one window; right lines a, b next to each other.
    col = [(100 + 3 * k, 100, 104 + 3 * k, 180) for k in range(4)]
    ab = [(95, 100, 99, 180), (96, 100, 100, 180)]
    # distances to a: 20, 20, 12, 12 (the second 20 and the second 12 are dropped); to b: 40, 40, 32, 32
    m4 = ([[(0, 20)], [(20, 40)], [(40, 52)], [(52, 64)]], [[], [(100, 120)]])
    add("lines_column_equal", W, H, col, ab, {}, masks=m4)
    add("lines_column_equal_no_lr", W, H, col, ab, {}, masks=m4, best_lr_matches=0)
    # an equal distance later in the column must not become the best: left 0 and left 1 both see a at 30; left 1 sees b at 32.
    # The reference drops left 1's a, so b is its single candidate and matches; with the equal distance kept, a (30) is its
    # best and b (32) its second: 30 < 32 * 0.9 fails.
    add("lines_column_equal_second_best", W, H, col[:2], ab, {}, masks=([[(0, 30)], [(100, 130)]], [[], [(100, 130), (130, 162)]]))
    # ratio test at equality in double, where float arithmetic decides otherwise: 30 < 50 * 0.6
    add("lines_ratio_equality", W, H, [(100, 100, 104, 180)], [(95, 100, 99, 180), (96, 100, 100, 180)],
        {(0, 0): 30, (0, 1): 50}, min_ratio_12_l=0.6)
    add("lines_ratio_equality_09", W, H, [(100, 100, 104, 180)], [(95, 100, 99, 180), (96, 100, 100, 180)],
        {(0, 0): 9, (0, 1): 10})
    add("lines_single_candidate", W, H, [(100, 100, 104, 180)], [(95, 100, 99, 180)], {(0, 0): 200})
    # mutual check: left 0 takes a (10) but so does left 1 with a lower distance
    add("lines_mutual", W, H, col[:2], [(95, 100, 99, 180)], {(0, 0): 10, (1, 0): 5})
    # NaN left direction with a right line that the direction gate would otherwise drop
    add("lines_nan_direction", W, H, [(295, 300.5, 304, 309.5), (300, 340, 380, 340)], [(285, 300.5, 294, 309.5), (300, 330, 304, 400)],
        {(0, 0): 3, (1, 1): 3})
    # no lines on one side
    add("lines_none_right", W, H, col, [], {})
    # many lines: random tables large enough for the sliced phases on a device with kl_cap >= 192
    n = 150
    def rnd(n):
        sx = rng.uniform(0, W, n); sy = rng.uniform(0, H, n); a = rng.uniform(0, 2 * np.pi, n); ln = rng.uniform(12, 200, n)
        return [(float(f32(sx[i])), float(f32(sy[i])), float(f32(sx[i] + ln[i] * np.cos(a[i]))), float(f32(sy[i] + ln[i] * np.sin(a[i]))))
                for i in range(n)]
    Lr = rnd(n)
    Rr = [(l[0] - 8, l[1], l[2] - 9, l[3]) for l in Lr]
    add("lines_random_150", W, H, Lr, Rr, {(i, i): int(rng.integers(0, 40)) for i in range(n)})
    return cases


POINT_LABELS = [
    # exits
    "no_row_candidates", "maxU_negative", "no_candidate_below_TH_HIGH", "hamming_not_below_thOrbDist", "left_window_outside_level",
    "strip_iniu_negative", "strip_endu_ge_cols", "strip_window_outside_level", "bestincR_minus_L", "bestincR_plus_L",
    "disparity_negative", "disparity_ge_maxD", "matched", "matched_then_cut",
    # edges
    "band_low_end", "band_high_end", "band_just_below", "band_just_above", "vL_fraction_ge_half", "left_octave_0", "left_octave_top",
    "octave_gate_low_end", "octave_gate_high_end", "octave_gate_below", "octave_gate_above", "uR_eq_minU", "uR_eq_maxU", "maxD_inf",
    "best_hamming_74", "best_hamming_75", "best_hamming_99", "best_hamming_100", "equal_best_hamming",
    "window_touches_top_octave_0", "window_touches_bottom_octave_0", "window_touches_left_octave_0", "window_touches_right_octave_0",
    "window_touches_top_octave_top", "window_touches_bottom_octave_top", "window_touches_left_octave_top",
    "window_touches_right_octave_top", "strip_touches_left_octave_0", "strip_touches_right_octave_0",
    "strip_touches_left_octave_top", "strip_touches_right_octave_top", "equal_sads", "deltaR_at_half", "disparity_zero",
    "disparity_eq_maxD",
    # the median cut (per frame)
    "survivors_none", "survivors_one", "survivors_even", "survivors_odd", "median_zero", "cut_removes_everything",
    "equal_sads_around_median", "sads_differ_in_upper_bytes_only", "sad_at_thDist",
]
# Struck from the issue's list, with the reason (see test_independent_matchers.py for the argument in full):
POINT_LABELS_UNREACHABLE = {
    "deltaR_nan": "the best SAD is the FIRST strict minimum, so dist1 > dist2 and dist3 >= dist2: dist1 + dist3 - 2 dist2 > 0, exactly, in float",
    "deltaR_outside": "with a = dist1 - dist2 > 0 and b = dist3 - dist2 >= 0, deltaR = (a - b) / (2 (a + b)) lies in [-0.5, 0.5]; +-1 and beyond cannot occur",
}
LINE_LABELS = [
    "no_candidates", "ratio_test_failed", "mutual_check_failed", "rejected_min_disp", "rejected_left_horizontal", "rejected_overlap",
    "matched", "no_lines",
    "left_endpoints_in_one_cell", "nan_direction_candidate_kept", "dot_eq_lineSimTh", "window_clipped_at_column_0",
    "window_at_column_63", "left_endpoint_outside_grid", "right_cells_outside_grid", "right_steep", "right_shallow",
    "right_walk_swapped", "right_walk_forward", "equal_distance_in_column_dropped", "best_lr_matches_off", "single_candidate",
    "ratio_test_at_equality", "right_horizontal_division_by_zero", "disparities_of_mixed_sign", "disparities_both_negative",
    "disparity_ratio_reset", "disp_eq_min_disp", "dy_eq_line_horiz_th", "overlap_eq_stereo_overlap_th", "overlap_length_le_0.01",
    "overlap_disjoint", "overlap_right_contains_left", "overlap_partial", "overlap_left_horizontal",
]
LINE_LABELS_UNREACHABLE = {
    "rejected_right_horizontal": "sp_r(1) / ep_r(1) are overwritten with sp_l(1) / ep_l(1) before the test, so it repeats the left line's test",
}


# ---------------------------------------------------------------------------------------------------------------------
# The projection searches: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, ...) (ORBmatcher.cc:2179-2323) and
# ORBmatcher::SearchByProjection(F, vpMapPoints, th, ...) for the rectified case (ORBmatcher.cc:44-143), on pli_proj_query
# records (include/pli_frontend.h: the projection, radius, level range, angle and flags of one map point), with
# Frame::GetFeaturesInArea / PosInGrid / AssignFeaturesToGrid (Frame.cc:451-482, 774-855) and ComputeThreeMaxima
# (ORBmatcher.cc:2449-2490).  Shaped without grid lists: every keypoint gets its cell once; a query's candidates are the
# keypoints whose cell lies in its cell range, taken in the order the reference walks them (cell column, cell row, index),
# and the best / second best come from one stable sort by distance.
# ---------------------------------------------------------------------------------------------------------------------
PROJ_QUERY_DT = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                          ("angle", "<f4"), ("valid", "<i4")])
HISTO_LENGTH = 30
PROJ_K = 64            # (the kernels keep this many candidates per query before they rescan; the tests straddle it)


def _cells(kp, bounds):
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    gw, gh = f32(f32(GRID_COLS) / f32(maxx - minx)), f32(f32(GRID_ROWS) / f32(maxy - miny))
    px = np.array([c_round(v) for v in ((kp["x"] - minx).astype(f32) * gw).astype(f32)], np.int64).reshape(-1)
    py = np.array([c_round(v) for v in ((kp["y"] - miny).astype(f32) * gh).astype(f32)], np.int64).reshape(-1)
    ingrid = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    return px, py, ingrid, gw, gh


def _area(Q, kp, px, py, ingrid, bounds, gw, gh, tags):
    """GetFeaturesInArea: candidate indices in the reference's walking order, or None when a cell range is empty."""
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    u, v, r = f32(Q["u"]), f32(Q["v"]), f32(Q["radius"])
    c0 = max(0, int(math.floor(f32(f32(f32(u - minx) - r) * gw))))
    if c0 >= GRID_COLS:
        return None
    c1 = min(GRID_COLS - 1, int(math.ceil(f32(f32(f32(u - minx) + r) * gw))))
    if c1 < 0:
        return None
    r0 = max(0, int(math.floor(f32(f32(f32(v - miny) - r) * gh))))
    if r0 >= GRID_ROWS:
        return None
    r1 = min(GRID_ROWS - 1, int(math.ceil(f32(f32(f32(v - miny) + r) * gh))))
    if r1 < 0:
        return None
    lo, hi = int(Q["min_level"]), int(Q["max_level"])
    m = ingrid & (px >= c0) & (px <= c1) & (py >= r0) & (py <= r1)
    near = m & (np.abs((kp["x"] - u).astype(f32)) < r) & (np.abs((kp["y"] - v).astype(f32)) < r)
    if lo > 0 or hi >= 0:
        o = kp["octave"]
        for name, mm in (("octave_eq_min_level", o == lo), ("octave_below_min_level", o == lo - 1)):
            if (near & mm).any() and lo > 0:
                tags.append(name)
        if hi >= 0:
            for name, mm in (("octave_eq_max_level", o == hi), ("octave_above_max_level", o == hi + 1)):
                if (near & mm).any():
                    tags.append(name)
        near = near & (o >= lo)
        if hi >= 0:
            near = near & (o <= hi)
    idx = np.flatnonzero(near)
    return idx[np.lexsort((idx, py[idx], px[idx]))]


def _ur_gate(Q, idx, uright, tags):
    ur = uright[idx]
    er = np.abs((f32(Q["ur"]) - ur).astype(f32))
    has = ur > 0
    if (~has).any():
        tags.append("ur_gate_absent")
    if (has & (er <= f32(Q["radius"]))).any():
        tags.append("ur_gate_passed")
    if (has & (er > f32(Q["radius"]))).any():
        tags.append("ur_gate_rejected")
    if (has & (er == f32(Q["radius"]))).any():
        tags.append("ur_error_eq_radius")
    return idx[~(has & (er > f32(Q["radius"])))]


def three_maxima(sizes):
    """ComputeThreeMaxima: the three fullest bins (equal sizes: the lower bin first; empty bins never), then the 10 % rule."""
    order = [i for i in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i)) if sizes[i] > 0][:3]
    ind = order + [-1] * (3 - len(order))
    mx = [sizes[i] if i >= 0 else 0 for i in ind]
    if f32(mx[1]) < f32(f32(0.1) * f32(mx[0])):
        return [ind[0], -1, -1], "maxima_one_kept"
    if f32(mx[2]) < f32(f32(0.1) * f32(mx[0])):
        return [ind[0], ind[1], -1], "maxima_two_kept"
    return ind, "maxima_three_kept"


def search_by_projection(q, qdesc, kp, desc, uright, bounds, check_ori=True, occupied=None, misread=()):
    """-> nmatches, best (after the rotation filter), raw (before it), exits, call_tags.  misread: deliberate misreadings that
    tests/test_ref_pin_match.py wants rejected ("min_last": of equal distances the last in walking order; "index_order": the window
    walked in index order; "rot_trunc": the rotation bin by truncation; "th_high_strict": bestDist < TH_HIGH; "bounds_half_open":
    a projection on mnMaxX / mnMaxY leaves)."""
    nq, ncur = len(q), len(kp)
    px, py, ingrid, gw, gh = _cells(kp, bounds)
    assigned = np.zeros(ncur, bool) if occupied is None else (np.asarray(occupied) != 0)
    best = np.full(nq, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    exits = [()] * nq
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    for i in range(nq):
        Q = q[i]
        tags = []
        if not Q["valid"]:
            exits[i] = ("invalid",); continue
        if Q["u"] < minx or Q["u"] > maxx or Q["v"] < miny or Q["v"] > maxy:
            exits[i] = ("outside_bounds",); continue
        if "bounds_half_open" in misread and (Q["u"] == maxx or Q["v"] == maxy):
            exits[i] = ("outside_bounds",); continue
        idx = _area(Q, kp, px, py, ingrid, bounds, gw, gh, tags)
        if idx is not None and "index_order" in misread:
            idx = np.sort(idx)
        if idx is None or idx.size == 0:
            exits[i] = ("no_features_in_area",) + tuple(tags); continue
        if assigned[idx].any():
            tags.append("occupied_keypoint_skipped")
        gated = _ur_gate(Q, idx, uright, tags)
        d_all = hamming(qdesc[i][None], desc[gated]) if gated.size else np.zeros(0, np.int32)
        nk = int((d_all <= TH_HIGH).sum())
        if nk in (PROJ_K, PROJ_K + 1):
            tags.append("window_holds_PROJ_K" if nk == PROJ_K else "window_holds_PROJ_K_plus_1")
        free = ~assigned[gated]
        cand, d = gated[free], d_all[free]
        if cand.size == 0:
            exits[i] = ("no_candidate",) + tuple(tags); continue
        k = int(np.argmin(d))                       # first minimum in walking order; 256 can never be undercut: dist <= 256
        if "min_last" in misread:
            k = len(d) - 1 - int(np.argmin(d[::-1]))
        if int(d[k]) in (TH_HIGH, TH_HIGH + 1):
            tags.append("distance_eq_TH_HIGH" if int(d[k]) == TH_HIGH else "distance_eq_TH_HIGH_plus_1")
        if int(d[k]) >= 256 or int(d[k]) > TH_HIGH - ("th_high_strict" in misread):
            exits[i] = ("distance_above_TH_HIGH",) + tuple(tags); continue
        b = int(cand[k])
        if Q["valid"] & 2:
            tags.append("map_point_without_observations")
        else:
            assigned[b] = True
        best[i] = b
        if check_ori:
            rot = f32(f32(Q["angle"]) - f32(kp["angle"][b]))
            if rot < 0:
                rot = f32(rot + f32(360.0))
            if float(rot) == 360.0:
                tags.append("rot_eq_360")
            elif float(rot) > 0 and float(rot) % 12.0 == 0:
                tags.append("rot_multiple_of_12")
            if float(rot) % 30.0 == 15.0:
                tags.append("rot_at_half_bin")
            bn = int(c_round(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH)))))
            if "rot_trunc" in misread:
                bn = int(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
            if bn == HISTO_LENGTH:
                bn = 0
            hist[bn].append(i)
        exits[i] = ("matched",) + tuple(tags)
    raw = best.copy()
    ctags = set()
    if check_ori:
        keep, which = three_maxima([len(h) for h in hist])
        if raw.max(initial=-1) >= 0:
            ctags.add(which)
        for bn in range(HISTO_LENGTH):
            if bn not in keep:
                for i in hist[bn]:
                    best[i] = -1
                    exits[i] = ("matched_then_rotation_filtered",) + exits[i][1:]
    return int((best >= 0).sum()), best, raw, exits, ctags


def search_local_map(q, qdesc, kp, desc, uright, occupied, bounds, nnratio, misread=()):
    """-> nmatches, best, exits.  misread: deliberate misreadings that tests/test_ref_pin_match.py wants rejected ("ratio_double":
    the ratio test in double; "ratio_any_level": the ratio test whatever the two levels; "index_order": the window walked in
    index order; "ur_gate_ge": the right coordinate leaves at |error| >= radius; "th_high_strict": bestDist < TH_HIGH)."""
    nq, ncur = len(q), len(kp)
    px, py, ingrid, gw, gh = _cells(kp, bounds)
    taken = np.zeros(ncur, bool) if occupied is None else (np.asarray(occupied) != 0)
    best = np.full(nq, -1, np.int32)
    exits = [()] * nq
    for i in range(nq):
        Q = q[i]
        tags = []
        if not Q["valid"]:
            exits[i] = ("invalid",); continue
        idx = _area(Q, kp, px, py, ingrid, bounds, gw, gh, tags)
        if idx is not None and "index_order" in misread:
            idx = np.sort(idx)
        if idx is None or idx.size == 0:
            exits[i] = ("no_features_in_area",) + tuple(tags); continue
        if taken[idx].any():
            tags.append("occupied_keypoint_skipped")
        gated = _ur_gate(Q, idx, uright, tags)
        if "ur_gate_ge" in misread:
            gated = gated[~((uright[gated] > 0) & (np.abs((f32(Q["ur"]) - uright[gated]).astype(f32)) == f32(Q["radius"])))]
        d_all = hamming(qdesc[i][None], desc[gated]) if gated.size else np.zeros(0, np.int32)
        nk = int((d_all <= TH_HIGH).sum())
        if nk in (PROJ_K, PROJ_K + 1):
            tags.append("window_holds_PROJ_K" if nk == PROJ_K else "window_holds_PROJ_K_plus_1")
        free = ~taken[gated]
        cand, d = gated[free], d_all[free]
        if cand.size == 0:
            exits[i] = ("no_candidate",) + tuple(tags); continue
        o = np.argsort(d, kind="stable")
        d1, l1, b = int(d[o[0]]), int(kp["octave"][cand[o[0]]]), int(cand[o[0]])
        d2, l2 = (int(d[o[1]]), int(kp["octave"][cand[o[1]]])) if o.size > 1 else (256, -1)
        if d2 >= 256:
            d2, l2 = 256, -1
        if d1 in (TH_HIGH, TH_HIGH + 1):
            tags.append("distance_eq_TH_HIGH" if d1 == TH_HIGH else "distance_eq_TH_HIGH_plus_1")
        if d1 >= 256 or d1 > TH_HIGH - ("th_high_strict" in misread):
            exits[i] = ("distance_above_TH_HIGH",) + tuple(tags); continue
        lim = f32(f32(nnratio) * f32(d2))
        fails = float(d1) > float(f32(nnratio)) * float(d2) if "ratio_double" in misread else f32(d1) > lim
        if l1 == l2 or "ratio_any_level" in misread:
            if f32(d1) == lim:
                tags.append("ratio_at_equality")
            if fails:
                exits[i] = ("ratio_test_failed_same_level",) + tuple(tags); continue
            tags.append("ratio_test_passed_same_level")
        else:
            tags.append("second_best_on_another_level" if l2 >= 0 else "single_candidate")
        taken[b] = True
        best[i] = b
        exits[i] = ("matched",) + tuple(tags)
    return int((best >= 0).sum()), best, exits


PROJ_LABELS = ["invalid", "outside_bounds", "no_features_in_area", "no_candidate", "distance_above_TH_HIGH", "matched",
               "matched_then_rotation_filtered", "distance_eq_TH_HIGH", "distance_eq_TH_HIGH_plus_1", "octave_eq_min_level",
               "octave_below_min_level", "octave_eq_max_level", "octave_above_max_level", "ur_gate_absent", "ur_gate_passed",
               "ur_gate_rejected", "ur_error_eq_radius", "occupied_keypoint_skipped", "map_point_without_observations",
               "window_holds_PROJ_K", "window_holds_PROJ_K_plus_1", "rot_eq_360", "rot_multiple_of_12", "rot_at_half_bin",
               "maxima_one_kept", "maxima_two_kept", "maxima_three_kept"]
LOCAL_MAP_LABELS = ["invalid", "no_features_in_area", "no_candidate", "distance_above_TH_HIGH", "matched", "ratio_test_failed_same_level",
                    "ratio_test_passed_same_level", "ratio_at_equality", "second_best_on_another_level", "single_candidate",
                    "distance_eq_TH_HIGH", "distance_eq_TH_HIGH_plus_1", "octave_eq_min_level", "octave_below_min_level",
                    "octave_eq_max_level", "octave_above_max_level", "ur_gate_absent", "ur_gate_passed", "ur_gate_rejected",
                    "occupied_keypoint_skipped", "window_holds_PROJ_K", "window_holds_PROJ_K_plus_1"]


# ---- the random / tie-rich generators of tests/test_gpu_parity.py (same seeds, same draws) ---------------------------
def local_map_ties_tables(seed=11, ncur=700, nq=500):
    rng = np.random.default_rng(seed)
    kp = np.zeros(ncur, KEYPOINT_DT)
    kp["x"] = rng.uniform(0, 640, ncur).astype(np.float32); kp["y"] = rng.uniform(0, 480, ncur).astype(np.float32)
    kp["octave"] = rng.integers(0, 4, ncur)
    desc = (rng.integers(0, 2, (ncur, 32)) * 255).astype(np.uint8)       # distances are multiples of 8
    ur = np.where(rng.random(ncur) < 0.5, kp["x"] - rng.uniform(0, 30, ncur), -1).astype(np.float32)
    q = np.zeros(nq, PROJ_QUERY_DT)
    src = rng.integers(0, ncur, nq)
    q["u"] = kp["x"][src] + rng.uniform(-4, 4, nq).astype(np.float32); q["v"] = kp["y"][src] + rng.uniform(-4, 4, nq).astype(np.float32)
    q["radius"] = rng.uniform(10, 60, nq).astype(np.float32)
    q["ur"] = q["u"] - rng.uniform(0, 30, nq).astype(np.float32)
    q["min_level"] = rng.integers(-1, 3, nq); q["max_level"] = q["min_level"] + rng.integers(0, 3, nq)
    q["valid"] = rng.random(nq) < 0.9
    qd = desc[src].copy()
    flip = rng.random((nq, 32)) < 0.25
    qd[flip] ^= 255
    return q, qd, kp, desc, ur, (0.0, 640.0, 0.0, 480.0)


def dense_window_tables(ncur, nq):
    """-> q, qd, kp, desc, ur, occ, bounds, rng (the generator, for the draws the caller makes after these)."""
    rng = np.random.default_rng(ncur)
    kp = np.zeros(ncur, KEYPOINT_DT)
    kp["x"] = rng.uniform(0, 640, ncur).astype(np.float32); kp["y"] = rng.uniform(0, 480, ncur).astype(np.float32)
    kp["octave"] = rng.integers(0, 8, ncur); kp["angle"] = rng.uniform(0, 360, ncur).astype(np.float32)
    desc = rng.integers(0, 256, (ncur, 32), dtype=np.uint8)
    desc[:, 8:] = desc[0, 8:]                                            # close descriptors: most candidates pass the limit
    ur = np.where(rng.random(ncur) < 0.5, kp["x"] - rng.uniform(0, 30, ncur), -1).astype(np.float32)
    occ = (rng.random(ncur) < 0.2).astype(np.uint8)
    q = np.zeros(nq, PROJ_QUERY_DT)
    src = rng.integers(0, ncur, nq)
    q["u"] = kp["x"][src] + rng.uniform(-4, 4, nq).astype(np.float32); q["v"] = kp["y"][src] + rng.uniform(-4, 4, nq).astype(np.float32)
    q["radius"] = np.where(rng.random(nq) < 0.5, rng.uniform(5, 30, nq), rng.uniform(60, 200, nq)).astype(np.float32)
    q["ur"] = q["u"] - rng.uniform(0, 30, nq).astype(np.float32)
    q["min_level"] = rng.integers(-1, 3, nq); q["max_level"] = np.where(rng.random(nq) < 0.3, -1, q["min_level"] + rng.integers(0, 6, nq))
    q["angle"] = (kp["angle"][src] + rng.choice([0.0, 0.0, 0.0, 90.0, 200.0], nq)).astype(np.float32) % 360
    q["valid"] = rng.random(nq) < 0.95
    qd = desc[src].copy()
    qd[:, :3] ^= rng.integers(0, 256, (nq, 3), dtype=np.uint8)
    return q, qd, kp, desc, ur, occ, (0.0, 640.0, 0.0, 480.0), rng


# ---- constructed projection cases --------------------------------------------------------------------------------------
class _Proj:
    """Queries on a 40-pixel lattice of a 640 x 480 frame, radius 10: the items do not see each other."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.q, self.qd, self.kp, self.d, self.ur, self.occ = [], [], [], [], [], []
        self.slot = 0

    def place(self):
        s = self.slot; self.slot += 1
        assert s < 16 * 11
        return 20.0 + 40 * (s % 16), 20.0 + 40 * (s // 16)

    def query(self, u, v, radius=10.0, ur=None, lo=0, hi=-1, angle=0.0, valid=1):
        self.q.append((u, v, radius, u - 5.0 if ur is None else ur, lo, hi, angle, valid))
        self.qd.append(self.rng.integers(0, 256, 32, dtype=np.uint8))
        return len(self.q) - 1

    def key(self, x, y, of, bits=0, octave=0, angle=0.0, ur=-1.0, occ=0):
        self.kp.append((x, y, octave, angle)); self.d.append(_flip(self.qd[of], bits)); self.ur.append(ur); self.occ.append(occ)
        return len(self.kp) - 1

    def item(self, bits=0, **kw):
        u, v = self.place()
        kq = {k: kw.pop(k) for k in ("lo", "hi", "angle", "valid", "ur") if k in kw}
        i = self.query(u, v, **kq)
        self.key(u, v, i, bits, **kw)
        return i

    def tables(self):
        q = np.zeros(len(self.q), PROJ_QUERY_DT)
        for i, r in enumerate(self.q):
            q[i] = r
        kp = np.zeros(len(self.kp), KEYPOINT_DT)
        for i, (x, y, o, a) in enumerate(self.kp):
            kp["x"][i], kp["y"][i], kp["octave"][i], kp["angle"][i] = x, y, o, a
        n = len(self.kp)
        return dict(q=q, qd=np.array(self.qd, np.uint8).reshape(len(self.q), 32), kp=kp, desc=np.array(self.d, np.uint8).reshape(n, 32),
                    ur=np.array(self.ur, np.float32), occ=np.array(self.occ, np.uint8), bounds=(0.0, 640.0, 0.0, 480.0))


def build_projection_cases():
    """-> list of dicts: name, q, qd, kp, desc, ur, occ, bounds, nnratio (the searches run each with and without `occ`)."""
    cases = []

    def edges(P):
        for bits in (99, 100, 101, 102):
            P.item(bits)
        for o in (1, 2, 4, 5):                                   # level gate [2, 4] at both ends
            P.item(3, lo=2, hi=4, octave=o)
        P.item(3, lo=2, hi=-1, octave=1); P.item(3, lo=2, hi=-1, octave=7); P.item(3, lo=0, hi=3, octave=4)
        P.item(3, ur=-1.0)                                       # no right coordinate: no gate
        u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.0)      # |error| == radius: passes
        u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.5)      # rejected
        u, v = P.place(); i = P.query(u, v, ur=u - 5.0); P.key(u, v, i, 3, ur=u - 15.5); P.key(u + 1, v, i, 9, ur=u - 6.0)
        u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2, occ=1); P.key(u + 2, v, i, 7)   # the nearest is occupied
        u, v = P.place(); i = P.query(u, v); P.key(u, v, i, 2, occ=1)                           # only an occupied one
        u, v = P.place(); i = P.query(u, v, valid=3); k = P.key(u, v, i, 2)                     # no observations: stays free ...
        j = P.query(u + 1, v); P.qd[j] = _flip(P.qd[i], 1)                                      # ... for the query behind it
        u, v = P.place(); i = P.query(u, v); k = P.key(u, v, i, 2)                              # taken by the first, so the second
        j = P.query(u + 1, v); P.qd[j] = _flip(P.qd[i], 1); P.key(u + 3, v, i, 30)              # gets the farther one
        P.item(2, valid=0)
        P.query(-3.0, 100.0); P.query(645.0, 100.0); P.query(100.0, -2.0); P.query(100.0, 481.0)
        P.query(5000.0, 100.0); P.query(100.0, 5000.0)
        # equal distances: the first in walking order (cell column, cell row, index) wins, not the lowest index
        u, v = P.place(); i = P.query(u, v, radius=30.0); P.key(u + 12, v, i, 5); P.key(u - 12, v, i, 5); P.key(u - 12, v - 12, i, 5)

    P = _Proj(31); edges(P)
    cases.append(dict(name="proj_edges", nnratio=0.8, **P.tables()))

    # windows that hold exactly PROJ_K and PROJ_K + 1 candidates (within radius, inside the level range, distance <= TH_HIGH)
    P = _Proj(32)
    for n in (PROJ_K, PROJ_K + 1, PROJ_K - 1):
        u, v = 100.0 + 200 * (n - PROJ_K + 1), 200.0
        i = P.query(u, v, radius=30.0)
        for k in range(n):
            P.key(u - 9 + 2 * (k % 9), v - 9 + 2 * (k // 9), i, 10 + (k * 7) % 50, octave=k % 3)
        P.key(u + 5, v + 5, i, 150)                               # beyond TH_HIGH: in the window, not a candidate
        j = P.query(u + 1, v + 1, radius=30.0); P.qd[j] = _flip(P.qd[i], 2)
    cases.append(dict(name="proj_window_PROJ_K", nnratio=0.8, **P.tables()))

    # the rotation histogram: bin = round(rot / 30) (factor = 1 / HISTO_LENGTH: bins are 30 degrees wide, their boundaries at
    # 15 + 30 k; multiples of 12 degrees and rot == 360 are there because the issue names them)
    def rot_case(name, groups):
        P = _Proj(33)
        for rot, n, ka in groups:
            for _ in range(n):
                P.item(1, angle=float(f32(ka) + f32(rot)) if rot >= 0 else 0.0, **({"angle": 0.0} if False else {}))
                P.kp[-1] = P.kp[-1][:3] + (ka if rot >= 0 else -rot,)
        cases.append(dict(name=name, nnratio=0.8, **P.tables()))
    rot_case("proj_rot_three", [(0.0, 10, 20.0), (12.0, 2, 0.0), (24.0, 2, 0.0), (36.0, 3, 0.0), (60.0, 2, 0.0), (15.0, 1, 0.0),
                                (45.0, 1, 0.0), (348.0, 1, 0.0), (-1e-6, 1, 0.0), (300.0, 1, 5.0)])
    rot_case("proj_rot_one", [(90.0, 30, 10.0), (180.0, 2, 0.0), (270.0, 1, 0.0), (0.0, 2, 0.0)])
    rot_case("proj_rot_two", [(90.0, 30, 10.0), (180.0, 3, 0.0), (270.0, 2, 0.0), (0.0, 1, 0.0)])

    # the local map's ratio rule: best / second best on one level or two, nnratio products at the float boundary
    P = _Proj(34)
    for d1, d2, same in ((8, 10, True), (9, 10, True), (7, 10, True), (16, 20, True), (17, 20, True), (80, 100, True), (81, 100, True),
                         (40, 50, True), (41, 50, True), (9, 10, False), (50, 50, True), (50, 50, False), (100, 120, True)):
        u, v = P.place(); i = P.query(u, v)
        P.key(u + 1, v, i, d2, octave=2); P.key(u, v, i, d1, octave=2 if same else 3)
    P.item(100); P.item(101)
    cases.append(dict(name="local_map_ratio", nnratio=0.8, **P.tables()))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# The stereo corpus: the oracle pipeline's own tables plus the constructed cases, with the pyramids the oracle builds.
# ---------------------------------------------------------------------------------------------------------------------
_CORPUS = {}


def stereo_corpus(po):
    """po: oracle.pyoracle.  Every case as a dict with cfg (oracle Config), tables and, for point cases, the two pyramids
    (pyr = None: a line-only case).  Built once per process."""
    if "c" in _CORPUS:
        return _CORPUS["c"]
    from pli_slam_amd import realdata, synth
    W, H = 752, 480

    def pipeline(name, L, R, **over):
        cfg = po.default_config(L.shape[1], L.shape[0], orb_nfeatures=1200, lsd_nfeatures=100, **over)
        fr = po.Frame(cfg)
        t = {}
        for eye, img, k in ((0, L, "L"), (1, R, "R")):
            _, t["kp" + k], t["desc" + k] = fr.orb_extract(eye, img)
            _, t["kl" + k], t["ld" + k] = fr.line_extract(eye, img)
        pyr = [[fr.pyramid(e, l) for l in range(8)] for e in (0, 1)]
        return dict(name="pipeline_" + name, W=L.shape[1], H=L.shape[0], nlevels=8, cfg=cfg, pyr=pyr, L=L, R=R, **t)

    photo = realdata.frames_752x480(1, seed=1)[0]
    pairs = {"synth0": synth.make_stereo_pair(0, W, H), "synth9": synth.make_stereo_pair(9, W, H), "photo": photo}
    cases = [pipeline(n, L, R) for n, (L, R) in pairs.items()]
    Lm, Rm, _ = realdata.motorcycle()
    cases.append(pipeline("motorcycle", Lm, Rm, bf=100.0, fx=500.0))
    for c in build_point_cases(pairs["synth0"], photo):
        c["cfg"] = po.default_config(c["W"], c["H"], **c["cfg"])
        fr = po.Frame(c["cfg"])
        c["pyr"] = []
        for eye, img in ((0, c["L"]), (1, c["R"])):
            fr.orb_extract(eye, img)
            c["pyr"].append([fr.pyramid(eye, l) for l in range(8)])
        cases.append(validate_tables(c))
    for c in build_line_cases():
        c["cfg"] = po.default_config(c["W"], c["H"], **c["cfg"])
        c["pyr"] = None
        cases.append(c)
    _CORPUS["c"] = cases
    return cases


def run_points(c, rules=REF):
    cfg = c["cfg"]
    sf, inv = scale_factors(cfg.orb_nlevels, cfg.orb_scale_factor)
    maxD = max_disparity(cfg.bf, cfg.fx, bool(cfg.stereo_maxd_inf))
    return stereo_points(c["kpL"], c["descL"], c["kpR"], c["descR"], c["pyr"][0], c["pyr"][1], sf, inv, cfg.bf, maxD, rules)
