"""ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:269-470), the branch F.Nleft != -1 (:342-369,
:373-433: a frame of two KannalaBrandt8 cameras, its N = Nleft + Nright features the left camera's first), restated in Python: the
checker of pli_search_by_bow_two_cameras (tests/test_bow_two_cameras_gpu.py).  CPU only, integers only: no margins are needed.

  search_scalar   the reference's control flow: per keyframe feature the running bestDist1 / bestDist2 / bestIdxF over the still
                  unmatched candidates < Nleft and bestDist1R / bestDist2R / bestIdxFR over the others (strict <), then the nesting
                  as written: only if bestDist1 <= TH_LOW, the left match on its ratio test, and - whether or not it was taken -
                  the right match when bestDist1R <= TH_LOW, with no ratio test (`|| true`, :405).  Every exit counted.
  search_closed   a second form, numpy per node: the two sides' free candidates sorted by (distance, index).

The angles are the caller's tables (kf: mvKeysUn or mvKeys / mvKeysRight, :379-382; frame: mvKeys / mvKeysRight, :386-389, :416-419).
"""
import bisect
import os
import re
from collections import Counter
from dataclasses import dataclass, replace

import numpy as np
import pytest

from test_bow_search_cpu import (F32, HISTO_LENGTH, POP8, TH_LOW, desc_with_bits, distance, feature_vector, keyframe_of, rot_bin,
                                 search_by_bow, three_maxima)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXITS = ("invalid_mp", "closed_candidate", "no_left_within_th_low", "left_ratio_failed", "left_taken", "right_above_th_low",
         "right_taken", "right_taken_after_left_failed", "right_taken_with_equal_second", "left_tie", "right_tie",
         "filtered_left", "filtered_right")


@dataclass(frozen=True)
class Rules:
    """The readings that the mutation tests flip; the defaults are the reference's."""
    right_independent: bool = False        # the right match does not ask for bestDist1 <= TH_LOW
    right_ratio: bool = False              # a ratio test on the right match
    right_after_left: bool = False         # the right match only after an accepted left match
    one_top2: bool = False                 # one best / second best over both cameras (the Nleft == -1 branch)


REF = Rules()


def search_scalar(kf_desc, kf_angle, kf_node, kf_valid, f_desc, f_angle, f_node, f_nleft, nnratio=0.7, check_orientation=True,
                  exits=None, rules=REF):
    """-> (matches[nf] = keyframe feature or -1, nmatches)."""
    exits = exits if exits is not None else Counter()
    nf = len(f_node)
    matches = [-1] * nf
    fv_kf, fv_f = feature_vector(kf_node), feature_vector(f_node)
    kf_keys, f_keys = sorted(fv_kf), sorted(fv_f)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    ratio = F32(nnratio)
    nmatches = 0

    def take(ikf, i_f):
        nonlocal nmatches
        matches[i_f] = ikf
        if check_orientation:
            rot_hist[rot_bin(kf_angle[ikf], f_angle[i_f])].append(i_f)
        nmatches += 1
    a, b = 0, 0
    while a < len(kf_keys) and b < len(f_keys):
        if kf_keys[a] == f_keys[b]:
            for ikf in fv_kf[kf_keys[a]]:
                if not kf_valid[ikf]:
                    exits["invalid_mp"] += 1; continue
                best1, idx, best2 = 256, -1, 256
                best1r, idxr, best2r = 256, -1, 256
                for i_f in fv_f[f_keys[b]]:
                    if matches[i_f] >= 0:
                        exits["closed_candidate"] += 1; continue
                    d = distance(kf_desc[ikf], f_desc[i_f])
                    left = i_f < f_nleft or rules.one_top2
                    if left and d < best1:
                        best2, best1, idx = best1, d, i_f
                    elif left and d < best2:
                        best2 = d
                        exits["left_tie"] += d == best1
                    if not left and d < best1r:
                        best2r, best1r, idxr = best1r, d, i_f
                    elif not left and d < best2r:
                        best2r = d
                        exits["right_tie"] += d == best1r
                left_taken = False
                if best1 <= TH_LOW:
                    if F32(best1) < F32(ratio * F32(best2)):
                        take(ikf, idx)
                        left_taken = True
                        exits["left_taken"] += 1
                    else:
                        exits["left_ratio_failed"] += 1
                else:
                    exits["no_left_within_th_low"] += 1
                if best1 <= TH_LOW or rules.right_independent:
                    if best1r <= TH_LOW:
                        if rules.right_after_left and not left_taken:
                            continue
                        if rules.right_ratio and not F32(best1r) < F32(ratio * F32(best2r)):
                            continue
                        take(ikf, idxr)
                        exits["right_taken"] += 1
                        exits["right_taken_after_left_failed"] += not left_taken
                        exits["right_taken_with_equal_second"] += best1r == best2r
                    else:
                        exits["right_above_th_low"] += 1
            a += 1
            b += 1
        elif kf_keys[a] < f_keys[b]:
            a = bisect.bisect_left(kf_keys, f_keys[b], a)
        else:
            b = bisect.bisect_left(f_keys, kf_keys[a], b)
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for i_f in rot_hist[i]:
                exits["filtered_left" if i_f < f_nleft else "filtered_right"] += 1
                matches[i_f] = -1
                nmatches -= 1
    return np.array(matches, np.int32), nmatches


def search_closed(kf_desc, kf_angle, kf_node, kf_valid, f_desc, f_angle, f_node, f_nleft, nnratio=0.7, check_orientation=True):
    """The same result by another route: per common node the distance matrix; a keyframe feature's best and second best of a
    camera are the two smallest (distance, frame index) pairs among that camera's free candidates."""
    nf = len(f_node)
    kf_desc, f_desc = np.asarray(kf_desc, np.uint8), np.asarray(f_desc, np.uint8)
    owner = np.full(nf, -1, np.int32)
    fv_kf, fv_f = feature_vector(kf_node), feature_vector(f_node)
    ratio = F32(nnratio)
    for node in sorted(set(fv_kf) & set(fv_f)):
        rows = [i for i in fv_kf[node] if kf_valid[i]]
        cols = np.array(fv_f[node], np.int64)
        if not rows:
            continue
        D = POP8[np.bitwise_xor(kf_desc[rows][:, None, :], f_desc[cols][None, :, :])].sum(-1, dtype=np.int64)
        for r, k in enumerate(rows):
            free = owner[cols] < 0
            top = {}
            for side, sel in (("l", free & (cols < f_nleft)), ("r", free & (cols >= f_nleft))):
                pairs = sorted(zip(D[r][sel].tolist(), cols[sel].tolist()))[:2]
                top[side] = (pairs[0][0] if pairs else 256, pairs[0][1] if pairs else -1, pairs[1][0] if len(pairs) > 1 else 256)
            if top["l"][0] > TH_LOW:
                continue
            if F32(top["l"][0]) < F32(ratio * F32(top["l"][2])):
                owner[top["l"][1]] = k
            if top["r"][0] <= TH_LOW:
                owner[top["r"][1]] = k
    matches = owner.copy()
    if check_orientation:
        bins = np.array([rot_bin(kf_angle[matches[i]], f_angle[i]) if matches[i] >= 0 else -1 for i in range(nf)], np.int64)
        keep = three_maxima([int((bins == i).sum()) for i in range(HISTO_LENGTH)])
        matches[(bins >= 0) & ~np.isin(bins, [k for k in keep if k >= 0])] = -1
    return matches, int((matches >= 0).sum())


# ---- the corpus ----------------------------------------------------------------------------------------------------------------

NF, F_NLEFT, NNODES = 300, 170, 20


def make_frame(rng, nf=NF, nleft=F_NLEFT, nnodes=NNODES):
    """A frame of two cameras: the right camera's features are copies of left ones a few bits away (the rig sees the scene twice),
    in the same node mostly.  Node 0 lists more than 64 features of each camera."""
    nright = nf - nleft
    ld = rng.integers(0, 256, (nleft, 32), dtype=np.uint8)
    ln = rng.integers(1, nnodes, nleft).astype(np.int32)
    ln[:70] = 0
    ln[rng.random(nleft) < 0.04] = -1
    for i in range(6, nleft, 9):                                     # exact duplicates: ties on the left
        ld[i] = ld[i - 1]; ln[i] = ln[i - 1]
    src = np.concatenate([rng.permutation(70)[:66], rng.integers(70, nleft, nright - 66)])
    rd = ld[src].copy()
    for i in range(nright):
        for bit in rng.integers(0, 256, int(rng.integers(0, 7))):
            rd[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    rn = np.where(rng.random(nright) < 0.9, ln[src], rng.integers(-1, nnodes, nright)).astype(np.int32)
    rn[:66] = 0
    for i in range(4, nright, 7):                                    # ties on the right
        rd[i] = rd[i - 1]; rn[i] = rn[i - 1]
    order = rng.permutation(nright)
    fd, fn = np.concatenate([ld, rd[order]]), np.concatenate([ln, rn[order]])
    fa = rng.uniform(0, 360, nf).astype(np.float32)
    fa[nleft:] = np.mod(fa[src][order] + rng.normal(0, 3, nright), 360.0).astype(np.float32)     # the right copy: nearly the same angle
    fa[fa >= 360.0] = 0.0
    return fd, fa, fn


_CORPUS = {}


def corpus(nkf):
    """-> (frame (desc, angle, node), [keyframe (desc, angle, node, valid)] * nkf): keyframes of ~260 features that see the frame's
    scene (more than 64 take part; several per node, so that a frame feature is matched by an earlier keyframe feature)."""
    if nkf not in _CORPUS:
        rng = np.random.default_rng(300 + nkf)
        frame = make_frame(rng)
        _CORPUS[nkf] = (frame, [keyframe_of(rng, frame, 260 + 11 * k, nnodes=NNODES) for k in range(nkf)])
    return _CORPUS[nkf]


SETTINGS = [(0.7, True), (0.7, False), (0.9, True)]


def test_scalar_and_closed_form_agree_on_the_corpus_and_every_exit_is_taken():
    exits = Counter()
    frame, kfs = corpus(4)
    fv = feature_vector(frame[2])
    assert sum(i < F_NLEFT for i in fv[0]) > 64 and sum(i >= F_NLEFT for i in fv[0]) > 64
    total = 0
    for kf in kfs:
        assert int(((kf[2] >= 0) & (kf[3] != 0) & np.isin(kf[2], list(fv))).sum()) > 64
        for ratio, ori in SETTINGS:
            a = search_scalar(*kf, *frame, F_NLEFT, ratio, ori, exits)
            b = search_closed(*kf, *frame, F_NLEFT, ratio, ori)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] == int((a[0] >= 0).sum())
            total += a[1]
    print(total, dict(exits))
    for name in EXITS:
        assert exits[name] > 0, (name, dict(exits))


def test_with_every_feature_on_the_left_the_result_is_the_one_camera_search_and_with_none_nothing_is_matched():
    frame, kfs = corpus(4)
    for kf in kfs:
        for ratio, ori in SETTINGS:
            a = search_scalar(*kf, *frame, NF, ratio, ori)
            b = search_by_bow(*kf, *frame, nnratio=ratio, check_orientation=ori)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1] > 0
            m, n = search_scalar(*kf, *frame, 0, ratio, ori)
            assert n == 0 and (m == -1).all()


# ---- known answers -------------------------------------------------------------------------------------------------------------

Z = np.zeros(32, np.uint8)


def run(kf, f, nleft, nnratio=0.7, check_orientation=False, exits=None):
    """kf / f: lists of (desc, angle, node[, valid]) per feature."""
    kd = np.array([x[0] for x in kf], np.uint8).reshape(-1, 32)
    ka = np.array([x[1] for x in kf], np.float32)
    kn = np.array([x[2] for x in kf], np.int32)
    kv = np.array([x[3] if len(x) > 3 else 1 for x in kf], np.uint8)
    fd = np.array([x[0] for x in f], np.uint8).reshape(-1, 32)
    fa = np.array([x[1] for x in f], np.float32)
    fn = np.array([x[2] for x in f], np.int32)
    m, n = search_scalar(kd, ka, kn, kv, fd, fa, fn, nleft, nnratio, check_orientation, exits)
    m2, n2 = search_closed(kd, ka, kn, kv, fd, fa, fn, nleft, nnratio, check_orientation)
    assert np.array_equal(m, m2) and n == n2
    return m.tolist(), n


def test_known_answer_a_right_candidate_without_a_left_one_within_th_low_stays_unmatched():
    # the right candidate is the keyframe feature's own descriptor; the only left candidate is 51 bits away
    assert run([(Z, 0, 7)], [(desc_with_bits(51), 0, 7), (Z, 0, 7)], nleft=1) == ([-1, -1], 0)
    assert run([(Z, 0, 7)], [(Z, 0, 7)], nleft=0) == ([-1], 0)                      # no left candidate at all
    assert run([(Z, 0, 7)], [(desc_with_bits(50), 0, 7), (Z, 0, 7)], nleft=1) == ([0, 0], 2)


def test_known_answer_a_right_match_is_taken_where_the_left_failed_its_ratio_test():
    # left: 30 and 40, 30 < 0.7 * 40 = 28 fails; right: 10
    f = [(desc_with_bits(30), 0, 3), (desc_with_bits(40, offset=60), 0, 3), (desc_with_bits(10, offset=120), 0, 3)]
    ex = Counter()
    assert run([(Z, 0, 3)], f, nleft=2, exits=ex) == ([-1, -1, 0], 1) and ex["right_taken_after_left_failed"] == 1


def test_known_answer_a_right_match_is_taken_without_a_ratio_test():
    # right: two candidates at distance 10 (bestDist1R == bestDist2R): the first listed is taken; left: a clean match
    f = [(desc_with_bits(5), 0, 3), (desc_with_bits(10, offset=60), 0, 3), (desc_with_bits(10, offset=120), 0, 3)]
    ex = Counter()
    assert run([(Z, 0, 3)], f, nleft=1, exits=ex) == ([0, 0, -1], 2) and ex["right_taken_with_equal_second"] == 1
    # a second keyframe feature of the node finds both taken and takes the remaining right one only if it has a left candidate
    assert run([(Z, 0, 3), (Z, 0, 3)], f, nleft=1) == ([0, 0, -1], 2)
    # left candidates 5 and 20: the first keyframe feature takes the 5 and the first right one, the second the 20 and the other
    f4 = f + [(desc_with_bits(20, offset=200), 0, 3)]
    assert run([(Z, 0, 3), (Z, 0, 3)], [f4[0], f4[3], f4[1], f4[2]], nleft=2) == ([0, 1, 0, 1], 4)


def test_known_answer_the_rotation_filter_removes_matches_of_both_cameras():
    # eleven keyframe features turned by 0 degrees against their left and right copies (22 matches in bin 0), one turned by 90
    # (bin 3, one match on each side): 2 < 0.1f * 22 drops bin 3; the count goes down by one left and one right match
    kf, left, right = [], [], []
    for i in range(12):
        d = desc_with_bits(3, offset=(i * 17) % 250)
        kf.append((d, 90.0 if i == 11 else 0.0, 100 + i))
        left.append((d, 0.0, 100 + i))
        right.append((d, 0.0, 100 + i))
    ex = Counter()
    m, n = run(kf, left + right, nleft=12, check_orientation=True, exits=ex)
    assert n == 22 and m == list(range(11)) + [-1] + list(range(11)) + [-1]
    assert ex["filtered_left"] == 1 and ex["filtered_right"] == 1
    assert run(kf, left + right, nleft=12, check_orientation=False)[1] == 24


@pytest.mark.parametrize("switch", ["right_independent", "right_ratio", "right_after_left", "one_top2"])
def test_the_corpus_tells_a_wrong_reading_apart(switch):
    frame, kfs = corpus(4)
    changed = 0
    for kf in kfs:
        a = search_scalar(*kf, *frame, F_NLEFT, 0.7, True)
        b = search_scalar(*kf, *frame, F_NLEFT, 0.7, True, rules=replace(REF, **{switch: True}))
        changed += int((a[0] != b[0]).sum())
    print(switch, changed)
    assert changed > 0


def test_the_binding_declares_the_entry_point():
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert re.search(r"pli_status\s+pli_search_by_bow_two_cameras\s*\(", hdr)
    assert "pli_search_by_bow_two_cameras" in capi._PROTOS and len(capi._PROTOS["pli_search_by_bow_two_cameras"][1]) == 16
    assert hasattr(Frontend, "search_by_bow_two_cameras")
