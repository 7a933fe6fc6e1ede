"""ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (ORBmatcher.cc:823-963, NLeft == -1 on both sides),
restated in Python: the checker of pli_search_by_bow_kf (tests/test_bow_kf_search_gpu.py, tests/test_cpp_bow_kf_search.py).
Here, without a device: hand-worked known answers for the restatement, the restatement against a second, vectorised one, a syntax
check of the SearchByBoW(KF, KF) adapters against stub KeyFrame types, and the case generator of the GPU tests.

Against SearchByBoW(KF, Frame) (tests/test_bow_search_cpu.py): pKF1 is walked and pKF2's features are taken away (vbMatched2), both
sides carry the map-point gate, the distance test is strict (bestDist1 < TH_LOW) and the result is indexed by pKF1's feature.
"""
import bisect
import os
import subprocess
import tempfile

import numpy as np

from test_bow_search_cpu import (F32, HISTO_LENGTH, POP8, TH_LOW, desc_with_bits, distance, feature_vector, keyframe_of,
                                 random_case, rot_bin, three_maxima)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def search_by_bow_kf(desc1, angle1, node1, valid1, desc2, angle2, node2, valid2, nnratio=0.75, check_orientation=True, misread=()):
    """The reference's control flow, scalar: returns (matches12[n1] = pKF2's feature or -1, nmatches).  misread: deliberate
    misreadings that tests/test_ref_pin_match.py wants rejected ("min_le": <= in the running minimum; "ratio_double": the ratio
    test in double; "rot_trunc": the rotation bin by truncation; "th_low_inclusive": bestDist1 <= TH_LOW, as the (KF, Frame) form
    has it)."""
    matches12 = [-1] * len(node1)
    matched2 = [False] * len(node2)
    fv1, fv2 = feature_vector(node1), feature_vector(node2)
    keys1, keys2 = sorted(fv1), sorted(fv2)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    ratio = F32(nnratio)
    nmatches = 0
    a, b = 0, 0
    while a < len(keys1) and b < len(keys2):
        if keys1[a] == keys2[b]:
            for idx1 in fv1[keys1[a]]:
                if not valid1[idx1]:
                    continue
                best1, best_idx2, best2 = 256, -1, 256
                for idx2 in fv2[keys2[b]]:
                    if matched2[idx2] or not valid2[idx2]:
                        continue
                    d = distance(desc1[idx1], desc2[idx2])
                    if d < best1 or ("min_le" in misread and d == best1):
                        best2, best1, best_idx2 = best1, d, idx2
                    elif d < best2:
                        best2 = d
                passes = (float(best1) < float(ratio) * float(best2)) if "ratio_double" in misread else F32(best1) < F32(ratio * F32(best2))
                if best1 < TH_LOW + ("th_low_inclusive" in misread) and passes:
                    matches12[idx1] = best_idx2
                    matched2[best_idx2] = True
                    if check_orientation:
                        rot_hist[rot_bin(angle1[idx1], angle2[best_idx2], "rot_trunc" in misread)].append(idx1)
                    nmatches += 1
            a += 1
            b += 1
        elif keys1[a] < keys2[b]:
            a = bisect.bisect_left(keys1, keys2[b], a)
        else:
            b = bisect.bisect_left(keys2, keys1[a], b)
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in rot_hist[i]:
                matches12[idx1] = -1
                nmatches -= 1
    return np.array(matches12, np.int32), nmatches


def search_by_bow_kf_fast(desc1, angle1, node1, valid1, desc2, angle2, node2, valid2, nnratio=0.75, check_orientation=True):
    """The same result with numpy per node (for the large GPU cases): the running best / second best of the scan is the first
    minimum and the second smallest distance of the candidates that are valid and not yet taken."""
    desc1, desc2 = np.asarray(desc1, np.uint8).reshape(-1, 32), np.asarray(desc2, np.uint8).reshape(-1, 32)
    matches12 = np.full(len(node1), -1, np.int32)
    fv1, fv2 = feature_vector(node1), feature_vector(node2)
    ratio = F32(nnratio)
    hist = [[] for _ in range(HISTO_LENGTH)]
    for node in sorted(set(fv1) & set(fv2)):
        i1 = np.array([i for i in fv1[node] if valid1[i]], np.int64)
        i2 = np.array([i for i in fv2[node] if valid2[i]], np.int64)
        if len(i1) == 0 or len(i2) == 0:
            continue
        D = POP8[np.bitwise_xor(desc1[i1][:, None, :], desc2[i2][None, :, :])].sum(-1, dtype=np.int32)
        free = np.ones(len(i2), bool)
        for r, idx1 in enumerate(i1):
            if not free.any():
                break
            d = np.where(free, D[r], 1 << 20)
            p = int(np.argmin(d))
            best1 = int(d[p])
            best2 = min(int(np.partition(d, 1)[1]), 256) if len(d) > 1 else 256
            if best1 < TH_LOW and F32(best1) < F32(ratio * F32(best2)):
                free[p] = False
                matches12[idx1] = i2[p]
                if check_orientation:
                    hist[rot_bin(angle1[idx1], angle2[i2[p]])].append(int(idx1))
    nmatches = int((matches12 >= 0).sum())
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i not in keep:
                matches12[hist[i]] = -1
                nmatches -= len(hist[i])
    return matches12, nmatches


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------

def table(rows):
    """rows: list of (desc, angle, node[, valid]) per feature -> (desc, angle, node, valid) arrays."""
    return (np.array([x[0] for x in rows], np.uint8).reshape(-1, 32), np.array([x[1] for x in rows], np.float32),
            np.array([x[2] for x in rows], np.int32), np.array([x[3] if len(x) > 3 else 1 for x in rows], np.uint8))


def run(kf1, kf2, nnratio=0.75, check_orientation=False):
    t1, t2 = table(kf1), table(kf2)
    m, n = search_by_bow_kf(*t1, *t2, nnratio, check_orientation)
    m2, n2 = search_by_bow_kf_fast(*t1, *t2, nnratio, check_orientation)
    assert np.array_equal(m, m2) and n == n2
    return m.tolist(), n


Z = np.zeros(32, np.uint8)


def test_a_distance_of_exactly_50_is_rejected_and_49_accepted():
    # a single candidate: bestDist2 stays 256, so only bestDist1 < TH_LOW decides (the KF-against-Frame form accepts 50)
    assert run([(Z, 0, 1)], [(desc_with_bits(49), 0, 1)]) == ([0], 1)
    assert run([(Z, 0, 1)], [(desc_with_bits(50), 0, 1)]) == ([-1], 0)
    assert run([(Z, 0, 1)], [(desc_with_bits(51), 0, 1)]) == ([-1], 0)


def test_a_single_candidate_passes_the_ratio_test_against_256():
    # 40 < 0.1 * 256 = 25.6 fails, 40 < 0.2 * 256 = 51.2 passes: the second best of one candidate is 256
    assert run([(Z, 0, 3)], [(desc_with_bits(40), 0, 3)], nnratio=0.1) == ([-1], 0)
    assert run([(Z, 0, 3)], [(desc_with_bits(40), 0, 3)], nnratio=0.2) == ([0], 1)


def test_two_equal_minima_are_rejected_for_a_ratio_up_to_one_and_a_tie_keeps_the_lowest_idx2():
    kf2 = [(desc_with_bits(60, offset=150), 0, 7), (desc_with_bits(10), 0, 7), (desc_with_bits(10, offset=100), 0, 7)]
    for ratio in (0.75, 1.0):                             # bestDist2 == bestDist1 == 10: 10 < ratio * 10 is false
        assert run([(Z, 0, 7)], kf2, nnratio=ratio) == ([-1], 0)
    assert run([(Z, 0, 7)], kf2, nnratio=1.5) == ([1], 1)        # strict <: the first listed of the two, idx2 = 1
    # 20, 20, then 5: best 5, second 20 -> 5 < 15, index 2
    kf2 = [(desc_with_bits(20), 0, 1), (desc_with_bits(20, offset=40), 0, 1), (desc_with_bits(5, offset=200), 0, 1)]
    assert run([(Z, 0, 1)], kf2) == ([2], 1)


def test_a_feature_of_kf2_taken_by_a_lower_idx1_is_unavailable_to_a_higher_one():
    # both features of pKF1 are nearest to idx2 = 0; idx1 = 0 takes it, idx1 = 1 then takes its second choice idx2 = 1
    kf2 = [(desc_with_bits(2), 0, 4), (desc_with_bits(20, offset=64), 0, 4), (desc_with_bits(60, offset=128), 0, 4)]
    kf1 = [(Z, 0, 4), (desc_with_bits(1), 0, 4)]
    assert run(kf1, kf2) == ([0, 1], 2)
    # the order is pKF1's index inside the node, whatever the nodes before it: idx1 = 0 sits in a later node
    kf1 = [(Z, 0, 9), (Z, 0, 4), (desc_with_bits(1), 0, 4)]
    assert run(kf1, kf2) == ([-1, 0, 1], 2)
    # with nothing left but the far one, the third goes without
    kf1 = [(Z, 0, 4), (desc_with_bits(1), 0, 4), (desc_with_bits(3), 0, 4)]
    assert run(kf1, kf2) == ([0, 1, -1], 2)


def test_invalid_on_either_side_is_skipped():
    kf2 = [(desc_with_bits(2), 0, 4), (desc_with_bits(12, offset=64), 0, 4)]
    assert run([(Z, 0, 4, 0)], kf2) == ([-1], 0)                           # pMP1 NULL / bad
    assert run([(Z, 0, 4)], [kf2[0] + (0,), kf2[1]]) == ([1], 1)           # pMP2 NULL / bad: the other one, alone (256)
    assert run([(Z, 0, 4)], [kf2[0] + (0,), kf2[1] + (0,)]) == ([-1], 0)
    assert run([(Z, 0, 4, 0), (Z, 0, 4)], kf2) == ([-1, 0], 1)             # an invalid idx1 takes nothing away
    assert run([], kf2) == ([], 0) and run([(Z, 0, 4)], []) == ([-1], 0)


def test_a_feature_with_node_minus_one_never_matches():
    assert run([(Z, 0, -1)], [(Z, 0, -1)]) == ([-1], 0)
    assert run([(Z, 0, -1), (Z, 0, 5)], [(Z, 0, -1), (desc_with_bits(1), 0, 5)]) == ([-1, 1], 1)
    assert run([(Z, 0, 5)], [(Z, 0, 6)]) == ([-1], 0)                      # no common node


def test_the_rotation_filter_clears_a_minority_bin_and_decrements_nmatches():
    # rotations 0 (x n0, bin 0), 60 (bin 2), 90 (bin 3), 120 (bin 4): with 10 in bin 0, 1 < 0.1f * 10 is false and bins 0, 2, 3
    # stay (the fourth, bin 4, goes); with 11, 1 < 1.1 drops bins 2 and 3 as well
    for n0, want in ((10, 12), (11, 11)):
        kf1, kf2 = [], []
        for i in range(n0 + 3):
            d = desc_with_bits(3, offset=(i * 17) % 250)
            ang = 0.0 if i < n0 else (60.0, 90.0, 120.0)[i - n0]
            kf1.append((d, ang, 100 + i))
            kf2.append((d, 0.0, 100 + i))
        m, n = run(kf1, kf2, check_orientation=True)
        assert n == want and m[:want] == list(range(want)) and m[want:] == [-1] * (n0 + 3 - want)
        assert run(kf1, kf2, check_orientation=False) == (list(range(n0 + 3)), n0 + 3)
    # rot = angle1 - angle2: 0 - 15 -> 345 -> bin 12, against 15 - 0 -> bin 1
    assert rot_bin(0.0, 15.0) == 12 and rot_bin(15.0, 0.0) == 1


def test_the_rotation_filter_does_not_give_a_taken_feature_back():
    # idx1 = 0 takes idx2 = 0 and is then cleared by the rotation filter; idx1 = 1 (same node) still had to take idx2 = 1
    kf1 = [(Z, 90.0, 4), (desc_with_bits(1), 0.0, 4)]
    kf2 = [(desc_with_bits(2), 0.0, 4), (desc_with_bits(20, offset=64), 0.0, 4)]
    for i in range(20):                                   # 21 matches in bin 0 against one in bin 3: 1 < 2.1
        d = desc_with_bits(3, offset=(i * 11) % 250)
        kf1.append((d, 0.0, 50 + i))
        kf2.append((d, 0.0, 50 + i))
    m, n = run(kf1, kf2, check_orientation=True)
    assert m[:2] == [-1, 1] and n == 21


# ---- generators (shared with the GPU tests) -----------------------------------------------------------------------------------

def kf_pair_case(rng, n1, n2, nnodes, ndup=0.3, invalid=0.2):
    """A tie-rich random pair (duplicated descriptors, as test_bow_search_cpu.random_case): (table1, table2)."""
    d1, a1, nd1, v1, d2, a2, nd2 = random_case(rng, n1, n2, nnodes, ndup=ndup, invalid=invalid)
    v2 = (rng.random(n2) >= invalid).astype(np.uint8)
    return (d1, a1, nd1, v1), (d2, a2, nd2, v2)


def batch_of(rng, nkf, n1=400, nnodes=30, max_n2=500):
    """pKF1 and nkf keyframes that see its scene (keyframe_of: copies of pKF1's features with a few bits flipped, mostly in the
    same node).  Every fifth keyframe is empty, every seventh has no valid feature."""
    d1, a1, nd1, v1, _, _, _ = random_case(rng, n1, 1, nnodes, ndup=0.5, invalid=0.2)
    kfs = []
    for k in range(nkf):
        n2 = 0 if k % 5 == 4 else int(rng.integers(1, max_n2))
        kf = keyframe_of(rng, (d1, a1, nd1), n2, invalid=float(rng.uniform(0, 0.4)), nnodes=nnodes)
        if k % 7 == 3:
            kf[3][:] = 0
        kfs.append(kf)
    return (d1, a1, nd1, v1), kfs


def boundary_case():
    """Best distances of exactly 49, 50 and 51 (and 48), each in a node of its own with a far second candidate, repeated."""
    kf1, kf2 = [], []
    for rep in range(6):
        for j, dist in enumerate((49, 50, 51, 48)):
            node = rep * 4 + j
            base = desc_with_bits(7, offset=rep * 9)
            kf1.append((base, 10.0, node))
            kf2.append((desc_with_bits(120, base=base, offset=130), 10.0, node))
            kf2.append((desc_with_bits(dist, base=base, offset=60), 10.0, node))
    return table(kf1), table(kf2)


def test_scalar_and_vectorised_restatements_agree():
    rng = np.random.default_rng(15)
    total = 0
    for it in range(70):
        t1, t2 = kf_pair_case(rng, int(rng.integers(0, 120)), int(rng.integers(0, 120)), int(rng.choice([1, 3, 10, 40])))
        for ratio, ori in ((0.75, True), (0.7, False), (1.2, True)):
            m1, n1 = search_by_bow_kf(*t1, *t2, nnratio=ratio, check_orientation=ori)
            m2, n2 = search_by_bow_kf_fast(*t1, *t2, nnratio=ratio, check_orientation=ori)
            assert np.array_equal(m1, m2) and n1 == n2, (it, ratio, ori)
            assert n1 == int((m1 >= 0).sum())
            taken = m1[m1 >= 0]
            assert len(set(taken.tolist())) == len(taken)                  # a feature of pKF2 is matched once
            assert t1[3][m1 >= 0].all() and t2[3][taken].all()             # by valid features only
            total += n1
    assert total > 0


def test_the_gpu_case_generators_yield_matches():
    rng = np.random.default_rng(21)
    t1, kfs = batch_of(rng, 8, n1=200, nnodes=8)
    total = 0
    for kf in kfs:
        m1, n1 = search_by_bow_kf(*t1, *kf)
        m2, n2 = search_by_bow_kf_fast(*t1, *kf)
        assert np.array_equal(m1, m2) and n1 == n2
        total += n1
    assert total > 0 and len(kfs[4][2]) == 0 and not kfs[3][3].any()
    t1, t2 = boundary_case()
    m, n = search_by_bow_kf(*t1, *t2, 0.75, False)
    assert m.reshape(6, 4).tolist() == [[2 * (4 * r) + 1, -1, -1, 2 * (4 * r + 3) + 1] for r in range(6)] and n == 12
    assert np.array_equal(search_by_bow_kf_fast(*t1, *t2, 0.75, False)[0], m)


STUB_SRC = r'''
#define PLI_ADAPTER_NO_KEYLINE_HEADER
#define PLI_ADAPTER_KEYLINE_TYPE StubKeyLine
#include <opencv2/core/core.hpp>
struct StubKeyLine { float angle; int class_id; int octave; cv::Point2f pt; float response; float size; float startPointX,
  startPointY, endPointX, endPointY, sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY, lineLength; int numOfPixels; };
#include "pli_slam_amd/adapters/orbslam_adapters.hpp"
#include <map>
#include <vector>
// the members SearchByBoW reads (include/KeyFrame.h, Frame.h, MapPoint.h; DBoW2::FeatureVector is a std::map)
typedef std::map<unsigned int, std::vector<unsigned int>> FeatureVector;
struct StubMapPoint { bool isBad(); cv::Mat GetWorldPos(); cv::Mat GetDescriptor(); int Observations(); };
struct StubCamera;
struct StubKeyFrame {
  int N, NLeft; cv::Mat mDescriptors; std::vector<cv::KeyPoint> mvKeysUn; FeatureVector mFeatVec; StubCamera* mpCamera2;
  std::vector<StubMapPoint*> GetMapPointMatches();
};
struct StubFrame {
  cv::Mat mTcw, mDescriptors; float mb, mbf, fx, fy, cx, cy, mnMinX, mnMaxX, mnMinY, mnMaxY; int N, Nleft;
  std::vector<StubMapPoint*> mvpMapPoints; std::vector<bool> mvbOutlier; std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  std::vector<float> mvScaleFactors, mvuRight; FeatureVector mFeatVec;
};
int use(StubKeyFrame* kf1, StubKeyFrame* kf2, std::vector<StubKeyFrame*>& kfs, StubFrame& F) {
  typedef ORB_SLAM3::PliORBmatcher<StubFrame, StubMapPoint> ORBmatcher;
  ORBmatcher matcher(0.75f, true);
  std::vector<StubMapPoint*> vpMatches12, vpMapPointMatches;
  std::vector<std::vector<StubMapPoint*>> vvpMatches12, vvpMapPointMatches;
  std::vector<int> vn, vnF;
  int n = matcher.SearchByBoW(kf1, kf2, vpMatches12);              // loop closing: (KF, KF)
  matcher.SearchByBoW(kf1, kfs, vvpMatches12, vn);                 // its batch form
  n += matcher.SearchByBoW(kf1, F, vpMapPointMatches);             // relocalisation: (KF, Frame) stays unambiguous
  matcher.SearchByBoW(kfs, F, vvpMapPointMatches, vnF);
  return n + (int)vn.size() + (int)vnF.size();
}
'''


def test_search_by_bow_kf_adapters_are_valid_cpp_against_stub_types():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "a.cpp")
        open(src, "w").write(STUB_SRC)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]


def test_the_header_and_the_ctypes_table_declare_search_by_bow_kf():
    src = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert "pli_status pli_search_by_bow_kf(" in src
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    assert "pli_search_by_bow_kf" in capi._PROTOS and hasattr(Frontend, "search_by_bow_kf")
