"""ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:269-470, F.Nleft == -1 branch) and
ComputeThreeMaxima (:2449-2490), restated in Python: the checker of pli_search_by_bow (tests/test_bow_search_gpu.py,
tests/test_cpp_bow_search.py).  Here, without a device: hand-worked known answers for the restatement, the restatement
against a second, vectorised one, and a syntax check of the SearchByBoW adapters against stub KeyFrame / Frame types.

The FeatureVector is built as DBoW2's transform() builds it: {node: [i for i in feature order if weight > 0]}; a feature with
node -1 stands for one whose word is stopped (weight 0).
"""
import bisect
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH_LOW, HISTO_LENGTH = 50, 30
F32 = np.float32
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def feature_vector(node):
    fv = {}
    for i, n in enumerate(np.asarray(node).tolist()):
        if n >= 0:
            fv.setdefault(int(n), []).append(i)
    return fv


def distance(a, b):
    return int(POP8[np.bitwise_xor(a, b)].sum())


def rot_bin(angle_kf, angle_f, trunc=False):
    """rot = kp.angle - Fkp.angle (+360 if negative), bin = round(rot * (1.0f / 30)), 30 -> 0 (float arithmetic); trunc: the
    misreading `int bin = rot * factor`."""
    rot = F32(F32(angle_kf) - F32(angle_f))
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    x = F32(rot * F32(F32(1.0) / F32(HISTO_LENGTH)))
    b = int(np.floor(np.float64(x) + (0.0 if trunc else 0.5)))          # round(): half away from zero; x >= 0
    return 0 if b == HISTO_LENGTH else b


def three_maxima(counts, tenth_of_second=False):
    """tenth_of_second: the misreading that tests the third bin against a tenth of the SECOND."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    tenth = F32(F32(0.1) * F32(max1))
    if F32(max2) < tenth:
        ind2 = ind3 = -1
    elif F32(max3) < (F32(F32(0.1) * F32(max2)) if tenth_of_second else tenth):
        ind3 = -1
    return ind1, ind2, ind3


def search_by_bow(kf_desc, kf_angle, kf_node, kf_valid, f_desc, f_angle, f_node, nnratio=0.75, check_orientation=True, misread=()):
    """The reference's control flow, scalar: returns (matches[nf] = keyframe feature or -1, nmatches).  misread: deliberate
    misreadings that tests/test_ref_pin_match.py wants rejected ("min_le": <= in the running minimum; "ratio_double": the ratio
    test in double; "rot_trunc": the rotation bin by truncation; "th_low_strict": bestDist1 < TH_LOW; "tenth_of_second": the 0.1
    rule of ComputeThreeMaxima's third bin applied to the second maximum)."""
    nf = len(f_node)
    matches = [-1] * nf
    fv_kf, fv_f = feature_vector(kf_node), feature_vector(f_node)
    kf_keys, f_keys = sorted(fv_kf), sorted(fv_f)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    ratio = F32(nnratio)
    nmatches = 0
    a, b = 0, 0
    while a < len(kf_keys) and b < len(f_keys):
        if kf_keys[a] == f_keys[b]:
            idx_f = fv_f[f_keys[b]]
            for ikf in fv_kf[kf_keys[a]]:
                if not kf_valid[ikf]:
                    continue
                best1, best_idx, best2 = 256, -1, 256
                for i_f in idx_f:
                    if matches[i_f] >= 0:
                        continue
                    d = distance(kf_desc[ikf], f_desc[i_f])
                    if d < best1 or ("min_le" in misread and d == best1):
                        best2, best1, best_idx = best1, d, i_f
                    elif d < best2:
                        best2 = d
                passes = (float(best1) < float(ratio) * float(best2)) if "ratio_double" in misread else F32(best1) < F32(ratio * F32(best2))
                if best1 <= TH_LOW - ("th_low_strict" in misread) and passes:
                    matches[best_idx] = ikf
                    if check_orientation:
                        rot_hist[rot_bin(kf_angle[ikf], f_angle[best_idx], "rot_trunc" in misread)].append(best_idx)
                    nmatches += 1
            a += 1
            b += 1
        elif kf_keys[a] < f_keys[b]:
            a = bisect.bisect_left(kf_keys, f_keys[b], a)
        else:
            b = bisect.bisect_left(f_keys, kf_keys[a], b)
    if check_orientation:
        keep = three_maxima([len(h) for h in rot_hist], "tenth_of_second" in misread)
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for i_f in rot_hist[i]:
                matches[i_f] = -1
                nmatches -= 1
    return np.array(matches, np.int32), nmatches


def search_by_bow_fast(kf_desc, kf_angle, kf_node, kf_valid, f_desc, f_angle, f_node, nnratio=0.75, check_orientation=True):
    """The same result with numpy per node (for the large GPU cases): the running best / second best of the scan is the first
    minimum and the second smallest distance of the free candidates."""
    nf = len(f_node)
    kf_desc, f_desc = np.asarray(kf_desc, np.uint8), np.asarray(f_desc, np.uint8)
    matches = np.full(nf, -1, np.int32)
    fv_kf, fv_f = feature_vector(kf_node), feature_vector(f_node)
    ratio = F32(nnratio)
    hist = [[] for _ in range(HISTO_LENGTH)]
    for node in sorted(set(fv_kf) & set(fv_f)):
        ikf = np.array([i for i in fv_kf[node] if kf_valid[i]], np.int64)
        if len(ikf) == 0:
            continue
        i_f = np.array(fv_f[node], np.int64)
        D = POP8[np.bitwise_xor(kf_desc[ikf][:, None, :], f_desc[i_f][None, :, :])].sum(-1, dtype=np.int32)
        free = np.ones(len(i_f), bool)
        for r, k in enumerate(ikf):
            d = np.where(free, D[r], 1 << 20)
            if not free.any():
                continue
            p = int(np.argmin(d))
            best1 = int(d[p])
            best2 = int(np.partition(d, 1)[1]) if len(d) > 1 else 256
            best2 = min(best2, 256)
            if best1 <= TH_LOW and F32(best1) < F32(ratio * F32(best2)):
                free[p] = False
                matches[i_f[p]] = k
                if check_orientation:
                    hist[rot_bin(kf_angle[k], f_angle[i_f[p]])].append(int(i_f[p]))
    nmatches = int((matches >= 0).sum())
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i not in keep:
                matches[hist[i]] = -1
                nmatches -= len(hist[i])
    return matches, nmatches


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------

def desc_with_bits(nbits, base=None, offset=0):
    """A descriptor that differs from `base` (zeros by default) in nbits bits, starting at bit `offset`."""
    d = np.zeros(32, np.uint8) if base is None else base.copy()
    for b in range(offset, offset + nbits):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def run(kf, f, nnratio=0.75, check_orientation=False):
    """kf / f: lists of (desc, angle, node[, valid]) per feature."""
    kd = np.array([x[0] for x in kf], np.uint8).reshape(-1, 32)
    ka = np.array([x[1] for x in kf], np.float32)
    kn = np.array([x[2] for x in kf], np.int32)
    kv = np.array([x[3] if len(x) > 3 else 1 for x in kf], np.uint8)
    fd = np.array([x[0] for x in f], np.uint8).reshape(-1, 32)
    fa = np.array([x[1] for x in f], np.float32)
    fn = np.array([x[2] for x in f], np.int32)
    m, n = search_by_bow(kd, ka, kn, kv, fd, fa, fn, nnratio, check_orientation)
    m2, n2 = search_by_bow_fast(kd, ka, kn, kv, fd, fa, fn, nnratio, check_orientation)
    assert np.array_equal(m, m2) and n == n2
    return m.tolist(), n


Z = np.zeros(32, np.uint8)


def test_ties_keep_the_first_listed_frame_feature():
    # two frame features at distance 10 in node 7: the first one listed wins; the second best equals the best -> 10 < 0.75 * 10 fails
    m, n = run([(Z, 0, 7)], [(desc_with_bits(10), 0, 7), (desc_with_bits(10, offset=100), 0, 7)])
    assert (m, n) == ([-1, -1], 0)
    # with ratio > 1 the tie passes and the FIRST listed frame feature takes the match
    m, n = run([(Z, 0, 7)], [(desc_with_bits(10), 0, 7), (desc_with_bits(10, offset=100), 0, 7)], nnratio=1.5)
    assert (m, n) == ([0, -1], 1)


def test_second_best_equal_to_best_and_single_candidate():
    # best 20, then another 20 (strict <: goes to bestDist2), then 5 -> best 5, second 20: 5 < 15 accepted, index 2
    f = [(desc_with_bits(20), 0, 1), (desc_with_bits(20, offset=40), 0, 1), (desc_with_bits(5, offset=200), 0, 1)]
    assert run([(Z, 0, 1)], f) == ([-1, -1, 0], 1)
    # a single candidate: bestDist2 stays 256
    assert run([(Z, 0, 1)], [(desc_with_bits(50), 0, 1)]) == ([0], 1)
    assert run([(Z, 0, 1)], [(desc_with_bits(51), 0, 1)]) == ([-1], 0)      # TH_LOW = 50


def test_ratio_exactly_at_the_float_boundary():
    # 30 < 0.75 * 40 = 30.0 is false; 30 < 0.75 * 41 = 30.75 is true
    for d2, want in ((40, 0), (41, 1)):
        f = [(desc_with_bits(30), 0, 3), (desc_with_bits(d2, offset=60), 0, 3)]
        assert run([(Z, 0, 3)], f)[1] == want
    # 0.6f * 25 rounds to 15.000001f: 15 < that is TRUE (in exact decimal 0.6 * 25 = 15 would reject); 0.7f * 50 is 35.0f
    assert F32(F32(0.6) * F32(25)) > F32(15) and F32(F32(0.7) * F32(50)) == F32(35)
    f = [(desc_with_bits(15), 0, 3), (desc_with_bits(25, offset=100), 0, 3)]
    assert run([(Z, 0, 3)], f, nnratio=0.6) == ([0, -1], 1)
    f = [(desc_with_bits(35), 0, 3), (desc_with_bits(50, offset=100), 0, 3)]
    assert run([(Z, 0, 3)], f, nnratio=0.7) == ([-1, -1], 0)


def test_a_frame_feature_claimed_earlier_in_the_same_node():
    # keyframe features 0 and 1 both nearest to frame feature 0; kf 0 takes it, kf 1 then gets frame feature 1
    f = [(desc_with_bits(2), 0, 4), (desc_with_bits(20, offset=64), 0, 4), (desc_with_bits(60, offset=128), 0, 4)]
    kf = [(Z, 0, 4), (desc_with_bits(1), 0, 4)]
    assert run(kf, f) == ([0, 1, -1], 2)


def test_invalid_map_points_no_common_node_and_stopped_words():
    f = [(desc_with_bits(2), 0, 4), (desc_with_bits(2, offset=8), 0, 9)]
    assert run([(Z, 0, 4, 0)], f) == ([-1, -1], 0)                       # map point NULL / bad
    assert run([(Z, 0, 5)], f) == ([-1, -1], 0)                          # no common node
    assert run([(Z, 0, -1)], [(Z, 0, -1)]) == ([-1], 0)                  # stopped words are listed nowhere
    assert run([(Z, 0, 9), (Z, 0, 4, 0)], f) == ([-1, 0], 1)             # the valid one in node 9 matches
    assert run([], f) == ([-1, -1], 0) and run([(Z, 0, 4)], []) == ([], 0)


def test_rotation_bins_at_half_steps_and_near_360():
    assert rot_bin(45.0, 0.0) == 2                # 1.5 -> 2 (half away from zero)
    assert rot_bin(15.0, 0.0) == 1                # 0.5 -> 1
    assert rot_bin(75.0, 0.0) == 3                # 2.5 -> 3 (not ties-to-even)
    assert rot_bin(0.0, 15.0) == 12               # -15 + 360 = 345 -> 11.5 -> 12
    assert rot_bin(359.99, 0.0) == 12             # rot / 30 < 12.0: bin 12, never 30
    assert rot_bin(0.0, 1e-5) == 12               # -1e-5 + 360 rounds to 360.0f -> 12
    assert rot_bin(10.0, 10.0) == 0
    assert max(rot_bin(a, b) for a in np.linspace(0, 359.9, 60) for b in np.linspace(0, 359.9, 60)) == 12


def test_three_maxima_branches():
    h = [0] * 30
    assert three_maxima(h) == (-1, -1, -1)
    h[3] = 10
    assert three_maxima(h) == (3, -1, -1)
    h[5], h[7] = 1, 1                      # 1 is 0.1 * 10 -> kept (1 < 1.0 false)
    assert three_maxima(h) == (3, 5, 7)
    h[5], h[7] = 1, 0
    assert three_maxima(h) == (3, 5, -1)
    h[3], h[5], h[7] = 20, 2, 1            # 1 < 2.0: third dropped
    assert three_maxima(h) == (3, 5, -1)
    h[3], h[5], h[7] = 21, 2, 2            # 2 < 2.1: second and third dropped
    assert three_maxima(h) == (3, -1, -1)
    h = [0] * 30
    h[1], h[2], h[3], h[4] = 4, 4, 5, 4    # ties: strict >, the first bins keep their places
    assert three_maxima(h) == (3, 1, 2)


def test_orientation_filter_clears_the_bins_not_kept():
    # rotations 0 (x10, bin 0), 60 (bin 2), 90 (bin 3), 120 (bin 4): 1 < 0.1f * 10 is false, so bins 0, 2, 3 stay and bin 4 goes;
    # with one more match in bin 0 (11), 1 < 1.1 drops bins 2 and 3 as well
    for n0, want in ((10, 12), (11, 11)):
        kf, f = [], []
        for i in range(n0 + 3):
            d = desc_with_bits(3, offset=(i * 17) % 250)
            ang = 0.0 if i < n0 else (60.0, 90.0, 120.0)[i - n0]
            kf.append((d, ang, 100 + i))
            f.append((d, 0.0, 100 + i))
        m, n = run(kf, f, check_orientation=True)
        assert n == want and m[:want] == list(range(want)) and m[want:] == [-1] * (n0 + 3 - want)
        assert run(kf, f, check_orientation=False)[1] == n0 + 3


def random_case(rng, nkf, nf, nnodes, ndup=0.3, invalid=0.2):
    base = rng.integers(0, 256, (max(4, nf // 3), 32), dtype=np.uint8)
    def feats(n):
        d = base[rng.integers(0, len(base), n)].copy()
        flips = rng.integers(0, 256, (n, rng.integers(1, 40)))
        for i in range(n):
            if rng.random() > ndup:
                for b in flips[i]:
                    d[i, b >> 3] ^= np.uint8(1 << (b & 7))
        node = rng.integers(-1, nnodes, n).astype(np.int32)
        ang = rng.uniform(0, 360, n).astype(np.float32)
        return d, ang, node
    kd, ka, kn = feats(nkf)
    kv = (rng.random(nkf) >= invalid).astype(np.uint8)
    fd, fa, fn = feats(nf)
    return kd, ka, kn, kv, fd, fa, fn


def keyframe_of(rng, frame, n, invalid=0.2, nnodes=None):
    """A keyframe that sees the frame's scene: n features copied from random frame features with 0-12 bits flipped, mostly in the
    same node (else a random one, or none), angles near the frame feature's (a rotation of the whole view) or random."""
    fd, fa, fn = frame
    src = rng.integers(0, max(1, len(fn)), n)
    kd = np.asarray(fd, np.uint8)[src].copy() if len(fn) else rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for i in range(n):
        for b in rng.integers(0, 256, int(rng.integers(0, 13))):
            kd[i, b >> 3] ^= np.uint8(1 << (b & 7))
    top = int(nnodes if nnodes is not None else (fn.max() + 1 if len(fn) and fn.max() >= 0 else 1))
    kn = np.where(rng.random(n) < 0.8, np.asarray(fn)[src] if len(fn) else -1, rng.integers(-1, top, n)).astype(np.int32)
    turn = float(rng.uniform(0, 360))
    ka = np.where(rng.random(n) < 0.7, (np.asarray(fa, np.float64)[src] if len(fn) else 0) + turn + rng.normal(0, 8, n),
                  rng.uniform(0, 360, n))
    ka = np.mod(ka, 360.0).astype(np.float32)
    ka[ka >= 360.0] = 0.0
    kv = (rng.random(n) >= invalid).astype(np.uint8)
    return kd, ka, kn, kv


def test_scalar_and_vectorised_restatements_agree():
    rng = np.random.default_rng(5)
    for it in range(60):
        case = random_case(rng, int(rng.integers(0, 120)), int(rng.integers(0, 120)), int(rng.choice([1, 3, 10, 40])))
        for ratio, ori in ((0.75, True), (0.7, False), (0.9, True)):
            m1, n1 = search_by_bow(*case, nnratio=ratio, check_orientation=ori)
            m2, n2 = search_by_bow_fast(*case, nnratio=ratio, check_orientation=ori)
            assert np.array_equal(m1, m2) and n1 == n2, (it, ratio, ori)
            assert n1 == int((m1 >= 0).sum())


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
  int N; cv::Mat mDescriptors; std::vector<cv::KeyPoint> mvKeysUn; FeatureVector mFeatVec; StubCamera* mpCamera2;
  std::vector<StubMapPoint*> GetMapPointMatches();
};
struct StubFrame {
  cv::Mat mTcw, mDescriptors; float mb, mbf, fx, fy, cx, cy, mnMinX, mnMaxX, mnMinY, mnMaxY; int N, Nleft;
  std::vector<StubMapPoint*> mvpMapPoints; std::vector<bool> mvbOutlier; std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  std::vector<float> mvScaleFactors, mvuRight; FeatureVector mFeatVec;
};
int use(StubKeyFrame* kf, std::vector<StubKeyFrame*>& kfs, StubFrame& F) {
  typedef ORB_SLAM3::PliORBmatcher<StubFrame, StubMapPoint> ORBmatcher;
  ORBmatcher matcher(0.75f, true);
  std::vector<StubMapPoint*> vpMapPointMatches;
  std::vector<std::vector<StubMapPoint*>> vvpMapPointMatches;
  std::vector<int> vn;
  int n = matcher.SearchByBoW(kf, F, vpMapPointMatches);
  matcher.SearchByBoW(kfs, F, vvpMapPointMatches, vn);
  return n + (int)vn.size();
}
'''


def test_search_by_bow_adapters_are_valid_cpp_against_stub_types():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "a.cpp")
        open(src, "w").write(STUB_SRC)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]


def test_the_header_declares_search_by_bow_with_its_cap():
    src = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    assert "pli_status pli_search_by_bow(" in src and "#define PLI_BOW_MAX_FEATURES 8192" in src
    from pli_slam_amd import capi
    assert "pli_search_by_bow" in capi._PROTOS
