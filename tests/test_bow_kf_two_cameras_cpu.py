"""ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (ORBmatcher.cc:823-963) for keyframes of two cameras
(NLeft != -1), restated with its two-camera text - the `continue`s at :858-860 and :878-880 for a feature idx >= mvKeysUn.size(),
the angles from mvKeysUn (:915) - and compared with the restatement of tests/test_bow_kf_search_cpu.py fed those rows as valid = 0:
what PliORBmatcherTwoCameras::SearchByBoW(pKF1, pKF2, ...) hands to pli_search_by_bow_kf.  A keyframe here is (desc, angle_un,
node, has_good_point, nleft, nun): N rows of descriptors, nodes and map-point flags, mvKeysUn.size() = nun angles."""
import bisect
import os

import numpy as np
import pytest

from test_bow_search_cpu import HISTO_LENGTH, TH_LOW, distance, feature_vector, keyframe_of, random_case, rot_bin, three_maxima
from test_bow_kf_search_cpu import search_by_bow_kf, search_by_bow_kf_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def search_literal(kf1, kf2, nnratio=0.75, check_orientation=True, no_continue=()):
    """The reference's control flow, scalar, on the keyframes' own members.  no_continue: 1 / 2 drops the `continue` of that side (a
    misreading; the angle of such a row is then read as 0)."""
    d1, a1, nd1, good1, nleft1, nun1 = kf1
    d2, a2, nd2, good2, nleft2, nun2 = kf2
    matches12 = [-1] * len(nd1)                          # vpMapPoints1.size() entries
    matched2 = [False] * len(nd2)
    fv1, fv2 = feature_vector(nd1), feature_vector(nd2)
    keys1, keys2 = sorted(fv1), sorted(fv2)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    ratio = F32(nnratio)
    angle = lambda a, nun, i: a[i] if i < nun else F32(0)
    nmatches = 0
    a, b = 0, 0
    while a < len(keys1) and b < len(keys2):
        if keys1[a] == keys2[b]:
            for idx1 in fv1[keys1[a]]:
                if nleft1 != -1 and idx1 >= nun1 and 1 not in no_continue:       # :858-860
                    continue
                if not good1[idx1]:
                    continue
                best1, best_idx2, best2 = 256, -1, 256
                for idx2 in fv2[keys2[b]]:
                    if nleft2 != -1 and idx2 >= nun2 and 2 not in no_continue:   # :878-880
                        continue
                    if matched2[idx2] or not good2[idx2]:
                        continue
                    d = distance(d1[idx1], d2[idx2])
                    if d < best1:
                        best2, best1, best_idx2 = best1, d, idx2
                    elif d < best2:
                        best2 = d
                if best1 < TH_LOW and F32(best1) < F32(ratio * F32(best2)):
                    matches12[idx1] = best_idx2
                    matched2[best_idx2] = True
                    if check_orientation:
                        rot_hist[rot_bin(angle(a1, nun1, idx1), angle(a2, nun2, best_idx2))].append(idx1)      # :915
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


def masked(kf):
    """(desc, angle, node, valid) as the adapter gathers a keyframe for pli_search_by_bow_kf."""
    d, a, nd, good, nleft, nun = kf
    n = len(nd)
    rows = np.arange(n) < (nun if nleft != -1 else n)
    angle = np.zeros(n, np.float32)
    angle[rows] = np.asarray(a, np.float32)[:n][rows]
    return d, angle, nd, (np.asarray(good, np.uint8) & rows).astype(np.uint8)


def cases(seed=7):
    """(kf1, [kf2]) with mvKeysUn.size() equal to 0, NLeft and N on either side, between them, and keyframes of one camera."""
    rng = np.random.default_rng(seed)
    out = []
    for n1, nnodes in ((260, 12), (90, 1), (400, 40)):
        d1, a1, nd1, _, _, _, _ = random_case(rng, n1, 1, nnodes, ndup=0.5)
        good1 = (rng.random(n1) < 0.8).astype(np.uint8)
        nl1 = int(0.55 * n1)
        kfs = []
        for k, pick in enumerate(("zero", "nleft", "n", "between", "one", "nleft")):
            kd, ka, kn, kv = keyframe_of(rng, (d1, a1, nd1), int(rng.integers(40, 420)), nnodes=nnodes)
            n2 = len(kn)
            nl2 = int(0.5 * n2)
            nun2 = {"zero": 0, "nleft": nl2, "n": n2, "between": (nl2 + n2) // 2, "one": n2}[pick]
            kfs.append((kd, ka, kn, kv, -1 if pick == "one" else nl2, nun2))
        for nun1, nleft1 in ((nl1, nl1), (n1, nl1), (0, nl1), ((nl1 + n1) // 2, nl1), (n1, -1)):
            out.append(((d1, a1, nd1, good1, nleft1, nun1), kfs))
    return out


def test_the_literal_restatement_equals_the_kf_kf_restatement_fed_the_masks():
    total = cut = 0
    for kf1, kfs in cases():
        for kf2 in kfs:
            for ratio, ori in ((0.75, True), (0.7, False)):
                m, n = search_literal(kf1, kf2, ratio, ori)
                m2, n2 = search_by_bow_kf(*masked(kf1), *masked(kf2), ratio, ori)
                m3, n3 = search_by_bow_kf_fast(*masked(kf1), *masked(kf2), ratio, ori)
                assert np.array_equal(m, m2) and n == n2 and np.array_equal(m, m3) and n == n3
                assert len(m) == len(kf1[2])
                if kf1[4] != -1:
                    assert (m[kf1[5]:] == -1).all()
                if kf2[4] != -1:
                    assert (m < kf2[5]).all()
                total += n
                # the keyframes cut to their first mvKeysUn.size() rows, as one-camera keyframes: the same matches
                c1, c2 = [tuple(np.asarray(c)[:(kf[5] if kf[4] != -1 else len(kf[2]))] for c in masked(kf)) for kf in (kf1, kf2)]
                mc, nc = search_by_bow_kf(*c1, *c2, ratio, ori)
                assert nc == n and np.array_equal(mc, m[:len(mc)])
                cut += 1
    assert total > 0 and cut > 0


@pytest.mark.parametrize("side", [1, 2])
def test_the_cases_tell_a_missing_continue_apart(side):
    differ = 0
    for kf1, kfs in cases():
        for kf2 in kfs:
            differ += int((search_literal(kf1, kf2)[0] != search_literal(kf1, kf2, no_continue=(side,))[0]).sum())
    assert differ > 0


def test_the_adapter_hides_both_forms():
    src = open(os.path.join(ROOT, "pli_slam_amd", "adapters", "orbslam_two_cameras.hpp")).read()
    assert "int SearchByBoW(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12)" in src
    assert "void SearchByBoW(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpKF2," in src


def test_the_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    import subprocess
    import torch
    from test_cpp_bow_kf_two_cameras import build, write_input
    exe = build(str(tmp_path))
    kf1, kfs = cases()[0]
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, kf1, kfs[:2], 0.75, True)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
