"""pli_search_by_bow_two_cameras on the MI355X (the product library): ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches)
(ORBmatcher.cc:269-470) for a frame of two cameras (F.Nleft != -1, :342-369, :373-433) and a batch of keyframes equals, for every
keyframe, the Python restatements of tests/test_bow_two_cameras_cpu.py exactly (matches and nmatches).  That file shows, on the
CPU, that the corpus takes every exit of the branch and tells the wrong readings apart."""
import numpy as np
import pytest

from pli_slam_amd import capi
from test_bow_search_cpu import desc_with_bits
from test_bow_two_cameras_cpu import F_NLEFT, NF, SETTINGS, Z, corpus, search_closed, search_scalar

pytestmark = pytest.mark.gpu
W, H = 512, 512


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=False)
    yield f
    f.close()


def check(fe, frame, kfs, nleft, nnratio=0.7, check_orientation=True, fn=search_closed):
    fd, fa, fnode = frame
    m, n = fe.search_by_bow_two_cameras(kfs, fd, fa, fnode, nleft, nnratio=nnratio, check_orientation=check_orientation)
    assert m.shape == (len(kfs), len(fnode)) and n.shape == (len(kfs),)
    for k, kf in enumerate(kfs):
        want_m, want_n = fn(*kf, fd, fa, fnode, nleft, nnratio, check_orientation)
        assert np.array_equal(m[k], want_m), "keyframe %d: %d of %d matches differ" % (k, int((m[k] != want_m).sum()), len(fnode))
        assert n[k] == want_n, (k, n[k], want_n)
    return m, n


@pytest.mark.parametrize("nkf", [0, 1, 4])
def test_the_corpus(fe, nkf):
    frame, kfs = corpus(nkf)
    total = 0
    for ratio, ori in SETTINGS:
        m, n = check(fe, frame, kfs, F_NLEFT, ratio, ori)
        total += int(n.sum())
        if nkf:
            assert (m[:, :F_NLEFT] >= 0).sum() > 20 * nkf and (m[:, F_NLEFT:] >= 0).sum() > 20 * nkf      # both cameras match
    if nkf:
        check(fe, frame, kfs[:1], F_NLEFT, 0.7, True, fn=search_scalar)       # the reference's control flow on one keyframe
    assert (total > 0) == (nkf > 0)


def test_every_feature_on_the_left_is_the_one_camera_search_and_none_matches_nothing(fe):
    frame, kfs = corpus(4)
    fd, fa, fnode = frame
    for ratio, ori in SETTINGS:
        m, n = check(fe, frame, kfs, NF, ratio, ori)
        m1, n1 = fe.search_by_bow(fd, fa, fnode, kfs, nnratio=ratio, check_orientation=ori)
        assert np.array_equal(m, m1) and np.array_equal(n, n1) and n.sum() > 0
        m, n = check(fe, frame, kfs, 0, ratio, ori)
        assert (m == -1).all() and (n == 0).all()
    for nleft in (1, 64, 65, NF - 1):                                # other splits of the same tables
        check(fe, frame, kfs[:2], nleft)


def tables(kf, f):
    kfs = [(np.array([x[0] for x in kf], np.uint8).reshape(-1, 32), np.array([x[1] for x in kf], np.float32),
            np.array([x[2] for x in kf], np.int32), np.ones(len(kf), np.uint8))]
    frame = (np.array([x[0] for x in f], np.uint8).reshape(-1, 32), np.array([x[1] for x in f], np.float32),
             np.array([x[2] for x in f], np.int32))
    return frame, kfs


def test_known_answers(fe):
    # a right candidate at distance 0 whose keyframe feature has no left candidate within TH_LOW stays unmatched
    frame, kfs = tables([(Z, 0, 7)], [(desc_with_bits(51), 0, 7), (Z, 0, 7)])
    assert check(fe, frame, kfs, 1, check_orientation=False)[0].tolist() == [[-1, -1]]
    # a right match is taken where the left failed its ratio test (30 < 0.7 * 40 fails)
    frame, kfs = tables([(Z, 0, 3)], [(desc_with_bits(30), 0, 3), (desc_with_bits(40, offset=60), 0, 3), (desc_with_bits(10, offset=120), 0, 3)])
    assert check(fe, frame, kfs, 2, check_orientation=False)[0].tolist() == [[-1, -1, 0]]
    # a right match is taken with bestDist1R == bestDist2R: no ratio test; the first listed
    frame, kfs = tables([(Z, 0, 3)], [(desc_with_bits(5), 0, 3), (desc_with_bits(10, offset=60), 0, 3), (desc_with_bits(10, offset=120), 0, 3)])
    assert check(fe, frame, kfs, 1, check_orientation=False)[0].tolist() == [[0, 0, -1]]
    # the rotation filter removes matches of both cameras (the case of the CPU file)
    kf, left, right = [], [], []
    for i in range(12):
        d = desc_with_bits(3, offset=(i * 17) % 250)
        kf.append((d, 90.0 if i == 11 else 0.0, 100 + i))
        left.append((d, 0.0, 100 + i))
        right.append((d, 0.0, 100 + i))
    frame, kfs = tables(kf, left + right)
    m, n = check(fe, frame, kfs, 12, check_orientation=True)
    assert n.tolist() == [22] and m[0].tolist() == list(range(11)) + [-1] + list(range(11)) + [-1]
    assert check(fe, frame, kfs, 12, check_orientation=False)[1].tolist() == [24]


def test_arguments(fe):
    frame, kfs = corpus(1)
    for nleft in (-1, NF + 1):
        with pytest.raises(capi.PliError) as e:
            fe.search_by_bow_two_cameras(kfs, *frame, nleft)
        assert e.value.status == -1                          # PLI_ERR_INVALID
    m, n = fe.search_by_bow_two_cameras(kfs, frame[0][:0], frame[1][:0], frame[2][:0], 0)
    assert m.shape == (1, 0) and n.tolist() == [0]
