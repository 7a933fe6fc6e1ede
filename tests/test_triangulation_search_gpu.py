"""pli_search_for_triangulation on the MI355X (the product library): ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12,
vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:965-1206, no second cameras) for one keyframe against a batch of neighbours
equals, for every neighbour, the Python restatement of tests/test_triangulation_search_cpu.py exactly (matches12 and nmatches).
F12 and the epipole are inputs of the entry point (host arithmetic of the adapter); here they come from a numpy helper."""
import numpy as np
import pytest

from pli_slam_amd import capi, realdata, synth
from test_triangulation_search_cpu import (NLEVELS, SETTINGS, Table, geometry_np, rot_xyz, search_for_triangulation,
                                           search_for_triangulation_fast, two_view_case)

pytestmark = pytest.mark.gpu
W, H = 752, 480


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=False)
    yield f
    f.close()


def keypoints(t):
    kp = np.zeros(len(t.node), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["angle"] = t.x, t.y, t.octave, t.angle
    kp["size"] = 31.0
    return kp


def kf_of(t):
    return keypoints(t), t.desc, t.node, t.has_mp, t.stereo


def check(fe, t1, nbrs, only_stereo=False, coarse=False, ori=False, scalar=False):
    """nbrs: (t2, F12, ep[, truth]) per neighbour.  Returns (matches12, nmatches) of the device, equal to the restatement's."""
    m, n = fe.search_for_triangulation(kf_of(t1), [kf_of(nb[0]) + (nb[1], nb[2]) for nb in nbrs], only_stereo, coarse, ori)
    assert m.shape == (len(nbrs), len(t1.node)) and n.shape == (len(nbrs),)
    restate = search_for_triangulation if scalar else search_for_triangulation_fast
    for k, nb in enumerate(nbrs):
        want_m, want_n = restate(t1, nb[0], nb[1], nb[2], only_stereo, coarse, ori)
        assert np.array_equal(m[k], want_m), "neighbour %d: %d of %d entries differ" % (k, int((m[k] != want_m).sum()), len(want_m))
        assert n[k] == want_n, (k, n[k], want_n)
    return m, n


@pytest.mark.parametrize("nkf", [0, 1, 10, 20])
def test_constructed_two_view_geometry(fe, nkf):
    """Random 3D points seen from two poses (tests/test_triangulation_search_cpu.py two_view_case: decoys off the line, twins,
    features at the epipole, map points, mono / stereo, one-sided nodes).  Every setting; the share of the true pairs that is
    recovered is the restatement's own share (the outputs are identical), printed for the record."""
    rng = np.random.default_rng(100 + nkf)
    t1, nbrs = two_view_case(rng, nkf, 500, nnodes=40)
    for only_stereo, coarse, ori in SETTINGS:
        m, n = check(fe, t1, nbrs, only_stereo, coarse, ori)
        if nkf == 0:
            assert m.shape == (0, len(t1.node)) and len(n) == 0
            continue
        got = want = true = 0
        for k, (t2, F12, ep, truth) in enumerate(nbrs):
            wm, _ = search_for_triangulation_fast(t1, t2, F12, ep, only_stereo, coarse, ori)
            true += int((truth >= 0).sum())
            got += int(((m[k] == truth) & (truth >= 0)).sum())
            want += int(((wm == truth) & (truth >= 0)).sum())
        print("nkf %d only_stereo %d coarse %d ori %d: %d matches, true pairs recovered %d of %d (restatement %d)"
              % (nkf, only_stereo, coarse, ori, int(n.sum()), got, true, want))
        assert got == want and n.sum() > 0
    if nkf:
        # the scalar restatement (the reference's control flow) on the first two neighbours as well
        check(fe, t1, nbrs[:2], False, False, True, scalar=True)


def test_nodes_with_more_than_64_candidates_and_many_ties(fe):
    rng = np.random.default_rng(5)
    t1, nbrs = two_view_case(rng, 3, 700, nnodes=2)
    for only_stereo, coarse, ori in ((False, False, True), (False, True, False), (True, False, False)):
        check(fe, t1, nbrs, only_stereo, coarse, ori)
    # every descriptor equal: distance 0 everywhere, the last listed candidate on the line wins
    same = lambda t: t._replace(desc=np.zeros_like(t.desc))
    check(fe, same(t1), [(same(nb[0]),) + nb[1:] for nb in nbrs], False, False, True)
    check(fe, same(t1), [(same(nb[0]),) + nb[1:] for nb in nbrs], False, True, False)


# ---- real ORB tables --------------------------------------------------------------------------------------------------

_vocabs = {}


def vocab(fe, k, L, seed=0):
    if (k, L, seed) not in _vocabs:
        _vocabs[(k, L, seed)] = fe.vocab_create(*synth.make_vocabulary(k, L, seed=seed))
    return _vocabs[(k, L, seed)]


def orb_table(fe, rng, img, voc, levelsup, mp_frac=0.2):
    """mvKeysUn / mDescriptors of one image from the device's extractor, the FeatureVector of pli_bow_transform, random map
    points and stereo flags (a synthetic mvuRight)."""
    n, kp, desc = fe.orb_extract(0, img)
    _, weight, node = fe.bow_transform(voc, desc, levelsup)
    ang = kp["angle"].astype(np.float32)
    assert ang.min() >= 0 and ang.max() < 360 and kp["octave"].max() < NLEVELS
    return Table(kp["x"].astype(np.float32), kp["y"].astype(np.float32), kp["octave"].astype(np.int32), ang, desc.copy(),
                 np.where(weight > 0, node, -1).astype(np.int32), (rng.random(n) < mp_frac).astype(np.uint8),
                 (rng.random(n) < 0.6).astype(np.uint8))


I3, Z3 = np.eye(3), np.zeros(3)
# the right camera of a rectified pair (epipolar lines = rows, the epipole at infinity) and a small forward motion (epipole in
# the image).  Any fixed pose serves: the test is parity with the restatement, not geometry.
SIDEWAYS = geometry_np(I3, Z3, I3, np.array([-0.11, 0.0, 0.0]))
FORWARD = geometry_np(I3, Z3, rot_xyz(0.002, -0.003, 0.0087), np.array([0.01, 0.004, -0.25]))


def test_real_orb_tables_synthetic_scenes(fe):
    """pKF1 = the left image of frame t; neighbours: its right image (lines = rows), the left image of t + 1 (3 px, 1 px, 0.5 deg
    away: mostly off its lines unless bCoarse) and itself under the forward motion."""
    rng = np.random.default_rng(1)
    voc = vocab(fe, 10, 4)
    total = 0
    for s in (3, 11):
        for lu in (2, 1):
            L0, R0 = synth.make_stereo_pair(s, W, H, t=0)
            t1 = orb_table(fe, rng, L0, voc, lu)
            nbrs = [(orb_table(fe, rng, R0, voc, lu),) + SIDEWAYS,
                    (orb_table(fe, rng, synth.make_stereo_pair(s, W, H, t=1)[0], voc, lu),) + FORWARD,
                    (orb_table(fe, rng, L0, voc, lu, mp_frac=0.0),) + FORWARD]
            for only_stereo, coarse, ori in SETTINGS:
                n = check(fe, t1, nbrs, only_stereo, coarse, ori)[1]
                total += int(n.sum())
    print("synthetic scenes: %d matches" % total)
    # the restatement yields 22621 matches for these seeds (the tables come from the device's extractor); floor = half of it
    assert total > 11310, total


def test_real_photographs(fe):
    rng = np.random.default_rng(2)
    voc = vocab(fe, 8, 5, seed=3)
    total = 0
    for L, R in realdata.frames_752x480(3, seed=4):
        for lu in (3, 2):
            t1 = orb_table(fe, rng, L, voc, lu)
            nbrs = [(orb_table(fe, rng, R, voc, lu),) + SIDEWAYS, (orb_table(fe, rng, L, voc, lu, mp_frac=0.0),) + FORWARD]
            for only_stereo, coarse, ori in ((False, False, False), (False, False, True), (True, False, True), (False, True, False)):
                total += int(check(fe, t1, nbrs, only_stereo, coarse, ori)[1].sum())
    print("photographs: %d matches" % total)
    # the restatement yields 21894 matches for these seeds; floor = half of it
    assert total > 10947, total


# ---- the call itself --------------------------------------------------------------------------------------------------

def test_a_batch_equals_single_calls_and_calls_repeat(fe):
    rng = np.random.default_rng(9)
    t1, nbrs = two_view_case(rng, 7, 400, nnodes=20)
    kfs = [kf_of(nb[0]) + (nb[1], nb[2]) for nb in nbrs]
    for only_stereo, coarse, ori in ((False, False, True), (True, False, False), (False, True, True)):
        m, n = fe.search_for_triangulation(kf_of(t1), kfs, only_stereo, coarse, ori)
        for k in range(len(kfs)):
            m1, n1 = fe.search_for_triangulation(kf_of(t1), kfs[k:k + 1], only_stereo, coarse, ori)
            assert np.array_equal(m1[0], m[k]) and n1[0] == n[k]
        for _ in range(3):
            m2, n2 = fe.search_for_triangulation(kf_of(t1), kfs, only_stereo, coarse, ori)
            assert np.array_equal(m2, m) and np.array_equal(n2, n)
        assert n.sum() > 0


def test_neighbours_of_different_sizes_and_empty_tables(fe):
    rng = np.random.default_rng(10)
    t1, nbrs = two_view_case(rng, 3, 300, nnodes=10)
    cut = lambda t, n: Table(*[col[:n] for col in t])
    mixed = [nbrs[0], (cut(nbrs[1][0], 0),) + nbrs[1][1:3], (cut(nbrs[2][0], 37),) + nbrs[2][1:3], (cut(nbrs[0][0], 1),) + nbrs[0][1:3]]
    m, n = check(fe, t1, mixed, False, False, True)
    assert n[1] == 0 and (m[1] == -1).all()
    # an empty pKF1: no matches, for every neighbour
    m, n = check(fe, cut(t1, 0), mixed)
    assert m.shape == (4, 0) and (n == 0).all()
    # no neighbours
    m, n = fe.search_for_triangulation(kf_of(t1), [])
    assert m.shape == (0, len(t1.node)) and n.shape == (0,)


def test_capacity_and_arguments(fe):
    rng = np.random.default_rng(3)
    cap = 8192                                            # PLI_BOW_MAX_FEATURES

    def table(n):
        return Table(rng.uniform(0, W, n).astype(np.float32), rng.uniform(0, H, n).astype(np.float32),
                     rng.integers(0, NLEVELS, n).astype(np.int32), rng.uniform(0, 359, n).astype(np.float32),
                     rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(-1, 30, n).astype(np.int32),
                     np.zeros(n, np.uint8), np.ones(n, np.uint8))
    small, big, full = table(50), table(cap + 1), table(cap)
    for kf1, kfs in ((big, [small]), (small, [small, big])):
        with pytest.raises(capi.PliError) as e:
            fe.search_for_triangulation(kf_of(kf1), [kf_of(t) + SIDEWAYS for t in kfs])
        assert e.value.status == -3                 # PLI_ERR_CAPACITY
    # exactly at the cap, on both sides, under bCoarse (every pair of a node is a candidate)
    check(fe, full, [(full,) + FORWARD, (small,) + FORWARD], False, True, True)
    # an octave outside the context's levels, an angle outside [0, 360) with the orientation check, a node below -1
    for field, value, ori in (("octave", NLEVELS, False), ("octave", -1, False), ("angle", 360.0, True), ("node", -2, False)):
        bad = small._replace(**{field: np.concatenate([getattr(small, field)[:-1], [value]]).astype(getattr(small, field).dtype)})
        for kf1, kfs in ((bad, [small]), (small, [bad])):
            with pytest.raises(capi.PliError) as e:
                fe.search_for_triangulation(kf_of(kf1), [kf_of(t) + SIDEWAYS for t in kfs], check_orientation=ori)
            assert e.value.status == -1             # PLI_ERR_INVALID
    check(fe, small._replace(angle=np.full(50, 400.0, np.float32)), [(small,) + FORWARD])      # angles are not read without it
