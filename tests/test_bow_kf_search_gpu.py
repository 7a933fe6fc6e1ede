"""pli_search_by_bow_kf on the MI355X (the product library): ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12)
(ORBmatcher.cc:823-963, NLeft == -1) for one keyframe against a batch of keyframes equals, for every pair, the Python restatement
of tests/test_bow_kf_search_cpu.py exactly (matches12 and nmatches).  FeatureVectors of the real ORB tables come from
pli_bow_transform on synthetic DBoW2 vocabularies (node_id where weight > 0, else -1), as KeyFrame::ComputeBoW builds them."""
import numpy as np
import pytest

from pli_slam_amd import capi, synth
from test_bow_search_cpu import keyframe_of
from test_bow_kf_search_cpu import batch_of, boundary_case, kf_pair_case, search_by_bow_kf, search_by_bow_kf_fast

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


def nodes(fe, voc, desc, levelsup):
    """The FeatureVector of transform(): node_id of every feature whose word is not stopped, else -1."""
    _, weight, node = fe.bow_transform(voc, desc, levelsup)
    return np.where(weight > 0, node, -1).astype(np.int32)


def check(fe, t1, kfs, nnratio=0.75, check_orientation=True, restatement=search_by_bow_kf_fast):
    m, n = fe.search_by_bow_kf(*t1, kfs, nnratio=nnratio, check_orientation=check_orientation)
    assert m.shape == (len(kfs), len(t1[2])) and n.shape == (len(kfs),)
    for k, kf in enumerate(kfs):
        want_m, want_n = restatement(*t1, *kf, nnratio, check_orientation)
        assert np.array_equal(m[k], want_m), "keyframe %d: %d of %d rows differ" % (k, int((m[k] != want_m).sum()), len(want_m))
        assert n[k] == want_n, (k, n[k], want_n)
    return m, n


def invalid_mask(rng, n, frac):
    return (rng.random(n) >= frac).astype(np.uint8)


def test_the_scalar_restatement_on_one_device_case(fe):
    rng = np.random.default_rng(11)
    t1, kfs = batch_of(rng, 2, n1=200, nnodes=8, max_n2=250)
    assert check(fe, t1, kfs, 0.75, True, restatement=search_by_bow_kf)[1].sum() > 0


def test_real_orb_tables_synthetic_scenes(fe):
    """pKF1 = frame t = 0 of a synthetic sequence, the keyframes are frames t = 1..3; bow_transform -> search_by_bow_kf."""
    rng = np.random.default_rng(1)
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))
    try:
        tabs = []
        for t in range(4):
            n, kp, desc = fe.orb_extract(0, synth.make_stereo_pair(3, W, H, t=t)[0])
            tabs.append((desc, kp["angle"].astype(np.float32)))
        total = 0
        for lu in (2, 1):
            nd = [nodes(fe, voc, d, lu) for d, _ in tabs]
            for frac in (0.0, 0.3):
                t1 = tabs[0] + (nd[0], invalid_mask(rng, len(nd[0]), frac))
                kfs = [tabs[t] + (nd[t], invalid_mask(rng, len(nd[t]), frac)) for t in (1, 2, 3)]
                total += int(check(fe, t1, kfs, 0.75, True)[1].sum())
    finally:
        fe.vocab_destroy(voc)
    assert total > 200, "the synthetic sequence should match plenty of features (%d)" % total


def test_a_single_node_with_more_than_64_candidates_and_a_run_longer_than_one_chunk(fe):
    """levelsup >= L: every listed feature sits in node 0, about 300 on each side."""
    rng = np.random.default_rng(64)
    voc = fe.vocab_create(*synth.make_vocabulary(6, 3, seed=9))
    try:
        t1, t2 = kf_pair_case(rng, 300, 310, 1, ndup=0.5, invalid=0.15)
        n1, n2 = nodes(fe, voc, t1[0], 3), nodes(fe, voc, t2[0], 5)
        assert (n1[n1 >= 0] == 0).all() and (n2[n2 >= 0] == 0).all()
        assert ((n1 == 0) & (t1[3] != 0)).sum() > 64 and ((n2 == 0) & (t2[3] != 0)).sum() > 64
        for ratio, ori in ((0.75, True), (1.2, False)):
            assert check(fe, (t1[0], t1[1], n1, t1[3]), [(t2[0], t2[1], n2, t2[3])], ratio, ori)[1].sum() > 0
    finally:
        fe.vocab_destroy(voc)


def test_tie_rich_descriptors_and_the_boundary_of_th_low(fe):
    """Exact and near duplicates of 40 base rows: the lowest idx2 on ties, bestDist2 == bestDist1 rejections; then best distances
    of exactly 49, 50 and 51."""
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    tabs = []
    for n in (600, 700):
        d = base[rng.integers(0, 40, n)].copy()
        rows = rng.choice(n, n // 3, replace=False)                          # a third of them one bit away from their base
        d[rows, rng.integers(0, 32, len(rows))] ^= (1 << rng.integers(0, 8, len(rows))).astype(np.uint8)
        tabs.append((d, rng.uniform(0, 360, n).astype(np.float32), rng.integers(-1, 12, n).astype(np.int32), invalid_mask(rng, n, 0.1)))
    total = 0
    for ratio in (0.7, 0.75, 1.2):
        for ori in (True, False):
            total += int(check(fe, tabs[0], [tabs[1]], ratio, ori)[1].sum())
    assert total > 0
    t1, t2 = boundary_case()
    m, n = check(fe, t1, [t2], 0.75, True)
    assert n[0] == 12 and (m[0].reshape(6, 4) >= 0).tolist() == [[True, False, False, True]] * 6


@pytest.mark.parametrize("nkf", [0, 1, 64])
def test_batches_of_keyframes(fe, nkf):
    """Every fifth keyframe is empty, every seventh has no valid feature (batch_of)."""
    rng = np.random.default_rng(100 + nkf)
    t1, kfs = batch_of(rng, nkf, n1=300, max_n2=350)
    m, n = check(fe, t1, kfs, 0.75, True)
    if nkf >= 64:
        assert (n == 0).any() and n.max() > 0 and len(kfs[4][2]) == 0 and not kfs[3][3].any()


def test_one_batch_equals_single_calls_and_permutes_with_the_keyframes(fe):
    rng = np.random.default_rng(9)
    t1, kfs = batch_of(rng, 12, n1=300, max_n2=350)
    m, n = fe.search_by_bow_kf(*t1, kfs, 0.7, True)
    assert n.sum() > 0
    for k, kf in enumerate(kfs):
        m1, n1 = fe.search_by_bow_kf(*t1, [kf], 0.7, True)
        assert np.array_equal(m1[0], m[k]) and n1[0] == n[k]
    perm = rng.permutation(len(kfs))
    mp, np_ = fe.search_by_bow_kf(*t1, [kfs[i] for i in perm], 0.7, True)
    assert np.array_equal(mp, m[perm]) and np.array_equal(np_, n[perm])


def test_an_empty_first_keyframe(fe):
    rng = np.random.default_rng(3)
    _, kfs = batch_of(rng, 5)
    e = (np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    m, n = fe.search_by_bow_kf(*e, kfs)
    assert m.shape == (5, 0) and (n == 0).all()
    t1, _ = batch_of(rng, 0)
    m, n = fe.search_by_bow_kf(*t1, [e] * 3)
    assert m.shape == (3, len(t1[2])) and (m == -1).all() and (n == 0).all()


def test_at_and_over_capacity(fe):
    cap = 8192
    rng = np.random.default_rng(8192)
    t1, _ = kf_pair_case(rng, cap, 1, 60, ndup=0.6, invalid=0.1)
    t2 = keyframe_of(rng, t1[:3], cap, invalid=0.1, nnodes=60)          # about 130 features per node on each side
    assert check(fe, t1, [t2], 0.75, True)[1][0] > 500
    b1, b2 = kf_pair_case(rng, cap + 1, cap + 1, 2000)
    with pytest.raises(capi.PliError) as e:
        fe.search_by_bow_kf(*b1, [t2])
    assert e.value.status == -3                     # PLI_ERR_CAPACITY: pKF1
    with pytest.raises(capi.PliError) as e:
        fe.search_by_bow_kf(*t1, [t2, b2])
    assert e.value.status == -3                     # PLI_ERR_CAPACITY: the second keyframe
    for side in (0, 1):
        bad = t1[1].copy() if side == 0 else t2[1].copy()
        bad[5] = 360.0
        a1 = (t1[0], bad, t1[2], t1[3]) if side == 0 else t1
        a2 = t2 if side == 0 else (t2[0], bad, t2[2], t2[3])
        with pytest.raises(capi.PliError) as e:
            fe.search_by_bow_kf(*a1, [a2])
        assert e.value.status == -1                 # PLI_ERR_INVALID: an angle outside [0, 360) with the orientation check
        check(fe, a1, [a2], 0.75, False)            # accepted without it
