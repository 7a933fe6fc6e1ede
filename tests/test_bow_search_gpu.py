"""pli_search_by_bow on the MI355X (the product library): ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches)
(ORBmatcher.cc:269-470, F.Nleft == -1) for a batch of keyframes against one frame equals, for every keyframe, the Python
restatement of tests/test_bow_search_cpu.py exactly (matches and nmatches).  FeatureVectors come from pli_bow_transform on
synthetic DBoW2 vocabularies (node_id where weight > 0, else -1), as Frame::ComputeBoW builds them."""
import numpy as np
import pytest

from pli_slam_amd import capi, realdata, synth
from test_bow_search_cpu import keyframe_of, random_case, search_by_bow, search_by_bow_fast

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


_vocabs = {}


def vocab(fe, k, L, seed=0):
    if (k, L, seed) not in _vocabs:
        _vocabs[(k, L, seed)] = fe.vocab_create(*synth.make_vocabulary(k, L, seed=seed))
    return _vocabs[(k, L, seed)]


def nodes(fe, voc, desc, levelsup):
    """The FeatureVector of transform(): node_id of every feature whose word is not stopped, else -1."""
    _, weight, node = fe.bow_transform(voc, desc, levelsup)
    return np.where(weight > 0, node, -1).astype(np.int32)


def check(fe, frame, kfs, nnratio=0.75, check_orientation=True):
    fd, fa, fn = frame
    m, n = fe.search_by_bow(fd, fa, fn, kfs, nnratio=nnratio, check_orientation=check_orientation)
    assert m.shape == (len(kfs), len(fn)) and n.shape == (len(kfs),)
    for k, (kd, ka, kn, kv) in enumerate(kfs):
        want_m, want_n = search_by_bow_fast(kd, ka, kn, kv, fd, fa, fn, nnratio, check_orientation)
        assert np.array_equal(m[k], want_m), "keyframe %d: %d of %d matches differ" % (k, int((m[k] != want_m).sum()), len(fn))
        assert n[k] == want_n, (k, n[k], want_n)
    return m, n


def orb(fe, img):
    n, kp, desc = fe.orb_extract(0, img)
    return desc, kp["angle"].astype(np.float32)


def invalid_mask(rng, n, frac):
    return (rng.random(n) >= frac).astype(np.uint8)


def test_real_orb_tables_synthetic_scenes(fe):
    """Keyframe = frame t = 0 of a synthetic sequence, frames t = 1..3; bow_transform -> search_by_bow on the device's tables."""
    rng = np.random.default_rng(1)
    voc = vocab(fe, 10, 4)
    total = 0
    for s in (3, 11):
        kd, ka = orb(fe, synth.make_stereo_pair(s, W, H, t=0)[0])
        valid = [invalid_mask(rng, len(kd), frac) for frac in (0.0, 0.2, 0.4)]
        for t in (1, 2, 3):
            fd, fa = orb(fe, synth.make_stereo_pair(s, W, H, t=t)[0])
            for lu in (2, 1):
                kn = nodes(fe, voc, kd, lu)
                kfs = [(kd, ka, kn, v) for v in valid]
                for ratio, ori in ((0.7, True), (0.75, True), (0.75, False)):
                    total += int(check(fe, (fd, fa, nodes(fe, voc, fd, lu)), kfs, ratio, ori)[1].sum())
    assert total > 1000, "the synthetic sequences should match plenty of features (%d)" % total


def test_real_photographs(fe):
    rng = np.random.default_rng(2)
    voc = vocab(fe, 8, 5, seed=3)
    total = 0
    for L, R in realdata.frames_752x480(3, seed=4):
        kd, ka = orb(fe, L)
        fd, fa = orb(fe, R)
        for lu in (3, 2):
            kfs = [(kd, ka, nodes(fe, voc, kd, lu), invalid_mask(rng, len(kd), frac)) for frac in (0.0, 0.3)]
            for ratio, ori in ((0.7, True), (0.75, False)):
                total += int(check(fe, (fd, fa, nodes(fe, voc, fd, lu)), kfs, ratio, ori)[1].sum())
    assert total > 500, total


@pytest.mark.parametrize("k,L", [(10, 3), (6, 5), (4, 2)])
def test_synthetic_vocabularies_every_levelsup(fe, k, L):
    """levelsup 4, 1, 0 and >= L (every feature in node 0: more than 64 candidates in one node)."""
    rng = np.random.default_rng(k * 10 + L)
    voc = vocab(fe, k, L, seed=k + L)
    for levelsup in (4, 1, 0, L, L + 3):
        n_f = 300 if levelsup >= L else 900
        kd, ka, _, kv, fd, fa, _ = random_case(rng, n_f, n_f, 1, ndup=0.5, invalid=0.25)
        fn = nodes(fe, voc, fd, levelsup)
        kfs = [(kd, ka, nodes(fe, voc, kd, levelsup), kv)]
        kd2, ka2, _, kv2 = keyframe_of(rng, (fd, fa, fn), 500, invalid=0.0)
        kfs.append((kd2, ka2, nodes(fe, voc, kd2, levelsup), kv2))
        if levelsup >= L:
            assert (fn[fn >= 0] == 0).all() and (fn == 0).sum() > 64
        for ratio, ori in ((0.7, True), (0.75, False)):
            check(fe, (fd, fa, fn), kfs, ratio, ori)


def test_tie_rich_descriptors_and_invalid_fractions(fe):
    """Exact and near duplicates: the first listed frame feature on ties, bestDist2 == bestDist1 rejections."""
    rng = np.random.default_rng(7)
    for frac in (0.0, 0.1, 0.4):
        base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
        fd = base[rng.integers(0, 40, 700)].copy()
        kd = base[rng.integers(0, 40, 600)].copy()
        for d in (fd, kd):                      # a third of them one or two bits away from their base
            rows = rng.choice(len(d), len(d) // 3, replace=False)
            d[rows, rng.integers(0, 32, len(rows))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        fn, kn = rng.integers(-1, 12, 700).astype(np.int32), rng.integers(-1, 12, 600).astype(np.int32)
        fa, ka = rng.uniform(0, 360, 700).astype(np.float32), rng.uniform(0, 360, 600).astype(np.float32)
        kfs = [(kd, ka, kn, invalid_mask(rng, 600, frac))]
        for ratio in (0.7, 0.75, 1.2):
            for ori in (True, False):
                check(fe, (fd, fa, fn), kfs, ratio, ori)


def batch_of(rng, nkf, nf=400, nnodes=30):
    _, _, _, _, fd, fa, fn = random_case(rng, 1, nf, nnodes, ndup=0.5)
    kfs = []
    for k in range(nkf):
        kf = keyframe_of(rng, (fd, fa, fn), int(rng.integers(0, 500)), invalid=float(rng.uniform(0, 0.4)))
        if k % 7 == 3:
            kf[3][:] = 0                                # a keyframe without a valid map point
        kfs.append(kf)
    return (fd, fa, fn), kfs


@pytest.mark.parametrize("nkf", [0, 1, 64, 300])
def test_batches_of_keyframes(fe, nkf):
    rng = np.random.default_rng(100 + nkf)
    f, kfs = batch_of(rng, nkf)
    m, n = check(fe, f, kfs, 0.75, True)
    if nkf >= 64:
        assert (n == 0).any() and n.max() > 0


def test_one_batch_equals_single_calls_and_permutes_with_the_keyframes(fe):
    rng = np.random.default_rng(9)
    f, kfs = batch_of(rng, 24)
    m, n = fe.search_by_bow(*f, kfs, 0.7, True)
    for k, kf in enumerate(kfs):
        m1, n1 = fe.search_by_bow(*f, [kf], 0.7, True)
        assert np.array_equal(m1[0], m[k]) and n1[0] == n[k]
    perm = rng.permutation(len(kfs))
    mp, np_ = fe.search_by_bow(*f, [kfs[i] for i in perm], 0.7, True)
    assert np.array_equal(mp, m[perm]) and np.array_equal(np_, n[perm])


def test_empty_frame_and_empty_keyframes(fe):
    rng = np.random.default_rng(3)
    _, kfs = batch_of(rng, 5)
    e = (np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int32))
    m, n = fe.search_by_bow(*e, kfs)
    assert m.shape == (5, 0) and (n == 0).all()
    f, _ = batch_of(rng, 0)
    m, n = fe.search_by_bow(*f, [e + (np.zeros(0, np.uint8),)] * 3)
    assert (m == -1).all() and (n == 0).all()


def test_the_4k_shape(fe):
    """BASELINE config 5's frame size: about 4000 features per frame and keyframe."""
    rng = np.random.default_rng(4000)
    voc = vocab(fe, 10, 4)
    kd, ka, _, kv, fd, fa, _ = random_case(rng, 4100, 3990, 1, ndup=0.6, invalid=0.2)
    kfs = [(kd, ka, nodes(fe, voc, kd, 2), kv), (kd[:3000], ka[:3000], nodes(fe, voc, kd[:3000], 2), kv[:3000])]
    check(fe, (fd, fa, nodes(fe, voc, fd, 2)), kfs, 0.75, True)


def test_at_and_over_capacity(fe):
    cap = 8192
    rng = np.random.default_rng(8192)
    kd, ka, kn, kv, fd, fa, fn = random_case(rng, cap, cap, 2000, ndup=0.6, invalid=0.1)
    check(fe, (fd, fa, fn), [(kd, ka, kn, kv)], 0.75, True)
    big = random_case(rng, cap + 1, cap + 1, 2000)
    with pytest.raises(capi.PliError) as e:
        fe.search_by_bow(big[4], big[5], big[6], [(kd, ka, kn, kv)])
    assert e.value.status == -3                     # PLI_ERR_CAPACITY: the frame
    with pytest.raises(capi.PliError) as e:
        fe.search_by_bow(fd, fa, fn, [(kd, ka, kn, kv), big[:4]])
    assert e.value.status == -3                     # PLI_ERR_CAPACITY: the second keyframe
    bad = fa.copy()
    bad[5] = 360.0
    with pytest.raises(capi.PliError) as e:
        fe.search_by_bow(fd, bad, fn, [(kd, ka, kn, kv)])
    assert e.value.status == -1                     # PLI_ERR_INVALID: an angle outside [0, 360) with the orientation check
    fe.search_by_bow(fd, bad, fn, [(kd, ka, kn, kv)], check_orientation=False)


def test_the_scalar_restatement_on_one_device_case(fe):
    """The vectorised restatement used above against the scalar one on a device case (tie-rich, two keyframes)."""
    rng = np.random.default_rng(11)
    f, kfs = batch_of(rng, 2, nf=200, nnodes=8)
    m, n = fe.search_by_bow(*f, kfs, 0.75, True)
    for k, (kd, ka, kn, kv) in enumerate(kfs):
        want_m, want_n = search_by_bow(kd, ka, kn, kv, *f, 0.75, True)
        assert np.array_equal(m[k], want_m) and n[k] == want_n


def check_scalar(fe, frame, kfs):
    """Exact equality with the scalar restatement, with and without the rotation filter."""
    for ori in (True, False):
        m, n = fe.search_by_bow(*frame, kfs, 0.75, ori)
        assert m.shape == (len(kfs), len(frame[2])) and n.shape == (len(kfs),)
        for k, (kd, ka, kn, kv) in enumerate(kfs):
            want_m, want_n = search_by_bow(kd, ka, kn, kv, *frame, 0.75, ori)
            assert np.array_equal(m[k], want_m) and n[k] == want_n, (ori, k, n[k], want_n)
    return m, n


@pytest.fixture(scope="module")
def small_scene():
    """A 65-feature frame in 4 nodes (every feature listed) and two keyframes of 65 features that see it."""
    rng = np.random.default_rng(65)
    _, _, _, _, fd, fa, fn = random_case(rng, 1, 65, 4, ndup=0.5)
    fn = np.abs(fn).astype(np.int32)                    # -1 -> 1: every feature listed
    kfs = [keyframe_of(rng, (fd, fa, fn), 65, invalid=0.1, nnodes=4) for _ in range(2)]
    return (fd, fa, fn), kfs


@pytest.mark.parametrize("nf", [1, 2, 63, 64, 65])
def test_frame_sizes_around_a_wave_and_a_power_of_two(fe, small_scene, nf):
    """The frame's sort runs in the batch sort kernel as one table without an offset list: one feature, one wave less one, a whole
    wave (a power of two), one more."""
    (fd, fa, fn), kfs = small_scene
    m, n = check_scalar(fe, (fd[:nf], fa[:nf], fn[:nf]), kfs)
    if nf >= 63:
        assert n.min() > 0


def test_a_frame_listed_in_no_node(fe, small_scene):
    (fd, fa, fn), kfs = small_scene
    m, n = check_scalar(fe, (fd, fa, np.full(len(fn), -1, np.int32)), kfs)
    assert (m == -1).all() and (n == 0).all()


def test_only_frame_feature_0_unlisted(fe, small_scene):
    (fd, fa, fn), kfs = small_scene
    fn = fn.copy()
    fn[0] = -1
    m, n = check_scalar(fe, (fd, fa, fn), kfs)
    assert (m[:, 0] == -1).all() and n.min() > 0


def test_a_batch_whose_first_and_last_keyframe_are_empty(fe, small_scene):
    frame, kfs = small_scene
    e = (np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    m, n = check_scalar(fe, frame, [e, kfs[0], kfs[1], e])
    assert n[0] == 0 and n[3] == 0 and n[1] > 0 and n[2] > 0
