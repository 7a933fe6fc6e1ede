"""pli_search_for_triangulation_two_cameras on the MI355X (the product library): ORBmatcher::SearchForTriangulation
(ORBmatcher.cc:965-1206) for keyframes of two KannalaBrandt8 cameras, one keyframe against a batch of neighbours, equals for every
neighbour the Python restatement of tests/test_triangulation_two_cameras_cpu.py exactly (matches12 and nmatches).  The gate of the
restatement is float64; every pair of the constructed corpus that reaches it is decided (see that file), so nothing is left
out there.  On the extracted tables a row of pKF1 with an undecided candidate is left out, at most 2 % of the rows that have a
candidate within TH_LOW (the CPU file asserts that cap on the same scene with the float64 statement alone)."""
import numpy as np
import pytest

from pli_slam_amd import capi, synth
import test_triangulation_two_cameras_cpu as two
from test_triangulation_two_cameras_cpu import CAMS, Table, corpus, search_closed, search_scalar

pytestmark = pytest.mark.gpu
PLI_ERR_INVALID, PLI_ERR_CAPACITY = -1, -3


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(two.scene_config(), dev=False)
    yield f
    f.close()


def keypoints(t):
    kp = np.zeros(len(t.node), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"], kp["angle"] = t.x, t.y, t.octave, t.angle
    kp["size"] = 31.0
    return kp


def kf_of(t):
    return keypoints(t), t.desc, t.node, t.has_mp, t.nleft


def nb_of(nb):
    return kf_of(nb.t2) + (nb.rel,)


def call(fe, t1, nbrs, coarse=False, ori=False, only_stereo=False):
    return fe.search_for_triangulation_two_cameras(kf_of(t1), [nb_of(nb) for nb in nbrs], CAMS[0], CAMS[1], coarse, ori, only_stereo)


def check(fe, t1, nbrs, coarse=False, ori=False, only_stereo=False, scalar=False):
    m, n = call(fe, t1, nbrs, coarse, ori, only_stereo)
    assert m.shape == (len(nbrs), len(t1.node)) and n.shape == (len(nbrs),)
    for k, nb in enumerate(nbrs):
        want_m, want_n = (search_scalar if scalar else search_closed)(t1, nb, only_stereo, coarse, ori)
        assert np.array_equal(m[k], want_m), "neighbour %d: %d of %d entries differ" % (k, int((m[k] != want_m).sum()), len(want_m))
        assert n[k] == want_n, (k, n[k], want_n)
    return m, n


def cut(t, rows):
    """The table with the given rows (an index array in ascending order), NLeft counted again."""
    rows = np.asarray(rows, np.int64)
    return Table(*[col[rows] for col in t[:7]], int((rows < t.nleft).sum()))


@pytest.mark.parametrize("nkf", [1, 3])
def test_the_constructed_corpus(fe, nkf):
    t1, nbrs, _ = corpus()
    total = 0
    for coarse in (False, True):
        for ori in (False, True):
            total += int(check(fe, t1, nbrs[:nkf], coarse, ori)[1].sum())
    check(fe, t1, nbrs[:nkf], False, True, scalar=True)
    m, n = check(fe, t1, nbrs[:nkf], only_stereo=True)
    assert (m == -1).all() and (n == 0).all() and total > 0


def test_a_node_with_more_than_64_candidates_and_many_ties(fe):
    t1, nbrs, _ = corpus(big=True)
    fv2 = two.feature_vector(nbrs[0].t2.node)
    assert max(len(v) for v in fv2.values()) > 128              # the lanes stride more than twice
    for coarse, ori in ((False, False), (False, True), (True, False)):
        check(fe, t1, nbrs, coarse, ori)
    # every descriptor equal in that neighbour: distance ties everywhere, the last listed candidate that passes the gate wins
    same = nbrs[0]._replace(t2=nbrs[0].t2._replace(desc=np.zeros_like(nbrs[0].t2.desc)))
    one_node = same._replace(t2=same.t2._replace(node=np.where(same.t2.node >= 0, 5, -1).astype(np.int32)))
    t1z = t1._replace(desc=np.zeros_like(t1.desc), node=np.where(t1.node >= 0, 5, -1).astype(np.int32))
    check(fe, t1z, [one_node], True, False)


def test_sizes_sides_and_empty_tables(fe):
    t1, nbrs, _ = corpus()
    n1 = len(t1.node)
    assert n1 % 16 != 0, n1                                     # (a block of the match kernel takes 16 features)
    # features of both cameras of both keyframes in one node: the quads of the corpus
    fv1, fv2 = two.feature_vector(t1.node), two.feature_vector(nbrs[0].t2.node)
    both = [nd for nd in fv1 if nd in fv2 and min(fv1[nd]) < t1.nleft <= max(fv1[nd]) and
            min(fv2[nd]) < nbrs[0].t2.nleft <= max(fv2[nd])]
    assert both
    check(fe, t1, nbrs[:1], False, True)
    # NLeft = 0 and NLeft = N: one camera's features only, on either side
    left1, right1 = cut(t1, np.arange(t1.nleft)), cut(t1, np.arange(t1.nleft, n1))
    assert left1.nleft == len(left1.node) and right1.nleft == 0
    nb = nbrs[0]
    left2 = nb._replace(t2=cut(nb.t2, np.arange(nb.t2.nleft)))
    right2 = nb._replace(t2=cut(nb.t2, np.arange(nb.t2.nleft, len(nb.t2.node))))
    total = 0
    for a in (left1, right1):
        total += int(check(fe, a, [left2, right2, nb], False, True)[1].min())
    assert total > 0
    # neighbours of different sizes, an empty neighbour, one feature
    empty = nb._replace(t2=cut(nb.t2, []))
    m, n = check(fe, t1, [nbrs[1], empty, nbrs[2]._replace(t2=cut(nbrs[2].t2, np.arange(37))), nb._replace(t2=cut(nb.t2, [0]))], False, True)
    assert n[1] == 0 and (m[1] == -1).all()
    # an empty pKF1, and no neighbours
    m, n = check(fe, cut(t1, []), [nb, empty])
    assert m.shape == (2, 0) and (n == 0).all()
    m, n = call(fe, t1, [])
    assert m.shape == (0, n1) and n.shape == (0,)


def test_a_batch_equals_single_calls_and_calls_repeat(fe):
    t1, nbrs, _ = corpus()
    for coarse, ori in ((False, True), (True, True), (False, False)):
        m, n = call(fe, t1, nbrs, coarse, ori)
        for k in range(len(nbrs)):
            m1, c1 = call(fe, t1, nbrs[k:k + 1], coarse, ori)
            assert np.array_equal(m1[0], m[k]) and c1[0] == n[k]
        m2, n2 = call(fe, t1, nbrs, coarse, ori)
        assert m2.tobytes() == m.tobytes() and n2.tobytes() == n.tobytes()
        assert n.sum() > 0


def test_capacity_and_arguments(fe):
    rng = np.random.default_rng(3)
    t1, nbrs, _ = corpus()
    nb = nbrs[0]

    def table(n):
        return Table(rng.uniform(60, 450, n).astype(np.float32), rng.uniform(60, 450, n).astype(np.float32),
                     rng.integers(0, two.NLEVELS, n).astype(np.int32), rng.uniform(0, 359, n).astype(np.float32),
                     rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(-1, 30, n).astype(np.int32), np.zeros(n, np.uint8), n // 2)

    def status(kf1, neighbours, **kw):
        with pytest.raises(capi.PliError) as e:
            call(fe, kf1, neighbours, **kw)
        return e.value.status
    big = table(8193)                                     # PLI_BOW_MAX_FEATURES + 1: refused before anything is launched
    assert status(big, [nb]) == PLI_ERR_CAPACITY
    assert status(t1, [nb, nb._replace(t2=big)]) == PLI_ERR_CAPACITY
    small = table(50)
    put = lambda t, field, value: t._replace(**{field: np.concatenate([getattr(t, field)[:-1], [value]]).astype(getattr(t, field).dtype)})
    for field, value, ori in (("octave", two.NLEVELS, False), ("octave", -1, False), ("angle", 360.0, True), ("angle", -1.0, True),
                              ("node", -2, False), ("x", np.inf, False), ("y", np.nan, False)):
        bad = put(small, field, value)
        assert status(bad, [nb], ori=ori) == PLI_ERR_INVALID, (field, value)
        assert status(small, [nb, nb._replace(t2=bad)], ori=ori) == PLI_ERR_INVALID, (field, value)
    call(fe, put(small, "angle", 400.0), [nb])            # the angles are not checked without the orientation test
    # NLeft outside [0, N] on either side, a relative pose that is not finite
    for nleft in (-1, 51):
        assert status(small._replace(nleft=nleft), [nb]) == PLI_ERR_INVALID
        assert status(small, [nb._replace(t2=small._replace(nleft=nleft))]) == PLI_ERR_INVALID
    for value in (np.nan, np.inf):
        rel = nb.rel.copy()
        rel[3, 11] = value
        assert status(small, [nb, nb._replace(rel=rel)]) == PLI_ERR_INVALID
    # the errors come before the bOnlyStereo shortcut
    assert status(put(small, "octave", 8), [nb], only_stereo=True) == PLI_ERR_INVALID
    # through the C entry point: a decreasing kf_off and null pointers
    from pli_slam_amd.frontend import ptr
    k1, d1, nd1, m1 = keypoints(small), small.desc, small.node, small.has_mp
    off, nl = np.array([0, 50, 40], np.int32), np.array([25, 0], np.int32)
    rel = np.ascontiguousarray(np.stack([nb.rel, nb.rel]), np.float32)
    cl, cr = np.asarray(CAMS[0], np.float32), np.asarray(CAMS[1], np.float32)
    out_m, out_n = np.zeros((2, 50), np.int32), np.zeros(2, np.int32)
    def raw(off=off, cam_left=cl, rel=rel, kp1=k1, nm=out_n):
        return fe.L.pli_search_for_triangulation_two_cameras(fe.h, ptr(kp1) if kp1 is not None else None, ptr(d1), ptr(nd1), ptr(m1), 50, 25, 2,
                                                             ptr(off), ptr(nl), ptr(k1), ptr(d1), ptr(nd1), ptr(m1),
                                                             ptr(cam_left) if cam_left is not None else None, ptr(cr),
                                                             ptr(rel) if rel is not None else None, 0, 0, 0, ptr(out_m),
                                                             ptr(nm) if nm is not None else None)
    assert raw() == PLI_ERR_INVALID
    good = np.array([0, 50, 50], np.int32)
    assert raw(off=good) == 0
    assert raw(off=good, cam_left=None) == PLI_ERR_INVALID and raw(off=good, rel=None) == PLI_ERR_INVALID
    assert raw(off=good, kp1=None) == PLI_ERR_INVALID and raw(off=good, nm=None) == PLI_ERR_INVALID


# ---- extracted tables ---------------------------------------------------------------------------------------------------------

def test_extracted_tables_of_a_synthetic_scene(fe):
    """Four keyframes cut from a synthetic stereo scene (tests/test_triangulation_two_cameras_cpu.py scene_tables) through
    pli_orb_extract and pli_bow_transform.  With bCoarse every row is compared; with the gate on, a row of pKF1 that has an
    undecided candidate is left out, at most 2 % of the rows that have a candidate within TH_LOW."""
    voc = fe.vocab_create(*synth.make_vocabulary(10, 4, seed=0))

    def extract(img):
        n, kp, desc = fe.orb_extract(0, img)
        return kp[:n].copy(), desc[:n].copy()

    def nodes_of(desc):
        _, weight, node = fe.bow_transform(voc, desc, 2)
        return np.where(weight > 0, node, -1)
    t1, nbrs = two.scene_tables(extract, nodes_of)
    fe.vocab_destroy(voc)
    for ori in (False, True):
        check(fe, t1, nbrs, True, ori)
        m, n = call(fe, t1, nbrs, False, ori)
        for k, nb in enumerate(nbrs):
            gate, have, und = two.scene_rows(t1, nb)
            want = search_closed(t1, nb, False, False, False, gate)[0]
            keep = np.ones(len(t1.node), bool)
            keep[sorted(und)] = False
            print("scene neighbour %d ori %d: %d rows with a candidate, %d left out (%.2f %%), %d matches" %
                  (k, ori, len(have), len(und), 100.0 * len(und) / max(len(have), 1), int(n[k])))
            assert len(und) <= 0.02 * len(have) and n[k] > 0
            if not ori:
                assert np.array_equal(m[k][keep], want[keep]), (k, int((m[k][keep] != want[keep]).sum()))
            elif not und:                                  # (the histogram is a sum over every row: exact when none is left out)
                assert np.array_equal(m[k], search_closed(t1, nb, False, False, True, gate)[0]) and \
                    n[k] == search_closed(t1, nb, False, False, True, gate)[1]
