"""pli_create_new_map_points_two_cameras on the MI355X (the product library): LocalMapping::CreateNewMapPoints from the search on
for keyframes of two KannalaBrandt8 cameras, one keyframe against a batch of neighbours, equals the literal loop of
tests/helpers_new_map_points_two_cameras.py byte for byte: matches12, nmatches, status, nnew and the bits of x3d where a point is
created.  The search's gate in that loop is float64 and every pair of the scene that reaches it is decided (the CPU file asserts
it); the geometry is the float32 restatement.  One scene of 10 neighbours serves every case: the loop is sequential, so its results
for the first nkf neighbours are those of a call with nkf neighbours."""
import numpy as np
import pytest

from pli_slam_amd import capi
import helpers_new_map_points_two_cameras as h
import test_triangulation_two_cameras_cpu as two
from helpers_new_map_points import CODE, CREATED, NOT_MATCHED, STATUS, TAKEN_EARLIER
from test_triangulation_two_cameras_cpu import CAMS, Table
from test_triangulation_two_cameras_gpu import cut, keypoints

pytestmark = pytest.mark.gpu
PLI_ERR_INVALID, PLI_ERR_CAPACITY = -1, -3
SEED = h.SEEDS[0]
_WANT = {}


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(two.scene_config(), dev=False)
    yield f
    f.close()


def kf_of(kf):
    return keypoints(kf.t), kf.t.desc, kf.t.node, kf.t.has_mp, kf.t.nleft, kf.pose


def nb_of(nb):
    return kf_of(nb.kf) + (nb.rel,)


def call(fe, kf1, nbrs, coarse=False, far=False, th_far=h.TH_FAR):
    return fe.create_new_map_points_two_cameras(kf_of(kf1), [nb_of(nb) for nb in nbrs], CAMS[0], CAMS[1], h.RATIO_FACTOR, coarse, far,
                                                th_far)


def want(po, coarse, far):
    """The literal loop on the scene of 10 neighbours, computed once per setting."""
    if (coarse, far) not in _WANT:
        kf1, nbrs, _ = h.scene(SEED)
        _WANT[(coarse, far)] = h.create_new_map_points(po, kf1, nbrs, coarse, far, h.TH_FAR)
    return _WANT[(coarse, far)]


def equal(got, exp, what=""):
    names = ("matches12", "nmatches", "status", "x3d", "nnew")
    for name, g, e in zip(names, got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape)
        if name == "x3d":
            made = exp[2] == CREATED
            assert g[made].tobytes() == e[made].tobytes(), (what, name, int((g[made] != e[made]).any(-1).sum()))
        else:
            assert g.tobytes() == e.tobytes(), (what, name, int((g != e).sum()), [(STATUS[a], STATUS[b]) for a, b in
                                                                              zip(g[g != e][:5], e[g != e][:5])] if name == "status" else "")


@pytest.mark.parametrize("nkf", [1, 3, 10])
def test_the_device_equals_the_literal_loop(fe, oracle, nkf):
    kf1, nbrs, _ = h.scene(SEED)
    seen = set()
    for coarse in (False, True):
        for far in (False, True):
            exp = tuple(a[:nkf] for a in want(oracle, coarse, far))
            got = call(fe, kf1, nbrs[:nkf], coarse, far)
            equal(got, exp, (nkf, coarse, far))
            seen.update(STATUS[s] for s in np.unique(got[2]))
            assert got[4].sum() > 0 and (got[1] >= got[4]).all()
    if nkf == 10:
        missing = set(h.REACHABLE) - seen - {"w_zero", "dist_zero"}
        assert not missing, missing
        assert int((want(oracle, False, False)[0] >= 0).sum()) > 64            # more than one block of the geometry kernel


def test_the_constructed_exits_come_back_from_the_device(fe, oracle):
    kf1, nbrs = h.w_zero_scene()                                   # also: a call with exactly one matched pair
    got = call(fe, kf1, nbrs, coarse=True)
    equal(got, h.create_new_map_points(oracle, kf1, nbrs, coarse=True), "w_zero")
    assert got[2][0, 0] == CODE["w_zero"] and got[1][0] == 1 and got[4][0] == 0
    kf1, nbrs, _ = h.scene(SEED)
    changed, (k, i) = h.dist_zero_scene(kf1, nbrs, want(oracle, False, False))
    got = call(fe, kf1, changed[:k + 1])
    equal(got, h.create_new_map_points(oracle, kf1, changed[:k + 1]), "dist_zero")
    assert got[2][k, i] == CODE["dist_zero"]
    a, b = h.gate_599_scene(oracle)                                 # between 5.99 and 5.991 sigma2: created
    got = call(fe, a, b)
    equal(got, h.create_new_map_points(oracle, a, b), "gate_599")
    assert got[2][0, 0] == CREATED and got[4][0] == 1


def test_sides_and_empty_tables(fe, oracle):
    kf1, nbrs, _ = h.scene(SEED)
    t1, n1 = kf1.t, len(kf1.t.node)
    left1 = kf1._replace(t=cut(t1, np.arange(t1.nleft)))            # n1_left == n1
    right1 = kf1._replace(t=cut(t1, np.arange(t1.nleft, n1)))       # n1_left == 0
    assert left1.t.nleft == len(left1.t.node) and right1.t.nleft == 0
    nb = nbrs[0]
    t2 = nb.kf.t
    right2 = nb._replace(kf=nb.kf._replace(t=cut(t2, np.arange(t2.nleft, len(t2.node)))))      # kf_nleft == 0
    empty = nb._replace(kf=nb.kf._replace(t=cut(t2, [])))
    for a in (left1, right1):
        lst = [right2, empty, nbrs[1]]
        got = call(fe, a, lst, far=True)
        equal(got, h.create_new_map_points(oracle, a, lst, False, True, h.TH_FAR), "sides")
        assert got[1][1] == 0 and (got[0][1] == -1).all() and (got[2][1] == NOT_MATCHED).all() and got[4].sum() > 0
    # an empty pKF1, and no neighbours
    got = call(fe, kf1._replace(t=cut(t1, [])), [nb, empty])
    assert got[0].shape == (2, 0) and got[3].shape == (2, 0, 3) and not got[1].any() and not got[4].any()
    got = call(fe, kf1, [])
    assert got[0].shape == (0, n1) and got[1].shape == (0,) and got[4].shape == (0,)


def test_a_batch_equals_single_calls_chained_through_has_mp_and_calls_repeat(fe):
    kf1, nbrs, _ = h.scene(SEED)
    nbrs = nbrs[:4]
    batch = call(fe, kf1, nbrs, far=True)
    has = kf1.t.has_mp.copy()
    for k, nb in enumerate(nbrs):
        one = call(fe, kf1._replace(t=kf1.t._replace(has_mp=has)), [nb], far=True)
        # (a single call cannot know that an earlier call took a feature: its label is "not matched")
        st = np.where(batch[2][k] == TAKEN_EARLIER, NOT_MATCHED, batch[2][k])
        assert np.array_equal(one[0][0], batch[0][k]) and np.array_equal(one[2][0], st)
        made = st == CREATED
        assert one[3][0][made].tobytes() == batch[3][k][made].tobytes() and one[1][0] == batch[1][k] and one[4][0] == batch[4][k]
        has = has | (one[2][0] == CREATED).astype(np.uint8)
    again = call(fe, kf1, nbrs, far=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, again))            # (x3d too, also where it is not defined)
    assert (batch[2] == TAKEN_EARLIER).any()


def test_the_matches_before_the_pick_are_the_search_alone(fe):
    kf1, nbrs, _ = h.scene(SEED)
    nbrs = nbrs[:3]
    for coarse in (False, True):
        m, _, status, _, _ = call(fe, kf1, nbrs, coarse)
        s, _ = fe.search_for_triangulation_two_cameras(kf_of(kf1)[:5], [kf_of(nb.kf)[:5] + (nb.rel,) for nb in nbrs], CAMS[0], CAMS[1],
                                                       coarse, False, False)
        taken = status == TAKEN_EARLIER
        assert np.array_equal(m[~taken], s[~taken]) and (m[taken] == -1).all() and (s[taken] >= 0).all()


def test_capacity_and_arguments(fe):
    rng = np.random.default_rng(3)
    kf1, nbrs, _ = h.scene(SEED)
    nb = nbrs[0]

    def table(n):
        return Table(rng.uniform(60, 450, n).astype(np.float32), rng.uniform(60, 450, n).astype(np.float32),
                     rng.integers(0, two.NLEVELS, n).astype(np.int32), rng.uniform(0, 359, n).astype(np.float32),
                     rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(-1, 30, n).astype(np.int32), np.zeros(n, np.uint8), n // 2)

    def status(a, neighbours):
        with pytest.raises(capi.PliError) as e:
            call(fe, a, neighbours)
        return e.value.status
    with_t = lambda kf, t: kf._replace(t=t)
    big = with_t(kf1, table(8193))                        # PLI_BOW_MAX_FEATURES + 1: refused before anything is launched
    assert status(big, [nb]) == PLI_ERR_CAPACITY
    assert status(kf1, [nb, nb._replace(kf=big)]) == PLI_ERR_CAPACITY
    small = table(50)
    put = lambda t, field, value: t._replace(**{field: np.concatenate([getattr(t, field)[:-1], [value]]).astype(getattr(t, field).dtype)})
    for field, value in (("octave", two.NLEVELS), ("octave", -1), ("node", -2), ("x", np.inf), ("y", np.nan)):
        bad = put(small, field, value)
        assert status(with_t(kf1, bad), [nb]) == PLI_ERR_INVALID, (field, value)
        assert status(with_t(kf1, small), [nb, nb._replace(kf=with_t(nb.kf, bad))]) == PLI_ERR_INVALID, (field, value)
    call(fe, with_t(kf1, put(small, "angle", 400.0)), [nb])           # (no orientation check: the angles are not read)
    for nleft in (-1, 51):
        assert status(with_t(kf1, small._replace(nleft=nleft)), [nb]) == PLI_ERR_INVALID
        assert status(with_t(kf1, small), [nb._replace(kf=with_t(nb.kf, small._replace(nleft=nleft)))]) == PLI_ERR_INVALID
    for value in (np.nan, np.inf):
        rel = nb.rel.copy()
        rel[3, 11] = value
        assert status(with_t(kf1, small), [nb, nb._replace(rel=rel)]) == PLI_ERR_INVALID
        pose = kf1.pose.copy()
        pose[1, 14] = value
        assert status(kf1._replace(t=small, pose=pose), [nb]) == PLI_ERR_INVALID
        assert status(with_t(kf1, small), [nb._replace(kf=nb.kf._replace(pose=pose))]) == PLI_ERR_INVALID
    # through the C entry point: a decreasing kf_off, the pair-index cap and null pointers
    from pli_slam_amd.frontend import ptr
    k1, d1, nd1, m1 = keypoints(small), small.desc, small.node, small.has_mp
    off, nl = np.array([0, 50, 40], np.int32), np.array([25, 0], np.int32)
    rel = np.ascontiguousarray(np.stack([nb.rel, nb.rel]), np.float32)
    p1, p2 = np.ascontiguousarray(kf1.pose, np.float32), np.ascontiguousarray(np.stack([nb.kf.pose, nb.kf.pose]), np.float32)
    cl, cr = np.asarray(CAMS[0], np.float32), np.asarray(CAMS[1], np.float32)
    out_m, out_n, out_s, out_x, out_c = (np.zeros((2, 50), np.int32), np.zeros(2, np.int32), np.zeros((2, 50), np.int32),
                                         np.zeros((2, 50, 3), np.float32), np.zeros(2, np.int32))
    opt = lambda a: ptr(a) if a is not None else None

    def raw(off=off, cam_left=cl, rel=rel, kp1=k1, pose1=p1, kf_pose=p2, st=out_s, nnew=out_c, nkf=2, n1=50):
        return fe.L.pli_create_new_map_points_two_cameras(fe.h, opt(kp1), ptr(d1), ptr(nd1), ptr(m1), n1, 25, nkf, ptr(off), ptr(nl), ptr(k1),
                                                          ptr(d1), ptr(nd1), ptr(m1), opt(cam_left), ptr(cr), opt(rel), opt(pose1),
                                                          opt(kf_pose), 0, 0, 0.0, float(h.RATIO_FACTOR), ptr(out_m), ptr(out_n),
                                                          opt(st), ptr(out_x), opt(nnew))
    assert raw() == PLI_ERR_INVALID
    good = np.array([0, 50, 50], np.int32)
    assert raw(off=good) == 0
    for name in ("cam_left", "rel", "kp1", "pose1", "kf_pose", "st", "nnew"):
        assert raw(off=good, **{name: None}) == PLI_ERR_INVALID, name
    # nkf x n1 beyond the pair index: 300000 empty neighbours x 8192 rows (nothing is read past the counts: refused first)
    many = 300000
    offs, nls = np.zeros(many + 1, np.int32), np.zeros(many, np.int32)
    bigt = table(8192)
    kb = keypoints(bigt)
    r = fe.L.pli_create_new_map_points_two_cameras(fe.h, ptr(kb), ptr(bigt.desc), ptr(bigt.node), ptr(bigt.has_mp), 8192, 4096, many,
                                                   ptr(offs), ptr(nls), None, None, None, None, ptr(cl), ptr(cr), ptr(rel), ptr(p1),
                                                   ptr(p2), 0, 0, 0.0, float(h.RATIO_FACTOR), ptr(out_m), ptr(out_n), ptr(out_s),
                                                   ptr(out_x), ptr(out_c))
    assert r == PLI_ERR_CAPACITY
