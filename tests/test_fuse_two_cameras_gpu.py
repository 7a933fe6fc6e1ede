"""pli_fuse_search_two_cameras on the MI355X (the product library): the search half of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight)
(ORBmatcher.cc:1399-1609) for keyframes with two KannalaBrandt8 cameras, both values of bRight of a batch of keyframes in one call,
equals the Python restatements of tests/test_fuse_two_cameras_cpu.py exactly (best_idx and best_dist).  That file shows, on the
CPU, that the corpus takes every exit of the reference's loop on both sides, produces matches, and that every decision of it lies
outside the margin within which the last bit of the fisheye projection could decide; the cases built here are settled by the same
rule (test_fuse_two_cameras_cpu.settle) before the device sees them."""
import numpy as np
import pytest

from pli_slam_amd import capi
from test_fuse_search_cpu import NLEVELS, level_ratio
from test_fuse_two_cameras_cpu import (BOUNDS, CAMS, KF2, MATCHES, P0, corpus, examine, fuse2_batch, fuse2_case, fuse2_fast,
                                       fuse2_scalar, kf_pose, settle)

pytestmark = pytest.mark.gpu
W = H = 512
BOUNDS4 = (BOUNDS.min_x, BOUNDS.max_x, BOUNDS.min_y, BOUNDS.max_y)


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=False)
    assert f.cfg.orb_nlevels == NLEVELS
    yield f
    f.close()


def dev_kf(kf):
    kp = np.zeros(len(kf.x), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = kf.x, kf.y, kf.octave
    kp["size"] = 31.0
    return kp, kf.desc, kf.nleft, kf.pose


def search(fe, pts, descs, kfs, th=3.0, sides=3, skip=None, **kw):
    return fe.fuse_search_two_cameras(pts, descs, [dev_kf(k) for k in kfs], CAMS[0], CAMS[1], BOUNDS4, th, sides, skip,
                                      level_ratio=level_ratio(), **kw)


def check(fe, pts, descs, kfs, th=3.0, sides=3, skip=None, scalar=False):
    bi, bd = search(fe, pts, descs, kfs, th, sides, skip)
    assert bi.shape == (len(kfs), 2, len(pts)) and bd.shape == bi.shape
    wi, wd = fuse2_batch(pts, descs, kfs, th, sides, skip, fuse2_scalar if scalar else fuse2_fast)
    assert np.array_equal(bi, wi), "%d of %d best_idx differ" % (int((bi != wi).sum()), bi.size)
    assert np.array_equal(bd, wd), "%d of %d best_dist differ" % (int((bd != wd).sum()), bd.size)
    for side in (0, 1):
        if not (sides >> side) & 1:                                  # a side that is not asked for: -1 / 256
            assert (bi[:, side] == -1).all() and (bd[:, side] == 256).all()
    return bi, bd


@pytest.mark.parametrize("nkf", [0, 1, 3])
def test_the_corpus(fe, nkf):
    C = corpus(nkf)
    for th in (3.0, 4.0):
        for sk in (None, C.skip):
            got = {}
            for sides in (1, 2, 3):
                bi, _ = check(fe, C.pts, C.descs, C.kfs, th, sides, sk)
                got[sides] = bi
            assert np.array_equal(got[3][:, 0], got[1][:, 0]) and np.array_equal(got[3][:, 1], got[2][:, 1])
            if nkf and sk is None:                                   # floor: half the restatement's own count (asserted on the CPU)
                assert (got[3] >= 0).sum() >= MATCHES[(nkf, th)] / 2
    if nkf:
        check(fe, C.pts, C.descs, C.kfs[:1], 3.0, 3, C.skip[:1], scalar=True)     # the reference's control flow on one keyframe
    else:
        assert search(fe, C.pts, C.descs, [])[0].shape == (0, 2, len(C.pts))


def only_side(kf, right):
    """The keyframe with the rows of one camera alone: NRight == 0, or NLeft == 0."""
    lo, hi = (kf.nleft, len(kf.x)) if right else (0, kf.nleft)
    return KF2(kf.x[lo:hi], kf.y[lo:hi], kf.octave[lo:hi], kf.desc[lo:hi], 0 if right else hi - lo, kf.pose)


def test_a_keyframe_without_right_rows_and_one_without_left_rows(fe):
    C = corpus(3)
    empty = KF2(C.kfs[0].x[:0], C.kfs[0].y[:0], C.kfs[0].octave[:0], C.kfs[0].desc[:0], 0, C.kfs[0].pose)
    kfs = [only_side(C.kfs[0], False), C.kfs[1], only_side(C.kfs[2], True), empty, only_side(C.kfs[1], True)]
    skip = np.concatenate([C.skip, C.skip[:2]])
    bi, bd = check(fe, C.pts, C.descs, kfs, 3.0, 3, skip)
    assert (bi[0, 1] == -1).all() and (bd[0, 1] == 256).all() and (bi[0, 0] >= 0).sum() > 0          # NRight == 0
    assert (bi[2, 0] == -1).all() and (bd[2, 0] == 256).all() and (bi[2, 1] >= 0).sum() > 0          # NLeft == 0: rows + 0
    assert (bi[3] == -1).all() and (bi[4, 1] >= 0).sum() > 0
    # the winners of the cut keyframe are the whole keyframe's, counted from the cut table's first row
    whole, _ = check(fe, C.pts, C.descs, C.kfs, 3.0, 3, C.skip)
    assert np.array_equal(bi[0, 0], whole[0, 0])
    assert np.array_equal(bi[2, 1], np.where(whole[2, 1] >= 0, whole[2, 1] - C.kfs[2].nleft, -1))
    bi, _ = check(fe, C.pts[:0], C.descs[:0], kfs)                   # no points
    assert bi.shape == (5, 2, 0)


_CROWDED = {}


def crowded():
    """More candidates in a window than the widest lane group holds: 30 copies of every keypoint of a keyframe within +-2.5 px,
    windows of a hundred candidates that straddle cell borders; settled like the corpus (a point with an undecided pair is drawn
    again)."""
    if "c" not in _CROWDED:
        rng = np.random.default_rng(8)
        C = fuse2_case(81, 1, nmp=300, noise=0.3)
        kf, rep, parts = C.kfs[0], 30, []
        for lo, hi in ((0, kf.nleft), (kf.nleft, len(kf.x))):
            m = (hi - lo) * rep
            parts.append(((np.repeat(kf.x[lo:hi], rep) + rng.uniform(-2.5, 2.5, m)).astype(np.float32),
                          (np.repeat(kf.y[lo:hi], rep) + rng.uniform(-2.5, 2.5, m)).astype(np.float32),
                          np.repeat(kf.octave[lo:hi], rep), np.repeat(kf.desc[lo:hi], rep, axis=0)))
        nl = 4100                                                    # 8192 rows: exactly at the cap
        cut = [tuple(c[:n] for c in p) for p, n in zip(parts, (nl, 8192 - nl))]
        big = KF2(*[np.concatenate([cut[0][j], cut[1][j]]) for j in range(4)], nl, kf.pose)
        pts = C.pts.copy()
        settle(rng, pts, [big, kf], ths=(3.0,))
        _CROWDED["c"] = (pts, C.descs, [big, kf])
    return _CROWDED["c"]


def test_crowded_windows(fe):
    pts, descs, kfs = crowded()
    info = {}
    fuse2_fast(pts, descs, kfs[0], True, 3.0, info=info)
    assert info["window_rows"].max() > 64
    bi, _ = check(fe, pts, descs, kfs, 3.0)
    assert (bi[0] >= 0).sum() > 40
    check(fe, pts[:40], descs[:40], kfs[:1], 3.0, scalar=True)


def test_all_descriptors_equal_the_visiting_order_decides_every_winner(fe):
    pts, descs, kfs = crowded()
    same = [k._replace(desc=np.zeros_like(k.desc)) for k in kfs]
    bi, bd = check(fe, pts, np.zeros_like(descs), same, 3.0)
    assert (bi[:, 0] >= 0).sum() > 40 and (bi[:, 1] >= 0).sum() > 40 and (bd[bi >= 0] == 0).all()
    check(fe, pts[:40], np.zeros_like(descs[:40]), same[:1], 3.0, scalar=True)


def test_one_keyframe_five_thousand_points(fe):
    """The shape of LocalMapping.cc:776-777: every neighbour's map points against the current keyframe, both cameras."""
    C = fuse2_case(77, 1, nmp=5000, nfeat=(700, 500))
    bi, _ = check(fe, C.pts, C.descs, C.kfs, 3.0, 3, C.skip)
    want = int((fuse2_batch(C.pts, C.descs, C.kfs, 3.0, 3, C.skip)[0] >= 0).sum())
    assert want > 100 and (bi >= 0).sum() >= want / 2
    assert not examine(C.pts, C.kfs, 3.0, C.skip)[1]


def launches(fe, call):
    fe.prof_enable(True)
    fe.prof_reset()
    try:
        call()
    finally:
        rep = fe.prof_report()
        fe.prof_enable(False)
    return sum(calls for calls, _ in rep.values())


def test_three_launches_whatever_the_batch(fe):
    for nkf in (1, 3):
        C = corpus(nkf)
        assert launches(fe, lambda: search(fe, C.pts, C.descs, C.kfs)) == 3


def test_capacity_and_arguments_nothing_is_launched(fe):
    rng = np.random.default_rng(3)
    C = corpus(1)

    def table(n, nleft):
        return KF2(rng.uniform(0, W, n).astype(np.float32), rng.uniform(0, H, n).astype(np.float32),
                   rng.integers(0, NLEVELS, n).astype(np.int32), rng.integers(0, 256, (n, 32), dtype=np.uint8), nleft, kf_pose(P0))
    small, big = table(50, 20), table(8193, 4000)                    # PLI_BOW_MAX_FEATURES + 1

    def refused(status, kfs, **kw):
        def call():
            with pytest.raises(capi.PliError) as e:
                search(fe, C.pts, C.descs, kfs, **kw)
            assert e.value.status == status
        assert launches(fe, call) == 0

    refused(-3, [small, big])                                        # PLI_ERR_CAPACITY
    for nleft in (-1, 51):
        refused(-1, [small, small._replace(nleft=nleft)])            # PLI_ERR_INVALID: kf_nleft outside the keyframe
    for sides in (0, 4, -1):
        refused(-1, [small], sides=sides)
    pose = small.pose.copy()
    pose[1, 10] = np.nan
    refused(-1, [small, small._replace(pose=pose)])
    pose = small.pose.copy()
    pose[0, 3] = np.inf
    refused(-1, [small._replace(pose=pose)])
    bad = small.x.copy()
    bad[7] = np.nan
    refused(-1, [small._replace(x=bad)])                             # a keypoint coordinate that is not finite
    octave = small.octave.copy()
    octave[3] = NLEVELS
    refused(-1, [small._replace(octave=octave)])
    assert launches(fe, lambda: search(fe, C.pts, C.descs, [small, table(8192, 8192)])) == 3        # exactly at the cap
    # raw calls: kf_off decreasing, null pointers
    L, h, ptr = fe.L, fe.h, capi.ptr
    kp, kd, nl = dev_kf(small)[0], np.ascontiguousarray(small.desc), np.array([10, 10], np.int32)
    pose2 = np.stack([small.pose, small.pose])
    cl, cr = np.array(CAMS[0], np.float32), np.array(CAMS[1], np.float32)
    out = np.zeros((2, 2, len(C.pts)), np.int32)
    lr = level_ratio()

    def raw(off, mp=C.pts, md=C.descs, kkp=kp, knl=nl, po=pose2, camr=cr, lvr=lr, bi=out, max_x=512.0):
        off = np.array(off, np.int32)
        return L.pli_fuse_search_two_cameras(h, ptr(mp), ptr(md), len(C.pts), 2, ptr(off), ptr(knl), ptr(kkp), ptr(kd), ptr(po), None,
                                             ptr(cl), ptr(camr), 0.0, max_x, 0.0, 512.0, 3.0, ptr(lvr), 3, ptr(bi), None)
    assert raw([0, 20, 50]) == 0
    assert raw([0, 30, 20]) == -1 and raw([1, 20, 50]) == -1 and raw([0, 20, 50], max_x=0.0) == -1
    for kw in (dict(mp=None), dict(md=None), dict(kkp=None), dict(knl=None), dict(po=None), dict(camr=None), dict(lvr=None),
               dict(bi=None)):
        assert raw([0, 20, 50], **kw) == -1, kw
