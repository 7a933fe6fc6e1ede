"""pli_search_by_projection_sim3 on the MI355X (the product library): loop closing's ORBmatcher::SearchByProjection(pKF, Scw, ...)
(ORBmatcher.cc:473-704) for one list of map points against a batch of (keyframe, Scw) pairs equals the Python restatements of
tests/test_sim3_projection_cpu.py exactly (row_point, best_idx and nmatches).  That file shows, on the CPU, that the constructed
scenes take every exit of the reference's loop and produce matches, so the equalities here are not vacuous."""
import numpy as np
import pytest

from pli_slam_amd import capi, realdata, synth
from test_fuse_search_cpu import CAM, IDENTITY, KF, NLEVELS, level_ratio, make_keyframe, make_points, make_pose, rot_xyz
from test_fuse_search_gpu import keypoints, real_case
from test_sim3_projection_cpu import (boundary_case, contention_cases, reversal_case, sim3_case, sim3_search_batch, sim3_search_fast,
                                      sim3_search_scalar)

pytestmark = pytest.mark.gpu
W, H = 752, 480


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


def dev_pair(kf, occupied=None):
    return keypoints(kf), kf.desc, kf.pose, occupied


def check(fe, pts, descs, kfs, th=3.0, ratio=1.0, form=0, skip=None, occupied=None, scalar=False, cam=CAM):
    pairs = [dev_pair(kf, None if occupied is None else occupied[k]) for k, kf in enumerate(kfs)]
    rows, bi, nm = fe.search_by_projection_sim3(pts, descs, pairs, cam, th, ratio, form, skip, level_ratio=level_ratio())
    assert bi.shape == (len(kfs), len(pts)) and nm.shape == (len(kfs),) and len(rows) == len(kfs)
    wr, wi, wn = sim3_search_batch(pts, descs, kfs, cam, th, ratio, form, skip, occupied,
                                   sim3_search_scalar if scalar else sim3_search_fast)
    assert np.array_equal(bi, wi), "%d of %d best_idx differ" % (int((bi != wi).sum()), bi.size)
    for k in range(len(kfs)):
        assert np.array_equal(rows[k], wr[k]), "pair %d: %d row_point differ" % (k, int((rows[k] != wr[k]).sum()))
    assert np.array_equal(nm, wn)
    return rows, bi, nm


@pytest.mark.parametrize("npair", [0, 1, 3, 6])
def test_constructed_scenes(fe, npair):
    """500 points (a quarter listed twice) against npair poses with 400 features each, a tenth of the rows occupied at entry and
    a tenth of the points skipped: both projection forms, th in {3, 5, 8}, ratio in {1.0, 1.5}."""
    pts, descs, kfs, skip, occ = sim3_case(np.random.default_rng(300 + npair), npair, 500)
    total = 0
    for form in (0, 1):
        for th in (3.0, 5.0, 8.0):
            for ratio in (1.0, 1.5):
                total += int(check(fe, pts, descs, kfs, th, ratio, form, skip, occ)[2].sum())
    print("npair %d: %d matches over the twelve settings" % (npair, total))
    if npair:
        check(fe, pts, descs, kfs[:1], 5.0, 1.5, 1, skip[:1], occ[:1], scalar=True)        # the reference's control flow
        check(fe, pts, descs, kfs, 8.0, 1.0, 0)                                          # no skip table, nothing occupied
        assert total > 12 * 60 * npair
    else:
        assert total == 0


def test_hand_worked_cases(fe):
    for name, (pts, descs, kf, kw, rows, best) in contention_cases().items():
        for form in (0, 1):
            occ = None if "occupied" not in kw else [kw["occupied"]]
            skip = None if "skip" not in kw else kw["skip"][None]
            r, b, n = check(fe, pts, descs, [kf], form=form, skip=skip, occupied=occ, scalar=True)
            assert (r[0].tolist(), b[0].tolist()) == (rows, best), (name, form)
    pts, descs, kf = reversal_case()
    assert check(fe, pts, descs, [kf])[0][0].tolist() == [0, 1, 2]
    assert check(fe, pts[::-1].copy(), descs[::-1].copy(), [kf])[0][0].tolist() == [1, 0, 2]


def test_thresholds(fe):
    from test_fuse_search_cpu import flip_bits, kf_of, point_at_pixel
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    P = point_at_pixel(300.0, 200.0)
    for ratio, inside, outside in ((1.0, (49, 50), (51,)), (1.5, (74, 75), (76,)), (1.01, (50,), (51,))):
        for nbits in inside + outside:
            _, b, n = check(fe, P, d[None], [kf_of([300], [200], [flip_bits(rng, d, nbits)])], ratio=ratio, scalar=True)
            assert b[0].tolist() == [0 if nbits in inside else -1] and n[0] == (nbits in inside), (ratio, nbits)


def test_the_projection_form_decides_a_keypoint_at_the_window_edge(fe):
    P, d, kf, (want0, want1) = boundary_case()
    assert want0 != want1
    assert check(fe, P, d, [kf], form=0, scalar=True)[1][0].tolist() == [want0]
    assert check(fe, P, d, [kf], form=1, scalar=True)[1][0].tolist() == [want1]


def test_heavy_contention(fe):
    """300 points projected onto about 30 spots and every descriptor equal: the point order and the key decide every row."""
    rng = np.random.default_rng(12)
    spots, _ = make_points(rng, 30)
    spots["valid"] = 1
    pts = spots[rng.integers(0, 30, 300)]
    descs = np.zeros((300, 32), np.uint8)
    pose = make_pose(rot_xyz(0.01, -0.01, 0.02), [0.1, -0.05, 0.1])
    kf = make_keyframe(rng, spots, np.zeros((30, 32), np.uint8), pose, 30, noise=0.3)
    rep = 12                                                             # 12 keypoints within +-2.5 px of every spot
    x = (np.repeat(kf.x, rep) + rng.uniform(-2.5, 2.5, len(kf.x) * rep)).astype(np.float32)
    y = (np.repeat(kf.y, rep) + rng.uniform(-2.5, 2.5, len(kf.x) * rep)).astype(np.float32)
    crowd = KF(x, y, np.repeat(kf.octave, rep), np.zeros((len(x), 32), np.uint8), np.repeat(kf.uright, rep), pose)
    for form, th in ((0, 3.0), (1, 5.0)):
        _, bi, nm = check(fe, pts, descs, [crowd], th, 1.0, form)
        assert nm[0] > 60
    # the reference's control flow, and the reversed list (another assignment)
    _, fwd, _ = check(fe, pts, descs, [crowd], 3.0, 1.0, 0, scalar=True)
    _, rev, _ = check(fe, pts[::-1].copy(), descs, [crowd], 3.0, 1.0, 0)
    assert not np.array_equal(fwd[0], rev[0][::-1])


def test_windows_with_more_candidates_than_the_list(fe):
    """Crowded copies (40 keypoints within +-2.5 px of each of 10 keypoints, the descriptor copied too) and 500 points on 30
    spots: windows of 40 to 100 candidates within the limit, above the candidate list's width, so the ordered phase walks those
    windows itself, a dozen points per spot taking one row after the other."""
    rng = np.random.default_rng(8)
    spots, sdesc = make_points(rng, 30)
    spots["valid"] = 1
    pose = make_pose(rot_xyz(0.01, 0.01, -0.01), [0.1, 0.05, -0.1])
    kf = make_keyframe(rng, spots, sdesc, pose, 10, noise=0.3)
    rep = 40
    x = (np.repeat(kf.x, rep) + rng.uniform(-2.5, 2.5, len(kf.x) * rep)).astype(np.float32)
    y = (np.repeat(kf.y, rep) + rng.uniform(-2.5, 2.5, len(kf.x) * rep)).astype(np.float32)
    crowded = KF(x, y, np.repeat(kf.octave, rep), np.repeat(kf.desc, rep, axis=0), np.repeat(kf.uright, rep), pose)
    assert len(crowded.x) == 400
    pick = rng.integers(0, 30, 500)
    pts, descs = spots[pick], sdesc[pick]
    for form, th, ratio in ((0, 3.0, 1.0), (1, 8.0, 1.5)):
        _, bi, nm = check(fe, pts, descs, [crowded, kf], th, ratio, form)
        assert nm[0] > 30
    same = crowded._replace(desc=np.zeros_like(crowded.desc))
    _, bi, nm = check(fe, pts, np.zeros_like(descs), [same], 8.0, 1.0, 0)
    assert nm[0] > 60
    check(fe, pts[:120], np.zeros_like(descs[:120]), [same], 5.0, 1.0, 1, scalar=True)


def test_the_same_keyframe_twice_in_one_batch(fe):
    """Different Scw and different occupied rows for the same keyframe: the pairs do not share owner state."""
    rng = np.random.default_rng(13)
    pts, descs, kfs, skip, occ = sim3_case(rng, 1, 400)
    # the second pair: the same rows seen through a slightly different Scw, other rows occupied
    R = rot_xyz(0.0005, -0.0004, 0.0003) @ kfs[0].pose[:9].reshape(3, 3).astype(np.float64)
    other = kfs[0]._replace(pose=make_pose(R, kfs[0].pose[9:12] + np.float32(0.002)))
    occ2 = (rng.random(len(other.x)) < 0.3).astype(np.uint8)
    batch = [kfs[0], other, kfs[0]]
    occs = [occ[0], occ2, None]
    sk = np.concatenate([skip, skip, np.zeros_like(skip)])
    rows, bi, nm = check(fe, pts, descs, batch, 5.0, 1.5, 0, sk, occs)
    for k in range(3):
        r1, b1, n1 = fe.search_by_projection_sim3(pts, descs, [dev_pair(batch[k], occs[k])], CAM, 5.0, 1.5, 0, sk[k:k + 1],
                                                  level_ratio=level_ratio())
        assert np.array_equal(r1[0], rows[k]) and np.array_equal(b1[0], bi[k]) and n1[0] == nm[k]
    assert nm.min() > 30 and not np.array_equal(bi[0], bi[1]) and not np.array_equal(bi[0], bi[2])
    for _ in range(2):                                                   # calls repeat
        r2, b2, n2 = fe.search_by_projection_sim3(pts, descs, [dev_pair(b, o) for b, o in zip(batch, occs)], CAM, 5.0, 1.5, 0, sk,
                                                  level_ratio=level_ratio())
        assert np.array_equal(b2, bi) and np.array_equal(n2, nm)


def test_real_orb_tables(fe):
    cam = CAM._replace(fx=np.float32(fe.cfg.fx), fy=np.float32(fe.cfg.fx), bf=np.float32(fe.cfg.bf))
    total = 0
    frames = realdata.frames_752x480(2, seed=4)
    for pair in ([synth.make_stereo_pair(3, W, H, t=0), synth.make_stereo_pair(3, W, H, t=1)], [frames[0], frames[1]]):
        pts, descs, kfs = real_case(fe, pair, cam)
        pts, descs = pts[:500], descs[:500]
        kfs = [KF(k.x[:400], k.y[:400], k.octave[:400], k.desc[:400], k.uright[:400], k.pose) for k in kfs]
        for form, th, ratio in ((0, 3.0, 1.0), (1, 8.0, 1.5)):
            total += int(check(fe, pts, descs, kfs, th, ratio, form, cam=cam)[2].sum())
    print("real ORB tables: %d matches" % total)
    assert total > 100, total


def test_capacity_arguments_and_empty_sides(fe):
    rng = np.random.default_rng(3)
    cap = 8192                                            # PLI_BOW_MAX_FEATURES
    pts, descs = make_points(rng, 200)

    def table(n):
        return KF(rng.uniform(0, W, n).astype(np.float32), rng.uniform(0, H, n).astype(np.float32),
                  rng.integers(0, NLEVELS, n).astype(np.int32), rng.integers(0, 256, (n, 32), dtype=np.uint8),
                  np.full(n, -1, np.float32), IDENTITY)
    small, big, full, empty = table(50), table(cap + 1), table(cap), table(0)
    with pytest.raises(capi.PliError) as e:
        fe.search_by_projection_sim3(pts, descs, [dev_pair(small), dev_pair(big)], CAM)
    assert e.value.status == -3                     # PLI_ERR_CAPACITY
    occ = (rng.random(cap) < 0.5).astype(np.uint8)
    check(fe, pts, descs, [full, small], 8.0, 1.5, 0, occupied=[occ, None])      # exactly at the cap
    for ratio in (5.2, 0.0, -1.0, float("nan"), float("inf"), 5.12):              # 50 * 5.12 = 256
        with pytest.raises(capi.PliError) as e:
            fe.search_by_projection_sim3(pts, descs, [dev_pair(small)], CAM, 3.0, ratio)
        assert e.value.status == -1, ratio          # PLI_ERR_INVALID
    check(fe, pts, descs, [small], 3.0, 5.1)        # 255: the largest limit
    bad = small._replace(octave=np.concatenate([small.octave[:-1], [NLEVELS]]).astype(np.int32))
    lr = level_ratio().copy()
    lr[3] = lr[1]
    for kw in (dict(pairs=[dev_pair(bad)]), dict(pairs=[dev_pair(small)], level_ratio=lr), dict(pairs=[dev_pair(small)], project_form=2)):
        with pytest.raises(capi.PliError) as e:
            fe.search_by_projection_sim3(pts, descs, cam=CAM, **kw)
        assert e.value.status == -1
    # empty sides: no points, an empty keyframe inside a batch, nothing but empty keyframes, no pairs
    rows, bi, nm = check(fe, pts[:0], descs[:0], [small, empty])
    assert bi.shape == (2, 0) and (rows[0] == -1).all() and len(rows[1]) == 0 and (nm == 0).all()
    rows, bi, nm = check(fe, pts, descs, [empty, small, empty], 8.0, 1.5)
    assert (bi[0] == -1).all() and nm[0] == 0 and nm[2] == 0
    check(fe, pts, descs, [empty, empty])
    rows, bi, nm = fe.search_by_projection_sim3(pts, descs, [], CAM)
    assert rows == [] and bi.shape == (0, len(pts)) and nm.shape == (0,)
    # raw calls: kf_off decreasing, null pointers
    import ctypes as C
    L, h, ptr = fe.L, fe.h, capi.ptr
    kp, kd = keypoints(small), np.ascontiguousarray(small.desc)
    pose = np.stack([IDENTITY, IDENTITY])
    camc = capi.FuseCamera(*[float(v) for v in CAM])
    out, nmo, lvr = np.zeros(50, np.int32), np.zeros(2, np.int32), level_ratio()

    def raw(off, mp=pts, md=descs, kkp=kp, po=pose, cam=camc, lv=lvr, rp=out, nm=nmo):
        off = np.array(off, np.int32)
        return L.pli_search_by_projection_sim3(h, ptr(mp), ptr(md), len(pts), 2, ptr(off), ptr(kkp), ptr(kd), ptr(po), None, None,
                                               C.byref(cam) if cam is not None else None, 3.0, ptr(lv), 1.0, 0, ptr(rp), None, ptr(nm))
    assert raw([0, 20, 50]) == 0
    assert raw([0, 30, 20]) == -1 and raw([1, 20, 50]) == -1
    for kw in (dict(mp=None), dict(md=None), dict(kkp=None), dict(po=None), dict(cam=None), dict(lv=None), dict(rp=None), dict(nm=None)):
        assert raw([0, 20, 50], **kw) == -1, kw
