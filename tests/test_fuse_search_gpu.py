"""pli_fuse_search on the MI355X (the product library): the search half of ORBmatcher::Fuse (ORBmatcher.cc:1399-1609 without second
cameras, and the Sim3 overload :1611-1733) for a list of map points against a batch of keyframes equals the Python restatements of
tests/test_fuse_search_cpu.py exactly (best_idx and best_dist).  That file shows, on the CPU, that the constructed scenes take
every exit of the reference's loop and produce matches, so the equalities here are not vacuous."""
import numpy as np
import pytest

from pli_slam_amd import capi, realdata, synth
from test_fuse_search_cpu import (CAM, FUSE_POINT_DT, IDENTITY, KF, NLEVELS, SF, fuse_case, fuse_search_batch, fuse_search_fast,
                                  fuse_search_scalar, level_ratio, make_keyframe, make_points, make_pose, rot_xyz)

pytestmark = pytest.mark.gpu
W, H = 752, 480


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(W, H), dev=False)
    assert np.array_equal(f.cfg.orb_nlevels, NLEVELS)
    yield f
    f.close()


def keypoints(kf):
    kp = np.zeros(len(kf.x), capi.KEYPOINT_DT)
    kp["x"], kp["y"], kp["octave"] = kf.x, kf.y, kf.octave
    kp["size"] = 31.0
    return kp


def dev_kf(kf):
    return keypoints(kf), kf.desc, kf.uright, kf.pose


def check(fe, pts, descs, kfs, th=3.0, gate=True, skip=None, scalar=False, cam=CAM):
    bi, bd = fe.fuse_search(pts, descs, [dev_kf(k) for k in kfs], cam, th, gate, skip, level_ratio=level_ratio())
    assert bi.shape == (len(kfs), len(pts)) and bd.shape == bi.shape
    wi, wd = fuse_search_batch(pts, descs, kfs, cam, th, gate, skip, fuse_search_scalar if scalar else fuse_search_fast)
    assert np.array_equal(bi, wi), "%d of %d best_idx differ" % (int((bi != wi).sum()), bi.size)
    assert np.array_equal(bd, wd), "%d of %d best_dist differ" % (int((bd != wd).sum()), bd.size)
    return bi, bd


@pytest.mark.parametrize("nkf", [0, 1, 10, 30])
def test_constructed_scenes(fe, nkf):
    """500 points from a reference view (normals, distance ranges, points behind / beside / too near / too far, grazing normals)
    against nkf target poses around it with ~400 features each (noisy projections, twins, decoys, mono and stereo rows)."""
    rng = np.random.default_rng(200 + nkf)
    pts, descs, kfs, skip = fuse_case(rng, nkf, 500)
    total = 0
    for gate, th, sk in ((True, 3.0, None), (True, 4.0, skip), (False, 3.0, skip), (False, 4.0, None)):
        bi, _ = check(fe, pts, descs, kfs, th, gate, sk)
        total += int((bi >= 0).sum())
    print("nkf %d: %d matches over the four settings" % (nkf, total))
    if nkf:
        check(fe, pts, descs, kfs[:2], 3.0, True, skip[:2], scalar=True)      # the reference's control flow on two keyframes
        assert total > 100 * nkf
    else:
        assert total == 0


def test_one_keyframe_twenty_thousand_points(fe):
    """The shape of LocalMapping.cc:776: every neighbour's map points against the current keyframe."""
    rng = np.random.default_rng(77)
    pts, descs = make_points(rng, 20000)
    kf = make_keyframe(rng, pts, descs, make_pose(rot_xyz(0.01, -0.02, 0.03), [0.2, -0.1, 0.3]), 1200)
    skip = (rng.random((1, len(pts))) < 0.1).astype(np.uint8)
    bi, _ = check(fe, pts, descs, [kf], 3.0, True, skip)
    # the restatement yields 277 matches for this seed; floor = half of it
    assert (bi >= 0).sum() > 138
    check(fe, pts, descs, [kf], 4.0, False, None)


def test_crowded_windows_and_ties(fe):
    """More candidates in a window than a lane group holds (every keypoint within a few pixels of a few spots), and all
    descriptors equal, so that the visiting order decides every winner."""
    rng = np.random.default_rng(8)
    pts, descs = make_points(rng, 300)
    pose = make_pose(rot_xyz(0.01, 0.01, -0.01), [0.1, 0.05, -0.1])
    kf = make_keyframe(rng, pts, descs, pose, 300, noise=0.3)
    # 40 copies of every keypoint within +-2.5 px: windows of 100+ candidates that straddle cell borders
    rep = 40
    x = (np.repeat(kf.x, rep) + rng.uniform(-2.5, 2.5, len(kf.x) * rep)).astype(np.float32)
    y = (np.repeat(kf.y, rep) + rng.uniform(-2.5, 2.5, len(kf.x) * rep)).astype(np.float32)
    octave, uright = np.repeat(kf.octave, rep), np.repeat(kf.uright, rep)
    d = np.repeat(kf.desc, rep, axis=0)
    crowded = KF(x[:8000], y[:8000], octave[:8000], d[:8000], uright[:8000], pose)
    for gate, th in ((True, 3.0), (False, 4.0)):
        bi, _ = check(fe, pts, descs, [crowded, kf], th, gate)
        assert (bi >= 0).sum() > 50
    same = crowded._replace(desc=np.zeros_like(crowded.desc))
    bi, bd = check(fe, pts, np.zeros_like(descs), [same, kf._replace(desc=np.zeros_like(kf.desc))], 4.0, False)
    assert (bi >= 0).sum() > 50 and (bd[bi >= 0] == 0).all()
    check(fe, pts[:60], np.zeros_like(descs[:60]), [same], 3.0, True, scalar=True)


# ---- tables of the device's own extractor ------------------------------------------------------------------------------------

def stereo_frame(fe, L, R):
    rec = fe.batch_run_host(np.stack([L, R])[None])[0]
    return rec


def table_kf(kp, desc, uright, pose):
    return KF(kp["x"].astype(np.float32), kp["y"].astype(np.float32), kp["octave"].astype(np.int32), desc.copy(),
              np.asarray(uright, np.float32).copy(), pose)


def unproject(rec, cam):
    """Map points from a frame's stereo keypoints (Frame::UnprojectStereo with the frame at the origin): the normal is the viewing
    ray, the distance range the one MapPoint::UpdateNormalAndDepth gives a point observed at that octave."""
    kp, z = rec["kpL"], rec["depth"].astype(np.float64)
    sel = np.nonzero(z > 0)[0]
    pts = np.zeros(len(sel), FUSE_POINT_DT)
    pos = np.stack([(kp["x"][sel] - float(cam.cx)) * z[sel] / float(cam.fx), (kp["y"][sel] - float(cam.cy)) * z[sel] / float(cam.fy),
                    z[sel]], 1)
    dist = np.linalg.norm(pos, axis=1)
    max_d = (dist * SF[kp["octave"][sel]]).astype(np.float32)
    pts["pos"], pts["normal"] = pos.astype(np.float32), (pos / dist[:, None]).astype(np.float32)
    pts["max_dist"] = max_d
    pts["min_dist_inv"] = np.float32(0.8) * (max_d / SF[-1]).astype(np.float32)
    pts["max_dist_inv"] = np.float32(1.2) * max_d
    pts["valid"] = 1
    return pts, rec["descL"][sel].copy()


def real_case(fe, frames, cam):
    """Points of frame 0; targets: its right image (a mono keyframe one baseline to the right), the next frame (stereo rows, a
    small motion) and frame 0 itself."""
    rec0, rec1 = stereo_frame(fe, *frames[0]), stereo_frame(fe, *frames[1])
    pts, descs = unproject(rec0, cam)
    base = float(cam.bf) / float(cam.fx)
    kfs = [table_kf(rec0["kpR"], rec0["descR"], np.full(len(rec0["kpR"]), -1.0), make_pose(np.eye(3), [-base, 0, 0])),
           table_kf(rec1["kpL"], rec1["descL"], rec1["uright"], make_pose(rot_xyz(0.001, -0.002, 0.004), [0.02, 0.01, -0.05])),
           table_kf(rec0["kpL"], rec0["descL"], rec0["uright"], IDENTITY)]
    return pts, descs, kfs


def test_real_orb_tables_synthetic_scenes(fe):
    cam = CAM._replace(fx=np.float32(fe.cfg.fx), fy=np.float32(fe.cfg.fx), bf=np.float32(fe.cfg.bf))
    total = 0
    for s in (3, 11):
        pts, descs, kfs = real_case(fe, [synth.make_stereo_pair(s, W, H, t=0), synth.make_stereo_pair(s, W, H, t=1)], cam)
        for gate, th in ((True, 3.0), (True, 4.0), (False, 3.0)):
            total += int((check(fe, pts, descs, kfs, th, gate, cam=cam)[0] >= 0).sum())
    print("synthetic scenes: %d matches" % total)
    # the restatement yields 6133 matches for these seeds (the tables come from the device's extractor); floor = half of it
    assert total > 3066, total


def test_real_photographs(fe):
    cam = CAM._replace(fx=np.float32(fe.cfg.fx), fy=np.float32(fe.cfg.fx), bf=np.float32(fe.cfg.bf))
    frames = realdata.frames_752x480(3, seed=4)
    total = 0
    for a, b in ((0, 1), (2, 1)):
        pts, descs, kfs = real_case(fe, [frames[a], frames[b]], cam)
        for gate, th in ((True, 3.0), (False, 4.0)):
            total += int((check(fe, pts, descs, kfs, th, gate, cam=cam)[0] >= 0).sum())
    print("photographs: %d matches" % total)
    # the restatement yields 4584 matches for these seeds; floor = half of it
    assert total > 2292, total



# ---- the call itself -----------------------------------------------------------------------------------------------------------

def test_a_batch_equals_single_calls_and_calls_repeat(fe):
    rng = np.random.default_rng(9)
    pts, descs, kfs, skip = fuse_case(rng, 7, 400)
    dk = [dev_kf(k) for k in kfs]
    for gate, th, sk in ((True, 3.0, skip), (False, 4.0, None)):
        bi, bd = fe.fuse_search(pts, descs, dk, CAM, th, gate, sk, level_ratio=level_ratio())
        for k in range(len(kfs)):
            i1, d1 = fe.fuse_search(pts, descs, dk[k:k + 1], CAM, th, gate, None if sk is None else sk[k:k + 1], level_ratio=level_ratio())
            assert np.array_equal(i1[0], bi[k]) and np.array_equal(d1[0], bd[k])
        for _ in range(3):
            i2, d2 = fe.fuse_search(pts, descs, dk, CAM, th, gate, sk, level_ratio=level_ratio())
            assert np.array_equal(i2, bi) and np.array_equal(d2, bd)
        assert (bi >= 0).sum() > 0
    # the binding's own table (math.log on the float) is this host's expression too
    i3, _ = fe.fuse_search(pts, descs, dk, CAM, 4.0, False)
    assert np.array_equal(i3, bi)


def test_keyframes_of_different_sizes_and_empty_ones(fe):
    rng = np.random.default_rng(10)
    pts, descs, kfs, _ = fuse_case(rng, 3, 300)
    cut = lambda kf, n: KF(kf.x[:n], kf.y[:n], kf.octave[:n], kf.desc[:n], kf.uright[:n], kf.pose)
    mixed = [cut(kfs[0], 0), kfs[0], cut(kfs[1], 37), cut(kfs[2], 0), cut(kfs[2], 1), cut(kfs[1], 0)]
    bi, bd = check(fe, pts, descs, mixed)
    assert (bi[0] == -1).all() and (bd[3] == 256).all() and (bi[1] >= 0).sum() > 0
    check(fe, pts, descs, [cut(kfs[0], 0)] * 2)                      # nothing but empty keyframes
    bi, bd = check(fe, pts[:0], descs[:0], mixed)                    # no points
    assert bi.shape == (6, 0)
    bi, bd = fe.fuse_search(pts, descs, [], CAM)                     # no keyframes
    assert bi.shape == (0, len(pts))


def test_capacity_and_arguments(fe):
    rng = np.random.default_rng(3)
    cap = 8192                                            # PLI_BOW_MAX_FEATURES
    pts, descs = make_points(rng, 200)

    def table(n):
        return KF(rng.uniform(0, W, n).astype(np.float32), rng.uniform(0, H, n).astype(np.float32),
                  rng.integers(0, NLEVELS, n).astype(np.int32), rng.integers(0, 256, (n, 32), dtype=np.uint8),
                  rng.choice([-1.0, 300.0], n).astype(np.float32), IDENTITY)
    small, big, full = table(50), table(cap + 1), table(cap)
    with pytest.raises(capi.PliError) as e:
        fe.fuse_search(pts, descs, [dev_kf(small), dev_kf(big)], CAM)
    assert e.value.status == -3                     # PLI_ERR_CAPACITY
    check(fe, pts, descs, [full, small], 4.0, False)     # exactly at the cap
    invalid = []
    for value in (NLEVELS, -1):                          # an octave outside the context's levels
        invalid.append(dict(keyframes=[dev_kf(small._replace(octave=np.concatenate([small.octave[:-1], [value]]).astype(np.int32)))]))
    lr = level_ratio().copy()
    lr[3] = lr[1]
    invalid.append(dict(keyframes=[dev_kf(small)], level_ratio=lr))                      # level_ratio decreasing
    lr = level_ratio().copy()
    lr[2] = np.nan
    invalid.append(dict(keyframes=[dev_kf(small)], level_ratio=lr))
    for kw in invalid:
        with pytest.raises(capi.PliError) as e:
            fe.fuse_search(pts, descs, cam=CAM, **kw)
        assert e.value.status == -1                 # PLI_ERR_INVALID
    # raw calls: kf_off decreasing, null pointers
    L, h, ptr = fe.L, fe.h, capi.ptr
    import ctypes as C
    kp, kd, ku = keypoints(small), np.ascontiguousarray(small.desc), small.uright
    pose = np.stack([IDENTITY, IDENTITY])
    camc = capi.FuseCamera(*[float(v) for v in CAM])
    out = np.zeros((2, len(pts)), np.int32)
    lr = level_ratio()

    def raw(off, mp=pts, md=descs, kkp=kp, po=pose, cam=camc, lvr=lr, bi=out):
        off = np.array(off, np.int32)
        return L.pli_fuse_search(h, ptr(mp), ptr(md), len(pts), 2, ptr(off), ptr(kkp), ptr(kd), ptr(ku), ptr(po), None,
                                 C.byref(cam) if cam is not None else None, 3.0, ptr(lvr), 1, ptr(bi), None)
    assert raw([0, 20, 50]) == 0
    assert raw([0, 30, 20]) == -1 and raw([1, 20, 50]) == -1
    for kw in (dict(mp=None), dict(md=None), dict(kkp=None), dict(po=None), dict(cam=None), dict(lvr=None), dict(bi=None)):
        assert raw([0, 20, 50], **kw) == -1, kw
